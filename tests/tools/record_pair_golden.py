"""Record tests/golden/pair_guidance.npz from the reference's own pair-relation losses (src/tbsim/utils/guidance_loss.py:
KeepDistanceLoss :1631-1688, CollisionLoss :1691-1734, KeepDistanceLoss2 :1739-1791, FrontCollisionLoss :1844-1896,
CollideLeftSideLoss :1899-1956, StayAwayLoss :2014-2082) + autograd, on the CPU.

    python tests/tools/record_pair_golden.py          (needs the reference tree, see oracle/_refimport.py)

One scene of A = 6 agents (synth.make_collision_scene), N = 2 plans each (synth.make_collision_trajectories), `agents: None`,
agent_from_world = the float64 inverse of world_from_agent (rounded to float32, as the class reads it).  Cases:
  keepdistance, collision   the two registered names through DiffuserGuidance.compute_guidance_loss (:2143-2173)
  stayaway, keepdistance2, front, left   the four other classes called directly with a full mask; total = weight * mean
  two                       two configs in the scene through DiffuserGuidance; one agent is ref of the first and target of the second
The inputs are stored (plans [A,N,52,6], both frame arrays).  Every case stores the per-agent values [A,N] of each of its configs
(the class's [N] under every agent of the scene), the total [1] and d total / d plans [A,N,52,6]; `meta` holds per case its pairs (target, ref, kind, lo, hi, decay, weight) and the error of the
reference's own float32 result against the float64 yardstick.
The distance bounds of a case are quantiles of the distances the yardstick reads on these plans (so that the clip branches named in
WANT are active at some step, or at none of a whole sample), moved on in steps of 0.137 m until the yardstick's margins hold: no
distance below 1e-2 m, no |d - bound|, |Dx| or |Dy| within 1e-3 of its kink.  For the frame relations the pair is moved on instead."""
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from cld_amd import synth                      # noqa: E402
from oracle import _refimport                  # noqa: E402
from tests import pair_yardstick as Y          # noqa: E402

A, N, SEED, T = 6, 2, 47, 52
# case -> [(class / config name, yardstick kind, upstream's names of (target, ref, lo, hi, decay), (target, ref), quantiles of (lo, hi), decay, weight)]
SPEC = {
    "keepdistance": [("gptkeepdistance", "keep_distance", ("target_ind", "ref_ind", "min_distance", "max_distance", None), (0, 4), (0.3, 0.7), 0.0, 2.0)],
    "collision": [("gptcollision", "collision", ("target_ind", "ref_ind", "collision_radius", None, None), (5, 1), (0.4, None), 0.0, 1.5)],
    "stayaway": [("StayAwayLoss", "stay_away", ("target_ind", "ref_ind", "min_dist", "max_dist", "decay_rate"), (2, 3), (0.25, 0.6), 0.9, 3.0)],
    "keepdistance2": [("KeepDistanceLoss2", "stay_away", ("target_ind", "ref_ind", "min_dist", "max_dist", "decay_rate"), (1, 5), (-1.0, 0.5), 0.8, 1.0)],
    "front": [("FrontCollisionLoss", "front_collision", ("target_ind", "ref_ind", None, None, None), (0, 2), (None, None), 0.0, 2.5)],
    "left": [("CollideLeftSideLoss", "collide_left", ("target_ind", "ref_ind", None, None, None), (4, 1), (None, None), 0.0, 0.5)],
    "two": [("gptcollision", "collision", ("target_ind", "ref_ind", "collision_radius", None, None), (1, 3), (0.5, None), 0.0, 2.0),
            ("gptkeepdistance", "keep_distance", ("target_ind", "ref_ind", "min_distance", "max_distance", None), (3, 4), (0.35, 0.65), 0.0, 1.0)],
}
# what the recording has to hold: (case, config, branch) active at some step of some sample / at no step of some whole sample
WANT_ACTIVE = [("keepdistance", 0, "below_min"), ("keepdistance", 0, "above_max"), ("collision", 0, "above"), ("stayaway", 0, "below_min"),
               ("stayaway", 0, "above_max"), ("front", 0, "y"), ("left", 0, "y")]
WANT_IDLE = [("keepdistance2", 0, "below_min")]


def settle(plans, frames, spec):
    """One config's pair dict with bounds / pair moved on until the margins hold."""
    name, kind, _, (ti, ri), (q_lo, q_hi), decay, weight = spec
    W, F = frames
    base = dict(kind=[kind], decay=[decay], scale=[weight / N], world_from_agent=W, agent_from_world=F)
    if kind in ("front_collision", "collide_left"):
        order = [(ti, ri)] + [c for c in itertools.permutations(range(A), 2) if c != (ti, ri)]
        for i, j in order:
            term = dict(base, target=[i], ref=[j], lo=[0.0], hi=[0.0])
            if Y.margins(plans, term)[1] >= 1e-3:
                return dict(target=i, ref=j, kind=kind, lo=0.0, hi=0.0, decay=decay, weight=weight)
        raise RuntimeError(f"{name}: no pair keeps the margins")
    d = Y._pair(plans, dict(base, target=[ti], ref=[ri], lo=[0.0], hi=[0.0]), 0)[2].reshape(-1)
    quant = lambda q: 0.0 if q is None else (0.5 if q < 0 else round(float(torch.quantile(d, q)), 1))
    lo, hi = quant(q_lo), quant(q_hi)
    for k in range(50):
        cand = dict(base, target=[ti], ref=[ri], lo=[lo + 0.137 * k], hi=[hi + 0.137 * k if q_hi is not None else 0.0])
        if kind == "collision":
            cand["hi"] = [0.0]
        dmin, kink = Y.margins(plans, cand)
        if dmin >= 1e-2 and kink >= 1e-3:
            return dict(target=ti, ref=ri, kind=kind, lo=cand["lo"][0], hi=cand["hi"][0], decay=decay, weight=weight)
    raise RuntimeError(f"{name}: no bounds keep the margins")


def main():
    _refimport.install()
    with _refimport.redirect_stdout(_refimport.io.StringIO()):
        import tbsim.utils.guidance_loss as gl
    sc = synth.make_collision_scene([A], SEED)
    plans = torch.from_numpy(synth.make_collision_trajectories(A, N, sc["curr_speed"], SEED))
    Wf = torch.from_numpy(sc["world_from_agent"])
    Ff = Y.invert_frames(Wf.double()).float()
    db = {"world_from_agent": Wf, "agent_from_world": Ff, "scene_index": torch.zeros(A, dtype=torch.long)}
    frames = (Wf.double(), Ff.double())
    out, meta_cases = {}, {}
    for name, specs in SPEC.items():
        pairs = [settle(plans.double(), frames, s) for s in specs]
        case = dict(pairs=pairs, configs=[s[0] for s in specs])
        term = Y.term_from_meta(case, Wf, Ff, N)
        dmin, kink = Y.margins(plans.double(), term)
        assert dmin >= 1e-2 and kink >= 1e-3, (name, dmin, kink)
        params = []
        for s, q in zip(specs, pairs):
            keys = s[2]
            prm = {keys[0]: q["target"], keys[1]: q["ref"]}
            for key, v in zip(keys[2:], (q["lo"], q["hi"], q["decay"])):
                if key is not None:
                    prm[key] = v
            params.append(prm)
        x = plans.clone().requires_grad_(True)
        if all(s[0].startswith("gpt") for s in specs):                  # the registered names, through DiffuserGuidance
            g = gl.DiffuserGuidance([[{"name": s[0], "weight": q["weight"], "agents": None, "params": prm} for s, q, prm in zip(specs, pairs, params)]])
            tot, per = g.compute_guidance_loss(x * 1.0, db)
            vals = [per["%s_scene_000_%02d" % (s[0], gi)] for gi, s in enumerate(specs)]
        else:                                                           # the class itself, full mask; total as DiffuserGuidance forms it
            (s,), (q,), (prm,) = specs, pairs, params
            v = getattr(gl, s[0])(**prm)(x * 1.0, db, agt_mask=torch.ones(A, dtype=torch.bool))
            tot = torch.mean(v) * q["weight"]
            vals = [v.detach()[None, :].expand(A, N).clone()]
        tot.backward()
        ref_g = x.grad.clone()
        yv, yg = Y.value_and_grad(plans.double(), term)
        err_v = max(float((yv[k][None, :] - vals[k].double()).abs().max()) for k in range(len(specs)))
        err_g = float((yg - ref_g.double()).abs().max())
        br = [{k: [a.tolist(), b.tolist()] for k, (a, b) in Y.branches(plans.double(), term, k).items()} for k in range(len(specs))]
        print(f"{name}: {pairs}\n   margins: distance {dmin:.3e} m, kink {kink:.3e}; branches (any, all per sample) {br}; reference fp32 against the "
              f"fp64 yardstick: values {err_v:.2e} of max {float(yv.abs().max()):.3f}, gradient {err_g:.2e} of max {float(yg.abs().max()):.3e}")
        for k in range(len(specs)):
            out[f"{name}_values_{k}"] = vals[k]
        out[name + "_grad"], out[name + "_total"] = ref_g, tot.detach().reshape(1)
        meta_cases[name] = dict(case, branches=br, ref_value_err=err_v, ref_grad_err=err_g, max_value=float(yv.abs().max()), max_grad=float(yg.abs().max()))
    for c, k, b in WANT_ACTIVE:
        assert any(meta_cases[c]["branches"][k][b][0]), (c, k, b, "never active")
    for c, k, b in WANT_IDLE:
        assert not all(meta_cases[c]["branches"][k][b][0]), (c, k, b, "active in every sample")
    out["world_from_agent"], out["agent_from_world"], out["plans"] = Wf, Ff, plans
    meta = dict(A=A, N=N, seed=SEED, scene="synth.make_collision_scene([A], seed)", plans="synth.make_collision_trajectories(A, N, curr_speed, seed)",
                cases=meta_cases, torch=torch.__version__, generator="tests/tools/record_pair_golden.py",
                source="the reference's pair-relation loss classes (through DiffuserGuidance.compute_guidance_loss where registered) + autograd")
    arrays = {k: np.ascontiguousarray(v.detach().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    path = os.path.join(ROOT, "tests", "golden", "pair_guidance.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f"pair_guidance: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
