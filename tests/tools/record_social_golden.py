"""Record tests/golden/social_group.npz from the reference's own SocialGroupLoss (src/tbsim/utils/guidance_loss.py:1137-1207) through
DiffuserGuidance.compute_guidance_loss (:2143-2173) + autograd, on the CPU.

    python tests/tools/record_social_golden.py          (needs the reference tree, see oracle/_refimport.py)

One scene of A = 8 agents (synth.make_collision_scene), N = 2 plans each (synth.make_collision_trajectories), a group of 6 on an
`agents` subset.  Cases: cohesion 0, 0.6 and 1 with a member as leader, and one whose leader_idx names no member (nobody detached).
The class draws on the CPU, torch.randint(0, M - 1, (T N, M, 1)) and then torch.rand((T N, M)): the same two calls after the same
torch.manual_seed replay its draws, which are stored rearranged to plan rows [A N, 52] (row = agent * N + sample; 0 outside the
group).  Every case stores the per-agent values [A,N] (NaN outside the config's agents), d total / d plans [A,N,52,6] and the draws;
`meta` holds the configs and, per case, the error of the reference's own float32 result against the float64 yardstick.  The seed of
a case is moved on until the yardstick's margins hold (nearest neighbour ahead of the second by 1e-3 m, no distance below 1e-2 m,
no u within 1e-6 of cohesion)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from cld_amd import synth                      # noqa: E402
from oracle import _refimport                  # noqa: E402
from tests import social_yardstick as Y        # noqa: E402

A, N, SEED, T = 8, 2, 43, 52
SUB = [0, 1, 3, 4, 6, 7]
CASES = {"coh0": dict(cohesion=0.0, leader_idx=3), "coh06": dict(cohesion=0.6, leader_idx=3), "coh1": dict(cohesion=1.0, leader_idx=4),
         "noleader": dict(cohesion=0.6, leader_idx=2)}


def replay(seed, M):
    """The class's draws after torch.manual_seed(seed) -> (r, u) in plan rows [A N, 52]; flat index of the class = t * N + n."""
    torch.manual_seed(seed)
    r = torch.randint(0, M - 1, (T * N, M, 1))[:, :, 0].reshape(T, N, M)
    u = torch.rand((T * N, M)).reshape(T, N, M)
    R, U = torch.zeros(A, N, T, dtype=torch.int32), torch.zeros(A, N, T)
    R[SUB] = r.permute(2, 1, 0).to(torch.int32)
    U[SUB] = u.permute(2, 1, 0)
    return R, U


def main():
    _refimport.install()
    with _refimport.redirect_stdout(_refimport.io.StringIO()):
        import tbsim.utils.guidance_loss as gl
    sc = synth.make_collision_scene([A], SEED)
    plans = torch.from_numpy(synth.make_collision_trajectories(A, N, sc["curr_speed"], SEED))
    Wf = torch.from_numpy(sc["world_from_agent"])
    db = {"world_from_agent": Wf, "scene_index": torch.zeros(A, dtype=torch.long)}
    out, meta_cases = {}, {}
    for name, c in CASES.items():
        case = dict(c, agents=SUB, weight=2.0, social_dist=1.5)
        term = Y.term_from_meta(case, Wf, N)
        seed = 100
        while True:                                                     # a seed whose draws keep the margins (cohesion 0 reads none: first seed)
            R, U = replay(seed, len(SUB))
            gap, dmin, umin = Y.margins(plans.double(), term, R, U)
            if gap >= 1e-3 and dmin >= 1e-2 and umin >= 1e-6:
                break
            seed += 1
        g = gl.DiffuserGuidance([[{"name": "social_group", "weight": case["weight"], "agents": SUB,
                                   "params": {"leader_idx": case["leader_idx"], "social_dist": case["social_dist"], "cohesion": case["cohesion"]}}]])
        x = plans.clone().requires_grad_(True)
        torch.manual_seed(seed)
        tot, per = g.compute_guidance_loss(x * 1.0, db)
        tot.backward()
        ref_v, ref_g = per["social_group_scene_000_00"], x.grad.clone()
        v, grad = Y.value_and_grad(plans.double(), term, R, U)
        err_v = float((v[SUB] - ref_v[SUB].double()).abs().max())
        err_g = float((grad - ref_g.double()).abs().max())
        outside = [a for a in range(A) if a not in SUB]
        quiet = outside + ([case["leader_idx"]] if case["leader_idx"] in SUB else [])
        assert bool(torch.isnan(ref_v[outside]).all()) and float(ref_g[quiet].abs().max()) == 0.0
        print(f"{name}: seed {seed}; margins: neighbour {gap:.3e} m, distance {dmin:.3e} m, u {umin:.3e}; reference fp32 against the fp64 yardstick: "
              f"values {err_v:.2e} of max {float(v.abs().max()):.3f}, gradient {err_g:.2e} of max {float(grad.abs().max()):.3e}")
        out[name + "_values"], out[name + "_grad"], out[name + "_total"] = ref_v, ref_g, tot.detach().reshape(1)
        out[name + "_draw_r"], out[name + "_draw_u"] = R.reshape(A * N, T), U.reshape(A * N, T)
        meta_cases[name] = dict(case, seed=seed, ref_value_err=err_v, ref_grad_err=err_g, max_value=float(v.abs().max()), max_grad=float(grad.abs().max()))
    out["world_from_agent"] = Wf
    meta = dict(A=A, N=N, seed=SEED, scene="synth.make_collision_scene([A], seed)", plans="synth.make_collision_trajectories(A, N, curr_speed, seed)",
                cases=meta_cases, torch=torch.__version__, generator="tests/tools/record_social_golden.py",
                source="the reference's SocialGroupLoss through DiffuserGuidance.compute_guidance_loss + autograd")
    arrays = {k: np.ascontiguousarray(v.detach().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    path = os.path.join(ROOT, "tests", "golden", "social_group.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f"social_group: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
