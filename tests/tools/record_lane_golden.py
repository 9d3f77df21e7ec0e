"""Record tests/golden/lane_guidance.npz from the reference's own lane projection and lane losses (src/tbsim/utils/trajdata_utils.py
project_onto :726-821; src/tbsim/utils/guidance_loss.py LaneFollowingLoss :1574-1628, ChangeToLeftLaneLoss :1795-1841, FollowLaneLoss
:1958-2011) + autograd, on the CPU.

    python tests/tools/record_lane_golden.py          (needs the reference tree, see oracle/_refimport.py)

get_lane_projection itself needs trajdata's vector map, which is not there; guidance_loss.get_current_lane_projection and
get_left_lane_projection are therefore replaced by a function that does what its lines 655-662 do with a polyline already in the
agent frame: sort the stored agent-frame polyline by x, repeat it per sample, call the reference's own project_onto.  The classes run
unchanged on top of it.

One scene of A = 6 agents, N = 2 plans each, 52 steps.  Every agent has a current-lane and a left-lane polyline (3.5 m to its left)
of 20 to 48 points about 1 m apart with gentle curvature, given in the WORLD frame in float64 and taken into the agent frame by
tests/lane_yardstick.prepare's transform (this project's definition; not pinned by the reference).  Agent 0's rows are shorter
(NaN-padded), agent 2's polylines hold a duplicated point (the junction of a lane and its successor), agent 3's are stored with
the successor FIRST (not x-sorted).  Cases:
  following      LaneFollowingLoss(target_inds=[2])
  following3     LaneFollowingLoss(target_inds=[1, 2, 3])
  changeleft     ChangeToLeftLaneLoss(target_ind=4)
  followlane     FollowLaneLoss(target_ind=0, decay_rate=0.9)
  clip           FollowLaneLoss(target_ind=5, decay_rate=0.8): agent 5 drifts off its lane, the clip at 5 is active at some steps only
  two            LaneFollowingLoss(target_inds=[1, 3]) + FollowLaneLoss(target_ind=3): agent 3 carries two entries
total = sum over configs of weight * mean over samples, as DiffuserGuidance forms it.  The plans are settled first: every plan point
whose projection gap is below 1e-4 m or whose kink margin is below 1e-3 under ANY case is nudged (one at a time, by 37 mm
sideways and 3.7 mrad in yaw) until none is left.  Stored: the inputs (plans, world polylines, frames, the agent-frame polylines unsorted and sorted),
per case the projections [E,N,52,3], the per-config values [N], the total and d total / d plans; `meta` holds per case its entries,
the error of the reference's float32 results against the float64 yardstick, and the clip flags."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import _refimport                  # noqa: E402
from tests import lane_yardstick as Y          # noqa: E402

A, N, T, S, SEED = 6, 2, 52, 48, 53
GAP_MIN, KINK_MIN = 1e-4, 1e-3
# case -> [(class, kind, constructor arguments, weight)]
SPEC = {
    "following": [("LaneFollowingLoss", "following", {"target_inds": [2]}, 2.0)],
    "following3": [("LaneFollowingLoss", "following", {"target_inds": [1, 2, 3]}, 1.5)],
    "changeleft": [("ChangeToLeftLaneLoss", "change_left", {"target_ind": 4}, 3.0)],
    "followlane": [("FollowLaneLoss", "follow_decayed", {"target_ind": 0, "decay_rate": 0.9}, 40.0)],
    "clip": [("FollowLaneLoss", "follow_decayed", {"target_ind": 5, "decay_rate": 0.8}, 25.0)],
    "two": [("LaneFollowingLoss", "following", {"target_inds": [1, 3]}, 1.0), ("FollowLaneLoss", "follow_decayed", {"target_ind": 3, "decay_rate": 0.9}, 30.0)],
}


def make_scene(rng):
    """-> (world polylines [2,A,S,3] float64 (current, left), agent_from_world [A,3,3] float32)."""
    pos = np.stack([40.0 * np.arange(A) + 120.0, -80.0 + 7.0 * np.arange(A)], axis=1) + rng.uniform(-1, 1, (A, 2))
    th = rng.uniform(-0.6, 0.6, A)
    W = np.zeros((A, 3, 3))
    W[:, 0, 0], W[:, 0, 1], W[:, 1, 0], W[:, 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    W[:, :2, 2], W[:, 2, 2] = pos, 1.0
    F = np.linalg.inv(W).astype(np.float32)
    lines = np.full((2, A, S, 3), np.nan)
    for a in range(A):
        n = 20 if a == 0 else int(rng.integers(36, S - 1))
        curv, y0, slope = rng.uniform(-0.004, 0.004), rng.uniform(-0.6, 0.6), rng.uniform(-0.05, 0.05)
        x = -4.0 + np.cumsum(rng.uniform(0.9, 1.1, n)) * (2.2 if a == 0 else 1.0)      # (agent 0: fewer, longer segments)
        for side in range(2):
            y = y0 + slope * x + curv * x * x + 3.5 * side
            h = np.arctan(slope + 2 * curv * x)
            loc = np.stack([x, y, h], axis=1)
            if a == 2:                                                    # a duplicated point: the junction of a lane and its successor
                k = n // 2
                loc = np.concatenate([loc[:k + 1], loc[k:]], axis=0)
            if a == 3:                                                    # the successor stored first: not x-sorted
                k = n // 3
                loc = np.concatenate([loc[k:], loc[:k]], axis=0)
            c, s = np.cos(loc[:, 2]), np.sin(loc[:, 2])
            wx = W[a, 0, 0] * loc[:, 0] + W[a, 0, 1] * loc[:, 1] + W[a, 0, 2]
            wy = W[a, 1, 0] * loc[:, 0] + W[a, 1, 1] * loc[:, 1] + W[a, 1, 2]
            wh = np.arctan2(W[a, 1, 0] * c + W[a, 1, 1] * s, W[a, 0, 0] * c + W[a, 0, 1] * s)
            lines[side, a, :loc.shape[0]] = np.stack([wx, wy, wh], axis=1)
    return lines, F


def make_plans(rng):
    plans = np.zeros((A, N, T, 6), np.float32)
    speed = rng.uniform(3.0, 7.5, (A, N, 1))
    t = np.arange(T) + 1
    plans[..., 0] = speed * 0.1 * t + 0.05 * rng.standard_normal((A, N, T))
    drift = rng.uniform(-0.03, 0.03, (A, N, 1))
    drift[5] = np.array([[0.16], [-0.19]])                               # agent 5 leaves its lane: |dx| + |dy| passes 5 on the way
    plans[..., 1] = rng.uniform(-1.0, 1.0, (A, N, 1)) + drift * t + 0.05 * rng.standard_normal((A, N, T))
    plans[..., 3] = 0.1 * rng.standard_normal((A, N, T))
    plans[..., 2] = speed
    plans[..., 4:] = 0.1 * rng.standard_normal((A, N, T, 2))
    return torch.from_numpy(plans)


def entries_of(specs):
    out = []
    for k, (cls, kind, prm, weight) in enumerate(specs):
        tg = prm.get("target_inds", [prm.get("target_ind")])
        for a in tg:
            out.append(dict(agent=int(a), line=int(a) + (A if kind == "change_left" else 0), kind=kind, decay=float(prm.get("decay_rate", 0.0)),
                            weight=float(weight), targets=len(tg), config=k))
    order = sorted(range(len(out)), key=lambda e: out[e]["agent"])      # an agent's entries contiguous (stable), as the kernel wants them
    return [out[e] for e in order]


def main():
    _refimport.install()
    with _refimport.redirect_stdout(_refimport.io.StringIO()):
        import tbsim.utils.guidance_loss as gl
        import tbsim.utils.trajdata_utils as tu
    rng = np.random.default_rng(SEED)
    world, F = make_scene(rng)
    frames = np.concatenate([np.arange(A), np.arange(A)])
    wl = world.reshape(2 * A, S, 3)
    unsorted = Y.transform(wl, frames, F)
    lines = Y.sort_by_x(unsorted)
    assert np.array_equal(np.sort(unsorted[..., 0], axis=1), lines[..., 0], equal_nan=True)
    assert not np.array_equal(unsorted[3], lines[3], equal_nan=True) and np.array_equal(unsorted[1], lines[1], equal_nan=True)
    stored = torch.from_numpy(unsorted)

    def routed(side):
        def fn(pos_pred, yaw_pred, data_batch, visualize_projection=""):
            cur = stored[side * A:(side + 1) * A].to(pos_pred.dtype)
            cur = torch.gather(cur, 1, torch.argsort(cur[:, :, 0], dim=1, stable=True).unsqueeze(-1).expand(-1, -1, 3))
            cur = cur.unsqueeze(1).repeat(1, pos_pred.shape[1], 1, 1)
            return tu.project_onto(torch.cat([pos_pred.detach(), yaw_pred.detach()], dim=-1), cur, "")
        return fn
    gl.get_current_lane_projection, gl.get_left_lane_projection = routed(0), routed(1)

    plans = make_plans(rng)
    cases = {name: dict(entries=entries_of(specs), configs=[s[0] for s in specs]) for name, specs in SPEC.items()}
    terms = {name: Y.term_from_meta(c, lines, N) for name, c in cases.items()}
    every = dict(agent=[], line=[], kind=[], decay=[], scale=[], lines=torch.from_numpy(lines).double())
    for tm in terms.values():
        for k in ("agent", "line", "kind", "decay", "scale"):
            every[k] += tm[k]
    moved = 0
    for _ in range(400):                                                  # settle: nudge offending plan points one at a time
        bad = Y.offenders(plans.double(), every, GAP_MIN, KINK_MIN)
        if not bad:
            break
        a, n, t = bad[0]
        plans[a, n, t, 1] += 0.037
        plans[a, n, t, 3] += 0.0037
        moved += 1
    else:
        raise RuntimeError("the plans do not settle")
    gap, kink = Y.margins(plans.double(), every)
    print(f"settled after {moved} nudges: gap {gap:.3e} m, kink margin {kink:.3e}")
    assert gap >= GAP_MIN and kink >= KINK_MIN
    db = {"scene_index": torch.zeros(A, dtype=torch.long)}
    out, meta_cases = {}, {}
    for name, specs in SPEC.items():
        term, case = terms[name], cases[name]
        x = plans.clone().requires_grad_(True)
        tot, vals = 0.0, []
        for cls, kind, prm, weight in specs:
            v = getattr(gl, cls)(**prm)(x * 1.0, db, agt_mask=torch.ones(A, dtype=torch.bool))
            assert v.shape == (N,)
            tot = tot + weight * torch.mean(v)
            vals.append(v.detach())
        tot.backward()
        ref_g = x.grad.clone()
        with torch.no_grad():                                             # the reference's own projection of the entries' agents
            proj = torch.stack([(routed(1) if q["kind"] == "change_left" else routed(0))(plans[..., :2], plans[..., 3:4], db)[q["agent"]] for q in case["entries"]])
        yv, yg = Y.value_and_grad(plans.double(), term)
        yp, ygap = Y.projections(plans.double(), term)
        per_cfg = [yv[[e for e, q in enumerate(case["entries"]) if q["config"] == k]].mean(dim=0) for k in range(len(specs))]
        err_v = max(float((pv - v.double()).abs().max()) for pv, v in zip(per_cfg, vals))
        err_g = float((yg - ref_g.double()).abs().max())
        err_p = float((yp - proj.double()).abs().max())
        clip = [[c.tolist() for c in Y.clip_active(plans.double(), term, e)] if q["kind"] == "follow_decayed" else None for e, q in enumerate(case["entries"])]
        print(f"{name}: entries {case['entries']}\n   reference fp32 against the fp64 yardstick: projection {err_p:.2e} m, values {err_v:.2e} of max "
              f"{float(yv.abs().max()):.4f}, gradient {err_g:.2e} of max {float(yg.abs().max()):.3e}; clip (any, all per sample) {clip}")
        assert err_p <= 1e-5, "the reference's fp32 projection chose another segment than the yardstick"
        assert bool(torch.isfinite(ref_g).all()) and float(ref_g[..., [2, 4, 5]].abs().max()) == 0.0
        for k, v in enumerate(vals):
            out[f"{name}_values_{k}"] = v
        out[name + "_proj"], out[name + "_grad"], out[name + "_total"] = proj, ref_g, tot.detach().reshape(1)
        meta_cases[name] = dict(case, weights=[s[3] for s in specs], clip=clip, ref_proj_err=err_p, ref_value_err=err_v, ref_grad_err=err_g,
                                max_value=float(yv.abs().max()), max_grad=float(yg.abs().max()), max_proj=float(yp.abs().max()))
    some, always = meta_cases["clip"]["clip"][0]
    assert any(s and not a for s, a in zip(some, always)), "the clip case needs a sample where the clip is active at some steps and idle at others"
    assert not any(meta_cases["followlane"]["clip"][0][0])
    out.update(plans=plans, world_lines=wl, line_frame=frames.astype(np.int32), agent_from_world=F, lines_unsorted=unsorted, lines=lines)
    meta = dict(A=A, N=N, S=S, seed=SEED, gap_min=GAP_MIN, kink_min=KINK_MIN, gap=gap, kink=kink, cases=meta_cases, torch=torch.__version__,
                generator="tests/tools/record_lane_golden.py",
                source="the reference's project_onto and lane loss classes + autograd; the lane supply (get_lane_projection up to the sort) replaced")
    arrays = {k: np.ascontiguousarray(v.detach().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    path = os.path.join(ROOT, "tests", "golden", "lane_guidance.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f"lane_guidance: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
