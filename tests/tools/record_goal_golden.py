"""Record tests/golden/global_goal.npz from the reference's own GlobalTargetPosLoss / GlobalTargetPosAtTimeLoss
(src/tbsim/utils/guidance_loss.py:876-1135) through DiffuserGuidance.compute_guidance_loss (:2143-2172) + autograd, on the CPU.

    python tests/tools/record_goal_golden.py          (needs the reference tree, see oracle/_refimport.py)

One scene of A = 8 agents (synth.make_collision_scene), N = 2 plans each (synth.make_collision_trajectories), three cases:
  pos    global_target_pos on a subset of 6 agents with a tolerance: two exact agents, a progress agent whose urgency puts the goal below
         min_progress_dist, one whose relu is inactive, one that has reached its target by its own history point and one flagged only
         through ANOTHER agent's history point (the reference's broadcast, see goal_yardstick.reached_update)
  time   global_target_pos_at_time on all agents at global_t = 7: target times passed, inside the plan and beyond it
  *2     the SAME loss objects after update(global_t=12), with moved frames, new histories and new plans: flags persist, branches change
Every case stores the per-agent values [A,N] (NaN outside the config's agents), d total / d plans [A,N,52,6] and have_reached_mask.
The inputs that are not a synth generator's (frames, histories) are stored too; the configs go into `meta`.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from cld_amd import synth                      # noqa: E402
from oracle import _refimport                  # noqa: E402
from tests import goal_yardstick as Y          # noqa: E402

A, N, SEED = 8, 2, 41


def world_points(W, local):
    return (np.einsum("aij,aj->ai", W[:, :2, :2].astype(np.float64), np.asarray(local, np.float64)) + W[:, :2, 2]).astype(np.float32)


def history(speed, steps=10):
    """[A,steps,2] agent-frame history positions: the agent came along its own axis at its current speed; the last point is 'now'."""
    h = np.zeros((len(speed), steps, 2), np.float32)
    h[:, :, 0] = -0.1 * speed[:, None] * np.arange(steps - 1, -1, -1)[None, :]
    return h


def main():
    _refimport.install()
    with _refimport.redirect_stdout(_refimport.io.StringIO()):
        import tbsim.utils.guidance_loss as gl
    sc = synth.make_collision_scene([A], SEED)
    speed = sc["curr_speed"]
    W1 = sc["world_from_agent"]
    # step 2: every agent has moved along its axis; agent 5 has side-stepped towards its target (progress -> exact)
    dxy = np.stack([0.4 * speed, np.full(A, 0.1)], axis=1)
    dxy[5] = (0.0, 2.5)
    W2 = Y.move_frames(W1, dxy, np.full(A, 0.05)).numpy().astype(np.float32)
    frames = {"": W1, "2": W2}
    hists = {"": history(speed), "2": history(speed * 0.9 + 0.3)}
    plans = {"": synth.make_collision_trajectories(A, N, speed, SEED), "2": synth.make_collision_trajectories(A, N, speed, SEED + 1)}

    sub = [0, 1, 2, 4, 5, 7]
    here = world_points(W1, hists[""][:, -5])                           # the history point the reference looks at, world frame
    local = np.zeros((A, 2))
    local[2], local[4] = (5.0, 1.5), (3.0, 3.0)                         # exact
    local[5] = (0.7, 8.5)                                               # progress, urgency 0.05: goal distance = min_progress_dist
    local[7] = (90.0, 0.0)                                              # progress, inactive relu
    local[0] = (1.0, 0.5)                                               # reached (own history point)
    tp = world_points(W1, local)
    tp[1] = here[7] + np.float32([0.3, -0.2])                           # flagged through agent 7's history point only
    pos_cfg = dict(name="global_target_pos", agents=sub, weight=2.0, target_pos=tp[sub].tolist(),
                   urgency=[0.8, 0.5, 0.6, 0.7, 0.05, 0.5], pref_speed=[1.42] * 6, dt=0.1, min_progress_dist=0.5,
                   target_tolerance=2.0, action_num=5)
    local_t = np.array([(10.0, 10.0), (2.5, 6.0), (20.0, 2.0), (45.0, 3.0), (60.0, 0.0), (5.0, 1.0), (30.0, -4.0), (50.0, 0.0)])
    time_cfg = dict(name="global_target_pos_at_time", agents=None, weight=3.0, target_pos=world_points(W1, local_t).tolist(),
                    target_time=[3, 10, 27, 60, 67, 70, 80, 90], urgency=[0.5, 0.5, 0.5, 0.3, 0.5, 0.0, 0.2, 0.0],
                    pref_speed=[1.42] * A, dt=0.1, target_tolerance=2.0, action_num=5)

    def params(c):
        p = {k: c[k] for k in ("target_pos", "urgency", "pref_speed", "dt", "target_tolerance", "action_num")}
        if c["name"] == "global_target_pos":
            p["min_progress_dist"] = c["min_progress_dist"]
        else:
            p["target_time"] = c["target_time"]
        return p

    out, meta_cases = {}, {}
    for tag, cfg in (("pos", pos_cfg), ("time", time_cfg)):
        g = gl.DiffuserGuidance([[{"name": cfg["name"], "weight": cfg["weight"], "params": params(cfg), "agents": cfg["agents"]}]])
        idx = list(range(A)) if cfg["agents"] is None else cfg["agents"]
        reached = torch.zeros(len(idx), dtype=torch.bool)
        for sfx, gt in (("", 7 if tag == "time" else 0), ("2", 12)):
            g.update(global_t=gt)
            Wf = torch.from_numpy(frames[sfx])
            afw = Y.invert_frames(Wf).float()
            db = {"agent_from_world": afw, "world_from_agent": Wf, "agent_hist": torch.from_numpy(hists[sfx]),
                  "scene_index": torch.zeros(A, dtype=torch.long)}
            x = torch.from_numpy(plans[sfx]).clone().requires_grad_(True)
            tot, per = g.compute_guidance_loss(x * 1.0, db)
            tot.backward()
            name = tag + sfx
            mask = g.guide_configs[0][0].func.have_reached_mask
            assert bool((mask == mask[:, :1]).all())
            full = torch.zeros(A, dtype=torch.bool)
            full[idx] = mask[:, 0]
            out[name + "_values"] = per[cfg["name"] + "_scene_000_00"]
            out[name + "_grad"] = x.grad.clone()
            out[name + "_total"] = tot.detach().reshape(1)
            out[name + "_reached"] = full
            case = dict(cfg, global_t=gt, frames=sfx, plans_seed=SEED + (1 if sfx else 0))
            meta_cases[name] = case
            # the yardstick's view of the same case: branches, margins, and its own flags
            arrays = {sfx + "agent_from_world": afw.numpy()}
            goal, _ = Y.goal_from_meta(case, arrays, sfx, A, N)
            reached, tol_margin = Y.reached_update(reached, goal["target_pos"][idx], Wf[idx].double(), db["agent_hist"][idx].double(), cfg["target_tolerance"], 5)
            goal["reached"][idx] = reached
            kink, dmin = Y.margins(torch.from_numpy(plans[sfx]).double(), goal)
            v = Y.values(torch.from_numpy(plans[sfx]).double(), goal)
            print(f"{name}: branches {Y.branches(goal)}\n   kink margin {kink:.3e} m, tolerance margin {tol_margin:.3e} m, smallest distance read {dmin:.3e} m; "
                  f"max |value - reference| {float((v[idx] - per[cfg['name'] + '_scene_000_00'][idx].double()).abs().max()):.2e}")
            print("   values", np.round(v.numpy(), 3).tolist())
            assert kink >= 1e-3 and tol_margin >= 1e-3 and dmin >= 1e-2
            assert torch.equal(goal["reached"], full)
    for sfx in ("", "2"):
        out[sfx + "world_from_agent"] = frames[sfx]
        out[sfx + "agent_from_world"] = Y.invert_frames(frames[sfx]).float().numpy()
        out[sfx + "agent_hist"] = hists[sfx]
    meta = dict(A=A, N=N, seed=SEED, scene="synth.make_collision_scene([A], seed)", plans="synth.make_collision_trajectories(A, N, curr_speed, plans_seed)",
                cases=meta_cases, torch=torch.__version__, generator="tests/tools/record_goal_golden.py",
                source="the reference's GlobalTargetPosLoss / GlobalTargetPosAtTimeLoss through DiffuserGuidance.compute_guidance_loss + autograd")
    arrays = {k: np.ascontiguousarray(v.detach().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    path = os.path.join(ROOT, "tests", "golden", "global_goal.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f"global_goal: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
