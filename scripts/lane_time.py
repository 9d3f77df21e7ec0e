"""Times of the lane term on the device at 32 scenes x 64 agents (2,048 plans), every agent carrying one entry (the three kinds in
turn), at polylines of 128 and of 1,024 points: the stand-alone cld_lane_loss launch (value + gradient, into a fresh gradient buffer
the launcher zeroes first and in place, grad_in == grad, which times the kernel alone; the pair and social-group launches on the
same batch beside it), cld_lane_prepare at the same sizes, and the collision-guided step (target speed + agent collisions, Adam) with
and without the term.  Device events around back-to-back library calls on prebuilt structs; versions alternate; three rounds."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cld_amd import synth                    # noqa: E402
from cld_amd.engine import Engine, _ptr      # noqa: E402

S, M = 32, 64
A, REPS, WARM, ROUNDS = S * M, 200, 20, 3
KINDS = ("following", "change_left", "follow_decayed")
SIZES = (128, 1024)


def timed(fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps        # us per call


def world_lines(sc, pts, seed=7):
    """Per agent a gently curved lane of `pts` points 1 m apart through its pose, in the world frame [A,pts,3] float64."""
    rng = np.random.default_rng(seed)
    W = np.asarray(sc["world_from_agent"], np.float64)
    x = -5.0 + np.arange(pts)[None, :] * 1.0 + rng.uniform(-0.05, 0.05, (A, pts))
    curv = rng.uniform(-0.004, 0.004, (A, 1)) * min(1.0, (60.0 / pts) ** 2)
    y = rng.uniform(-0.5, 0.5, (A, 1)) + curv * x * x
    h = np.arctan(2 * curv * x)
    th = np.arctan2(W[:, 1, 0], W[:, 0, 0])[:, None]
    return np.stack([W[:, 0, 0, None] * x + W[:, 0, 1, None] * y + W[:, 0, 2, None], W[:, 1, 0, None] * x + W[:, 1, 1, None] * y + W[:, 1, 2, None], h + th], axis=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lane", "lane_time.json"))
    args = ap.parse_args()
    e = Engine(n_timesteps=100, device="cuda:0")
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True)); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
    out = {"scenes": S, "agents_per_scene": M, "entries": A, "reps": REPS, "rounds": ROUNDS, "unit": "us per call, device events around back-to-back calls"}
    stream = e._stream()
    sc = synth.make_collision_scene([M] * S, 7)
    Wt = torch.from_numpy(sc["world_from_agent"]).double()
    F = torch.linalg.inv(Wt).float().cuda()
    traj = torch.from_numpy(synth.make_collision_trajectories(A, 1, sc["curr_speed"], 7)).reshape(A, 52, 6).cuda()
    loss = torch.empty(A, device="cuda"); grad = torch.empty(A, 52, 6, device="cuda"); value = torch.empty(A, device="cuda")
    frames = torch.arange(A, dtype=torch.int32, device="cuda")
    fns, terms = {}, {}
    for pts in SIZES:
        wl = torch.from_numpy(world_lines(sc, pts)).cuda()
        lines = torch.empty(A, pts, 3, device="cuda")
        fns[f"lane_prepare_{pts}_pts"] = (lambda wl=wl, lines=lines, pts=pts:
                                          e.lib.cld_lane_prepare(e._h, _ptr(wl), _ptr(frames), _ptr(F), _ptr(lines), A, pts, A, stream))
        assert fns[f"lane_prepare_{pts}_pts"]() == 0
        ct, keep = e._lane(dict(agent=list(range(A)), line=list(range(A)), kind=[KINDS[a % 3] for a in range(A)], decay=0.9, scale=[1.0] * A, lines=lines), A)
        terms[pts] = (ct, keep)
        fns[f"lane_loss_{pts}_pts"] = (lambda ct=ct: e.lib.cld_lane_loss(e._h, _ptr(traj), C.byref(ct), None, _ptr(value), None, _ptr(grad), A, stream))
        # grad_in == grad: the launcher fills nothing, the kernel adds to the buffer in place (what run_guidance does) -- the kernel alone
        fns[f"lane_loss_{pts}_pts_in_place"] = (lambda ct=ct: e.lib.cld_lane_loss(e._h, _ptr(traj), C.byref(ct), _ptr(grad), _ptr(value), None, _ptr(grad), A, stream))
    tg = [s * M + 2 * p for s in range(S) for p in range(8)]
    pt, pkeep = e._pair(dict(target=tg, ref=[a + 1 for a in tg], kind="keep_distance", lo=2.0, hi=4.0, scale=[1.0] * len(tg), world_from_agent=sc["world_from_agent"]), A)
    pvalue = torch.empty(len(tg), device="cuda")
    fns["pair_8_per_scene"] = lambda: e.lib.cld_pair_loss(e._h, _ptr(traj), C.byref(pt), None, _ptr(pvalue), _ptr(grad), A, stream)
    groups = [list(range(g * M, (g + 1) * M)) for g in range(S)]
    cs_, skeep = e._social(dict(groups=groups, leader=[g[0] for g in groups], cohesion=0.8, scale=[1.0 / M] * S, world_from_agent=sc["world_from_agent"]), A)
    fns["social_cohesion_0.8"] = lambda: e.lib.cld_social_group_loss(e._h, _ptr(traj), C.byref(cs_), None, _ptr(loss), _ptr(grad), A, stream)
    res = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            assert fn() == 0
            res[k].append(round(timed(fn), 2))
    out["launch"] = res
    print("launch:", res, flush=True)
    # the collision-guided step at 2,048 agents: target speed + agent collisions, without the term / with it at both polyline sizes
    inp = synth.make_inputs(A, 7)
    cond, cs = torch.from_numpy(inp["cond_feat"]).cuda(), torch.from_numpy(inp["curr_states"]).cuda()
    mean = (torch.from_numpy(synth.normal(7, "m", (A, 52, 4))) * 0.7).cuda()
    tgt = torch.from_numpy(synth.uniform(7, "tgt", (A, 52), 0.0, 12.0)).cuda()
    col = dict(extent=sc["extent"], world_from_agent=sc["world_from_agent"], curr_speed=sc["curr_speed"], scene_index=sc["scene_index"], weight=1.0)
    cg, gkeep = e._guidance(dict(curr_states=cs, target_speed=tgt, lr=0.3, optimizer="adam", agent_collision=col), A)
    mg = torch.empty_like(mean)
    ws, wsn = e._workspace(A)
    built = {"collision": None}
    for pts in SIZES:
        built[f"collision+lane_{pts}_pts"] = terms[pts]

    def step(k):
        lt = built[k]
        if lt is not None:
            e.lib.cld_set_lane_term(e._h, C.byref(lt[0]))
        rc = e.lib.cld_guidance_step(e._h, _ptr(mean), _ptr(cond), C.byref(cg), C.c_float(0.5), None, _ptr(mg), None, None, A, ws, wsn, stream)
        if lt is not None:
            e.lib.cld_set_lane_term(e._h, None)
        return rc
    res = {k: [] for k in built}
    for _ in range(ROUNDS):
        for k in built:
            assert step(k) == 0
            res[k].append(round(timed(lambda: step(k), 50, 5), 1))
    out["guided_step"] = res
    print("guided step:", res, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
