"""Times of the pair-relation term on the device at 32 scenes x 64 agents (2,048 plans): the stand-alone launch with 1 and with 8
pairs per scene (value + gradient, into a fresh gradient buffer the launcher zeroes first and in place, grad_in == grad, which
times the kernel alone; the social-group and agent-collision launches on the same scenes beside it), and the
collision-guided step (target speed + agent collisions, Adam) with and without the term.
Device events around back-to-back library calls on prebuilt structs; versions alternate; three rounds.
`--without-only` measures nothing but the guided step without the term and touches no pair entry point, so the same file runs in a
checkout of the parent commit; `--parent-json` merges what that run wrote into this one's output as `guided_step_parent`."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cld_amd import synth                    # noqa: E402
from cld_amd.engine import Engine, _ptr      # noqa: E402

S, M = 32, 64
A, REPS, WARM, ROUNDS = S * M, 200, 20, 3
KINDS = ("keep_distance", "collision", "stay_away", "front_collision", "collide_left")


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


def pair_term(sc, per_scene):
    """`per_scene` pairs in every scene: agents 2p -> 2p + 1 of the scene, the five relations in turn."""
    tg = [s * M + 2 * p for s in range(S) for p in range(per_scene)]
    rf = [a + 1 for a in tg]
    P = len(tg)
    kind = [KINDS[p % 5] for p in range(P)]
    return dict(target=tg, ref=rf, kind=kind, lo=[2.0] * P, hi=[4.0] * P, decay=[0.9 if k == "stay_away" else 0.0 for k in kind], scale=[1.0] * P,
                world_from_agent=sc["world_from_agent"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair", "pair_time.json"))
    ap.add_argument("--without-only", action="store_true")
    ap.add_argument("--parent-json", default=None)
    args = ap.parse_args()
    e = Engine(n_timesteps=100, device="cuda:0")
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True)); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
    out = {"scenes": S, "agents_per_scene": M, "reps": REPS, "rounds": ROUNDS, "unit": "us per call, device events around back-to-back calls"}
    stream = e._stream()
    sc = synth.make_collision_scene([M] * S, 7)
    if not args.without_only:
        traj = torch.from_numpy(synth.make_collision_trajectories(A, 1, sc["curr_speed"], 7)).reshape(A, 52, 6).cuda()
        loss = torch.empty(A, device="cuda"); grad = torch.empty(A, 52, 6, device="cuda")
        fns = {}
        for per_scene in (1, 8):
            ct, keep = e._pair(pair_term(sc, per_scene), A)
            value = torch.empty(S * per_scene, device="cuda")
            fns[f"pair_{per_scene}_per_scene"] = (lambda ct=ct, keep=keep, value=value:
                                                  e.lib.cld_pair_loss(e._h, _ptr(traj), C.byref(ct), None, _ptr(value), _ptr(grad), A, stream))
            # grad_in == grad: the launcher fills nothing, the kernel adds to the buffer in place (what run_guidance does) -- the kernel alone
            fns[f"pair_{per_scene}_per_scene_in_place"] = (lambda ct=ct, keep=keep, value=value:
                                                           e.lib.cld_pair_loss(e._h, _ptr(traj), C.byref(ct), _ptr(grad), _ptr(value), _ptr(grad), A, stream))
        groups = [list(range(g * M, (g + 1) * M)) for g in range(S)]
        cs_, skeep = e._social(dict(groups=groups, leader=[g[0] for g in groups], cohesion=0.8, scale=[1.0 / M] * S, world_from_agent=sc["world_from_agent"]), A)
        fns["social_cohesion_0.8"] = lambda: e.lib.cld_social_group_loss(e._h, _ptr(traj), C.byref(cs_), None, _ptr(loss), _ptr(grad), A, stream)
        cc, ckeep = e._collision(dict(extent=sc["extent"], world_from_agent=sc["world_from_agent"], curr_speed=sc["curr_speed"], scene_index=sc["scene_index"], weight=1.0), A)
        fns["agent_collision"] = lambda: e.lib.cld_agent_collision(e._h, _ptr(traj), C.byref(cc), None, _ptr(loss), _ptr(grad), A, stream)
        res = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                assert fn() == 0
                res[k].append(round(timed(fn), 2))
        out["launch"] = res
        print("launch:", res, flush=True)
    # the collision-guided step at 2,048 agents: target speed + agent collisions, without the term / with 1 / with 8 pairs per scene
    inp = synth.make_inputs(A, 7)
    cond, cs = torch.from_numpy(inp["cond_feat"]).cuda(), torch.from_numpy(inp["curr_states"]).cuda()
    mean = (torch.from_numpy(synth.normal(7, "m", (A, 52, 4))) * 0.7).cuda()
    tgt = torch.from_numpy(synth.uniform(7, "tgt", (A, 52), 0.0, 12.0)).cuda()
    col = dict(extent=sc["extent"], world_from_agent=sc["world_from_agent"], curr_speed=sc["curr_speed"], scene_index=sc["scene_index"], weight=1.0)
    cg, gkeep = e._guidance(dict(curr_states=cs, target_speed=tgt, lr=0.3, optimizer="adam", agent_collision=col), A)
    mg = torch.empty_like(mean)
    ws, wsn = e._workspace(A)
    built = {"collision": None}
    if not args.without_only:
        built["collision+pair_1_per_scene"] = e._pair(pair_term(sc, 1), A)
        built["collision+pair_8_per_scene"] = e._pair(pair_term(sc, 8), A)

    def step(k):
        pt = built[k]
        if pt is not None:
            e.lib.cld_set_pair_term(e._h, C.byref(pt[0]))
        rc = e.lib.cld_guidance_step(e._h, _ptr(mean), _ptr(cond), C.byref(cg), C.c_float(0.5), None, _ptr(mg), None, None, A, ws, wsn, stream)
        if pt is not None:
            e.lib.cld_set_pair_term(e._h, None)
        return rc
    res = {k: [] for k in built}
    for _ in range(ROUNDS):
        for k in built:
            assert step(k) == 0
            res[k].append(round(timed(lambda: step(k), 50, 5), 1))
    out["guided_step"] = res
    print("guided step:", res, flush=True)
    if args.parent_json:
        out["guided_step_parent"] = json.load(open(args.parent_json))["guided_step"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
