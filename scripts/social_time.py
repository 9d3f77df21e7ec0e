"""Times of the social-group term on the device: the stand-alone launch at 2,048 plans (32 groups of 64, 512 groups of 4), the
agent-collision launch at the same scene sizes as the yardstick, and a guided step at 2,048 agents with and without the term.
Device events around back-to-back library calls on prebuilt structs; versions alternate; three rounds."""
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

A, REPS, WARM, ROUNDS = 2048, 200, 20, 3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "social", "social_time.json"))
    args = ap.parse_args()
    e = Engine(n_timesteps=100, device="cuda:0")
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True)); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
    out = {"agents": A, "reps": REPS, "rounds": ROUNDS, "unit": "us per call, device events around back-to-back calls", "launch": {}, "guided_step": {}}
    stream = e._stream()
    for G, M in ((32, 64), (512, 4)):
        sc = synth.make_collision_scene([M] * G, 7)
        traj = torch.from_numpy(synth.make_collision_trajectories(A, 1, sc["curr_speed"], 7)).reshape(A, 52, 6).cuda()
        loss = torch.empty(A, device="cuda"); grad = torch.empty(A, 52, 6, device="cuda")
        groups = [list(range(g * M, (g + 1) * M)) for g in range(G)]
        fns = {}
        for name, coh in (("social_cohesion_0.8", 0.8), ("social_cohesion_0", 0.0)):
            cs_, keep = e._social(dict(groups=groups, leader=[g[0] for g in groups], cohesion=coh, scale=[1.0 / M] * G, world_from_agent=sc["world_from_agent"]), A)
            fns[name] = (lambda cs_=cs_, keep=keep: e.lib.cld_social_group_loss(e._h, _ptr(traj), C.byref(cs_), None, _ptr(loss), _ptr(grad), A, stream))
        cc, ckeep = e._collision(dict(extent=sc["extent"], world_from_agent=sc["world_from_agent"], curr_speed=sc["curr_speed"], scene_index=sc["scene_index"], weight=1.0), A)
        fns["agent_collision"] = (lambda cc=cc, ckeep=ckeep: e.lib.cld_agent_collision(e._h, _ptr(traj), C.byref(cc), None, _ptr(loss), _ptr(grad), A, stream))
        res = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                assert fn() == 0
                res[k].append(round(timed(fn), 2))
        out["launch"][f"{G}x{M}"] = res
        print(f"{G} groups of {M}:", res, flush=True)
    # a guided step at 2,048 agents (32 scenes of 64): target speed alone / + the social term / + agent collisions
    sc = synth.make_collision_scene([64] * 32, 7)
    inp = synth.make_inputs(A, 7)
    cond, cs = torch.from_numpy(inp["cond_feat"]).cuda(), torch.from_numpy(inp["curr_states"]).cuda()
    mean = (torch.from_numpy(synth.normal(7, "m", (A, 52, 4))) * 0.7).cuda()
    tgt = torch.from_numpy(synth.uniform(7, "tgt", (A, 52), 0.0, 12.0)).cuda()
    groups = [list(range(g * 64, (g + 1) * 64)) for g in range(32)]
    base = dict(curr_states=cs, target_speed=tgt, lr=0.3, optimizer="adam")
    social = dict(groups=groups, leader=[g[0] for g in groups], scale=[1.0 / 64] * 32, world_from_agent=sc["world_from_agent"])
    col = dict(extent=sc["extent"], world_from_agent=sc["world_from_agent"], curr_speed=sc["curr_speed"], scene_index=sc["scene_index"], weight=1.0)
    mg = torch.empty_like(mean)
    ws, wsn = e._workspace(A)
    variants = {"target_speed": (base, None), "target_speed+social": (base, social), "target_speed+agent_collision": (dict(base, agent_collision=col), None),
                "target_speed+agent_collision+social": (dict(base, agent_collision=col), social)}
    built = {}
    for k, (gd, so) in variants.items():
        cg, keep = e._guidance(gd, A)
        st = e._social(so, A) if so is not None else None
        built[k] = (cg, keep, st)

    def step(k):
        cg, keep, st = built[k]
        e.lib.cld_set_social_term(e._h, C.byref(st[0]) if st else None)
        rc = e.lib.cld_guidance_step(e._h, _ptr(mean), _ptr(cond), C.byref(cg), C.c_float(0.5), None, _ptr(mg), None, None, A, ws, wsn, stream)
        e.lib.cld_set_social_term(e._h, None)
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
