"""Time of the map term of the collision guidance (cld_map_collision_loss, csrc/collision_kernels.hip) with HIP events, warmed up, the median
of repeated windows of 100 launches: 64 and 2,048 agents in scenes of 64, 10 x 10 sample points, value and gradient, in raster mode (a
per-agent drivable raster [A,224,224]), in map mode (cld_set_map_source: the scene map read directly) and as the pair map mode
replaces when nobody has rasterised: cld_rasterize of one history frame + the three semantic planes for all agents, then raster mode
(through Engine.rasterize: its allocations are part of what a caller pays).  The library calls themselves are timed on prebuilt structs.
On a tree without cld_set_map_source only raster mode is timed; `--parent a.json [b.json ...]` merges such runs -- the windows of
several processes are pooled, since a process's own nine windows agree to 0.2 % and two processes of the same code differ by more --
and records whether this tree's raster-mode medians lie within the parent's run-to-run spread (min .. max of its windows).
    python3 scripts/map_source_time.py [--rounds 9] [--parent parent.json ...] [--out profiles/map_source/map_source_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cld_amd.engine import Engine

dev = "cuda:0"
REPS = 100


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def windows(fn, rounds):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t = sorted(event_ms(fn, REPS) for _ in range(rounds))
    return dict(ms=t[len(t) // 2], ms_min=t[0], ms_max=t[-1], ms_all=t)


def time_case(e, agents, g, rounds):
    scenes = max(1, agents // 64)
    sizes = [agents // scenes] * scenes
    pos = (torch.rand(agents, 2, device=dev, generator=g) - 0.5) * 600.0
    world = torch.cat([pos, (torch.rand(agents, 1, device=dev, generator=g) - 0.5) * 6.28], 1).contiguous()
    extent = torch.tensor([[4.5, 2.0, 1.5]], device=dev).repeat(agents, 1)
    maps = (torch.randint(0, 3, (1, 3, 256, 256), device=dev, generator=g).float() * 0.5).repeat_interleave(8, 2).repeat_interleave(8, 3).contiguous()
    mfw = torch.tensor([[[2.0, 0.0, 1024.0], [0.0, 2.0, 1024.0], [0.0, 0.0, 1.0]]], device=dev)
    scene_map = torch.zeros(scenes, dtype=torch.int32)
    scene_start = torch.tensor([0] + [sum(sizes[:k + 1]) for k in range(scenes)], dtype=torch.int32)
    speed = 2.0 + 8.0 * torch.rand(agents, device=dev, generator=g)
    t = 0.1 * torch.arange(1, 53, device=dev)
    traj = torch.zeros(agents, 52, 6, device=dev)
    traj[..., 0] = speed[:, None] * t
    traj[..., 1] = (torch.rand(agents, 1, device=dev, generator=g) - 0.5) * 3.0 + 0.05 * t
    traj[..., 2] = speed[:, None]
    traj[..., 3] = (torch.rand(agents, 1, device=dev, generator=g) - 0.5) * 0.3
    rfa = torch.tensor([[2.0, 0.0, 56.0], [0.0, 2.0, 112.0], [0.0, 0.0, 1.0]], device=dev).repeat(agents, 1, 1)
    ones = torch.ones(agents, 1, dtype=torch.uint8, device=dev)
    image = torch.empty(agents, 4, 224, 224, device=dev)

    def rasterize():
        return e.rasterize(world.reshape(agents, 1, 3), ones, scene_start, maps, scene_map, mfw, out=image, want_raster_from_world=False)[1]
    drv = rasterize()
    base = dict(extent=extent, raster_from_agent=rfa, curr_speed=speed, scene_sizes=sizes, weight=1.0, num_points_lw=(10, 10))
    loss, grad = torch.empty(agents, device=dev), torch.empty(agents, 52, 6, device=dev)

    def call(cc):
        e._check(e.lib.cld_map_collision_loss(e._h, C.c_void_p(traj.data_ptr()), C.byref(cc), None, C.c_void_p(loss.data_ptr()),
                                              C.c_void_p(grad.data_ptr()), agents, e._stream()), "cld_map_collision_loss")
    res = dict(agents=agents, scenes=scenes)
    cc_r, keep_r = e._map_collision(dict(base, drivable_map=drv), agents)
    res["raster"] = windows(lambda: call(cc_r), rounds)
    value_r, grad_r = loss.clone(), grad.clone()
    res["mixed_steps_share"] = float((grad_r.abs().sum(-1) > 0).float().mean())
    if hasattr(e.lib, "cld_set_map_source"):
        term = dict(base, map_source=dict(maps=maps, scene_map=scene_map, map_from_world=mfw, world=world))
        cc_m, keep_m = e._map_collision(term, agents)
        with e._handle_terms({"map_collision": term}, agents):
            res["map"] = windows(lambda: call(cc_m), rounds)
        res["map_equals_raster"] = bool(torch.equal(loss, value_r) and torch.equal(grad, grad_r))

        def pair():
            cc, keep = e._map_collision(dict(base, drivable_map=rasterize()), agents)
            call(cc)
        res["rasterize_then_raster"] = windows(pair, rounds)
    for k in ("raster", "map", "rasterize_then_raster"):
        if k in res:
            print(f"{agents} agents, {k}: {res[k]['ms'] * 1e3:.1f} us (min {res[k]['ms_min'] * 1e3:.1f}, max {res[k]['ms_max'] * 1e3:.1f})", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent", nargs="+", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    e = Engine(n_timesteps=10, device=dev)
    res = []
    for agents in (64, 2048):
        g = torch.Generator(device=dev).manual_seed(5)
        res.append(time_case(e, agents, g, args.rounds))
    if args.parent:
        runs = []
        for path in args.parent:
            with open(path) as f:
                runs.append({r["agents"]: r["raster"] for r in json.load(f)})
        for r in res:
            pooled = sorted(t for run in runs for t in run[r["agents"]]["ms_all"])
            p = dict(ms=pooled[len(pooled) // 2], ms_min=pooled[0], ms_max=pooled[-1], ms_all=pooled, processes=len(runs),
                     process_medians=[run[r["agents"]]["ms"] for run in runs])
            r["parent_raster"] = p
            r["raster_within_parent_spread"] = bool(p["ms_min"] <= r["raster"]["ms"] <= p["ms_max"])
            print(f"{r['agents']} agents: raster mode {r['raster']['ms'] * 1e3:.1f} us, parent {p['ms'] * 1e3:.1f} us "
                  f"(spread {p['ms_min'] * 1e3:.1f} .. {p['ms_max'] * 1e3:.1f}): within = {r['raster_within_parent_spread']}", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
