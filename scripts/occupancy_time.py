"""Time of the occupancy metrics' launches (cld_occupancy_splat / cld_occupancy_read, csrc/occupancy_kernels.hip) with HIP events, warmed up,
the median of repeated windows of 300 launches (a launch takes microseconds; a window is milliseconds): 4,096 agents in 64 scenes of 64 on
80 m x 80 m each, windows of the agents' bounding box +- 100 m, for the coverage grid (step 2 m, 7 x 7 cells per agent) and the diversity grid
(step 4 m, 5 x 5 cells per agent).
    python3 scripts/occupancy_time.py [--rounds 9] [--out profiles/occupancy/occupancy_time.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cld_amd.engine import Engine
from cld_amd.metrics import COVERAGE_DEFAULTS, DIVERSITY_DEFAULTS, OccupancyMetrics

dev = "cuda:0"


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = torch.Generator(device=dev).manual_seed(5)
    e = Engine(n_timesteps=10, device=dev)
    scenes, agents = 64, 64
    B = scenes * agents
    centre = (torch.rand(scenes, 1, 2, device=dev, generator=g) - 0.5) * 4000.0
    pos = (centre + (torch.rand(scenes, agents, 2, device=dev, generator=g) - 0.5) * 80.0).reshape(B, 2)
    world = torch.cat([pos, (torch.rand(B, 1, device=dev, generator=g) - 0.5) * 6.28], 1).contiguous()
    maps = (torch.randint(0, 3, (1, 3, 256, 256), device=dev, generator=g).float() * 0.5).repeat_interleave(8, 2).repeat_interleave(8, 3).contiguous()
    mfw = torch.tensor([[[0.25, 0.0, 1024.0], [0.0, 0.25, 1024.0], [0.0, 0.0, 1.0]]], device=dev)
    occ = OccupancyMetrics(e, list(range(0, B + 1, agents)), world, maps, torch.zeros(scenes, dtype=torch.int32), mfw)
    res = []
    for name, cfg in (("coverage", COVERAGE_DEFAULTS), ("diversity", DIVERSITY_DEFAULTS)):
        gr = occ._grids[name]
        setup, plane, dropped = gr["setup"], gr["grid"][0], gr["dropped"]
        splat = lambda: e.occupancy_splat(setup, world, plane, dropped)
        if name == "coverage":
            read = lambda: e.occupancy_read(setup, plane, occ._success, threshold=cfg["threshold"])
        else:
            read = lambda: e.occupancy_read(setup, plane, counts=False, values=True, lane=True, mass=True)
        for _ in range(20):
            splat()
            read()
        torch.cuda.synchronize()
        t = sorted(event_ms(splat, 300) for _ in range(args.rounds))
        plane.zero_()                                                # (6,000 adds of up to 2^40 per cell stay far below 2^64; start the read from a plain state)
        splat()
        r = sorted(event_ms(read, 300) for _ in range(args.rounds))
        n_win = (2 * setup[4] + 1) ** 2
        res.append(dict(grid=name, scenes=scenes, agents_per_scene=agents, cells=setup[3], window_cells=n_win, adds_per_launch=B * n_win,
                        splat_ms=t[len(t) // 2], splat_ms_all=t, read_ms=r[len(r) // 2], read_ms_all=r,
                        read_outputs="counts" if name == "coverage" else "values, lane, mass"))
        print(f"{name}: {setup[3]} cells, splat {res[-1]['splat_ms'] * 1e3:.1f} us (min {t[0] * 1e3:.1f}, max {t[-1] * 1e3:.1f}) for "
              f"{B * n_win} adds, read {res[-1]['read_ms'] * 1e3:.1f} us (min {r[0] * 1e3:.1f}, max {r[-1] * 1e3:.1f})", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
