"""Time of one environment step of the episode metrics (cld_scene_metrics_step, csrc/metrics_kernels.hip) with HIP events, warmed up, the
median of repeated windows of 300 launches (a launch takes microseconds; a window is milliseconds): 64 scenes x 64 agents, and one scene of 4,096 agents (the partner loop is quadratic per scene).
    python3 scripts/metrics_time.py [--rounds 9] [--out profiles/metrics/metrics_time.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cld_amd.engine import Engine

dev = "cuda:0"


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def time_case(e, scenes, agents, g, rounds):
    B = scenes * agents
    centre = (torch.rand(scenes, 1, 2, device=dev, generator=g) - 0.5) * 400.0
    side = 80.0 * (agents / 64.0) ** 0.5                                     # the density of 64 agents on 80 m x 80 m
    pos = (centre + (torch.rand(scenes, agents, 2, device=dev, generator=g) - 0.5) * side).reshape(B, 2)
    world = torch.cat([pos, (torch.rand(B, 1, device=dev, generator=g) - 0.5) * 6.28], 1).contiguous()
    extent = torch.tensor([[4.5, 2.0, 1.5]], device=dev).repeat(B, 1)
    maps = (torch.randint(0, 3, (1, 3, 256, 256), device=dev, generator=g).float() * 0.5).repeat_interleave(8, 2).repeat_interleave(8, 3).contiguous()
    mfw = torch.tensor([[[2.0, 0.0, 1024.0], [0.0, 2.0, 1024.0], [0.0, 0.0, 1.0]]], device=dev)
    setup = e.scene_metrics_setup(list(range(0, B + 1, agents)), extent, maps, torch.zeros(scenes, dtype=torch.int32), mfw)
    state = e.scene_metrics_state(B)
    step = lambda: e.scene_metrics_step(setup, world, state, 0)
    for _ in range(20):
        step()
    torch.cuda.synchronize()
    t = sorted(event_ms(step, 300) for _ in range(rounds))
    read = sorted(event_ms(lambda: e.scene_metrics_read(setup, state), 300) for _ in range(rounds))
    res = dict(scenes=scenes, agents_per_scene=agents, step_ms=t[len(t) // 2], step_ms_all=t, read_ms=read[len(read) // 2])
    print(f"{scenes} scenes x {agents} agents: step {res['step_ms'] * 1e3:.1f} us (min {t[0] * 1e3:.1f}, max {t[-1] * 1e3:.1f}), read {res['read_ms'] * 1e3:.1f} us",
          flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = torch.Generator(device=dev).manual_seed(5)
    e = Engine(n_timesteps=10, device=dev)
    res = [time_case(e, 64, 64, g, args.rounds), time_case(e, 1, 4096, g, args.rounds)]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
