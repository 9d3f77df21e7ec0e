"""Time of one environment step and of the read of the guidance satisfaction metrics (cld_guide_metrics_step / cld_guide_metrics_read,
csrc/guide_metrics_kernels.hip) with HIP events, warmed up, the median of repeated windows of launches: 64 scenes x 64 agents and one
scene of 4,096 agents, one config of every guidance name per scene with agents=None (13 entries per scene: the collision kinds are
quadratic per scene, social_group quadratic per entry).  cld_scene_metrics_step is timed in the same run on the same poses as the
yardstick, and the ratio to it is reported.
    python3 scripts/guide_metrics_time.py [--rounds 9] [--out profiles/guide_metrics/guide_metrics_time.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cld_amd.engine import Engine
from cld_amd.metrics import guidance_metric_table

dev = "cuda:0"


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def config(scenes, agents, pos, g):
    B = scenes * agents
    ts = torch.rand(B, 52, generator=g) * 10.0
    out = []
    for s in range(scenes):
        p = pos[s * agents:(s + 1) * agents].cpu().double()
        out.append([
            dict(name="target_speed", weight=1.0, agents=None, params=dict(target_speed=ts)),
            dict(name="speed_limit", weight=1.0, agents=None, params=dict(speed_limit=5.0)),
            dict(name="acc_limit", weight=1.0, agents=None, params=dict(acc_limit=1.0)),
            dict(name="agent_collision", weight=1.0, agents=None, params=dict(excluded_agents=[s * agents, s * agents + 1])),
            dict(name="map_collision", weight=1.0, agents=None, params={}),
            dict(name="target_pos", weight=1.0, agents=None, params=dict(target_pos=torch.rand(agents, 2, generator=g).double() * 20.0)),
            dict(name="global_target_pos", weight=1.0, agents=None, params=dict(target_pos=p + 5.0)),
            dict(name="target_pos_at_time", weight=1.0, agents=None,
                 params=dict(target_pos=torch.rand(agents, 2, generator=g).double() * 20.0, target_time=[10] * agents)),
            dict(name="global_target_pos_at_time", weight=1.0, agents=None, params=dict(target_pos=p - 5.0, target_time=[20] * agents)),
            dict(name="social_group", weight=1.0, agents=None, params=dict(social_dist=2.0)),
        ])
    return out


def time_case(e, scenes, agents, g, rounds):
    B = scenes * agents
    centre = (torch.rand(scenes, 1, 2, device=dev, generator=g) - 0.5) * 400.0
    side = 80.0 * (agents / 64.0) ** 0.5                                     # the density of 64 agents on 80 m x 80 m
    pos = (centre + (torch.rand(scenes, agents, 2, device=dev, generator=g) - 0.5) * side).reshape(B, 2)
    world = torch.cat([pos, (torch.rand(B, 1, device=dev, generator=g) - 0.5) * 6.28], 1).contiguous()
    speed, acc = torch.rand(B, device=dev, generator=g) * 10.0, (torch.rand(B, device=dev, generator=g) - 0.5) * 4.0
    extent = torch.tensor([[4.5, 2.0, 1.5]], device=dev).repeat(B, 1)
    maps = (torch.randint(0, 3, (1, 3, 256, 256), device=dev, generator=g).float() * 0.5).repeat_interleave(8, 2).repeat_interleave(8, 3).contiguous()
    mfw = torch.tensor([[[2.0, 0.0, 1024.0], [0.0, 2.0, 1024.0], [0.0, 0.0, 1.0]]], device=dev)
    ss = list(range(0, B + 1, agents))
    sm = torch.zeros(scenes, dtype=torch.int32)
    table = guidance_metric_table(config(scenes, agents, pos, torch.Generator().manual_seed(5)), ss)
    setup = e.guide_metrics_setup(ss, extent, table, maps, sm, mfw)
    state = e.guide_metrics_state(setup)
    ysetup = e.scene_metrics_setup(ss, extent, maps, sm, mfw)
    ystate = e.scene_metrics_state(B)
    step = lambda: e.guide_metrics_step(setup, world, speed, acc, state, 0)
    yard = lambda: e.scene_metrics_step(ysetup, world, ystate, 0)
    reps = 300 if agents <= 64 else 50
    for fn in (step, yard):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    med = lambda fn, n: sorted(event_ms(fn, n) for _ in range(rounds))
    t, y = med(step, reps), med(yard, reps)
    read = med(lambda: e.guide_metrics_read(setup, state), 20)
    res = dict(scenes=scenes, agents_per_scene=agents, entries=setup[3], members=setup[4], step_ms=t[len(t) // 2], step_ms_all=t,
               read_ms=read[len(read) // 2], scene_metrics_step_ms=y[len(y) // 2], ratio_to_scene_metrics_step=t[len(t) // 2] / y[len(y) // 2])
    print(f"{scenes} scenes x {agents} agents, {setup[3]} entries, {setup[4]} members: step {res['step_ms'] * 1e3:.1f} us "
          f"(min {t[0] * 1e3:.1f}, max {t[-1] * 1e3:.1f}), read {res['read_ms'] * 1e3:.1f} us, cld_scene_metrics_step "
          f"{res['scene_metrics_step_ms'] * 1e3:.1f} us, ratio {res['ratio_to_scene_metrics_step']:.2f}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "guide_metrics", "guide_metrics_time.json"))
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
