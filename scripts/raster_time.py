"""Time of the observation raster (cld_rasterize, csrc/raster_kernels.hip) at 1,024 and 4,096 agents in 64-agent scenes, 34 x 224 x 224:
  * the kernel, with HIP events, warmed up;
  * a torch-ROCm composition of the same definition (scatter for the history planes, gather for the semantic planes), alternating with
    the kernel in the same run; it works through the agents in chunks so that its index tensors fit;
  * a configs[4]-shaped closed loop (4,096 agents, ContextEncoder + 100-step sampler + decode + world step per sim step) with
    SceneObserver(encode=True) as the observation stage, against the same loop encoding one static raster.
    python3 scripts/raster_time.py [--agents 1024 4096] [--loop-agents 4096] [--sim-steps 3] [--out profiles/raster/raster_time.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cld_amd import synth
from cld_amd.engine import Engine

T, NS, H, W, A = 31, 3, 224, 224, 64
STORE_RATE = 6.1e12          # plain 16-byte stores, MI355X (6.0-6.2 TB/s measured for that shape)
dev = "cuda:0"


def scene_set(B, g):
    """B agents in scenes of A: poses within +-40 m of a scene centre, straight histories, 90 % of the frames available, one shared map."""
    S = B // A
    centre = (torch.rand(S, 1, 2, device=dev, generator=g) - 0.5) * 400.0
    pos = (centre + (torch.rand(S, A, 2, device=dev, generator=g) - 0.5) * 80.0).reshape(B, 2)
    yaw = (torch.rand(B, device=dev, generator=g) - 0.5) * 6.28
    speed = torch.rand(B, device=dev, generator=g) * 10.0
    back = 0.1 * torch.arange(T - 1, -1, -1.0, device=dev)
    xy = pos[:, None, :] - speed[:, None, None] * back[None, :, None] * torch.stack([torch.cos(yaw), torch.sin(yaw)], -1)[:, None, :]
    hw = torch.cat([xy, yaw[:, None, None].expand(B, T, 1)], -1).contiguous()
    av = (torch.rand(B, T, device=dev, generator=g) < 0.9).to(torch.uint8)
    av[:, T - 1] = 1
    start = torch.arange(0, B + 1, A, dtype=torch.int32, device=dev)
    maps = (torch.randint(0, 3, (1, NS, 256, 256), device=dev, generator=g).float() * 0.5).repeat_interleave(8, 2).repeat_interleave(8, 3).contiguous()
    mfw = torch.tensor([[[2.0, 0.0, 1024.0], [0.0, 2.0, 1024.0], [0.0, 0.0, 1.0]]], device=dev)
    return dict(hist_world=hw, hist_avail=av, scene_start=start, maps=maps, scene_map=torch.zeros(S, dtype=torch.int32, device=dev), map_from_world=mfw)


def torch_raster(sc, out, drv, chunk=128, dist=30.0):
    """The definition of include/cld.h `cld_rasterize` composed from torch ops, for scenes of A agents and one map."""
    hw, av, maps, M = sc["hist_world"], sc["hist_avail"] != 0, sc["maps"][0], sc["map_from_world"][0]
    B = hw.shape[0]
    vv, uu = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    ax, ay = (uu - 56.0) / 2.0, (vv - 112.0) / 2.0
    for b0 in range(0, B, chunk):
        b1 = min(b0 + chunk, B)
        rows = torch.arange(b0, b1, device=dev)
        n = b1 - b0
        pose = hw[rows, T - 1]
        c, s = torch.cos(pose[:, 2]), torch.sin(pose[:, 2])
        members = (rows // A * A)[:, None] + torch.arange(A, device=dev)[None, :]                      # [n,A]
        p = hw[members]                                                                                # [n,A,T,3]
        dx, dy = p[..., 0] - pose[:, None, None, 0], p[..., 1] - pose[:, None, None, 1]
        rx = (c[:, None, None] * dx + s[:, None, None] * dy) * 2.0 + 56.0
        ry = (c[:, None, None] * dy - s[:, None, None] * dx) * 2.0 + 112.0
        ego = members == rows[:, None]
        near = av[members][:, :, T - 1] & (dx[:, :, T - 1] ** 2 + dy[:, :, T - 1] ** 2 <= dist * dist)
        ok = av[members] & (near | ego)[:, :, None]
        rx, ry = torch.where(ok, rx, 0.0).clamp_(0, W - 1).round_(), torch.where(ok, ry, 0.0).clamp_(0, H - 1).round_()
        flat = (ry.long() * W + rx.long()).permute(0, 2, 1)                                            # [n,T,A]
        ego_flat = torch.where(ego[:, None, :], flat, 0).sum(-1, keepdim=True)
        hist = torch.zeros(n, T, H * W, device=dev)
        hist.scatter_(2, torch.where(ego[:, None, :], torch.zeros_like(flat), flat), -1.0)             # (the ego's own slot goes to pixel 0)
        hist.scatter_(2, ego_flat, 1.0)
        hist[:, :, 0] = 0.0
        hist[:, :, -1] = 0.0
        out[b0:b1, :T] = hist.view(n, T, H, W)
        wx = pose[:, 0, None, None] + c[:, None, None] * ax - s[:, None, None] * ay
        wy = pose[:, 1, None, None] + s[:, None, None] * ax + c[:, None, None] * ay
        mx, my = (M[0, 0] * wx + M[0, 1] * wy + M[0, 2]).round_(), (M[1, 0] * wx + M[1, 1] * wy + M[1, 2]).round_()
        inside = (mx >= 0) & (mx < maps.shape[2]) & (my >= 0) & (my < maps.shape[1])
        idx = my.clamp_(0, maps.shape[1] - 1).long() * maps.shape[2] + mx.clamp_(0, maps.shape[2] - 1).long()
        sem = maps.view(NS, -1)[:, idx.view(-1)].view(NS, n, H, W).permute(1, 0, 2, 3)
        out[b0:b1, T:] = torch.where(inside[:, None], sem, -1.0)
        drv[b0:b1] = (out[b0:b1, T] != 0).to(torch.uint8)


def event_ms(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def time_kernel(e, B, g, rounds):
    sc = scene_set(B, g)
    img = torch.empty(B, T + NS, H, W, device=dev)
    ref = torch.empty_like(img)
    drv = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    kern = lambda: e.rasterize(sc["hist_world"], sc["hist_avail"], sc["scene_start"], sc["maps"], sc["scene_map"], sc["map_from_world"], out=img)
    comp = lambda: torch_raster(sc, ref, drv)
    bare = lambda: e.rasterize(sc["hist_world"], sc["hist_avail"], sc["scene_start"], out=img)       # no map: the semantic planes are a constant
    kern(); comp(); bare(); kern()
    torch.cuda.synchronize()
    diff = int((img != ref).sum())
    tk, tt, tb = [], [], []
    for _ in range(rounds):
        tk.append(event_ms(kern, 10))                 # (ten launches per window: one is about a millisecond)
        tb.append(event_ms(bare, 10))
        tt.append(event_ms(comp))
    nbytes = img.numel() * 4 + drv.numel()
    k, t = sorted(tk)[len(tk) // 2], sorted(tt)[len(tt) // 2]
    res = dict(agents=B, kernel_ms=k, kernel_ms_all=tk, kernel_no_map_ms=sorted(tb)[len(tb) // 2], torch_ms=t, torch_ms_all=tt, bytes=nbytes, bytes_per_s=nbytes / (k * 1e-3),
               share_of_store_rate=nbytes / (k * 1e-3) / STORE_RATE, torch_over_kernel=t / k, pixels_differing_from_torch=diff,
               floor_ms=nbytes / STORE_RATE * 1e3)
    print(f"{B} agents: kernel {k:.3f} ms (floor {res['floor_ms']:.3f} ms at {STORE_RATE / 1e12:.1f} TB/s) = {res['bytes_per_s'] / 1e12:.2f} TB/s, "
          f"{res['share_of_store_rate']:.1%} of the store rate ({res['kernel_no_map_ms']:.3f} ms without a map); torch composition {t:.1f} ms = {t / k:.1f} x; {diff} of {img.numel()} pixels differ "
          f"(fp32 rounding at pixel boundaries)", flush=True)
    del img, ref, drv
    torch.cuda.empty_cache()
    return res


def time_loop(B, g, sim_steps, n):
    from cld_amd.dm_model import DmModel
    from cld_amd.observe import SceneObserver
    from cld_amd.policy import CldPolicy, closed_loop_rollout
    from cld_amd.vae_model import VaeModel
    e = Engine(n_timesteps=n, device=dev)
    for sd in (synth.make_unet_weights(0, affine_jitter=True), synth.make_decoder_weights(0), synth.make_context_weights(0)):
        e.load_state_dict(sd)
    e.finalize()
    pol = CldPolicy(DmModel(None, None, n_timesteps=n, engine=e), VaeModel(engine=e))
    sc = scene_set(B, g)
    cs = torch.zeros(B, 4, device=dev)
    cs[:, 2] = torch.rand(B, device=dev, generator=g) * 10.0
    hw = sc["hist_world"]
    static = e.rasterize(hw, sc["hist_avail"], sc["scene_start"], sc["maps"], sc["scene_map"], sc["map_from_world"])[0]
    out = {}
    for name in ("static", "observer", "static", "observer"):          # alternating; the first pair warms up
        if name == "static":
            fn = lambda s, w, c: e.context_encode(static, c)
        else:
            fn = SceneObserver(e, sc["scene_start"], hw, sc["hist_avail"], sc["maps"], sc["scene_map"], sc["map_from_world"], encode=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        closed_loop_rollout(pol, fn, hw[:, -1, :2], hw[:, -1, 2], cs, n_sim_steps=sim_steps, gather=lambda traj: traj)
        torch.cuda.synchronize()
        out[name] = (time.perf_counter() - t0) / sim_steps * 1e3
        print(f"closed loop, {B} agents, {n} denoising steps, {name} raster: {out[name]:.1f} ms per sim step", flush=True)
    return dict(agents=B, denoising_steps=n, sim_steps=sim_steps, static_ms_per_sim_step=out["static"], observer_ms_per_sim_step=out["observer"],
                added_ms_per_sim_step=out["observer"] - out["static"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="*", default=[1024, 4096])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop-agents", type=int, default=4096)
    ap.add_argument("--sim-steps", type=int, default=3)
    ap.add_argument("--denoise", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = torch.Generator(device=dev).manual_seed(3)
    e = Engine(n_timesteps=10, device=dev)
    res = {"kernel": [time_kernel(e, B, g, args.rounds) for B in args.agents]}
    if args.loop_agents:
        res["closed_loop"] = time_loop(args.loop_agents, g, args.sim_steps, args.denoise)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
