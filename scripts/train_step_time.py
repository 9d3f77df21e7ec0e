"""Time one U-Net training step (compute_losses-shaped: forward + backward with per-row t) on the HIP training path and on
torch-ROCm fp32 autograd of oracle.unet_forward (TF32 off), with HIP events.  Prints one JSON line per batch size.

    python scripts/train_step_time.py [--sizes 256 2048] [--iters 10]

FLOP: the algorithmic count of the convolutions and Linears (2 MACs per multiply-add), forward x 3 for a step (forward, data and
weight gradients).  The library's kernels execute at least this many (padded tiles, the zero taps of the stride-2 data gradients),
so the fraction of the 157.3 TFLOP/s fp32-MFMA peak printed is a lower bound of the fraction on executed FLOP.
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cld_amd import synth, _lib  # noqa: E402
from cld_amd.train import TrainableDm  # noqa: E402
from oracle import cld_oracle as O  # noqa: E402

PEAK = 157.3e12


def forward_flop_per_row(w):
    f = 0
    L = {"downs.0": 52, "downs.1": 26, "downs.2": 13, "mid": 13, "ups.0": 13, "ups.1": 26, "final": 52}
    for k, v in w.items():
        if not k.endswith("weight") or v.ndim < 2:
            continue
        if v.ndim == 2:
            f += 2 * v.size
            continue
        lvl = next((L[p] for p in L if p in k), 52)
        if ".2.conv" in k and "downs" in k:
            lvl //= 2                      # Downsample1d: output length
        if ".2.conv" in k and "ups" in k:
            lvl *= 2                       # Upsample1d: output length (each output sums k/2 = 2 taps)
            f += v.size * lvl              # 2 flop x C_in C_out x 2 taps per output
            continue
        f += 2 * v.size * lvl
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 2048])
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    wn = synth.make_unet_weights(0, affine_jitter=True)
    dm = TrainableDm(wn, n_timesteps=100, device="cuda:0")
    wt = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in wn.items()}
    sched = {k: v.cuda() for k, v in O.schedule(100).items()}
    emb = O.sinusoidal_emb

    def sinus_dev(t, dim=32, dtype=torch.float32):       # the oracle builds its frequency table on the CPU
        return emb(t.cpu(), dim, dtype).to(t.device)
    O.sinusoidal_emb = sinus_dev
    fl_row = 3 * forward_flop_per_row(wn)
    tape_row = int(_lib.load().cld_unet_tape_bytes(None, 1))
    for B in a.sizes:
        z0 = torch.randn(B, 52, 4, device="cuda:0")
        cond = torch.randn(B, 256, device="cuda:0")
        t = torch.randint(0, 100, (B,), device="cuda:0")
        noise = torch.randn(B, 52, 4, device="cuda:0")

        def hip_step():
            dm.zero_grad()
            dm.compute_losses({"cond_feat": cond}, z0, t=t, noise=noise).backward()

        def torch_step():
            for v in wt.values():
                v.grad = None
            O.compute_losses(wt, sched, z0, cond, t, noise).backward()

        out = {"B": B}
        for name, fn in (("hip", hip_step), ("torch", torch_step)):
            fn(); fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[f"{name}_ms"] = round(e0.elapsed_time(e1) / a.iters, 3)
        out["step_flop"] = fl_row * B
        out["hip_frac_of_peak_algorithmic"] = round(fl_row * B / (out["hip_ms"] * 1e-3) / PEAK, 4)
        out["speedup_vs_torch"] = round(out["torch_ms"] / out["hip_ms"], 3)
        out["tape_bytes_per_row"] = tape_row
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
