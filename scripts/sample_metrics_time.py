"""Times of the open-loop sample metrics at the bench size, 4,096 agents x 20 samples x 52 steps: the device call
(cld_sample_metrics: per-agent kernel + the two fold launches), on [B,N,52,2] positions and in place on the [B,N,52,6] state-action
tensor; and what the same ten numbers cost without it: the device-to-host copy of the positions plus a numpy float32 restatement of
the formulas on the host (the [B,N,N,T,2] temporary and all).  Device: one event pair per launch, warm, the median over the launches
and, beside it, the mean of back-to-back launches.  Host: wall clock, the median of a few repetitions."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cld_amd.engine import Engine, _ptr      # noqa: E402

B, N, T = 4096, 20, 52
REPS, WARM, HOST_REPS = 200, 20, 3


def host_float32(pred, gt, avail):
    """The eight keys (and the two last-step ones) in numpy float32, as a user without the device call computes them."""
    n = pred.shape[1]
    e = np.sqrt((((gt[:, None] - pred) * avail[:, None, :, None]) ** 2).sum(-1))
    ade = e.mean(-1)
    last = ((avail > 0) * np.arange(pred.shape[2])).max(-1)
    fde = np.take_along_axis(e, last[:, None, None].repeat(n, 1), 2)[..., 0]
    diff = pred[:, None] - pred[:, :, None]
    apd = np.sqrt((diff ** 2).sum(-1)).mean(-1).reshape(len(pred), -1)
    fpd = np.sqrt((diff[..., 1] ** 2).sum(-1)).reshape(len(pred), -1)
    lpd = np.sqrt((diff[:, :, :, -1] ** 2).sum(-1)).reshape(len(pred), -1)
    cols = [ade.mean(1), ade.min(1), fde.mean(1), fde.min(1), apd.mean(1), apd.max(1), fpd.mean(1), fpd.max(1), lpd.mean(1), lpd.max(1)]
    return np.array([c.mean() for c in cols], np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_metrics", "sample_metrics_time.json"))
    args = ap.parse_args()
    e = Engine(n_timesteps=10, device="cuda:0")
    rng = np.random.default_rng(7)
    gt = np.cumsum(rng.normal(0, 1.4, (B, T, 2)), 1).astype(np.float32)
    pred6 = rng.normal(0, 1.0, (B, N, T, 6)).astype(np.float32)
    pred6[..., :2] = gt[:, None] + np.cumsum(rng.normal(0, 0.4, (B, N, T, 2)), 2).astype(np.float32)
    avail = (rng.random((B, T)) < 0.9).astype(np.float32)
    d6, dg, da = torch.from_numpy(pred6).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(avail).cuda()
    d2 = d6[..., :2].contiguous()
    rows = torch.empty(B, 10, dtype=torch.float64, device="cuda"); idx = torch.empty(B, 4, dtype=torch.int32, device="cuda")
    means = torch.empty(10, dtype=torch.float64, device="cuda")
    wsn = int(e.lib.cld_sample_metrics_workspace_bytes(B))
    ws = torch.empty(wsn, dtype=torch.uint8, device="cuda")
    stream = e._stream()
    out = {"agents": B, "samples": N, "steps": T, "reps": REPS, "unit": "us"}

    def call(p, c, with_means=True):
        return e.lib.cld_sample_metrics(e._h, _ptr(p), c, _ptr(dg), _ptr(da), B, N, T, _ptr(rows), _ptr(idx), _ptr(means) if with_means else None,
                                        _ptr(ws), wsn, stream)
    fns = {"positions_C2": lambda: call(d2, 2), "state_action_C6_in_place": lambda: call(d6, 6), "positions_C2_rows_only": lambda: call(d2, 2, False)}
    for name, fn in fns.items():
        for _ in range(WARM):
            assert fn() == 0
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
        for a, b in ev:
            a.record(); fn(); b.record()
        torch.cuda.synchronize()
        each = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name] = {"median": round(each[REPS // 2], 2), "min": round(each[0], 2), "p90": round(each[REPS * 9 // 10], 2),
                     "back_to_back_mean": round(a.elapsed_time(b) * 1e3 / REPS, 2)}
        print(name, out[name], flush=True)
    call(d2, 2)
    torch.cuda.synchronize()
    dev = means.cpu().numpy()
    # the host path: copy, then numpy float32
    copies, hosts = [], []
    for _ in range(HOST_REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hp, hg, ha = d2.cpu().numpy(), dg.cpu().numpy(), da.cpu().numpy()
        t1 = time.perf_counter()
        host = host_float32(hp, hg, ha)
        t2 = time.perf_counter()
        copies.append((t1 - t0) * 1e6); hosts.append((t2 - t1) * 1e6)
    out["host_copy_of_positions"] = {"median": round(sorted(copies)[HOST_REPS // 2], 1), "bytes": int(d2.numel() * 4)}
    out["host_numpy_float32"] = {"median": round(sorted(hosts)[HOST_REPS // 2], 1), "threads": os.cpu_count()}
    out["device_vs_host_float32_max_rel"] = float(np.max(np.abs(dev - host) / np.abs(host)))
    print({k: out[k] for k in ("host_copy_of_positions", "host_numpy_float32", "device_vs_host_float32_max_rel")}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
