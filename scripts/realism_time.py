"""Time of `RealismDeviation.compute()` (six cld_sort_f32, three cld_wasserstein_f32 and the mean; csrc/realism_kernels.hip) with HIP
events, warmed up, the median of repeated windows, at 2,048 and 65,536 rows of [rows,52,6] per side -- and of the same six sorts, three
distances (paired form: equal sizes) and mean written with torch.sort on the same device, which is the comparator: there is no earlier
time, the library could not do this before.  Also the time of one `add` (two cld_realism_terms launches).
    python3 scripts/realism_time.py [--rounds 9] [--out profiles/realism/realism_time.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cld_amd.engine import Engine
from cld_amd.metrics import RealismDeviation

dev = "cuda:0"


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def torch_compute(vals):
    wd = [(torch.sort(vals["gt"][n])[0].double() - torch.sort(vals["pred"][n])[0].double()).abs().mean() for n in ("lon", "lat", "jerk")]
    return wd, (wd[0] + wd[1] + wd[2]) / 3.0


def time_case(e, rows, g, rounds):
    gt = torch.randn(rows, 52, 6, device=dev, generator=g)
    pred = torch.randn(rows, 52, 6, device=dev, generator=g) * 1.1 + 0.05
    m = RealismDeviation(e, dt=0.1, capacity=rows * 52)
    m.add(gt, pred)
    vals = m.values()
    reps = 200 if rows <= 4096 else 100                       # a window is about 0.1 s
    for _ in range(5):
        ours, theirs = m.compute(), torch_compute(vals)
    torch.cuda.synchronize()
    agree = abs(float(ours["realism_deviation"]) - float(theirs[1])) / float(theirs[1])
    t_ours, t_torch = [], []
    for _ in range(rounds):                                    # the two forms alternate, window by window
        t_ours.append(event_ms(m.compute, reps))
        t_torch.append(event_ms(lambda: torch_compute(vals), reps))
    t_ours.sort()
    t_torch.sort()

    def add():
        m.reset()
        m.add(gt, pred)
    t_add = sorted(event_ms(add, reps) for _ in range(rounds))
    mid = rounds // 2
    res = dict(rows=rows, values_per_array=rows * 52, compute_ms=t_ours[mid], compute_ms_all=t_ours, torch_sort_ms=t_torch[mid],
               torch_sort_ms_all=t_torch, ratio_ours_over_torch=t_ours[mid] / t_torch[mid], add_ms=t_add[mid], relative_difference=agree)
    print(f"{rows} rows: compute {res['compute_ms']:.3f} ms (min {t_ours[0]:.3f}, max {t_ours[-1]:.3f}); torch.sort form {res['torch_sort_ms']:.3f} ms "
          f"(min {t_torch[0]:.3f}, max {t_torch[-1]:.3f}); ratio {res['ratio_ours_over_torch']:.2f}; add {res['add_ms']:.3f} ms; "
          f"the two agree to {agree:.1e}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = torch.Generator(device=dev).manual_seed(5)
    e = Engine(n_timesteps=10, device=dev)
    res = [time_case(e, 2048, g, args.rounds), time_case(e, 65536, g, args.rounds)]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
