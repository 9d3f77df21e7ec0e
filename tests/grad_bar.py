"""The calibrated gradient bar of the GPU training tests (test_gpu_train.py, test_gpu_vae_train.py): against autograd in float64 on the
CPU, with the same autograd in float32 setting the scale, per tensor
    max|g - g64| <= 4 max|g32 - g64| + 1e-7 max|g64|.
A plain module, imported by those tests."""
import math

import torch


def ratio(g, g64, g32):
    """max|g - g64| over the bar."""
    g, g64, g32 = (torch.as_tensor(a).double().cpu() for a in (g, g64, g32))
    bar = 4 * (g32 - g64).abs().max() + 1e-7 * g64.abs().max()
    err = float((g - g64).abs().max())
    return err / float(bar) if bar > 0 else (0.0 if err == 0 else math.inf)


def check_all(label, ratios, tag, got, g64, g32):
    """Every tensor of g64 within the bar; the worst ratio is printed as `[label] tag: ...` and kept in ratios[tag]."""
    worst = (0.0, None)
    bad = []
    for k in g64:
        r = ratio(got[k], g64[k], g32[k])
        worst = max(worst, (r, k), key=lambda a: a[0])
        if not r <= 1.0:
            bad.append((k, r))
    ratios[tag] = worst
    print(f"\n[{label}] {tag}: worst ratio {worst[0]:.3g} ({worst[1]}), {len(g64)} tensors")
    assert not bad, f"{tag}: over the bar: {bad[:6]}"
