"""CPU tests of the U-Net training path's yardstick and parameter table (no GPU).

- The fp64 autograd of oracle.unet_forward, the yardstick of tests/test_gpu_train.py, agrees with central finite differences on
  entries of every layer kind (k5 convolution, GroupNorm weight and bias, block Linear, residual 1x1, Downsample1d, ConvTranspose1d,
  final 1x1, both time-MLP Linears) and on x and cond.
- The flat parameter table of the C-ABI (cld_unet_param_info, no handle needed) holds the reference's 148 tensors in state_dict
  order with their shapes, 4,349,284 values, at aligned offsets.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from cld_amd import synth
from oracle import cld_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = [
    ("model.downs.0.0.blocks.0.block.0.weight", (3, 1, 2)),
    ("model.downs.1.1.blocks.1.block.0.weight", (7, 100, 4)),
    ("model.mid_block1.blocks.0.block.2.weight", (17,)),
    ("model.ups.0.0.blocks.1.block.2.bias", (5,)),
    ("model.downs.2.0.time_mlp.1.weight", (9, 40)),
    ("model.ups.1.0.residual_conv.weight", (2, 200, 0)),
    ("model.downs.0.2.conv.weight", (11, 12, 0)),
    ("model.ups.0.2.conv.weight", (3, 70, 1)),
    ("model.ups.1.2.conv.bias", (21,)),
    ("model.final_conv.1.weight", (1, 33, 0)),
    ("model.time_mlp.1.weight", (50, 6)),
    ("model.time_mlp.3.bias", (4,)),
]


def _setup(B=2):
    w = {k: torch.tensor(v, dtype=torch.float64) for k, v in synth.make_unet_weights(3, affine_jitter=True).items()}
    x = torch.from_numpy(synth.normal(1, "fd_x", (B, 52, 4))).double() * 2.0
    cond = torch.from_numpy(synth.make_inputs(B, 1)["cond_feat"]).double()
    t = torch.tensor([0, 63][:B])
    d = torch.from_numpy(synth.normal(1, "fd_d", (B, 52, 4))).double()
    return w, x, cond, t, d


def _loss(w, x, cond, t, d):
    return float((O.unet_forward(w, x, cond, t) * d).sum())


def test_fp64_oracle_autograd_matches_finite_differences():
    torch.manual_seed(0)
    w, x, cond, t, d = _setup()
    wg = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    xg, cg = x.clone().requires_grad_(True), cond.clone().requires_grad_(True)
    (O.unet_forward(wg, xg, cg, t) * d).sum().backward()
    h = 1e-5
    checks = [(wg[k].grad[idx], w[k], idx) for k, idx in ENTRIES]
    checks += [(xg.grad[1, 30, 2], x, (1, 30, 2)), (cg.grad[0, 17], cond, (0, 17))]
    for g, tensor, idx in checks:
        old = float(tensor[idx])
        tensor[idx] = old + h
        fp = _loss(w, x, cond, t, d)
        tensor[idx] = old - h
        fm = _loss(w, x, cond, t, d)
        tensor[idx] = old
        fd = (fp - fm) / (2 * h)
        assert abs(float(g) - fd) <= 1e-6 * max(1.0, abs(fd)), (idx, float(g), fd)


def test_parameter_table_is_the_reference_state_dict():
    from cld_amd import _lib
    from cld_amd.engine import unet_param_table
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    table, nflat = unet_param_table(_lib.load(), None)
    ref = synth.make_unet_weights(0)
    assert [n for n, *_ in table] == list(ref)
    assert len(table) == 148 and sum(n for _, _, n, _ in table) == 4349284
    end = 0
    for name, off, n, shape in table:
        assert off % 64 == 0 and off >= end
        assert shape == ref[name].shape and n == ref[name].size
        end = off + n
    assert nflat >= end
    lib = _lib.load()
    assert lib.cld_unet_param_info(None, 148, None, None, None, None, None) == -1
    assert lib.cld_unet_tape_bytes(None, 3) == 3 * lib.cld_unet_tape_bytes(None, 1) > 0
