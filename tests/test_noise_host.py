"""CPU tests of tests/noise_replica.py, the numpy restatement of the on-device generator (csrc/cld_kernels.h normal4) that
tests/test_gpu_noise.py holds every draw site of the library to.

Moments over seed 7, steps 0..99 and 64 x 52 rows (1.33 M values), each bar five standard errors of the estimate for independent N(0, 1)
values: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N), |m4 - 3| <= 5 sqrt(96 / N); the correlations between adjacent rows, between
the same row at adjacent steps and between components 0 / 1 and 2 / 3 of a row within 5 / sqrt(n) for their n.  Measured: mean -1.0e-4
(bar 4.3e-3), variance 0.9992 (1 +- 6.1e-3), fourth moment 2.996 (3 +- 4.2e-2), correlations 6.4e-4 (rows), 2.7e-4 (steps; bar 4.3e-3),
-2.1e-4 and 1.5e-4 (components; bar 8.7e-3).

Sensitivity of the GPU tests' bars, with the oracle: a noise tensor shifted by one row or by one step moves a 10-step chain by 34 and
29 times the chain bar 1e-3 max(1, max|x0|) (ten times is asserted), and a single draw by O(1) against the one-step bar 1e-4."""
import math

import numpy as np
import pytest
import torch

import noise_replica as R
from cld_amd import synth
from oracle import cld_oracle as O

SEED, STEPS, B = 7, 100, 64


@pytest.fixture(scope="module")
def draws():
    z = np.stack([R.step_noise(SEED, it, B) for it in range(STEPS)])       # [100, 64, 52, 4] float64
    return z.reshape(STEPS, B * 52, 4)


def _corr(a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    return float(np.corrcoef(a, b)[0, 1]), a.size


def test_integer_core_matches_the_published_splitmix64():
    """splitmix64's reference output stream for state 0 (Vigna's splitmix64.c: the state advances by the golden-ratio constant, the
    finaliser is what cld_kernels.h applies to state + constant): the first three outputs."""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    state, got = 0, []
    for _ in range(3):
        got.append(int(R.splitmix64(np.uint64(state))))
        state = (state + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    assert got == want


def test_u01_is_float32_and_inside_the_unit_interval():
    bits = np.array([0, 1 << 40, (1 << 63), 0xFFFFFFFFFFFFFFFF, ((1 << 23) + 1) << 40], dtype=np.uint64)
    u = R.u01(bits)
    assert u.dtype == np.float32
    assert u[0] == np.float32(0.5 / 16777216.0) and u[1] == np.float32(1.5 / 16777216.0) and u[2] == np.float32(0.5)      # 2^23 + 0.5: a tie, to even
    assert u[3] == np.float32(1.0)                       # 16777215.5 rounds to even in float32: log(1) = 0, a draw of exactly 0
    assert u[4] == np.float32((2 ** 23 + 2) / 16777216.0)  # 2^23 + 1.5 is a tie, to even
    assert np.isfinite(R.normal4(0, 0, np.arange(4))).all()


def test_keying():
    """(seed, step, row) are all live, a seed beyond 32 bits differs from its low word, and rows are taken modulo 2^32 as the kernels'
    `unsigned row` is."""
    rows = np.arange(8)
    base = R.normal4(7, 3, rows)
    assert np.array_equal(base, R.normal4(7, 3, rows))
    for other in (R.normal4(8, 3, rows), R.normal4(7, 4, rows), R.normal4(7, 3, rows + 1), R.normal4(2 ** 40 + 7, 3, rows)):
        assert not np.any(other == base)
    assert np.array_equal(R.normal4(7, 3, rows + 2 ** 32), base)
    assert np.array_equal(R.chain_noise(7, 2, 3)[1], R.step_noise(7, 1, 3).astype(np.float32))


def test_moments(draws):
    x = draws.reshape(-1)
    N = x.size
    assert N == STEPS * B * 52 * 4
    mean, var, m4 = float(x.mean()), float(x.var()), float(((x - x.mean()) ** 4).mean())
    print(f"\n[noise] N={N} mean {mean:.3e} (bar {5 / math.sqrt(N):.2e}) var {var:.5f} (1 +- {5 * math.sqrt(2 / N):.2e}) "
          f"m4 {m4:.4f} (3 +- {5 * math.sqrt(96 / N):.2e})")
    assert abs(mean) <= 5 / math.sqrt(N)
    assert abs(var - 1.0) <= 5 * math.sqrt(2.0 / N)
    assert abs(m4 - 3.0) <= 5 * math.sqrt(96.0 / N)


def test_correlations(draws):
    pairs = {"adjacent rows": (draws[:, :-1], draws[:, 1:]),
             "adjacent steps": (draws[:-1], draws[1:]),
             "components 0/1": (draws[..., 0], draws[..., 1]),
             "components 2/3": (draws[..., 2], draws[..., 3])}
    for name, (a, b) in pairs.items():
        c, n = _corr(a, b)
        print(f"\n[noise] correlation, {name}: {c:.3e} (bar {5 / math.sqrt(n):.2e}, n={n})")
        assert abs(c) <= 5 / math.sqrt(n), name


def test_a_shifted_noise_tensor_fails_the_bars_tenfold():
    """What the GPU tests would see if a draw site were off by one row or one step: the oracle's 10-step chain on Z shifted that way
    against the chain on Z, over the chain bar; and the draws themselves over the one-step bar."""
    n, Bc, seed = 10, 6, 7
    w = O.to_torch(synth.make_unet_weights(0, affine_jitter=True))
    sched = O.schedule(n)
    inp, nz = synth.make_inputs(Bc, 3), synth.make_noise(Bc, n, 5)
    x_T, cond = torch.from_numpy(nz["x_T"]), torch.from_numpy(inp["cond_feat"])
    Z = R.chain_noise(seed, n, Bc)
    rows = np.stack([R.normal4(seed, it, np.arange(Bc * 52) + 1).reshape(Bc, 52, 4) for it in range(n)]).astype(np.float32)
    steps = np.stack([R.step_noise(seed, it + 1, Bc) for it in range(n)]).astype(np.float32)
    torch.set_num_threads(8)
    ref = O.sample(w, sched, x_T, torch.from_numpy(Z), cond)["pred_traj"]
    bar = 1e-3 * max(1.0, float(ref.abs().max()))
    for name, Zs in (("row + 1", rows), ("step + 1", steps)):
        got = O.sample(w, sched, x_T, torch.from_numpy(Zs), cond)["pred_traj"]
        d = float((got - ref).abs().max())
        print(f"\n[noise] Z shifted by {name}: chain moves {d:.3g} = {d / bar:.0f} x the chain bar; draws move {np.abs(Zs - Z).max():.2f}")
        assert d >= 10 * bar and float(np.abs(Zs[0] - Z[0]).max()) >= 10 * 1e-4
