"""The realism-deviation kernels (csrc/realism_kernels.hip: cld_realism_terms, cld_sort_f32, cld_wasserstein_f32) and
`cld_amd.metrics.RealismDeviation` on the device.

The sort and the terms are compared bit for bit: with np.sort (NaN positions equal) and with tests/realism_cases.terms.
The distances are compared with tests/realism_cases.w1 on the device-sorted inputs cast to float64.  Every term is non-negative, so any
summation order is within (n - 1) 2^-53 relative of any other; the bar is |y - ref| <= (nu + nv + 8) 2^-52 ref (realism_cases.bar),
derived and not tuned.  tests/golden/realism.npz holds the reference's own values (torch + scipy; tests/tools/record_realism_golden.py).
Every test runs in both precision modes of the library; the kernels are plain fp32 / fp64 in both, so the results are the same bits.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import realism_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(precision):
    from cld_amd.engine import Engine
    return Engine(n_timesteps=10, device="cuda:0", precision=precision)          # no weights: none of this needs any


@pytest.fixture(scope="module")
def gold():
    return RC.load_golden()


def tile():
    from cld_amd import _lib
    return int(_lib.load().cld_debug_sort_items_per_block())


def sort_sizes():
    P = tile()
    return [1, 2, 63, 64, 65, 255, 256, 257, P - 1, P, P + 1, 3 * P + 17, 2 ** 20 + 3]


_CONTENTS = {}


def contents(n):
    if n not in _CONTENTS:
        _CONTENTS[n] = RC.sort_contents(n)
    return _CONTENTS[n]


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def within(y, ref, nu, nv):
    print(f"y = {y!r} ref = {ref!r} |y - ref| / ref = {abs(y - ref) / ref if ref else abs(y - ref):.3e} bar = {RC.bar(nu, nv):.3e}")
    return abs(y - ref) <= RC.bar(nu, nv) * ref


# ---------------------------------------------------------------- sort
@pytest.mark.parametrize("k", range(13))
def test_sort_equals_numpy_at_every_size_and_content(eng, k):
    n = sort_sizes()[k]
    for name, x in contents(n).items():
        assert x.dtype == np.float32 and x.shape == (n,)
        d = torch.from_numpy(x).cuda()
        out = eng.sort(d)
        got, want = out.cpu().numpy(), np.sort(x)
        assert np.array_equal(got, want, equal_nan=True), f"n = {n}, {name}: first difference at {np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4]}"
        assert np.array_equal(bits(d), x.view(np.uint32)), "the input was written to"
        if name == "neg_zero_denormal":          # moved as bits: the denormals survive, and the zeros keep their count per sign
            assert np.array_equal(np.sort(got.view(np.uint32)), np.sort(x.view(np.uint32)))


@pytest.mark.parametrize("k", (4, 9, 11, 12))
def test_sort_in_place_and_twice_are_the_same_bits(eng, k):
    n = sort_sizes()[k]
    for name in ("normal", "inf_nan", "byte3", "two_values"):
        x = contents(n)[name]
        d = torch.from_numpy(x).cuda()
        a, b = eng.sort(d), eng.sort(d)
        assert np.array_equal(bits(a), bits(b)), f"n = {n}, {name}: two runs differ"
        inplace = d.clone()
        r = eng.sort(inplace, out=inplace)
        assert r.data_ptr() == inplace.data_ptr() and np.array_equal(bits(inplace), bits(a)), f"n = {n}, {name}: in place differs"
        assert np.array_equal(a.cpu().numpy(), np.sort(x), equal_nan=True)


# ---------------------------------------------------------------- terms
@pytest.mark.parametrize("M,T", [(1, 52), (3, 52), (65, 52), (5, 2)])
def test_terms_equal_the_numpy_restatement_bit_for_bit(eng, M, T):
    sa = RC.make_sa(M, 21 + M, "terms")[:, :T].copy()
    sa[0, 0, 4] = np.float32(1e-41)                                  # a denormal difference and quotient are not flushed
    sa[0, 1, 4] = np.float32(3e-41)
    want = RC.terms(sa, RC.DT)
    got = eng.realism_terms(torch.from_numpy(sa).cuda(), RC.DT)
    for name, g, w in zip(RC.NAMES, got, want):
        assert g.shape == w.shape and np.array_equal(bits(g), w.view(np.uint32)), f"{name} at M = {M}, T = {T}"
    # NULL outputs: the others are written, the sentinel around them is not
    for keep in range(3):
        outs = [torch.full((w.size + 2,), -7.0, device="cuda") if i == keep else None for i, w in enumerate(want)]
        eng.realism_terms(torch.from_numpy(sa).cuda(), RC.DT, out=outs)
        o = outs[keep].cpu().numpy()
        assert np.array_equal(o[:-2].view(np.uint32), want[keep].view(np.uint32)) and (o[-2:] == -7.0).all()
    other = eng.realism_terms(torch.from_numpy(sa).cuda(), 0.25)[2]
    assert np.array_equal(bits(other), RC.terms(sa, 0.25)[2].view(np.uint32))


# ---------------------------------------------------------------- distance
def device_distance(eng, u, v):
    """-> (device value, restatement on the device-sorted inputs, nu, nv)."""
    us, vs = eng.sort(torch.from_numpy(u).cuda()), eng.sort(torch.from_numpy(v).cuda())
    y = eng.wasserstein_distance(us, vs, presorted=True)
    assert y.dtype == torch.float64 and y.dim() == 0 and y.is_cuda
    return float(y.cpu()), RC.w1(us.cpu().numpy().astype(np.float64), vs.cpu().numpy().astype(np.float64)), u.size, v.size


@pytest.mark.parametrize("name", list(RC.distance_cases()))
def test_distance_is_within_the_bar_of_the_restatement(eng, name):
    u, v = RC.distance_cases()[name]
    y, ref, nu, nv = device_distance(eng, u, v)
    assert ref > 0.0 and within(y, ref, nu, nv)
    y2 = float(eng.wasserstein_distance(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()).cpu())         # sorts by itself
    assert y2 == y
    ys, _, _, _ = device_distance(eng, v, u)                                                                    # symmetric
    assert within(ys, ref, nu, nv)


def test_identical_samples_give_exactly_zero(eng):
    for n in (1, 64, 4097, 2 ** 18 + 1):
        x = torch.from_numpy(contents(2 ** 20 + 3)["normal"][:n].copy()).cuda()
        assert float(eng.wasserstein_distance(x, x.flip(0).contiguous()).cpu()) == 0.0
    t = torch.from_numpy(RC.distance_cases()["ties_4096_4096"][0]).cuda()
    assert float(eng.wasserstein_distance(t, t.clone()).cpu()) == 0.0


def test_a_power_of_two_shift_comes_back(eng):
    u, v, c = RC.shift_case()
    y, ref, nu, nv = device_distance(eng, u, v)
    assert ref == c and within(y, c, nu, nv)
    y, ref, nu, nv = device_distance(eng, u, v[:-7].copy())          # the CDF form on nearly the same pair
    assert within(y, ref, nu, nv)


def test_nan_in_either_sample_gives_nan(eng):
    u, v = (a.copy() for a in RC.distance_cases()["normal_999_1000"])
    for nu, nv in ((999, 1000), (999, 999)):                         # the CDF form and the paired form
        for side in (0, 1):
            a, b = u[:nu].copy(), v[:nv].copy()
            (a, b)[side][5] = np.nan
            assert np.isnan(float(eng.wasserstein_distance(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).cpu()))
    a, b = np.array([0.0, np.inf], np.float32), np.array([1.0, np.inf, np.inf], np.float32)      # inf - inf between neighbours
    assert np.isnan(float(eng.wasserstein_distance(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).cpu()))
    only = np.array([np.nan], np.float32)
    assert np.isnan(float(eng.wasserstein_distance(torch.from_numpy(only).cuda(), torch.from_numpy(u).cuda()).cpu()))


def test_two_runs_of_the_distance_are_the_same_bits(eng):
    for name in ("normal_262145_262139", "normal_4096_4096", "ties_1000_777"):
        u, v = (torch.from_numpy(a).cuda() for a in RC.distance_cases()[name])
        a, b = eng.wasserstein_distance(u, v), eng.wasserstein_distance(u, v)
        assert np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64))


# ---------------------------------------------------------------- RealismDeviation
KEYS = ("wd_long", "wd_lat", "wd_jerk", "realism_deviation")


def as_bits(res):
    assert set(res) == set(KEYS)
    for k in KEYS:
        assert res[k].dtype == torch.float64 and res[k].dim() == 0 and res[k].is_cuda
    return np.array([float(res[k].cpu()) for k in KEYS], np.float64).view(np.uint64)


def fed(eng, sa_gt, sa_pred, **kw):
    from cld_amd.metrics import RealismDeviation
    m = RealismDeviation(eng, dt=RC.DT, **kw)
    m.add(torch.from_numpy(sa_gt).cuda(), torch.from_numpy(sa_pred).cuda())
    return m


@pytest.mark.parametrize("case", ("eq", "uneq"))
def test_realism_deviation_reproduces_the_golden(eng, gold, case):
    m = fed(eng, gold[f"{case}_sa_gt"], gold[f"{case}_sa_pred"])
    res = m.compute()
    v = m.values()
    for n in RC.NAMES:
        for side in ("gt", "pred"):
            assert np.array_equal(bits(v[side][n]), gold[f"{case}_{n}_{side}"].view(np.uint32)), (n, side)
    nu, nv = gold[f"{case}_lon_gt"].size, gold[f"{case}_lon_pred"].size
    for k, want in zip(KEYS[:3], gold[f"{case}_wd"]):
        assert within(float(res[k].cpu()), float(want), nu, nv), k
    assert within(float(res["realism_deviation"].cpu()), float(gold[f"{case}_realism_deviation"]), nu, nv)


def test_uneven_adds_across_a_doubling_equal_one_add(eng):
    gt, pred = RC.make_sa(23, 31, "gt"), RC.make_sa(23, 32, "pred")
    one = fed(eng, gt, pred)
    m = None
    for lo, hi in ((0, 2), (2, 9), (9, 23)):
        if m is None:
            m = fed(eng, gt[lo:hi], pred[lo:hi], capacity=3 * RC.T)          # 2 rows fit, the second add overflows: 156 -> 468 -> 1196
        else:
            m.add(torch.from_numpy(gt[lo:hi]).cuda(), torch.from_numpy(pred[lo:hi]).cuda())
    assert m._buf[("gt", "lon")].numel() > 3 * RC.T
    for side in ("gt", "pred"):
        for n in RC.NAMES:
            assert np.array_equal(bits(m.values()[side][n]), bits(one.values()[side][n]))
    assert np.array_equal(as_bits(m.compute()), as_bits(one.compute()))


def test_reset_add_values_and_two_runs(eng):
    gt, pred = RC.make_sa(9, 41, "gt"), RC.make_sa(6, 42, "pred")
    fresh = fed(eng, gt, pred)
    want = as_bits(fresh.compute())
    assert np.array_equal(as_bits(fresh.compute()), want), "two runs differ"
    m = fed(eng, pred, gt)
    m.reset()
    assert all(t.numel() == 0 for side in m.values().values() for t in side.values())
    m.add(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda())
    assert np.array_equal(as_bits(m.compute()), want), "reset() then add differs from a fresh instance"
    from cld_amd.metrics import RealismDeviation
    byval = RealismDeviation(eng, dt=RC.DT)
    for side, sa in (("gt", gt), ("pred", pred)):
        lon, lat, jerk = RC.terms(sa, RC.DT)
        byval.add_values(side, lon=torch.from_numpy(lon).cuda(), lat=lat, jerk=torch.from_numpy(jerk))
    assert np.array_equal(as_bits(byval.compute()), want), "add_values differs from add"
    ref = [RC.w1(*(np.sort(t) for t in (RC.terms(gt, RC.DT)[i], RC.terms(pred, RC.DT)[i]))) for i in range(3)]
    assert within(float(fresh.compute()["realism_deviation"].cpu()), (ref[0] + ref[1] + ref[2]) / 3.0, gt.size // 6, pred.size // 6)


def test_an_empty_side_raises(eng):
    from cld_amd.metrics import RealismDeviation
    m = RealismDeviation(eng, dt=RC.DT)
    with pytest.raises(ValueError):
        m.compute()
    m.add_values("gt", lon=[1.0, 2.0], lat=[1.0], jerk=[0.5])
    with pytest.raises(ValueError):
        m.compute()
    with pytest.raises(ValueError):
        m.add_values("logged", lon=[1.0])
    m.add_values("pred", lon=[1.5], lat=[2.0, 0.0], jerk=[0.5])
    assert float(m.compute()["wd_long"].cpu()) == RC.w1([1.0, 2.0], [1.5]) == 0.5


def test_both_precision_modes_give_the_same_bits():
    from cld_amd.engine import Engine
    u, v = RC.distance_cases()["normal_999_1000"]
    gt, pred = RC.make_sa(5, 51, "gt"), RC.make_sa(4, 52, "pred")
    res = []
    for mode in ("f32", "f16x2"):
        e = Engine(n_timesteps=10, device="cuda:0", precision=mode)
        d = e.wasserstein_distance(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()).cpu().numpy().view(np.uint64)
        res.append((int(d), as_bits(fed(e, gt, pred).compute()).tolist(), bits(e.sort(torch.from_numpy(u).cuda())).tolist()))
    assert res[0] == res[1]


# ---------------------------------------------------------------- status codes
def test_bad_arguments_return_status_codes(eng):
    """Bad arguments only: every call returns before a launch."""
    from cld_amd import _lib
    lib, h, st = eng.lib, eng._h, eng._stream()
    ARG, WS = -1, -3
    n = 1000
    x, y = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    need = int(lib.cld_sort_workspace_bytes(n))
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.cld_sort_f32(h, p(x), p(y), 0, p(ws), need, st) == ARG
    assert lib.cld_sort_f32(h, p(x), p(y), -5, p(ws), need, st) == ARG
    assert lib.cld_sort_f32(h, p(x), p(y), 2 ** 30 + 1, p(ws), need, st) == ARG
    assert lib.cld_sort_f32(h, None, p(y), n, p(ws), need, st) == ARG
    assert lib.cld_sort_f32(h, p(x), None, n, p(ws), need, st) == ARG
    assert lib.cld_sort_f32(None, p(x), p(y), n, p(ws), need, st) == ARG
    assert lib.cld_sort_f32(h, p(x), p(y), n, p(ws), need - 1, st) == WS
    assert lib.cld_sort_f32(h, p(x), p(y), n, None, need, st) == WS
    assert b"workspace" in lib.cld_last_error(h)
    out = torch.zeros((), dtype=torch.float64, device="cuda")
    wneed = int(lib.cld_wasserstein_workspace_bytes(n, n - 1))
    assert wneed > 0
    assert lib.cld_wasserstein_f32(h, p(x), 0, p(y), n, p(out), p(ws), need, st) == ARG
    assert lib.cld_wasserstein_f32(h, p(x), n, p(y), 0, p(out), p(ws), need, st) == ARG
    assert lib.cld_wasserstein_f32(h, None, n, p(y), n, p(out), p(ws), need, st) == ARG
    assert lib.cld_wasserstein_f32(h, p(x), n, None, n, p(out), p(ws), need, st) == ARG
    assert lib.cld_wasserstein_f32(h, p(x), n, p(y), n, None, p(ws), need, st) == ARG
    assert lib.cld_wasserstein_f32(h, p(x), n, p(y), n - 1, p(out), p(ws), wneed - 1, st) == WS
    assert lib.cld_wasserstein_f32(h, p(x), n, p(y), n - 1, p(out), None, wneed, st) == WS
    sa = torch.zeros(4, 52, 6, device="cuda")
    lon = torch.zeros(4 * 52, device="cuda")
    assert lib.cld_realism_terms(h, None, 4, 52, 0.1, p(lon), None, None, st) == ARG
    assert lib.cld_realism_terms(h, p(sa), 4, 52, 0.1, None, None, None, st) == ARG
    assert lib.cld_realism_terms(h, p(sa), 0, 52, 0.1, p(lon), None, None, st) == ARG
    assert lib.cld_realism_terms(h, p(sa), 4, 1, 0.1, p(lon), None, None, st) == ARG
    assert lib.cld_realism_terms(h, p(sa), 4, 52, 0.0, p(lon), None, None, st) == ARG
    assert lib.cld_realism_terms(h, p(sa), 4, 52, float("nan"), p(lon), None, None, st) == ARG
    assert lib.cld_realism_terms(h, p(sa), 4, 52, 0.1, p(lon), None, None, st) == 0
    torch.cuda.synchronize()
    assert float(out.cpu()) == 0.0 and not y.any() and not lon.any()
    with pytest.raises(_lib.CldError):
        eng.sort(torch.zeros(0))
    with pytest.raises(_lib.CldError):
        eng.realism_terms(torch.zeros(2, 1, 6), 0.1)
