"""Inputs and the float64 restatement of the realism deviation (include/cld.h `cld_realism_terms`, `cld_sort_f32`, `cld_wasserstein_f32`;
the reference: src/trainers/guide_dm_trainer.py:204-295 with scipy.stats.wasserstein_distance).

terms(sa, dt)    numpy fp32, operation for operation: a copy, one product, one difference and one division by float32(dt).
w1(u, v)         the CDF form on float64 copies: over the merged values a_k, |cu_k nv - cv_k nu| (a_{k+1} - a_k) / (nu nv) with the
                 right-continuous (inclusive) counts, which are exact integers; a run of equal values contributes at its last element only.
w1_paired(u, v)  mean |sort(u) - sort(v)| for equal sizes.
Every term of both sums is non-negative, so any summation order of the same terms is within (n - 1) 2^-53 relative of any other:
bar(nu, nv) = (nu + nv + 8) 2^-52 relative is what the device result is held to (the 8 covers the roundings of the counts, the
products and the one division on either side).
"""
import os

import numpy as np

from cld_amd import synth

T = 52
DT = 0.1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "realism.npz")
NAMES = ("lon", "lat", "jerk")


def bar(nu: int, nv: int) -> float:
    return (nu + nv + 8) * 2.0 ** -52


def terms(sa, dt):
    """sa [M,T,6] -> (lon [M T], lat [M T], jerk [M (T-1)]) in fp32, as test_step forms them."""
    sa = np.asarray(sa, np.float32)
    lon = sa[..., 4]
    lat = sa[..., 2] * sa[..., 5]
    jerk = (lon[:, 1:] - lon[:, :-1]) / np.float32(dt)
    assert lat.dtype == np.float32 and jerk.dtype == np.float32
    return lon.reshape(-1).copy(), lat.reshape(-1), jerk.reshape(-1)


def w1(u, v) -> float:
    u, v = np.sort(np.asarray(u, np.float64).reshape(-1)), np.sort(np.asarray(v, np.float64).reshape(-1))
    nu, nv = u.size, v.size
    a = np.sort(np.concatenate([u, v]))
    with np.errstate(invalid="ignore"):
        delta = np.diff(a)
        cu = np.searchsorted(u, a[:-1], "right").astype(np.int64)
        cv = np.searchsorted(v, a[:-1], "right").astype(np.int64)
        if np.isnan(delta).any():
            return float("nan")
        return float(np.sum(np.abs(cu * nv - cv * nu).astype(np.float64) * delta) / (float(nu) * float(nv)))


def w1_paired(u, v) -> float:
    u, v = np.sort(np.asarray(u, np.float64).reshape(-1)), np.sort(np.asarray(v, np.float64).reshape(-1))
    assert u.size == v.size
    with np.errstate(invalid="ignore"):
        return float(np.sum(np.abs(u - v)) / float(u.size))


def make_sa(M: int, seed: int, name: str = "sa"):
    """[M,52,6] scaled state-and-action rows in synth's manner: unit-scale columns, the acceleration column a smooth profile plus noise
    so that its differences (the jerk) spread over a range of magnitudes."""
    sa = synth.normal(seed, name, (M, T, 6)).astype(np.float32)
    t = np.arange(T, dtype=np.float32)[None, :]
    ph = synth.uniform(seed, name + ".phase", (M, 1), 0.0, 6.28).astype(np.float32)
    sa[..., 4] = (np.sin(0.2 * t + ph) * synth.uniform(seed, name + ".amp", (M, 1), 0.2, 1.5).astype(np.float32)
                  + 0.05 * sa[..., 4]).astype(np.float32)
    return sa


def golden_inputs():
    """The two recorded cases: equal rows (16 / 16) and a pred side with fewer rows (16 / 11) against the same ground truth."""
    gt = make_sa(16, 11, "gt")
    return {"eq": (gt, make_sa(16, 12, "pred")), "uneq": (gt, make_sa(11, 13, "pred"))}


def load_golden(path=GOLDEN):
    """The fixture's arrays; the ground-truth side of "uneq" is that of "eq" and is stored once."""
    with np.load(path) as z:
        g = {k: z[k] for k in z.files if k != "meta"}
    for k in [k for k in g if k.startswith("eq_") and k.endswith("_gt")]:
        g["un" + k] = g[k]
    return g


def _draw(seed, name, n):
    return synth.normal(seed, name, (n,)).astype(np.float32)


def distance_cases():
    """name -> (u, v) fp32 samples, unsorted: the sizes of the issue, ties, exact sums."""
    c = {}
    for nu, nv in ((1, 1), (1, 1000), (64, 65), (999, 1000), (4096, 4096), (2 ** 18 + 1, 2 ** 18 - 5)):
        c[f"normal_{nu}_{nv}"] = (_draw(3, f"u{nu}", nu), (_draw(4, f"v{nv}", nv) * np.float32(1.25) + np.float32(0.3)).astype(np.float32))
    for nu, nv in ((4096, 4096), (1000, 777), (65, 5000)):
        c[f"ties_{nu}_{nv}"] = (np.floor(synth.uniform(5, f"tu{nu}", (nu,), 0.0, 7.0)).astype(np.float32),
                                np.floor(synth.uniform(6, f"tv{nv}", (nv,), 0.0, 7.0)).astype(np.float32) - np.float32(1.0))
    c["ties_signed_zero"] = (np.array([-0.0, 0.0, 0.0, 1.0, 1.0, 2.0], np.float32), np.array([0.0, -0.0, 1.0, 3.0], np.float32))
    return c


def shift_case(n: int = 3000, c: float = 0.25):
    """u multiples of 2^-10 below 1, v = u + c with c a power of two: every |u_i - v_i| is c exactly and so is every partial sum."""
    u = (np.floor(synth.uniform(7, "shift", (n,), -1.0, 1.0) * 1024.0) / 1024.0).astype(np.float32)
    return u, (u + np.float32(c)).astype(np.float32), c


def sort_contents(n: int, seed: int = 0):
    """name -> fp32 array of n values: the contents the sort is tried on at every size."""
    rng_u = synth.uniform(seed, f"sortu{n}", (n,), 0.0, 1.0)
    x = _draw(seed, f"sort{n}", n)
    out = {"normal": x, "all_equal": np.full(n, 1.5, np.float32),
           "two_values": np.where(rng_u < 0.5, np.float32(-2.0), np.float32(3.0)).astype(np.float32),
           "sorted": np.sort(x), "reversed": np.sort(x)[::-1].copy()}
    base = 0x3f123456                                            # bit 23 clear: with any top byte the exponent stays below 0xff (finite)
    for byte in range(4):                                       # keys that differ in one byte only: a broken pass shows here
        b = np.floor(rng_u * 256.0).astype(np.uint32) << np.uint32(8 * byte)
        out[f"byte{byte}"] = (np.uint32(base & ~(0xff << 8 * byte)) | b).astype(np.uint32).view(np.float32)
    sel = np.floor(rng_u * 8.0).astype(np.int64)
    den = np.array([1e-45, -1e-45, 1e-40, -1e-40], np.float32)[sel % 4]
    out["neg_zero_denormal"] = np.choose(sel, [-np.abs(x), np.full(n, -0.0, np.float32), np.zeros(n, np.float32), den, den,
                                               -np.abs(x) * np.float32(1e-38), x, np.full(n, -0.0, np.float32)]).astype(np.float32)
    special = np.array([np.inf, -np.inf, np.nan, -np.nan, 0.0, 1.0], np.float32)
    special[3] = np.array([0xffc00001], np.uint32).view(np.float32)[0]           # a NaN with the sign bit and a payload
    out["inf_nan"] = np.where(sel < 6, special[np.minimum(sel, 5)], x).astype(np.float32)
    return out
