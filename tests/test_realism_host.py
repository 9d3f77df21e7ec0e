"""The realism deviation on the CPU: the float64 restatement of tests/realism_cases.py against tests/golden/realism.npz (recorded from
torch + scipy as the reference evaluates them; tests/tools/record_realism_golden.py) and against scipy where it is installed, and the
C-ABI's bookkeeping.  The device kernels are held to the same restatement in tests/test_gpu_realism.py."""
import os
import re

import numpy as np
import pytest

from tests import realism_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("eq", "uneq")


@pytest.fixture(scope="module")
def gold():
    return RC.load_golden()


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_golden_distances(gold, case):
    """Two float64 evaluations of the same sums: scipy's order differs in summation and in how it forms the CDF difference."""
    wd = [RC.w1(gold[f"{case}_{n}_gt"], gold[f"{case}_{n}_pred"]) for n in RC.NAMES]
    for got, want in zip(wd, gold[f"{case}_wd"]):
        assert abs(got - want) <= 1e-12 * want
    dev = (wd[0] + wd[1] + wd[2]) / 3.0
    assert abs(dev - float(gold[f"{case}_realism_deviation"])) <= 1e-12 * dev


@pytest.mark.parametrize("case", CASES)
def test_terms_equal_the_golden_arrays_bit_for_bit(gold, case):
    inputs = RC.golden_inputs()[case]
    for side, sa in zip(("gt", "pred"), inputs):
        assert np.array_equal(sa.view(np.uint32), gold[f"{case}_sa_{side}"].view(np.uint32)), "golden_inputs() moved: record again"
        for n, got in zip(RC.NAMES, RC.terms(sa, RC.DT)):
            want = gold[f"{case}_{n}_{side}"]
            assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (case, side, n)
    assert gold["uneq_lon_gt"].size != gold["uneq_lon_pred"].size and gold["eq_lon_gt"].size == gold["eq_lon_pred"].size


def test_paired_form_equals_the_cdf_form_on_equal_sizes(gold):
    pairs = [(u, v) for u, v in RC.distance_cases().values() if u.size == v.size]
    pairs += [(gold[f"eq_{n}_gt"], gold[f"eq_{n}_pred"]) for n in RC.NAMES]
    u, v, c = RC.shift_case()
    assert RC.w1_paired(u, v) == c
    pairs.append((u, v))
    assert len(pairs) >= 6
    for u, v in pairs:
        a, b = RC.w1_paired(u, v), RC.w1(u, v)
        assert abs(a - b) <= RC.bar(u.size, v.size) * b
    x = RC.sort_contents(1000)["normal"]
    assert RC.w1_paired(x, x) == 0.0 and RC.w1(x, x) == 0.0


def test_cdf_form_equals_scipy_on_every_case():
    stats = pytest.importorskip("scipy.stats")
    cases = dict(RC.distance_cases())
    u, v, _ = RC.shift_case()
    cases["shift"] = (u, v)
    for name, (u, v) in cases.items():
        want = float(stats.wasserstein_distance(u.astype(np.float64), v.astype(np.float64)))
        got = RC.w1(u, v)
        # scipy subtracts two rounded CDF values (each within 2^-53 of a number <= 1) per step: up to 2^-52 of the samples' range in all
        span = float(max(u.max(), v.max()) - min(u.min(), v.min()))
        assert abs(got - want) <= 1e-12 * want + 2.0 ** -51 * span, name


def test_nan_and_inf_minus_inf_give_nan():
    u = np.array([0.0, 1.0, np.nan], np.float32)
    v = np.array([0.5, 2.0], np.float32)
    assert np.isnan(RC.w1(u, v)) and np.isnan(RC.w1(v, u)) and np.isnan(RC.w1_paired(u, u))
    assert np.isnan(RC.w1(np.array([0.0, np.inf], np.float32), np.array([1.0, np.inf, np.inf], np.float32)))


def test_sort_contents_hold_what_they_are_named_for():
    c = RC.sort_contents(4097)
    for byte in range(4):
        bits = c[f"byte{byte}"].view(np.uint32)
        assert len(np.unique(bits)) > 100 and np.all((bits ^ bits[0]) & ~np.uint32(0xff << 8 * byte) == 0) and np.isfinite(c[f"byte{byte}"]).all()
    z = c["neg_zero_denormal"]
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    assert ((np.abs(z) > 0) & (np.abs(z) < np.finfo(np.float32).tiny)).any()
    s = c["inf_nan"]
    assert np.isposinf(s).any() and np.isneginf(s).any() and (np.isnan(s) & np.signbit(s)).any() and (np.isnan(s) & ~np.signbit(s)).any()
    assert len(np.unique(c["two_values"])) == 2 and len(np.unique(c["all_equal"])) == 1


def test_header_binding_and_documents_name_the_realism_entry_points():
    from cld_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cld.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym, nargs in (("cld_sort_workspace_bytes", 1), ("cld_sort_f32", 7), ("cld_wasserstein_workspace_bytes", 2),
                       ("cld_wasserstein_f32", 9), ("cld_realism_terms", 9), ("cld_debug_sort_items_per_block", 0)):
        assert sym in _lib.SIGNATURES and len(_lib.SIGNATURES[sym][1]) == nargs and re.search(r"\b" + sym + r"\s*\(", hdr) and sym in doc
    assert "## Realism deviation" in doc
    not_built = [l for l in doc.splitlines() if l.startswith("Not built:")]
    assert not_built and all("Wasserstein" not in l for l in not_built)


def test_size_queries_need_no_device():
    from cld_amd import _lib
    lib = _lib.load()
    P = lib.cld_debug_sort_items_per_block()
    assert P >= 256 and P % 64 == 0
    assert lib.cld_sort_workspace_bytes(0) == 0 and lib.cld_sort_workspace_bytes(2 ** 30 + 1) == 0
    one, two = lib.cld_sort_workspace_bytes(P), lib.cld_sort_workspace_bytes(P + 1)
    assert one >= 4 * P and two > one                      # a second copy of the keys, and counts per tile
    assert lib.cld_sort_workspace_bytes(2 ** 30) >= 2 ** 32
    assert lib.cld_wasserstein_workspace_bytes(0, 5) == 0 and lib.cld_wasserstein_workspace_bytes(5, 0) == 0
    assert lib.cld_wasserstein_workspace_bytes(1, 1) >= 8
    assert lib.cld_wasserstein_workspace_bytes(2 ** 30, 2 ** 30 - 1) > lib.cld_wasserstein_workspace_bytes(2 ** 30, 2 ** 30) > 0
