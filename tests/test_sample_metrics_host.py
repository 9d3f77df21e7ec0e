"""Host-side checks of the open-loop sample metrics (ADE / FDE / APD / FPD): the float64 yardstick (tests/sample_metrics_yardstick.py)
against the recording made from the reference's own four functions (tests/golden/sample_metrics.npz,
tests/tools/record_sample_metrics_golden.py), upstream's FPD quirk, the mutants that show the recorded cases discriminate, and the
third ctypes table against include/cld_eval.h."""
import os
import re

import numpy as np
import pytest

from tests import sample_metrics_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["n5", "n1"]
PER_AGENT = ("ade_mean", "ade_min", "fde_mean", "fde_min", "apd_mean", "apd_max", "fpd_mean", "fpd_max")      # columns 0 .. 7


def recorded(golden, case):
    meta, g = golden("sample_metrics")
    rec = {k[len(case) + 1:]: v for k, v in g.items() if k.startswith(case + "_")}
    rec["per_agent"] = np.stack([rec[k] for k in PER_AGENT], axis=1)
    return meta, rec


def miss(res, rec):
    """How far a yardstick result lies from the recording: the largest relative error over the eight keys, the per-agent columns and
    the per-sample ade / fde (inf where one is non-zero at a recorded zero); inf when a best-sample index differs from the first
    minimum of the recorded per-sample values."""
    if not (np.array_equal(res["index"][:, 0], np.argmin(rec["ade"], axis=1)) and np.array_equal(res["index"][:, 1], np.argmin(rec["fde"], axis=1))):
        return float("inf")
    return max(Y.rel_err(res["means"][:8], rec["keys"]), Y.rel_err(res["per_agent"][:, :8], rec["per_agent"]),
               Y.rel_err(res["ade"], rec["ade"]), Y.rel_err(res["fde"], rec["fde"]))


@pytest.mark.parametrize("case", CASES)
def test_yardstick_matches_the_reference_recording(golden, case):
    """The eight keys, every per-agent array and the per-sample ade / fde within 2e-6 relative; a yardstick zero is a recorded zero."""
    meta, rec = recorded(golden, case)
    res = Y.metrics(rec["pred"], rec["gt"], rec["avail"])
    for name, got, want in (("keys", rec["keys"], res["means"][:8]), ("per_agent", rec["per_agent"], res["per_agent"][:, :8]),
                            ("ade", rec["ade"], res["ade"]), ("fde", rec["fde"], res["fde"])):
        err = Y.rel_err(got, want)                       # the recording measured against the yardstick: zeros of the yardstick are exact
        print(f"{case} {name}: {err:.2e}")
        assert err <= Y.BAR, (case, name, err)
        assert np.array_equal(np.asarray(got) == 0, np.asarray(want) == 0), (case, name)
    assert miss(res, rec) <= Y.BAR
    assert list(Y.keys(res)) == meta["keys"] == list(Y.UPSTREAM_KEYS)


def test_the_recording_holds_the_cases_it_is_meant_to(golden):
    meta, rec = recorded(golden, "n5")
    _, rec1 = recorded(golden, "n1")
    assert (meta["B"], meta["N"], meta["T"]) == (6, 5, 52) and meta["cases"] == CASES
    assert rec["pred"].shape == (6, 5, 52, 2) and rec["gt"].shape == (6, 52, 2) and rec["avail"].shape == (6, 52)
    assert rec1["pred"].shape == (6, 1, 52, 2) and np.array_equal(rec1["pred"][:, 0], rec["pred"][:, 0])
    assert all(rec[k].dtype == np.float32 for k in ("pred", "gt", "avail"))
    a = rec["avail"]
    assert np.array_equal(a, Y.availability_patterns(52))
    assert a[0].all() and a[1, :26].all() and not a[1, 26:].any() and not a[2].any() and not a[3, 13:26].any() and a[3].sum() == 39
    assert a[4].sum() == 1 and a[4, 0] == 1 and a[5].sum() == 1 and a[5, 51] == 1
    assert 3.0 < np.abs(rec["gt"]).max() < 100.0                                    # O(10 m)
    res = Y.metrics(rec["pred"], rec["gt"], a)
    assert res["last"].tolist() == [51, 25, 0, 51, 0, 51]
    # nothing available: every error is exactly 0, a tie over all samples, first index
    assert not rec["ade"][2].any() and not rec["fde"][2].any() and res["index"][2].tolist() == [0, 0, 0, 0]
    # one sample: no pair, diversity exactly 0; the mean over the samples is the best sample
    assert not any(rec1[k].any() for k in ("apd_mean", "apd_max", "fpd_mean", "fpd_max"))
    assert np.array_equal(rec1["fde_mean"], rec1["fde_min"])


def test_recorded_fpd_is_the_y_coordinate_over_time_and_not_the_last_step_distance(golden):
    """Upstream's batch_final_diversity takes pred[..., -1] -- the last coordinate -- and the norm over time.  The recording pins it."""
    _, rec = recorded(golden, "n5")
    p = rec["pred"].astype(np.float64)
    y_over_time = np.sqrt(((p[:, :, None, :, 1] - p[:, None, :, :, 1]) ** 2).sum(axis=-1)).reshape(6, -1)
    last_step = np.sqrt(((p[:, :, None, -1] - p[:, None, :, -1]) ** 2).sum(axis=-1)).reshape(6, -1)
    assert Y.rel_err(rec["fpd_mean"], y_over_time.mean(axis=1)) <= Y.BAR and Y.rel_err(rec["fpd_max"], y_over_time.max(axis=1)) <= Y.BAR
    for b in range(6):
        assert abs(rec["fpd_mean"][b] - last_step[b].mean()) > 0.05 * rec["fpd_mean"][b]
        assert abs(rec["fpd_max"][b] - last_step[b].max()) > 0.05 * rec["fpd_max"][b]
    res = Y.metrics(rec["pred"], rec["gt"], rec["avail"])
    assert Y.rel_err(res["per_agent"][:, 8], last_step.mean(axis=1)) <= 1e-14 and Y.rel_err(res["per_agent"][:, 9], last_step.max(axis=1)) <= 1e-14


@pytest.mark.parametrize("variant", Y.VARIANTS)
def test_every_mutant_misses_the_recorded_cases(golden, variant):
    """Each mis-statement of the formulas lies further from the recording than the bar: the recorded cases tell them apart."""
    _, rec = recorded(golden, "n5")
    res = Y.metrics(rec["pred"], rec["gt"], rec["avail"], variant=variant)
    m = miss(res, rec)
    print(f"{variant}: {m:.3e}")
    assert m > 1000 * Y.BAR


def test_yardstick_decisions_on_exact_inputs():
    """Small dyadic coordinates: identical samples, a tie, nothing available, a non-finite value."""
    T = 4
    gt = np.zeros((1, T, 2), np.float32)
    pred = np.zeros((1, 4, T, 2), np.float32)
    pred[0, 0, :, 0], pred[0, 1, :, 0], pred[0, 2, :, 0], pred[0, 3, :, 1] = 2.0, 0.5, 0.75, -0.5      # ade 2, 0.5, 0.75, 0.5: a tie of 1 and 3
    res = Y.metrics(pred, gt, np.ones((1, T), bool))
    assert res["ade"][0].tolist() == [2.0, 0.5, 0.75, 0.5] and res["index"][0].tolist() == [1, 1, 3, 0]
    assert Y.metrics(pred, gt, np.ones((1, T), bool), variant="last_tie")["index"][0, 0] == 3
    res0 = Y.metrics(pred, gt, np.zeros((1, T), bool))
    assert res0["last"][0] == 0 and not res0["per_agent"][0, :4].any() and res0["index"][0].tolist() == [0, 0, 0, 0]
    same = np.repeat(pred[:, :1], 2, axis=1)
    assert not Y.metrics(same, gt, np.ones((1, T)))["per_agent"][0, 4:].any()
    pred[0, 2, 1, 1] = np.nan
    assert Y.metrics(pred, gt, np.ones((1, T)))["index"][0, 3] == 1


def _header():
    return open(os.path.join(ROOT, "include", "cld_eval.h")).read()


def test_eval_header_matches_the_third_signature_table_and_the_others_keep_their_size():
    """include/cld_eval.h <=> _lib.EVAL_SIGNATURES <=> the library's exports, in the manner of test_lane_host.py; include/cld.h and
    include/cld_lane.h hold none of the names and the first two tables keep 88 and 3."""
    from cld_amd import _lib
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cld_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.EVAL_SIGNATURES) == {"cld_sample_metrics_workspace_bytes", "cld_sample_metrics", "cld_debug_sample_metrics_max_blocks"}
    for name, (_, args) in _lib.EVAL_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1).strip()
        assert (0 if proto == "void" else len(proto.split(","))) == len(args), name
    assert '#include "cld.h"' in code
    others = open(os.path.join(ROOT, "include", "cld.h")).read() + open(os.path.join(ROOT, "include", "cld_lane.h")).read()
    assert len(_lib.SIGNATURES) == 88 and len(_lib.LANE_SIGNATURES) == 3
    assert not any(n in _lib.SIGNATURES or n in _lib.LANE_SIGNATURES or n in others for n in _lib.EVAL_SIGNATURES)
    # the column constants, in order, and the reach
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bCLD_SM_([A-Z_]+) = (\d+)", code)}
    assert list(enum.values()) == list(range(10)) and int(re.search(r"#define CLD_SM_COLS (\d+)", code).group(1)) == 10 == len(_lib.SAMPLE_METRIC_COLS)
    assert list(enum) == ["ADE_MEAN", "ADE_MIN", "FDE_MEAN", "FDE_MIN", "APD_MEAN", "APD_MAX", "FPD_MEAN", "FPD_MAX", "LAST_PD_MEAN", "LAST_PD_MAX"]
    assert _lib.SAMPLE_METRIC_COLS == Y.COLS and _lib.SAMPLE_METRIC_COLS[:8] == Y.UPSTREAM_KEYS
    assert int(re.search(r"#define CLD_SM_MAX_SAMPLES (\d+)", code).group(1)) == _lib.SAMPLE_METRICS_MAX_SAMPLES == 256
    assert int(re.search(r"#define CLD_SM_MAX_POINTS (\d+)", code).group(1)) == _lib.SAMPLE_METRICS_MAX_POINTS == 8192
    # the header states the two rules nobody should "fix" unnoticed
    assert "QUIRK" in hdr and "divide by T" in hdr
    if os.path.exists(_lib.LIB_PATH):                                      # where the library is built: it exports all three
        lib = _lib.load()
        for name, (res, args) in _lib.EVAL_SIGNATURES.items():
            fn = getattr(lib, name)
            assert fn.restype is res and list(fn.argtypes) == args
        cap = lib.cld_debug_sample_metrics_max_blocks()                    # no handle, no device call
        assert 1 <= cap <= 1 << 16
        assert lib.cld_sample_metrics_workspace_bytes(0) == 0 and lib.cld_sample_metrics_workspace_bytes((1 << 20) + 1) == 0
        assert [lib.cld_sample_metrics_workspace_bytes(b) for b in (1, 256, 257, 4096)] == [80, 80, 160, 1280]


def test_build_script_compiles_the_kernel_file_and_tracks_its_headers():
    sh = open(os.path.join(ROOT, "controllable-latent-diffusion-for-traffic-simulation_amd", "build.sh")).read()
    srcs = re.search(r'^SRCS="(.*)"$', sh, re.M).group(1).split()
    assert "sample_metrics_kernels" in srcs and srcs[-1] == "cld_api" and len(srcs) == len(set(srcs))
    assert "csrc/sample_metrics_kernels.h -nt" in sh and "../include/cld_eval.h -nt" in sh
