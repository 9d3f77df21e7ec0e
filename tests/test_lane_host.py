"""Host-side checks of the lane guidance (`gptlanefollowing`, `gptchangetoleftlane`, `gptfollowlane`): the fp64 yardstick
(tests/lane_yardstick.py) against the recording made from the reference's own project_onto and classes
(tests/golden/lane_guidance.npz, tests/tools/record_lane_golden.py), the margins of the recorded inputs, the configuration adapter,
the ctypes layout of `cld_lane_term` and the second signature table against include/cld_lane.h."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import lane_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["following", "following3", "changeleft", "followlane", "clip", "two"]
GAP_MIN, KINK_MIN = 1e-4, 1e-3


def recorded_case(golden, name):
    """-> (meta, arrays, plans [A,N,52,6] float32, yardstick term)."""
    meta, g = golden("lane_guidance")
    return meta, g, torch.from_numpy(g["plans"]), Y.term_from_meta(meta["cases"][name], g["lines"], meta["N"])


def config_values(case, v):
    """Per config of a recorded case the mean of its entries' values [N] (LaneFollowingLoss: the mean over the targets)."""
    n_cfg = len(case["configs"])
    return [v[[e for e, q in enumerate(case["entries"]) if q["config"] == k]].mean(dim=0) for k in range(n_cfg)]


def sum_bar(ref_err, max_ref):
    """The bar of the kernel tests: 4 x the larger of the reference's own fp32 error against the yardstick and the rounding bound of
    a 52-term fp32 sum, 52 2^-24 max|ref|."""
    return 4.0 * max(ref_err, 52 * 2.0 ** -24 * max_ref)


@pytest.mark.parametrize("name", CASES)
def test_yardstick_matches_the_reference_recording(golden, name):
    """Projection, per-config values, total and gradient within the reference's own recorded fp32 error (x 1.01 for the float32
    storage of the recording); gradient only in columns 0, 1 and 3 (0 and 1 for the decayed class) of the entries' agents."""
    meta, g, plans, term = recorded_case(golden, name)
    case = meta["cases"][name]
    v, grad = Y.value_and_grad(plans.double(), term)
    proj, gap = Y.projections(plans.double(), term)
    err_p = float((proj - torch.from_numpy(g[name + "_proj"]).double()).abs().max())
    assert err_p <= 1.01 * case["ref_proj_err"] and case["ref_proj_err"] <= 1e-5
    for k, cv in enumerate(config_values(case, v)):
        ref_v = torch.from_numpy(g[f"{name}_values_{k}"]).double()
        assert ref_v.shape == (meta["N"],) and float((cv - ref_v).abs().max()) <= 1.01 * case["ref_value_err"]
    ref_g = torch.from_numpy(g[name + "_grad"]).double()
    err_g = float((grad - ref_g).abs().max())
    print(f"{name}: projection {err_p:.2e} m, gradient {err_g:.2e} of max {float(ref_g.abs().max()):.3e}; smallest gap {float(gap.min()):.3e} m")
    assert float(ref_g.abs().max()) > 0 and err_g <= 1.01 * case["ref_grad_err"]
    tot = float(g[name + "_total"][0])
    assert abs(float(Y.total(plans.double(), term)) - tot) <= 1e-6 * max(1.0, abs(tot))
    quiet = np.ones(meta["A"], bool)
    quiet[term["agent"]] = False
    assert float(ref_g[quiet].abs().max()) == 0.0 and float(grad[quiet].abs().max()) == 0.0
    assert float(ref_g[..., [2, 4, 5]].abs().max()) == 0.0 and float(grad[..., [2, 4, 5]].abs().max()) == 0.0
    yaw_expected = any(k != "follow_decayed" for k in term["kind"])
    assert (float(ref_g[..., 3].abs().max()) > 0) == yaw_expected and (float(grad[..., 3].abs().max()) > 0) == yaw_expected


def test_the_recorded_inputs_keep_the_margins(golden):
    """Every element of every case: projection gap >= 1e-4 m, kink margins >= 1e-3 (what the kernel tests against the golden rely on)."""
    meta, g = golden("lane_guidance")
    assert list(meta["cases"]) == CASES and (meta["A"], meta["N"], meta["S"]) == (6, 2, 48) and g["plans"].shape == (6, 2, 52, 6)
    for name in CASES:
        _, _, plans, term = recorded_case(golden, name)
        gap, kink = Y.margins(plans.double(), term)
        assert gap >= GAP_MIN and kink >= KINK_MIN, (name, gap, kink)


def test_the_recording_holds_the_cases_it_is_meant_to(golden):
    meta, g = golden("lane_guidance")
    cases, lines, raw = meta["cases"], g["lines"], g["lines_unsorted"]
    assert [cases[n]["configs"] for n in CASES] == [["LaneFollowingLoss"], ["LaneFollowingLoss"], ["ChangeToLeftLaneLoss"], ["FollowLaneLoss"],
                                                   ["FollowLaneLoss"], ["LaneFollowingLoss", "FollowLaneLoss"]]
    assert [q["agent"] for q in cases["following3"]["entries"]] == [1, 2, 3] and [q["agent"] for q in cases["two"]["entries"]] == [1, 3, 3]
    assert cases["changeleft"]["entries"][0]["line"] == 6 + 4                      # the LEFT lane's polyline
    # the polylines: the yardstick's preparation of the stored world lines; 20 to 48 points; a NaN-padded row, a duplicated point,
    # a stored order that is not x-sorted
    assert np.array_equal(Y.transform(g["world_lines"], g["line_frame"], g["agent_from_world"]), raw, equal_nan=True)
    assert np.array_equal(Y.sort_by_x(raw), lines, equal_nan=True)
    count = np.isfinite(lines[..., 0]).sum(axis=1)
    assert count.min() == 20 and count.max() <= 48 and count[0] == 20 and bool(np.isnan(lines[0, 20:]).all())
    step = np.linalg.norm(np.diff(lines[2, :count[2], :2], axis=0), axis=1)
    assert (step == 0).sum() == 1 and step[step > 0].min() > 0.5 and step.max() < 1.5
    assert not np.array_equal(raw[3], lines[3], equal_nan=True) and np.array_equal(raw[1], lines[1], equal_nan=True)
    # the clip at 5 of FollowLaneLoss: active at some steps and idle at others in `clip`, idle throughout in `followlane` (recomputed)
    for n in ("clip", "followlane"):
        _, _, plans, term = recorded_case(golden, n)
        some, always = Y.clip_active(plans.double(), term, 0)
        assert [some.tolist(), always.tolist()] == cases[n]["clip"][0]
    some, always = cases["clip"]["clip"][0]
    assert any(s and not a for s, a in zip(some, always)) and not any(cases["followlane"]["clip"][0][0])


def test_decayed_form_is_normalised_and_averaged_and_ties_take_the_first_segment():
    line = torch.tensor([[0.0, 0.0, 0.1], [1.0, 0.0, 0.2], [2.0, 0.0, 0.3], [float("nan")] * 3], dtype=torch.float64)
    plans = torch.zeros(1, 1, 52, 6, dtype=torch.float64)
    plans[..., 0], plans[..., 1] = 1.0, 2.0                                # above the shared point of the two segments: a tie
    term = dict(agent=[0], line=[0], kind=["follow_decayed"], decay=[0.9], scale=[1.0], lines=line[None])
    assert abs(float(Y.values(plans, term)[0, 0]) - 2.0 / 52) <= 1e-12   # sum_t w_t = 1, then the mean over 52 steps
    pr, best, gap = Y.project(plans[0, 0, :, :2], line)
    assert bool((best == 0).all()) and bool((pr[:, 2] == 0.1).all()) and float(gap.max()) == 0.0
    dup = torch.tensor([[0.0, 0.0, 0.1], [1.0, 0.0, 0.2], [1.0, 0.0, 0.25], [2.0, 0.0, 0.3]], dtype=torch.float64)
    _, best, _ = Y.project(torch.tensor([[1.5, 1.0]], dtype=torch.float64), dup)
    assert int(best) == 2 and not bool(Y.segments(dup)[3][1])              # the zero-length segment is never chosen


def _cfg():
    scene_index = torch.tensor([4, 4, 4, 4, 4, 9, 9, 9, 9, 9, 9, 9])
    cfg = [[{"name": "gptlanefollowing", "weight": 3.0, "agents": None, "params": {}},
            {"name": "speed_limit", "weight": 3.0, "params": {"speed_limit": 6.0}, "agents": None},
            {"name": "gptfollowlane", "weight": 2.0, "agents": None, "params": {"target_ind": 2, "decay_rate": 0.8}}],
           [{"name": "gptchangetoleftlane", "weight": 0.5, "agents": None, "params": {}},
            {"name": "gptfollowlane", "weight": 1.0, "agents": None, "params": {}}]]
    B, S = 12, 5
    pts = torch.zeros(B, S, 3, dtype=torch.float64)
    pts[..., 0] = torch.arange(S, dtype=torch.float64) * 2.0 + torch.arange(B, dtype=torch.float64)[:, None]
    left = pts.clone()
    left[..., 1] += 3.5
    left = torch.cat([left, torch.full((B, 2, 3), float("nan"), dtype=torch.float64)], dim=1)
    db = {"world_from_agent": torch.eye(3).repeat(B, 1, 1), "lane_points": pts, "left_lane_points": left}
    return cfg, scene_index, db


def test_lane_terms_from_config_peels_the_names_and_orders_the_entries():
    from cld_amd.policy import guidance_from_config, lane_terms_from_config
    cfg, scene_index, db = _cfg()
    rest, term = lane_terms_from_config(cfg, scene_index, db)
    assert [[c["name"] for c in s] for s in rest] == [["speed_limit"], []] and rest[0][0] is cfg[0][1] and [len(s) for s in cfg] == [3, 2]
    # upstream's defaults: target_inds [1, 2, 3]; target_ind 6 (left) and 4 (decay 0.9), scene-local -> batch indices; ordered by agent
    assert term["agent"] == [1, 2, 2, 3, 9, 11] and term["kind"] == ["following", "following", "follow_decayed", "following", "follow_decayed", "change_left"]
    assert term["decay"][2] == 0.8 and term["decay"][4] == 0.9 and term["weight"] == [1.0, 1.0, 2.0, 1.0, 1.0, 0.5]
    assert term["configs"] == [(0, 0), (0, 0), (0, 2), (0, 0), (1, 1), (1, 0)] and term["names"][5] == "gptchangetoleftlane"
    assert term["sources"] == [("lane_points", 1), ("lane_points", 2), ("lane_points", 3), ("left_lane_points", 11), ("lane_points", 9)]
    assert term["line"] == [0, 1, 1, 2, 4, 3] and term["line_frame"] == [1, 2, 3, 11, 9] and "scale" not in term
    wl = term["world_lines"]
    assert wl.shape == (5, 7, 3) and wl.dtype == torch.float64 and torch.equal(wl[0, :5], db["lane_points"][1]) and bool(torch.isnan(wl[0, 5:]).all())
    assert torch.equal(wl[3, :5], db["left_lane_points"][11, :5])
    assert torch.equal(term["agent_from_world"], torch.eye(3).repeat(12, 1, 1))          # the inverse of world_from_agent
    F = torch.eye(3).repeat(12, 1, 1) * 1.0
    _, term4 = lane_terms_from_config(cfg, scene_index, dict(db, agent_from_world=F), num_samp=4)
    assert term4["agent_from_world"] is F and np.allclose(term4["scale"], [0.25, 0.25, 0.5, 0.25, 0.25, 0.125])      # weight / (K num_samp)
    assert "speed_limit" in guidance_from_config(rest, scene_index)
    plain = [[cfg[0][1]], []]
    rest2, term2 = lane_terms_from_config(plain, scene_index, None)       # nothing to peel: no data_batch needed
    assert term2 is None and rest2 == plain


def test_lane_terms_from_config_errors():
    from cld_amd.policy import lane_terms_from_config
    cfg, scene_index, db = _cfg()
    lc = lambda name="gptfollowlane", **kw: [[dict({"name": name, "weight": 1.0, "agents": None, "params": {}}, **kw)], []]
    with pytest.raises(ValueError, match="agent_from_world or world_from_agent"):
        lane_terms_from_config(cfg, scene_index, None)
    with pytest.raises(ValueError, match="agent_from_world or world_from_agent"):
        lane_terms_from_config(cfg, scene_index, {"lane_points": db["lane_points"]})
    with pytest.raises(ValueError, match="left_lane_points"):
        lane_terms_from_config(lc("gptchangetoleftlane", params={"target_ind": 1}), scene_index, {k: v for k, v in db.items() if k != "left_lane_points"})
    with pytest.raises(ValueError, match="outside scene"):
        lane_terms_from_config(lc(params={"target_ind": 5}), scene_index, db)                        # scene 0 has 5 agents
    with pytest.raises(ValueError, match="outside scene"):
        lane_terms_from_config(lc("gptchangetoleftlane"), scene_index, db)                           # upstream's default target_ind = 6
    with pytest.raises(ValueError, match="T = 40"):
        lane_terms_from_config(lc(params={"target_ind": 1, "T": 40}), scene_index, db)
    with pytest.raises(NotImplementedError, match="agents"):
        lane_terms_from_config(lc(agents=[0, 1], params={"target_ind": 1}), scene_index, db)
    nan_row = db["lane_points"].clone()
    nan_row[3] = float("nan")
    with pytest.raises(ValueError, match="no usable polyline"):
        lane_terms_from_config(lc(params={"target_ind": 3}), scene_index, dict(db, lane_points=nan_row))
    assert lane_terms_from_config(lc(params={"target_ind": 2}), scene_index, dict(db, lane_points=nan_row))[1]["agent"] == [2]   # only targeted rows need be finite
    one = db["lane_points"].clone()
    one[3, 1:] = one[3, :1]                                                # a single point repeated: no segment
    with pytest.raises(ValueError, match="no usable polyline"):
        lane_terms_from_config(lc(params={"target_ind": 3}), scene_index, dict(db, lane_points=one))
    with pytest.raises(ValueError, match="must be"):
        lane_terms_from_config(lc(params={"target_ind": 3}), scene_index, dict(db, lane_points=torch.zeros(12, 1025, 3)))


def test_guidance_from_config_still_refuses_the_names_and_set_guidance_takes_them():
    from cld_amd.dm_model import repeat_guidance
    from cld_amd.policy import LANE_NAMES, SCENE_LEVEL_LOSSES, CldPolicy, guidance_from_config, refresh_lane_term
    cfg, scene_index, db = _cfg()
    assert set(LANE_NAMES) == {"gptlanefollowing", "gptchangetoleftlane", "gptfollowlane"} and all(n in SCENE_LEVEL_LOSSES for n in LANE_NAMES)
    for name in LANE_NAMES:
        with pytest.raises(NotImplementedError, match="is not built"):
            guidance_from_config([[{"name": name, "weight": 1.0, "agents": None, "params": {"target_ind": 0}}], []], scene_index, data_batch=db)
    pol = CldPolicy(None, None)
    pol.set_guidance(cfg, scene_index, data_batch=db, lr=0.05)
    g = pol._guidance
    assert g["lane"]["agent"] == [1, 2, 2, 3, 9, 11] and "speed_limit" in g and g["lr"] == 0.05 and "pair" not in g
    pol.set_guidance([[cfg[0][2]], []], scene_index, data_batch=db)       # nothing but a lane config: still a guidance
    assert set(pol._guidance) == {"lane"}
    both = [[cfg[0][2], {"name": "gptcollision", "weight": 1.0, "agents": None, "params": {"target_ind": 0, "ref_ind": 1}}], []]
    pol.set_guidance(both, scene_index, data_batch=db)
    assert set(pol._guidance) == {"lane", "pair"}
    rep = repeat_guidance({"lane": g["lane"]}, 4)
    assert rep["lane"]["num_samp"] == 4 and "num_samp" not in g["lane"]
    # the term follows an observation: new frames (the inverse of world_from_agent when that is all there is), new polylines when carried
    W2 = torch.eye(3).repeat(12, 1, 1)
    W2[:, 0, 2] = 5.0
    g2 = refresh_lane_term(g, {"world_from_agent": W2})
    assert float(g2["lane"]["agent_from_world"][0, 0, 2]) == -5.0 and g2["lane"]["world_lines"] is g["lane"]["world_lines"]
    assert float(g["lane"]["agent_from_world"][0, 0, 2]) == 0.0           # nothing is modified in place
    moved = {k: db[k] + 1.0 for k in ("lane_points", "left_lane_points")}
    g3 = refresh_lane_term(g, dict(moved, agent_from_world=W2))
    assert g3["lane"]["agent_from_world"] is W2 and torch.equal(g3["lane"]["world_lines"][0, :5], moved["lane_points"][1])
    g4 = refresh_lane_term(g, {"lane_points": moved["lane_points"]})      # the left lane is missing: the polylines stay
    assert g4 is g
    assert refresh_lane_term(g, {}) is g and refresh_lane_term({"lr": 1.0}, {"world_from_agent": W2}) == {"lr": 1.0}


def _header():
    return open(os.path.join(ROOT, "include", "cld_lane.h")).read()


def test_cld_lane_term_layout_matches_the_header():
    """ctypes mirror of `cld_lane_term` against include/cld_lane.h, field by field in declaration order."""
    from cld_amd import _lib
    hdr = _header()
    body = re.search(r"typedef struct cld_lane_term \{(.*?)\} cld_lane_term;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(2), "*" in m.group(1)) for m in re.finditer(r"([A-Za-z_0-9 ]+\*?)\s*\b([a-z_]+);", body)]
    assert [n for n, _ in fields] == [n for n, _ in _lib.CldLaneTerm._fields_]
    off = 0
    for (name, is_ptr), (_, ctype) in zip(fields, _lib.CldLaneTerm._fields_):
        size = 8 if is_ptr else 4
        assert (ctype is ctypes.c_void_p) == is_ptr and ctypes.sizeof(ctype) == size, name
        assert getattr(_lib.CldLaneTerm, name).offset == off, name
        off += size
    assert ctypes.sizeof(_lib.CldLaneTerm) == 64 and _lib.CldLaneTerm.num_entries.offset == 48
    enum = dict((m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"CLD_LANE_([A-Z_]+) = (\d)", hdr))
    assert enum == _lib.LANE_KINDS and tuple(sorted(enum, key=enum.get)) == Y.KINDS
    assert int(re.search(r"#define CLD_LANE_MAX_PTS (\d+)", hdr).group(1)) == _lib.LANE_MAX_PTS == 1024


def test_lane_header_matches_the_second_signature_table_and_the_first_keeps_its_size():
    """include/cld_lane.h <=> _lib.LANE_SIGNATURES <=> the library's exports, in the manner of test_host_logic.py; include/cld.h
    and _lib.SIGNATURES hold no lane entry point and still count 88."""
    from cld_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(cld_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.LANE_SIGNATURES) == {"cld_lane_prepare", "cld_lane_loss", "cld_set_lane_term"}
    for name, (_, args) in _lib.LANE_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1)
        assert len(proto.split(",")) == len(args), name
    assert '#include "cld.h"' in code
    main_hdr = open(os.path.join(ROOT, "include", "cld.h")).read()
    assert len(_lib.SIGNATURES) == 88 and not any(n in _lib.SIGNATURES or n in main_hdr for n in _lib.LANE_SIGNATURES)
    if os.path.exists(_lib.LIB_PATH):                                      # where the library is built: it exports all three
        lib = _lib.load()
        for name, (res, args) in _lib.LANE_SIGNATURES.items():
            fn = getattr(lib, name)
            assert fn.restype is res and list(fn.argtypes) == args
        assert lib.cld_lane_loss.argtypes[2]._type_ is _lib.CldLaneTerm


def test_the_random_kernel_cases_keep_their_conditions():
    """The unsettled cases of tests/test_gpu_lane.py, for the chosen seeds: near-tie elements (gap < 1e-4 m) are at most 10 % of a case,
    every case keeps at least one checked (entry, sample) row per kind, and on the checked rows no kink quantity is within 1e-5 of its
    kink (an fp32 projection may not change a sign or the clip's side there); the clip at 5 is active somewhere and idle somewhere."""
    from tests import lane_cases as LC
    built = [((S, N), LC.size_case(S, N)) for S in LC.SIZES for N in LC.SAMPLES] + [("scenes", LC.scenes_case())]
    for key, (plans, term) in built:
        frac, per_kind, kink, rows = LC.conditions(plans, term)
        print(f"{key}: near-tie fraction {frac:.4f}, checked rows per kind {per_kind}, kink margin {kink:.2e}")
        assert frac <= 0.10 and all(v >= 1 for v in per_kind.values()) and kink >= LC.KINK, key
        clips = [Y.clip_active(plans.double(), term, e) for e in range(len(term["agent"])) if term["kind"][e] == "follow_decayed"]
        assert any(bool(s.any()) for s, _ in clips) and not all(bool(a.all()) for _, a in clips), key
    plans, term = built[-1][1]
    assert plans.shape[0] == 70 and len(set(term["agent"])) < len(term["agent"]) and len(set(range(70)) - set(term["agent"])) >= 20
    assert all(term["agent"][e] <= term["agent"][e + 1] for e in range(len(term["agent"]) - 1))          # an agent's entries are contiguous
