"""CPU tests of the episode metrics: the fp64 restatement (tests/metrics_cases.py) against the recording of the reference's metric
classes (tests/golden/rollout_metrics.npz), the margins of the case the kernel tests run on, the box restatement against hand-worked
cases, and the C-ABI mirror."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import metrics_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rollout_metrics.npz")


@pytest.fixture(scope="module")
def restated():
    case, z = MC.load_golden(GOLDEN)
    return case, z, {name: MC.restate(case, MC.cfg_of(name)) for name in MC.RASTERS}


def same(a, b, tol):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool((np.abs(np.nan_to_num(a) - np.nan_to_num(b)) <= tol).all())


def test_the_builder_reproduces_the_goldens_inputs():
    case, z = MC.load_golden(GOLDEN)
    built = MC.case()
    for k in ("world", "extent", "scene_start", "maps", "scene_map", "map_from_world"):
        assert np.array_equal(built[k], case[k], equal_nan=True), k
    assert tuple(np.diff(case["scene_start"])) == MC.SCENE_SIZES and case["world"].shape == (MC.N_STEPS, 330, 3)
    xy = case["world"][..., :2].astype(np.float64) * 1024.0
    assert np.array_equal(np.nan_to_num(xy), np.rint(np.nan_to_num(xy)))          # multiples of 2^-10 m
    nan = np.isnan(case["world"][..., 0])
    assert nan.all(0).sum() == 1 and 0 < (nan.any(0) & ~nan.all(0)).sum()         # one agent absent throughout, a few on some steps


def test_restatement_equals_the_golden(restated):
    case, z, rs = restated
    for name, r in rs.items():
        assert np.array_equal(r["flags"], z[f"{name}_flags"]) and np.array_equal(r["partner"], z[f"{name}_partner"]), name
        assert same(r["per_agent"], z[f"{name}_per_agent"], 1e-12) and same(r["per_scene"], z[f"{name}_per_scene"], 1e-12), name
    empty = MC.aggregate(case, [], np.zeros((330, 0, 3)))
    assert same(empty[0], z["empty_per_agent"], 0.0) and same(empty[1], z["empty_per_scene"], 0.0)


def test_a_scene_without_a_valid_record_as_the_reference_reports_it():
    """The small episode recorded beside the case: its one-agent scene is NaN on every step.  pandas gives that scene a NaN rate, an nframe
    of 0, collision and failure values of 0 and NaN comfort -- what include/cld.h states."""
    z = np.load(GOLDEN)
    case = MC.absent_scene_case()
    for k in ("world", "extent", "scene_start"):
        assert np.array_equal(case[k], z["absent_" + k], equal_nan=True), k
    r = MC.restate(case, MC.cfg_of("r64"))
    assert r["dist_margin"] >= MC.DIST_MARGIN and r["pix_margin"] >= MC.PIX_MARGIN
    assert np.array_equal(r["flags"], z["absent_flags"]) and np.array_equal(r["partner"], z["absent_partner"])
    assert same(r["per_agent"], z["absent_per_agent"], 1e-12) and same(r["per_scene"], z["absent_per_scene"], 1e-12)
    lone = z["absent_per_scene"][0]
    assert np.isnan(lone[[0, 2, 12, 13, 14, 15]]).all() and (lone[[1, 3, 4, 5, 6, 7, 8, 9, 10, 11]] == 0).all()


def test_margins_and_coverage_of_the_case(restated):
    case, z, rs = restated
    for name, r in rs.items():
        assert r["dist_margin"] >= MC.DIST_MARGIN and r["pix_margin"] >= MC.PIX_MARGIN, (name, r["dist_margin"], r["pix_margin"])
        f = r["flags"]
        assert ((f[..., 0] == 0) & (f[..., 1] == 1)).any()                        # centroid on the road, disk off it
        assert any(s["fill_used"] for s in r["steps"])
        sides = np.concatenate([s["side"] for s in r["steps"]])
        assert set(sides[sides >= 0].tolist()) == {0, 1, 2, 3}                    # front, rear, left, right
        assert (f[..., 2] == 1).any() and (f[..., 0] == 1).any()
    ss, first = case["scene_start"], rs["r224"]["steps"][0]
    b = ss[MC.CONSTRUCTED_SCENE]
    assert first["side"][b:b + 4].tolist() == [0, 1, 2, 3] and first["partner"][b:b + 4].tolist() == [b + 1, b, b + 3, b + 2]
    assert first["partner"][b + 5] == b + 4                                       # the lowest index, not the nearest (b + 6)
    assert first["code"][b + 7:b + 11].tolist() == [0, 0, 0, 0] and first["coll_disk"][b + 7:b + 11].tolist() == [0, 0, 0, 0]
    assert first["code"][b + 11:b + 13].tolist() == [3, 3] and first["coll_disk"][b + 11:b + 13].tolist() == [1, 1]
    # the giant agent's samples are clamped at every border of both rasters
    g = ss[MC.GIANT]
    for name, borders in (("r224", {"l", "r", "t", "b"}), ("r64", {"l", "r", "t", "b"})):
        cfg = MC.cfg_of(name)
        u, v, _ = MC.sample_pixels(case["extent"][g, :2].astype(np.float64), cfg)
        hit = {k for k, c in (("l", (u == 0)), ("r", (u == cfg["width"] - 1)), ("t", (v == 0)), ("b", (v == cfg["height"] - 1))) if c.any()}
        assert hit == borders, (name, hit)


def test_box_restatement_on_hand_worked_cases():
    P = lambda *a: np.array([a], np.float64)
    E = np.array([[4.0, 2.0]])
    # axis-aligned: j ahead of i by 3.5 and 0.25 to the left -> front 1.75 (y in [-0.75, 1]), left 0.5 (x in [1.5, 2]); seen from j: rear 1.75, right 0.5
    assert np.allclose(MC.side_lengths(P(0, 0, 0), E, P(3.5, 0.25, 0), E), [[1.75, 0.0, 0.5, 0.0]], atol=1e-14)
    assert np.allclose(MC.side_lengths(P(3.5, 0.25, 0), E, P(0, 0, 0), E), [[0.0, 1.75, 0.0, 0.5]], atol=1e-14)
    t = MC.pair_tests(P(0, 0, 0), E, P(3.5, 0.25, 0), E)
    assert t["box"][0] and t["side"][0] == 0 and not t["disk"][0] and np.isclose(t["margin"][0], 0.5)      # x overlap 0.5
    # side by side: left 3.75, front 0.5
    assert np.allclose(MC.side_lengths(P(0, 0, 0), E, P(0.25, 1.5, 0), E), [[0.5, 0.0, 3.75, 0.0]], atol=1e-14)
    # apart by 0.01 along x: the gap on i's long axis
    g = MC.sat_gaps(P(0, 0, 0), E, P(4.01, 0, 0), E)
    assert np.isclose(g[0, 0], 0.01) and not MC.pair_tests(P(0, 0, 0), E, P(4.01, 0, 0), E)["box"][0]
    # 45 degrees: a 2 x 2 square turned by 45 degrees, centred at i's front-right corner region: j at (2 + sqrt 2 - d, 0), its corner reaches
    # d into i through the front side, which it cuts over a length 2 d
    d = 0.25
    sq = np.array([[2.0, 2.0]])
    L = MC.side_lengths(P(0, 0, 0), E, P(2.0 + np.sqrt(2.0) - d, 0, np.pi / 4), sq)
    assert np.allclose(L, [[2 * d, 0.0, 0.0, 0.0]], atol=1e-12)
    assert MC.pair_tests(P(0, 0, 0), E, P(2.0 + np.sqrt(2.0) - d, 0, np.pi / 4), sq)["box"][0]
    assert not MC.pair_tests(P(0, 0, 0), E, P(2.0 + np.sqrt(2.0) + d, 0, np.pi / 4), sq)["box"][0]
    # the diagonal neighbour that axis-aligned bounding boxes would call a hit: separated on j's axis only
    assert not MC.pair_tests(P(0, 0, 0), E, P(2.9, 1.9, np.pi / 4), sq)["box"][0]
    # containment: i inside j -> every side whole, left (index 2) wins the tie with right -> SIDE; j inside i -> no side inside, argmax 0 -> FRONT
    big = np.array([[10.0, 6.0]])
    assert np.allclose(MC.side_lengths(P(0, 0, 0.3), E, P(0.5, 0.2, 0.1), big), [[2.0, 2.0, 4.0, 4.0]], atol=1e-12)
    assert MC.pair_tests(P(0, 0, 0.3), E, P(0.5, 0.2, 0.1), big)["side"][0] == 2
    inner = MC.pair_tests(P(0.5, 0.2, 0.1), big, P(0, 0, 0.3), E)
    assert inner["box"][0] and inner["side"][0] == 0 and np.allclose(MC.side_lengths(P(0.5, 0.2, 0.1), big, P(0, 0, 0.3), E), 0.0)


def test_comfort_restatement_on_a_parabola():
    """x = t^2 along a fixed heading 0.3, sampled every 0.1 s: speed terms (2 t + 0.5), |acc| = 2, jerk 0."""
    t = 0.1 * np.arange(21)
    traj = np.stack([t * t, np.zeros(21), np.full(21, 0.3)], -1)[None]
    val, E = MC.comfort(traj)
    assert np.allclose(val[0], [np.mean(2 * t[::5][:-1] + 0.5), 2 * np.cos(0.3), 2 * np.sin(0.3), 0.0], atol=1e-12)
    assert np.allclose(E[0], [val[0, 0], 2.0, 2.0, 8.0])


def test_cld_scene_metrics_layout_matches_the_header():
    from cld_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cld.h")).read()
    body = re.search(r"typedef struct cld_scene_metrics \{(.*?)\} cld_scene_metrics;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(const\s+)?(float|double|int32_t|uint8_t)\s*(\*?)\s*(.+)$", decl.strip(), re.S)
        if m:
            for nm in m.group(4).split(","):
                nm = nm.strip()
                arr = re.match(r"([a-z_0-9]+)\[(\d+)\]", nm)
                fields.append((arr.group(1) if arr else nm, "*" if m.group(3) else m.group(2), int(arr.group(2)) if arr else 1))
    assert [f[0] for f in fields] == [n for n, _ in _lib.CldSceneMetrics._fields_]
    off = 0
    for (name, kind, count), (_, ctype) in zip(fields, _lib.CldSceneMetrics._fields_):
        size = {"*": 8, "double": 8, "float": 4, "int32_t": 4}[kind]
        want = {"*": ctypes.c_void_p, "double": ctypes.c_double, "float": ctypes.c_float, "int32_t": ctypes.c_int32}[kind]
        assert (ctype is want) if count == 1 else (ctype._type_ is want and ctype._length_ == count), name
        off = (off + size - 1) // size * size
        assert getattr(_lib.CldSceneMetrics, name).offset == off, name
        off += size * count
    assert ctypes.sizeof(_lib.CldSceneMetrics) == 112 and _lib.CldSceneMetrics.sim_dt.offset == 40
    assert ctypes.sizeof(_lib.CldGuidance) == 144 and ctypes.sizeof(_lib.CldCollision) == 88 and ctypes.sizeof(_lib.CldMapCollision) == 80
    assert len(_lib.METRICS_AGENT_COLS) == int(re.search(r"#define CLD_METRICS_AGENT_COLS (\d+)", hdr).group(1))
    assert _lib.METRICS_SCENE_COLS == int(re.search(r"#define CLD_METRICS_SCENE_COLS (\d+)", hdr).group(1)) == MC.SCENE_COLS
    for sym in ("cld_scene_metrics_state_bytes", "cld_scene_metrics_step", "cld_scene_metrics_read"):
        assert sym in _lib.SIGNATURES and re.search(r"\b" + sym + r"\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "PARITY UNPINNED" in hdr[hdr.index("coll_box, type"):hdr.index("comfort        (Comfort)")]


def test_closed_loop_rollout_takes_metrics():
    from cld_amd.policy import closed_loop_rollout
    p = inspect.signature(closed_loop_rollout).parameters["metrics"]
    assert p.default is None
    from cld_amd.metrics import RolloutMetrics
    assert {"add_step", "add_plans", "get_episode_metrics", "per_agent", "reset"} <= set(dir(RolloutMetrics))
