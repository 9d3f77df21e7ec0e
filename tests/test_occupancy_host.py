"""CPU tests of the occupancy metrics: the fp64 restatement (tests/occupancy_cases.py) against the recording of the reference's
OccupancyCoverage / OccupancyDiversity (tests/golden/occupancy.npz), the properties of the case the kernel tests run on, the default
transport solver against closed forms, and the C-ABI mirror."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import occupancy_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "occupancy.npz")


@pytest.fixture(scope="module")
def gold():
    return OC.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def restated(gold):
    case, z = gold
    cov = OC.restate_grid(case, OC.GRIDS["coverage"], case["world_full"])
    counts, detail = OC.coverage_counts(case, OC.GRIDS["coverage"], cov, case["failed"])
    return dict(cov=cov, counts=counts, detail=detail, dists=OC.distributions(case, OC.GRIDS["diversity"], case["world_full"]))


def test_the_builder_reproduces_the_goldens_inputs(gold):
    case, z = gold
    built = OC.case()
    for k in OC.INPUT_KEYS:
        assert np.array_equal(built[k], case[k]), k
    assert tuple(np.diff(case["scene_start"])) == OC.SCENE_SIZES and case["world_full"].shape == (OC.N_EPISODES, OC.N_STEPS, 61, 3)
    xy = case["world_full"][..., :2].astype(np.float64) * 1024.0
    assert not np.isnan(xy).any() and np.array_equal(xy, np.rint(xy)) and (xy < 0).any()       # multiples of 2^-10 m, some negative
    assert (case["failed"][0] != case["failed"][1]).any()
    nan = np.isnan(built["world"][..., 0])
    assert nan.all((0, 1)).sum() == 1 and (nan.any((0, 1)) & ~nan.all((0, 1))).sum() == len(OC.ABSENT_SOME)
    assert np.array_equal(np.nan_to_num(built["world"]), np.where(nan[..., None] & (np.arange(3) < 2), 0.0, built["world_full"]))


def test_restated_coverage_equals_the_golden(gold, restated):
    case, z = gold
    assert np.array_equal(restated["counts"], z["cov_counts"])
    for s, d in enumerate(restated["detail"]):
        cells, values, lane = z[f"cov_s{s}_cells"], z[f"cov_s{s}_values"], z[f"cov_s{s}_lane"]
        order = np.lexsort((cells[:, 1], cells[:, 0]))               # the restatement keeps its cells sorted
        assert np.array_equal(cells[order], d["cells"]), s
        assert np.abs(values[order] - d["value"]).max() <= 1e-12, s
        assert np.array_equal(lane[order] != 0, d["lane"] != 0), s
    # success as the touch sets give it: the three counts again, from the golden's own values and lane flags
    for s, d in enumerate(restated["detail"]):
        order = np.lexsort((z[f"cov_s{s}_cells"][:, 1], z[f"cov_s{s}_cells"][:, 0]))
        v, lane = z[f"cov_s{s}_values"][order], z[f"cov_s{s}_lane"][order].astype(np.float64)
        assert [(v > OC.THRESHOLD).sum(), (v * lane > OC.THRESHOLD).sum(), (v * lane * d["ok"] > OC.THRESHOLD).sum()] == z["cov_counts"][s].tolist()


def test_restated_distributions_equal_the_golden(gold, restated):
    case, z = gold
    cfg = OC.GRIDS["diversity"]
    for s, d in enumerate(restated["dists"]):
        for e in range(OC.N_EPISODES):                               # the per-episode grids
            cells = z[f"div_s{s}_e{e}_cells"]
            g = OC.restate_grid(case, cfg, case["world_full"], [e])[s]
            assert sorted(map(tuple, cells.tolist())) == sorted(g["value"])
            assert np.abs(z[f"div_s{s}_e{e}_values"] - np.array([g["value"][tuple(c)] for c in cells.tolist()])).max() <= 1e-12
            assert np.array_equal(z[f"div_s{s}_e{e}_lane"] != 0, OC.lane_of(case, cfg, s, cells))
        union = z[f"emd_s{s}_cells"]                                 # what pyemd.emd was handed, in upstream's order of the union
        assert sorted(map(tuple, union.tolist())) == list(map(tuple, d["cells"].tolist()))
        at = {tuple(c): k for k, c in enumerate(d["cells"].tolist())}
        perm = np.array([at[tuple(c)] for c in union.tolist()])
        assert np.abs(z[f"emd_s{s}_i1"] - d["distr"][1][perm]).max() <= 1e-12 and np.abs(z[f"emd_s{s}_j0"] - d["distr"][0][perm]).max() <= 1e-12
        assert np.array_equal(OC.distance_matrix(z[f"emd_s{s}_D2"], len(union)), d["D"][np.ix_(perm, perm)])
        assert abs(z[f"emd_s{s}_i1"].sum() - 1.0) < 1e-12


def _drop_variant(case):
    cfg = OC.GRIDS["coverage"]
    win = OC.windows(case["world"][0, 0], case["scene_start"], cfg, OC.DROP_REACH)
    return win, OC.restate_grid(case, cfg, case["world"], win=win)


def test_no_cell_value_is_within_its_bar_of_the_threshold(restated):
    """A condition on the case: the kernel's value of a cell differs from the restatement's by at most (adds into the cell) 2^-40, so with
    every value, value * lane and value * lane * ok farther than that from 1e-2 the GPU count tests leave no cell out."""
    case = OC.case()
    win, dropped = _drop_variant(case)
    _, detail2 = OC.coverage_counts(case, OC.GRIDS["coverage"], dropped, case["failed"])
    for detail in (restated["detail"], detail2):
        for d in detail:
            bar = d["adds"] * 2.0 ** -40
            for prod in (d["value"], d["value"] * d["lane"], d["value"] * d["lane"] * d["ok"]):
                assert (np.abs(prod - OC.THRESHOLD) > bar).all()


def test_the_case_holds_what_the_kernel_tests_need(restated):
    case = OC.case()
    cov_cfg, div_cfg = OC.GRIDS["coverage"], OC.GRIDS["diversity"]
    assert [OC.half_width(OC.GRIDS[k]) for k in ("coverage", "diversity", "wide")] == [3, 2, 4]      # 7 x 7, 5 x 5, 9 x 9 cells
    # rounding ties: a coordinate exactly between two cells, in both grids
    for cfg in (cov_cfg, div_cfg):
        f = (case["world_full"][..., :2].astype(np.float64) - np.array(cfg["offset"])) / np.array(cfg["step"])
        assert (np.abs(f - np.floor(f) - 0.5) == 0).any()
    w = case["world_full"][:, :, 0, 0]
    assert (w == 1.0).any() and (w == 3.0).any()
    # several agents on one cell at one step
    a = case["scene_start"][1]
    c = np.round(case["world_full"][0, :, a:a + 2, :2].astype(np.float64) / 2.0)
    assert (c[:, 0] == c[:, 1]).all(1).any()
    # every drivable boundary of the map is an odd integer of the world frame, both grids' points are even integers
    k = np.arange(OC.MAP_SIZE - 1)
    edge = OC.block_of(k) != OC.block_of(k + 1)
    x = (k[edge] + 0.5 - OC.MAP_SHIFT) / OC.MAP_SCALE
    assert np.array_equal(x, np.rint(x)) and (np.abs(x) % 2 == 1).all()
    for cfg in (cov_cfg, div_cfg):
        assert all(v % 2 == 0 for v in cfg["offset"] + cfg["step"])
    assert any(v != 0 for v in div_cfg["offset"])
    rim = case["maps"][0, 0]
    assert (rim[[0, -1]] != 0).all() and (rim[:, [0, -1]] != 0).all() and OC.NO_MAP_FILL != 0      # no boundary at the map's edge
    assert (case["maps"][0, 0] == 0).any() and case["scene_map"].tolist() == [0, 0, -1]
    # the two special cells of scene 1: touched by failed agents only / by an agent that fails in episode 0 and not in episode 1
    d = restated["detail"][1]
    at = {tuple(c): k for k, c in enumerate(d["cells"].tolist())}
    lone = at[(-30, 20)]
    assert restated["cov"][1]["touch"][(-30, 20)] == {(0, OC.LONE_FAILED), (1, OC.LONE_FAILED)} and case["failed"][:, OC.LONE_FAILED].all()
    assert d["lane"][lone] and d["value"][lone] > 1.0 and not d["ok"][lone]
    mixed = at[(30, 20)]
    assert restated["cov"][1]["touch"][(30, 20)] == {(0, OC.LONE_MIXED), (1, OC.LONE_MIXED)}
    assert case["failed"][:, OC.LONE_MIXED].tolist() == [1, 0] and d["ok"][mixed] and d["lane"][mixed]
    assert restated["counts"][1, 2] < restated["counts"][1, 1] < restated["counts"][1, 0]
    # with the small reach an agent's window is cut by its scene's window; with the default nothing is
    win, dropped = _drop_variant(case)
    assert dropped[1]["dropped"] > 0
    full = OC.windows(case["world_full"][0, 0], case["scene_start"], cov_cfg, OC.GOLDEN_REACH)
    assert all(g["dropped"] == 0 for g in OC.restate_grid(case, cov_cfg, case["world_full"], win=full))


def test_default_solver_against_closed_forms():
    from scipy.stats import wasserstein_distance
    from cld_amd.metrics import emd_linprog
    worst = 0.0
    for d in (1.0, 4.0, 123.456):                                    # two cells at distance d: |p - q| d
        for p, q in ((0.3, 0.9), (0.5, 0.5), (1.0, 0.0), (0.123456789, 0.987654321)):
            v = emd_linprog(np.array([p, 1 - p]), np.array([q, 1 - q]), np.array([[0.0, d], [d, 0.0]]))
            ref = abs(p - q) * d
            worst = max(worst, abs(v - ref) / ref if ref else abs(v))
    for seed in range(5):                                            # random weights on a line, some of them zero
        rng = np.random.default_rng(seed)
        for n in (5, 40, 150):
            x = np.sort(rng.uniform(-50, 50, n))
            p, q = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
            p[rng.uniform(size=n) < 0.3], q[rng.uniform(size=n) < 0.3] = 0.0, 0.0
            p, q = p / p.sum(), q / q.sum()
            v = emd_linprog(p, q, np.abs(x[:, None] - x[None]))
            ref = wasserstein_distance(x, x, p, q)
            worst = max(worst, abs(v - ref) / ref)
    print("largest relative deviation", worst)
    assert worst <= OC.SOLVER_RTOL


def test_default_solver_refuses_what_it_cannot_take():
    from cld_amd._lib import CldError
    from cld_amd import metrics
    n = metrics.EMD_MAX_CELLS + 1
    with pytest.raises(CldError, match="cells"):
        metrics.emd_linprog(np.full(n, 1.0 / n), np.full(n, 1.0 / n), np.zeros((n, n)))
    assert metrics.emd_linprog(np.zeros(3), np.zeros(3), np.ones((3, 3))) == 0.0


def test_the_package_does_not_import_scipy():
    import subprocess
    import sys
    code = "import sys; import cld_amd.metrics, cld_amd.policy, cld_amd.engine; assert not any(m.split('.')[0] == 'scipy' for m in sys.modules)"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


def test_cld_occupancy_layout_matches_the_header():
    from cld_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cld.h")).read()
    body = re.search(r"typedef struct cld_occupancy \{(.*?)\} cld_occupancy;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(const\s+)?(float|double|int32_t|int64_t|uint8_t)\s*(\*?)\s*(.+)$", decl.strip(), re.S)
        if m:
            for nm in m.group(4).split(","):
                nm = nm.strip()
                arr = re.match(r"([a-z_0-9]+)\[(\d+)\]", nm)
                fields.append((arr.group(1) if arr else nm, "*" if m.group(3) else m.group(2), int(arr.group(2)) if arr else 1))
    assert [f[0] for f in fields] == [n for n, _ in _lib.CldOccupancy._fields_]
    off = 0
    kinds = {"*": (8, ctypes.c_void_p), "double": (8, ctypes.c_double), "int64_t": (8, ctypes.c_int64), "float": (4, ctypes.c_float),
             "int32_t": (4, ctypes.c_int32)}
    for (name, kind, count), (_, ctype) in zip(fields, _lib.CldOccupancy._fields_):
        size, want = kinds[kind]
        assert (ctype is want) if count == 1 else (ctype._type_ is want and ctype._length_ == count), name
        off = (off + size - 1) // size * size
        assert getattr(_lib.CldOccupancy, name).offset == off, name
        off += size * count
    assert ctypes.sizeof(_lib.CldOccupancy) == 136 and _lib.CldOccupancy.offset.offset == 56
    assert _lib.OCCUPANCY_MAX_WINDOW_CELLS == int(re.search(r"#define CLD_OCCUPANCY_MAX_WINDOW_CELLS (\d+)", hdr).group(1))
    for sym in ("cld_occupancy_splat", "cld_occupancy_mark", "cld_occupancy_read"):
        assert sym in _lib.SIGNATURES and re.search(r"\b" + sym + r"\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    text = hdr[hdr.index("The occupancy metrics of a closed-loop evaluation"):hdr.index("typedef struct cld_occupancy")]
    for word in ("absent agents", "lane flag", "bounded window", "fixed point", "diversity"):
        assert word in text, word


def test_the_python_layer_has_the_interface():
    from cld_amd.engine import Engine
    from cld_amd.metrics import OccupancyMetrics
    from cld_amd.policy import closed_loop_rollout
    assert {"occupancy_setup", "occupancy_splat", "occupancy_mark", "occupancy_read"} <= set(dir(Engine))
    assert {"begin_episode", "add_step", "add_plans", "end_episode", "coverage", "dropped", "diversity_distributions", "diversity",
            "reset"} <= set(dir(OccupancyMetrics))
    p = inspect.signature(OccupancyMetrics.__init__).parameters
    assert p["reach"].default == 100.0 and p["max_episodes"].default == 8 and p["n_step_action"].default == 5 and p["window"].default is None
    assert inspect.signature(closed_loop_rollout).parameters["metrics"].default is None
