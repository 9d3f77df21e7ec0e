"""The occupancy kernels (csrc/occupancy_kernels.hip; cld_occupancy_splat / cld_occupancy_mark / cld_occupancy_read) and `OccupancyMetrics`
against tests/golden/occupancy.npz (recorded from the reference's OccupancyCoverage / OccupancyDiversity;
tests/tools/record_occupancy_golden.py) and the fp64 restatement of tests/occupancy_cases.py.

The bar of a cell value is n_c 2^-40, n_c the number of adds into the cell: each add is rounded to a multiple of 2^-40, an error of at most
2^-41, and the fp64 exp and the restatement's fp64 sum are below 2^-50 per add.  tests/test_occupancy_host.py asserts on the CPU that no
value of the case is within that bar of the coverage threshold, so the counts are compared exactly."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from cld_amd import synth
from tests import occupancy_cases as OC
from tests import raster_cases as RC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "occupancy.npz")
ULP = 2.0 ** -40


@pytest.fixture(scope="module")
def eng():
    from cld_amd.engine import Engine
    return Engine(n_timesteps=10, device="cuda:0")          # no weights: the metrics need none


@pytest.fixture(scope="module")
def gold():
    return OC.load_golden(GOLDEN)


def map_args(case):
    return dict(maps=case["maps"], scene_map=case["scene_map"], map_from_world=case["map_from_world"], no_map_fill=OC.NO_MAP_FILL,
                n_sem=OC.N_SEM)


def setup_of(eng, case, cfg, win):
    return eng.occupancy_setup(case["scene_start"], win, cfg["offset"], cfg["step"], cfg["sigma"], OC.KERNEL_CUT, **map_args(case))


def planes(eng, setup):
    return (torch.zeros(setup[3], dtype=torch.int64, device="cuda"), torch.zeros(setup[2], dtype=torch.int64, device="cuda"))


def feed(eng, setup, steps):
    """steps: a list of [B,3] arrays -> (grid [cells] int64, dropped [S] int64) on the host."""
    grid, dropped = planes(eng, setup)
    for w in steps:
        eng.occupancy_splat(setup, torch.from_numpy(np.ascontiguousarray(w)), grid, dropped)
    return grid, dropped


def metrics_of(eng, case, world0, **kw):
    from cld_amd.metrics import OccupancyMetrics
    m = map_args(case)
    kw.setdefault("coverage", dict(OC.GRIDS["coverage"], threshold=OC.THRESHOLD))
    kw.setdefault("diversity", OC.GRIDS["diversity"])
    return OccupancyMetrics(eng, case["scene_start"], world0, m["maps"], m["scene_map"], m["map_from_world"], no_map_fill=OC.NO_MAP_FILL,
                            n_sem=OC.N_SEM, **kw)


def all_steps(world):
    return [world[e, t] for e in range(world.shape[0]) for t in range(world.shape[1])]


@pytest.mark.parametrize("name", list(OC.GRIDS))
def test_splat_equals_the_restatement_within_the_rounding_of_its_adds(eng, name):
    """Both episodes of the case with its absent agents, on windows small enough to cut some agents' kernel windows."""
    case, cfg = OC.case(), OC.GRIDS[name]
    win = OC.windows(case["world"][0, 0], case["scene_start"], cfg, OC.DROP_REACH)
    setup = setup_of(eng, case, cfg, win)
    assert setup[4] == OC.half_width(cfg)
    grid, dropped = feed(eng, setup, all_steps(case["world"]))
    values = eng.occupancy_read(setup, grid, counts=False, values=True)["values"].cpu().numpy()
    assert np.array_equal(values, grid.cpu().numpy() / OC.Q)
    rs = OC.restate_grid(case, cfg, case["world"], win=win)
    cs = setup[5][7].numpy()
    worst = 0.0
    for s, g in enumerate(rs):
        cells = np.array(sorted(g["value"]), np.int64).reshape(-1, 2)
        want = OC.dense(win[s], cells, [g["value"][tuple(c)] for c in cells.tolist()])
        adds = OC.dense(win[s], cells, [g["adds"][tuple(c)] for c in cells.tolist()])
        err = np.abs(values[cs[s]:cs[s + 1]] - want)
        worst = max(worst, (err / np.maximum(adds, 1) / ULP).max())
        assert (err <= adds * ULP).all(), (name, s)              # (no add: exactly 0)
    print(name, "largest error in units of n_c 2^-40:", worst)
    assert dropped.cpu().tolist() == [g["dropped"] for g in rs] and dropped[1] > 0


def test_the_plane_is_the_same_bits_under_any_order_of_agents_and_steps(eng):
    case, cfg = OC.case(), OC.GRIDS["coverage"]
    win = OC.windows(case["world"][0, 0], case["scene_start"], cfg, OC.DROP_REACH)
    setup = setup_of(eng, case, cfg, win)
    steps = all_steps(case["world"])
    grid, dropped = feed(eng, setup, steps)
    rng = np.random.default_rng(1)
    ss = case["scene_start"]
    perm = np.concatenate([ss[s] + rng.permutation(ss[s + 1] - ss[s]) for s in range(len(ss) - 1)])
    grid2, dropped2 = feed(eng, setup, [w[perm] for w in reversed(steps)])
    again, _ = feed(eng, setup, steps)
    assert torch.equal(grid, grid2) and torch.equal(dropped, dropped2) and torch.equal(grid, again) and bool(grid.any())


def test_64_agents_on_one_point_add_up_exactly(eng):
    cfg = OC.GRIDS["wide"]
    win = np.array([[-8, -8, 17, 17]], np.int64)
    case = dict(scene_start=np.array([0, 64], np.int32), maps=None, scene_map=None, map_from_world=None)
    setup = setup_of(eng, case, cfg, win)
    point = np.array([0.8125, -1.40625, 0.3], np.float32)
    one = np.full((64, 3), np.nan, np.float32)
    one[37] = point
    single, d1 = feed(eng, setup, [one])
    every, d2 = feed(eng, setup, [np.tile(point, (64, 1))] * 21)
    assert torch.equal(every, single * (64 * 21)) and int((single > 0).sum()) == 81 and not d1.any() and not d2.any()


@pytest.fixture(scope="module")
def golden_run(eng, gold):
    """The golden's inputs through OccupancyMetrics: two episodes with end_episode -> the object and the success plane after episode 0."""
    case, z = gold
    occ = metrics_of(eng, case, case["world_full"][0, 0])
    world = torch.from_numpy(case["world_full"]).cuda()
    success0 = None
    for e in range(world.shape[0]):
        occ.begin_episode()
        for t in range(world.shape[1]):
            occ.add_step(world[e, t])
        occ.end_episode(torch.from_numpy(case["failed"][e]).cuda())
        if e == 0:
            success0 = occ._success.clone()
    return occ, success0


def test_coverage_counts_values_and_lane_flags_equal_the_golden(eng, gold, golden_run):
    case, z = gold
    occ, success0 = golden_run
    cov = occ.coverage()
    got = torch.stack([cov["total"], cov["onroad"], cov["success"]], 1).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, z["cov_counts"])
    assert not occ.dropped().any() and not occ.dropped("diversity").any()
    g = occ._grids["coverage"]
    win, cs = g["setup"][5][6].numpy(), g["setup"][5][7].numpy()
    assert np.array_equal(win, OC.windows(case["world_full"][0, 0], case["scene_start"], OC.GRIDS["coverage"], OC.GOLDEN_REACH))
    r = eng.occupancy_read(g["setup"], g["grid"][0], occ._success, counts=False, values=True, lane=True)
    values, lane = r["values"].cpu().numpy(), r["lane"].cpu().numpy()
    rs = OC.restate_grid(case, OC.GRIDS["coverage"], case["world_full"])
    for s in range(3):
        cells = z[f"cov_s{s}_cells"]
        adds = OC.dense(win[s], cells, [rs[s]["adds"][tuple(c)] for c in cells.tolist()])
        assert (np.abs(values[cs[s]:cs[s + 1]] - OC.dense(win[s], cells, z[f"cov_s{s}_values"])) <= adds * ULP + 1e-12).all()
        at = (cells[:, 0] - win[s, 0]) * win[s, 3] + (cells[:, 1] - win[s, 1])
        assert np.array_equal(lane[cs[s]:cs[s + 1]][at], z[f"cov_s{s}_lane"])
    # the two special cells of scene 1, as upstream's sets say: failed writers only -> never a success; a writer that fails in episode
    # 0 and not in episode 1 -> a success once episode 1 is marked
    flat = lambda c: int(cs[1] + (c[0] - win[1, 0]) * win[1, 3] + (c[1] - win[1, 1]))
    final = occ._success.cpu().numpy()
    assert final[flat((-30, 20))] == 0 and final[flat((30, 20))] == 1 and success0.cpu().numpy()[flat((30, 20))] == 0
    assert values[flat((-30, 20))] > OC.THRESHOLD and lane[flat((-30, 20))] == 1


def test_absent_agents_and_the_scene_without_a_map_as_the_restatement_says(eng):
    from cld_amd._lib import CldError
    case, cfg = OC.case(), OC.GRIDS["coverage"]
    occ = metrics_of(eng, case, case["world"][0, 0], reach=OC.DROP_REACH, diversity=None)
    world = torch.from_numpy(case["world"]).cuda()
    for e in range(world.shape[0]):
        for t in range(world.shape[1]):
            occ.add_step(world[e, t])                               # (opens the episode itself)
        occ.end_episode(case["failed"][e])
    win = OC.windows(case["world"][0, 0], case["scene_start"], cfg, OC.DROP_REACH)
    assert np.array_equal(occ._grids["coverage"]["setup"][5][6].numpy(), win)
    rs = OC.restate_grid(case, cfg, case["world"], win=win)
    counts, detail = OC.coverage_counts(case, cfg, rs, case["failed"])
    cov = occ.coverage()
    assert np.array_equal(torch.stack([cov["total"], cov["onroad"], cov["success"]], 1).cpu().numpy(), counts)
    assert occ.dropped().cpu().tolist() == [g["dropped"] for g in rs]
    assert counts[2, 0] == counts[2, 1] >= counts[2, 2] > 0          # no map: every cell is on the road (the fill)
    absent = OC.ABSENT_ALWAYS
    assert not any((e, int(absent)) in t for g in rs for t in g["touch"].values() for e in (0, 1))
    with pytest.raises(CldError, match="diversity=None"):
        occ.diversity()


def test_diversity_distributions_equal_the_golden_and_the_value_the_restatement(eng, gold, golden_run):
    case, z = gold
    occ, _ = golden_run
    cfg = OC.GRIDS["diversity"]
    win = occ._grids["diversity"]["setup"][5][6].numpy()
    dists = OC.distributions(case, cfg, case["world_full"])
    got = occ.diversity_distributions()
    worst, slack = 0.0, []
    for s, (pts, distr) in enumerate(got):
        assert distr.is_cuda and distr.dtype == torch.float64 and tuple(distr.shape) == (2, win[s, 2] * win[s, 3])
        cells = z[f"emd_s{s}_cells"].astype(np.int64)
        at = (cells[:, 0] - win[s, 0]) * win[s, 3] + (cells[:, 1] - win[s, 1])
        d, p = distr.cpu().numpy(), pts.cpu().numpy()
        assert np.array_equal(p[at], cells * np.array(cfg["step"]) + np.array(cfg["offset"]))
        rest = np.ones(d.shape[1], bool)
        rest[at] = False
        assert not d[:, rest].any()                                  # nothing outside upstream's union of touched cells
        order = {tuple(c): k for k, c in enumerate(dists[s]["cells"].tolist())}
        perm = np.array([order[tuple(c)] for c in cells.tolist()])
        bars = []
        for e, ref in ((1, z[f"emd_s{s}_i1"]), (0, z[f"emd_s{s}_j0"])):
            bar = dists[s]["adds"][e][perm] * ULP / dists[s]["mass"][e]
            err = np.abs(d[e, at] - ref)
            worst = max(worst, (err / np.maximum(bar, ULP * 1e-3)).max())
            assert (err <= bar).all(), (s, e)
            bars.append(bar.sum())
        slack.append(dists[s]["D"].max() * sum(bars) / 2.0)         # an EMD moves by at most diam |dp|_1 / 2 per argument
    print("largest distribution error in units of its bar:", worst)
    from cld_amd.metrics import emd_linprog
    want = OC.diversity(dists, emd_linprog)
    value = occ.diversity()
    assert value.dtype == torch.float64 and tuple(value.shape) == (3,)
    print("diversity", value.tolist(), "restated", want.tolist())
    assert (np.abs(value.numpy() - want) <= np.array(slack) + 2.0 * OC.SOLVER_RTOL * want).all() and (want > 0).all()
    calls = []
    occ.diversity(solver=lambda a, b, D: calls.append((a.sum(), b.sum(), D.shape)) or 0.0)
    assert len(calls) == 3 and all(abs(a - 1.0) < 1e-12 and abs(b - 1.0) < 1e-12 for a, b, _ in calls)


def test_fewer_than_two_episodes_or_no_mass_on_the_road_give_nan(eng):
    case = OC.case()
    occ = metrics_of(eng, case, case["world_full"][0, 0], coverage=None)
    assert torch.isnan(occ.diversity()).all()
    for t in range(3):
        occ.add_step(case["world_full"][0, t])
    occ.end_episode(np.zeros(61))
    assert torch.isnan(occ.diversity()).all()                        # one episode: no pair
    nowhere = case["world_full"][0, 0].copy()
    nowhere[:1, :2] = np.nan                                         # scene 0's only agent is absent in episode 1: no mass
    occ.add_step(nowhere)
    occ.end_episode(np.zeros(61))
    d = occ.diversity()
    assert torch.isnan(d[0]) and not torch.isnan(d[1:]).any()
    occ.reset()
    assert occ.episodes == 0 and not occ._grids["diversity"]["grid"].any()


def _policy(n=10):
    from cld_amd.dm_model import DmModel
    from cld_amd.engine import Engine
    from cld_amd.policy import CldPolicy
    from cld_amd.vae_model import VaeModel
    e = Engine(n_timesteps=n, device="cuda:0")
    for sd in (synth.make_unet_weights(0, affine_jitter=True), synth.make_decoder_weights(0), synth.make_context_weights(0)):
        e.load_state_dict(sd)
    e.finalize()
    return e, CldPolicy(DmModel(None, None, n_timesteps=n, engine=e), VaeModel(engine=e))


def test_rollout_with_two_scorers_changes_no_pose_and_feeds_both():
    """closed_loop_rollout(metrics=(rm, occ)) over 8 + 3 agents, 3 sim steps on a 10-step schedule: the poses and the RolloutMetrics state
    are those of metrics=rm alone bit for bit, and occ is in the state feeding the same plans by hand gives."""
    from cld_amd.metrics import OccupancyMetrics, RolloutMetrics
    from cld_amd.observe import SceneObserver
    from cld_amd.policy import closed_loop_rollout
    n, S, B = 10, 3, 11
    e, pol = _policy(n)
    case = RC.build_case(23, [8, 3], spread=8.0, with_maps=[(320, 256)])
    args = (case["scene_start"], case["hist_world"], case["hist_avail"], case["maps"], case["scene_map"], case["map_from_world"])
    g = torch.Generator(device="cuda").manual_seed(7)
    noise = {"x_T": torch.randn(B, 52, 4, device="cuda", generator=g), "noise": torch.randn(n, B, 52, 4, device="cuda", generator=g)}
    cs = torch.zeros(B, 4, device="cuda"); cs[:, 2] = torch.rand(B, device="cuda", generator=g) * 10.0
    hw = torch.from_numpy(case["hist_world"])
    extent = torch.tensor([[4.5, 2.0, 1.5]]).repeat(B, 1)
    margs = (case["scene_start"], extent, hw[:, -1], case["maps"], case["scene_map"], case["map_from_world"])
    oargs = (case["scene_start"], hw[:, -1], case["maps"], case["scene_map"], case["map_from_world"])
    fed = []

    def go(metrics):
        obs = SceneObserver(e, *args, n_step_action=5)
        return closed_loop_rollout(pol, obs, hw[:, -1, :2], hw[:, -1, 2], cs, n_sim_steps=S, n_step_action=5,
                                   gather=lambda traj: fed.append(traj.clone()) or traj, noise=noise, metrics=metrics)
    rm1 = RolloutMetrics(e, *margs)
    alone = go(rm1)
    fed.clear()
    rm2, occ = RolloutMetrics(e, *margs), OccupancyMetrics(e, *oargs)
    both = go([rm2, occ])
    assert torch.equal(alone, both) and torch.equal(rm1.state, rm2.state) and rm2.steps == 15
    assert torch.equal(occ.poses, both[-1]) and len(occ._steps) == 15 and len(fed) == S
    hand = OccupancyMetrics(e, *oargs)
    for plans in fed:
        hand.add_plans(plans)
    for name in ("coverage", "diversity"):
        assert torch.equal(hand._grids[name]["grid"], occ._grids[name]["grid"]) and bool(occ._grids[name]["grid"].any())
        assert torch.equal(hand._grids[name]["dropped"], occ._grids[name]["dropped"])
    assert torch.equal(hand.poses, occ.poses)
    failed = rm2.per_agent()[:, 11] != 0
    occ.end_episode(failed)
    hand.end_episode(failed)
    assert torch.equal(hand._success, occ._success)
    c = occ.coverage()
    assert (c["total"] >= c["onroad"]).all() and (c["onroad"] >= c["success"]).all() and (c["total"] > 0).all()


def test_error_paths(eng):
    from cld_amd._lib import CldError
    case, cfg = OC.case(), OC.GRIDS["coverage"]
    w0 = case["world_full"][0, 0]
    occ = metrics_of(eng, case, w0, max_episodes=1)
    occ.add_step(w0)
    for call in (occ.coverage, occ.diversity_distributions, occ.diversity, occ.begin_episode):
        with pytest.raises(CldError, match="episode is open"):
            call()
    occ.end_episode(np.zeros(61))
    with pytest.raises(CldError, match="no episode is open"):
        occ.end_episode(np.zeros(61))
    with pytest.raises(CldError, match="max_episodes"):
        occ.add_step(w0)
    occ.reset()
    occ.add_step(w0)
    with pytest.raises(CldError, match="failed must be"):
        occ.end_episode(np.zeros(60))
    occ._adds = 2 ** 24 // 40                                       # as many steps as a scene of 40 agents may add
    with pytest.raises(CldError, match="2\\^24"):
        occ.add_step(w0)
    with pytest.raises(CldError, match="kernel window"):            # sigma 200 at step 2: 35 x 35 cells
        metrics_of(eng, case, w0, coverage=dict(sigma=200.0))
    with pytest.raises(CldError, match="positive step"):
        metrics_of(eng, case, w0, coverage=dict(step=(0.0, 2.0)))
    with pytest.raises(CldError, match="world0"):
        metrics_of(eng, case, w0[:-1])
    with pytest.raises(TypeError, match="unknown"):
        metrics_of(eng, case, w0, coverage=dict(sgima=1.0))
    # the library's own checks
    win = OC.windows(w0, case["scene_start"], cfg, 10.0)
    good = setup_of(eng, case, cfg, win)
    grid, dropped = planes(eng, good)
    world = torch.from_numpy(w0).cuda()
    for bad, word in ((dict(sigma=200.0), "CLD_OCCUPANCY_MAX_WINDOW_CELLS"), (dict(step=(0.0, 2.0)), "step"), (dict(step=(2.0, -1.0)), "step"),
                      (dict(sigma=0.0), "sigma"), (dict(sigma=float("nan")), "sigma")):
        st = setup_of(eng, case, dict(cfg, **bad), win)
        with pytest.raises(CldError, match=word):
            eng.occupancy_splat(st, world, grid, dropped)
        with pytest.raises(CldError, match=word):
            eng.occupancy_read(st, grid)
    for cut in (0.0, 1.0):
        st = eng.occupancy_setup(case["scene_start"], win, cfg["offset"], cfg["step"], 1.0, cut, **map_args(case))
        with pytest.raises(CldError, match="kernel_cut"):
            eng.occupancy_splat(st, world, grid, dropped)
    with pytest.raises(CldError, match="drivable_layer"):
        eng.occupancy_splat(eng.occupancy_setup(case["scene_start"], win, (0, 0), drivable_layer=3), world, grid, dropped)
    with pytest.raises(CldError, match="scene_start"):
        eng.occupancy_setup([0, 5, 4], win, (0, 0))
    with pytest.raises(CldError, match="window"):
        eng.occupancy_setup(case["scene_start"], win[:2], (0, 0))
    with pytest.raises(CldError, match="nx, ny"):
        eng.occupancy_setup(case["scene_start"], np.array([[0, 0, 0, 4]] * 3), (0, 0))
    for bad_grid in (grid[:-1], grid.cpu(), grid.to(torch.int32)):
        with pytest.raises(CldError, match="grid"):
            eng.occupancy_splat(good, world, bad_grid, dropped)
    with pytest.raises(CldError, match="threshold"):
        eng.occupancy_read(good, grid, threshold=-1.0)
    with pytest.raises(CldError, match="no output"):
        eng.occupancy_read(good, grid, counts=False)
    rc = eng.lib.cld_occupancy_splat(eng._h, C.byref(good[0]), None, C.c_void_p(grid.data_ptr()), C.c_void_p(dropped.data_ptr()), eng._stream())
    assert rc != 0 and b"world" in eng.lib.cld_last_error(eng._h)
    rc = eng.lib.cld_occupancy_mark(eng._h, C.byref(good[0]), C.c_void_p(world.data_ptr()), 0, C.c_void_p(grid.data_ptr()),
                                    C.c_void_p(grid.data_ptr()), eng._stream())
    assert rc != 0 and b"n_steps" in eng.lib.cld_last_error(eng._h)
    torch.cuda.synchronize()
    assert not bool(grid.any()) and not bool(dropped.any())          # nothing ran
