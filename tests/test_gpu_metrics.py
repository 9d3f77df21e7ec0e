"""The episode-metric kernels (csrc/metrics_kernels.hip; cld_scene_metrics_step / cld_scene_metrics_read) and `RolloutMetrics` against
tests/golden/rollout_metrics.npz (recorded from the reference's metric classes; tests/tools/record_metrics_golden.py) and the fp64
restatement of tests/metrics_cases.py.  The case keeps every discrete decision out of fp32's reach (tests/test_metrics_host.py asserts
the margins on the CPU), so flags, types, partners and rates are compared exactly.

Comfort is compared with |y - y_ref| <= KAPPA 2^-24 E, E the mean absolute magnitude entering the value (metrics_cases.comfort).
KAPPA from the operation count, in units of u = 2^-24: pose differences and the division by stat_dt = 0.5 are
exact; |vel| and |acc| are two squares, a sum and a correctly rounded square root: 2 u; cosf / sinf within 2 ulp: 4 u; the product 1 u
-> a lon / lat term 7 u of |acc|; a jerk term 2 u (|acc_k| + |acc_k+1|) / dt + 1 u; the per-agent sums are fp64 and their mean is
rounded to fp32 once: 8 u; the per-scene mean of those (fp64, rounded once) 9 u; the reference's own float64 steps and second-order
terms take it to KAPPA = 10.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from cld_amd import synth
from tests import metrics_cases as MC
from tests import raster_cases as RC

pytestmark = pytest.mark.gpu
KAPPA = 10.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_metrics.npz")


@pytest.fixture(scope="module")
def eng():
    from cld_amd.engine import Engine
    return Engine(n_timesteps=10, device="cuda:0")          # no weights: the metrics need none


@pytest.fixture(scope="module")
def gold():
    return MC.load_golden(GOLDEN)


def make(eng, case, name, world0=None, **kw):
    from cld_amd.metrics import RolloutMetrics
    cfg = MC.cfg_of(name)
    w0 = case["world"][0] if world0 is None else world0
    return RolloutMetrics(eng, case["scene_start"], case["extent"], w0, case["maps"], case["scene_map"], case["map_from_world"],
                          sim_dt=MC.SIM_DT, stat_dt=MC.STAT_DT, **cfg, **kw)


_RUNS = {}


def run(eng, case, name):
    """All 21 steps of the case on one raster (once per process) -> dict(flags [T,B,4], partner [T,B], per_agent, per_scene, state bytes)."""
    if name not in _RUNS:
        m = make(eng, case, name)
        world = torch.from_numpy(case["world"]).cuda()
        outs = [m.add_step(world[t], want_flags=True) for t in range(world.shape[0])]
        pa, ps = eng.scene_metrics_read(m._setup, m.state)
        torch.cuda.synchronize()
        _RUNS[name] = dict(flags=np.stack([o[0].cpu().numpy() for o in outs]), partner=np.stack([o[1].cpu().numpy() for o in outs]),
                           per_agent=pa.cpu().numpy().astype(np.float64), per_scene=ps.cpu().numpy().astype(np.float64),
                           state=m.state.cpu().numpy().copy(), episode=m.get_episode_metrics())
    return _RUNS[name]


def same(a, b, tol=0.0):
    """NaN in the same places, elsewhere within tol."""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool((np.abs(np.nan_to_num(a) - np.nan_to_num(b)) <= tol).all())


@pytest.mark.parametrize("name", list(MC.RASTERS))
def test_per_step_flags_type_and_partner_equal_the_golden(eng, gold, name):
    case, z = gold
    out = run(eng, case, name)
    for k, what in enumerate(("off_road", "off_road_disk", "coll_disk", "box code")):
        bad = out["flags"][..., k] != z[f"{name}_flags"][..., k]
        assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at (step, agent) = {np.argwhere(bad)[0].tolist()}"
    bad = out["partner"] != z[f"{name}_partner"]
    assert not bad.any(), f"partner: {int(bad.sum())} differ, first at (step, agent) = {np.argwhere(bad)[0].tolist()}"


@pytest.mark.parametrize("name", list(MC.RASTERS))
def test_rates_and_failures_equal_the_golden(eng, gold, name):
    case, z = gold
    out = run(eng, case, name)
    assert same(out["per_agent"][:, :12], z[f"{name}_per_agent"][:, :12], 1e-6)
    assert same(out["per_scene"][:, :12], z[f"{name}_per_scene"][:, :12], 1e-6)
    ep = out["episode"]
    assert set(ep) == {"all_off_road_rate", "all_disk_off_road_rate", "all_collision_rate", "all_disk_collision_rate", "all_failure", "all_comfort"}
    assert set(ep["all_collision_rate"]) == {"CollisionType.FRONT", "CollisionType.REAR", "CollisionType.SIDE", "coll_any"}
    assert same(ep["all_off_road_rate"]["nframe"].cpu().numpy().astype(np.float64), z[f"{name}_per_scene"][:, 1], 1e-6)
    assert same(ep["all_failure"]["failure_any"].cpu().numpy().astype(np.float64), z[f"{name}_per_scene"][:, 11], 1e-6)


def test_comfort_within_the_derived_bound(eng, gold):
    case, z = gold
    out = run(eng, case, "r224")
    traj = np.transpose(case["world"].astype(np.float64), (1, 0, 2))
    ref, E = MC.comfort(traj)
    got = out["per_agent"][:, 12:]
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ratio = np.nanmax(np.abs(got - ref) / (2.0 ** -24 * np.maximum(E, 1e-30)))
    print(f"comfort per agent: max |y - y_ref| / (2^-24 E) = {ratio:.3f} (bound {KAPPA})")
    assert ratio <= KAPPA
    ss = case["scene_start"]
    for s in range(len(ss) - 1):
        r = slice(ss[s], ss[s + 1])
        for k in range(4):
            y, y_ref, e = out["per_scene"][s, 12 + k], MC._nanmean(ref[r, k]), MC._nanmean(E[r, k])
            assert np.isnan(y) == np.isnan(y_ref)
            if not np.isnan(y):
                assert abs(y - y_ref) <= KAPPA * 2.0 ** -24 * e, (s, k, y, y_ref)
                assert abs(y - z["r224_per_scene"][s, 12 + k]) <= KAPPA * 2.0 ** -24 * e + 1e-12, (s, k)       # the reference's Comfort class


@pytest.mark.parametrize("name", list(MC.RASTERS))
def test_off_road_flags_equal_the_observation_rasters_bytes(eng, gold, name):
    """off_road and the disk flag against cld_rasterize's drivable bytes gathered at the 53 sample pixels of every agent, for the same
    poses: the centroid byte, and any of the 52 disk bytes (the kernel reports the disk test as one flag)."""
    case, _ = gold
    cfg = MC.cfg_of(name)
    out = run(eng, case, name)
    ext = case["extent"].astype(np.float64)
    pix = [MC.sample_pixels(ext[i, :2], cfg)[:2] for i in range(ext.shape[0])]
    u, v = np.stack([p[0] for p in pix]), np.stack([p[1] for p in pix])
    for t in range(case["world"].shape[0]):
        w = case["world"][t]
        valid = ~(np.isnan(w[:, 0]) | np.isnan(w[:, 1]))
        hw = torch.from_numpy(np.where(np.isnan(w), 0.0, w).astype(np.float32))[:, None].cuda()
        drv = np.zeros((w.shape[0], 53), np.uint8)
        for a in range(0, w.shape[0], 66):                      # (chunks keep the image buffer small)
            n = min(66, w.shape[0] - a)
            d = eng.rasterize(hw, torch.ones(w.shape[0], 1, dtype=torch.uint8), case["scene_start"], case["maps"], case["scene_map"],
                              case["map_from_world"], row0=a, B=n, max_neighbor_dist=30.0, want_raster_from_world=False, **cfg)[1].cpu().numpy()
            drv[a:a + n] = d[np.arange(n)[:, None], v[a:a + n], u[a:a + n]]
        assert np.array_equal(out["flags"][t, valid, 0], 1 - drv[valid, 52]), t
        assert np.array_equal(out["flags"][t, valid, 1], (drv[valid, :52] == 0).any(1).astype(np.uint8)), t
        assert (out["flags"][t, ~valid, :2] == 255).all()


def test_add_plans_equals_add_step_on_the_restated_poses(eng, gold):
    case, _ = gold
    B = case["extent"].shape[0]
    g = torch.Generator().manual_seed(3)
    w0 = np.nan_to_num(case["world"][0]).astype(np.float32)
    a, b = make(eng, case, "r64", world0=w0), make(eng, case, "r64", world0=w0)
    pose = torch.from_numpy(w0).cuda()
    for _ in range(4):
        plans = (torch.randn(B, 52, 6, generator=g) * torch.tensor([3.0, 0.5, 1.0, 0.2, 1.0, 0.1])).cuda()
        a.add_plans(plans)
        for k in range(5):
            w = eng.world_step(plans, pose[:, :2].contiguous(), pose[:, 2].contiguous(), k)[0]
            ref = RC.world_step(plans.cpu().numpy(), pose[:, :2].cpu().numpy(), pose[:, 2].cpu().numpy(), k)
            assert np.abs(w.cpu().numpy() - ref).max() <= 1e-4
            b.add_step(w)
        pose = w
        assert torch.equal(a.poses, pose)
    assert a.steps == b.steps == 20 and torch.equal(a.state, b.state)
    assert float(a.per_agent()[:, 0].min()) == 20.0


def test_two_runs_give_the_same_bytes_and_reset_empties(eng, gold):
    case, z = gold
    first = run(eng, case, "r64")
    m = make(eng, case, "r64")
    world = torch.from_numpy(case["world"]).cuda()
    for t in range(world.shape[0]):
        m.add_step(world[t])
    assert np.array_equal(m.state.cpu().numpy(), first["state"])
    pa, ps = eng.scene_metrics_read(m._setup, m.state)
    assert np.array_equal(pa.cpu().numpy().astype(np.float64), first["per_agent"], equal_nan=True)
    assert np.array_equal(ps.cpu().numpy().astype(np.float64), first["per_scene"], equal_nan=True)
    m.reset()
    assert m.steps == 0 and not bool(m.state.any())
    pa, ps = eng.scene_metrics_read(m._setup, m.state)
    assert same(pa.cpu().numpy().astype(np.float64), z["empty_per_agent"]) and same(ps.cpu().numpy().astype(np.float64), z["empty_per_scene"])


def test_a_scene_without_a_valid_record_equals_the_reference(eng, gold):
    """The small episode recorded from the reference beside the case: a one-agent scene that is NaN on every step."""
    from cld_amd.metrics import RolloutMetrics
    _, z = gold
    case = MC.absent_scene_case()
    m = RolloutMetrics(eng, case["scene_start"], case["extent"], case["world"][0], sim_dt=MC.SIM_DT, stat_dt=MC.STAT_DT, **MC.cfg_of("r64"))
    world = torch.from_numpy(case["world"]).cuda()
    outs = [m.add_step(world[t], want_flags=True) for t in range(world.shape[0])]
    assert np.array_equal(np.stack([o[0].cpu().numpy() for o in outs]), z["absent_flags"])
    assert np.array_equal(np.stack([o[1].cpu().numpy() for o in outs]), z["absent_partner"])
    pa, ps = (t.cpu().numpy().astype(np.float64) for t in eng.scene_metrics_read(m._setup, m.state))
    assert same(pa[:, :12], z["absent_per_agent"][:, :12], 1e-6) and same(ps[:, :12], z["absent_per_scene"][:, :12], 1e-6)
    assert np.isnan(ps[0, 0]) and np.isnan(ps[0, 2]) and np.isnan(ps[0, 12:]).all()
    ref, E = MC.comfort(np.transpose(case["world"].astype(np.float64), (1, 0, 2)))
    for k in range(4):                                                           # scene 1 = agents 1, 2: the bound of the module docstring
        y, y_ref, e = ps[1, 12 + k], z["absent_per_scene"][1, 12 + k], MC._nanmean(E[1:3, k])
        assert np.isnan(y) == np.isnan(y_ref) and (np.isnan(y) or abs(y - y_ref) <= KAPPA * 2.0 ** -24 * e + 1e-12), (k, y, y_ref)


def test_bad_arguments_return_status_codes(eng, gold):
    from cld_amd._lib import CldError
    from cld_amd.metrics import RolloutMetrics
    case, _ = gold
    B = case["extent"].shape[0]
    w0 = torch.zeros(B, 3)
    with pytest.raises(CldError, match="scene_start"):
        RolloutMetrics(eng, case["scene_start"][:-1], case["extent"], w0)
    with pytest.raises(CldError, match="scene_start"):
        eng.scene_metrics_setup([0, 5, B - 1], case["extent"])
    with pytest.raises(CldError, match="stat_dt"):
        RolloutMetrics(eng, case["scene_start"], case["extent"], w0, sim_dt=0.5, stat_dt=0.1)
    state = eng.scene_metrics_state(B)
    world = w0.cuda()
    good = eng.scene_metrics_setup(case["scene_start"], case["extent"])
    for bad_state in (state[:-128], state.cpu(), state.view(torch.int32)):       # too short, not on the device, not bytes
        with pytest.raises(CldError, match="state"):
            eng.scene_metrics_step(good, world, bad_state, 0)
        with pytest.raises(CldError, match="state"):
            eng.scene_metrics_read(good, bad_state)
    with pytest.raises(CldError, match="scene_start"):                            # a malformed split that is already on the device
        eng.scene_metrics_setup(torch.tensor([0, 5, B - 1], dtype=torch.int32, device="cuda"), case["extent"])
    with pytest.raises(CldError, match="drivable_layer"):
        eng.scene_metrics_step(eng.scene_metrics_setup(case["scene_start"], case["extent"], drivable_layer=3), world, state, 0)
    with pytest.raises(CldError, match="sim_dt"):
        eng.scene_metrics_step(eng.scene_metrics_setup(case["scene_start"], case["extent"], sim_dt=0.5, stat_dt=0.1), world, state, 0)
    setup = eng.scene_metrics_setup(case["scene_start"], case["extent"])
    rc = eng.lib.cld_scene_metrics_step(eng._h, C.byref(setup[0]), None, C.c_void_p(state.data_ptr()), None, None, 0, eng._stream())
    assert rc != 0 and b"world" in eng.lib.cld_last_error(eng._h)
    rc = eng.lib.cld_scene_metrics_read(eng._h, C.byref(setup[0]), None, None, None, eng._stream())
    assert rc != 0
    torch.cuda.synchronize()
    assert not bool(state.any())                                 # nothing ran


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


def test_rollout_with_metrics_scores_the_observers_history_and_changes_no_pose():
    """closed_loop_rollout(metrics=...) over 8 + 3 agents, 3 sim steps on a 10-step schedule: the per-agent table equals scoring the
    observer's appended history frames afterwards, and the poses are the bits of the run without metrics=."""
    from cld_amd._lib import CldError
    from cld_amd.metrics import RolloutMetrics
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

    def go(metrics):
        obs = SceneObserver(e, *args, n_step_action=5)
        poses = closed_loop_rollout(pol, obs, hw[:, -1, :2], hw[:, -1, 2], cs, n_sim_steps=S, n_step_action=5, gather=lambda traj: traj,
                                    noise=noise, **({} if metrics is None else {"metrics": metrics}))
        return poses, obs
    plain, _ = go(None)
    met = RolloutMetrics(e, *margs)
    scored, _ = go(met)
    assert torch.equal(plain, scored)
    assert met.steps == 15 and torch.equal(met.poses, scored[-1])
    after = RolloutMetrics(e, *margs)
    # the frames the rollout appended: the executed states of the three plans, from the observer of a second identical run
    obs2 = SceneObserver(e, *args, n_step_action=5)
    frames = []

    def cond_fn(step, world, c, plans):
        o = obs2(step, world, c, plans)
        if step:
            frames.append(obs2.hist_world[:, -5:].clone())
        return o
    poses2 = closed_loop_rollout(pol, cond_fn, hw[:, -1, :2], hw[:, -1, 2], cs, n_sim_steps=S + 1, n_step_action=5, gather=lambda traj: traj,
                                 noise=noise)
    assert torch.equal(poses2[:S], plain)
    for f in frames:
        for k in range(5):
            after.add_step(f[:, k].contiguous())
    assert after.steps == 15 and torch.equal(after.state, met.state)
    assert torch.allclose(after.per_agent(), met.per_agent(), rtol=0.0, atol=0.0, equal_nan=True)         # (15 steps: no jerk term yet, NaN)
    with pytest.raises(CldError, match="metrics"):
        closed_loop_rollout(pol, SceneObserver(e, *args), hw[:, -1, :2], hw[:, -1, 2], cs, n_sim_steps=1, gather=lambda traj: traj[:5],
                            noise=noise, metrics=RolloutMetrics(e, *margs))
