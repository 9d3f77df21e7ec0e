"""The guidance metric kernels (csrc/guide_metrics_kernels.hip; cld_guide_metrics_step / cld_guide_metrics_read) and `GuidanceMetrics`
against tests/golden/guide_metrics.npz (recorded from the reference's GuidanceMetric classes; tests/tools/record_guide_metrics_golden.py)
and the fp64 restatement of tests/guide_metrics_cases.py.  The cases keep every discrete decision out of fp32's reach
(tests/test_guide_metrics_host.py asserts the margins on the CPU).

Flag-derived values (the collision and map kinds) are compared exactly: the per-member values are ratios of small integers and the
mean over members is taken in numpy's order.  Distance and speed values are compared with
|y - y_ref| <= (n + 16) 2^-52 max(|term|, |coordinate|), n the number of summed terms: both sides are float64 from the same fp32 inputs;
n covers the order of the sums (numpy's pairwise order against the kernel's), 16 the square root, the products of the first-step frame,
a one-ulp difference of sin / cos there and the final divisions (DESIGN.md section 4.20 has the measured maxima).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from cld_amd import synth
from tests import guide_metrics_cases as GC
from tests import raster_cases as RC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guide_metrics.npz")


@pytest.fixture(scope="module")
def eng():
    from cld_amd.engine import Engine
    return Engine(n_timesteps=10, device="cuda:0")          # no weights: the metrics need none


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return z, json.loads(bytes(z["meta"]).decode())


def make(eng, case, config=None, constraint="case", world0=None, **kw):
    from cld_amd.metrics import GuidanceMetrics
    return GuidanceMetrics(eng, case["config"] if config is None else config, case["scene_start"], case["extent"],
                           case["world"][0] if world0 is None else world0, maps=case["maps"], scene_map=case["scene_map"],
                           map_from_world=case["map_from_world"], constraint_config=case["constraint"] if constraint == "case" else constraint,
                           **case["cfg"], **kw)


def feed(m, case):
    world, speed, acc = (torch.from_numpy(case[k]).cuda() for k in ("world", "speed", "acc"))
    for t in range(world.shape[0]):
        m.add_step(world[t], speed[t], acc[t])
    return m


_RUNS = {}


def run(eng, name):
    if name not in _RUNS:
        case = GC.case(name)
        m = feed(make(eng, case), case)
        ep = m.get_episode_metrics()
        pm = {k: m.per_member(k).cpu().numpy() for k in m.keys}
        torch.cuda.synchronize()
        _RUNS[name] = dict(m=m, episode={k: v.cpu().numpy() for k, v in ep.items()}, per_member=pm, state=m.state.cpu().numpy().copy())
    return _RUNS[name]


def err_in_bound(got, ref, n, scale):
    """-> |got - ref| / ((n + 16) 2^-52 scale), 0 where both are NaN or the same infinity, inf where only one is."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    special = np.isnan(ref) | np.isinf(ref) | np.isnan(got) | np.isinf(got)
    same = (np.isnan(got) & np.isnan(ref)) | (got == ref)
    with np.errstate(invalid="ignore"):
        r = np.abs(got - ref) / ((n + 16) * 2.0 ** -52 * scale)
    return np.where(special, np.where(same, 0.0, np.inf), r)


@pytest.mark.parametrize("name", ["main", "small"])
def test_episode_values_against_the_golden(eng, gold, name):
    z, meta = gold
    case, out = GC.case(name), run(eng, name)
    rs = case["restated"]
    pre = "" if name == "main" else "small_"
    keys = meta[pre + "keys"]
    assert list(out["episode"]) == keys                                          # upstream's names in upstream's order
    S = len(case["scene_start"]) - 1
    worst = {}
    for ent, ref in zip(rs["table"], z[pre + "values"]):
        key, kind = ent["key"], ent["kind"]
        v = out["episode"][key]
        assert v.shape == (S,) and v.dtype == np.float64
        assert np.isnan(np.delete(v, ent["scene"])).all(), key                   # NaN except at the entry's scene
        got = v[ent["scene"]]
        if kind in GC.FLAG_KINDS:
            print(f"{key}: got {got!r} golden {ref!r}")
            assert got == ref, (key, got, ref)
            continue
        r = float(err_in_bound(got, ref, rs["n_terms"][key], rs["scale"][key]))
        worst[kind] = max(worst.get(kind, 0.0), r)
        print(f"{key}: got {got!r} golden {ref!r} |diff| / bound = {r:.3f}")
        assert r <= 1.0, (key, got, ref, r)
    print("largest |diff| / bound per kind:", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("name", ["main", "small"])
def test_per_member_values_against_the_restatement(eng, gold, name):
    z, meta = gold
    case, out = GC.case(name), run(eng, name)
    rs = case["restated"]
    pre = "" if name == "main" else "small_"
    off = 0
    for ent in rs["table"]:
        key, n = ent["key"], len(ent["members"])
        got, ref = out["per_member"][key], z[pre + "per_member"][off:off + n]
        off += n
        assert got.shape == (n,)
        if ent["kind"] in GC.FLAG_KINDS:
            assert np.array_equal(got, ref), (key, got, ref)
        else:
            terms = max(rs["n_terms"][key] // n, 1)
            r = err_in_bound(got, ref, terms, rs["scale"][key])
            assert (r <= 1.0).all(), (key, got, ref, r)


def test_flags_equal_rollout_metrics_bit_for_bit(eng):
    """Without exclusions and with agents=None the disk flag, the box flag and the disk off-road flag are RolloutMetrics' coll_disk,
    coll_any and off_road_disk on the same poses."""
    from cld_amd.metrics import RolloutMetrics
    case = GC.case("main")
    S = len(case["scene_start"]) - 1
    config = [[dict(name="agent_collision", weight=1.0, params=dict(buffer_dist=0.0), agents=None),
               dict(name="map_collision", weight=1.0, params={}, agents=None)] for _ in range(S)]
    gm = feed(make(eng, case, config=config, constraint=None), case)
    rm = RolloutMetrics(eng, case["scene_start"], case["extent"], case["world"][0], case["maps"], case["scene_map"], case["map_from_world"],
                        **case["cfg"])
    world = torch.from_numpy(case["world"]).cuda()
    flags = np.stack([rm.add_step(world[t], want_flags=True)[0].cpu().numpy() for t in range(world.shape[0])])       # [T, B, 4]
    T = flags.shape[0]
    ss = case["scene_start"]
    assert flags[..., 2].any() and (flags[..., 3] > 0).any() and (flags[..., 1] == 1).any() and (flags[..., 1] == 255).any()
    for s in range(S):
        r = slice(ss[s], ss[s + 1])
        assert np.array_equal(gm.per_member(f"guide_agent_collision_disk_s{s}g0").cpu().numpy(), flags[:, r, 2].max(0).astype(np.float64))
        assert np.array_equal(gm.per_member(f"guide_social_dist_s{s}g0").cpu().numpy(), flags[:, r, 2].max(0).astype(np.float64))      # buffer 0
        assert np.array_equal(gm.per_member(f"guide_agent_collision_s{s}g0").cpu().numpy(), (flags[:, r, 3] > 0).max(0).astype(np.float64))
        disk = np.where(flags[:, r, 1] == 255, 0, flags[:, r, 1]).sum(0).astype(np.float64) / float(T)               # absent: 0, in the denominator
        assert np.array_equal(gm.per_member(f"guide_map_collision_disk_s{s}g1").cpu().numpy(), disk)


@pytest.mark.parametrize("sizes", [(130, 300), (4200,)])
def test_the_mean_over_members_is_numpys(eng, sizes):
    """Scenes of more than 128 members (numpy's pairwise blocks split) and of more than the read kernel's staged 4,096: the entry value
    is np.mean of the per-member step fractions, bit for bit."""
    from cld_amd.metrics import GuidanceMetrics
    rng = np.random.default_rng(5)
    B, T = sum(sizes), 3
    ss = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    maps = np.kron(rng.integers(0, 2, (1, 3, 12, 12)).astype(np.float32), np.ones((8, 8), np.float32))
    mfw = np.array([[[1.0, 0.0, 48.0], [0.0, 1.0, 48.0], [0.0, 0.0, 1.0]]], np.float32)
    world = np.concatenate([rng.uniform(-40.0, 40.0, (T, B, 2)), rng.uniform(-3.0, 3.0, (T, B, 1))], -1).astype(np.float32)
    extent = np.tile(np.array([[4.5, 2.0, 1.5]], np.float32), (B, 1))
    config = [[dict(name="map_collision", weight=1.0, params={}, agents=None), dict(name="acc_limit", weight=1.0, params=dict(acc_limit=0.5),
                                                                                     agents=None)] for _ in sizes]
    gm = GuidanceMetrics(eng, config, ss, extent, world[0], maps=maps, scene_map=np.zeros(len(sizes), np.int32), map_from_world=mfw,
                         **GC.CFG)
    acc = rng.uniform(-2.0, 2.0, (T, B)).astype(np.float32)
    for t in range(T):
        gm.add_step(torch.from_numpy(world[t]), torch.zeros(B), torch.from_numpy(acc[t]))
    ep = gm.get_episode_metrics()
    for s, n in enumerate(sizes):
        for met in ("map_collision", "map_collision_disk"):
            pm = gm.per_member(f"guide_{met}_s{s}g0").cpu().numpy()
            assert pm.shape == (n,) and 0.0 < pm.mean() < 1.0 and set(np.unique(pm)) <= {0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0}
            assert float(ep[f"guide_{met}_s{s}g0"][s]) == np.mean(pm)
        r = slice(ss[s], ss[s + 1])
        ref = np.mean([np.mean(np.clip(np.abs(acc[t, r].astype(np.float64)) - 0.5, 0, None)) for t in range(T)])
        assert abs(float(ep[f"guide_acc_limit_s{s}g1"][s]) - ref) <= (T * n + 16) * 2.0 ** -52 * 2.0


def test_add_plans_equals_add_step_on_the_restated_pre_action_states(eng):
    case = GC.case("main")
    B = case["extent"].shape[0]
    g = torch.Generator().manual_seed(3)
    w0 = np.nan_to_num(case["world"][0]).astype(np.float32)
    sp0, ac0 = case["speed"][0], case["acc"][0]
    a, b = make(eng, case, world0=w0, curr_speed0=sp0, acc0=ac0), make(eng, case, world0=w0)
    plans = [(torch.randn(B, 52, 6, generator=g) * torch.tensor([3.0, 0.5, 1.0, 0.2, 1.0, 0.1])) for _ in range(2)]
    for p in plans:
        a.add_plans(p.cuda())
    W, V, A, carry = GC.pre_action_states(w0, sp0, ac0, [p.numpy() for p in plans])
    assert W.shape[0] == GC.N_STEPS - 1                                          # two plans score ten states; the eleventh is carried
    pose, speed, acc = torch.from_numpy(w0).cuda(), torch.from_numpy(sp0).cuda(), torch.from_numpy(ac0).cuda()
    t = 0
    for p in plans:
        pc = p.cuda()
        start = pose
        for k in range(5):
            assert np.abs(pose.cpu().numpy() - W[t]).max() <= 1e-4 and np.array_equal(speed.cpu().numpy(), V[t].astype(np.float32))
            assert np.array_equal(acc.cpu().numpy(), A[t].astype(np.float32))
            b.add_step(pose, speed, acc)
            t += 1
            pose = eng.world_step(pc, start[:, :2].contiguous(), start[:, 2].contiguous(), k)[0]
            speed, acc = pc[:, k, 2].contiguous(), pc[:, k, 4].contiguous()
    assert a.steps == b.steps == 10 and torch.equal(a.state, b.state)
    assert torch.equal(a.poses, pose) and torch.equal(a.speed, speed) and torch.equal(a.acc, acc)
    assert np.abs(a.poses.cpu().numpy() - carry[0]).max() <= 1e-4


def test_two_runs_give_the_same_bytes_and_reset_empties(eng):
    case = GC.case("main")
    first = run(eng, "main")
    m = feed(make(eng, case), case)
    assert np.array_equal(m.state.cpu().numpy(), first["state"])
    ep = m.get_episode_metrics()
    for k, v in first["episode"].items():
        assert np.array_equal(ep[k].cpu().numpy(), v, equal_nan=True), k
    m.reset()
    assert m.steps == 0 and not bool(m.state.any())
    ep = m.get_episode_metrics()
    for ent in case["restated"]["table"]:
        v = float(ep[ent["key"]][ent["scene"]])
        assert np.isinf(v) if ent["kind"] in ("target_pos", "global_target_pos") else np.isnan(v), ent["key"]


def test_bad_arguments_return_status_codes(eng):
    from cld_amd._lib import CldError
    from cld_amd.metrics import GuidanceMetrics
    case = GC.case("small")
    B = case["extent"].shape[0]
    args = (case["scene_start"], case["extent"], case["world"][0])
    with pytest.raises(ValueError, match="Unknown guidance metric: stop_sign"):
        GuidanceMetrics(eng, [[dict(name="stop_sign", weight=1.0, params={}, agents=None)]], *args)
    with pytest.raises(CldError, match="no entry"):
        GuidanceMetrics(eng, [[]], *args)
    with pytest.raises(CldError, match="scene_start"):
        GuidanceMetrics(eng, [[dict(name="speed_limit", weight=1.0, params=dict(speed_limit=1.0), agents=None)]], [0, B - 1], case["extent"],
                        case["world"][0])
    with pytest.raises(CldError, match="world0"):
        GuidanceMetrics(eng, case["config"], case["scene_start"], case["extent"], case["world"][0][:2])
    with pytest.raises(CldError, match="maps need"):
        GuidanceMetrics(eng, case["config"], *args, maps=np.zeros((1, 3, 8, 8), np.float32))
    m = GuidanceMetrics(eng, case["config"], *args, **case["cfg"])
    setup, state = m._setup, m.state
    world, zeros = torch.zeros(B, 3).cuda(), torch.zeros(B).cuda()
    for bad_state in (state[:-16], state.cpu(), state.view(torch.int32)):        # too short, not on the device, not bytes
        with pytest.raises(CldError, match="state"):
            eng.guide_metrics_step(setup, world, zeros, zeros, bad_state, 0)
        with pytest.raises(CldError, match="state"):
            eng.guide_metrics_read(setup, bad_state)
    with pytest.raises(CldError, match="global_t"):
        eng.guide_metrics_step(setup, world, zeros, zeros, state, -1)
    with pytest.raises(CldError, match="shape"):
        eng.guide_metrics_step(setup, world, zeros[:-1], zeros, state, 0)
    with pytest.raises(CldError, match="unknown kind"):
        eng.guide_metrics_setup(case["scene_start"], case["extent"], [dict(kind="stop_sign", scene=0, members=[0])])
    with pytest.raises(CldError, match="rows within"):
        eng.guide_metrics_setup(case["scene_start"], case["extent"], [dict(kind="speed_limit", scene=0, members=[B], params=[1.0])])
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = eng.lib.cld_guide_metrics_step(eng._h, C.byref(setup[0]), None, ptr(zeros), ptr(zeros), ptr(state), 0, eng._stream())
    assert rc != 0 and b"world" in eng.lib.cld_last_error(eng._h)
    rc = eng.lib.cld_guide_metrics_step(eng._h, C.byref(setup[0]), ptr(world), ptr(zeros), None, ptr(state), 0, eng._stream())
    assert rc != 0
    rc = eng.lib.cld_guide_metrics_read(eng._h, C.byref(setup[0]), ptr(state), None, None, eng._stream())
    assert rc != 0 and b"no output" in eng.lib.cld_last_error(eng._h)
    assert eng.lib.cld_guide_metrics_state_bytes(0, 5) == 0 and eng.lib.cld_guide_metrics_state_bytes(2, 5) == 2 * 32 + 5 * 80
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


def test_rollout_with_both_scorers_changes_no_pose():
    """closed_loop_rollout(metrics=(RolloutMetrics, GuidanceMetrics)) over 8 + 3 agents, 3 sim steps on a 10-step schedule: the poses are
    the bits of the run without metrics=, the guidance scorer saw 15 pre-action states and carries the last pose."""
    from cld_amd.metrics import GuidanceMetrics, RolloutMetrics
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
    config = [[dict(name="agent_collision", weight=1.0, params=dict(excluded_agents=[0, 1]), agents=None),
               dict(name="global_target_pos", weight=1.0, params=dict(target_pos=[[5.0, 5.0]]), agents=[2])],
              [dict(name="speed_limit", weight=1.0, params=dict(speed_limit=3.0), agents=None),
               dict(name="map_collision", weight=1.0, params={}, agents=None)]]

    def go(metrics):
        obs = SceneObserver(e, *args, n_step_action=5)
        return closed_loop_rollout(pol, obs, hw[:, -1, :2], hw[:, -1, 2], cs, n_sim_steps=S, n_step_action=5, gather=lambda traj: traj,
                                   noise=noise, **({} if metrics is None else {"metrics": metrics}))
    plain = go(None)
    rm = RolloutMetrics(e, case["scene_start"], extent, hw[:, -1], case["maps"], case["scene_map"], case["map_from_world"])
    gm = GuidanceMetrics(e, config, case["scene_start"], extent, hw[:, -1], curr_speed0=cs[:, 2], maps=case["maps"],
                         scene_map=case["scene_map"], map_from_world=case["map_from_world"])
    scored = go((rm, gm))
    assert torch.equal(plain, scored)
    assert rm.steps == 15 and gm.steps == 15 and torch.equal(gm.poses, scored[-1]) and torch.equal(rm.poses, scored[-1])
    ep = gm.get_episode_metrics()
    assert list(ep) == ["guide_agent_collision_disk_s0g0", "guide_social_dist_s0g0", "guide_agent_collision_s0g0", "guide_global_target_pos_s0g1",
                        "guide_speed_limit_s1g0", "guide_map_collision_s1g1", "guide_map_collision_disk_s1g1"]
    v = {k: t.cpu().numpy() for k, t in ep.items()}
    assert np.isfinite(v["guide_global_target_pos_s0g1"][0]) and np.isnan(v["guide_global_target_pos_s0g1"][1])
    assert v["guide_speed_limit_s1g0"][1] >= 0.0 and 0.0 <= v["guide_map_collision_s1g1"][1] <= 1.0
