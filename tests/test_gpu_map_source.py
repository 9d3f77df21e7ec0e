"""The map term of the collision guidance on the scene map (include/cld.h `cld_set_map_source`, csrc/collision_kernels.hip
map_collision_kernel<true>) and both collision terms following the observation over a closed loop.  Map mode must be BIT FOR BIT what
rasterising every agent at its pose (cld_rasterize) and running the raster form gives: values, gradients, and whole guided chains.  The
case (tests/map_source_cases.py; its properties are asserted on the CPU by tests/test_map_source_host.py) puts sampled pixels within
fp32 rounding of the boundary between two map pixels, where a lookup that rounds differently from raster_kernel picks the other one.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from cld_amd import synth
from tests import map_source_cases as MC

pytestmark = pytest.mark.gpu

COMBOS = [(r, g, f) for r in MC.RASTERS for g in MC.GRIDS for f in MC.FILLS]
CLD_ERR_ARG = -1
NO_SOURCE = "no map source is set"


@pytest.fixture(scope="module")
def eng(precision):
    from cld_amd.engine import Engine
    e = Engine(n_timesteps=10, device="cuda:0", precision=precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True))
    e.load_state_dict(synth.make_decoder_weights(0))
    return e.finalize()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def drivable(eng, c, fill, poses=None):
    """cld_rasterize's drivable bytes [A,H,W] for agents standing at the case's poses (a one-frame history)."""
    poses = _t(c["poses"]) if poses is None else poses
    A = poses.shape[0]
    return eng.rasterize(poses.reshape(A, 1, 3), torch.ones(A, 1, dtype=torch.uint8), _t(c["scene_start"]), _t(c["maps"]), _t(c["scene_map"]),
                         _t(c["map_from_world"]), want_raster_from_world=False, **dict(c["cfg"], no_map_fill=float(fill)))[1]


def raster_term(c, drv, grid, N):
    return dict(extent=_t(c["extent"]), raster_from_agent=_t(c["raster_from_agent"]), drivable_map=drv, curr_speed=_t(c["curr_speed"]),
                scene_sizes=c["sizes"], weight=c["weights"], num_samp=N, num_points_lw=grid)


def source(c, fill, poses=None):
    return dict(dict(c["cfg"], no_map_fill=float(fill)), maps=_t(c["maps"]), scene_map=_t(c["scene_map"]), map_from_world=_t(c["map_from_world"]),
                world=_t(c["poses"]) if poses is None else poses)


def map_term(c, fill, grid, N):
    t = raster_term(c, None, grid, N)
    del t["drivable_map"]
    return dict(t, map_source=source(c, fill))


_RESULTS = {}


def both_modes(eng, raster, grid, fill):
    """-> (drivable bytes, (loss, grad) in raster mode, (loss, grad) in map mode) on the case's plans; computed once per precision."""
    key = (eng.precision, raster, grid, fill)
    if key not in _RESULTS:
        c = MC.case(raster)
        traj = _t(c["plans"]).reshape(-1, 52, 6)
        drv = drivable(eng, c, fill)
        _RESULTS[key] = (drv, eng.map_collision(traj, raster_term(c, drv, grid, MC.NUM_SAMP)), eng.map_collision(traj, map_term(c, fill, grid, MC.NUM_SAMP)))
    return _RESULTS[key]


def assert_no_source_left(eng, c):
    """cld_map_collision_loss with drivable_map == NULL and nothing on the handle: CLD_ERR_ARG, and the message names the missing source."""
    traj = _t(c["plans"]).reshape(-1, 52, 6).cuda()
    cc, keep = eng._map_collision(map_term(c, -1.0, (10, 10), MC.NUM_SAMP), traj.shape[0])
    assert not cc.drivable_map
    loss = torch.empty(traj.shape[0], device="cuda")
    rc = eng.lib.cld_map_collision_loss(eng._h, C.c_void_p(traj.data_ptr()), C.byref(cc), None, C.c_void_p(loss.data_ptr()), None, traj.shape[0],
                                        eng._stream())
    assert rc == CLD_ERR_ARG and NO_SOURCE in eng.lib.cld_last_error(eng._h).decode()


@pytest.mark.parametrize("raster,grid,fill", COMBOS)
def test_map_mode_is_bit_for_bit_the_raster_mode(eng, raster, grid, fill):
    drv, (loss_r, grad_r), (loss_m, grad_m) = both_modes(eng, raster, grid, fill)
    c = MC.case(raster)
    differ = int((loss_r != loss_m).sum()), int((grad_r != grad_m).sum())
    print(f"{raster} {grid} fill {fill}: max value {float(loss_r.max()):.3f}, max|g| {float(grad_r.abs().max()):.3e}; elements that differ: "
          f"values {differ[0]}, gradient {differ[1]}")
    assert float(loss_r.max()) > 0.5 and float(grad_r.abs().max()) > 0.0
    assert torch.equal(loss_m, loss_r) and torch.equal(grad_m, grad_r)
    if fill == -1.0:                                                      # no map, fill -1: drivable everywhere
        assert float(loss_m.reshape(-1, MC.NUM_SAMP)[c["scene_index"] == 2].abs().max()) == 0.0
    assert_no_source_left(eng, c)


@pytest.mark.parametrize("raster,grid,fill", COMBOS)
def test_map_mode_vs_fp64_on_the_device_made_bytes(eng, raster, grid, fill):
    """oracle.map_collision_loss / map_collision_grad_bounds on the bytes cld_rasterize made, against map mode: the bars of
    test_map_collision_kernel_vs_oracle_multi_scene -- values to 2e-5, untied gradient elements to 1e-3 of max|g|, tied ones inside the
    interval their candidates span."""
    from oracle import cld_oracle as O
    drv, _, (loss, grad) = both_modes(eng, raster, grid, fill)
    c = MC.case(raster)
    A, N = c["poses"].shape[0], MC.NUM_SAMP
    x = _t(c["plans"])
    ext, rfa, spd, dm = _t(c["extent"]), _t(c["raster_from_agent"]), _t(c["curr_speed"]), drv.cpu()
    vref = O.map_collision_loss(x, ext, rfa, dm, spd, num_points_lw=grid).reshape(-1)
    xg = x.reshape(A * N, 52, 6).clone().requires_grad_(True)
    tot = O.scene_map_collision_total(xg, dict(extent=ext, raster_from_agent=rfa, drivable_map=dm, curr_speed=spd, scene_index=_t(c["scene_index"]),
                                               scene_weight=c["weights"], num_points_lw=grid), N)
    (gref,) = torch.autograd.grad(tot, xg)
    assert float(vref.max()) > 0.5 and float(gref.abs().max()) > 0.0
    assert float((loss.cpu() - vref).abs().max()) <= 2e-5 * max(1.0, float(vref.max()))
    coef = torch.tensor([c["weights"][int(s)] / (c["sizes"][int(s)] * N) for s in c["scene_index"]]).view(A, 1).expand(A, N)
    lo, hi, tied = O.map_collision_grad_bounds(x, ext, rfa, dm, spd, coef, num_points_lw=grid)
    gmax = float(gref.abs().max())
    got = grad.cpu().double().reshape(A, N, 52, 6)[..., [0, 1, 3]]
    ref3 = gref.double().reshape(A, N, 52, 6)[..., [0, 1, 3]]
    assert float(grad.cpu().reshape(A, N, 52, 6)[..., [2, 4, 5]].abs().max()) == 0.0
    assert float(torch.maximum(lo - ref3, ref3 - hi).max()) <= 1e-5 * gmax            # the oracle's own autograd gradient lies in its intervals
    out = torch.maximum(lo - got, got - hi).clamp(min=0)
    d_un = (got - ref3).abs()[~tied]
    print(f"{raster} {grid} fill {fill}: {int(tied.sum())} of {tied.numel()} (plan, step) pairs hang on a tie; untied: max |d| = "
          f"{float(d_un.max()) / gmax:.2e} of max|g|; tied: outside the interval by {float(out[tied].max()) / gmax if tied.any() else 0.0:.2e}")
    assert float(d_un.max()) <= 1e-3 * gmax
    assert float(out.max()) <= 1e-3 * gmax


@pytest.mark.parametrize("rows", [64, 256])
def test_guided_chain_in_map_mode_equals_raster_mode_in_every_guide_kernel_form(eng, rows):
    """Three guided steps of a 10-step schedule (t = 9, 8, 7; two SGD steps each) with agent_collision + map_collision, at 64 rows and at
    256 rows -- where the automatic path decodes with the guidance kernel's own forward sweep and runs its backward half as a second
    launch -- in every form of the guidance kernel: the map-mode chain is the raster-mode chain, bit for bit, and the map term acts."""
    from cld_amd.policy import frames_from_pose
    c = MC.tiled("vec", rows)
    inp = synth.make_inputs(rows, 61)
    cond, cs = _t(inp["cond_feat"]), _t(inp["curr_states"])
    speed = cs[:, 2].clone()
    S = len(c["sizes"])
    col = dict(extent=_t(c["extent"]), world_from_agent=frames_from_pose(_t(c["poses"])), curr_speed=speed, scene_index=_t(c["scene_index"]),
               weight=[40.0 + (s % 7) for s in range(S)])
    drv = drivable(eng, c, -1.0)
    terms = {"raster": dict(raster_term(c, drv, (10, 10), 1), curr_speed=speed), "map": dict(map_term(c, -1.0, (10, 10), 1), curr_speed=speed),
             "none": None}
    x_T = _t(synth.normal(61, "xt", (rows, 52, 4))) * 0.7
    zs = [_t(synth.normal(62 + k, "z", (rows, 52, 4))) for k in range(3)]

    def chain(term):
        gd = dict(curr_states=cs, lr=5.0, optimizer="sgd", grad_steps=2, agent_collision=col)
        if term is not None:
            gd["map_collision"] = term
        x, out = x_T, []
        for k, t in enumerate((9, 8, 7)):
            r = eng.sample_step(x, cond, t, z=zs[k], guidance=gd)
            out += [r["mean_guided"], r["x_next"]]
            x = r["x_next"]
        return out
    for kernel in ("auto", "valu", "mfma", "quad"):
        eng.force_kernel("guide", kernel)
        try:
            got = {k: chain(v) for k, v in terms.items()}
        finally:
            eng.force_kernel("guide", "auto")
        moved = float((got["map"][-1] - got["none"][-1]).abs().max())
        print(f"{rows} rows, guide kernel {kernel}: the map term moved x_7 by {moved:.3e}")
        assert moved > 1e-4, kernel
        for a, b in zip(got["map"], got["raster"]):
            assert torch.equal(a, b), kernel
    assert_no_source_left(eng, MC.case("vec"))


def test_no_source_outlives_its_call_and_bad_sources_are_refused(eng):
    from cld_amd._lib import CldError
    c = MC.case("vec")
    traj = _t(c["plans"]).reshape(-1, 52, 6)
    term = map_term(c, -1.0, (10, 10), MC.NUM_SAMP)
    good = eng.map_collision(traj, term)
    assert_no_source_left(eng, c)
    with pytest.raises(CldError, match="sample points"):                 # refused by the library, with the source already on the handle
        eng.map_collision(traj, dict(term, num_points_lw=(20, 20)))
    assert_no_source_left(eng, c)
    with pytest.raises(CldError, match="drivable_layer"):
        eng.map_collision(traj, dict(term, map_source=dict(term["map_source"], drivable_layer=MC.N_SEM)))
    assert_no_source_left(eng, c)
    with pytest.raises(CldError, match="px_per_m"):
        eng.map_collision(traj, dict(term, map_source=dict(term["map_source"], px_per_m=0.0)))
    with pytest.raises(CldError, match="scene_map"):                     # the source's scenes are the term's scenes
        eng.map_collision(traj, dict(term, map_source=dict(term["map_source"], scene_map=_t(c["scene_map"][:2]))))
    with pytest.raises(CldError, match="pass one"):
        eng.map_collision(traj, dict(term, drivable_map=drivable(eng, c, -1.0)))
    # the other drivable layer is another road: the layer is read
    other = eng.map_collision(traj, dict(term, map_source=dict(term["map_source"], drivable_layer=1)))
    assert not torch.equal(other[0], good[0])
    again = eng.map_collision(traj, term)
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])
    assert_no_source_left(eng, c)


def test_closed_loop_collision_guidance_follows_the_observation(precision):
    """2 scenes x 4 agents on converging headings beside a road edge, 3 sim steps of 5 executed states, a 10-step schedule, fixed noise.
    Run A: set_guidance once with follow_observation=True and a map source, then closed_loop_rollout.  Run B: a hand-written loop that
    calls set_guidance anew at every sim step with a data_batch built from that step's pose -- world_from_agent from frames_from_pose,
    curr_speed from the carried state, drivable_map from cld_rasterize at the pose.  The poses are the same bits; both terms are non-zero
    at sim steps 1 and 2; and a run on frozen frames (follow_observation=False) goes elsewhere."""
    from cld_amd.dm_model import DmModel
    from cld_amd.engine import Engine
    from cld_amd.policy import CldPolicy, closed_loop_rollout, frames_from_pose, raster_frames
    from cld_amd.vae_model import VaeModel
    e = Engine(n_timesteps=10, device="cuda:0", precision=precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True)); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
    pol = CldPolicy(DmModel(None, None, n_timesteps=10, engine=e), VaeModel(engine=e))
    c = MC.loop_case()
    B = 8
    cond = _t(synth.make_inputs(B, 71)["cond_feat"]).cuda()
    centroid, yaw, cs0 = _t(c["centroid"]), _t(c["yaw"]), _t(c["curr_states"])
    world0 = torch.cat([centroid, yaw[:, None]], dim=1)
    nz = synth.make_noise(B, 10, 9)
    noise = {"x_T": _t(nz["x_T"]).reshape(B, 1, 52, 4), "noise": _t(nz["noise"])}
    cfgs = [[{"name": "agent_collision", "weight": 100.0, "params": {}, "agents": None},
             {"name": "map_collision", "weight": 5.0, "params": {}, "agents": None}] for _ in range(2)]
    scene_index, extent = _t(c["scene_index"]), _t(c["extent"])
    opt = dict(lr=2.0, optimizer="sgd", grad_steps=2)
    ms = dict(c["cfg"], maps=_t(c["maps"]), scene_map=_t(c["scene_map"]), map_from_world=_t(c["map_from_world"]), world=world0)
    seen = []
    inner = pol.get_action

    def spy(obs, **kw):
        act, info = inner(obs, **kw)
        seen.append({k: float(torch.nansum(v.abs())) for k, v in info["guide_losses"].items()})
        return act, info
    pol.get_action = spy
    cond_fn = lambda step, world, cs: cond
    db0 = dict(extent=extent, world_from_agent=frames_from_pose(world0), curr_speed=cs0[:, 2])

    def run_a(follow):
        seen.clear()
        pol.set_guidance(cfgs, scene_index, data_batch=db0, follow_observation=follow, map_source=ms, **opt)
        return closed_loop_rollout(pol, cond_fn, centroid, yaw, cs0, 3, n_step_action=5, noise=noise), [dict(s) for s in seen]
    poses_a, losses_a = run_a(True)

    # Run B
    seen.clear()
    world, cs, poses_b = world0.cuda(), cs0.cuda(), []
    for step in range(3):
        db = dict(extent=extent, world_from_agent=frames_from_pose(world), curr_speed=cs[:, 2].contiguous(), raster_from_agent=raster_frames(c["cfg"], B),
                  drivable_map=drivable(e, c, -1.0, poses=world))
        pol.set_guidance(cfgs, scene_index, data_batch=db, **opt)
        _, info = pol.get_action({"cond_feat": cond, "curr_states": cs}, step_index=step, noise=noise)
        traj = info["executed_trajectory"].contiguous()
        world, cs = e.world_step(traj, world[:, :2].contiguous(), world[:, 2].contiguous(), 4)
        poses_b.append(world)
    poses_b, losses_b = torch.stack(poses_b), [dict(s) for s in seen]
    keys = [f"{name}_scene_{s:03d}_{k:02d}" for s in range(2) for k, name in enumerate(("agent_collision", "map_collision"))]
    for step in (1, 2):
        print(f"sim step {step}: guide losses (summed) A {losses_a[step]}")
        assert sorted(losses_a[step]) == sorted(keys) == sorted(losses_b[step])
        for k in keys:
            assert losses_a[step][k] > 0.0 and losses_b[step][k] > 0.0, (step, k)
    assert torch.equal(poses_a, poses_b)
    assert losses_a == losses_b
    poses_frozen, _ = run_a(False)
    print(f"frozen frames end {float((poses_frozen[-1, :, :2] - poses_a[-1, :, :2]).norm(dim=-1).max()):.3e} m from the run that follows the observation")
    assert torch.equal(poses_frozen[0], poses_a[0]) and not torch.equal(poses_frozen, poses_a)
    assert pol._guidance["map_collision"]["map_source"]["world"] is world0      # the configured source itself was never modified
