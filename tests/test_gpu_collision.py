"""GPU parity of round 3's widening of the guidance row: upstream's AgentCollisionLoss as a kernel
(csrc/collision_kernels.hip), grad_steps > 1 with the optimiser's state carried across the steps, and guide_clean.
Goldens `agent_collision` / `guidance_multi` were recorded from the reference's own classes (oracle/make_golden.py); larger
cases are checked against the oracle's autograd restatement, itself pinned by those goldens (tests/test_oracle_golden.py).
"""
import numpy as np
import pytest
import torch

from cld_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(precision):
    from cld_amd.engine import Engine
    e = Engine(n_timesteps=100, device="cuda:0", precision=precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True))
    e.load_state_dict(synth.make_decoder_weights(0))
    return e.finalize()


def _col_cfg(db, meta_tag, N=1):
    agents = {int(k): v for k, v in meta_tag.get("agents", {}).items()}
    return dict(extent=db["extent"], world_from_agent=db["world_from_agent"], curr_speed=db["curr_speed"], scene_index=db["scene_index"],
                weight=meta_tag["weights"], agents=agents or None, num_samp=N)


@pytest.mark.parametrize("tag", ["all", "scene1", "subset"])
def test_agent_collision_kernel_golden(golden, eng, tag):
    """Per-agent values and d total / d plans against the reference's AgentCollisionLoss + DiffuserGuidance + autograd."""
    from tests.test_oracle_golden import collision_inputs
    meta, g = golden("agent_collision")
    db = collision_inputs(meta)
    B, N = sum(meta["scenes"]), meta["N"]
    traj = torch.from_numpy(synth.make_collision_trajectories(B, N, db["curr_speed"].numpy(), meta["in_seed"])).reshape(B * N, 52, 6)
    loss, grad = eng.agent_collision(traj, _col_cfg(db, meta[tag], N))
    si = 1 if tag == "scene1" else 0
    per = g[f"{tag}_agent_collision_scene_{si:03d}_00"]
    ok = ~np.isnan(per)
    got = loss.cpu().numpy().reshape(B, N)
    assert np.abs(got[ok] - per[ok]).max() <= 2e-7
    ref = g[f"grad_{tag}"].reshape(B * N, 52, 6)
    assert np.abs(grad.cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()
    assert (np.abs(grad.cpu().numpy()) > 0).any()
    if tag == "subset":
        untouched = np.ones(B, bool); untouched[[0, 2, 3]] = False
        assert np.abs(grad.cpu().numpy().reshape(B, N, 52, 6)[untouched]).max() == 0.0


@pytest.mark.parametrize("tag", ["scene0", "scene1"])
def test_agent_collision_excluded_agents_golden(golden, eng, tag):
    """upstream's `excluded_agents` (guidance_loss.py:447,586-593) in the kernel: values and gradient against the reference's own
    AgentCollisionLoss(excluded_agents=...) through DiffuserGuidance + autograd; and through the policy's config adapter."""
    from tests.test_oracle_golden import collision_inputs
    from cld_amd.policy import guidance_from_config
    meta, g = golden("agent_collision_excluded")
    db = collision_inputs(meta)
    B, N = sum(meta["scenes"]), meta["N"]
    traj = torch.from_numpy(synth.make_collision_trajectories(B, N, db["curr_speed"].numpy(), meta["in_seed"])).reshape(B * N, 52, 6)
    cfg = dict(_col_cfg(db, meta[tag], N), excluded_agents=meta[tag]["excluded_agents"])
    loss, grad = eng.agent_collision(traj, cfg)
    si = int(tag[-1])
    per = g[f"{tag}_agent_collision_scene_{si:03d}_00"]
    ok = ~np.isnan(per)
    assert np.abs(loss.cpu().numpy().reshape(B, N)[ok] - per[ok]).max() <= 2e-7
    ref = g[f"grad_{tag}"].reshape(B * N, 52, 6)
    assert np.abs(grad.cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()
    loss0, _ = eng.agent_collision(traj, _col_cfg(db, meta[tag], N))
    assert float((loss0 - loss).abs().max()) > 5e-4                        # the exclusion matters on this scene
    # the same configuration as upstream writes it (a guidance config list), through the adapter
    cfgs = [[], []]
    cfgs[si] = [{"name": "agent_collision", "weight": meta[tag]["weights"][si], "agents": None,
                 "params": {"num_disks": 5, "buffer_dist": 0.2, "excluded_agents": meta[tag]["excluded_agents"]}}]
    gd = guidance_from_config(cfgs, db["scene_index"], data_batch=db)
    loss2, grad2 = eng.agent_collision(traj, dict(gd["agent_collision"], num_samp=N))
    assert torch.equal(loss2, loss) and torch.equal(grad2, grad)


def test_agent_collision_scene_larger_than_declared_is_refused_not_overrun(eng):
    """include/cld.h contract on cld_collision.max_scene_agents: a scene whose device-side scene_start holds more agents than the launch
    was sized for is not evaluated -- NaN values, gradient = grad_in (or 0) -- and the other scenes are unaffected."""
    import ctypes as C
    from cld_amd import _lib
    sizes, N = [12, 5], 1
    B = sum(sizes)
    sc = synth.make_collision_scene(sizes, 3, spacing=2.5)
    db = {k: torch.from_numpy(v) for k, v in sc.items()}
    traj = torch.from_numpy(synth.make_collision_trajectories(B, N, sc["curr_speed"], 3)).reshape(B, 52, 6).cuda()
    good_loss, good_grad = eng.agent_collision(traj, dict(extent=db["extent"], world_from_agent=db["world_from_agent"], curr_speed=db["curr_speed"],
                                                          scene_index=db["scene_index"], weight=[1.0, 1.0]))
    cc, keep = eng._collision(dict(extent=db["extent"], world_from_agent=db["world_from_agent"], curr_speed=db["curr_speed"],
                                   scene_index=db["scene_index"], weight=[1.0, 1.0]), B)
    cc.max_scene_agents = 8                                            # a caller that under-declares the 12-agent scene
    gin = torch.randn(B, 52, 6, device="cuda")
    loss = torch.zeros(B, device="cuda"); grad = torch.full((B, 52, 6), 7.0, device="cuda")
    eng._check(eng.lib.cld_agent_collision(eng._h, C.c_void_p(traj.data_ptr()), C.byref(cc), C.c_void_p(gin.data_ptr()), C.c_void_p(loss.data_ptr()),
                                           C.c_void_p(grad.data_ptr()), B, eng._stream()), "cld_agent_collision")
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss[:12]).all()) and torch.equal(grad[:12], gin[:12])
    assert torch.equal(loss[12:], good_loss[12:]) and float((grad[12:] - (good_grad[12:] + gin[12:])).abs().max()) <= 1e-6


def test_agent_collision_kernel_vs_oracle_at_scene_size(eng):
    """Two 64-agent scenes (the unit BASELINE's configs name) + a 5-agent one, 2 samples, both big scenes guided with different
    weights: values and gradient against the oracle's autograd; grad_in is added; deterministic."""
    from oracle import cld_oracle as O
    sizes, N = [64, 5, 64], 2
    B = sum(sizes)
    sc = synth.make_collision_scene(sizes, 11, spacing=3.0)
    db = {k: torch.from_numpy(v) for k, v in sc.items()}
    traj = torch.from_numpy(synth.make_collision_trajectories(B, N, sc["curr_speed"], 11)).reshape(B * N, 52, 6)
    wts = [1.0, 0.0, 2.5]
    x = traj.clone().requires_grad_(True)
    tot = O.scene_collision_total(x, dict(db, scene_weight=wts), N)
    (gref,) = torch.autograd.grad(tot, x)
    vref = O.agent_collision_loss(traj.reshape(B, N, 52, 6), db["extent"], db["world_from_agent"], db["curr_speed"], db["scene_index"]).reshape(-1)
    cfg = dict(extent=db["extent"], world_from_agent=db["world_from_agent"], curr_speed=db["curr_speed"], scene_index=db["scene_index"],
               weight=wts, num_samp=N)
    loss, grad = eng.agent_collision(traj, cfg)
    assert float(vref.max()) > 0.01                                   # the scene does collide
    assert float((loss.cpu() - vref).abs().max()) <= 1e-6
    assert float((grad.cpu() - gref).abs().max()) <= 1e-4 * float(gref.abs().max())
    gin = torch.randn(B * N, 52, 6)
    loss2, grad2 = eng.agent_collision(traj, cfg, grad_in=gin)
    assert torch.equal(loss2, loss) and float((grad2.cpu() - (grad.cpu() + gin)).abs().max()) <= 1e-6
    assert torch.equal(eng.agent_collision(traj, cfg)[1], grad)


@pytest.mark.parametrize("kernel", ["valu", "mfma", "quad"])
@pytest.mark.parametrize("case", ["ts_adam3", "ts_sgd3", "col_sgd1", "col_adam3"])
def test_guidance_multi_step_and_collision_golden(golden, eng, case, kernel):
    """The reference's perturb() with grad_steps = 3 (Adam / SGD state carried across the steps) and with an agent_collision
    config (one SGD step; three Adam steps), in every formulation of the guidance kernel."""
    from tests.test_oracle_golden import guidance_multi_inputs
    meta, g = golden("guidance_multi")
    cond, cs, mean, tgt, ts_scale, col_ts_scale, col = guidance_multi_inputs(meta)
    opt, lr, steps = meta["cases"][case]
    gd = dict(curr_states=cs, target_speed=tgt, lr=lr, perturb_th=None, optimizer=opt, grad_steps=steps)
    if case.startswith("ts_"):
        gd["loss_scale"] = ts_scale
    else:
        gd["loss_scale"] = col_ts_scale
        gd["agent_collision"] = dict(extent=col["extent"], world_from_agent=col["world_from_agent"], curr_speed=col["curr_speed"],
                                     scene_index=col["scene_index"], weight=meta["col_weights"])
    eng.force_kernel("guide", kernel)
    try:
        xg = eng.guidance_step(mean, cond, gd, sigma=0.5)
    finally:
        eng.force_kernel("guide", "auto")
    err = np.abs(xg.cpu().numpy() - g[f"guided_{case}"])
    if opt == "adam":
        # Adam's normalised step is sign-like where a gradient element is within rounding of zero: THERE an element may land up to lr per
        # step (3.5 lr with the bias corrections) from the reference; nowhere else.  Which elements those are is not assumed: the fp64
        # oracle's gradient of every one of the steps says so (flag = some step's |g| within 5 x the gradient tolerance 2e-5 max|g| that
        # tests/guided_checks.py holds the kernel to, or exactly zero).  Every element outside the flagged set must match to rounding.
        from oracle import cld_oracle as O
        wd64 = {k: v.double() for k, v in O.to_torch(synth.make_decoder_weights(meta["w_seed"])).items()}
        d = lambda t: t.double()
        tr = []
        kw = dict(grad_steps=steps, trace=tr)
        if case.startswith("ts_"):
            O.guidance_step(wd64, d(mean), d(cond), d(cs), d(tgt), d(ts_scale), lr, None, opt, **kw)
        else:
            c64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in col.items()}
            c64["scene_weight"] = meta["col_weights"]
            O.guidance_step(wd64, d(mean), d(cond), d(cs), d(tgt), d(col_ts_scale), lr, None, opt, collision=c64, **kw)
        G = torch.stack(tr).abs()                                       # [steps, B, 52, 4]
        flagged = (G.min(dim=0)[0] <= 1e-4 * float(G.max())).numpy()
        big = err > 2e-4
        print(f"   [{case}/{kernel}] elements flagged as near-zero-gradient: {int(flagged.sum())} of {flagged.size}; beyond rounding: {int(big.sum())} "
              f"(all flagged: {bool((~big | flagged).all())}); max err unflagged {err[~flagged].max():.2e}, flagged {err[flagged].max() if flagged.any() else 0.0:.2e}")
        assert (~big | flagged).all(), "an element whose gradient is well away from zero at every step differs from the reference"
        assert err.max() <= 3.5 * lr
    else:
        assert err.max() <= 2e-4 * max(1.0, float(np.abs(g[f"guided_{case}"] - mean.numpy()).max()))
    assert np.abs(g[f"guided_{case}"] - mean.numpy()).max() > 1e-3


def test_guided_sampling_step_with_collision_and_guide_clean_vs_oracle(eng):
    """cld_sample_step at t = 40 on two 6-agent scenes: collision + target-speed guidance, two SGD steps, on the posterior mean
    and (guide_clean) on the model's clean prediction, against the oracle's restatement of upstream's p_sample."""
    from oracle import cld_oracle as O
    sizes = [6, 6]
    B = sum(sizes)
    w, wd = O.to_torch(synth.make_unet_weights(0, affine_jitter=True)), O.to_torch(synth.make_decoder_weights(0))
    inp = synth.make_inputs(B, 21)
    cond, cs = torch.from_numpy(inp["cond_feat"]), torch.from_numpy(inp["curr_states"])
    sc = synth.make_collision_scene(sizes, 21)
    sc["curr_speed"] = inp["curr_states"][:, 2].copy()
    db = {k: torch.from_numpy(v) for k, v in sc.items()}
    x_t = torch.from_numpy(synth.normal(21, "xt", (B, 52, 4))) * 0.7
    z = torch.from_numpy(synth.normal(22, "z", (B, 52, 4)))
    tgt = torch.from_numpy(synth.uniform(21, "tgt", (B, 52), 0.0, 12.0))
    scale = torch.full((B,), 1.0 / (6 * 52))
    sched = O.schedule(100)
    for clean in (False, True):
        ref = O.sample_step(w, wd, sched, x_t, cond, 40, z, guidance=dict(curr_states=cs, target_speed=tgt, loss_scale=scale, lr=5.0, optimizer="sgd",
                            grad_steps=2, guide_clean=clean, collision=dict(db, scene_weight=[40.0, 60.0])))
        got = eng.sample_step(x_t, cond, 40, z=z, guidance=dict(curr_states=cs, target_speed=tgt, loss_scale=scale, lr=5.0, optimizer="sgd",
                              grad_steps=2, guide_clean=clean, agent_collision=dict(extent=db["extent"], world_from_agent=db["world_from_agent"],
                              curr_speed=db["curr_speed"], scene_index=db["scene_index"], weight=[40.0, 60.0])))
        sc_ = max(1.0, float(ref["mean"].abs().max()))
        assert float((got["mean"].cpu() - ref["mean"]).abs().max()) <= 1e-4 * sc_
        assert float((got["mean_guided"].cpu() - ref["mean_guided"]).abs().max()) <= 2e-4 * sc_
        assert float((got["x_next"].cpu() - ref["x_next"]).abs().max()) <= 2e-4 * sc_
        assert float((ref["mean_guided"] - ref["mean"]).abs().max()) > 1e-3


def test_collision_guidance_descends_the_loss_and_weight_zero_is_a_no_op(eng):
    """Property: gradient steps on the collision term lower the collision value of the decoded plans (a step size normalised by
    the first gradient), and in a short guided chain weight 0 reproduces the unguided chain bit for bit."""
    from cld_amd.engine import Engine
    sizes = [16]
    B = 16
    inp = synth.make_inputs(B, 5)
    cond, cs = torch.from_numpy(inp["cond_feat"]).cuda(), torch.from_numpy(inp["curr_states"]).cuda()
    sc = synth.make_collision_scene(sizes, 5, spacing=2.5)
    sc["curr_speed"] = inp["curr_states"][:, 2].copy()
    col = dict(extent=sc["extent"], world_from_agent=sc["world_from_agent"], curr_speed=sc["curr_speed"], scene_index=sc["scene_index"])
    mean = torch.from_numpy(synth.normal(5, "col_mean", (B, 52, 4))).cuda() * 0.5

    def value(z):
        return float(eng.agent_collision(eng.decode(z, cond, cs, descaled_output=True), dict(col, weight=1.0), want_grad=False).sum())
    gd = dict(curr_states=cs, lr=1.0, optimizer="sgd", agent_collision=dict(col, weight=1.0))
    _, g = eng.guidance_step(mean, cond, gd, sigma=0.0, want_grad=True)
    gmax = float(g.abs().max())
    assert gmax > 0.0
    c0 = value(mean)
    c1 = value(eng.guidance_step(mean, cond, dict(gd, lr=0.2 / gmax), sigma=0.0))
    c6 = value(eng.guidance_step(mean, cond, dict(gd, lr=0.2 / gmax, grad_steps=6), sigma=0.0))
    print(f"collision value of the decoded plans: {c0:.5f} -> {c1:.5f} (1 SGD step) -> {c6:.5f} (6 steps)")
    assert c0 > c1 > c6 > 0.0          # (most of the value is overlap at the first steps, which no plan can undo: the descent is slow but monotone)
    e = Engine(n_timesteps=10, device="cuda:0", precision=eng.precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True)); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
    nz = synth.make_noise(B, 10, 77)
    xT, noise = torch.from_numpy(nz["x_T"]), torch.from_numpy(nz["noise"])
    x_free, _, _ = e.sample(xT, cond, noise=noise, guidance=dict(curr_states=cs, lr=0.05, optimizer="sgd", grad_steps=2, agent_collision=dict(col, weight=0.0)))
    x_plain, _, _ = e.sample(xT, cond, noise=noise)
    assert torch.equal(x_free, x_plain)


def test_get_action_with_a_collision_config_and_guide_clean():
    """The policy surface (algos.py:2024-2099) with upstream's guidance configuration carrying an agent_collision entry: the
    per-sample collision values come back under upstream's key, equal to the oracle's on the returned trajectories; the loss is
    scene-level, so every agent of the scene executes the SAME sample (choose_action_from_guidance, guidance_loss.py:39-46);
    guide_clean=True runs (it used to raise) and changes the plans."""
    from cld_amd.dm_model import DmModel
    from cld_amd.engine import Engine
    from cld_amd.policy import CldPolicy
    from cld_amd.vae_model import VaeModel
    from oracle import cld_oracle as O
    e = Engine(n_timesteps=10, device="cuda:0")
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True)); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
    pol = CldPolicy(DmModel(None, None, n_timesteps=10, engine=e), VaeModel(engine=e))
    B, N = 7, 3
    inp = synth.make_inputs(B, 9)
    sc = synth.make_collision_scene([B], 9, spacing=2.5)
    sc["curr_speed"] = inp["curr_states"][:, 2].copy()
    db = {k: torch.from_numpy(v) for k, v in sc.items()}
    cfg = [[{"name": "agent_collision", "weight": 500.0, "params": {"num_disks": 5, "buffer_dist": 0.2}, "agents": None}]]
    pol.set_guidance(cfg, db["scene_index"], lr=0.1, optimizer="sgd", grad_steps=2, data_batch=db)
    obs = {"cond_feat": torch.from_numpy(inp["cond_feat"]).cuda(), "curr_states": torch.from_numpy(inp["curr_states"]).cuda()}
    nz = synth.make_noise(B * N, 10, 3)
    noise = {"x_T": torch.from_numpy(nz["x_T"]).reshape(B, N, 52, 4), "noise": torch.from_numpy(nz["noise"])}
    act, info = pol.get_action(obs, num_action_samples=N, noise=noise)
    key = "agent_collision_scene_000_00"
    assert list(info["guide_losses"]) == [key]
    traj = info["trajectories"].cpu()                                       # [B,N,52,6]
    ref = O.agent_collision_loss(traj, db["extent"], db["world_from_agent"], db["curr_speed"], db["scene_index"])
    assert float((info["guide_losses"][key].cpu() - ref).abs().max()) <= 1e-6
    idx = info["act_idx"].cpu()
    assert bool((idx == idx[0]).all()) and int(idx[0]) == int(torch.argmin(ref.sum(dim=0)))
    act2, info2 = pol.get_action(obs, num_action_samples=N, noise=noise, guide_clean=True)
    assert torch.isfinite(info2["trajectories"]).all() and not torch.equal(info2["trajectories"], info["trajectories"])


def _map_cfg(db, weight, N=1, sizes=None):
    c = dict(extent=db["extent"], raster_from_agent=db["raster_from_agent"], drivable_map=db["drivable_map"], curr_speed=db["curr_speed"],
             weight=weight, num_samp=N)
    if sizes is not None:
        c["scene_sizes"] = sizes
    return c


def test_map_collision_kernel_golden(golden, eng):
    """Upstream's MapCollisionLoss + DiffuserGuidance + autograd: per-plan values to rounding, the gradient to the ~0.3 % of
    noise the reference's torch.cdist backward carries (fixture generator), and one SGD step through perturb() in every
    formulation of the guidance kernel."""
    from tests.test_oracle_golden import map_inputs
    meta, g = golden("map_collision")
    B, N = meta["B"], meta["N"]
    db = map_inputs(B, meta["in_seed"])
    traj = torch.from_numpy(synth.make_map_trajectories(B, N, db["curr_speed"].numpy(), meta["in_seed"])).reshape(B * N, 52, 6)
    loss, grad = eng.map_collision(traj, _map_cfg(db, meta["weight"], N))
    assert np.abs(loss.cpu().numpy().reshape(B, N) - g["values"]).max() <= 2e-5
    ref = g["grad"].reshape(B * N, 52, 6)
    # No blanket percentage: the oracle says which (plan, step) elements the loss DEFINES and which hang on a tie between equidistant
    # on-road samples (O.map_collision_grad_bounds: the interval a tie admits; lo == hi elsewhere).  Untied steps are held to the
    # reference's own gradient, tied ones to the interval; the reference's gradient itself lies in it (checked: its cdist noise only
    # ever decided ties).
    from oracle import cld_oracle as O
    coef = torch.full((B, N), float(meta["weight"]) / (B * N))
    lo, hi, tied = O.map_collision_grad_bounds(traj.reshape(B, N, 52, 6), db["extent"], db["raster_from_agent"], db["drivable_map"], db["curr_speed"], coef)
    got = grad.cpu().double().reshape(B, N, 52, 6)
    gmax = float(np.abs(ref).max())
    assert float(got[..., [2, 4, 5]].abs().max()) == 0.0
    out = torch.maximum(lo - got[..., [0, 1, 3]], got[..., [0, 1, 3]] - hi).clamp(min=0)
    refo = torch.from_numpy(ref).double().reshape(B, N, 52, 6)[..., [0, 1, 3]]
    d_ref = (got[..., [0, 1, 3]] - refo).abs()
    print(f"map-collision gradient vs the reference: untied steps max {float(d_ref[~tied].max()) / gmax:.2e} of max|g|; {int(tied.sum())} tied steps, "
          f"outside their interval by {float(out[tied].max()) / gmax if tied.any() else 0.0:.2e}")
    assert float(torch.maximum(lo - refo, refo - hi).max()) <= 1e-4 * gmax          # the reference's own gradient is inside the interval
    assert float(d_ref[~tied].max()) <= 1e-3 * gmax
    assert float(out.max()) <= 1e-3 * gmax
    gm = meta["guided"]
    B2 = gm["B"]
    inp = synth.make_inputs(B2, meta["in_seed"])
    db2 = map_inputs(B2, meta["in_seed"] + 1, (0.6, 1.4))
    db2["curr_speed"] = torch.from_numpy(inp["curr_states"][:, 2].copy())
    mean = torch.from_numpy(synth.normal(meta["in_seed"], "guide_mean", (B2, 52, 4)))
    tgt = torch.from_numpy(synth.uniform(meta["in_seed"], "guide_target_speed", (B2, 52), 0.0, 12.0))
    gd = dict(curr_states=torch.from_numpy(inp["curr_states"]), target_speed=tgt, loss_scale=torch.full((B2,), gm["target_speed_weight"] / (B2 * 52)),
              lr=gm["lr"], optimizer="sgd", map_collision=_map_cfg(db2, gm["map_weight"]))
    moved = np.abs(g["guided_map_sgd1"] - mean.numpy()).max()
    for kernel in ("valu", "mfma", "quad"):
        eng.force_kernel("guide", kernel)
        try:
            xg = eng.guidance_step(mean, torch.from_numpy(inp["cond_feat"]), gd, sigma=0.5)
        finally:
            eng.force_kernel("guide", "auto")
        assert np.abs(xg.cpu().numpy() - g["guided_map_sgd1"]).max() <= 1e-2 * moved, kernel


def _offroad_counts(traj, db, grid):
    """[B,N,52] number of off-road samples per step, formed as oracle.map_collision_loss forms its flags."""
    lwise, wwise = torch.linspace(-0.5, 0.5, grid[0]), torch.linspace(-0.5, 0.5, grid[1])
    locs = torch.cartesian_prod(lwise, wwise).reshape(-1, 2)[None] * db["extent"][:, None, :2]
    c, s_ = torch.cos(traj[..., 3])[..., None], torch.sin(traj[..., 3])[..., None]
    lx, wy = locs[:, None, None, :, 0], locs[:, None, None, :, 1]
    pts = torch.stack([lx * c - wy * s_, lx * s_ + wy * c], dim=-1) + traj[..., None, :2]
    R = db["raster_from_agent"]
    pix = ((R[:, None, None, None, :2, :2] @ pts.unsqueeze(-1)).squeeze(-1) + R[:, None, None, None, :2, 2]).long()
    H, W = db["drivable_map"].shape[-2:]
    bi = torch.arange(traj.shape[0]).view(-1, 1, 1, 1).expand(pix.shape[:-1])
    return (db["drivable_map"][bi, pix[..., 1].clamp(0, H - 1), pix[..., 0].clamp(0, W - 1)] == 0).sum(dim=-1)


@pytest.mark.parametrize("grid", [(1, 16), (14, 1), (12, 6), (16, 16), (2, 1)])
def test_map_collision_kernel_vs_oracle_multi_scene(eng, grid):
    """Three scenes (40 + 7 + 30 agents, 2 samples, one scene unguided): values against the oracle to rounding, deterministic,
    grad_in added.  The gradient, element by element: along the box and on a two-dimensional grid an isolated off-road sample can sit
    between mirror-image on-road neighbours that are equidistant in exact arithmetic -- torch shares the gradient among the minima it
    finds bit-equal and otherwise takes whichever rounding made smaller, the kernel shares it among candidates within 1e-5.  The
    oracle separates the two kinds of element (O.map_collision_grad_bounds): steps without such a tie (every off-road sample's two
    nearest on-road samples more than 1e-4 m apart in distance) must match the oracle's autograd to 1e-3 of max|g|; steps with one
    must lie in the interval the tied candidates span (+ the same 1e-3).  No element is exempt.
    Grid (16, 16) is the kernel's sample-count limit, 256 points = four 64-lane chunks per step, with steps of more than 64 off-road
    samples (more than one pass of the search); its scenes are 3 + 1 + 2 agents, because the oracle's [B,N,T,P,P] table takes 0.3 GB per
    agent there.  Grid (2, 1) is the smallest that can overlap: one sample on the road and one off it."""
    from oracle import cld_oracle as O
    sizes, N = ([3, 1, 2] if grid == (16, 16) else [40, 7, 30]), 2
    B = sum(sizes)
    sc = synth.make_map_scene(B, 17)
    db = {k: torch.from_numpy(v) for k, v in sc.items()}
    db["scene_index"] = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    traj = torch.from_numpy(synth.make_map_trajectories(B, N, sc["curr_speed"], 17)).reshape(B * N, 52, 6)
    wts = [1.5, 0.0, 0.7]
    if grid == (16, 16):
        cnt = _offroad_counts(traj.reshape(B, N, 52, 6), db, grid)
        busy = (cnt > 64) & (cnt < 256) & (db["curr_speed"].abs() > 0.5).view(B, 1, 1) & (db["scene_index"] != 1).view(B, 1, 1)
        assert int(busy.sum()) >= 20                                   # counted steps of guided, moving agents with n_off > 64
    x = traj.clone().requires_grad_(True)
    tot = O.scene_map_collision_total(x, dict(db, scene_weight=wts, num_points_lw=grid), N)
    (gref,) = torch.autograd.grad(tot, x)
    vref = O.map_collision_loss(traj.reshape(B, N, 52, 6), db["extent"], db["raster_from_agent"], db["drivable_map"], db["curr_speed"], num_points_lw=grid).reshape(-1)
    cfg = dict(_map_cfg(db, wts, N, sizes), num_points_lw=grid)
    loss, grad = eng.map_collision(traj, cfg)
    # (the cases do overlap the kerb.  Two samples can give 1 - length / diagonal at the most, 0.135 for these boxes)
    assert float(vref.max()) > (0.5 if grid[0] * grid[1] > 2 else 0.05) and float(gref.abs().max()) > 0.0
    assert float((loss.cpu() - vref).abs().max()) <= 2e-5 * max(1.0, float(vref.max()))
    _, local = torch.unique_consecutive(db["scene_index"], return_inverse=True)
    coef = torch.tensor([wts[int(local[b])] / (sizes[int(local[b])] * N) for b in range(B)]).view(B, 1).expand(B, N)
    lo, hi, tied = O.map_collision_grad_bounds(traj.reshape(B, N, 52, 6), db["extent"], db["raster_from_agent"], db["drivable_map"], db["curr_speed"],
                                               coef, num_points_lw=grid)
    gmax = float(gref.abs().max())
    got = grad.cpu().double().reshape(B, N, 52, 6)[..., [0, 1, 3]]
    ref3 = gref.double().reshape(B, N, 52, 6)[..., [0, 1, 3]]
    assert float(grad.cpu().reshape(B, N, 52, 6)[..., [2, 4, 5]].abs().max()) == 0.0
    assert float(torch.maximum(lo - ref3, ref3 - hi).max()) <= 1e-5 * gmax            # the oracle's own autograd gradient lies in its intervals
    out = torch.maximum(lo - got, got - hi).clamp(min=0)
    d_un = (got - ref3).abs()[~tied]
    print(f"grid {grid}: {int(tied.sum())} of {tied.numel()} (plan, step) pairs hang on a tie; untied: max |d| = {float(d_un.max()) / gmax:.2e} of max|g|; "
          f"tied: outside the interval by {float(out[tied].max()) / gmax if tied.any() else 0.0:.2e}, interval width up to {float((hi - lo).max()) / gmax:.2e}")
    assert float(d_un.max()) <= 1e-3 * gmax
    assert float(out.max()) <= 1e-3 * gmax
    gin = torch.randn(B * N, 52, 6)
    _, grad2 = eng.map_collision(traj, cfg, grad_in=gin)
    assert float((grad2.cpu() - (grad.cpu() + gin)).abs().max()) <= 1e-6
    assert torch.equal(eng.map_collision(traj, cfg)[1], grad)


def test_sampling_step_with_both_collision_terms_vs_oracle(eng):
    """cld_sample_step with agent_collision + map_collision + target speed in one guided step (two SGD steps) against the oracle."""
    from oracle import cld_oracle as O
    sizes = [6, 6]
    B = sum(sizes)
    w, wd = O.to_torch(synth.make_unet_weights(0, affine_jitter=True)), O.to_torch(synth.make_decoder_weights(0))
    inp = synth.make_inputs(B, 21)
    cond, cs = torch.from_numpy(inp["cond_feat"]), torch.from_numpy(inp["curr_states"])
    sc = synth.make_collision_scene(sizes, 21)
    sc["curr_speed"] = inp["curr_states"][:, 2].copy()
    db = {k: torch.from_numpy(v) for k, v in sc.items()}
    ms = synth.make_map_scene(B, 23, half_width_m=(0.6, 1.4))
    mdb = {k: torch.from_numpy(v) for k, v in ms.items()}
    mdb["curr_speed"], mdb["scene_index"] = db["curr_speed"], db["scene_index"]
    x_t = torch.from_numpy(synth.normal(21, "xt", (B, 52, 4))) * 0.7
    z = torch.from_numpy(synth.normal(22, "z", (B, 52, 4)))
    tgt = torch.from_numpy(synth.uniform(21, "tgt", (B, 52), 0.0, 12.0))
    scale = torch.full((B,), 1.0 / (6 * 52))
    sched = O.schedule(100)
    t = torch.full((B,), 40, dtype=torch.long)
    mean = sched["x_t_cof"][40] * x_t - sched["noise_cof"][40] * O.unet_forward(w, x_t, cond, t)
    sigma = float((0.5 * sched["posterior_log_variance_clipped"][40]).exp())
    ref, _ = O.guidance_step(wd, mean, cond, cs, tgt, scale, 5.0, None, "sgd", collision=dict(db, scene_weight=[40.0, 60.0]),
                             grad_steps=2, map_collision=dict(mdb, scene_weight=[0.3, 0.2]))
    got = eng.sample_step(x_t, cond, 40, z=z, guidance=dict(curr_states=cs, target_speed=tgt, loss_scale=scale, lr=5.0, optimizer="sgd", grad_steps=2,
                          agent_collision=dict(extent=db["extent"], world_from_agent=db["world_from_agent"], curr_speed=db["curr_speed"],
                                               scene_index=db["scene_index"], weight=[40.0, 60.0]),
                          map_collision=dict(_map_cfg(mdb, [0.3, 0.2]), scene_index=db["scene_index"])))
    sc_ = max(1.0, float(mean.abs().max()))
    assert float((got["mean_guided"].cpu() - ref).abs().max()) <= 2e-4 * sc_
    assert float((got["x_next"].cpu() - (ref + sigma * z)).abs().max()) <= 2e-4 * sc_
    assert float((ref - mean).abs().max()) > 1e-3


@pytest.mark.parametrize("sizes", [[64, 64, 64, 64], [64] * 8])
def test_collision_guided_step_at_the_batch_sizes_that_take_the_forward_sweep_path(eng, sizes):
    """From 256 rows a collision- / map-guided optimiser step decodes the current iterate with the guidance kernel's OWN forward sweep
    (guide_quad_kernel stopped behind its forward half, actions parked in the gradient buffer) + the O(T) roll-out kernel with scaled
    input, instead of cld_decode's kernel (csrc/cld_api.hip run_guidance) -- the default at the headline's 2,048 agents.  Checked here at
    256 and 512 agents (4 / 8 scenes of 64): the guided mean of the automatic path against the same step with the decoder forced
    (which takes launch_decode), <= 1e-5 of the mean's scale, and -- at 256 agents -- against the oracle's autograd restatement."""
    from oracle import cld_oracle as O
    B = sum(sizes)
    inp = synth.make_inputs(B, 31)
    cond, cs = torch.from_numpy(inp["cond_feat"]), torch.from_numpy(inp["curr_states"])
    sc = synth.make_collision_scene(sizes, 31, spacing=3.0)
    sc["curr_speed"] = inp["curr_states"][:, 2].copy()
    db = {k: torch.from_numpy(v) for k, v in sc.items()}
    ms = synth.make_map_scene(B, 33, half_width_m=(0.6, 1.4))
    mdb = {k: torch.from_numpy(v) for k, v in ms.items()}
    mdb["curr_speed"], mdb["scene_index"] = db["curr_speed"], db["scene_index"]
    mean = torch.from_numpy(synth.normal(31, "fwd_path_mean", (B, 52, 4))) * 0.7
    tgt = torch.from_numpy(synth.uniform(31, "fwd_path_tgt", (B, 52), 0.0, 12.0))
    scale = torch.full((B,), 1.0 / (64 * 52))
    S = len(sizes)
    wcol, wmap = [40.0 + 5.0 * s for s in range(S)], [0.3 + 0.05 * s for s in range(S)]
    gd = dict(curr_states=cs, target_speed=tgt, loss_scale=scale, lr=5.0, optimizer="sgd", grad_steps=2,
              agent_collision=dict(extent=db["extent"], world_from_agent=db["world_from_agent"], curr_speed=db["curr_speed"],
                                   scene_index=db["scene_index"], weight=wcol),
              map_collision=dict(_map_cfg(mdb, wmap), scene_index=db["scene_index"]))
    auto = eng.guidance_step(mean, cond, gd, sigma=0.3).clone()
    eng.force_kernel("decode", "mfma")
    try:
        forced = eng.guidance_step(mean, cond, gd, sigma=0.3).clone()
    finally:
        eng.force_kernel("decode", "auto")
    sc_ = max(1.0, float(mean.abs().max()))
    moved = float((auto.cpu() - mean).abs().max())
    d = float((auto - forced).abs().max())
    print(f"forward-sweep decode path vs launch_decode at {B} agents: max|d| = {d:.3e}; the guided step moved the mean by {moved:.3e}")
    assert moved > 3e-4 and d <= 1e-5 * sc_
    if B == 256:
        wd = O.to_torch(synth.make_decoder_weights(0))
        ref, _ = O.guidance_step(wd, mean, cond, cs, tgt, scale, 5.0, None, "sgd", collision=dict(db, scene_weight=wcol),
                                 grad_steps=2, map_collision=dict(mdb, scene_weight=wmap))
        err = float((auto.cpu() - ref).abs().max())
        print(f"   vs the oracle: {err:.3e}")
        assert err <= 2e-4 * sc_


def test_map_collision_constructed_tie_is_shared_evenly(eng):
    """ONE off-road sample of a 5-point line along the box with on-road neighbours at exactly equal distance on both sides (drivable
    everywhere but the pixel column under the middle sample): upstream's torch.amin backward gives the whole pull to whichever
    neighbour rounding made nearer -- parity unpinned by nature -- the kernel shares it evenly, so the pull along the
    line cancels.  Value exact; gradient inside the interval the two candidates span (oracle.map_collision_grad_bounds), and zero along x."""
    from oracle import cld_oracle as O
    ext = torch.tensor([[4.0, 2.0, 1.5]])
    rfa = torch.tensor([[[2.0, 0.0, 100.0], [0.0, 2.0, 100.0], [0.0, 0.0, 1.0]]])
    dm = torch.ones(1, 200, 200, dtype=torch.bool)
    dm[0, :, 100] = False
    x = torch.zeros(1, 52, 6)
    x[..., 0] = 0.25
    spd = torch.tensor([5.0])
    cfg = dict(extent=ext, raster_from_agent=rfa, drivable_map=dm, curr_speed=spd, weight=1.0, num_samp=1, num_points_lw=(5, 1))
    loss, grad = eng.map_collision(x, cfg)
    vref = O.map_collision_loss(x.reshape(1, 1, 52, 6), ext, rfa, dm, spd, num_points_lw=(5, 1))
    assert float(vref) > 0.0 and abs(float(loss.cpu()) - float(vref)) <= 1e-6
    lo, hi, tied = O.map_collision_grad_bounds(x.reshape(1, 1, 52, 6), ext, rfa, dm, spd, torch.ones(1, 1), num_points_lw=(5, 1))
    got = grad.cpu().double().reshape(1, 1, 52, 6)[..., [0, 1, 3]]
    assert bool(tied.all()) and float(torch.maximum(lo - got, got - hi).max()) <= 1e-9
    assert float(got[..., 0].abs().max()) <= 1e-9 and float(lo[..., 0].max()) < 0.0 < float(hi[..., 0].min())
