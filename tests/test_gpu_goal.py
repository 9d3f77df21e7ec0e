"""GPU parity of the global waypoint guidance (csrc/goal_kernels.hip; upstream's GlobalTargetPosLoss / GlobalTargetPosAtTimeLoss,
guidance_loss.py:876-1135): the kernel against the recording made from the reference's own classes (tests/golden/global_goal.npz) and
against the fp64 yardstick (tests/goal_yardstick.py, pinned by that recording: tests/test_goal_host.py); the term inside the guided
sampler (cld_set_goal_term) in every formulation of the guidance kernel; the policy surface and the closed-loop rollout.

Every row of every test lies >= 1e-3 m from every kink of the value (the relu arguments, the exact / progress boundary, the tolerance)
and reads no distance below 1e-2 m: asserted on the yardstick, no row excluded.
"""
import numpy as np
import pytest
import torch

from cld_amd import synth
from tests import goal_yardstick as Y

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(precision):
    from cld_amd.engine import Engine
    e = Engine(n_timesteps=100, device="cuda:0", precision=precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True))
    e.load_state_dict(synth.make_decoder_weights(0))
    return e.finalize()


def engine_goal(goal, N=1):
    """The yardstick's goal dict (fp64) as Engine.goal_loss / the guidance dict take it."""
    return dict({k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in goal.items()}, num_samp=N)


def check_margins(plans, goal):
    kink, dmin = Y.margins(plans.double(), goal)
    assert kink >= 1e-3 and dmin >= 1e-2, (kink, dmin)
    return kink, dmin


def check_kernel(eng, plans, goal, ref_v, ref_g, rows_without_gradient):
    """Engine.goal_loss on plans [A,N,52,6] against reference values [A,N] / gradient [A,N,52,6]: the two bars of the recording, exact
    zeros where nothing is guided, grad_in added, bit-identical on a second run."""
    A, N = plans.shape[:2]
    ge = engine_goal(goal, N)
    loss, grad = eng.goal_loss(plans.reshape(A * N, 52, 6), ge)
    got_v, got_g = loss.cpu().double().reshape(A, N), grad.cpu().double().reshape(A, N, 52, 6)
    err_v, err_g = float((got_v - ref_v).abs().max()), float((got_g - ref_g).abs().max())
    print(f"   values: max error {err_v:.2e} (max|ref| {float(ref_v.abs().max()):.3f}); gradient: {err_g:.2e} (max|ref| {float(ref_g.abs().max()):.3e})")
    assert err_v <= 2e-5 * max(1.0, float(ref_v.abs().max()))
    assert float(ref_g.abs().max()) > 0 and err_g <= 1e-4 * float(ref_g.abs().max())
    assert float(got_g[rows_without_gradient].abs().max()) == 0.0 and float(got_v[rows_without_gradient].abs().max()) == 0.0
    assert float(got_g[..., 2:].abs().max()) == 0.0                      # only x, y receive a contribution
    gin = torch.from_numpy(synth.normal(3, "goal_grad_in", (A * N, 52, 6)))
    loss2, grad2 = eng.goal_loss(plans.reshape(A * N, 52, 6), ge, grad_in=gin)
    assert torch.equal(loss2, loss) and float((grad2.cpu() - (grad.cpu() + gin)).abs().max()) <= 1e-6
    loss3, grad3 = eng.goal_loss(plans.reshape(A * N, 52, 6), ge)
    assert torch.equal(loss3, loss) and torch.equal(grad3, grad)
    assert torch.equal(eng.goal_loss(plans.reshape(A * N, 52, 6), ge, want_grad=False), loss)


@pytest.mark.parametrize("name", ["pos", "pos2", "time", "time2"])
def test_goal_kernel_golden(golden, eng, name):
    """The fixture's 16 rows, cases 1-3: per-row values and d total / d plans against the reference's own loss classes through
    DiffuserGuidance.compute_guidance_loss + autograd."""
    from tests.test_goal_host import recorded_case
    meta, g, plans, goal, idx = recorded_case(golden, name)
    check_margins(plans, goal)
    ref_v = torch.from_numpy(np.nan_to_num(g[name + "_values"], nan=0.0)).double()        # outside the config's agents the kernel reports 0
    ref_g = torch.from_numpy(g[name + "_grad"]).double()
    quiet = torch.tensor([b in ("off", "reached", "passed") for b in Y.branches(goal)])      # outside the subset, arrived, target time passed
    assert int(quiet.sum()) >= 1
    check_kernel(eng, plans, goal, ref_v, ref_g, quiet)


def many_branch_case(sizes, N, seed, global_t=9):
    """Agents of `sizes` scenes with plans from synth and, agent by agent in turn, one of nine roles that cover the six branches of the
    value (off; exact; progress with an active and with an inactive relu; target time passed / inside the plan / beyond it with an active
    and with an inactive relu) and a reached agent.  Targets are placed relative to the agent's own plans, so that every row is well
    away from the kinks.  -> (plans [A,N,52,6] float32, goal fp64, roles)."""
    A = sum(sizes)
    sc = synth.make_collision_scene(sizes, seed)
    plans = torch.from_numpy(synth.make_collision_trajectories(A, N, sc["curr_speed"], seed))
    W = torch.from_numpy(sc["world_from_agent"]).double()
    end = plans[:, :, -1, :2].double().mean(dim=1)                                          # mean end point of the agent's plans
    roles = ["off", "exact", "progress", "progress0", "passed", "at_time", "on_time", "on_time0", "reached"]
    goal = dict(kind=torch.zeros(A, dtype=torch.int32), target_time=torch.zeros(A, dtype=torch.int32), urgency=torch.full((A,), 0.5, dtype=torch.float64),
                pref_speed=torch.full((A,), 1.42, dtype=torch.float64), scale=torch.zeros(A, dtype=torch.float64), reached=torch.zeros(A, dtype=torch.bool),
                global_t=global_t, dt=0.1, min_progress_dist=0.5)
    local = torch.zeros(A, 2, dtype=torch.float64)
    got = []
    for a in range(A):
        r = roles[a % len(roles)]
        got.append(r)
        goal["scale"][a] = 0.3 + 0.1 * (a % 4)
        goal["kind"][a] = 0 if r == "off" else (1 if r in ("exact", "progress", "progress0", "reached") else 2)
        if r in ("exact", "reached"):
            local[a] = torch.tensor([3.0, 2.5])
            goal["reached"][a] = r == "reached"
        elif r == "progress":                       # a target abeam: no plan gets 7.4 m closer to it
            local[a], goal["urgency"][a] = torch.tensor([0.5, 12.0]), 1.0
        elif r == "progress0":                      # a target far ahead on the plans' own course: they all make more than min_progress_dist
            local[a], goal["urgency"][a] = end[a] * 3.0 + torch.tensor([30.0, 0.0]), 0.01
        elif r == "passed":
            local[a], goal["target_time"][a] = torch.tensor([5.0, 1.0]), global_t - 3
        elif r == "at_time":
            local[a], goal["target_time"][a] = torch.tensor([10.0, 2.0]), global_t + 17
        elif r == "on_time":
            local[a], goal["target_time"][a] = end[a] + torch.tensor([200.0, 0.0]), global_t + 60
        elif r == "on_time0":
            local[a], goal["target_time"][a], goal["urgency"][a] = end[a] + torch.tensor([1.0, 1.0]), global_t + 400, 0.0
    goal["target_pos"] = (torch.einsum("aij,aj->ai", W[:, :2, :2], local) + W[:, :2, 2]).float().double()
    goal["agent_from_world"] = Y.invert_frames(W).float().double()
    return plans, goal, got


def test_goal_kernel_vs_yardstick_all_branches_at_27_rows(eng):
    """Two scenes of 5 + 4 agents x 3 samples = 27 rows (no multiple of the four rows of a workgroup; num_samp does not divide a wave):
    all six branches of the value, at least two rows each, against the fp64 yardstick's values and autograd gradient."""
    plans, goal, roles = many_branch_case([5, 4], 3, 17)
    A, N = plans.shape[:2]
    br = Y.branches(goal)
    v, g = Y.value_and_grad(plans.double(), goal)
    active = {r: [bool(x > 0) for x in v[a]] for a, r in enumerate(roles)}
    assert br == ["off", "exact", "progress", "progress", "passed", "at_time", "on_time", "on_time", "reached"]
    assert all(active["progress"]) and not any(active["progress0"]) and all(active["on_time"]) and not any(active["on_time0"])
    for b in ("off", "exact", "progress", "passed", "at_time", "on_time"):
        assert br.count(b) * N >= 2
    kink, dmin = check_margins(plans, goal)
    print(f"27 rows: kink margin {kink:.3e} m, smallest distance read {dmin:.3e} m")
    quiet = torch.tensor([b in ("off", "reached", "passed") for b in br])
    check_kernel(eng, plans, goal, v, g, quiet)


def guided_case(A, N, seed):
    """A guided step's inputs at A agents x N samples: latent means, conditioning, current states, and goals of every branch placed
    relative to the plans the fp64 decoder gives for those means.  -> (mean, cond, cs [A N,...] float32, goal fp64, decoder weights fp64)."""
    from oracle import cld_oracle as O
    B = A * N
    inp = synth.make_inputs(B, seed)
    cond, cs = torch.from_numpy(inp["cond_feat"]), torch.from_numpy(inp["curr_states"])
    mean = torch.from_numpy(synth.normal(seed, "goal_mean", (B, 52, 4))) * 0.7
    wd64 = {k: v.double() for k, v in O.to_torch(synth.make_decoder_weights(0)).items()}
    with torch.no_grad():
        plans = O.decode(wd64, mean.double(), cond.double(), cs.double(), True).reshape(A, N, 52, 6)
    end = plans[:, :, -1, :2].mean(dim=1)
    goal = dict(kind=torch.zeros(A, dtype=torch.int32), target_time=torch.zeros(A, dtype=torch.int32), urgency=torch.full((A,), 0.5, dtype=torch.float64),
                pref_speed=torch.full((A,), 1.42, dtype=torch.float64), scale=torch.ones(A, dtype=torch.float64), reached=torch.zeros(A, dtype=torch.bool),
                global_t=4, dt=0.1, min_progress_dist=0.5)
    local = torch.zeros(A, 2, dtype=torch.float64)
    for a in range(A):
        r = a % 6
        goal["kind"][a] = 0 if r == 5 else (1 if r < 2 else 2)
        if r == 0:                                   # exact
            local[a] = torch.tensor([3.0, 2.5])
        elif r == 1:                                 # progress, active: a target abeam
            local[a], goal["urgency"][a] = torch.tensor([0.5, 12.0]), 1.0
        elif r == 2:                                 # inside the plan
            local[a], goal["target_time"][a] = end[a] * 0.5 + torch.tensor([1.0, 2.0]), 4 + 30
        elif r == 3:                                 # beyond the plan, behind schedule
            local[a], goal["target_time"][a] = end[a] + torch.tensor([60.0, 5.0]), 4 + 70
        elif r == 4:                                 # target time passed: no gradient
            local[a], goal["target_time"][a] = torch.tensor([5.0, 1.0]), 1
    goal["target_pos"] = local.float().double()      # identity frames: the world frame is every agent's own
    goal["agent_from_world"] = torch.eye(3, dtype=torch.float64).repeat(A, 1, 1)
    return mean, cond, cs, goal, wd64


def check_guided_step(eng, A, N, seed, kernel):
    from oracle import cld_oracle as O
    mean, cond, cs, goal, wd64 = guided_case(A, N, seed)
    d = lambda t: t.double()
    _, g1 = Y.sgd_step(wd64, d(mean), d(cond), d(cs), goal, 0.0, 1, N)
    lr = 0.05 / float(g1.abs().max())                                    # a step size normalised by the first gradient
    ref, gref = Y.sgd_step(wd64, d(mean), d(cond), d(cs), goal, lr, 2, N)
    x1, _ = Y.sgd_step(wd64, d(mean), d(cond), d(cs), goal, lr, 1, N)
    with torch.no_grad():
        for x in (d(mean), x1):                                          # both iterates the two steps evaluate the loss on
            check_margins(O.decode(wd64, x, d(cond), d(cs), True).reshape(A, N, 52, 6), goal)
    gd = dict(curr_states=cs, goal=engine_goal(goal, N), optimizer="sgd", lr=lr, grad_steps=2)
    if kernel != "auto":
        eng.force_kernel("guide", kernel)
    try:
        mg, grad = eng.guidance_step(mean, cond, gd, sigma=0.0, want_grad=True)
    finally:
        eng.force_kernel("guide", "auto")
    err_m, err_g = float((mg.cpu().double() - ref).abs().max()), float((grad.cpu().double() - gref).abs().max())
    moved = float((ref - mean).abs().max())
    print(f"   [{A * N} rows / {kernel}] guided mean: max error {err_m:.2e}, moved by {moved:.2e}; gradient: {err_g:.2e} of max {float(gref.abs().max()):.2e}")
    assert moved > 1e-3
    assert err_m <= 2e-4 * max(1.0, float(mean.abs().max()))
    assert err_g <= 1e-4 * float(gref.abs().max())


@pytest.mark.parametrize("kernel", ["valu", "mfma", "quad"])
def test_goal_guided_step_vs_yardstick_in_every_guide_kernel_form(eng, kernel):
    """cld_guidance_step with the goal term on the handle: two SGD steps at 6 agents x 3 samples = 18 rows, against the yardstick's SGD
    written out over the oracle's decoder."""
    check_guided_step(eng, 6, 3, 51, kernel)


def test_goal_guided_step_on_the_forward_sweep_path_at_256_rows(eng):
    """From 256 rows run_guidance decodes the iterate with the guidance kernel's own forward sweep + the roll-out kernel: the goal
    kernel runs behind that path too."""
    check_guided_step(eng, 128, 2, 53, "auto")


def test_sampling_step_with_goal_collision_and_target_speed_vs_oracle(eng):
    """cld_sample_step at t = 40, two scenes of 6 agents: goal + agent_collision + target_speed in one guided step (two SGD steps)
    against the yardstick's goal total + the oracle's collision total and target-speed loss."""
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
    t = torch.full((B,), 40, dtype=torch.long)
    mean = sched["x_t_cof"][40] * x_t - sched["noise_cof"][40] * O.unet_forward(w, x_t, cond, t)
    sigma = float((0.5 * sched["posterior_log_variance_clipped"][40]).exp())
    # goals in the world frame of the collision scene: two of every kind per scene
    W = db["world_from_agent"].double()
    local = torch.tensor([[3.0, 2.5], [0.5, 12.0], [12.0, 2.0], [150.0, 5.0], [5.0, 1.0], [0.0, 0.0]] * 2, dtype=torch.float64)
    goal = dict(kind=torch.tensor([1, 1, 2, 2, 2, 0] * 2, dtype=torch.int32), target_time=torch.tensor([0, 0, 40, 90, 2, 0] * 2, dtype=torch.int32),
                urgency=torch.tensor([0.5, 1.0, 0.5, 0.5, 0.5, 0.5] * 2, dtype=torch.float64), pref_speed=torch.full((B,), 1.42, dtype=torch.float64),
                scale=torch.full((B,), 2.0 / 5, dtype=torch.float64), reached=torch.zeros(B, dtype=torch.bool), global_t=10, dt=0.1, min_progress_dist=0.5,
                target_pos=(torch.einsum("aij,aj->ai", W[:, :2, :2], local) + W[:, :2, 2]).float().double(),
                agent_from_world=Y.invert_frames(W).float().double())
    col = dict(db, scene_weight=[40.0, 60.0])

    def extra(traj):
        return ((traj[..., 2] - tgt).abs().sum(dim=1) * scale).sum() + O.scene_collision_total(traj, col, 1)
    goal32 = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in goal.items()}
    ref, _ = Y.sgd_step(wd, mean, cond, cs, goal32, 5.0, 2, 1, extra=extra)
    x1, _ = Y.sgd_step(wd, mean, cond, cs, goal32, 5.0, 1, 1, extra=extra)
    wd64 = {k: v.double() for k, v in wd.items()}
    with torch.no_grad():
        for x in (mean, x1):
            check_margins(O.decode(wd64, x.double(), cond.double(), cs.double(), True).reshape(B, 1, 52, 6), goal)
    without, _ = O.guidance_step(wd, mean, cond, cs, tgt, scale, 5.0, None, "sgd", collision=col, grad_steps=2)
    assert float((ref - without).abs().max()) > 1e-3                     # the goal term matters in this step
    got = eng.sample_step(x_t, cond, 40, z=z, guidance=dict(curr_states=cs, target_speed=tgt, loss_scale=scale, lr=5.0, optimizer="sgd", grad_steps=2,
                          goal=engine_goal(goal),
                          agent_collision=dict(extent=db["extent"], world_from_agent=db["world_from_agent"], curr_speed=db["curr_speed"],
                                               scene_index=db["scene_index"], weight=[40.0, 60.0])))
    sc_ = max(1.0, float(mean.abs().max()))
    print(f"   guided mean: max error {float((got['mean_guided'].cpu() - ref).abs().max()):.2e} of scale {sc_:.2f}; the goal term moved it by "
          f"{float((ref - without).abs().max()):.2e}")
    assert float((got["mean_guided"].cpu() - ref).abs().max()) <= 2e-4 * sc_
    assert float((got["x_next"].cpu() - (ref + sigma * z)).abs().max()) <= 2e-4 * sc_


def test_a_goal_guided_step_lowers_the_goal_value(eng):
    """Property: SGD steps on the goal term, normalised by the first gradient, lower the summed goal value of the decoded plans."""
    mean, cond, cs, goal, _ = guided_case(12, 2, 57)
    ge = engine_goal(goal, 2)

    def value(z):
        v = eng.goal_loss(eng.decode(z, cond, cs, descaled_output=True), ge, want_grad=False)
        return float((v.cpu().reshape(12, 2) * goal["scale"].float()[:, None]).sum())
    gd = dict(curr_states=cs, goal=ge, optimizer="sgd", lr=1.0)
    _, g = eng.guidance_step(mean, cond, gd, sigma=0.0, want_grad=True)
    gmax = float(g.abs().max())
    assert gmax > 0.0
    v0 = value(mean)
    v1 = value(eng.guidance_step(mean, cond, dict(gd, lr=0.05 / gmax), sigma=0.0))
    v4 = value(eng.guidance_step(mean, cond, dict(gd, lr=0.05 / gmax, grad_steps=4), sigma=0.0))
    print(f"   goal value of the decoded plans: {v0:.4f} -> {v1:.4f} (1 SGD step) -> {v4:.4f} (4 steps)")
    assert v0 > v1 > v4 > 0.0


def test_goal_chains_that_guide_nothing_equal_the_unguided_chain_and_errors_leave_no_term(eng):
    """A 10-step guided chain with every scale 0, and one with every agent arrived, reproduce the unguided chain bit for bit.  A call
    that raises on a malformed goal leaves no term on the handle: the plain guided call behind it gives what it gave before."""
    from cld_amd.engine import Engine
    from cld_amd._lib import CldError
    A = 16
    mean, cond, cs, goal, _ = guided_case(A, 1, 59)
    e = Engine(n_timesteps=10, device="cuda:0", precision=eng.precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True)); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
    nz = synth.make_noise(A, 10, 77)
    xT, noise = torch.from_numpy(nz["x_T"]), torch.from_numpy(nz["noise"])
    x_plain, _, _ = e.sample(xT, cond, noise=noise)
    gd = dict(curr_states=cs, lr=0.05, optimizer="sgd", grad_steps=2)
    x_zero, _, _ = e.sample(xT, cond, noise=noise, guidance=dict(gd, goal=engine_goal(dict(goal, scale=torch.zeros(A)))))
    x_done, _, _ = e.sample(xT, cond, noise=noise, guidance=dict(gd, goal=engine_goal(dict(goal, reached=torch.ones(A, dtype=torch.bool)))))
    x_goal, _, _ = e.sample(xT, cond, noise=noise, guidance=dict(gd, goal=engine_goal(goal)))
    assert torch.equal(x_zero, x_plain) and torch.equal(x_done, x_plain) and not torch.equal(x_goal, x_plain)
    tgt = torch.from_numpy(synth.uniform(59, "tgt", (A, 52), 0.0, 12.0))
    plain = dict(gd, target_speed=tgt, loss_scale=torch.full((A,), 1.0 / (A * 52)))
    before = e.guidance_step(mean, cond, plain, sigma=0.0).clone()
    with pytest.raises(CldError):
        e.guidance_step(mean, cond, dict(plain, goal=engine_goal(dict(goal, target_pos=goal["target_pos"][:-1]))), sigma=0.0)
    with pytest.raises(CldError):                                        # refused by the library, with the term already on the handle
        e.guidance_step(mean, cond, dict(plain, goal=engine_goal(goal), grad_steps=100), sigma=0.0)
    assert torch.equal(e.guidance_step(mean, cond, plain, sigma=0.0), before)
    with pytest.raises(CldError):                                        # no term is set: a guidance struct without a loss is refused as ever
        e.guidance_step(mean, cond, gd, sigma=0.0)


def _policy(n_timesteps=10):
    from cld_amd.dm_model import DmModel
    from cld_amd.engine import Engine
    from cld_amd.policy import CldPolicy
    from cld_amd.vae_model import VaeModel
    e = Engine(n_timesteps=n_timesteps, device="cuda:0")
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True)); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
    return CldPolicy(DmModel(None, None, n_timesteps=n_timesteps, engine=e), VaeModel(engine=e))


def test_get_action_with_goal_configs():
    """Upstream's guidance configuration with one goal loss per scene, three samples: the values come back under upstream's keys with
    NaN outside each config's agents, equal to the yardstick's on the returned trajectories; every agent executes the sample
    choose_action_from_guidance picks for it (per agent: the goal losses are not scene-level)."""
    pol = _policy()
    sizes, N = [4, 3], 3
    B = sum(sizes)
    inp = synth.make_inputs(B, 9)
    sc = synth.make_collision_scene(sizes, 9)
    W = torch.from_numpy(sc["world_from_agent"])
    local0, local1 = torch.tensor([[3.0, 2.5], [40.0, 30.0], [0.5, 12.0]]), torch.tensor([[12.0, 2.0], [150.0, 5.0], [5.0, 1.0]])
    world = lambda idx, loc: (torch.einsum("aij,aj->ai", W[idx, :2, :2].double(), loc.double()) + W[idx, :2, 2].double()).float()
    a0, a1 = [0, 1, 3], [4, 5, 6]
    cfg = [[{"name": "global_target_pos", "weight": 2.0, "agents": [0, 1, 3],
             "params": {"target_pos": world(a0, local0).tolist(), "urgency": [0.5, 0.9, 1.0], "pref_speed": 1.42}}],
           [{"name": "global_target_pos_at_time", "weight": 1.5, "agents": None,
             "params": {"target_pos": world(a1, local1).tolist(), "target_time": [23, 90, 1], "urgency": [0.5, 0.4, 0.5], "target_tolerance": None}}]]
    pol.set_guidance(cfg, torch.from_numpy(sc["scene_index"]), lr=0.05, optimizer="sgd", grad_steps=2)
    obs = {"cond_feat": torch.from_numpy(inp["cond_feat"]).cuda(), "curr_states": torch.from_numpy(inp["curr_states"]).cuda(), "world_from_agent": W.cuda()}
    nz = synth.make_noise(B * N, 10, 3)
    noise = {"x_T": torch.from_numpy(nz["x_T"]).reshape(B, N, 52, 4), "noise": torch.from_numpy(nz["noise"])}
    act, info = pol.get_action(obs, num_action_samples=N, noise=noise, step_index=3)
    keys = ["global_target_pos_scene_000_00", "global_target_pos_at_time_scene_001_00"]
    assert list(info["guide_losses"]) == keys and info["goal_global_t"] == 3
    traj = info["trajectories"].cpu()
    gg = pol._guidance["goal"]
    goal = Y.to64(dict({k: gg[k] for k in ("kind", "target_pos", "target_time", "urgency", "pref_speed", "scale")}, reached=None, global_t=3, dt=0.1,
                       min_progress_dist=0.5, agent_from_world=Y.invert_frames(W)))
    check_margins(traj, goal)
    ref = Y.values(traj.double(), goal)
    for key, idx in zip(keys, (a0, a1)):
        got = info["guide_losses"][key].cpu()
        inside = torch.zeros(B, dtype=torch.bool)
        inside[idx] = True
        assert bool(torch.isnan(got[~inside]).all()) and not bool(torch.isnan(got[inside]).any())
        assert float((got[inside].double() - ref[inside]).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max()))
    # upstream's selection as written: the last scene's per-agent argmin applies to the whole batch (nansum of NaN rows is 0 -> sample 0)
    expect = torch.argmin(torch.nan_to_num(info["guide_losses"][keys[1]].cpu(), nan=0.0), dim=-1)
    assert torch.equal(info["act_idx"].cpu(), expect) and torch.equal(expect[a1], torch.argmin(ref[a1], dim=-1))
    assert torch.equal(act.positions.cpu(), traj[torch.arange(B), expect][..., :2])
    # filter-only: the same machinery without guidance in the loop still reports and selects by the goal values
    act2, info2 = pol.get_action(obs, num_action_samples=N, noise=noise, step_index=3, guide_as_filter_only=True)
    assert list(info2["guide_losses"]) == keys and not torch.equal(info2["trajectories"], info["trajectories"])


def test_closed_loop_rollout_carries_the_goal_state():
    """Three sim steps, four agents, five executed steps per plan: agent 2's target lies 0.5 m from where it starts, so it has arrived
    when the second plan is made (the flag is asserted on what get_action reports); from then on its goal is off, and its poses equal
    those of a rollout that never gave it a goal; global_t advances with the sim step; set_guidance starts over.  The other agents'
    targets lie far behind them: they never arrive, and the progress term always pulls."""
    from cld_amd.policy import closed_loop_rollout, frames_from_pose
    pol = _policy()
    B = 4
    inp = synth.make_inputs(B, 13)
    cond = torch.from_numpy(inp["cond_feat"]).cuda()
    centroid = torch.tensor([[0.0, 0.0], [10.0, 0.0], [20.0, 5.0], [30.0, -5.0]])
    yaw = torch.tensor([0.0, 0.5, -0.3, 1.0])
    W0 = frames_from_pose(torch.cat([centroid, yaw[:, None]], dim=1)).double()
    local = torch.tensor([[-50.0, 10.0], [-60.0, -5.0], [0.5, 0.0], [-45.0, 8.0]], dtype=torch.float64)
    tp = (torch.einsum("aij,aj->ai", W0[:, :2, :2], local) + W0[:, :2, 2]).float()
    nz = synth.make_noise(B, 10, 5)
    noise = {"x_T": torch.from_numpy(nz["x_T"]).reshape(B, 1, 52, 4), "noise": torch.from_numpy(nz["noise"])}
    seen = []
    inner = pol.get_action

    def spy(obs, **kw):
        act, info = inner(obs, **kw)
        seen.append((kw["step_index"], info["goal_global_t"], info["goal_reached"].clone(), obs["agent_hist"].clone()))
        return act, info
    pol.get_action = spy

    def run(agents):
        idx = list(range(B)) if agents is None else agents
        cfg = [[{"name": "global_target_pos", "weight": 4.0, "agents": agents,
                 "params": {"target_pos": tp[idx].tolist(), "urgency": [1.0] * len(idx), "target_tolerance": 2.0, "action_num": 5}}]]
        pol.set_guidance(cfg, torch.zeros(B, dtype=torch.long), lr=0.05, optimizer="adam")
        seen.clear()
        return closed_loop_rollout(pol, lambda step, world, cs: cond, centroid, yaw, torch.from_numpy(inp["curr_states"]), 3, n_step_action=5, noise=noise)
    poses = run(None)
    assert [s[0] for s in seen] == [0, 1, 2] and [s[1] for s in seen] == [0, 1, 2] and pol.goal_global_t == 2       # global_t advanced
    assert seen[1][2].tolist() == [False, False, True, False] and seen[2][2].tolist() == [False, False, True, False]
    assert pol.goal_reached.tolist() == [False, False, True, False]
    assert float(seen[0][3].abs().max()) == 0.0                                 # first step: the current position repeated
    assert seen[1][3].shape == (B, 5, 2) and float(seen[1][3][:, -1].abs().max()) <= 1e-4 and float(seen[1][3][:, 0].norm(dim=-1).max()) > 0.05
    flags_with = [s[2].clone() for s in seen]
    poses_without = run([0, 1, 3])
    assert pol.goal_reached.tolist() == [False] * 4                             # set_guidance started over; agent 2 has no goal in this run
    first = next(i for i, f in enumerate(flags_with) if bool(f[2]))
    assert torch.equal(poses[first:, 2], poses_without[first:, 2])
    pol.clear_guidance()
    pol.get_action = inner                                                      # (no goal from here on: nothing for the spy to record)
    poses_free = closed_loop_rollout(pol, lambda step, world, cs: cond, centroid, yaw, torch.from_numpy(inp["curr_states"]), 3, n_step_action=5, noise=noise)
    assert not torch.equal(poses_free[:, [0, 1, 3]], poses[:, [0, 1, 3]])       # the goals did steer the others
