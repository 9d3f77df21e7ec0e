"""GPU parity of the social-group guidance (csrc/social_kernels.hip; upstream's SocialGroupLoss, guidance_loss.py:1137-1207): the
kernel against the recording made from the reference's own class (tests/golden/social_group.npz) and against the fp64 yardstick
(tests/social_yardstick.py, pinned by that recording: tests/test_social_host.py) at the sizes where the launch logic changes; the
on-device draws against their numpy replica (tests/social_replica.py); the term inside the guided sampler (cld_set_social_term) in
every formulation of the guidance kernel; the policy surface and the closed-loop rollout.

In every case, asserted on the yardstick with no row excluded: where the nearest neighbour is used the second-nearest is >= 1e-3 m
farther, no read distance is below 1e-2 m, and no u is within 1e-6 of cohesion.
"""
import numpy as np
import pytest
import torch

from cld_amd import synth
from tests import social_replica as SR
from tests import social_yardstick as Y
from tests.test_social_host import CASES, check_margins, recorded_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(precision):
    from cld_amd.engine import Engine
    e = Engine(n_timesteps=100, device="cuda:0", precision=precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True))
    e.load_state_dict(synth.make_decoder_weights(0))
    return e.finalize()


def engine_term(term, N=1, **kw):
    """The yardstick's term as Engine.social_group_loss / the guidance dict take it."""
    return dict(groups=term["groups"], leader=term["leader"], social_dist=term["social_dist"], cohesion=term["cohesion"], scale=term["scale"],
                world_from_agent=term["world_from_agent"].float(), num_samp=N, **kw)


def check_kernel(eng, plans, term, r, u, ref_v, ref_g):
    """Engine.social_group_loss on plans [A,N,52,6] with caller draws r / u [A,N,52] against reference values [A,N] / gradient
    [A,N,52,6]: the two bars of the goal recording, exact zeros for non-members and the leaders' gradient, zeros in columns 2..5,
    grad_in added, bit-identical on a second run, want_grad=False gives the same values."""
    A, N = plans.shape[:2]
    te = engine_term(term, N, draw_r=r.reshape(A * N, 52), draw_u=u.reshape(A * N, 52))
    flat = plans.reshape(A * N, 52, 6)
    loss, grad = eng.social_group_loss(flat, te)
    got_v, got_g = loss.cpu().double().reshape(A, N), grad.cpu().double().reshape(A, N, 52, 6)
    err_v, err_g = float((got_v - ref_v).abs().max()), float((got_g - ref_g).abs().max())
    bar_v = 2e-5 * max(1.0, float(ref_v.abs().max()))
    print(f"   values: max error {err_v:.2e} (bar {bar_v:.2e}, max|ref| {float(ref_v.abs().max()):.3f}); gradient: {err_g:.2e} (max|ref| {float(ref_g.abs().max()):.3e})")
    assert err_v <= bar_v
    assert float(ref_g.abs().max()) > 0 and err_g <= 1e-4 * float(ref_g.abs().max())
    member = torch.zeros(A, dtype=torch.bool)
    quiet = torch.ones(A, dtype=torch.bool)
    for grp, ld in zip(term["groups"], term["leader"]):
        member[grp] = True
        quiet[[a for a in grp if a != ld]] = False
    assert float(got_v[~member].abs().max()) == 0.0 and float(got_g[quiet].abs().max()) == 0.0 and float(got_v[member].min()) > 0.0
    assert float(got_g[..., 2:].abs().max()) == 0.0                      # only x, y receive a contribution
    gin = torch.from_numpy(synth.normal(3, "social_grad_in", (A * N, 52, 6)))
    loss2, grad2 = eng.social_group_loss(flat, te, grad_in=gin)
    assert torch.equal(loss2, loss) and float((grad2.cpu() - (grad.cpu() + gin)).abs().max()) <= 1e-6
    assert torch.equal(grad2.cpu().reshape(A, N, 52, 6)[quiet], gin.reshape(A, N, 52, 6)[quiet])
    loss3, grad3 = eng.social_group_loss(flat, te)
    assert torch.equal(loss3, loss) and torch.equal(grad3, grad)
    assert torch.equal(eng.social_group_loss(flat, te, want_grad=False), loss)
    return loss, grad


@pytest.mark.parametrize("name", CASES)
def test_social_kernel_golden(golden, eng, name):
    """The fixture's 16 rows, every case: per-row values and d total / d plans against the reference's own class through
    DiffuserGuidance.compute_guidance_loss + autograd, with its replayed draws."""
    meta, g, plans, term, r, u, idx = recorded_case(golden, name)
    check_margins(plans, term, r, u)
    ref_v = torch.from_numpy(np.nan_to_num(g[name + "_values"], nan=0.0)).double()        # outside the config's agents the kernel reports 0
    ref_g = torch.from_numpy(g[name + "_grad"]).double()
    check_kernel(eng, plans, term, r, u, ref_v, ref_g)


def constructed_case(group_sizes, N, seed, offset=(300.0, -200.0)):
    """Groups of the given sizes with non-members before, between and behind them.  A group's members stand along a line at spacings
    that grow with the index (2 m + 0.4 m per member), with staggered lateral offsets and headings of their own, `offset` away from the
    world origin; every plan creeps 0.2 m forward with a wobble of centimetres, so the neighbour order of the stance holds over the
    plan.  Cohesion 0 / 0.6 / 1 / 0.3 in turn, a member as leader in every other group.  -> (plans [A,N,52,6] float32, yardstick term,
    caller draws r int32 / u float32 [A,N,52])."""
    rng = np.random.default_rng(seed)
    groups, a = [], 0
    for gi, M in enumerate(group_sizes):
        a += 1 + gi % 2
        groups.append(list(range(a, a + M)))
        a += M
    A = a + 1
    pos = rng.uniform(-30.0, 30.0, (A, 2))
    th = rng.uniform(-0.3, 0.3, A)
    coh_cycle = (0.0, 0.6, 1.0, 0.3)
    term = dict(groups=groups, leader=[], social_dist=[], cohesion=[], scale=[])
    r, u = np.zeros((A, N, 52), np.int32), rng.uniform(0.0, 1.0, (A, N, 52)).astype(np.float32)
    for gi, grp in enumerate(groups):
        M = len(grp)
        i = np.arange(M)
        pos[grp, 0] = 2.0 * i + 0.4 * i * (i - 1) / 2
        pos[grp, 1] = 45.0 * gi + 0.1 * ((5 * i) % 7)
        term["leader"].append(grp[M // 2] if gi % 2 == 0 else -1)
        term["social_dist"].append(1.5 + 0.25 * gi)
        term["cohesion"].append(coh_cycle[gi % 4])
        term["scale"].append(0.7 * (1 + gi) / (M * N))
        r[grp] = rng.integers(0, M - 1, (M, N, 52))
    pos += np.asarray(offset)
    W = np.zeros((A, 3, 3))
    W[:, 0, 0], W[:, 0, 1], W[:, 1, 0], W[:, 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    W[:, :2, 2], W[:, 2, 2] = pos, 1.0
    term["world_from_agent"] = torch.from_numpy(W.astype(np.float32)).double()
    plans = np.zeros((A, N, 52, 6), np.float32)
    plans[..., 0] = 0.2 * (np.arange(52) + 1) / 52 + 0.02 * rng.standard_normal((A, N, 52))
    plans[..., 1] = 0.02 * rng.standard_normal((A, N, 52))
    plans[..., 2:] = rng.standard_normal((A, N, 52, 4))
    return torch.from_numpy(plans), term, torch.from_numpy(r), torch.from_numpy(u)


@pytest.mark.parametrize("sizes,N", [((2, 3, 65, 128), 1), ((2, 3, 65), 2)])
def test_social_kernel_vs_yardstick_at_the_sizes_where_the_launch_changes(eng, sizes, N):
    """Groups of 2 (one candidate, nothing to draw from), 3, 65 (more members than a wave has lanes; the launch splits the 52 steps
    into runs of 3, the last of 1, and the members into runs of 8, the last of 1) and 128 (the bound on max_members: runs of 2 steps),
    the small groups riding in a launch sized for the large ones, non-members between them, 300 m from the world origin, one and two
    samples, caller draws: 205 + 150 rows against the fp64 yardstick's values and autograd gradient.  (One run of steps and one of
    members: the group of 4 of test_get_action_with_a_social_group_config; 42 + 10 steps: the recording's group of 6.)"""
    plans, term, r, u = constructed_case(sizes, N, 31 + N)
    gap, dmin, umin = check_margins(plans, term, r, u)
    print(f"{plans.shape[0] * N} rows: neighbour margin {gap:.3e} m, smallest distance read {dmin:.3e} m, |u - cohesion| >= {umin:.3e}")
    v, g = Y.value_and_grad(plans.double(), term, r, u)
    check_kernel(eng, plans, term, r, u, v, g)


def test_a_group_beyond_max_members_gets_nan_and_passes_grad_in_through(eng):
    """The stated contract: a term that declares max_members = 64 while the device-side group_start holds a group of 65 -- that
    group's members get NaN values and the gradient of grad_in; the other groups are evaluated as ever.  Beyond the bound of 128, and
    below 2, the term is refused."""
    from cld_amd._lib import CldError
    plans, term, r, u = constructed_case((2, 64, 65), 1, 37)
    A = plans.shape[0]
    check_margins(plans, term, r, u)
    v, g = Y.value_and_grad(plans.double(), term, r, u)
    te = engine_term(term, 1, draw_r=r.reshape(A, 52), draw_u=u.reshape(A, 52), max_members=64)
    gin = torch.from_numpy(synth.normal(5, "social_grad_in", (A, 52, 6)))
    loss, grad = eng.social_group_loss(plans.reshape(A, 52, 6), te, grad_in=gin)
    big = torch.zeros(A, dtype=torch.bool)
    big[term["groups"][2]] = True
    assert bool(torch.isnan(loss.cpu()[big]).all()) and torch.equal(grad.cpu()[big], gin[big])
    assert float((loss.cpu().double()[~big] - v[~big, 0]).abs().max()) <= 2e-5 * max(1.0, float(v[~big].abs().max()))
    assert float((grad.cpu().double()[~big] - gin.double()[~big] - g[~big, 0]).abs().max()) <= 1e-4 * float(g[~big].abs().max())
    loss0 = eng.social_group_loss(plans.reshape(A, 52, 6), te, want_grad=False)
    assert torch.equal(torch.isnan(loss0), torch.isnan(loss)) and torch.equal(loss0[~big.cuda()], loss[~big.cuda()])
    for bad in (129, 1):
        with pytest.raises(CldError, match="members"):
            eng.social_group_loss(plans.reshape(A, 52, 6), dict(te, max_members=bad))
    with pytest.raises(CldError, match="two groups"):
        eng.social_group_loss(plans.reshape(A, 52, 6), dict(te, groups=[[1, 2], [2, 3]], leader=[-1, -1], scale=[1.0, 1.0], social_dist=1.5, cohesion=0.5))
    with pytest.raises(CldError, match="go together"):
        eng.social_group_loss(plans.reshape(A, 52, 6), {k: v_ for k, v_ in te.items() if k != "draw_u"})


def test_on_device_draws_equal_the_replica_bit_for_bit(eng):
    """With draw_r = draw_u = NULL the generator of cld_kernels.h draws under (seed, the term's own stream tag, evaluation index,
    row * 52 + t): the result equals the one with tests/social_replica.py's draws handed in, bit for bit; two evaluation indices (and
    two seeds) give different draws; cohesion 0 does not depend on them at all."""
    plans, term, _, _ = constructed_case((2, 3, 25), 2, 41)
    A, N = plans.shape[:2]
    flat = plans.reshape(A * N, 52, 6)
    size = SR.group_size_of_row(term["groups"], A, N)
    seen = {}
    for seed, it in ((9, 0), (9, 5), (10, 0)):
        r, u = SR.draws(seed, it, 0, size)
        rt, ut = torch.from_numpy(r).reshape(A, N, 52), torch.from_numpy(u).reshape(A, N, 52)
        check_margins(plans, term, rt, ut)
        dev = eng.social_group_loss(flat, engine_term(term, N, seed=seed, iter_base=it))
        rep = eng.social_group_loss(flat, engine_term(term, N, draw_r=r, draw_u=u))
        assert torch.equal(dev[0], rep[0]) and torch.equal(dev[1], rep[1])
        v, _ = Y.value_and_grad(plans.double(), term, rt, ut)
        assert float((dev[0].cpu().double().reshape(A, N) - v).abs().max()) <= 2e-5 * max(1.0, float(v.abs().max()))
        seen[(seed, it)] = dev
    drawn = torch.zeros(A, dtype=torch.bool)
    still = torch.zeros(A, dtype=torch.bool)
    for grp, coh in zip(term["groups"], term["cohesion"]):
        (drawn if coh > 0 and len(grp) > 2 else still)[grp] = True
    rows = lambda m: m.repeat_interleave(N).cuda()
    for other in ((9, 5), (10, 0)):
        assert not torch.equal(seen[other][0][rows(drawn)], seen[(9, 0)][0][rows(drawn)])
        assert torch.equal(seen[other][0][rows(still)], seen[(9, 0)][0][rows(still)])       # cohesion 0, and a pair's only candidate


def guided_case(group_sizes, N, seed, cohesion, n_steps=2):
    """A guided step's inputs: latent means, conditioning, current states (speeds scaled to <= 3 m/s, so that a plan stays within
    15 m), groups of the given sizes with non-members between them whose frames stand abreast at spacings that grow with the index,
    and caller draws for n_steps optimiser steps.  -> (mean, cond, cs float32 [A N,...], yardstick term, decoder weights fp64,
    draws [(r, u)] each [A N,52])."""
    from oracle import cld_oracle as O
    rng = np.random.default_rng(seed)
    groups, a = [], 0
    for gi, M in enumerate(group_sizes):
        a += gi % 2
        groups.append(list(range(a, a + M)))
        a += M
    A = a + 1
    B = A * N
    inp = synth.make_inputs(B, seed)
    cond = torch.from_numpy(inp["cond_feat"])
    cs = torch.from_numpy(inp["curr_states"]) * torch.tensor([1.0, 1.0, 0.2, 1.0])
    mean = torch.from_numpy(synth.normal(seed, "social_mean", (B, 52, 4))) * 0.7
    pos = rng.uniform(-30.0, 30.0, (A, 2))
    th = rng.uniform(-0.1, 0.1, A)
    term = dict(groups=groups, leader=[], social_dist=[], cohesion=[], scale=[])
    for gi, grp in enumerate(groups):
        M = len(grp)
        i = np.arange(M)
        pos[grp, 0] = 120.0 * gi + 0.4 * ((3 * i) % 5)
        pos[grp, 1] = 3.0 * i + 0.5 * i * (i - 1) / 2
        term["leader"].append(grp[0] if gi % 2 == 0 else -1)
        term["social_dist"].append(1.5)
        term["cohesion"].append(cohesion[gi % len(cohesion)])
        term["scale"].append(1.0 / (M * N))
    W = np.zeros((A, 3, 3))
    W[:, 0, 0], W[:, 0, 1], W[:, 1, 0], W[:, 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    W[:, :2, 2], W[:, 2, 2] = pos, 1.0
    term["world_from_agent"] = torch.from_numpy(W.astype(np.float32)).double()
    size = SR.group_size_of_row(groups, A, N)
    draws = []
    for k in range(n_steps):
        r = (rng.integers(0, 1 << 30, (B, 52)) % np.maximum(size - 1, 1)[:, None]).astype(np.int32)
        u = rng.uniform(0.0, 1.0, (B, 52)).astype(np.float32)
        draws.append((torch.from_numpy(r), torch.from_numpy(u)))
    wd64 = {k: v.double() for k, v in O.to_torch(synth.make_decoder_weights(0)).items()}
    return mean, cond, cs, term, wd64, draws


def stacked(draws):
    """[(r, u)] per optimiser step -> draw_r / draw_u [1, n_opt, B, 52]."""
    return dict(draw_r=torch.stack([r for r, _ in draws])[None], draw_u=torch.stack([u for _, u in draws])[None])


def check_guided_step(eng, group_sizes, N, seed, kernel, cohesion):
    """Two SGD steps of cld_guidance_step with the social-group term on the handle against decode -> yardstick gradient -> decoder
    backward written out over the oracle's decoder (Y.sgd_steps), the margins asserted on both iterates the loss is evaluated on."""
    mean, cond, cs, term, wd64, draws = guided_case(group_sizes, N, seed, cohesion)
    d = lambda t: t.double()
    _, g1, _ = Y.sgd_steps(wd64, d(mean), d(cond), d(cs), term, draws[:1], 0.0, N)
    lr = 0.05 / float(g1.abs().max())                                    # a step size normalised by the first gradient
    ref, gref, seen = Y.sgd_steps(wd64, d(mean), d(cond), d(cs), term, draws, lr, N)
    for plans, (r, u) in zip(seen, draws):
        check_margins(plans, term, r.reshape(-1, N, 52), u.reshape(-1, N, 52))
    gd = dict(curr_states=cs, social_group=engine_term(term, N, **stacked(draws)), optimizer="sgd", lr=lr, grad_steps=2)
    if kernel != "auto":
        eng.force_kernel("guide", kernel)
    try:
        mg, grad = eng.guidance_step(mean, cond, gd, sigma=0.0, want_grad=True)
    finally:
        eng.force_kernel("guide", "auto")
    err_m, err_g = float((mg.cpu().double() - ref).abs().max()), float((grad.cpu().double() - gref).abs().max())
    moved = float((ref - mean).abs().max())
    print(f"   [{mean.shape[0]} rows / {kernel}] guided mean: max error {err_m:.2e}, moved by {moved:.2e}; gradient: {err_g:.2e} of max {float(gref.abs().max()):.2e}")
    assert moved > 1e-3
    assert err_m <= 2e-4 * max(1.0, float(mean.abs().max()))
    assert err_g <= 1e-4 * float(gref.abs().max())


@pytest.mark.parametrize("kernel", ["valu", "mfma", "quad"])
def test_social_guided_step_vs_yardstick_in_every_guide_kernel_form(eng, kernel):
    """cld_guidance_step with the term on the handle: two SGD steps at 9 agents x 3 samples = 27 rows (groups of 5 and 2, two
    non-members), cohesion 0.5 and 0."""
    check_guided_step(eng, (5, 2), 3, 64, kernel, (0.5, 0.0))


def test_social_guided_step_on_the_forward_sweep_path_at_256_rows(eng):
    """From 256 rows run_guidance decodes the iterate with the guidance kernel's own forward sweep + the roll-out kernel: the social
    kernel runs behind that path too.  128 agents x 2 samples: two groups of 12 that pair by draw alone, 41 pairs (the nearest
    neighbour is the only candidate), 22 non-members between them."""
    check_guided_step(eng, (12, 12) + (2,) * 41, 2, 63, "auto", (1.0, 1.0, 0.5, 0.0))


def test_adam_with_three_grad_steps_reads_the_draws_of_every_optimiser_step(eng):
    """Adam, grad_steps = 3: caller draws [1, 3, B, 52] made by the replica for evaluations (iter_base, 0..2) give the bits of the
    on-device generator -- every optimiser step reads its own slab -- and draws in another order give another result."""
    mean, cond, cs, term, _, _ = guided_case((5, 3), 2, 65, (0.5, 0.7), 3)
    A, N = mean.shape[0] // 2, 2
    size = SR.group_size_of_row(term["groups"], A, N)
    draws = [tuple(torch.from_numpy(x) for x in SR.draws(21, 4, k, size)) for k in range(3)]
    gd = dict(curr_states=cs, optimizer="adam", lr=0.02, grad_steps=3)
    dev = eng.guidance_step(mean, cond, dict(gd, social_group=engine_term(term, N, seed=21, iter_base=4)), sigma=0.0)
    rep = eng.guidance_step(mean, cond, dict(gd, social_group=engine_term(term, N, **stacked(draws))), sigma=0.0)
    swapped = eng.guidance_step(mean, cond, dict(gd, social_group=engine_term(term, N, **stacked(draws[::-1]))), sigma=0.0)
    assert torch.equal(dev, rep) and not torch.equal(swapped, rep)
    assert float((dev.cpu() - mean).abs().max()) > 0.0


def combined_case():
    """The inputs of the four-term step below and its reference, all on the CPU -> (x_t, cond, z, guidance dict without the social
    term, yardstick term, draws, posterior mean, reference guided mean, sigma)."""
    from oracle import cld_oracle as O
    from tests import goal_yardstick as GY
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
    W = db["world_from_agent"].double()
    local = torch.tensor([[3.0, 2.5], [0.5, 12.0], [12.0, 2.0], [150.0, 5.0], [5.0, 1.0], [0.0, 0.0]] * 2, dtype=torch.float64)
    goal = dict(kind=torch.tensor([1, 1, 2, 2, 2, 0] * 2, dtype=torch.int32), target_time=torch.tensor([0, 0, 40, 90, 2, 0] * 2, dtype=torch.int32),
                urgency=torch.tensor([0.5, 1.0, 0.5, 0.5, 0.5, 0.5] * 2, dtype=torch.float64), pref_speed=torch.full((B,), 1.42, dtype=torch.float64),
                scale=torch.full((B,), 2.0 / 5, dtype=torch.float64), reached=torch.zeros(B, dtype=torch.bool), global_t=10, dt=0.1, min_progress_dist=0.5,
                target_pos=(torch.einsum("aij,aj->ai", W[:, :2, :2], local) + W[:, :2, 2]).float().double(),
                agent_from_world=GY.invert_frames(W).float().double())
    col = dict(db, scene_weight=[40.0, 60.0])
    term = dict(groups=[[0, 2, 3, 5], [7, 8, 10]], leader=[2, -1], social_dist=[1.5, 2.0], cohesion=[1.0, 1.0], scale=[0.05 / 4, 0.08 / 3], world_from_agent=W)
    rng = np.random.default_rng(23)
    size = SR.group_size_of_row(term["groups"], B, 1)
    draws = [(torch.from_numpy((rng.integers(0, 1 << 30, (B, 52)) % np.maximum(size - 1, 1)[:, None]).astype(np.int32)),
              torch.from_numpy(rng.uniform(0.0, 0.999, (B, 52)).astype(np.float32))) for _ in range(2)]
    step = [0]

    def extra(traj):
        r, u = draws[step[0]]
        step[0] += 1
        return (((traj[..., 2] - tgt).abs().sum(dim=1) * scale).sum() + O.scene_collision_total(traj, col, 1)
                + Y.total(traj.reshape(B, 1, 52, 6), term, r.reshape(B, 1, 52), u.reshape(B, 1, 52)))
    goal32 = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in goal.items()}
    ref, _ = GY.sgd_step(wd, mean, cond, cs, goal32, 5.0, 2, 1, extra=extra)
    wd64 = {k: v.double() for k, v in wd.items()}
    step[0] = 0
    x1, _ = GY.sgd_step(wd, mean, cond, cs, goal32, 5.0, 1, 1, extra=extra)
    with torch.no_grad():
        for x, (r, u) in zip((mean, x1), draws):
            plans = O.decode(wd64, x.double(), cond.double(), cs.double(), True).reshape(B, 1, 52, 6)
            check_margins(plans, term, r.reshape(B, 1, 52), u.reshape(B, 1, 52))
    gd = dict(curr_states=cs, target_speed=tgt, loss_scale=scale, lr=5.0, optimizer="sgd", grad_steps=2, goal=dict(goal32, num_samp=1),
              agent_collision=dict(extent=db["extent"], world_from_agent=db["world_from_agent"], curr_speed=db["curr_speed"],
                                   scene_index=db["scene_index"], weight=[40.0, 60.0]))
    return x_t, cond, z, gd, term, draws, mean, ref, sigma


def test_sampling_step_with_social_goal_collision_and_target_speed_vs_oracle(eng):
    """cld_sample_step at t = 40, two scenes of 6 agents: social groups + goal + agent_collision + target_speed in one guided step
    (two SGD steps) against the two yardsticks' totals + the oracle's collision total and target-speed loss."""
    x_t, cond, z, gd, term, draws, mean, ref, sigma = combined_case()
    without = eng.sample_step(x_t, cond, 40, z=z, guidance=gd)
    got = eng.sample_step(x_t, cond, 40, z=z, guidance=dict(gd, social_group=engine_term(term, 1, **stacked(draws))))
    sc_ = max(1.0, float(mean.abs().max()))
    mattered = float((got["mean_guided"] - without["mean_guided"]).abs().max())
    print(f"   guided mean: max error {float((got['mean_guided'].cpu() - ref).abs().max()):.2e} of scale {sc_:.2f}; the social term moved it by {mattered:.2e}")
    assert mattered > 1e-3                                               # the social term matters in this step
    assert float((got["mean_guided"].cpu() - ref).abs().max()) <= 2e-4 * sc_
    assert float((got["x_next"].cpu() - (ref + sigma * z)).abs().max()) <= 2e-4 * sc_


def test_a_chain_stepped_with_iter_base_equals_the_guided_chain_and_errors_leave_no_term(eng):
    """A 10-step guided chain in one call (cld_sample_guided, iter_base 0) equals the chain stepped through cld_sample_step with
    iter_base = the loop iteration, bit for bit -- with the generator's draws and with caller draws [10, 2, B, 52] sliced per step.
    Caller draws that do not cover the call are refused before anything runs, and no term is left on the handle."""
    from cld_amd.engine import Engine
    from cld_amd._lib import CldError
    mean, cond, cs, term, _, _ = guided_case((5, 2), 2, 67, (0.5, 0.5))
    B, N = mean.shape[0], 2
    e = Engine(n_timesteps=10, device="cuda:0", precision=eng.precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True)); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
    nz = synth.make_noise(B, 10, 77)
    xT, noise = torch.from_numpy(nz["x_T"]), torch.from_numpy(nz["noise"])
    gd = dict(curr_states=cs, lr=0.05, optimizer="sgd", grad_steps=2)
    size = SR.group_size_of_row(term["groups"], B // N, N)
    rr, uu = zip(*[zip(*[SR.draws(3, it, k, size) for k in range(2)]) for it in range(10)])
    dr, du = torch.from_numpy(np.asarray(rr)), torch.from_numpy(np.asarray(uu))              # [10, 2, B, 52]
    x_plain, _, _ = e.sample(xT, cond, noise=noise)
    x_gen, _, _ = e.sample(xT, cond, noise=noise, guidance=dict(gd, social_group=engine_term(term, N, seed=3)))
    x_draws, _, _ = e.sample(xT, cond, noise=noise, guidance=dict(gd, social_group=engine_term(term, N, draw_r=dr, draw_u=du)))
    assert torch.equal(x_gen, x_draws) and not torch.equal(x_gen, x_plain)
    for mode in ("generator", "draws"):
        x = xT
        for it in range(10):
            tm = engine_term(term, N, seed=3, iter_base=it) if mode == "generator" else engine_term(term, N, draw_r=dr[it:it + 1], draw_u=du[it:it + 1])
            x = e.sample_step(x, cond, 9 - it, z=noise[it], guidance=dict(gd, social_group=tm))["x_next"]
        assert torch.equal(x, x_gen), mode
    tgt = torch.from_numpy(synth.uniform(59, "tgt", (B, 52), 0.0, 12.0))
    plain = dict(gd, target_speed=tgt, loss_scale=torch.full((B,), 1.0 / (B * 52)))
    before = e.guidance_step(mean, cond, plain, sigma=0.0).clone()
    with pytest.raises(CldError, match="do not cover"):                  # 10 iterations asked of draws for 9
        e.sample(xT, cond, noise=noise, guidance=dict(gd, social_group=engine_term(term, N, draw_r=dr[:9], draw_u=du[:9])))
    with pytest.raises(CldError, match="do not cover"):                  # 2 optimiser steps asked of draws for 1
        e.guidance_step(mean, cond, dict(plain, social_group=engine_term(term, N, draw_r=dr[:1, :1], draw_u=du[:1, :1])), sigma=0.0)
    with pytest.raises(CldError):                                        # malformed on the host side
        e.guidance_step(mean, cond, dict(plain, social_group=engine_term(term, N, draw_r=dr[0, 0, :-1], draw_u=du[0, 0, :-1])), sigma=0.0)
    assert torch.equal(e.guidance_step(mean, cond, plain, sigma=0.0), before)
    with pytest.raises(CldError):                                        # no term is set: a guidance struct without a loss is refused as ever
        e.guidance_step(mean, cond, gd, sigma=0.0)


def test_a_social_guided_step_lowers_the_groups_value(eng):
    """Property, cohesion 0 (nothing random): SGD steps on the social term, normalised by the first gradient, lower the summed value
    of the decoded plans."""
    mean, cond, cs, term, _, _ = guided_case((5, 4, 2), 2, 69, (0.0,))
    N = 2
    te = engine_term(term, N)

    def value(z):
        return float(eng.social_group_loss(eng.decode(z, cond, cs, descaled_output=True), te, want_grad=False).sum())
    gd = dict(curr_states=cs, social_group=te, optimizer="sgd", lr=1.0)
    _, g = eng.guidance_step(mean, cond, gd, sigma=0.0, want_grad=True)
    gmax = float(g.abs().max())
    assert gmax > 0.0
    v0 = value(mean)
    v1 = value(eng.guidance_step(mean, cond, dict(gd, lr=0.05 / gmax), sigma=0.0))
    v4 = value(eng.guidance_step(mean, cond, dict(gd, lr=0.05 / gmax, grad_steps=4), sigma=0.0))
    print(f"   social value of the decoded plans: {v0:.4f} -> {v1:.4f} (1 SGD step) -> {v4:.4f} (4 steps)")
    assert v0 > v1 > v4 > 0.0


def _policy(n_timesteps=10):
    from cld_amd.dm_model import DmModel
    from cld_amd.engine import Engine
    from cld_amd.policy import CldPolicy
    from cld_amd.vae_model import VaeModel
    e = Engine(n_timesteps=n_timesteps, device="cuda:0")
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True)); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
    return CldPolicy(DmModel(None, None, n_timesteps=n_timesteps, engine=e), VaeModel(engine=e))


def test_get_action_with_a_social_group_config():
    """Upstream's guidance configuration with a social group on a subset of scene 0 and a speed limit in scene 1, three samples: the
    values come back under upstream's key with NaN outside the group, equal to the yardstick's on the returned trajectories under
    the draws of the evaluation index behind the plan's loop iterations; the choice of sample is scene-level; the next get_action
    moves the evaluation index on."""
    pol = _policy()
    sizes, N = [5, 3], 3
    B = sum(sizes)
    inp = synth.make_inputs(B, 9)
    sc = synth.make_collision_scene(sizes, 9, spacing=6.0)
    W = torch.from_numpy(sc["world_from_agent"])
    cfg = [[{"name": "social_group", "weight": 2.0, "agents": [0, 1, 3, 4], "params": {"leader_idx": 1, "social_dist": 2.0, "cohesion": 0.5}}],
           [{"name": "speed_limit", "weight": 1.0, "agents": None, "params": {"speed_limit": 6.0}}]]
    pol.set_guidance(cfg, torch.from_numpy(sc["scene_index"]), data_batch={"world_from_agent": W}, lr=0.05, optimizer="sgd", grad_steps=2, social_seed=5)
    obs = {"cond_feat": torch.from_numpy(inp["cond_feat"]).cuda(), "curr_states": torch.from_numpy(inp["curr_states"]).cuda()}
    nz = synth.make_noise(B * N, 10, 3)
    noise = {"x_T": torch.from_numpy(nz["x_T"]).reshape(B, N, 52, 4), "noise": torch.from_numpy(nz["noise"])}
    act, info = pol.get_action(obs, num_action_samples=N, noise=noise, step_index=0)
    keys = ["social_group_scene_000_00", "speed_limit_scene_001_00"]
    assert list(info["guide_losses"]) == keys and pol.social_iter == 11
    traj = info["trajectories"].cpu()
    sg = pol._guidance["social_group"]
    term = dict(groups=sg["groups"], leader=sg["leader"], social_dist=sg["social_dist"], cohesion=sg["cohesion"], scale=sg["scale"], world_from_agent=W.double())
    assert term["groups"] == [[0, 1, 3, 4]] and term["leader"] == [1]
    r, u = SR.draws(5, 10, 0, SR.group_size_of_row(term["groups"], B, N))
    rt, ut = torch.from_numpy(r).reshape(B, N, 52), torch.from_numpy(u).reshape(B, N, 52)
    check_margins(traj, term, rt, ut)
    ref = Y.values(traj.double(), term, rt, ut)
    got = info["guide_losses"][keys[0]].cpu()
    inside = torch.zeros(B, dtype=torch.bool)
    inside[term["groups"][0]] = True
    assert bool(torch.isnan(got[~inside]).all()) and not bool(torch.isnan(got[inside]).any())
    assert float((got[inside].double() - ref[inside]).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    # upstream's selection as written: the last scene's choice (per agent: a speed limit is not scene-level) applies to the whole batch
    expect = torch.argmin(torch.nan_to_num(info["guide_losses"][keys[1]].cpu(), nan=0.0), dim=-1)
    assert torch.equal(info["act_idx"].cpu(), expect)
    _, info2 = pol.get_action(obs, num_action_samples=N, noise=noise, step_index=1)
    assert pol.social_iter == 22 and not torch.equal(info2["trajectories"], info["trajectories"])       # other draws: another plan
    _, info3 = pol.get_action(obs, num_action_samples=N, noise=noise, step_index=0, guide_as_filter_only=True)
    assert list(info3["guide_losses"]) == keys


def test_closed_loop_rollout_with_a_social_group_feeds_the_guidance_metrics():
    """Three sim steps, six agents, follow_observation=True: the term's frames follow the world pose of every re-plan (the loop
    supplies world_from_agent), GuidanceMetrics scores the executed states under guide_social_group_*, and the group's poses differ
    from an unguided rollout's while the detached leader and the agent outside the group move exactly as they do without guidance."""
    from cld_amd.metrics import GuidanceMetrics
    from cld_amd.policy import closed_loop_rollout
    pol = _policy()
    B = 6
    inp = synth.make_inputs(B, 13)
    cond = torch.from_numpy(inp["cond_feat"]).cuda()
    centroid = torch.tensor([[0.0, 0.0], [4.0, 3.0], [9.0, -2.0], [13.0, 4.0], [18.0, 0.5], [60.0, 30.0]])
    yaw = torch.tensor([0.0, 0.2, -0.1, 0.3, 0.1, 1.0])
    world0 = torch.cat([centroid, yaw[:, None]], dim=1)
    nz = synth.make_noise(B, 10, 5)
    noise = {"x_T": torch.from_numpy(nz["x_T"]).reshape(B, 1, 52, 4), "noise": torch.from_numpy(nz["noise"])}
    cfg = [[{"name": "social_group", "weight": 4.0, "agents": [0, 1, 2, 3, 4], "params": {"leader_idx": 0, "social_dist": 1.5, "cohesion": 0.5}}]]
    from cld_amd.policy import frames_from_pose
    seen = []
    inner = pol.get_action

    def spy(obs, **kw):
        seen.append(torch.as_tensor(obs["world_from_agent"]).clone().cpu())
        return inner(obs, **kw)
    pol.get_action = spy
    pol.set_guidance(cfg, torch.zeros(B, dtype=torch.long), data_batch={"world_from_agent": frames_from_pose(world0)}, lr=0.05, optimizer="adam",
                     follow_observation=True)
    gm = GuidanceMetrics(pol.vae.engine, cfg, [0, B], torch.tensor([[4.5, 2.0, 1.5]]).repeat(B, 1), world0,
                         curr_speed0=torch.from_numpy(inp["curr_states"][:, 2]))
    poses = closed_loop_rollout(pol, lambda step, world, cs: cond, centroid, yaw, torch.from_numpy(inp["curr_states"]), 3, n_step_action=5,
                                noise=noise, metrics=gm)
    assert len(seen) == 3 and pol.social_iter == 33
    assert torch.equal(seen[0], frames_from_pose(world0.cuda()).cpu()) and torch.equal(seen[1], frames_from_pose(poses[0]).cpu()) and not torch.equal(seen[1], seen[0])
    ep = gm.get_episode_metrics()
    assert list(ep) == ["guide_social_group_s0g0"] and gm.steps == 15
    assert np.isfinite(float(ep["guide_social_group_s0g0"][0])) and float(ep["guide_social_group_s0g0"][0]) >= 0.0
    pol.get_action = inner
    pol.clear_guidance()
    free = closed_loop_rollout(pol, lambda step, world, cs: cond, centroid, yaw, torch.from_numpy(inp["curr_states"]), 3, n_step_action=5, noise=noise)
    assert not torch.equal(free[:, 1:5], poses[:, 1:5])                  # the group's followers were steered
    assert torch.equal(free[:, 0], poses[:, 0]) and torch.equal(free[:, 5], poses[:, 5])      # the detached leader and the outsider were not
