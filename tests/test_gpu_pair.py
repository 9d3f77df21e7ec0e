"""GPU parity of the pair-relation guidance (csrc/pair_kernels.hip; upstream's KeepDistanceLoss, CollisionLoss, KeepDistanceLoss2 /
StayAwayLoss, FrontCollisionLoss, CollideLeftSideLoss, guidance_loss.py:1631-1791, 1844-1956, 2014-2082): the kernel against the
recording made from the reference's own classes (tests/golden/pair_guidance.npz) and against the fp64 yardstick
(tests/pair_yardstick.py, pinned by that recording: tests/test_pair_host.py) on a constructed multi-scene batch; the term inside the
guided sampler (cld_set_pair_term) in every formulation of the guidance kernel; the policy surface and the closed-loop rollout.

In every case, asserted on the yardstick with no row excluded: no distance read below 1e-2 m, and no |d - bound|, |Dx| or |Dy|
within 1e-3 of its kink.
"""
import numpy as np
import pytest
import torch

from cld_amd import synth
from tests import pair_yardstick as Y
from tests.test_pair_host import CASES, check_margins, recorded_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(precision):
    from cld_amd.engine import Engine
    e = Engine(n_timesteps=100, device="cuda:0", precision=precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True))
    e.load_state_dict(synth.make_decoder_weights(0))
    return e.finalize()


def engine_term(term, N=1, **kw):
    """The yardstick's term as Engine.pair_loss / the guidance dict take it."""
    F = term.get("agent_from_world")
    return dict(target=term["target"], ref=term["ref"], kind=term["kind"], lo=term["lo"], hi=term["hi"], decay=term["decay"], scale=term["scale"],
                world_from_agent=term["world_from_agent"].float(), agent_from_world=None if F is None else F.float(), num_samp=N, **kw)


def check_kernel(eng, plans, term, ref_v, ref_g):
    """Engine.pair_loss on plans [A,N,52,6] against reference values [P,N] / gradient [A,N,52,6]: the two bars of the social tests,
    exact zeros outside the pairs and in columns 2..5, grad_in passed through bit for bit on rows in no pair, bit-identical on a
    second run, want_grad=False gives the same values."""
    A, N = plans.shape[:2]
    te = engine_term(term, N)
    flat = plans.reshape(A * N, 52, 6)
    value, grad = eng.pair_loss(flat, te)
    got_v, got_g = value.cpu().double(), grad.cpu().double().reshape(A, N, 52, 6)
    assert got_v.shape == ref_v.shape
    err_v, err_g = float((got_v - ref_v).abs().max()), float((got_g - ref_g).abs().max())
    bar_v = 2e-5 * max(1.0, float(ref_v.abs().max()))
    print(f"   values: max error {err_v:.2e} (bar {bar_v:.2e}, max|ref| {float(ref_v.abs().max()):.3f}); gradient: {err_g:.2e} (max|ref| {float(ref_g.abs().max()):.3e})")
    assert err_v <= bar_v
    assert float(ref_g.abs().max()) > 0 and err_g <= 1e-4 * float(ref_g.abs().max())
    quiet = torch.ones(A, dtype=torch.bool)
    quiet[term["target"] + term["ref"]] = False
    if bool(quiet.any()):
        assert float(got_g[quiet].abs().max()) == 0.0
    assert float(got_g[..., 2:].abs().max()) == 0.0                      # only x, y receive a contribution
    gin = torch.from_numpy(synth.normal(3, "pair_grad_in", (A * N, 52, 6)))
    value2, grad2 = eng.pair_loss(flat, te, grad_in=gin)
    assert torch.equal(value2, value) and float((grad2.cpu() - (grad.cpu() + gin)).abs().max()) <= 1e-6
    assert torch.equal(grad2.cpu().reshape(A, N, 52, 6)[quiet], gin.reshape(A, N, 52, 6)[quiet])
    assert torch.equal(grad2.cpu()[..., 2:], gin[..., 2:])
    value3, grad3 = eng.pair_loss(flat, te)
    assert torch.equal(value3, value) and torch.equal(grad3, grad)
    assert torch.equal(eng.pair_loss(flat, te, want_grad=False), value)
    return value, grad


@pytest.mark.parametrize("name", CASES)
def test_pair_kernel_golden(golden, eng, name):
    """The fixture's 12 rows, every case: per-pair values and d total / d plans against the reference's own classes (through
    DiffuserGuidance.compute_guidance_loss where the name is registered) + autograd; `two` has an agent in two pairs."""
    meta, g, plans, term = recorded_case(golden, name)
    check_margins(plans, term)
    ref_v = torch.stack([torch.from_numpy(g[f"{name}_values_{k}"][0]) for k in range(len(term["target"]))]).double()
    ref_g = torch.from_numpy(g[name + "_grad"]).double()
    check_kernel(eng, plans, term, ref_v, ref_g)
    te = engine_term(term, meta["N"])
    if name != "collision":                                               # agent_from_world = NULL: the inverse rotation of world_from_agent
        v0 = eng.pair_loss(plans.reshape(-1, 52, 6), dict(te, agent_from_world=None), want_grad=False)
        assert float((v0.cpu().double() - ref_v).abs().max()) <= 2e-5 * max(1.0, float(ref_v.abs().max()))


P_CONSTRUCTED = 302


def constructed_case(N, seed, offset=(300.0, -200.0), P=P_CONSTRUCTED):
    """40 agents in three scenes (15, 12, 13) standing on a jittered 6-m grid `offset` away from the world origin, plans that drive
    forward at 0..5 m/s with a wobble of centimetres, and P pairs inside the scenes over all five relations: the first agent of
    every scene sits in no pair, agent 1 in exactly one (as target), agent 2 in exactly nine (five as target, four as ref), the others
    share the remaining P - 10 drawn at random (so some (target, ref) repeat under another relation).  The distance bounds of a pair
    are the 30 % / 70 % quantiles of the distances its plans read, moved on in steps of 13.7 mm until no distance is within 1e-3 m of
    a bound; the frame relations keep a drawn pair only if its |Dx|, |Dy| stay 1e-3 away from 0.  decay 0.9 on the stay_away pairs.
    -> (plans [A,N,52,6] float32, yardstick term)."""
    rng, sizes, starts, Wd, plans = constructed_scene(N, seed, offset)
    A = sum(sizes)
    special = {int(starts[0]), 1, 2, int(starts[1]), int(starts[2])}
    scene_of = np.repeat(np.arange(3), sizes)
    busy = [[a for a in range(starts[s], starts[s + 1]) if a not in special] for s in range(3)]
    cand = [(1, 5)] + [(2, 3 + k) for k in range(5)] + [(7 + k, 2) for k in range(4)]
    while len(cand) < 4 * P:
        s = int(rng.integers(0, 3))
        i, j = rng.choice(busy[s], 2, replace=False)
        cand.append((int(i), int(j)))
    term = dict(target=[], ref=[], kind=[], lo=[], hi=[], decay=[], scale=[], world_from_agent=Wd, agent_from_world=None)
    for c, (i, j) in enumerate(cand):
        if len(term["target"]) == P:
            break
        forced = c < 10
        kind = Y.KINDS[c % 5] if not forced else Y.KINDS[(0, 1, 2, 0, 1, 2)[c % 6]]       # (the forced pairs take distance relations: always kept)
        bounds = settle_bounds(plans, Wd, i, j, kind)
        if bounds is None:
            continue
        for k, v in (("target", i), ("ref", j), ("kind", kind), ("lo", bounds[0]), ("hi", bounds[1]), ("decay", 0.9 if kind == "stay_away" else 0.0),
                     ("scale", 0.3 * (1 + len(term["target"]) % 7) / N)):
            term[k].append(v)
    assert len(term["target"]) == P and all(scene_of[i] == scene_of[j] for i, j in zip(term["target"], term["ref"]))
    count = np.bincount(term["target"] + term["ref"], minlength=A)
    assert count[0] == 0 and count[starts[1]] == 0 and count[1] == 1 and count[2] == 9 and term["target"].count(2) == 5 and term["ref"].count(2) == 4
    return plans, term


def settle_bounds(plans, Wd, i, j, kind):
    """(lo, hi) of pair (i, j) under `kind` on these plans, or None when the pair cannot keep the margins: the distance relations take
    the 30 % / 70 % quantiles of the distances the plans read, moved on in steps of 13.7 mm until no distance is within 1.1e-3 m of a
    bound; the frame relations have no bounds and keep the pair only if |Dx|, |Dy| stay 1e-3 away from 0."""
    base = dict(world_from_agent=Wd, agent_from_world=None, decay=[0.0], scale=[1.0], target=[i], ref=[j], lo=[0.0], hi=[0.0])
    if kind in ("front_collision", "collide_left"):
        return (0.0, 0.0) if Y.margins(plans.double(), dict(base, kind=[kind]))[1] >= 1e-3 else None
    d = Y._pair(plans.double(), dict(base, kind=["collision"]), 0)[2].reshape(-1)
    lo, hi = float(torch.quantile(d, 0.3)), float(torch.quantile(d, 0.7))
    while float(torch.minimum((d - lo).abs(), (d - hi).abs()).min()) < 1.1e-3:
        lo, hi = lo + 0.0137, hi + 0.0137
    return (lo, 0.0) if kind == "collision" else (lo, hi)


def constructed_scene(N, seed, offset=(300.0, -200.0)):
    """The 40 agents of constructed_case -> (the generator behind it, scene sizes, scene starts, world_from_agent [A,3,3] float64 of
    float32 values, plans [A,N,52,6] float32)."""
    rng = np.random.default_rng(seed)
    sizes = (15, 12, 13)
    A = sum(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    pos = np.zeros((A, 2))
    for s, n in enumerate(sizes):
        k = np.arange(n)
        pos[starts[s]:starts[s + 1]] = np.stack([6.0 * (k % 4), 70.0 * s + 6.0 * (k // 4)], axis=1)
    pos += rng.uniform(-1.0, 1.0, (A, 2)) + np.asarray(offset)
    th = rng.uniform(-0.5, 0.5, A)
    W = np.zeros((A, 3, 3))
    W[:, 0, 0], W[:, 0, 1], W[:, 1, 0], W[:, 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    W[:, :2, 2], W[:, 2, 2] = pos, 1.0
    Wd = torch.from_numpy(W.astype(np.float32)).double()
    plans = np.zeros((A, N, 52, 6), np.float32)
    speed = rng.uniform(0.0, 5.0, (A, N, 1))
    plans[..., 0] = speed * 0.1 * (np.arange(52) + 1) + 0.02 * rng.standard_normal((A, N, 52))
    plans[..., 1] = 0.02 * rng.standard_normal((A, N, 52))
    plans[..., 2:] = rng.standard_normal((A, N, 52, 4))
    return rng, sizes, starts, Wd, torch.from_numpy(plans)


@pytest.mark.parametrize("N", [1, 2])
def test_pair_kernel_vs_yardstick_on_a_multi_scene_batch(eng, N):
    """302 pairs over 40 agents in three scenes, 300 m from the world origin, one and two samples, all five relations, against the
    fp64 yardstick's values and autograd gradient.  The launch (pair_kernels.hip): kThreads = 256, so a workgroup of the gradient role
    covers 256 (involved agent, sample, step) items -- 37 x 52 N items are 7.5 (N = 1) / 15.03 (N = 2) workgroups, the last one partly
    empty -- and one of the value role kWaves = 4 (pair, sample) waves: 302 N pairs are 75.5 / 151 workgroups.  An agent in 0, 1
    and 9 pairs (both roles), the busiest in more than twenty."""
    plans, term = constructed_case(N, 31 + N)
    dmin, kink = check_margins(plans, term)
    print(f"{plans.shape[0] * N} rows, {len(term['target'])} pairs: smallest distance read {dmin:.3e} m, kink margin {kink:.3e}")
    v, g = Y.value_and_grad(plans.double(), term)
    assert float(v.min()) >= 0.0 and float((v > 0).double().mean()) > 0.5
    check_kernel(eng, plans, term, v, g)


@pytest.mark.parametrize("N", [1, 2])
def test_a_single_pair_in_a_later_scene_of_the_multi_scene_batch(eng, N):
    """P = 1 on the 40-agent, three-scene batch 300 m from the world origin, the pair in the LAST scene (batch indices 27..39, so
    scene-local and batch indices differ), one and two samples, each of the five relations in turn as a term of one pair: two
    involved agents -- 104 N gradient items in one partly filled workgroup of 256 -- and one value workgroup with 4 - N idle waves;
    the 38 other agents' rows keep grad_in bit for bit.  Margins checked when the case is built."""
    _, sizes, starts, Wd, plans = constructed_scene(N, 41 + N)
    last = list(range(int(starts[2]), int(starts[3])))
    for kind in Y.KINDS:
        i, j, bounds = next((i, j, b) for i in last[3:] for j in last[:3] for b in [settle_bounds(plans, Wd, i, j, kind)] if b is not None)
        term = dict(target=[i], ref=[j], kind=[kind], lo=[bounds[0]], hi=[bounds[1]], decay=[0.9 if kind == "stay_away" else 0.0], scale=[0.7 / N],
                    world_from_agent=Wd, agent_from_world=None)
        dmin, kink = check_margins(plans, term)
        v, g = Y.value_and_grad(plans.double(), term)
        print(f"{kind}: pair ({i}, {j}), value {v.reshape(-1).tolist()}, smallest distance read {dmin:.3e} m, kink margin {kink:.3e}")
        assert float(v.min()) > 0.0
        check_kernel(eng, plans, term, v, g)


def test_decayed_relations_are_normalised_and_averaged_by_the_kernel(eng):
    """Upstream's quirk on the kernel itself: two agents 10 m apart at every step, band 1..4 m, so every step's term is 6.  Undecayed
    the value is 6; with decay 0.9 the weights decay^t / sum_t decay^t sum to 1 and the mean over 52 steps follows: 6 / 52.  The
    gradient's x column of the target sums to scale (undecayed: 1 / 52 at every step) and to scale / 52 (decayed: falling with t)."""
    plans = torch.zeros(2, 52, 6)
    W = torch.eye(3).repeat(2, 1, 1)
    W[1, 0, 2] = 10.0
    base = dict(target=[0], ref=[1], lo=1.0, hi=4.0, scale=[1.0], world_from_agent=W)
    v0, g0 = eng.pair_loss(plans, dict(base, kind="keep_distance", decay=0.0))
    v1, g1 = eng.pair_loss(plans, dict(base, kind="stay_away", decay=0.9))
    assert abs(float(v0) - 6.0) <= 2e-5 * 6.0 and abs(float(v1) - 6.0 / 52) <= 2e-5
    g0, g1 = g0.cpu().double(), g1.cpu().double()
    w = torch.tensor([0.9 ** t for t in range(52)], dtype=torch.float64)
    assert float((g0[0, :, 0] + 1.0 / 52).abs().max()) <= 1e-4 / 52 and float((g1[0, :, 0] + w / w.sum() / 52).abs().max()) <= 1e-4 * float(w[0] / w.sum() / 52)
    assert torch.equal(g0[1], -g0[0]) and torch.equal(g1[1], -g1[0]) and float(g0[..., 1:].abs().max()) == 0.0 and float(g1[..., 1:].abs().max()) == 0.0


def test_a_pair_outside_the_batch_gets_nan_and_contributes_nothing(eng):
    """The stated contract: device-side pairs whose target or ref lies outside [0, A) (on either side), or with target == ref, get a
    NaN value and no gradient; every other pair's value and the whole gradient keep their bits.  The Engine refuses such a term
    unless told not to look (validate=False)."""
    from cld_amd._lib import CldError
    plans, term = constructed_case(2, 37, P=24)
    A, N = plans.shape[:2]
    flat = plans.reshape(A * N, 52, 6)
    gin = torch.from_numpy(synth.normal(5, "pair_grad_in", (A * N, 52, 6)))
    value, grad = eng.pair_loss(flat, engine_term(term, N), grad_in=gin)
    bad = dict(term)
    extra = [(3, A + 3), (-1, 4), (5, 5), (A, A + 1), (4, 2 ** 31 - 1)]
    for k in ("kind", "lo", "hi", "decay", "scale"):
        bad[k] = term[k] + [term[k][c % 5] for c in range(len(extra))]
    bad["target"], bad["ref"] = term["target"] + [i for i, _ in extra], term["ref"] + [j for _, j in extra]
    with pytest.raises(CldError, match="two different agents"):
        eng.pair_loss(flat, engine_term(bad, N))
    value_b, grad_b = eng.pair_loss(flat, engine_term(bad, N, validate=False), grad_in=gin)
    P = len(term["target"])
    assert bool(torch.isnan(value_b[P:]).all()) and torch.equal(value_b[:P], value) and torch.equal(grad_b, grad)
    assert torch.equal(eng.pair_loss(flat, engine_term(bad, N, validate=False), want_grad=False)[:P], value)
    for broken in (dict(kind="nearby"), dict(kind=7), dict(lo=[1.0]), dict(target=term["target"][:-1])):
        with pytest.raises(CldError):
            eng.pair_loss(flat, dict(engine_term(term, N), **broken))
    with pytest.raises(CldError, match="num_samp"):
        eng.pair_loss(flat, engine_term(term, 3))


def guided_case(A, N, seed, n_pairs, kinds=Y.KINDS):
    """A guided step's inputs: latent means, conditioning, current states (speeds scaled to <= 3 m/s, so that a plan stays within
    15 m), frames 25 m apart along x and 3 m along y with headings of their own, and n_pairs pairs (target, ref) of agents 2..A-1 drawn
    at random -- agents 0 and 1 sit in none -- over `kinds`, with bounds that keep every clip firmly on one side: a band above the
    distance (min = 200 m + 50 m per agent), a band below it (max = 2 m), a collision radius of 0.5 m.
    -> (mean, cond, cs float32 [A N,...], yardstick term, decoder weights fp64)."""
    from oracle import cld_oracle as O
    rng = np.random.default_rng(seed)
    B = A * N
    inp = synth.make_inputs(B, seed)
    cond = torch.from_numpy(inp["cond_feat"])
    cs = torch.from_numpy(inp["curr_states"]) * torch.tensor([1.0, 1.0, 0.2, 1.0])
    mean = torch.from_numpy(synth.normal(seed, "pair_mean", (B, 52, 4))) * 0.7
    i = np.arange(A)
    pos = np.stack([25.0 * i, 3.0 * i + 0.4 * ((3 * i) % 5)], axis=1)
    th = rng.uniform(-0.1, 0.1, A)
    W = np.zeros((A, 3, 3))
    W[:, 0, 0], W[:, 0, 1], W[:, 1, 0], W[:, 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    W[:, :2, 2], W[:, 2, 2] = pos, 1.0
    term = dict(target=[], ref=[], kind=[], lo=[], hi=[], decay=[], scale=[], world_from_agent=torch.from_numpy(W.astype(np.float32)).double(),
                agent_from_world=None)
    for p in range(n_pairs):
        a, b = rng.choice(np.arange(2, A), 2, replace=False)
        kind = kinds[p % len(kinds)]
        above = p % 2 == 0
        lo, hi = ((200.0 + 50.0 * A, 400.0 + 50.0 * A) if above else (0.5, 2.0)) if kind in ("keep_distance", "stay_away") else (0.5, 0.0)
        for k, v in (("target", int(a)), ("ref", int(b)), ("kind", kind), ("lo", lo), ("hi", hi), ("decay", 0.9 if kind == "stay_away" else 0.0),
                     ("scale", (52.0 if kind == "stay_away" else 1.0) / N)):
            term[k].append(v)
    wd64 = {k: v.double() for k, v in O.to_torch(synth.make_decoder_weights(0)).items()}
    return mean, cond, cs, term, wd64


def check_guided_step(eng, A, N, seed, kernel, n_pairs):
    """Two SGD steps of cld_guidance_step with the pair term on the handle against decode -> yardstick gradient -> decoder backward
    written out over the oracle's decoder (Y.sgd_steps), the margins asserted on both iterates the loss is evaluated on; the first
    step's gradient also against the yardstick's gradient taken through Engine.decode_vjp."""
    mean, cond, cs, term, wd64 = guided_case(A, N, seed, n_pairs)
    d = lambda t: t.double()
    _, g1, _ = Y.sgd_steps(wd64, d(mean), d(cond), d(cs), term, 1, 0.0, N)
    lr = 0.05 / float(g1.abs().max())                                    # a step size normalised by the first gradient
    ref, gref, seen = Y.sgd_steps(wd64, d(mean), d(cond), d(cs), term, 2, lr, N)
    for plans in seen:
        check_margins(plans, term)
    gd = dict(curr_states=cs, pair=engine_term(term, N), optimizer="sgd", lr=lr, grad_steps=2)
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
    # the same gradient assembled from the pieces: yardstick gradient w.r.t. the decoded plans, pulled back by the library's own VJP
    _, gp = Y.value_and_grad(seen[0], term)
    via = eng.decode_vjp(mean, cond, cs, gp.reshape(-1, 52, 6).float())
    assert float((grad.cpu().double() - via.cpu().double()).abs().max()) <= 1e-4 * float(gref.abs().max())
    untouched = torch.zeros(A, dtype=torch.bool)
    untouched[:2] = True
    rows = untouched.repeat_interleave(N)
    assert torch.equal(mg.cpu()[rows], mean[rows]) and float(grad.cpu()[rows].abs().max()) == 0.0      # agents in no pair do not move


@pytest.mark.parametrize("kernel", ["valu", "mfma", "quad"])
def test_pair_guided_step_vs_yardstick_in_every_guide_kernel_form(eng, kernel):
    """cld_guidance_step with the term on the handle: two SGD steps at 9 agents x 3 samples = 27 rows, 10 pairs over the five
    relations, agents in several pairs and two in none."""
    check_guided_step(eng, 9, 3, 64, kernel, 10)


def test_pair_guided_step_on_the_forward_sweep_path_at_256_rows(eng):
    """From 256 rows run_guidance decodes the iterate with the guidance kernel's own forward sweep + the roll-out kernel: the pair
    kernel runs behind that path too.  128 agents x 2 samples, 60 pairs, frames up to 3.2 km from the world origin."""
    check_guided_step(eng, 128, 2, 63, "auto", 60)


def adam_budget(grads, lr, tols):
    """How far step k = len(grads) of torch's Adam (betas 0.9 / 0.999, eps 1e-8, bias-corrected) can differ, per element, between two
    evaluations whose gradients g_1 .. g_k agree to +- tols[i] (the state starts at zero, all k steps belong to one call).
    The step is f = -lr M / (S + eps) with M = sum_i a_i g_i, S = sqrt(sum_i b_i g_i^2), a_i = 0.1 0.9^(k-i) / (1 - 0.9^k),
    b_i = 0.001 0.999^(k-i) / (1 - 0.999^k).  By Cauchy-Schwarz |M| <= c S with c = sqrt(sum_i a_i^2 / b_i) (1 for k = 1, 1.0014 for
    k = 2), so |f| <= c lr and two evaluations differ by at most 2 c lr; and |df / dg_i| <= lr (a_i + c sqrt(b_i)) / S (the second
    term from b_i |g_i| <= sqrt(b_i) S), so along the segment between the two evaluations, on which S >= S_min =
    sqrt(sum_i b_i max(|g_i| - tol_i, 0)^2), they differ by at most lr sum_i tol_i (a_i + c sqrt(b_i)) / S_min.  The smaller of the two
    bounds: ~0 wherever the gradients are well above their tolerance, 2 c lr where a sign may flip.  No element is exempt."""
    k = len(grads)
    a = [0.1 * 0.9 ** (k - i) / (1.0 - 0.9 ** k) for i in range(1, k + 1)]
    b = [0.001 * 0.999 ** (k - i) / (1.0 - 0.999 ** k) for i in range(1, k + 1)]
    c = float(np.sqrt(sum(ai * ai / bi for ai, bi in zip(a, b))))
    s_min = sum(bi * (g.abs() - t).clamp(min=0) ** 2 for bi, g, t in zip(b, grads, tols)).sqrt()
    lin = lr * sum(t * (ai + c * np.sqrt(bi)) for ai, bi, t in zip(a, b, tols)) / s_min          # (inf where S_min = 0)
    return torch.minimum(lin, torch.full_like(lin, 2.0 * c * lr))


def test_adam_with_three_grad_steps_evaluates_the_term_on_every_iterate(eng):
    """Adam, grad_steps = 3, against the yardstick through Engine.decode / Engine.decode_vjp, every element of every step held to the
    bar of the guided-step tests, 2e-4 max(1, max|mean|), plus adam_budget at the gradient bar (1e-4 max|g| of the step).
    Adam's step is close to -lr sign(g) and the smallest |g| of these rows is 1e-7 of the largest, so an element may legitimately
    step either way, and at the end of a chain such a flip has changed every later gradient of its sample.  As tests/guided_checks.py
    does, every step is therefore checked on IDENTICAL inputs: the library's own iterate after k - 1 steps is what the call with
    grad_steps = k - 1 returns (the kernels are deterministic, and Adam's state after k - 1 steps does not depend on how many follow),
    the reference gradient of step k is taken THERE -- decode, the yardstick's fp64 gradient w.r.t. the plans, the library's VJP --
    and the reference step k is torch's Adam formula on the reference gradients of steps 1 .. k.  The result of the call with
    grad_steps = k must lie within bar + adam_budget of it: k = 1, 2 and 3, the last being the three-step result itself.  A step
    evaluated on a stale iterate, or an Adam state that is not carried, moves the well-conditioned elements out of that bound.
    Also: rows in no pair do not move, the same bits on a second call, three steps go further than two can (2.003 lr, adam_budget's
    c), and the weighted total falls from step to step."""
    A, N, lr = 9, 3, 0.02
    mean, cond, cs, term, _ = guided_case(A, N, 66, 10)
    te = engine_term(term, N)
    involved = torch.zeros(A, dtype=torch.bool)
    involved[term["target"] + term["ref"]] = True
    rows = involved.repeat_interleave(N)
    sc = torch.tensor(term["scale"], dtype=torch.float64)
    gd = dict(curr_states=cs, pair=te, optimizer="adam", lr=lr)
    iterates = [mean] + [eng.guidance_step(mean, cond, dict(gd, grad_steps=k), sigma=0.0) for k in (1, 2, 3)]
    assert torch.equal(eng.guidance_step(mean, cond, dict(gd, grad_steps=3), sigma=0.0), iterates[3])
    bar = 2e-4 * max(1.0, float(mean.abs().max()))
    grads, tols = [], []
    m = v = 0.0
    for k in (1, 2, 3):
        x_prev = iterates[k - 1]
        plans = eng.decode(x_prev, cond, cs, descaled_output=True).cpu().reshape(A, N, 52, 6)
        check_margins(plans, term)
        _, gp = Y.value_and_grad(plans.double(), term)
        g = eng.decode_vjp(x_prev, cond, cs, gp.reshape(-1, 52, 6).float()).cpu().double()
        grads.append(g)
        tols.append(1e-4 * float(g.abs().max()))
        m, v = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
        ref = x_prev.cpu().double() - (lr / (1.0 - 0.9 ** k)) * m / (v.sqrt() / np.sqrt(1.0 - 0.999 ** k) + 1e-8)
        budget = adam_budget(grads, lr, tols)
        err = (iterates[k].cpu().double() - ref).abs()
        print(f"   Adam step {k}: max error {float(err.max()):.2e} (bar {bar:.2e}), worst excess over bar + budget {float((err - bar - budget).max()):.2e}; "
              f"budget above the bar on {float((budget[rows] > bar).double().mean()):.3f} of the involved rows' elements, at 2 c lr on "
              f"{float((budget[rows] >= 2.0 * lr).double().mean()):.4f}")
        assert bool((err <= bar + budget).all()), k
    one, got = iterates[1].cpu().double(), iterates[3].cpu().double()
    assert torch.equal(got[~rows], mean.double()[~rows]) and torch.equal(one[~rows], mean.double()[~rows])
    assert float((one - mean).abs().max()) <= lr * 1.001 and float((got - mean).abs().max()) > 2.01 * lr

    def value(z):
        return float((eng.pair_loss(eng.decode(z.float(), cond, cs, descaled_output=True), te, want_grad=False).cpu().double() * sc[:, None]).sum())
    v0, v1, v3 = value(mean), value(one), value(got)
    print(f"   pair total of the decoded plans: {v0:.5f} -> {v1:.5f} (1 Adam step) -> {v3:.5f} (3 steps)")
    assert v0 > v1 > v3 > 0.0


def combined_case():
    """The inputs of the five-term step below and its reference, all on the CPU -> (x_t, cond, z, guidance dict without the pair
    term, social yardstick term, social draws, pair yardstick term, posterior mean, reference guided mean, sigma)."""
    from oracle import cld_oracle as O
    from tests import goal_yardstick as GY
    from tests import social_replica as SR
    from tests import social_yardstick as SY
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
    social = dict(groups=[[0, 2, 3, 5], [7, 8, 10]], leader=[2, -1], social_dist=[1.5, 2.0], cohesion=[1.0, 1.0], scale=[0.05 / 4, 0.08 / 3], world_from_agent=W)
    # agent 5 is the ref of a pair and a member of a social group; agent 9 the target of two pairs
    pair = dict(target=[1, 9, 9], ref=[5, 6, 11], kind=["keep_distance", "front_collision", "stay_away"], lo=[60.0, 0.0, 80.0], hi=[90.0, 0.0, 95.0],
                decay=[0.0, 0.0, 0.9], scale=[0.3, 0.2, 12.0], world_from_agent=W, agent_from_world=Y.invert_frames(W).float().double())
    rng = np.random.default_rng(23)
    size = SR.group_size_of_row(social["groups"], B, 1)
    draws = [(torch.from_numpy((rng.integers(0, 1 << 30, (B, 52)) % np.maximum(size - 1, 1)[:, None]).astype(np.int32)),
              torch.from_numpy(rng.uniform(0.0, 0.999, (B, 52)).astype(np.float32))) for _ in range(2)]
    step = [0]

    def extra(traj):
        r, u = draws[step[0]]
        step[0] += 1
        return (((traj[..., 2] - tgt).abs().sum(dim=1) * scale).sum() + O.scene_collision_total(traj, col, 1)
                + SY.total(traj.reshape(B, 1, 52, 6), social, r.reshape(B, 1, 52), u.reshape(B, 1, 52)) + Y.total(traj.reshape(B, 1, 52, 6), pair))
    goal32 = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in goal.items()}
    ref, _ = GY.sgd_step(wd, mean, cond, cs, goal32, 5.0, 2, 1, extra=extra)
    wd64 = {k: v.double() for k, v in wd.items()}
    step[0] = 0
    x1, _ = GY.sgd_step(wd, mean, cond, cs, goal32, 5.0, 1, 1, extra=extra)
    with torch.no_grad():
        for x, (r, u) in zip((mean, x1), draws):
            plans = O.decode(wd64, x.double(), cond.double(), cs.double(), True).reshape(B, 1, 52, 6)
            check_margins(plans, pair)
            gap, dmin, umin = SY.margins(plans, social, r.reshape(B, 1, 52), u.reshape(B, 1, 52))
            assert gap >= 1e-3 and dmin >= 1e-2 and umin >= 1e-6
    gd = dict(curr_states=cs, target_speed=tgt, loss_scale=scale, lr=5.0, optimizer="sgd", grad_steps=2, goal=dict(goal32, num_samp=1),
              agent_collision=dict(extent=db["extent"], world_from_agent=db["world_from_agent"], curr_speed=db["curr_speed"],
                                   scene_index=db["scene_index"], weight=[40.0, 60.0]))
    return x_t, cond, z, gd, social, draws, pair, mean, ref, sigma


def test_sampling_step_with_pair_social_goal_collision_and_target_speed_vs_oracle(eng):
    """cld_sample_step at t = 40, two scenes of 6 agents: pair relations + social groups + goal + agent_collision + target_speed in one
    guided step (two SGD steps) against the three yardsticks' totals + the oracle's collision total and target-speed loss."""
    from tests.test_gpu_social import engine_term as social_term, stacked
    x_t, cond, z, gd, social, draws, pair, mean, ref, sigma = combined_case()
    gd = dict(gd, social_group=social_term(social, 1, **stacked(draws)))
    without = eng.sample_step(x_t, cond, 40, z=z, guidance=gd)
    got = eng.sample_step(x_t, cond, 40, z=z, guidance=dict(gd, pair=engine_term(pair, 1)))
    sc_ = max(1.0, float(mean.abs().max()))
    mattered = float((got["mean_guided"] - without["mean_guided"]).abs().max())
    print(f"   guided mean: max error {float((got['mean_guided'].cpu() - ref).abs().max()):.2e} of scale {sc_:.2f}; the pair term moved it by {mattered:.2e}")
    assert mattered > 1e-3                                               # the pair term matters in this step
    assert float((got["mean_guided"].cpu() - ref).abs().max()) <= 2e-4 * sc_
    assert float((got["x_next"].cpu() - (ref + sigma * z)).abs().max()) <= 2e-4 * sc_
    # no term outlives the call that set it: the step without the pair entry gives what it gave before
    again = eng.sample_step(x_t, cond, 40, z=z, guidance=gd)
    assert torch.equal(again["mean_guided"], without["mean_guided"])


def test_a_pair_guided_step_lowers_the_pairs_value(eng):
    """Property: SGD steps on the pair term, normalised by the first gradient, lower the weighted total of the decoded plans."""
    mean, cond, cs, term, _ = guided_case(9, 2, 69, 8)
    N = 2
    te = engine_term(term, N)
    sc = torch.tensor(term["scale"], dtype=torch.float64)

    def value(z):
        v = eng.pair_loss(eng.decode(z, cond, cs, descaled_output=True), te, want_grad=False).cpu().double()
        return float((v * sc[:, None]).sum())
    gd = dict(curr_states=cs, pair=te, optimizer="sgd", lr=1.0)
    _, g = eng.guidance_step(mean, cond, gd, sigma=0.0, want_grad=True)
    gmax = float(g.abs().max())
    assert gmax > 0.0
    v0 = value(mean)
    v1 = value(eng.guidance_step(mean, cond, dict(gd, lr=0.05 / gmax), sigma=0.0))
    v4 = value(eng.guidance_step(mean, cond, dict(gd, lr=0.05 / gmax, grad_steps=4), sigma=0.0))
    print(f"   pair total of the decoded plans: {v0:.4f} -> {v1:.4f} (1 SGD step) -> {v4:.4f} (4 steps)")
    assert v0 > v1 > v4 > 0.0


def test_get_action_with_a_gptcollision_config():
    """Upstream's guidance configuration with a speed limit in scene 0 and `gptcollision` + `gptkeepdistance` in scene 1, three
    samples: the values come back under upstream's keys on EVERY agent of the scene (NaN outside it), equal to the yardstick's on the
    returned trajectories; the choice of sample is scene-level: one sample for the scene, the one with the smallest summed loss."""
    from tests.test_gpu_social import _policy
    pol = _policy()
    sizes, N = [3, 5], 3
    B = sum(sizes)
    inp = synth.make_inputs(B, 9)
    sc = synth.make_collision_scene(sizes, 9, spacing=6.0)
    W = torch.from_numpy(sc["world_from_agent"])
    F = Y.invert_frames(W.double()).float()
    cfg = [[{"name": "speed_limit", "weight": 1.0, "agents": None, "params": {"speed_limit": 6.0}}],
           [{"name": "gptcollision", "weight": 2.0, "agents": None, "params": {"target_ind": 4, "ref_ind": 1, "collision_radius": 0.5}},
            {"name": "gptkeepdistance", "weight": 1.0, "agents": None, "params": {"target_ind": 1, "ref_ind": 2, "min_distance": 50.0, "max_distance": 60.0}}]]
    pol.set_guidance(cfg, torch.from_numpy(sc["scene_index"]), data_batch={"world_from_agent": W, "agent_from_world": F}, lr=0.05, optimizer="sgd", grad_steps=2)
    obs = {"cond_feat": torch.from_numpy(inp["cond_feat"]).cuda(), "curr_states": torch.from_numpy(inp["curr_states"]).cuda()}
    nz = synth.make_noise(B * N, 10, 3)
    noise = {"x_T": torch.from_numpy(nz["x_T"]).reshape(B, N, 52, 4), "noise": torch.from_numpy(nz["noise"])}
    act, info = pol.get_action(obs, num_action_samples=N, noise=noise, step_index=0)
    keys = ["speed_limit_scene_000_00", "gptcollision_scene_001_00", "gptkeepdistance_scene_001_01"]
    assert list(info["guide_losses"]) == keys
    traj = info["trajectories"].cpu()
    pt = pol._guidance["pair"]
    assert pt["target"] == [7, 4] and pt["ref"] == [4, 5] and pt["configs"] == [(1, 0), (1, 1)]
    term = dict(target=pt["target"], ref=pt["ref"], kind=pt["kind"], lo=pt["lo"], hi=pt["hi"], decay=pt["decay"], scale=[w / N for w in pt["weight"]],
                world_from_agent=W.double(), agent_from_world=F.double())
    check_margins(traj, term)
    ref = Y.values(traj.double(), term)
    inside = torch.from_numpy(sc["scene_index"]) == 1
    for p, key in enumerate(keys[1:]):
        got = info["guide_losses"][key].cpu()
        assert bool(torch.isnan(got[~inside]).all()) and not bool(torch.isnan(got[inside]).any())
        assert torch.equal(got[inside], got[inside][:1].expand(int(inside.sum()), N))          # the [N] value under every agent of the scene
        assert float((got[inside][0].double() - ref[p]).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    # upstream's selection: the last scene's losses are scene-level, so ONE sample is chosen, for the whole batch as upstream writes it
    scene_loss = sum(torch.nan_to_num(info["guide_losses"][k].cpu(), nan=0.0) for k in keys[1:])
    expect = torch.argmin(scene_loss.sum(dim=0))
    assert bool((info["act_idx"].cpu() == expect).all())
    without = pol.get_action(obs, num_action_samples=N, noise=noise, step_index=0, guide_as_filter_only=True)[1]
    assert list(without["guide_losses"]) == keys and not torch.equal(without["trajectories"], info["trajectories"])    # the term steered the plans
    # the same term as a plain `guidance=` dict (one scene): keyed by the relations' config names, the same values, one sample for all
    plain = pol.get_action(obs, num_action_samples=N, noise=noise, guidance=dict(pair=pt, lr=0.05, optimizer="sgd", grad_steps=2))[1]
    assert list(plain["guide_losses"]) == ["gptcollision_scene_000_00", "gptkeepdistance_scene_000_01"]
    assert len(set(plain["act_idx"].cpu().tolist())) == 1
    check_margins(plain["trajectories"].cpu(), term)
    ref_p = Y.values(plain["trajectories"].cpu().double(), term)
    for p, key in enumerate(plain["guide_losses"]):
        got = plain["guide_losses"][key].cpu()
        assert torch.equal(got, got[:1].expand(B, N)) and float((got[0].double() - ref_p[p]).abs().max()) <= 2e-5 * max(1.0, float(ref_p.abs().max()))
    with pytest.raises(NotImplementedError, match="agents"):
        pol.set_guidance([[], [dict(cfg[1][0], agents=[0, 1])]], torch.from_numpy(sc["scene_index"]), data_batch={"world_from_agent": W})


def test_closed_loop_rollout_with_a_pair_term_follows_the_observation():
    """Three sim steps, six agents, follow_observation=True: the term's frames follow the world pose of every re-plan (the loop
    supplies world_from_agent; with no agent_from_world in the observation the library inverts the rotation), the two agents of the
    pair are steered and the four others move exactly as they do without guidance."""
    from cld_amd.policy import closed_loop_rollout, frames_from_pose
    from tests.test_gpu_social import _policy
    pol = _policy()
    B = 6
    inp = synth.make_inputs(B, 13)
    cond = torch.from_numpy(inp["cond_feat"]).cuda()
    centroid = torch.tensor([[0.0, 0.0], [4.0, 3.0], [9.0, -2.0], [13.0, 4.0], [18.0, 0.5], [60.0, 30.0]])
    yaw = torch.tensor([0.0, 0.2, -0.1, 0.3, 0.1, 1.0])
    world0 = torch.cat([centroid, yaw[:, None]], dim=1)
    nz = synth.make_noise(B, 10, 5)
    noise = {"x_T": torch.from_numpy(nz["x_T"]).reshape(B, 1, 52, 4), "noise": torch.from_numpy(nz["noise"])}
    cfg = [[{"name": "gptkeepdistance", "weight": 4.0, "agents": None, "params": {"target_ind": 1, "ref_ind": 3, "min_distance": 40.0, "max_distance": 50.0}}]]
    seen, terms = [], []
    inner = pol.get_action

    def spy(obs, **kw):
        seen.append(torch.as_tensor(obs["world_from_agent"]).clone().cpu())
        return inner(obs, **kw)
    pol.get_action = spy
    pol.set_guidance(cfg, torch.zeros(B, dtype=torch.long), data_batch={"world_from_agent": frames_from_pose(world0)}, lr=0.05, optimizer="adam",
                     follow_observation=True)
    poses = closed_loop_rollout(pol, lambda step, world, cs: cond, centroid, yaw, torch.from_numpy(inp["curr_states"]), 3, n_step_action=5, noise=noise)
    assert len(seen) == 3
    assert torch.equal(seen[0], frames_from_pose(world0.cuda()).cpu()) and torch.equal(seen[1], frames_from_pose(poses[0]).cpu()) and not torch.equal(seen[1], seen[0])
    assert pol._guidance["pair"]["world_from_agent"] is not seen[1]      # the configured term itself is not modified
    pol.get_action = inner
    pol.clear_guidance()
    free = closed_loop_rollout(pol, lambda step, world, cs: cond, centroid, yaw, torch.from_numpy(inp["curr_states"]), 3, n_step_action=5, noise=noise)
    assert not torch.equal(free[:, 1], poses[:, 1]) and not torch.equal(free[:, 3], poses[:, 3])      # both ends of the pair were steered
    for a in (0, 2, 4, 5):
        assert torch.equal(free[:, a], poses[:, a])                       # the others were not
