"""GPU parity of the lane guidance (csrc/lane_kernels.hip; upstream's LaneFollowingLoss, ChangeToLeftLaneLoss, FollowLaneLoss,
guidance_loss.py:1574-1628, 1795-1841, 1958-2011, on project_onto, trajdata_utils.py:726-821): the kernels against the recording made
from the reference's own code (tests/golden/lane_guidance.npz) and against the fp64 yardstick (tests/lane_yardstick.py, pinned by
that recording: tests/test_lane_host.py) at the polyline sizes where the launch logic changes; cld_lane_prepare against numpy; the
term inside the guided sampler (cld_set_lane_term); the policy surface and the closed-loop rollout.

Bars: 4 x the larger of the reference's own fp32 error against the yardstick (the recording's meta) and the rounding bound of a
52-term fp32 sum, 52 2^-24 max|ref| (tests/test_lane_host.sum_bar).  The conditions of the random cases (near-tie fraction, checked
rows per kind, kink margins) are asserted on the CPU in tests/test_lane_host.py."""
import ctypes

import numpy as np
import pytest
import torch

from cld_amd import synth
from tests import lane_cases as LC
from tests import lane_yardstick as Y
from tests.test_lane_host import CASES, config_values, recorded_case, sum_bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(precision):
    from cld_amd.engine import Engine
    e = Engine(n_timesteps=100, device="cuda:0", precision=precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True))
    e.load_state_dict(synth.make_decoder_weights(0))
    return e.finalize()


@pytest.fixture(scope="module")
def ref_err(golden):
    """The reference's own fp32 errors against the yardstick, the largest over the recorded cases: (projection, value, gradient)."""
    cases = golden("lane_guidance")[0]["cases"]
    return tuple(max(c[k] for c in cases.values()) for k in ("ref_proj_err", "ref_value_err", "ref_grad_err"))


def engine_term(term, N=1, **kw):
    """The yardstick's term as Engine.lane_loss / the guidance dict take it."""
    return dict(agent=term["agent"], line=term["line"], kind=term["kind"], decay=term["decay"], scale=term["scale"],
                lines=torch.as_tensor(term["lines"]).float(), num_samp=N, **kw)


def check_kernel(eng, plans, term, errs, ref=None):
    """Engine.lane_loss on plans [A,N,52,6] against the yardstick (or `ref` = (projection, values, gradient) of the recording):
    projection per element -- an element whose gap is below 1e-4 m may take the outcome of any segment within that gap --, values on
    the (entry, sample) rows free of such elements, the gradient on the (agent, sample) rows all of whose entries are; exact zeros in
    columns 2, 4, 5 and on agents without an entry, whose rows carry grad_in bit for bit; the same bits on a second run."""
    A, N = plans.shape[:2]
    E = len(term["agent"])
    te = engine_term(term, N)
    flat = plans.reshape(A * N, 52, 6)
    value, grad, proj = eng.lane_loss(flat, te, want_proj=True)
    yv, yg = Y.value_and_grad(plans.double(), term)
    yp, gap = Y.projections(plans.double(), term)
    if ref is not None:
        assert float(gap.min()) >= LC.NEAR
        yp, yv, yg = ref
    near = gap < LC.NEAR
    got_p, got_v, got_g = proj.cpu().double(), value.cpu().double(), grad.cpu().double().reshape(A, N, 52, 6)
    bar_p, bar_v, bar_g = sum_bar(errs[0], float(yp.abs().max())), sum_bar(errs[1], float(yv.abs().max())), sum_bar(errs[2], float(yg.abs().max()))
    diff = (got_p - yp).abs().amax(dim=-1)
    worst = float(diff[~near].max())
    for e, n, t in torch.nonzero(near & ~(diff <= bar_p)).tolist():      # a near-tie that went the other way: any outcome within the gap
        line = torch.as_tensor(term["lines"])[term["line"][e]].double()
        out, mask = Y.candidates(plans[term["agent"][e], n, t, :2].double(), line, LC.NEAR)
        d = float((out[mask] - got_p[e, n, t]).abs().amax(dim=-1).min())
        assert d <= bar_p, (e, n, t, d)
    rows = ~near.any(dim=-1)
    err_v = float((got_v - yv).abs()[rows].max())
    clean = torch.ones(A, N, dtype=torch.bool)
    for e in range(E):
        clean[term["agent"][e]] &= rows[e]
    err_g = float((got_g - yg).abs()[clean].max())
    print(f"   {E} entries x {N}: near-ties {float(near.double().mean()):.4f}; projection {worst:.2e} (bar {bar_p:.2e}), values {err_v:.2e} (bar {bar_v:.2e}, "
          f"max {float(yv.abs().max()):.3f}), gradient {err_g:.2e} (bar {bar_g:.2e}, max {float(yg.abs().max()):.3e})")
    assert worst <= bar_p and err_v <= bar_v and float(yg.abs().max()) > 0 and err_g <= bar_g
    quiet = torch.ones(A, dtype=torch.bool)
    quiet[term["agent"]] = False
    assert float(got_g[quiet].abs().max()) == 0.0 and float(got_g[..., [2, 4, 5]].abs().max()) == 0.0
    for e in range(E):                                                    # the decayed form has no yaw term
        others = [k for k in range(E) if term["agent"][k] == term["agent"][e] and term["kind"][k] != "follow_decayed"]
        if term["kind"][e] == "follow_decayed" and not others:
            assert float(got_g[term["agent"][e], ..., 3].abs().max()) == 0.0
    gin = torch.from_numpy(synth.normal(3, "lane_grad_in", (A * N, 52, 6)))
    value2, grad2, proj2 = eng.lane_loss(flat, te, grad_in=gin, want_proj=True)
    g2 = grad2.cpu().reshape(A, N, 52, 6)
    assert torch.equal(value2, value) and torch.equal(proj2, proj)
    assert float((g2 - (grad.cpu().reshape(A, N, 52, 6) + gin.reshape(A, N, 52, 6))).abs().max()) <= 1e-6
    assert torch.equal(g2[quiet], gin.reshape(A, N, 52, 6)[quiet]) and torch.equal(g2[..., [2, 4, 5]], gin.reshape(A, N, 52, 6)[..., [2, 4, 5]])
    value3, grad3, proj3 = eng.lane_loss(flat, te, want_proj=True)        # determinism: the same bits
    assert torch.equal(value3, value) and torch.equal(grad3, grad) and torch.equal(proj3, proj)
    assert torch.equal(eng.lane_loss(flat, te, want_grad=False), value)
    return value, grad


@pytest.mark.parametrize("name", CASES)
def test_lane_kernel_golden(golden, eng, name):
    """The recording's 12 rows, every case, against the reference's own project_onto and classes + autograd: the projection per
    element, the per-config values (LaneFollowingLoss: the mean over its targets), d total / d plans."""
    meta, g, plans, term = recorded_case(golden, name)
    case = meta["cases"][name]
    yv = Y.values(plans.double(), term)
    ref = (torch.from_numpy(g[name + "_proj"]).double(), yv, torch.from_numpy(g[name + "_grad"]).double())
    errs = (case["ref_proj_err"], case["ref_value_err"], case["ref_grad_err"])
    value, _ = check_kernel(eng, plans, term, errs, ref=ref)
    for k, cv in enumerate(config_values(case, value.cpu().double())):
        ref_v = torch.from_numpy(g[f"{name}_values_{k}"]).double()
        assert float((cv - ref_v).abs().max()) <= sum_bar(case["ref_value_err"], float(ref_v.abs().max()))
    tot = float((value.cpu().double() * torch.tensor(term["scale"], dtype=torch.float64)[:, None]).sum())
    assert abs(tot - float(g[name + "_total"][0])) <= sum_bar(case["ref_value_err"], 1.0) * sum(q["weight"] for q in case["entries"])


@pytest.mark.parametrize("N", LC.SAMPLES)
@pytest.mark.parametrize("S", LC.SIZES)
def test_lane_kernel_vs_yardstick_at_the_sizes_where_the_launch_changes(eng, ref_err, S, N):
    """Polylines of 2 .. 1024 points (tests/lane_cases.py), one and three samples; an agent with two entries, one with none."""
    plans, term = LC.size_case(S, N)
    check_kernel(eng, plans, term, ref_err)


def test_lane_kernel_vs_yardstick_on_two_scenes_of_70_agents(eng, ref_err):
    """70 agents in two scenes, two samples: one workgroup per (entry, sample), the entries of an agent walked by its first one."""
    plans, term = LC.scenes_case()
    check_kernel(eng, plans, term, ref_err)


def test_lane_prepare_vs_numpy(golden, eng):
    """cld_lane_prepare against the numpy restatement (fp64 transform, one rounding, stable sort by x): to 1 fp32 ulp on the recording's
    polylines (about 1 m apart: far more than that, so the order is the same), the exact index order on constructed equal x (-0 = +0),
    NaN rows last, a frame outside the array gives NaN, 1024 points accepted and 1025 refused."""
    from cld_amd._lib import CldError
    _, g = golden("lane_guidance")
    got = eng.lane_prepare(g["world_lines"], g["line_frame"], g["agent_from_world"]).cpu().numpy()
    ref = g["lines"]
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert bool((np.abs(got[ok] - ref[ok]) <= np.spacing(np.abs(ref[ok]))).all())
    print(f"   lane_prepare: {int((got[ok] != ref[ok]).sum())} of {int(ok.sum())} values differ from numpy's, each by one ulp")
    eye = np.eye(3, dtype=np.float32)[None]
    xs = np.array([1.0, np.nan, 1.0, -0.0, 0.0, 1.0, np.nan, -0.0, -2.0, 1.0, 0.0])
    wl = np.stack([xs, np.arange(xs.size, dtype=np.float64), np.zeros(xs.size)], axis=1)[None]
    wl[0, np.isnan(xs), 1:] = np.nan
    out = eng.lane_prepare(wl, [0], eye).cpu().numpy()[0]
    assert out[:9, 1].tolist() == [8.0, 3.0, 4.0, 7.0, 10.0, 0.0, 2.0, 5.0, 9.0] and bool(np.isnan(out[9:]).all())
    assert np.array_equal(out, Y.prepare(wl, [0], eye)[0], equal_nan=True)
    assert bool(np.isnan(eng.lane_prepare(wl, [3], eye).cpu().numpy()).all()) and bool(np.isnan(eng.lane_prepare(wl, [-1], eye).cpu().numpy()).all())
    rng = np.random.default_rng(5)
    for S in (1, 2, 700, 1024):                 # a shuffled polyline (x' at least 0.5 m apart), a rotated frame, a third of the rows NaN
        th = 0.4
        F = np.array([[[np.cos(th), np.sin(th), 3.0], [-np.sin(th), np.cos(th), -2.0], [0, 0, 1]]], np.float32)
        big = np.stack([rng.permutation(S) * 1.0 + 500.0, rng.uniform(-0.5, 0.5, S) + 300.0, rng.uniform(-3, 3, S)], axis=1)[None]
        big[0, rng.random(S) < 0.33] = np.nan
        got, ref = eng.lane_prepare(big, [0], F).cpu().numpy(), Y.prepare(big, [0], F)
        ok = ~np.isnan(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and bool((np.abs(got[ok] - ref[ok]) <= np.spacing(np.abs(ref[ok]))).all()), S
    with pytest.raises(CldError, match="max_pts"):
        eng.lane_prepare(np.zeros((1, 1025, 3)), [0], eye)


def test_malformed_terms_are_refused_before_any_launch_and_bad_entries_get_nan(eng):
    """The contracts: a malformed cld_lane_term is CLD_ERR_ARG with no output written, standalone and on the handle; device-side
    entries outside the batch or the polylines, and an all-NaN (or single-point) polyline, get a NaN value and projection, make no
    contribution and leave every other bit alone; the Engine refuses such entries unless told not to look."""
    from cld_amd._lib import CldError
    plans, term = LC.size_case(6, 3)
    A, N = plans.shape[:2]
    flat = plans.reshape(A * N, 52, 6)
    gin = torch.from_numpy(synth.normal(5, "lane_grad_in", (A * N, 52, 6)))
    value, grad, proj = eng.lane_loss(flat, engine_term(term, N), grad_in=gin, want_proj=True)
    lines = torch.as_tensor(term["lines"]).float()
    dead = torch.full_like(lines[:2], float("nan"))
    dead[1, 0] = torch.tensor([1.0, 2.0, 0.0])
    dead[1, 1] = torch.tensor([1.0, 2.0, 0.5])                             # two equal points: no segment of non-zero length
    bad = dict(term, lines=torch.cat([lines, dead]).double())
    L = lines.shape[0]
    # agent 1's bad entries sit next to its real one (an agent's entries are contiguous); agent 0 carries only dead polylines
    extra = [(1, L + 2), (1, -1), (0, L), (0, L + 1), (A, 0), (-1, 1), (2 ** 31 - 1, 2)]
    E0 = len(term["agent"])
    order = [0, E0, E0 + 1] + list(range(1, E0)) + list(range(E0 + 2, E0 + len(extra)))
    for k, add in (("agent", [a for a, _ in extra]), ("line", [l for _, l in extra]), ("kind", [Y.KINDS[c % 3] for c in range(len(extra))]),
                   ("decay", [0.9] * len(extra)), ("scale", [1.0] * len(extra))):
        full = term[k] + add
        bad[k] = [full[e] for e in order]
    with pytest.raises(CldError, match="outside"):
        eng.lane_loss(flat, engine_term(bad, N))
    vb, gb, pb = eng.lane_loss(flat, engine_term(bad, N, validate=False), grad_in=gin, want_proj=True)
    E = len(term["agent"])
    real = [i for i, e in enumerate(order) if e < E]
    fake = [i for i, e in enumerate(order) if e >= E]
    assert torch.equal(vb[real], value) and torch.equal(pb[real], proj) and torch.equal(gb, grad)
    assert bool(torch.isnan(vb[fake]).all()) and bool(torch.isnan(pb[fake]).all())
    with pytest.raises(CldError, match="not contiguous"):
        eng.lane_loss(flat, dict(engine_term(term, N), agent=[1, 2, 3, 2, 4]))
    for broken in (dict(kind="nearby"), dict(kind=7), dict(decay=[0.9]), dict(agent=term["agent"][:-1]), dict(lines=lines[:, :1])):
        with pytest.raises(CldError):
            eng.lane_loss(flat, dict(engine_term(term, N), **broken))
    with pytest.raises(CldError, match="num_samp"):
        eng.lane_loss(flat, engine_term(term, 2))
    # the library itself: CLD_ERR_ARG, nothing written
    cs, keep = eng._lane(engine_term(term, N), A * N)
    out = torch.full((E, N), 7.0, device="cuda:0")
    for field, v in (("max_pts", 1025), ("max_pts", 1), ("num_entries", 0), ("num_lines", 0), ("num_samp", 2), ("scale", None)):
        old = getattr(cs, field)
        setattr(cs, field, v)
        rc = eng.lib.cld_lane_loss(eng._h, ctypes.c_void_p(flat.cuda().data_ptr()), ctypes.byref(cs), None, ctypes.c_void_p(out.data_ptr()), None, None, A * N, None)
        setattr(cs, field, old)
        torch.cuda.synchronize()
        assert rc != 0 and bool((out == 7.0).all()), field
    inp = synth.make_inputs(A * N, 3)
    mean, cond, cs4 = torch.from_numpy(synth.normal(3, "lane_mean", (A * N, 52, 4))) * 0.7, torch.from_numpy(inp["cond_feat"]), torch.from_numpy(inp["curr_states"])
    cs.max_pts = 1
    assert eng.lib.cld_set_lane_term(eng._h, ctypes.byref(cs)) == 0
    try:
        with pytest.raises(CldError, match="lane term"):
            eng.guidance_step(mean, cond, dict(curr_states=cs4, target_speed=torch.ones(A * N, 52), loss_scale=torch.ones(A * N), lr=0.1, optimizer="sgd"), sigma=0.0)
    finally:
        eng.lib.cld_set_lane_term(eng._h, None)


def guided_case(A, N, seed, S=40):
    """A guided step's inputs: latent means, conditioning, current states (speeds scaled to <= 3 m/s) and a lane term over agents
    1 .. A-1 -- agent 0 carries no entry, agent 2 two -- on agent-frame polylines of S points (S = 2: one segment, so no element can
    be a near-tie) -> (mean, cond, cs float32 [A N,...], yardstick term)."""
    rng = np.random.default_rng(seed)
    B = A * N
    inp = synth.make_inputs(B, seed)
    cond = torch.from_numpy(inp["cond_feat"])
    cs = torch.from_numpy(inp["curr_states"]) * torch.tensor([1.0, 1.0, 0.2, 1.0])
    mean = torch.from_numpy(synth.normal(seed, "lane_mean", (B, 52, 4))) * 0.7
    lines = np.stack([LC.make_line(rng, S) for _ in range(A)] + [LC.make_line(rng, S, left=True) for _ in range(A)])
    term = dict(agent=[], line=[], kind=[], decay=[], scale=[], lines=torch.from_numpy(lines).double())
    for a in range(1, A):
        for kind in ([Y.KINDS[a % 3]] + (["following"] if a == 2 else [])):
            for k, v in (("agent", a), ("line", a + (A if kind == "change_left" else 0)), ("kind", kind), ("decay", 0.9), ("scale", {"following": 0.5, "change_left": 2.0, "follow_decayed": 40.0}[kind] / N)):
                term[k].append(v)
    return mean, cond, cs, term


def manual_step(eng, mean, cond, cs, parts):
    """decode -> the loss kernels of `parts` [(Engine method, term)] chained through grad_in in that order -> the decoder's VJP."""
    traj = eng.decode(mean, cond, cs, descaled_output=True)
    g = None
    for fn, te in parts:
        g = fn(traj, te, grad_in=g)[1]
    return eng.decode_vjp(mean, cond, cs, g)


@pytest.mark.parametrize("decode", ["auto", "valu", "mfma"])
@pytest.mark.parametrize("kernel", ["valu", "mfma", "quad"])
def test_lane_guided_step_is_decode_lane_loss_update_in_every_kernel_form(eng, kernel, decode):
    """cld_guidance_step and cld_sample_step with the term on the handle against the manual composition of the library's own parts on
    the same iterate -- decode, cld_lane_loss, the decoder's VJP, x - lr g -- in every forced form of the guidance and decode kernels:
    the same kernels on the same inputs, so the gradient has the SAME BITS, and the guided mean is within one rounding of x - lr g.
    (The lane kernel itself is held against the yardstick above.)  9 agents x 2 samples; agent 0 carries no entry and does not move."""
    A, N = 9, 2
    mean, cond, cs, term = guided_case(A, N, 71)
    te = engine_term(term, N)
    eng.force_kernel("guide", kernel)
    eng.force_kernel("decode", decode)
    try:
        via = manual_step(eng, mean, cond, cs, [(eng.lane_loss, te)])
        lr = 0.05 / float(via.abs().max())
        gd = dict(curr_states=cs, lane=te, optimizer="sgd", lr=lr)
        mg, grad = eng.guidance_step(mean, cond, gd, sigma=0.0, want_grad=True)
        z = torch.from_numpy(synth.normal(72, "z", (A * N, 52, 4)))
        st = eng.sample_step(mean, cond, 40, z=z, guidance=gd, want_grad=True)
        via_s = manual_step(eng, st["mean"], cond, cs, [(eng.lane_loss, te)])
    finally:
        eng.force_kernel("guide", "auto")
        eng.force_kernel("decode", "auto")
    assert float(via.abs().max()) > 0 and torch.equal(grad, via) and torch.equal(st["grad"], via_s)
    one = 2.0 ** -23 * max(1.0, float(mean.abs().max()))
    assert float((mg.cpu().double() - (mean.double() - lr * via.cpu().double())).abs().max()) <= one
    assert float((st["mean_guided"].cpu().double() - (st["mean"].cpu().double() - lr * via_s.cpu().double())).abs().max()) <= 2.0 ** -23 * max(1.0, float(st["mean"].abs().max()))
    assert torch.equal(mg.cpu()[:N], mean[:N]) and float(grad.cpu()[:N].abs().max()) == 0.0 and float((mg.cpu() - mean).abs().max()) > 1e-3


def test_lane_guided_step_on_the_forward_sweep_path_at_256_rows(eng):
    """From 256 rows run_guidance decodes the iterate with the guidance kernel's forward sweep + the roll-out kernel, not cld_decode:
    the lane kernel runs behind that path too.  Single-segment polylines (no element can be a near-tie); the first step's gradient
    against decode -> the yardstick's fp64 gradient -> the library's VJP, at 1e-4 max|g| (the bar the pair term's test holds there)."""
    A, N = 128, 2
    mean, cond, cs, term = guided_case(A, N, 73, S=2)
    plans = eng.decode(mean, cond, cs, descaled_output=True).cpu().reshape(A, N, 52, 6)
    _, gp = Y.value_and_grad(plans.double(), term)
    ref = eng.decode_vjp(mean, cond, cs, gp.reshape(-1, 52, 6).float()).cpu().double()
    mg, grad = eng.guidance_step(mean, cond, dict(curr_states=cs, lane=engine_term(term, N), optimizer="sgd", lr=0.01), sigma=0.0, want_grad=True)
    err = float((grad.cpu().double() - ref).abs().max())
    print(f"   256 rows: gradient error {err:.2e} of max {float(ref.abs().max()):.2e}")
    assert float(ref.abs().max()) > 0 and err <= 1e-4 * float(ref.abs().max())


def test_the_lane_gradient_is_added_after_the_social_and_pair_terms(eng):
    """A lane term together with a pair and a social-group term: the guided step's gradient has the bits of decode -> social -> pair ->
    lane chained through grad_in in THAT order -> VJP; fp32 addition does not commute bit for bit, so the lane term added anywhere
    else gives other bits on this case (asserted)."""
    from tests.test_gpu_pair import engine_term as pair_term
    from tests.test_gpu_social import engine_term as social_term
    A, N = 9, 1
    mean, cond, cs, term = guided_case(A, N, 75)
    te = engine_term(term, N)
    i = np.arange(A)
    W = np.zeros((A, 3, 3), np.float32)
    W[:, 0, 0] = W[:, 1, 1] = W[:, 2, 2] = 1.0
    W[:, 0, 2], W[:, 1, 2] = 6.0 * i, 2.0 * (i % 3)
    Wd = torch.from_numpy(W).double()
    pair = dict(target=[2, 4, 5], ref=[3, 2, 7], kind=["keep_distance", "stay_away", "front_collision"], lo=[20.0, 30.0, 0.0], hi=[25.0, 35.0, 0.0],
                decay=[0.0, 0.9, 0.0], scale=[0.7, 20.0, 0.3], world_from_agent=Wd, agent_from_world=None)
    social = dict(groups=[[1, 2, 4, 5]], leader=[2], social_dist=[1.5], cohesion=[1.0], scale=[0.05], world_from_agent=Wd)
    rng = np.random.default_rng(76)
    r = torch.from_numpy((rng.integers(0, 1 << 30, (A, 52)) % 3).astype(np.int32))
    u = torch.from_numpy(rng.uniform(0.0, 0.999, (A, 52)).astype(np.float32))
    pe, se = pair_term(pair, N), social_term(social, N, draw_r=r, draw_u=u)
    gd = dict(curr_states=cs, lane=te, pair=pe, social_group=social_term(social, N, draw_r=r[None, None], draw_u=u[None, None]), optimizer="sgd", lr=0.01)
    _, grad = eng.guidance_step(mean, cond, gd, sigma=0.0, want_grad=True)
    parts = {"social": (eng.social_group_loss, se), "pair": (eng.pair_loss, pe), "lane": (eng.lane_loss, te)}
    right = manual_step(eng, mean, cond, cs, [parts[k] for k in ("social", "pair", "lane")])
    assert torch.equal(grad, right)
    for order in (("lane", "social", "pair"), ("social", "lane", "pair")):
        assert not torch.equal(manual_step(eng, mean, cond, cs, [parts[k] for k in order]), right), order
    for k in ("lane", "pair", "social_group"):                             # each of the three matters in this step
        assert not torch.equal(eng.guidance_step(mean, cond, {q: v for q, v in gd.items() if q != k}, sigma=0.0, want_grad=True)[1], grad)


CHAIN = ("agent_collision", "map_collision", "goal", "social_group", "pair", "lane")


def six_term_case(eng, N, steps=1):
    """Nine agents x N samples with all six plan-space terms and a caller gradient -> (mean, cond, cs, guidance dict, the stand-alone
    loss of every term by its guidance key, ext_grad).  The agent-collision scene puts the agents 3 m apart, the map term reads a
    random 32 x 32 drivable raster at 2 px/m, goals / social group / pairs / lanes overlap on agents 1 .. 7."""
    from tests.test_gpu_goal import engine_goal
    from tests.test_gpu_pair import engine_term as pair_term
    from tests.test_gpu_social import engine_term as social_term
    A = 9
    B = A * N
    mean, cond, cs, term = guided_case(A, N, 81)
    rng = np.random.default_rng(82)
    i = np.arange(A)
    W = np.zeros((A, 3, 3), np.float32)
    W[:, 0, 0] = W[:, 1, 1] = W[:, 2, 2] = 1.0
    W[:, 0, 2], W[:, 1, 2] = 6.0 * i, 2.0 * (i % 3)
    Wd = torch.from_numpy(W).double()
    F = Wd.clone()
    F[:, :2, 2] = -Wd[:, :2, 2]
    speed = cs[::N, 2].clone()
    sc = synth.make_collision_scene([A], 83, spacing=3.0)
    col = dict(extent=torch.from_numpy(sc["extent"]), world_from_agent=torch.from_numpy(sc["world_from_agent"]), curr_speed=speed,
               scene_sizes=[A], weight=40.0, num_samp=N)
    R = torch.zeros(A, 3, 3)
    R[:, 0, 0] = R[:, 1, 1] = 2.0
    R[:, 0, 2], R[:, 1, 2], R[:, 2, 2] = 6.0, 16.0, 1.0
    mcol = dict(extent=torch.from_numpy(sc["extent"]), raster_from_agent=R, drivable_map=torch.from_numpy((rng.random((A, 32, 32)) < 0.6).astype(np.uint8)),
                curr_speed=speed, weight=0.3, num_samp=N)
    local = torch.tensor([[3.0, 2.5], [0.5, 12.0], [6.0, 1.0], [9.0, -2.0]] * 3, dtype=torch.float64)[:A]
    goal = engine_goal(dict(kind=torch.tensor([1, 1, 2, 2] * 3, dtype=torch.int32)[:A], target_time=torch.tensor([0, 0, 34, 50] * 3, dtype=torch.int32)[:A],
                            urgency=torch.tensor([0.5, 1.0, 0.5, 0.5] * 3, dtype=torch.float64)[:A], pref_speed=torch.full((A,), 1.42, dtype=torch.float64),
                            scale=torch.full((A,), 0.4 / N, dtype=torch.float64), reached=torch.zeros(A, dtype=torch.bool), global_t=4, dt=0.1,
                            min_progress_dist=0.5, target_pos=(local + Wd[:, :2, 2]).float().double(), agent_from_world=F), N)
    pair = dict(target=[2, 4, 5], ref=[3, 2, 7], kind=["keep_distance", "stay_away", "front_collision"], lo=[20.0, 30.0, 0.0], hi=[25.0, 35.0, 0.0],
                decay=[0.0, 0.9, 0.0], scale=[0.7 / N, 20.0 / N, 0.3 / N], world_from_agent=Wd, agent_from_world=None)
    social = dict(groups=[[1, 2, 4, 5]], leader=[2], social_dist=[1.5], cohesion=[1.0], scale=[0.05 / N], world_from_agent=Wd)
    r = torch.from_numpy((rng.integers(0, 1 << 30, (1, steps, B, 52)) % 3).astype(np.int32))
    u = torch.from_numpy(rng.uniform(0.0, 0.999, (1, steps, B, 52)).astype(np.float32))
    ext = torch.from_numpy(synth.normal(84, "six_term_ext_grad", (B, 52, 6))) * 0.05
    te = engine_term(term, N)
    gd = dict(curr_states=cs, agent_collision=col, map_collision=mcol, goal=goal, social_group=social_term(social, N, draw_r=r, draw_u=u),
              pair=pair_term(pair, N), lane=te, ext_grad=ext, optimizer="sgd", lr=0.01, grad_steps=steps)
    parts = {"agent_collision": (eng.agent_collision, col), "map_collision": (eng.map_collision, mcol), "goal": (eng.goal_loss, goal),
             "social_group": (eng.social_group_loss, social_term(social, N, draw_r=r[0, 0], draw_u=u[0, 0])), "pair": (eng.pair_loss, gd["pair"]),
             "lane": (eng.lane_loss, te)}
    return mean, cond, cs, gd, parts, ext


@pytest.mark.parametrize("N", [1, 2])
def test_the_six_plan_space_terms_are_chained_in_order_on_top_of_the_callers_gradient(eng, N):
    """All six plan-space terms and a caller ext_grad in one SGD step: the gradient has the bits of decode -> agent collision -> map
    collision -> goal -> social group -> pair -> lane chained through grad_in in THAT order, starting from ext_grad -> VJP (the same
    decode and loss kernels on the same inputs: no tolerance).  Swapping any two neighbours of the chain gives other bits, and so does
    leaving out any term or the caller's gradient."""
    mean, cond, cs, gd, parts, ext = six_term_case(eng, N)

    def chain(order):
        g = ext
        traj = eng.decode(mean, cond, cs, descaled_output=True)
        for k in order:
            fn, te = parts[k]
            g = fn(traj, te, grad_in=g)[1]
        return eng.decode_vjp(mean, cond, cs, g)
    _, grad = eng.guidance_step(mean, cond, gd, sigma=0.0, want_grad=True)
    right = chain(CHAIN)
    assert float(right.abs().max()) > 0 and torch.equal(grad, right)
    for j in range(len(CHAIN) - 1):
        order = list(CHAIN)
        order[j], order[j + 1] = order[j + 1], order[j]
        assert not torch.equal(chain(order), right), order
    for k in CHAIN + ("ext_grad",):
        assert not torch.equal(eng.guidance_step(mean, cond, {q: v for q, v in gd.items() if q != k}, sigma=0.0, want_grad=True)[1], grad), k


def test_two_grad_steps_over_the_six_terms_give_the_same_bits_on_a_second_call(eng):
    """grad_steps = 2 over the six-term chain (the second evaluation reads its own social draws): guided mean and gradient are
    reproducible bit for bit, and the second step matters."""
    mean, cond, cs, gd, _, _ = six_term_case(eng, 2, steps=2)
    mg, grad = eng.guidance_step(mean, cond, gd, sigma=0.0, want_grad=True)
    mg2, grad2 = eng.guidance_step(mean, cond, gd, sigma=0.0, want_grad=True)
    assert torch.equal(mg, mg2) and torch.equal(grad, grad2)
    assert not torch.equal(eng.guidance_step(mean, cond, dict(gd, grad_steps=1), sigma=0.0), mg)


def test_adam_with_three_grad_steps_evaluates_the_lane_term_on_every_iterate(eng):
    """Adam, grad_steps = 3, step by step on the library's own iterates, as tests/test_gpu_pair.py does for the pair term: the iterate
    after k - 1 steps is what the call with grad_steps = k - 1 returns; the reference gradient of step k is taken THERE (decode, the
    yardstick's fp64 gradient w.r.t. the plans, the library's VJP), the reference step is torch's Adam formula on the reference
    gradients of steps 1 .. k, and the call with grad_steps = k must lie within 2e-4 max(1, max|mean|) + adam_budget (gradients
    agreeing to 1e-4 max|g|) of it.  Single-segment polylines: the projection has no near-ties.  Rows without an entry do not move,
    the same bits on a second call, the weighted total falls from step to step."""
    from tests.test_gpu_pair import adam_budget
    A, N, lr = 9, 2, 0.02
    mean, cond, cs, term = guided_case(A, N, 77, S=2)
    te = engine_term(term, N)
    sc = torch.tensor(term["scale"], dtype=torch.float64)
    gd = dict(curr_states=cs, lane=te, optimizer="adam", lr=lr)
    iterates = [mean] + [eng.guidance_step(mean, cond, dict(gd, grad_steps=k), sigma=0.0) for k in (1, 2, 3)]
    assert torch.equal(eng.guidance_step(mean, cond, dict(gd, grad_steps=3), sigma=0.0), iterates[3])
    bar = 2e-4 * max(1.0, float(mean.abs().max()))
    grads, tols = [], []
    m = v = 0.0
    for k in (1, 2, 3):
        x_prev = iterates[k - 1]
        plans = eng.decode(x_prev, cond, cs, descaled_output=True).cpu().reshape(A, N, 52, 6)
        _, gp = Y.value_and_grad(plans.double(), term)
        g = eng.decode_vjp(x_prev, cond, cs, gp.reshape(-1, 52, 6).float()).cpu().double()
        grads.append(g)
        tols.append(1e-4 * float(g.abs().max()))
        m, v = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
        ref = x_prev.cpu().double() - (lr / (1.0 - 0.9 ** k)) * m / (v.sqrt() / np.sqrt(1.0 - 0.999 ** k) + 1e-8)
        err = (iterates[k].cpu().double() - ref).abs()
        budget = adam_budget(grads, lr, tols)
        print(f"   Adam step {k}: max error {float(err.max()):.2e} (bar {bar:.2e}), worst excess over bar + budget {float((err - bar - budget).max()):.2e}")
        assert bool((err <= bar + budget).all()), k
    one, got = iterates[1].cpu().double(), iterates[3].cpu().double()
    assert torch.equal(got[:N], mean.double()[:N]) and float((one - mean).abs().max()) <= lr * 1.001 and float((got - mean).abs().max()) > 2.01 * lr

    def value(z):
        return float((eng.lane_loss(eng.decode(z.float(), cond, cs, descaled_output=True), te, want_grad=False).cpu().double() * sc[:, None]).sum())
    v0, v1, v3 = value(mean), value(one), value(got)
    print(f"   lane total of the decoded plans: {v0:.5f} -> {v1:.5f} (1 Adam step) -> {v3:.5f} (3 steps)")
    assert v0 > v1 > v3 > 0.0


def test_clearing_the_term_restores_the_previous_behaviour_bit_for_bit(eng):
    """No term outlives the call that set it (cld_set_lane_term(NULL) behind every call): a target-speed step gives the same bits before
    and after a lane-guided one, and the lane term matters in between."""
    A, N = 6, 1
    mean, cond, cs, term = guided_case(A, N, 79)
    gd = dict(curr_states=cs, target_speed=torch.full((A, 52), 4.0), loss_scale=torch.full((A,), 1.0 / 52), lr=0.1, optimizer="sgd")
    before = eng.guidance_step(mean, cond, gd, sigma=0.0)
    with_lane = eng.guidance_step(mean, cond, dict(gd, lane=engine_term(term, N)), sigma=0.0)
    after = eng.guidance_step(mean, cond, gd, sigma=0.0)
    assert torch.equal(before, after) and not torch.equal(with_lane, before)


def straight_lanes(world, rng):
    """Per agent a straight two-point lane through the world -- from 6 m behind to 70 m ahead of its pose, up to 1.5 m to its side --
    and its left neighbour 3.5 m further left -> (lane_points, left_lane_points) [B,2,3] float64, world frame."""
    B = world.shape[0]
    x, y, h = world[:, 0].double().numpy(), world[:, 1].double().numpy(), world[:, 2].double().numpy()
    out = []
    side = rng.uniform(-1.5, 1.5, B)
    for off in (side, side + 3.5):
        pts = np.zeros((B, 2, 3))
        for k, along in enumerate((-6.0, 70.0)):
            pts[:, k, 0] = x + along * np.cos(h) - off * np.sin(h)
            pts[:, k, 1] = y + along * np.sin(h) + off * np.cos(h)
            pts[:, k, 2] = h
        out.append(torch.from_numpy(pts))
    return out


def test_get_action_with_the_three_lane_configs():
    """Upstream's guidance configuration with `gptlanefollowing` (two targets) in scene 0 and `gptchangetoleftlane` + `gptfollowlane`
    in scene 1, three samples: the values come back under '<name>_scene_%03d_%02d' on EVERY agent of the scene (NaN outside it), equal
    to the yardstick's on the returned trajectories (LaneFollowingLoss: the mean over its targets); the choice of sample is
    scene-level; the terms steer the plans.  Single-segment lanes: no near-ties."""
    from cld_amd.policy import frames_from_pose
    from tests.test_gpu_social import _policy
    pol = _policy()
    sizes, N = [4, 5], 3
    B = sum(sizes)
    inp = synth.make_inputs(B, 9)
    rng = np.random.default_rng(9)
    world = torch.tensor(np.stack([30.0 * np.arange(B) + 200.0, -100.0 + 9.0 * np.arange(B), rng.uniform(-0.5, 0.5, B)], axis=1), dtype=torch.float32)
    W = frames_from_pose(world)
    lane, left = straight_lanes(world, rng)
    scene_index = torch.tensor([0] * 4 + [1] * 5)
    cfg = [[{"name": "gptlanefollowing", "weight": 2.0, "agents": None, "params": {"target_inds": [1, 3]}}],
           [{"name": "gptchangetoleftlane", "weight": 1.0, "agents": None, "params": {"target_ind": 2}},
            {"name": "gptfollowlane", "weight": 30.0, "agents": None, "params": {"target_ind": 4, "decay_rate": 0.85}}]]
    pol.set_guidance(cfg, scene_index, data_batch={"world_from_agent": W, "lane_points": lane, "left_lane_points": left}, lr=0.05, optimizer="sgd", grad_steps=2)
    obs = {"cond_feat": torch.from_numpy(inp["cond_feat"]).cuda(), "curr_states": torch.from_numpy(inp["curr_states"]).cuda()}
    nz = synth.make_noise(B * N, 10, 3)
    noise = {"x_T": torch.from_numpy(nz["x_T"]).reshape(B, N, 52, 4), "noise": torch.from_numpy(nz["noise"])}
    act, info = pol.get_action(obs, num_action_samples=N, noise=noise, step_index=0)
    keys = ["gptlanefollowing_scene_000_00", "gptchangetoleftlane_scene_001_00", "gptfollowlane_scene_001_01"]
    assert list(info["guide_losses"]) == keys
    lt = pol._guidance["lane"]
    assert lt["agent"] == [1, 3, 6, 8] and lt["kind"] == ["following", "following", "change_left", "follow_decayed"] and lt["weight"] == [1.0, 1.0, 1.0, 30.0]
    lines = Y.prepare(lt["world_lines"].numpy(), lt["line_frame"], torch.as_tensor(lt["agent_from_world"]).numpy())
    term = dict(agent=lt["agent"], line=lt["line"], kind=lt["kind"], decay=lt["decay"], scale=[w / N for w in lt["weight"]], lines=torch.from_numpy(lines).double())
    traj = info["trajectories"].cpu()
    ref = Y.values(traj.double(), term)
    want = [ref[:2].mean(dim=0), ref[2], ref[3]]
    errs = golden_errs()
    for k, key in enumerate(keys):
        inside = scene_index == (0 if k == 0 else 1)
        got = info["guide_losses"][key].cpu()
        assert bool(torch.isnan(got[~inside]).all()) and not bool(torch.isnan(got[inside]).any())
        assert torch.equal(got[inside], got[inside][:1].expand(int(inside.sum()), N))
        assert float((got[inside][0].double() - want[k]).abs().max()) <= sum_bar(errs[1], float(ref.abs().max()))
    scene_loss = sum(torch.nan_to_num(info["guide_losses"][k].cpu(), nan=0.0) for k in keys[1:])
    assert bool((info["act_idx"].cpu() == torch.argmin(scene_loss.sum(dim=0))).all())          # the last scene's choice, one sample for all (upstream)
    without = pol.get_action(obs, num_action_samples=N, noise=noise, step_index=0, guide_as_filter_only=True)[1]
    assert list(without["guide_losses"]) == keys and not torch.equal(without["trajectories"], info["trajectories"])
    for a in lt["agent"]:
        assert not torch.equal(without["trajectories"][a], info["trajectories"][a])
    for a in (0, 2, 4, 5, 7):
        assert torch.equal(without["trajectories"][a], info["trajectories"][a])                # agents without an entry are not steered
    with pytest.raises(NotImplementedError, match="agents"):
        pol.set_guidance([[dict(cfg[0][0], agents=[0, 1])], []], scene_index, data_batch={"world_from_agent": W, "lane_points": lane})
    with pytest.raises(ValueError, match="T = 30"):
        pol.set_guidance([[], [dict(cfg[1][1], params={"target_ind": 4, "T": 30})]], scene_index, data_batch={"world_from_agent": W, "lane_points": lane})


def golden_errs():
    from tests.conftest import load_golden
    cases = load_golden("lane_guidance")[0]["cases"]
    return tuple(max(c[k] for c in cases.values()) for k in ("ref_proj_err", "ref_value_err", "ref_grad_err"))


def test_closed_loop_rollout_with_a_lane_term_follows_the_observation():
    """Three sim steps, five agents, follow_observation=True, `gptfollowlane` on agent 2 whose lane lies 2 m to its left: at every
    re-plan the term is prepared again with the frames of THAT step's world pose (what the policy prepared equals a by-hand
    lane_prepare with those frames, bit for bit) and the polylines stay in the world; the guided agent ends closer to its lane than
    without the term on the same noise -- its mean lateral distance over the three sim steps is smaller -- and the others move exactly
    as they do without guidance."""
    from cld_amd.policy import closed_loop_rollout, frames_from_pose, invert_frames
    from tests.test_gpu_social import _policy
    pol = _policy()
    eng = pol.vae.engine
    B = 5
    inp = synth.make_inputs(B, 13)
    cond = torch.from_numpy(inp["cond_feat"]).cuda()
    centroid = torch.tensor([[0.0, 0.0], [14.0, 8.0], [30.0, -6.0], [45.0, 5.0], [60.0, 30.0]])
    yaw = torch.tensor([0.0, 0.2, -0.1, 0.3, 1.0])
    world0 = torch.cat([centroid, yaw[:, None]], dim=1)
    lane = torch.zeros(B, 2, 3, dtype=torch.float64)
    for k, along in enumerate((-10.0, 90.0)):                              # 2 m to the left of every agent's pose, straight
        lane[:, k, 0] = centroid[:, 0].double() + along * torch.cos(yaw.double()) - 2.0 * torch.sin(yaw.double())
        lane[:, k, 1] = centroid[:, 1].double() + along * torch.sin(yaw.double()) + 2.0 * torch.cos(yaw.double())
        lane[:, k, 2] = yaw.double()
    nz = synth.make_noise(B, 10, 5)
    noise = {"x_T": torch.from_numpy(nz["x_T"]).reshape(B, 1, 52, 4), "noise": torch.from_numpy(nz["noise"])}
    cfg = [[{"name": "gptfollowlane", "weight": 200.0, "agents": None, "params": {"target_ind": 2, "decay_rate": 0.95}}]]
    calls, seen = [], []
    inner_prepare, inner_action = eng.lane_prepare, pol.get_action

    def spy_prepare(world_lines, line_frame, agent_from_world):
        out = inner_prepare(world_lines, line_frame, agent_from_world)
        calls.append((torch.as_tensor(world_lines).clone(), list(line_frame), torch.as_tensor(agent_from_world).clone().cpu(), out.clone()))
        return out

    def spy_action(obs, **kw):
        seen.append(torch.as_tensor(obs["world_from_agent"]).clone().cpu())
        return inner_action(obs, **kw)
    eng.lane_prepare, pol.get_action = spy_prepare, spy_action
    try:
        pol.set_guidance(cfg, torch.zeros(B, dtype=torch.long), data_batch={"world_from_agent": frames_from_pose(world0), "lane_points": lane}, lr=0.3,
                         optimizer="adam", follow_observation=True)
        poses = closed_loop_rollout(pol, lambda step, world, cs: cond, centroid, yaw, torch.from_numpy(inp["curr_states"]), 3, n_step_action=5, noise=noise)
    finally:
        eng.lane_prepare, pol.get_action = inner_prepare, inner_action
    assert len(seen) == 3 and len(calls) >= 3
    pose_of = [world0.cuda()] + [poses[k] for k in range(2)]
    per_step = len(calls) // 3
    for k in range(3):
        F = invert_frames(frames_from_pose(pose_of[k]).float()).cpu()
        assert torch.equal(seen[k], frames_from_pose(pose_of[k]).cpu())
        for wl, fr, afw, out in calls[k * per_step:(k + 1) * per_step]:
            assert torch.equal(afw, F) and fr == [2] and torch.equal(wl[0], lane[2])
            assert torch.equal(out, eng.lane_prepare(lane[2:3], [2], F))
    assert not torch.equal(calls[0][3], calls[per_step][3])               # the frames moved, and the prepared polyline with them
    pol.clear_guidance()
    free = closed_loop_rollout(pol, lambda step, world, cs: cond, centroid, yaw, torch.from_numpy(inp["curr_states"]), 3, n_step_action=5, noise=noise)

    def lateral(p):                                                        # distance of agent 2's poses from its (straight) lane
        p0, h = lane[2, 0, :2], float(lane[2, 0, 2])
        d = p[:, 2, :2].cpu().double() - p0
        return float((d[:, 1] * np.cos(h) - d[:, 0] * np.sin(h)).abs().mean())
    print(f"   agent 2's mean lateral distance from its lane: {lateral(poses):.3f} m with the term, {lateral(free):.3f} m without")
    assert lateral(poses) < lateral(free)
    for a in (0, 1, 3, 4):
        assert torch.equal(free[:, a], poses[:, a])
