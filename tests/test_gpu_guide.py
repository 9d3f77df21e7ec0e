"""GPU tests of the guidance kernels (csrc/guide_kernels.hip): guide_kernel (VALU, 2 agents per workgroup), guide_mfma8_kernel (16) and
guide_quad_kernel (8) with the roll-out gradient they share (chain_grad, chain_grad_group), against autograd over the oracle's own loss in
float64 on the CPU -- in the regimes of the roll-out that the golden and parity tests never enter, and at the batch sizes where a
workgroup comes back for a second and a third group of agents.

Inputs and references: tests/guide_cases.py (what they reach is asserted on the CPU by tests/test_guide_host.py).  Three decoder weight
sets: "cool" (synth's: nothing saturates or clips), "hot" (recurrence x 4, head x 30: accelerations and speeds on their bounds) and "steer"
(hot with the acceleration row x 0.005 and the yaw-rate row x 2: agents keep their speed, slow ones stay under the 0.1 floor of the yaw-rate
bound, and the yaw rate is clipped in each of the bound's three regimes).  Seven loss cases, each term alone and all together.

Bar, over the agents that are not kink-adjacent (guide_cases.kink_adjacent; none in the regime batch), the calibrated one of grad_bar.py:
    max|g - g64| <= 4 max|g32 - g64| + 1e-7 max|g64|
with g32 the same autograd in float32; for the two MFMA forms it evaluates the gates as those kernels document them.  On the cool set the
absolute bars of tests/test_gpu_parity.py hold as well (2e-5 max|g|; 1e-4 max|g| where the gradient runs through positions).  A
kink-adjacent agent's gradient is finite and within 2 max|g64|.

Sizes.  Regime batch: B = 1 and 41 (21 VALU groups, the last half empty; 6 quad groups, the last with one agent; 3 MFMA groups, the last
with nine).  Large batches (hot set, combined case): valu 1,025 (2 passes of 512 workgroups) and 2,051 (3), quad 2,049 (2) and 4,100 (3),
mfma and auto 4,097 (2).  There the references cover whole groups (at most 64 rows: the first two groups -- one for the 16-agent kernel,
whose four groups and one row make 65 --, the last of pass one, the first of pass two, one between, the ragged last): every row finite,
the subset within the bar, the subset bit for bit what the same groups give as a small batch in the same form, and every non-kink row
within 2 x 2e-5 max|g| of another form that splits the rows into passes differently.  The same with Adam over three optimiser steps and
a clip (moments carried by global row, the iterate updated in place), the device noise of the second pass, and the forward-only launch
of the 8-agent kernel on 257 groups.

Worst ratios (error over bar) measured on the MI355X, printed with -s: see MEASURED below.
"""
import numpy as np
import pytest
import torch

import grad_bar
import guide_cases as GC
import noise_replica as R
from cld_amd import synth
from cld_amd.engine import Engine

pytestmark = pytest.mark.gpu

MEASURED = """
Regime cases, error over the calibrated bar, B = 1 / B = 41 per form (valu, mfma, quad):
  cool   target_speed 0.06 / 0.12, 0.27 / 0.20, 0.11 / 0.14; speed_limit - / 0.09, - / 0.17, - / 0.14 (no gradient on the slow first
         agent); acc_limit 0.23 / 0.11, 0.14 / 0.12, 0.13 / 0.11; waypoint 0.21 / 0.11, 0.11 / 0.16, 0.06 / 0.13; target_pos 0.09 / 0.09,
         0.40 / 0.17, 0.37 / 0.11; ext_grad 0.17 / 0.10, 0.22 / 0.23, 0.13 / 0.16; combined 0.10 / 0.15, 0.32 / 0.18, 0.22 / 0.15
  hot    target_speed 0.08 / 0.48, 0.16 / 0.23, 0.10 / 0.45; speed_limit 0.24 / 0.34, 0.22 / 0.39, 0.22 / 0.25; acc_limit 0.28 / 0.48,
         0.37 / 0.35, 0.27 / 0.32; waypoint - / 0.33, - / 0.14, - / 0.17; target_pos 0.04 / 0.31, 0.04 / 0.15, 0.03 / 0.16; ext_grad
         0.17 / 0.17, 0.26 / 0.21, 0.24 / 0.21; combined 0.21 / 0.51, 0.21 / 0.15, 0.15 / 0.09
  steer  target_speed 0.36 / 0.34, 0.29 / 0.24, 0.16 / 0.18; speed_limit - / 0.44, - / 0.22, - / 0.16; acc_limit 0.32 / 0.40, 0.41 / 0.41,
         0.28 / 0.30; waypoint 0.52 / 0.33, 0.14 / 0.30, 0.25 / 0.42; target_pos 0.21 / 0.12, 0.45 / 0.22, 0.29 / 0.32; ext_grad
         0.15 / 0.26, 0.16 / 0.32, 0.16 / 0.23; combined 0.22 / 0.14, 0.15 / 0.68, 0.13 / 0.82
Large batches (hot, combined), subset over the bar: valu 1,025 and 2,051 0.57; quad 2,049 and 4,100 0.16; mfma and auto 4,097 0.35.  Against
the other form, as a fraction of max|g| (bar 4e-5): valu / quad 1.0e-6 at 1,025 and 8.1e-7 at 2,051; quad / mfma 8.4e-7 at 2,049, 4,100
and 4,097.  Device noise in the later passes: 5.3e-6 (valu 1,025), 7.9e-6 (quad 2,049, mfma 4,097) against 1e-4.  Forward-only launch at
2,049 rows against the decoder's kernel: 4.8e-7 on a step that moved the mean by 1.9e-2 (bar 1e-5).  Epilogue: every element within 2 ulp;
the clips took 50 % (SGD) and 79 % (Adam) of the elements.

The roll-out gradient was over the bar wherever the loss reads positions when these tests were written, in all three forms (they share
chain_grad / chain_grad_group), and was changed in two steps (csrc/guide_kernels.hip):
  The running sums of the roll-out (speed, heading, x, y) and the four suffix sums of the backward sweep were carried in float: cool
    target_pos at B = 1 was 1.18 (valu), 1.51 (mfma), 1.38 (quad) times the bar -- 3.6e-12 .. 3.9e-12 off float64 on a gradient of 9e-7,
    where the float32 oracle is 0.6e-12 .. 1.0e-12 off, because torch.cumsum on the CPU carries a float32 sum in float64
    (tests/test_guide_host.py shows the oracle's own arithmetic with float sums at 3.6e-12); steer combined at B = 41 1.36 (mfma), 1.83
    (quad).  Sums in double, read back rounded to float: 0.10 / 0.35 / 0.35 and 1.18 / 0.60.
  TargetPosLoss (softmin over the steps of the squared distance to the waypoint) was evaluated in float: its gradient holds S - dist_t^2, a
    difference of squared distances of hundreds of m^2.  With the sums above in double, cool combined at B = 41 stood at 1.01 (valu), 0.84
    (mfma, quad) and steer combined at 1.18 (mfma); the error was the same 1.1e-7 in all three forms, which differ in everything but
    this code.  Distances, softmin and the factor on e_t in double: 0.15 / 0.18 / 0.15 and 0.68, and the forms now agree with each other
    on the large batches to 8e-7 .. 1e-6 of max|g| instead of 3.6e-6 .. 5.0e-6.
The benchmark's workload (target-speed guidance) takes neither the position path nor the softmin: 823.2 k / 823.7 k step-agent/s before,
824.0 k / 823.1 k after, alternating runs on one device.
"""

_RATIOS = {}
FORMS = ("valu", "mfma", "quad")
COOL_BAR = {"target_speed": 2e-5, "speed_limit": 2e-5, "acc_limit": 2e-5, "waypoint": 1e-4, "target_pos": 1e-4, "ext_grad": 1e-4,
            "combined": 1e-4}
SIGMA = 0.5


@pytest.fixture(scope="module")
def engines():
    out = {}
    unet = synth.make_unet_weights(0)
    for kind in GC.KINDS:
        e = Engine(n_timesteps=10, device="cuda:0")
        e.load_state_dict(unet)
        e.load_state_dict(GC.decoder_weights(kind))
        out[kind] = e.finalize()
    return out


class _forced:
    def __init__(self, e, which, form):
        self.e, self.which, self.form = e, which, form

    def __enter__(self):
        self.e.force_kernel(self.which, self.form)

    def __exit__(self, *exc):
        self.e.force_kernel(self.which, "auto")


def _step(e, form, inp, gd, z=True):
    """One Engine.guidance_step in `form` -> {"mean", "x_next", "grad"} on the CPU."""
    with _forced(e, "guide", form):
        out = e.guidance_step(inp["mean"], inp["cond"], gd, SIGMA, z=inp["z"] if z else None, want_grad=True)
        torch.cuda.synchronize()
    names = ("mean", "x_next", "grad") if z else ("mean", "grad")
    return {k: v.cpu() for k, v in zip(names, out)}


def _check_grad(tag, got, refs, adj, fast, cool_bar=None):
    """got [B,52,4] against the references: the calibrated bar (and the cool set's absolute one) over the agents that are not
    kink-adjacent, the bound on those that are."""
    g64, g32 = refs["f64"], refs["f32fast" if fast else "f32"]
    keep = ~adj
    gmax = float(g64.abs().max())
    assert bool(torch.isfinite(got).all()), (tag, "not finite")
    if bool(adj.any()):
        assert float(got[adj].abs().max()) <= 2 * gmax, (tag, "kink-adjacent agent out of bounds")
    err = float((got[keep].double() - g64[keep]).abs().max())
    print(f"\n[guide] {tag}: max|g - g64| {err:.3g}, max|g32 - g64| {float((g32[keep].double() - g64[keep]).abs().max()):.3g}, "
          f"max|g64| {gmax:.3g}, {int(adj.sum())} kink-adjacent")
    if cool_bar is not None:
        assert err <= cool_bar * gmax, (tag, err / gmax)
    grad_bar.check_all("guide", _RATIOS, tag, {"grad": got[keep]}, {"grad": g64[keep]}, {"grad": g32[keep]})


@pytest.mark.parametrize("B", [1, GC.B_REG])
@pytest.mark.parametrize("case", GC.CASES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", GC.KINDS)
def test_regime_cases_match_fp64(engines, kind, form, case, B):
    """Every case in every form at B = 1 and 41; the worst ratios are in MEASURED."""
    adj, record = GC.regime_kinks(kind, case)
    assert float(adj.double().mean()) <= 0.02 and not bool(adj[0]), record            # the condition test_guide_host.py asserts
    inp = GC.take(GC.inputs(GC.B_REG), range(B))
    got = _step(engines[kind], form, inp, GC.guidance(case, kind, inp))
    refs = {p: g[:B] for p, g in GC.grads(kind, case).items()}
    _check_grad(f"{kind} {case} {form} B={B}", got["grad"], refs, adj[:B], form != "valu", COOL_BAR[case] if kind == "cool" else None)
    # SGD, lr 1, no clip: the guided mean is the mean minus this gradient
    assert float((got["mean"] - (inp["mean"] - got["grad"])).abs().max()) <= 2 * float(np.spacing(np.float32(got["mean"].abs().max())))


def _ulp2(t):
    return 2 * float(np.spacing(np.float32(t.abs().max())))


@pytest.mark.parametrize("form", FORMS)
def test_optimiser_epilogue(engines, form):
    """SGD and Adam's first step, each plain and with a numeric perturb_th, and x_next = guided + sigma z, against the step written out in
    float32 on the gradient the same launch returned: 2 ulp of the result's scale, every element."""
    e, kind = engines["hot"], "hot"
    inp = GC.inputs(GC.B_REG)
    mean, z = inp["mean"], inp["z"]
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    for case, opt, lr in (("combined", "sgd", 0.5), ("combined", "adam", 0.3), ("target_speed", "sgd", 0.5), ("target_speed", "adam", 0.3)):
        g64 = GC.grads(kind, case)["f64"]
        th = float(g64.abs().median()) * lr if opt == "sgd" else 0.5 * lr
        if opt == "sgd" and th == 0.0:
            th = float(g64[g64 != 0].abs().median()) * lr
        # (Adam's first step is +-lr wherever |g| >> 1e-8: with ext_grad in the loss a clip below lr would take every element)
        for clip in ((None,) if (case, opt) == ("combined", "adam") else (None, th)):
            got = _step(e, form, inp, GC.guidance(case, kind, inp, optimizer=opt, lr=lr, perturb_th=clip))
            g = got["grad"]
            delta = -f32(lr) * g if opt == "sgd" else -f32(lr) * g / (g.abs() + f32(1e-8))
            want = mean + delta
            if clip is not None:
                share = float(((want - mean).abs() > clip).float().mean())
                print(f"\n[guide] epilogue {form} {case} {opt}: perturb_th {clip:.3g} clips {100 * share:.1f} % of the elements")
                assert 0.1 <= share <= 0.95, (case, opt, share)
                want = mean + (want - mean).clamp(-f32(clip), f32(clip))
                assert float((got["mean"] - mean).abs().max()) <= clip + _ulp2(mean)
            assert float((got["mean"] - want).abs().max()) <= _ulp2(want), (form, case, opt, clip)
            xn = got["mean"] + f32(SIGMA) * z
            assert float((got["x_next"] - xn).abs().max()) <= _ulp2(xn), (form, case, opt, clip)


def _small_form(form):
    return "mfma" if form == "auto" else form


@pytest.mark.parametrize("form,B,passes,other", GC.BIG_CASES)
def test_grid_stride_passes_sgd(engines, form, B, passes, other):
    """More groups than workgroups: the second and third pass reuse the workgroup's scratch slot and all of its LDS."""
    e, kind, case = engines["hot"], "hot", "combined"
    adj = GC.big_kinks(form, B)[0] | GC.big_kinks(other, B)[0]
    assert float(adj.double().mean()) <= 0.01, "the kink condition of test_guide_host.py does not hold"
    inp = GC.inputs(B)
    rows, groups = GC.big_subset(form, B)
    got = _step(e, form, inp, GC.guidance(case, kind, inp))
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (k, "not finite")
    idx = list(rows)
    _check_grad(f"{kind} {case} {form} B={B} ({len(rows)} rows, groups {groups})", got["grad"][idx], GC.grads(kind, case, B, rows),
                adj[idx], form != "valu")
    sub = GC.take(inp, rows)
    small = _step(e, _small_form(form), sub, GC.guidance(case, kind, sub))
    for k in got:
        assert torch.equal(got[k][idx], small[k]), (k, "rows of the large batch differ from the same groups as a small batch")
    pair = _step(e, other, inp, GC.guidance(case, kind, inp))
    keep = ~adj
    gmax = float(got["grad"][keep].abs().max())
    d = float((got["grad"][keep] - pair["grad"][keep]).abs().max())
    print(f"\n[guide] {form} against {other} at B={B}: max|dg| {d:.3g} = {d / gmax:.3g} max|g| over {int(keep.sum())} rows (bar 4e-5)")
    _RATIOS[f"{form} against {other} B={B}"] = (d / (4e-5 * gmax), "grad")
    assert d <= 2 * 2e-5 * gmax, (form, other, B, d / gmax)
    if bool(adj.any()):
        assert float(got["grad"][adj].abs().max()) <= 2 * float(got["grad"].abs().max())
    if form == "auto":
        forced = _step(e, "mfma", inp, GC.guidance(case, kind, inp))
        for k in got:
            assert torch.equal(got[k], forced[k]), (k, "the automatic choice above 2,048 rows is not the 16-agent kernel")


@pytest.mark.parametrize("form,B,passes,other", GC.BIG_CASES)
def test_grid_stride_passes_adam_three_steps(engines, form, B, passes, other):
    """Adam over three optimiser steps with a clip: the moments are carried by global row, the iterate is read and written in place from
    step 2 on, and the clip is around the first mean."""
    e, kind, case = engines["hot"], "hot", "combined"
    inp = GC.inputs(B)
    rows, _ = GC.big_subset(form, B)
    over = dict(optimizer="adam", lr=0.05, perturb_th=0.08, grad_steps=3)
    got = _step(e, form, inp, GC.guidance(case, kind, inp, **over))
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (k, "not finite")
    moved = (got["mean"] - inp["mean"]).abs()
    assert float(moved.max()) <= 0.08 + _ulp2(inp["mean"]) and float((moved > 0.079).float().mean()) > 0.1      # three steps of 0.05 meet the clip
    sub = GC.take(inp, rows)
    small = _step(e, _small_form(form), sub, GC.guidance(case, kind, sub, **over))
    for k in got:
        assert torch.equal(got[k][list(rows)], small[k]), (k, "rows of the large batch differ from the same groups as a small batch")


@pytest.mark.parametrize("form,B", [("valu", 1025), ("quad", 2049), ("mfma", 4097)])
def test_device_noise_beyond_the_first_pass(engines, form, B):
    inp = GC.inputs(B)
    e = engines["hot"]
    x_t = torch.from_numpy(synth.normal(GC.BIG_SEED, "x_t", (B, 52, 4)))
    with _forced(e, "guide", form):
        out = e.sample_step(x_t, inp["cond"], 5, z=None, guidance=GC.guidance("combined", "hot", inp))
        torch.cuda.synchronize()
    assert not torch.equal(out["mean_guided"], out["mean"])
    z = (out["x_next"].double().cpu() - out["mean_guided"].double().cpu()) / out["sigma"]
    err = float((z - torch.from_numpy(R.step_noise(0, 0, B))).abs().max())
    print(f"\n[guide] device noise {form} B={B}: sigma {out['sigma']:.4f}, max|z - normal4| = {err:.2e}")
    assert err <= 1e-4, (form, B, err)


def _goal(kind, inp):
    """Goals of every branch, placed relative to the plans the float64 decoder gives for the means (as tests/test_gpu_goal.py builds
    them): exact, progress, inside the plan, beyond it, target time passed, none."""
    A = inp["mean"].shape[0]
    end = GC.big_forward64(kind, A)["traj"][:, -1, :2]
    r = torch.arange(A) % 6
    local = torch.zeros(A, 2, dtype=torch.float64)
    time = torch.zeros(A, dtype=torch.int32)
    local[r == 0] = torch.tensor([3.0, 2.5], dtype=torch.float64)
    local[r == 1] = torch.tensor([0.5, 12.0], dtype=torch.float64)
    local[r == 2], time[r == 2] = (end * 0.5 + torch.tensor([1.0, 2.0]))[r == 2], 4 + 30
    local[r == 3], time[r == 3] = (end + torch.tensor([60.0, 5.0]))[r == 3], 4 + 70
    local[r == 4], time[r == 4] = torch.tensor([5.0, 1.0], dtype=torch.float64), 1
    kinds = torch.where(r == 5, 0, torch.where(r < 2, 1, 2)).to(torch.int32)
    return dict(kind=kinds, target_time=time, urgency=torch.where(r == 1, 1.0, 0.5).float(), pref_speed=torch.full((A,), 1.42),
                scale=torch.ones(A), reached=torch.zeros(A, dtype=torch.bool), global_t=4, dt=0.1, min_progress_dist=0.5,
                target_pos=local.float(), agent_from_world=torch.eye(3).repeat(A, 1, 1), num_samp=1)


def test_forward_only_launch_takes_a_second_pass(engines):
    """A goal-guided step at 2,049 rows with the 8-agent kernel forced: run_guidance decodes the iterate with that kernel's forward half,
    257 groups on 256 workgroups (the split into halves is unavailable there and the full kernel follows).  Against the same step with
    the decoder forced, which decodes with the decoder's own kernel: 1e-5 of the mean's scale."""
    B, kind = 2049, "cool"
    e, inp = engines[kind], GC.inputs(B)
    gd = dict(curr_states=inp["curr_states"], goal=_goal(kind, inp), optimizer="sgd", lr=0.5, grad_steps=2)
    with _forced(e, "guide", "quad"):
        auto = e.guidance_step(inp["mean"], inp["cond"], gd, 0.0).clone()
        with _forced(e, "decode", "mfma"):
            forced = e.guidance_step(inp["mean"], inp["cond"], gd, 0.0).clone()
        torch.cuda.synchronize()
    sc = max(1.0, float(inp["mean"].abs().max()))
    moved = (auto.cpu() - inp["mean"]).abs().amax(dim=(1, 2))
    d = float((auto - forced).abs().max())
    print(f"\n[guide] forward-only launch at {B} rows against the decoder's kernel: max|d| = {d:.3e}; the step moved the mean by "
          f"{float(moved.max()):.3e}, the last row by {float(moved[-1]):.3e}")
    assert bool(torch.isfinite(auto).all()) and float(moved.max()) > 3e-4 and float(moved[-1]) > 0
    assert d <= 1e-5 * sc
