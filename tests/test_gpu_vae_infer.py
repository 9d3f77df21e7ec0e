"""GPU tests of the LSTM-VAE inference kernels (csrc/misc_kernels.hip): decode_kernel / decode_mfma_kernel, encode_kernel /
encode_mfma_kernel, rollout_agent / action_to_state_kernel, state_to_state_action_kernel and the two vae_loss kernels, each against the
oracle in float64 on the CPU, kernel form by kernel form, at the batch sizes where the launch logic changes.

Inputs and references: tests/vae_infer_cases.py (what they reach is asserted on the CPU by tests/test_vae_infer_host.py).  Two weight
sets: "cool" (synth's, as every other test uses them: no gate saturates, nothing is clipped) and "hot" (recurrence x 4, output heads
x 30 / x 8: 1 % of the gate pre-activations beyond |4|, a third of the accelerations clipped, the speed on its upper bound).

Bar, per output tensor (dynamics: per channel), the calibrated one of tests/grad_bar.py:
    max|gpu - ref64| <= 4 max|ref32 - ref64| + 1e-7 max|ref64|
with ref32 the same oracle in float32; for the MFMA forms ref32 evaluates the gates as those kernels document them, 1 / (1 + exp(-x))
and 2 / (1 + exp(-2 x)) - 1.  On the cool set the absolute bars of tests/test_gpu_parity.py hold as well (actions 2e-5, trajectories
1e-4, encoder 2e-5).  The LSTM kernels do not depend on CLD_PRECISION_*: the module is not parametrised over `precision`.

Sizes.  Decoder and encoder: forced valu 1, 2, 2049 (the grid is capped at 2048 workgroups: the first one takes a second agent with
the LDS state the first left), forced mfma 1, 15, 16, 17, 33 (tail slots replay the last agent) and 16385 (1024 groups of 16, then a
second pass), auto 255, 256, 257 (the selection boundary).  At 2049 and 16385 the oracle covers a subset of at most 64 rows (the first
rows, the last of the first pass, the first of the second, a few between); every row must be finite, the subset equals the same rows run
as a small batch in the same form bit for bit, and at 2049 the two forms agree on every row within the sum of their bars.  Dynamics:
1, 63, 64, 65, 256 (64-thread blocks).  vae_loss: 1, 255, 256, 257, 513 (the final reduction strides 256 threads over the agents).

Worst ratios (error over bar) measured on the MI355X, printed with -s: see MEASURED below.
"""
import numpy as np
import pytest
import torch

import grad_bar
import vae_infer_cases as VC
from cld_amd.engine import Engine

pytestmark = pytest.mark.gpu

MEASURED = """
decoder (act, traj descaled / scaled), worst of the three per case:
  cool  valu B=1 0.81, B=2 0.86; mfma B=1 0.26, B=15 / 16 / 17 0.23, B=33 0.29; auto B=255 0.49, B=256 / 257 0.26;
        valu B=2049 0.49, mfma B=16385 0.27; valu against mfma at 2049, over the sum of their bars: 0.29
  hot   valu B=1, 2 0.48; mfma B=1 0.37, B=15 / 16 / 17 0.32, B=33 0.38; auto B=255 0.42, B=256 / 257 0.41;
        valu B=2049 0.28, mfma B=16385 0.28; valu against mfma at 2049: 0.18
encoder (z with and without noise, mu, logvar):
  cool  valu B=1 0.75, B=2 0.53; mfma B=1 0.32, B=15 / 16 / 17 0.31, B=33 0.26; auto B=255 0.35, B=256 / 257 0.24;
        valu B=2049 0.43, mfma B=16385 0.26; valu against mfma at 2049: 0.25
  hot   valu B=1 0.32, B=2 0.29; mfma B=1 0.37, B=15 / 16 / 17 / 33 0.33; auto B=255 0.51, B=256 / 257 0.44;
        valu B=2049 0.26, mfma B=16385 0.29; valu against mfma at 2049: 0.65
action_to_state, worst channel: 0.18 .. 0.28 in all 20 cases
state_to_state_and_action, worst channel: 0.21 .. 0.23 at every size, scaled or not (the yaw rate)
vae_loss: B=1 0.51 (kld), B=255 0.17, B=256 0.16, B=257 0.17, B=513 0.20

Two kernels went over the bar when these tests were written, and were changed (csrc/misc_kernels.hip):
  encode_kernel summed each gate's 70 / 128 products in one chain of fmaf: logvar of the single row at B = 1 on the cool set was 10 ulp off
    float64 after 52 steps, 1.41 times the bar (B = 2: 0.999).  Four partial sums per product: 0.75.
  rollout_agent carried its four running sums in float: the state channels of action_to_state were up to 1.99 times the bar (x 1.32,
    y 1.37, v 1.99, yaw 1.34 at B = 256, raw input), because the oracle in float32 does not: torch.cumsum on the CPU carries a float32 sum
    in float64 (tests/test_vae_infer_host.py shows the oracle's own arithmetic with float sums at 1.30 / 1.34 / 1.65 / 1.18).  Sums in
    double: 0.28 at worst.
"""

_RATIOS = {}
KINDS = ("cool", "hot")
LSTM_CASES = [("valu", 1), ("valu", 2), ("mfma", 1), ("mfma", 15), ("mfma", 16), ("mfma", 17), ("mfma", 33),
              ("auto", 255), ("auto", 256), ("auto", 257)]
BIG_CASES = [("valu", 2049, 2048), ("mfma", 16385, 16384)]          # (form, rows, rows of the first grid-stride pass)
DYN_SIZES = (1, 63, 64, 65, 256)
COOL_BARS = {"act": 2e-5, "traj_descaled": 1e-4, "traj_scaled": 1e-4, "z": 2e-5, "mu": 2e-5, "logvar": 2e-5, "z_nonoise": 2e-5}


@pytest.fixture(scope="module")
def engines():
    out = {}
    for kind in KINDS:
        e = Engine(n_timesteps=10, device="cuda:0")
        e.load_state_dict(VC.decoder_weights(kind))
        e.load_state_dict(VC.encoder_weights(kind))
        out[kind] = e.finalize()
    return out


class _forced:
    def __init__(self, e, which, form):
        self.e, self.which, self.form = e, which, form

    def __enter__(self):
        self.e.force_kernel(self.which, self.form)

    def __exit__(self, *exc):
        self.e.force_kernel(self.which, "auto")


def _is_mfma(form, B):
    return form == "mfma" or (form == "auto" and B >= 256)


def _cpu(d):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


def _run_decoder(e, form, z, cond, cs):
    """Every way into the decoder kernel: decode with either output scaling, and lstm_decode (the launch without a trajectory)."""
    with _forced(e, "decode", form):
        td, act = e.decode(z, cond, cs, descaled_output=True, want_act=True)
        ts, act_s = e.decode(z, cond, cs, descaled_output=False, want_act=True)
        act_alone = e.lstm_decode(z, cond)
        out = _cpu({"act": act, "traj_descaled": td, "traj_scaled": ts, "act_s": act_s, "act_alone": act_alone})
    assert torch.equal(out["act"], out.pop("act_s")) and torch.equal(out["act"], out.pop("act_alone"))
    return out


def _run_encoder(e, form, x6, cond, noise):
    with _forced(e, "encode", form):
        z, mu, lv = e.traj2z(x6, cond, noise)
        z0, mu0, lv0 = e.traj2z(x6, cond, None)
        out = _cpu({"z": z, "mu": mu, "logvar": lv, "z_nonoise": z0, "mu0": mu0, "lv0": lv0})
    assert torch.equal(out["mu"], out.pop("mu0")) and torch.equal(out["logvar"], out.pop("lv0"))
    assert torch.equal(out["z_nonoise"], out["mu"])
    return out


RUN = {"decode": (_run_decoder, VC.decoder_inputs, VC.decoder_refs), "encode": (_run_encoder, VC.encoder_inputs, VC.encoder_refs)}


def _check(tag, got, refs, mfma, kind):
    g64 = refs["f64"]
    if kind == "cool":
        for k, v in g64.items():
            err = float((got[k].double() - v).abs().max())
            assert err <= COOL_BARS[k], (tag, k, err)
    grad_bar.check_all("vae infer", _RATIOS, tag, got, g64, refs["f32fast" if mfma else "f32"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form,B", LSTM_CASES)
@pytest.mark.parametrize("which", ["decode", "encode"])
def test_lstm_kernels_match_fp64(engines, which, form, B, kind):
    run, inputs, refs = RUN[which]
    got = run(engines[kind], form, *(a[:B] for a in inputs(VC.NREF)))
    _check(f"{which} {kind} {form} B={B}", got, VC.head_rows(refs(kind), B), _is_mfma(form, B), kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form,B,per_pass", BIG_CASES)
@pytest.mark.parametrize("which", ["decode", "encode"])
def test_second_grid_stride_pass(engines, which, form, B, per_pass, kind):
    """More rows than one pass of the capped grid takes: workgroups come back for a second agent / group of 16."""
    run, inputs, refs = RUN[which]
    e, inp = engines[kind], inputs(B)
    rows = VC.big_subset(B, per_pass)
    got = run(e, form, *inp)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (k, "not finite")
    sub = {k: v[rows] for k, v in got.items()}
    r = refs(kind, B, tuple(rows))
    _check(f"{which} {kind} {form} B={B} ({len(rows)} rows)", sub, r, form == "mfma", kind)
    small = run(e, form, *(a[rows] for a in inp))
    for k in sub:
        assert torch.equal(sub[k], small[k]), (k, "rows of the large batch differ from the same rows as a small batch")
    if B == 2049:
        other = run(e, "mfma", *inp)
        for k, v in r["f64"].items():
            bars = sum(4 * float((r[p][k].double() - v).abs().max()) + 1e-7 * float(v.abs().max()) for p in ("f32", "f32fast"))
            d = float((got[k].double() - other[k].double()).abs().max())
            print(f"\n[vae infer] {which} {kind} B=2049 valu vs mfma {k}: {d:.3g} over {bars:.3g} = {d / bars:.3g}")
            assert d <= bars, (k, d, bars)


@pytest.mark.parametrize("form", ["valu", "mfma"])
@pytest.mark.parametrize("which", ["decode", "encode"])
def test_bit_for_bit_properties(engines, which, form):
    """At B = 100 on the hot set, within one form: the same call twice, the rows permuted, and a few rows on their own."""
    run, inputs, _ = RUN[which]
    e = engines["hot"]
    inp = tuple(a[:100] for a in inputs(VC.NREF))
    a, b = run(e, form, *inp), run(e, form, *inp)
    perm = torch.from_numpy(np.random.RandomState(5).permutation(100))
    p = run(e, form, *(t[perm] for t in inp))
    alone_rows = [0, 15, 16, 47, 99]
    alone = run(e, form, *(t[alone_rows] for t in inp))
    single = run(e, form, *(t[47:48] for t in inp))
    for k in a:
        assert torch.equal(a[k], b[k]), (k, "not deterministic")
        assert torch.equal(a[k][perm], p[k]), (k, "depends on the row order")
        assert torch.equal(a[k][alone_rows], alone[k]) and torch.equal(a[k][47:48], single[k]), (k, "depends on the neighbours")


def _channels(t):
    return {f"ch{k}": t[..., k] for k in range(6)}


@pytest.mark.parametrize("B", DYN_SIZES)
@pytest.mark.parametrize("scaled_input,descaled_output", [(True, True), (True, False), (False, True), (False, False)])
def test_action_to_state_matches_fp64(engines, scaled_input, descaled_output, B):
    act, cs = VC.rollout_input(scaled_input)
    got = engines["cool"].action_to_state(act[:B], cs[:B], scaled_input, descaled_output)
    torch.cuda.synchronize()
    refs = VC.rollout_refs(scaled_input, descaled_output)
    grad_bar.check_all("vae infer", _RATIOS, f"action_to_state scaled_input={scaled_input} descaled_output={descaled_output} B={B}",
                       _channels(got.cpu()), _channels(refs["f64"][:B]), _channels(refs["f32"][:B]))


@pytest.mark.parametrize("B", DYN_SIZES)
@pytest.mark.parametrize("scaled", [False, True])
def test_state_to_state_and_action_matches_fp64(engines, scaled, B):
    pos, yaw, speed = VC.inverse_case()
    got = engines["cool"].state_to_state_and_action(pos[:B], yaw[:B], speed[:B], scaled_output=scaled)
    torch.cuda.synchronize()
    refs = VC.inverse_refs(scaled)
    grad_bar.check_all("vae infer", _RATIOS, f"state_to_state_and_action scaled={scaled} B={B}",
                       _channels(got.cpu()), _channels(refs["f64"][:B]), _channels(refs["f32"][:B]))


@pytest.mark.parametrize("B", VC.VAE_LOSS_SIZES)
def test_vae_loss_matches_fp64(engines, B):
    got = engines["cool"].vae_loss(*VC.vae_loss_case(B), VC.BETA).cpu()
    refs = VC.vae_loss_refs(B)
    print(f"\n[vae infer] vae_loss B={B}: gpu {got.tolist()} ref64 {[float(v) for v in refs['f64'].values()]} "
          f"ref32 {[float(v) for v in refs['f32'].values()]}")
    grad_bar.check_all("vae infer", _RATIOS, f"vae_loss B={B}", dict(zip(("loss", "recon", "kld"), got)), refs["f64"], refs["f32"])
