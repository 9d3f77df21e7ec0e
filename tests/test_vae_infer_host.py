"""CPU tests of tests/vae_infer_cases.py: that the inputs of tests/test_gpu_vae_infer.py reach what they claim to reach, shown with the
float64 oracle alone, and that the bars of that module tell a wrong kernel from a right one.

  * the restated loops (`lstm2` with its gate pre-activations, `unicycle` with its branch shares) equal the oracle bit for bit with their
    switches off, in float32 and float64;
  * hot weight sets: >= 0.5 % of gate pre-activations beyond |4|, >= 10 % of decoded accelerations outside [acce_lo, acce_hi], the
    decoded speed on a bound, logvar spanning a few units either way, and the float32 oracle within 1e-4 of float64 (not chaotic);
  * roll-out case: each of the eight branch shares >= 1 %;
  * inverse case: no raw yaw difference within 1e-3 of an odd multiple of pi, on any row; >= 10 % of steps wrap each way;
  * sensitivity: two gate blocks swapped, the speed clip dropped, v_k for v_{k-1} in the yaw-rate bound -- each at least ten times over
    the calibrated bar 4 max|ref32 - ref64| + 1e-7 max|ref64| of the tensor or channel it shows in.  Measured (times the bar): gate
    blocks i / f swapped 1.7e5 (hot decoder actions), 2.1e5 (hot encoder mu); speed clip dropped 5.7e4 (hot decoder trajectory),
    1.2e6 (roll-out case, speed channel); v_k in the bound 1.2e4 (hot decoder trajectory), 2.0e5 (roll-out case, yaw channel).
"""
import math

import numpy as np
import pytest
import torch

import vae_infer_cases as VC
from oracle import cld_oracle as O


def _bar(ref):
    return 4 * float((ref["f32"].double() - ref["f64"]).abs().max()) + 1e-7 * float(ref["f64"].abs().max())


def _pick(refs, key, sl=None):
    out = {p: refs[p][key] if key is not None else refs[p] for p in ("f64", "f32")}
    return out if sl is None else {p: v[..., sl] for p, v in out.items()}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_restated_loops_equal_the_oracle(dtype):
    z, cond, cs = (a[:33].to(dtype) for a in VC.decoder_inputs(VC.NREF))
    x6, _, nz = (a[:33].to(dtype) for a in VC.encoder_inputs(VC.NREF))
    for kind in ("cool", "hot"):
        wd, we = O.to_torch(VC.decoder_weights(kind), dtype), O.to_torch(VC.encoder_weights(kind), dtype)
        act = VC.lstm_decode(wd, z, cond)
        assert torch.equal(act, O.lstm_decode(wd, z, cond))
        for a, b in zip(VC.traj2z(we, x6, cond, nz), O.traj2z(we, x6, cond, nz)):
            assert torch.equal(a, b)
        for si, do in ((True, True), (True, False), (False, False)):
            assert torch.equal(VC.action_to_state(act, cs, si, do), O.action_to_state_and_action(act, cs, si, do))
    act, cs = (a.to(dtype) for a in VC.rollout_case())
    assert torch.equal(VC.action_to_state(act, cs, True, True), O.action_to_state_and_action(act, cs, True, True))


def test_fast_gate_forms_are_the_same_functions():
    """1 / (1 + exp(-x)) and 2 / (1 + exp(-2 x)) - 1 in float64 against sigmoid and tanh, saturated ends included (exp overflows to inf
    and the quotient to 0, as v_exp_f32 / v_rcp_f32 do)."""
    wd = O.to_torch(VC.decoder_weights("hot"), torch.float64)
    z, cond, _ = (a[:16].double() for a in VC.decoder_inputs(VC.NREF))
    assert float((VC.lstm_decode(wd, z, cond, fast=True) - O.lstm_decode(wd, z, cond)).abs().max()) <= 1e-12
    x = torch.tensor([-200.0, -90.0, 0.0, 90.0, 200.0])
    assert torch.equal(1.0 / (1.0 + torch.exp(-x)), torch.tensor([0.0, 0.0, 0.5, 1.0, 1.0]))
    assert torch.equal(2.0 / (1.0 + torch.exp(-2.0 * x)) - 1.0, torch.tensor([-1.0, -1.0, 0.0, 1.0, 1.0]))


def _gate_shares(w, pre, x, cond):
    taps = []
    VC.lstm2(w, pre, x, cond, taps=taps)
    g = torch.stack(taps).abs()
    return float((g > 4).double().mean()), float((g > 8).double().mean()), float(g.max())


def test_cool_sets_are_cool():
    """What the existing tests run on: nothing near saturation, nothing clipped -- the reason the hot sets exist."""
    z, cond, cs = (a.double() for a in VC.decoder_inputs(VC.NREF))
    _, _, top = _gate_shares(O.to_torch(VC.decoder_weights("cool"), torch.float64), "lstm_dec", z, cond)
    ref = VC.decoder_refs("cool")["f64"]
    a = ref["traj_descaled"][..., 4]
    print(f"\n[vae infer host] cool decoder: largest gate pre-activation {top:.2f}, accelerations in [{float(a.min()):.2f}, {float(a.max()):.2f}]")
    assert top < 4 and float(a.min()) > O.DYN["acce_lo"] and float(a.max()) < O.DYN["acce_hi"]


def test_hot_decoder_saturates_and_clips():
    z, cond, cs = (a.double() for a in VC.decoder_inputs(VC.NREF))
    w = O.to_torch(VC.decoder_weights("hot"), torch.float64)
    s4, s8, top = _gate_shares(w, "lstm_dec", z, cond)
    refs = VC.decoder_refs("hot")
    stats = {}
    VC.action_to_state(refs["f64"]["act"], cs, True, True, stats=stats)
    v = refs["f64"]["traj_descaled"][..., 2]
    clipped = stats["acc_below"] + stats["acc_above"]
    e_act = float((refs["f32"]["act"].double() - refs["f64"]["act"]).abs().max())
    e_traj = float((refs["f32"]["traj_descaled"].double() - refs["f64"]["traj_descaled"]).abs().max())
    print(f"\n[vae infer host] hot decoder: |gate| > 4: {100 * s4:.2f} %, > 8: {100 * s8:.2f} %, max {top:.1f}; accelerations clipped "
          f"{100 * clipped:.1f} %; raw speed above v_hi {100 * stats['v_above']:.1f} %, below v_lo {100 * stats['v_below']:.1f} %; "
          f"fp32 oracle off by {e_act:.2e} (act) {e_traj:.2e} (traj)")
    assert s4 >= 0.005
    assert clipped >= 0.10
    assert float(v.max()) == O.DYN["v_hi"] or float(v.min()) == O.DYN["v_lo"]
    assert e_act <= 1e-4


def test_hot_encoder_saturates_and_spreads_logvar():
    x6, cond, _ = (a.double() for a in VC.encoder_inputs(VC.NREF))
    s4, s8, top = _gate_shares(O.to_torch(VC.encoder_weights("hot"), torch.float64), "lstm_enc", x6, cond)
    refs = VC.encoder_refs("hot")
    mu, lv = refs["f64"]["mu"], refs["f64"]["logvar"]
    e_mu = float((refs["f32"]["mu"].double() - mu).abs().max())
    e_lv = float((refs["f32"]["logvar"].double() - lv).abs().max())
    print(f"\n[vae infer host] hot encoder: |gate| > 4: {100 * s4:.2f} %, > 8: {100 * s8:.2f} %, max {top:.1f}; logvar in "
          f"[{float(lv.min()):.2f}, {float(lv.max()):.2f}], mu in [{float(mu.min()):.2f}, {float(mu.max()):.2f}]; fp32 oracle off by "
          f"{e_mu:.2e} (mu) {e_lv:.2e} (logvar)")
    assert s4 >= 0.005
    assert float(lv.min()) <= -3.0 and float(lv.max()) >= 3.0          # exp(0.5 logvar) spans 0.22 .. 4.5 at the least
    assert e_mu <= 1e-4 and e_lv <= 1e-4


def test_rollout_case_takes_every_branch():
    act, cs = (a.double() for a in VC.rollout_case())
    stats = {}
    VC.action_to_state(act, cs, True, True, stats=stats)
    print("\n[vae infer host] roll-out case: " + ", ".join(f"{k} {100 * v:.1f} %" for k, v in stats.items()))
    assert len(stats) == 8
    for k, v in stats.items():
        assert v >= 0.01, k
    # the unscaled entry is fed the same physical actions
    raw, _ = VC.rollout_input(False)
    assert float((raw.double() - (act * torch.tensor(O.NORM_STD[4:6]) + torch.tensor(O.NORM_MEAN[4:6]))).abs().max()) <= 1e-5


def test_inverse_case_wraps_both_ways_clear_of_the_discontinuity():
    d = VC.inverse_raw_differences()
    _, yaw, _ = VC.inverse_case()
    k = np.round((d / math.pi - 1.0) / 2.0)                     # the nearest odd multiple of pi is (2 k + 1) pi
    margin = np.abs(d - (2.0 * k + 1.0) * math.pi)
    up, down = float((d < -math.pi).mean()), float((d >= math.pi).mean())
    print(f"\n[vae infer host] inverse case: wraps up {100 * up:.1f} %, down {100 * down:.1f} %, smallest margin {margin.min():.2e} "
          f"(per-row minimum >= {margin.min(axis=1).min():.2e}), |yaw| <= {float(yaw.abs().max()):.2f}, |d| <= {np.abs(d).max():.2f}")
    assert (margin.min(axis=1) >= 1e-3).all()                   # every row: nothing is left out of the comparison
    assert up >= 0.10 and down >= 0.10
    assert float(yaw.abs().max()) > math.pi and np.abs(d[:, 1:]).max() < 2 * math.pi
    # and the float32 oracle takes the same fold as float64 everywhere (else its error, and the bar, would be 2 pi / dt)
    r = VC.inverse_refs(False)
    assert float((r["f32"][..., 5].double() - r["f64"][..., 5]).abs().max()) < 1e-2


def test_vae_loss_case_spans_what_it_says():
    x6, act, mu, lv = VC.vae_loss_case(513)
    assert float(lv.min()) < -5.9 and float(lv.max()) > 4.9 and 1.8 < float(mu.std()) < 2.2
    assert 0.8 < float((x6[..., 4:6] - act).pow(2).mean()) < 1.2
    r = VC.vae_loss_refs(513)
    assert all(math.isfinite(float(v)) for v in r["f64"].values())


def test_bars_discriminate_tenfold():
    """Each wrong reference against the right one, over the calibrated bar of the tensor (decoder, encoder) or channel (dynamics)."""
    out = {}
    # two gate blocks swapped
    z, cond, cs = (a.double() for a in VC.decoder_inputs(VC.NREF))
    refs = VC.decoder_refs("hot")
    wd = O.to_torch(VC.decoder_weights("hot"), torch.float64)
    bad = VC.lstm_decode(wd, z, cond, gate_order=(1, 0, 2, 3))
    out["gates swapped, hot decoder act"] = float((bad - refs["f64"]["act"]).abs().max()) / _bar(_pick(refs, "act"))
    x6, cond_e, nz = (a.double() for a in VC.encoder_inputs(VC.NREF))
    erefs = VC.encoder_refs("hot")
    _, bad_mu, _ = VC.traj2z(O.to_torch(VC.encoder_weights("hot"), torch.float64), x6, cond_e, nz, gate_order=(1, 0, 2, 3))
    out["gates swapped, hot encoder mu"] = float((bad_mu - erefs["f64"]["mu"]).abs().max()) / _bar(_pick(erefs, "mu"))
    # the dynamics variants, on the hot decoder's trajectory (whole tensor) and on the roll-out case (per channel)
    act, rcs = (a.double() for a in VC.rollout_case())
    rr = VC.rollout_refs(True, True)
    for name, kw, ch in (("v clip dropped", {"clip_v": False}, 2), ("v_k in the yaw bound", {"bound_on_v_k": True}, 3)):
        bad = VC.action_to_state(refs["f64"]["act"], cs, True, True, **kw)
        out[f"{name}, hot decoder traj"] = float((bad - refs["f64"]["traj_descaled"]).abs().max()) / _bar(_pick(refs, "traj_descaled"))
        bad = VC.action_to_state(act, rcs, True, True, **kw)
        out[f"{name}, roll-out case channel {ch}"] = float((bad[..., ch] - rr["f64"][..., ch]).abs().max()) / _bar(_pick(rr, None, ch))
    for k, v in out.items():
        print(f"\n[vae infer host] {k}: {v:.3g} x the bar")
    for k, v in out.items():
        assert v >= 10.0, (k, v)


def test_float32_oracle_carries_its_running_sums_in_float64():
    """Why rollout_agent carries its four running sums in double: torch.cumsum on the CPU carries a float32 sum in float64 and rounds
    each output once, so the oracle in float32 has none of the rounding that 52 running float32 additions have, and the calibrated
    bar 4 max|ref32 - ref64| + 1e-7 max|ref64| leaves no room for it.  Shown here: its cumsum equals the float64 one rounded, and the
    same roll-out with the sums carried in float32 (`cumsum_f32`) is over the per-channel bar on the state channels: x 1.30, y 1.34,
    v 1.65, yaw 1.18 times the bar -- what the HIP kernel measured at the same 256 rows while it summed in float (1.30, 1.27, 1.65, 1.18)."""
    act, cs = VC.rollout_case()
    x = torch.cat((cs[:, 2:3], act[..., 0]), dim=1)
    assert torch.equal(torch.cumsum(x, 1), torch.cumsum(x.double(), 1).float())
    rr = VC.rollout_refs(True, True)
    seq = VC.action_to_state(act, cs, True, True, cumsum=VC.cumsum_f32)
    ratios = [float((seq[..., k].double() - rr["f64"][..., k]).abs().max()) / _bar(_pick(rr, None, k)) for k in range(4)]
    print("\n[vae infer host] roll-out with float32 running sums over the calibrated bar, channels x y v yaw: "
          + " ".join(f"{r:.2f}" for r in ratios))
