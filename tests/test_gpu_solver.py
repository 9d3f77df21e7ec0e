"""GPU tests of the few-step samplers (include/cld_solver.h: cld_solver_step / cld_sample_solver / cld_solver_tables,
csrc/solver_kernels.hip): DDIM(eta) and DPM-Solver++(2M) on a timestep subset, plain, with CFG and with mean-form guidance.

The reference has no few-step sampler, so no recording pins this mode.  Yardstick: tests/solver_yardstick.py -- the definitions of the
header in torch over the pinned oracle -- in float64 on the CPU; the same in float32 calibrates the bar of tests/grad_bar.py, per tensor
    max|got - f64| <= 4 max|f32 - f64| + 1e-7 max|f64|,
and tests/test_solver_host.py shows on the CPU what the cases claim (the two anchors, that the yardstick tells the two kinds apart by
at least 100 x this bar on every step that reads history, clip shares, kink margins).  Single steps, teacher-forced, are the primary
evidence; whole chains confirm the loop: the loop is compared bit for bit with its own steps, and one free chain per kind with the
float64 chain under the bar the float32 chain calibrates.  Elements of an SGD step whose float64 |delta| lies within the bar of the clip
threshold are held to the interval of the clipped and the unclipped alternative (at most 2 % of a case).  -s prints the worst ratio of
every case.

Measured on the MI355X, worst ratio to the bar, exact fp32 / f16x2: single steps (128 cases per mode) 0.70 / 0.43; guided steps before
guidance (x0_hat, mu, grad) 0.50 / 0.36, behind it (mu_guided, x_next) 0.65 / 0.70, next to the clip threshold at most 0.04 % of a case;
teacher-forced chains 0.53 / 0.41; free K = 10 chains 0.35 / 0.27; eta = 1 on the full sequence against the reference's recording 0.38 /
0.30.  The noise prediction of a row alone and in a batch of 37 differs by up to 1.6e-6 in every form of the U-Net.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from cld_amd import _lib, synth
from cld_amd.dm_model import DmModel, solver_timesteps
from cld_amd.engine import Engine
from oracle import cld_oracle as O
from tests import grad_bar
from tests import noise_replica as R
from tests import solver_cases as SC
from tests import solver_yardstick as Y

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
STEP_KEYS = ("x_next", "x0_hat", "mu")


def _engine(n, precision, weights):
    e = Engine(n_timesteps=n, device="cuda:0", precision=precision)
    e.load_state_dict(weights)
    return e.finalize()


@pytest.fixture(scope="module")
def eng(precision):
    return _engine(SC.N_T, precision, SC.all_weights())


@pytest.fixture(scope="module")
def eng10(precision):
    w = dict(synth.make_unet_weights(0, affine_jitter=True))
    w.update(synth.make_decoder_weights(0))
    return _engine(10, precision, w)


def _ratios(tag, got, r64, r32, keys, rows=None):
    """Worst ratio to the bar per tensor, printed; asserts every one <= 1."""
    cut = (lambda v: v) if rows is None else (lambda v: v[:rows])
    worst = {k: grad_bar.ratio(got[k], cut(r64[k]), cut(r32[k])) for k in keys}
    print(f"\n[solver] {tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad)
    return max(worst.values())


def _step_case(eng, kind, eta, lst, cfg, k, B):
    inp = SC.step_inputs()
    x, prev = SC.seen(lst, cfg)[k]
    return eng.solver_step(x[:B], inp["cond"][:B], SC.sampler(kind, eta, SC.STEP_LISTS[lst]), k, x0_prev=None if prev is None else prev[:B],
                           z=inp["z"][:B], non_cond=inp["non_cond"][:B] if cfg else None, guidance_w=SC.GW if cfg else 0.0)


# ------------------------------------------------------------------------------------------------------------- 1. single steps
@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("B", SC.BATCHES)
def test_single_steps_against_float64(eng, B, cfg):
    """99 -> 88, 50 -> 45, 11 -> 0 and 0 -> end; DDIM eta 0 / 0.5 / 1; 2M at a first step, at two middle steps with the history of a
    real preceding step and at a last step."""
    worst = 0.0
    for lst, k in SC.STEP_PAIRS:
        for kind, eta in SC.VARIANTS:
            got = _step_case(eng, kind, eta, lst, cfg, k, B)
            r64, r32 = (SC.step_reference(kind, eta, lst, cfg, k, d) for d in ("f64", "f32"))
            ts = SC.STEP_LISTS[lst]
            worst = max(worst, _ratios(f"B={B} cfg={cfg} {kind} eta={eta} {ts[k]} -> {ts[k + 1] if k + 1 < len(ts) else 'end'}", got, r64, r32, STEP_KEYS, B))
            last = k == len(ts) - 1
            if last or (eta == 0.0):
                assert torch.equal(got["x_next"], got["mu"])                    # no noise: x' is the deterministic part
            if last:
                assert torch.equal(got["x_next"], got["x0_hat"])                # the output step gives the clean prediction itself
            assert torch.equal(got["x0_prev"], got["x0_hat"])                    # the history the next step takes
    print(f"\n[solver] single steps B={B} cfg={cfg}: worst ratio {worst:.3g}")


def test_a_second_order_step_reads_its_history(eng):
    """The 2M middle steps differ from DDIM(0) on the device as the float64 yardstick says they do (>= 100 x the bar), and return the
    history the next step takes."""
    inp = SC.step_inputs()
    for lst, k in SC.HISTORY_STEPS:
        m, d = _step_case(eng, "dpmpp_2m", 0.0, lst, False, k, 5), _step_case(eng, "ddim", 0.0, lst, False, k, 5)
        m64, m32 = (SC.step_reference("dpmpp_2m", 0.0, lst, False, k, p) for p in ("f64", "f32"))
        bar = SC.bar(m64["x_next"][:5], m32["x_next"][:5])
        assert float((m["x_next"] - d["x_next"]).abs().max()) >= 100 * bar, (lst, k)
        assert torch.equal(m["x0_hat"], d["x0_hat"])                            # same (x, eps), same instructions
    x, prev = SC.seen("low", False)[2]
    with pytest.raises(_lib.CldError, match=r"\(-1\).*needs x0_prev"):
        eng.solver_step(x[:5], inp["cond"][:5], SC.sampler("dpmpp_2m", 0.0, SC.STEP_LISTS["low"]), 2)


# ------------------------------------------------------------------------------------------------------------- 2. guided steps
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("name", list(SC.GUIDED))
def test_guided_steps_against_float64(eng, name, optimizer):
    B, loss, cfg = SC.GUIDED[name]
    inp = SC.guided_inputs(name)
    for kind, eta in SC.GUIDE_VARIANTS:
        _, ge = SC.guidance_dicts(name, kind, optimizer)
        for k in (0, 2):                                                        # an intermediate and the output step
            x = SC.guided_x(name, kind, eta, k)
            got = eng.solver_step(x, inp["cond"], SC.sampler(kind, eta, SC.GUIDE_TS), k, z=inp["z"], non_cond=inp["non_cond"] if cfg else None,
                                  guidance_w=SC.GW if cfg else 0.0, guidance=ge, want_grad=True)
            r64, r32 = (SC.guided_reference(name, kind, eta, optimizer, k, d) for d in ("f64", "f32"))
            tag = f"{name} {kind} {optimizer} k={k}"
            _ratios(tag + " (before guidance)", got, r64, r32, ("x0_hat", "mu", "grad"))
            amb, d64 = SC.clip_ambiguous(r64, r32) if k == 0 and optimizer == "sgd" else (torch.zeros(B, 52, 4, dtype=torch.bool), None)
            share = float(amb.double().mean())
            assert share <= 0.02, (tag, share)
            worst = {}
            for key in ("mu_guided", "x_next"):
                g = got[key].cpu().double()
                bar = SC.bar(r64[key], r32[key], ~amb)
                worst[key] = float((g - r64[key]).abs()[~amb].max()) / bar
                if bool(amb.any()):                                             # either side of the clip: the interval of the two alternatives
                    noise = r64["x_next"] - r64["mu_guided"] if key == "x_next" else 0.0
                    alts = (r64["mu"] + torch.sign(d64) * r64["th"] + noise, r64["mu"] + d64 + noise)
                    lo, hi = torch.minimum(*alts) - bar, torch.maximum(*alts) + bar
                    assert bool(((g >= lo) & (g <= hi))[amb].all()), (tag, key)
            print(f"\n[solver] {tag}: " + ", ".join(f"{k_} {v:.3g}" for k_, v in worst.items()) + f"; next to the clip threshold {100 * share:.2f} %")
            assert all(v <= 1.0 for v in worst.values()), (tag, worst)
            if k == 2:
                assert torch.equal(got["x_next"], got["mu_guided"])             # no noise behind the output step
            elif optimizer == "sgd":
                clipped = (got["mu_guided"] - got["mu"]).abs().cpu().double() >= 0.999 * r64["th"]
                assert 0.08 <= float(clipped.double().mean()) <= 0.92           # the clip is effective on the device
            # a step the guidance settings switch off is the unguided step, bit for bit
            if k == 0 and optimizer == "adam":
                off = eng.solver_step(x, inp["cond"], SC.sampler(kind, eta, SC.GUIDE_TS), k, z=inp["z"], non_cond=inp["non_cond"] if cfg else None,
                                      guidance_w=SC.GW if cfg else 0.0, guidance=dict(ge, intermediate=False))
                plain = eng.solver_step(x, inp["cond"], SC.sampler(kind, eta, SC.GUIDE_TS), k, z=inp["z"], non_cond=inp["non_cond"] if cfg else None,
                                        guidance_w=SC.GW if cfg else 0.0)
                assert "mu_guided" not in off and all(torch.equal(off[q], plain[q]) for q in STEP_KEYS) and torch.equal(plain["mu"], got["mu"])


# ------------------------------------------------------------------------------------------------------------- 3. regimes of the kernel
def test_grid_stride_passes_and_row_independence(eng):
    """37 x 52 rows on 2 workgroups are 4 passes, the last one ragged: the bits of the default launch.  A row alone gives the bits it
    has in the batch of 37 -- shown on the kernel itself (cld_debug_solver_kernel) with one and the same noise prediction: the U-Net
    picks the tiling of its launches by the padded batch size, so through the whole step a row alone (16 padded rows) and in the batch
    (48) meet noise predictions that differ in the last bits (measured 1.6e-6; tests/test_gpu_properties.py holds the U-Net to 2e-5
    there, not to bits).  Through the step the same is shown where the U-Net's launches are the same: alone against a batch of 16."""
    lst, k, B = "low", 2, 37
    inp = SC.step_inputs()
    t = SC.STEP_LISTS[lst][k]
    for kind, eta, cfg in (("dpmpp_2m", 0.0, True), ("ddim", 0.5, False)):
        smp = SC.sampler(kind, eta, SC.STEP_LISTS[lst])
        gw = SC.GW if cfg else 0.0
        x, prev = SC.seen(lst, cfg)[k]
        eps = eng.unet_forward(x, inp["cond"], t)
        eu = eng.unet_forward(x, inp["non_cond"], t) if cfg else None
        kernel = lambda rows: eng.debug_solver_kernel(smp, k, x[rows], eps[rows], None if eu is None else eu[rows], gw, x0_prev=prev[rows], z=inp["z"][rows])
        whole, batch = _step_case(eng, kind, eta, lst, cfg, k, B), kernel(slice(0, B))
        try:
            assert eng.solver_grid_cap(2) == 2
            capped, batch_capped = _step_case(eng, kind, eta, lst, cfg, k, B), kernel(slice(0, B))
            torch.cuda.synchronize()
        finally:
            assert eng.solver_grid_cap(0) == 1024
        for key in STEP_KEYS:
            assert torch.equal(capped[key], whole[key]) and torch.equal(batch_capped[key], batch[key]), (kind, key)
            if not cfg:                            # the kernel-only call is the step's own launch: same U-Net launches, same noise prediction
                assert torch.equal(batch[key], whole[key]), (kind, key)
        small = _step_case(eng, kind, eta, lst, cfg, k, 16)
        r64, r32 = (SC.step_reference(kind, eta, lst, cfg, k, d) for d in ("f64", "f32"))
        for b in (0, 17, 36):
            alone = kernel(slice(b, b + 1))
            for key in STEP_KEYS:
                assert torch.equal(alone[key][0], batch[key][b]), (kind, b, key)
            step_alone = eng.solver_step(x[b:b + 1], inp["cond"][b:b + 1], smp, k, x0_prev=prev[b:b + 1], z=inp["z"][b:b + 1],
                                         non_cond=inp["non_cond"][b:b + 1] if cfg else None, guidance_w=gw)
            for key in STEP_KEYS:              # ... and through the whole step within the one-step bar of the row
                assert grad_bar.ratio(step_alone[key], r64[key][b:b + 1], r32[key][b:b + 1]) <= 1.0, (kind, b, key)
        for b in (0, 7, 15):
            step_alone = eng.solver_step(x[b:b + 1], inp["cond"][b:b + 1], smp, k, x0_prev=prev[b:b + 1], z=inp["z"][b:b + 1],
                                         non_cond=inp["non_cond"][b:b + 1] if cfg else None, guidance_w=gw)
            for key in STEP_KEYS:
                assert torch.equal(step_alone[key][0], small[key][b]), (kind, b, key)


# ------------------------------------------------------------------------------------------------------------- 4. the loop is its steps
def _step_through(e, smp, x_T, cond, noise, seed, **kw):
    x, prev, outs = x_T.cuda(), None, []
    for k in range(len(smp["timesteps"])):
        o = e.solver_step(x, cond, smp, k, x0_prev=prev, z=None if noise is None else noise[k], seed=seed, **kw)
        outs.append(o)
        x, prev = o["x_next"], o["x0_prev"]
    return x, outs


@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("B", [5, 37])
def test_loop_equals_its_steps_bit_for_bit(eng, B, cfg):
    inp = SC.step_inputs()
    ts = [99, 70, 40, 11, 0]
    kw = dict(non_cond=inp["non_cond"][:B] if cfg else None, guidance_w=SC.GW if cfg else 0.0)
    noise = torch.from_numpy(synth.normal(SC.SEED, "solver_loop_noise", (5, B, 52, 4))).cuda()
    for kind, eta in (("ddim", 0.0), ("ddim", 1.0), ("dpmpp_2m", 0.0)):
        smp = SC.sampler(kind, eta, ts)
        x0 = eng.sample_solver(inp["x_T"][:B], inp["cond"][:B], smp, noise=noise, **kw)
        assert torch.equal(x0, eng.sample_solver(inp["x_T"][:B], inp["cond"][:B], smp, noise=noise, **kw)) and bool(torch.isfinite(x0).all())
        s0, _ = _step_through(eng, smp, inp["x_T"][:B], inp["cond"][:B], noise, 0, **kw)
        assert torch.equal(x0, s0), (kind, eta, "caller's noise")
        # the on-device generator: the same draw for (seed, step, row, element) in the loop, in the steps and in the numpy replica
        seed = 2 ** 40 + 3
        d0 = eng.sample_solver(inp["x_T"][:B], inp["cond"][:B], smp, noise=None, seed=seed, **kw)
        t0, outs = _step_through(eng, smp, inp["x_T"][:B], inp["cond"][:B], None, seed, **kw)
        assert torch.equal(d0, t0), (kind, eta, "generator")
        if eta == 0.0:
            assert torch.equal(d0, x0)                                          # eta = 0 and 2M draw nothing
            continue
        assert not torch.equal(d0, x0)
        sig = eng.solver_tables(smp)["sigma"]
        for k, o in enumerate(outs[:-1]):
            zgot = (o["x_next"].cpu().double() - o["mu"].cpu().double()) / float(sig[k])
            scale = max(1.0, float(o["mu"].abs().max())) / float(sig[k])
            assert float((zgot - torch.from_numpy(R.step_noise(seed, k, B))).abs().max()) <= 1e-6 * scale + 1e-4, (kind, k)
        assert float(sig[-1]) == 0.0 and torch.equal(outs[-1]["x_next"], outs[-1]["x0_hat"])


def test_guided_loop_equals_its_steps_bit_for_bit(eng):
    name = "ts_b5_cfg"
    B, loss, cfg = SC.GUIDED[name]
    inp = SC.guided_inputs(name)
    noise = torch.from_numpy(synth.normal(SC.SEED, "solver_loop_noise", (3, B, 52, 4))).cuda()
    for kind, eta in SC.GUIDE_VARIANTS:
        _, ge = SC.guidance_dicts(name, kind, "adam")
        smp = SC.sampler(kind, eta, SC.GUIDE_TS)
        kw = dict(non_cond=inp["non_cond"], guidance_w=SC.GW, guidance=ge)
        x0 = eng.sample_solver(inp["x_t"], inp["cond"], smp, noise=noise, **kw)
        s0, outs = _step_through(eng, smp, inp["x_t"], inp["cond"], noise, 0, **kw)
        assert torch.equal(x0, s0) and all("mu_guided" in o for o in outs)
        plain = eng.sample_solver(inp["x_t"], inp["cond"], smp, noise=noise, non_cond=inp["non_cond"], guidance_w=SC.GW)
        assert not torch.equal(plain, x0) and bool(torch.isfinite(x0).all())


# ------------------------------------------------------------------------------------------------------------- 5. chains against float64
@pytest.mark.parametrize("lst", list(SC.STEP_LISTS))
def test_teacher_forced_chains(eng, lst):
    """The float64 chain's own x_t and x0_prev fed step by step: every step of both lists, both kinds, under the one-step bar."""
    for cfg in (False, True):
        for kind in ("ddim", "dpmpp_2m"):
            for k in range(len(SC.STEP_LISTS[lst])):
                got = _step_case(eng, kind, 0.0, lst, cfg, k, 5)
                r64, r32 = (SC.step_reference(kind, 0.0, lst, cfg, k, d) for d in ("f64", "f32"))
                _ratios(f"teacher-forced {lst} cfg={cfg} {kind} k={k}", got, r64, r32, STEP_KEYS, 5)


@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m"])
def test_free_chain_against_float64(eng, kind):
    c = SC.chain_inputs()
    x0 = eng.sample_solver(c["x_T"], c["cond"], {"kind": kind, "steps": SC.CHAIN_K})
    r = grad_bar.ratio(x0, SC.free_chain(kind, "f64"), SC.free_chain(kind, "f32"))
    print(f"\n[solver] free K = {SC.CHAIN_K} chain {kind}: ratio {r:.3g}")
    assert r <= 1.0
    other = SC.free_chain("ddim" if kind == "dpmpp_2m" else "dpmpp_2m", "f64")
    assert float((x0.cpu().double() - other).abs().max()) > 10 * float((x0.cpu().double() - SC.free_chain(kind, "f64")).abs().max())


# ------------------------------------------------------------------------------------------------------------- 6. the eta = 1 anchor
def test_eta_one_on_the_full_sequence_is_the_ancestral_sampler(golden, eng10):
    meta, g = golden("sample_n10_jitter")
    n, B = 10, meta["B"]
    assert B == 8
    nz = synth.make_noise(B, n, meta["noise_seed"])
    x_T, noise = torch.from_numpy(nz["x_T"]), torch.from_numpy(nz["noise"])
    cond = torch.from_numpy(synth.make_inputs(B, meta["in_seed"])["cond_feat"])
    ts = list(range(n - 1, -1, -1))
    wn = synth.make_unet_weights(0, affine_jitter=True)
    got = eng10.sample_solver(x_T, cond, {"kind": "ddim", "timesteps": ts, "eta": 1.0}, noise=noise)
    anc, _, _ = eng10.sample(x_T, cond, noise=noise)
    y64, _ = Y.chain(wn, None, n, "ddim", ts, 1.0, x_T, noise, cond, dtype=F64)
    y32, _ = Y.chain(wn, None, n, "ddim", ts, 1.0, x_T, noise, cond, dtype=F32)
    r_gold = grad_bar.ratio(got, torch.from_numpy(g["pred_traj"]).double(), torch.from_numpy(g["pred_traj"]).double() + (y32.double() - y64))
    r_anc = grad_bar.ratio(got, anc.cpu().double(), anc.cpu().double() + (y32.double() - y64))
    r_y = grad_bar.ratio(got, y64, y32)
    print(f"\n[solver] eta = 1, n = 10: against the reference's recording {r_gold:.3g}, against cld_sample {r_anc:.3g}, against the float64 chain {r_y:.3g}")
    assert r_gold <= 1.0 and r_anc <= 1.0 and r_y <= 1.0
    # the coefficients themselves: the fp32 tables the ancestral sampler reads, to their rounding
    t = eng10.solver_tables({"kind": "ddim", "timesteps": ts, "eta": 1.0})
    idx = np.asarray(ts)
    assert np.allclose(t["a"], eng10.x_t_cof[idx], rtol=1e-6) and np.allclose(-t["b"], eng10.noise_cof[idx], rtol=1e-5)
    assert np.allclose(t["sigma_g"], np.exp(0.5 * eng10.posterior_log_variance_clipped[idx]), rtol=1e-5)


def test_tables_are_the_float64_coefficients_rounded_once(eng):
    for kind, eta, ts in (("ddim", 0.5, SC.STEP_LISTS["low"]), ("ddim", 1.0, SC.STEP_LISTS["top"]), ("dpmpp_2m", 0.0, SC.STEP_LISTS["low"]),
                          ("dpmpp_2m", 0.0, solver_timesteps(100, 20)), ("ddim", 0.0, (50,))):
        got = eng.solver_tables(SC.sampler(kind, eta, ts))
        want = Y.tables(SC.N_T, kind, ts, eta)
        assert got["timesteps"].tolist() == list(ts)
        for col, name in zip(Y.COLS, _lib.SOLVER_TABLE_COLS):
            w32 = want[col].float().numpy()
            # libm and torch may differ in the last bit of log / expm1 in double: one float32 ulp after the rounding
            assert np.all(np.abs(got[name] - w32) <= np.spacing(np.abs(w32))), (kind, col, got[name], w32)


# ------------------------------------------------------------------------------------------------------------- 7. the surface
def _policy(e):
    from cld_amd.policy import CldPolicy
    from cld_amd.vae_model import VaeModel
    return CldPolicy(DmModel(None, None, n_timesteps=e.n_timesteps, engine=e), VaeModel(engine=e))


def test_dm_model_surface(eng):
    B, N = 5, 2
    inp = SC.guided_inputs("ts_b5_cfg")
    dm = DmModel(None, None, n_timesteps=SC.N_T, engine=eng)
    smp = {"kind": "dpmpp_2m", "steps": 10}
    x_T = torch.from_numpy(synth.normal(5, "dm_xT", (B * N, 52, 4)))
    aux = {"cond_feat": inp["cond"].cuda(), "curr_states": inp["curr_states"].cuda()}
    out = dm({"history_positions": torch.zeros(B, 31, 2)}, aux, {"num_samp": N}, noise={"x_T": x_T}, sampler=smp)
    assert out["x1"] is None and out["log_prob_final"] is None and set(out) == {"pred_traj", "x1", "log_prob_final", "aux_info"}
    rep = lambda v: v.repeat_interleave(N, dim=0)
    assert torch.equal(out["pred_traj"], eng.sample_solver(x_T, rep(inp["cond"]), smp))
    # DDIM with eta > 0 takes the caller's [K,BN,52,4] noise
    smp = {"kind": "ddim", "steps": 5, "eta": 1.0}
    nz = torch.from_numpy(synth.normal(6, "dm_noise", (5, B * N, 52, 4)))
    out = dm({"history_positions": torch.zeros(B, 31, 2)}, aux, {"num_samp": N}, noise={"x_T": x_T, "noise": nz}, sampler=smp)
    assert torch.equal(out["pred_traj"], eng.sample_solver(x_T, rep(inp["cond"]), smp, noise=nz))
    with pytest.raises(NotImplementedError, match="guide_clean=True"):
        dm({"history_positions": torch.zeros(B, 31, 2)}, aux, {"num_samp": 1}, sampler=smp, guidance={"guide_clean": True})
    with pytest.raises(NotImplementedError, match="guidance_fn"):
        dm({"history_positions": torch.zeros(B, 31, 2)}, aux, {"num_samp": 1}, sampler=smp, guidance_fn=lambda t: t.sum())


def test_policy_and_closed_loop(eng):
    from cld_amd.policy import closed_loop_rollout
    pol = _policy(eng)
    B, N = 5, 2
    inp = synth.make_inputs(B, 13)
    cond, cs = torch.from_numpy(inp["cond_feat"]).cuda(), torch.from_numpy(inp["curr_states"]).cuda()
    obs = {"cond_feat": cond, "curr_states": cs}
    tgt = synth.uniform(13, "tgt", (B, 52), 0.0, 12.0)
    x_T = torch.from_numpy(synth.normal(7, "pol_xT", (B * N, 52, 4)))
    pol.set_guidance([[{"name": "target_speed", "weight": 1.0, "params": {"target_speed": tgt}, "agents": None}]], torch.zeros(B, dtype=torch.long),
                     lr=0.3, optimizer="adam")
    smp = {"kind": "dpmpp_2m", "steps": 10}
    act_a, info_a = pol.get_action(obs, num_action_samples=N, noise={"x_T": x_T, "noise": torch.zeros(SC.N_T, B * N, 52, 4)})
    act_s, info_s = pol.get_action(obs, num_action_samples=N, noise={"x_T": x_T}, sampler=smp)
    assert set(info_a) == set(info_s) and list(info_a["guide_losses"]) == list(info_s["guide_losses"])
    for k in ("trajectories", "act_idx", "executed_trajectory"):
        assert info_a[k].shape == info_s[k].shape and info_a[k].dtype == info_s[k].dtype, k
    assert act_a.positions.shape == act_s.positions.shape and bool(torch.isfinite(info_s["trajectories"]).all())
    assert not torch.equal(info_a["trajectories"], info_s["trajectories"])
    # the sample selection on the few-step plans is the oracle's
    want = O.choose_action_from_guidance({k: v.cpu() for k, v in info_s["guide_losses"].items()}, [["target_speed"]])
    assert torch.equal(info_s["act_idx"].cpu(), want)
    for gc in (True, "video_diff"):
        with pytest.raises(NotImplementedError, match="sampler= together with guide_clean"):
            pol.get_action(obs, sampler=smp, guide_clean=gc)
    # a 3-step closed loop with a deterministic sampler, bit-identical run to run
    pol.clear_guidance()
    run = lambda: closed_loop_rollout(pol, lambda step, world, cs_: cond, torch.zeros(B, 2), torch.zeros(B), cs, 3,
                                      noise={"x_T": x_T[:B]}, sampler=smp)
    a, b = run(), run()
    assert a.shape == (3, B, 3) and torch.equal(a, b) and bool(torch.isfinite(a).all())
    # ... and it is the sampler that ran: the loop is get_action(sampler=) stepped by hand, and not the ancestral rollout
    world, cs_k, poses = torch.zeros(B, 3, device="cuda:0"), cs, []
    for step in range(3):
        _, info = pol.get_action({"cond_feat": cond, "curr_states": cs_k}, step_index=step, noise={"x_T": x_T[:B]}, sampler=smp)
        world, cs_k = eng.world_step(info["executed_trajectory"].contiguous(), world[:, :2].contiguous(), world[:, 2].contiguous(), 4)
        poses.append(world)
    assert torch.equal(torch.stack(poses), a)
    anc = closed_loop_rollout(pol, lambda step, world, cs_: cond, torch.zeros(B, 2), torch.zeros(B), cs, 3,
                              noise={"x_T": x_T[:B], "noise": torch.zeros(SC.N_T, B, 52, 4)})
    assert anc.shape == a.shape and not torch.equal(anc, a)


def test_refusals(eng):
    inp = SC.guided_inputs("ts_b5_cfg")
    x, cond = inp["x_t"], inp["cond"]
    _, ge = SC.guidance_dicts("ts_b5_cfg", "ddim", "adam")
    lib, B = eng.lib, 5
    ts = np.ascontiguousarray([50, 45, 0], np.int32)
    ws = torch.empty(int(lib.cld_solver_workspace_bytes(eng._h, B, 1)), dtype=torch.uint8, device="cuda:0")
    xg, cg_, out = x.cuda(), cond.cuda(), torch.empty(B, 52, 4, device="cuda:0")
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(sv, guidance=None, nbytes=None, cfg=False):
        return lib.cld_sample_solver(eng._h, C.byref(sv), ptr(xg), None, ptr(cg_), ptr(cg_) if cfg else None, C.c_float(2.0),
                                     None if guidance is None else C.byref(guidance), ptr(out), B, 0, ptr(ws), ws.numel() if nbytes is None else nbytes, None)

    def refused(sv, what, **kw):
        assert call(sv, **kw) == -1
        msg = lib.cld_last_error(eng._h).decode()
        assert what in msg, (what, msg)

    mk = lambda kind, arr, eta, n=None: _lib.CldSolver(kind, len(arr) if n is None else n, arr.ctypes.data, eta)
    refused(mk(0, np.ascontiguousarray([50, 50, 0], np.int32), 0.0), "not strictly decreasing at index 1")
    refused(mk(0, np.ascontiguousarray([100, 0], np.int32), 0.0), "out of range [0, n_timesteps) at index 0")
    refused(mk(0, np.ascontiguousarray([5, -1], np.int32), 0.0), "out of range")
    refused(mk(0, ts, 0.0, n=0), "n_steps < 1")
    refused(mk(0, ts, 1.5), "eta outside [0, 1]")
    refused(mk(0, ts, float("nan")), "eta outside [0, 1]")
    refused(mk(1, ts, 0.5), "deterministic: eta != 0")
    refused(mk(7, ts, 0.0), "unknown solver kind")
    refused(_lib.CldSolver(0, 3, None, 0.0), "null timesteps")
    cg, keep = eng._guidance(dict(ge, guide_clean=True), B)
    refused(mk(0, ts, 0.0), "guide_clean != 0", guidance=cg)
    # the workspace: the sampler's plus the history rows, one byte short is refused, with and without CFG
    for cfg in (0, 1):
        need = int(lib.cld_solver_workspace_bytes(eng._h, B, cfg))
        assert need >= int(lib.cld_workspace_bytes(eng._h, 2 * 16 if cfg else B)) + B * 52 * 4 * 4
        assert call(mk(0, ts, 0.0), nbytes=need - 1, cfg=bool(cfg)) == -3
        assert call(mk(0, ts, 0.0), nbytes=need, cfg=bool(cfg)) == 0
        torch.cuda.synchronize()
    assert lib.cld_solver_workspace_bytes(eng._h, 0, 0) == 0 and lib.cld_solver_workspace_bytes(None, 4, 0) == 0
    # the same causes through the Python layer, and the combinations it refuses itself
    for bad, what in (({"kind": "ddim", "timesteps": [50, 50, 0]}, "not strictly decreasing"), ({"kind": "dpmpp_2m", "steps": 10, "eta": 0.5}, "deterministic"),
                      ({"kind": "ddim", "steps": 10, "eta": 2.0}, "eta outside")):
        with pytest.raises(_lib.CldError, match=what):
            eng.sample_solver(x, cond, bad)
        with pytest.raises(_lib.CldError, match=what):
            eng.solver_tables(bad)
    with pytest.raises(_lib.CldError, match=r"\(-1\).*step index out of range"):
        eng.solver_step(x, cond, {"kind": "ddim", "timesteps": [50, 45, 0]}, 3)
    for g in (dict(ge, guide_clean=True), dict(ge, reconstruction={"params": None})):
        with pytest.raises(NotImplementedError, match="sampler= together with"):
            eng.sample_solver(x, cond, {"kind": "ddim", "steps": 10}, guidance=g)
        with pytest.raises(NotImplementedError, match="sampler= together with"):
            eng.solver_step(x, cond, {"kind": "ddim", "steps": 10}, 0, guidance=g)


def test_the_new_path_leaves_no_state_behind(eng10):
    """cld_sample on the same handle returns the bits it returned before a solver call (plain, CFG and guided, stepwise and looped)."""
    B, n = 8, 10
    nz = synth.make_noise(B, n, 21)
    inp = synth.make_inputs(B, 21)
    x_T, noise, cond = torch.from_numpy(nz["x_T"]), torch.from_numpy(nz["noise"]), torch.from_numpy(inp["cond_feat"])
    cs = torch.from_numpy(inp["curr_states"])
    non_cond = torch.from_numpy(synth.make_inputs(B, 1021)["cond_feat"])
    g = dict(curr_states=cs, target_speed=torch.from_numpy(synth.uniform(21, "tgt", (B, 52), 0.0, 12.0)), lr=None, optimizer="adam")
    before = eng10.sample(x_T, cond, noise=noise)
    before_g = eng10.sample(x_T, cond, noise=noise, non_cond=non_cond, guidance_w=2.0, guidance=g)
    smp = {"kind": "dpmpp_2m", "timesteps": [9, 6, 3, 0]}
    eng10.sample_solver(x_T, cond, smp)
    eng10.sample_solver(x_T, cond, {"kind": "ddim", "steps": 5, "eta": 0.7}, non_cond=non_cond, guidance_w=2.0, guidance=dict(g, output=True), seed=5)
    eng10.solver_step(x_T, cond, smp, 1, x0_prev=x_T)
    after = eng10.sample(x_T, cond, noise=noise)
    after_g = eng10.sample(x_T, cond, noise=noise, non_cond=non_cond, guidance_w=2.0, guidance=g)
    for a, b in zip(before + before_g, after + after_g):
        assert torch.equal(a, b)
