"""GPU tests of the on-device noise (csrc/cld_kernels.h normal4: splitmix64 -> Box-Muller keyed by (seed, step, row)) at every site that
draws it: head_kernel (one launch per layer; the f16x2 mode), the fused DDPM updates of the tail chains (conv_chain.hip: "chain1" /
"chain4"; chain_wino.hip: "chain" / "chainw"), and the three guidance kernels ("valu", "mfma", "quad").  The yardstick is the numpy
restatement tests/noise_replica.py, whose distribution tests/test_noise_host.py checks.  Every form must draw the same value for
(seed, step, agent, element).

One step: a step call without caller noise (cld_ddpm_step / cld_sample_step with z = NULL: seed 0, step 0) at t = 50 of 100; the draw
recovered as (x_next - mean) / sigma_t is compared with normal4(0, 0, b * 52 + l)[d].  Bar 1e-4 absolute: the float32 rounding of two
O(1) latents over sigma_50 = 0.175 and logf / sincosf in float32 stay near 1e-6, a wrong row, component, step or seed is O(1).
B = 1, 17, 300.

Chains: n_timesteps = 10, sample(noise=None, seed=s) against sample(noise=Z), Z[it, b, l, :] = normal4(s, it, b * 52 + l) in float32,
for s = 7 and s = 2^40 + 3, B = 6 and 70: the plain chain (f32: in every U-Net form), the CFG chain (w = 2) and the target-speed-guided
chain (SGD) with each guidance kernel.  Bar: the chain bar 1e-3 max(1, max|x0|); the same seed through two forms within it as well.

Measured on the MI355X (-s prints them): see MEASURED below.
"""
import pytest
import torch

import noise_replica as R
from cld_amd import synth
from cld_amd.engine import Engine

pytestmark = pytest.mark.gpu

MEASURED = """
one step, max|z - normal4| over B = 1, 17, 300 (bar 1e-4): head kernel (layers; f16x2; every ddpm_step) 9.4e-7, direct tail chain
  (chain1 / chain4) 9.4e-7, Winograd tail chain (chain / chainw) 1.4e-6, guidance kernels valu / mfma / quad 2.4e-6
chains, seeded against the replica's noise, worst over both seeds, B = 6, 70, x0 and x1, both precisions (fraction of the chain bar):
  plain 0.23 (layers, chain1), 0.21 (chain, chainw), 0.38 (chain4), 0.19 (f16x2); cfg 0.25; guided valu 0.28, mfma 0.30, quad 0.26
the same seed through two forms (fraction of the chain bar): U-Net forms 0.72, guidance kernels 0.32
"""

T_MID = 50
SEEDS = (7, 2 ** 40 + 3)
UNET_FORMS = {"f32": ("layers", "chain", "chain1", "chain4", "chainw"), "f16x2": ("auto",)}
GUIDE_FORMS = ("valu", "mfma", "quad")


def _engine(n, precision, jitter):
    e = Engine(n_timesteps=n, device="cuda:0", precision=precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=jitter))
    e.load_state_dict(synth.make_decoder_weights(0))
    return e.finalize()


@pytest.fixture(scope="module")
def eng100(precision):
    return _engine(100, precision, False)


@pytest.fixture(scope="module")
def eng10(precision):
    return _engine(10, precision, True)


def _inputs(B, seed=21):
    inp = synth.make_inputs(B, seed)
    x = torch.from_numpy(synth.normal(seed, "x_t", (B, 52, 4)))
    return x, torch.from_numpy(inp["cond_feat"]), torch.from_numpy(inp["curr_states"])


def _guidance(B, cs, seed=21):
    return {"curr_states": cs, "target_speed": torch.from_numpy(synth.uniform(seed, "tgt", (B, 52), 0.0, 12.0)), "lr": 2000.0,
            "optimizer": "sgd"}


def _check_draw(tag, x_next, centre, sigma, B):
    z = (x_next.double().cpu() - centre.double().cpu()) / sigma
    err = float((z - torch.from_numpy(R.step_noise(0, 0, B))).abs().max())
    print(f"\n[noise] {tag} B={B}: sigma {sigma:.4f}, max|z - normal4| = {err:.2e}, z std {float(z.std()) if B > 1 else float('nan'):.3f}")
    assert err <= 1e-4, (tag, err)


@pytest.mark.parametrize("B", [1, 17, 300])
def test_one_step_draws_the_replica(eng100, precision, B):
    x, cond, _ = _inputs(B)
    for form in UNET_FORMS[precision]:
        eng100.force_kernel("unet", form)
        try:
            xn, mean, sigma = eng100.ddpm_step(x, cond, T_MID, None)                   # always the head kernel
            _check_draw(f"ddpm_step unet={form}", xn, mean, sigma, B)
            out = eng100.sample_step(x, cond, T_MID, z=None)                           # the loop's own step: the tail chains draw themselves
            _check_draw(f"sample_step unet={form}", out["x_next"], out["mean"], out["sigma"], B)
        finally:
            eng100.force_kernel("unet", "auto")


@pytest.mark.parametrize("kernel", GUIDE_FORMS)
@pytest.mark.parametrize("B", [1, 17, 300])
def test_one_guided_step_draws_the_replica(eng100, kernel, B):
    """The guidance kernels add the noise to the guided mean themselves (row b * 52 + (r >> 2), component r & 3)."""
    x, cond, cs = _inputs(B)
    eng100.force_kernel("guide", kernel)
    try:
        out = eng100.sample_step(x, cond, T_MID, z=None, guidance=_guidance(B, cs))
    finally:
        eng100.force_kernel("guide", "auto")
    assert not torch.equal(out["mean_guided"], out["mean"])
    _check_draw(f"guided sample_step guide={kernel}", out["x_next"], out["mean_guided"], out["sigma"], B)


def _chain_pair(e, tag, x_T, cond, seed, **kw):
    """sample(noise=None, seed) against sample(noise=Z of the replica) -> the seeded chain's x0, x1 (on the CPU)."""
    B = x_T.shape[0]
    Z = torch.from_numpy(R.chain_noise(seed, e.loop_steps, B))
    a0, a1, _ = e.sample(x_T, cond, noise=None, seed=seed, **kw)
    b0, b1, _ = e.sample(x_T, cond, noise=Z, **kw)
    a0, a1, b0, b1 = (t.cpu() for t in (a0, a1, b0, b1))
    for name, a, b in (("x0", a0, b0), ("x1", a1, b1)):
        bar = 1e-3 * max(1.0, float(b.abs().max()))
        d = float((a - b).abs().max())
        print(f"\n[noise] chain {tag} seed={seed} B={B} {name}: seeded vs replica noise {d:.3g} over {bar:.3g} = {d / bar:.3g}")
        assert d <= bar, (tag, name, d, bar)
    return a0


def _within_chain_bar(tag, outs):
    forms = list(outs)
    for f in forms[1:]:
        bar = 1e-3 * max(1.0, float(outs[forms[0]].abs().max()))
        d = float((outs[f] - outs[forms[0]]).abs().max())
        print(f"\n[noise] chain {tag}: {f} vs {forms[0]} {d:.3g} over {bar:.3g} = {d / bar:.3g}")
        assert d <= bar, (tag, f, d, bar)


@pytest.mark.parametrize("B", [6, 70])
@pytest.mark.parametrize("seed", SEEDS)
def test_plain_chain_draws_the_replica(eng10, precision, seed, B):
    x_T, cond, _ = _inputs(B, 23)
    outs = {}
    for form in UNET_FORMS[precision]:
        eng10.force_kernel("unet", form)
        try:
            outs[form] = _chain_pair(eng10, f"plain unet={form}", x_T, cond, seed)
        finally:
            eng10.force_kernel("unet", "auto")
    _within_chain_bar(f"plain seed={seed} B={B}", outs)
    other = eng10.sample(x_T, cond, noise=None, seed=seed + 1)[0].cpu()
    assert float((other - outs[UNET_FORMS[precision][0]]).abs().max()) > 1e-3 * max(1.0, float(other.abs().max()))      # the seed is live


@pytest.mark.parametrize("B", [6, 70])
@pytest.mark.parametrize("seed", SEEDS)
def test_cfg_chain_draws_the_replica(eng10, seed, B):
    x_T, cond, _ = _inputs(B, 23)
    non_cond = torch.from_numpy(synth.normal(23, "non_cond_feat", (B, 256)))
    _chain_pair(eng10, "cfg w=2", x_T, cond, seed, non_cond=non_cond, guidance_w=2.0)


@pytest.mark.parametrize("B", [6, 70])
@pytest.mark.parametrize("seed", SEEDS)
def test_guided_chain_draws_the_replica(eng10, seed, B):
    x_T, cond, cs = _inputs(B, 23)
    gd = _guidance(B, cs, 23)
    outs = {}
    for kernel in GUIDE_FORMS:
        eng10.force_kernel("guide", kernel)
        try:
            outs[kernel] = _chain_pair(eng10, f"guided sgd guide={kernel}", x_T, cond, seed, guidance=gd)
        finally:
            eng10.force_kernel("guide", "auto")
    _within_chain_bar(f"guided seed={seed} B={B}", outs)
