"""GPU tests of the LSTM-VAE training path (cld_vae_encode_train / cld_vae_encode_backward, cld_vae_decode_train / cld_vae_decode_backward,
cld_amd.train.TrainableVae).

Yardstick: autograd of tests/vae_yardstick.py (the reference's LSTMVAE with nn.LSTM's inter-layer dropout as an explicit mask, pinned to
the oracle and to the reference's goldens by tests/test_vae_train_host.py) on the CPU in float64 with the same weights and masks.  The
bar is calibrated by the same autograd in float32, as for the U-Net (tests/test_gpu_train.py): for every one of the 26 tensors, for dx6,
dz and dcond,
    max|g_gpu - g64| <= 4 max|g32 - g64| + 1e-7 max|g64|.
The worst ratios (left side over the bar) are printed with -s.  Batch sizes 1, 5, 16, 17, 33, 301: one row, a ragged 16-row group, one
whole group, a whole group and one row, three groups, and many groups whose weight-gradient K split (at most 256 chunks of whole rows,
train_kernels.hip train_wgrad) has chunks of two rows and a ragged last chunk of one.  Inputs are scaled so that some gates saturate.
In the f16x2 parametrisation the library refuses the training calls, which is asserted; the rest of the module is skipped there.
"""
import numpy as np
import pytest
import torch

import grad_bar
import vae_yardstick as Y
from cld_amd import _lib, synth
from cld_amd.engine import Engine
from oracle import cld_oracle as O

pytestmark = pytest.mark.gpu

W_SEED = 4
SIZES = (1, 5, 16, 17, 33, 301)
_RATIOS = {}


@pytest.fixture(scope="module")
def weights():
    return Y.weights(W_SEED)


@pytest.fixture(scope="module")
def vae(precision, weights):
    if precision != "f32":
        e = Engine(device="cuda:0", precision=precision)
        _, nflat = e.vae_param_table()
        flat = torch.zeros(nflat, device="cuda:0")
        cond = torch.zeros(2, 256, device="cuda:0")
        with pytest.raises(_lib.CldError, match=r"\(-2\).*exact fp32"):
            e.vae_encode_train(flat, torch.zeros(2, 52, 6, device="cuda:0"), cond)
        with pytest.raises(_lib.CldError, match=r"\(-2\).*exact fp32"):
            e.vae_decode_train(flat, torch.zeros(2, 52, 4, device="cuda:0"), cond)
        pytest.skip("training is exact fp32 only: the f16x2 handle refuses it (asserted)")
    from cld_amd.train import TrainableVae
    return TrainableVae(weights, device="cuda:0").eval()


def _inputs(B, seed=11, scale=3.0):
    x6 = torch.from_numpy(synth.normal(seed, "vae_x6", (B, 52, 6))) * scale
    z = torch.from_numpy(synth.normal(seed, "vae_z", (B, 52, 4))) * (2.0 * scale / 3.0)
    cond = torch.from_numpy(synth.make_inputs(B, seed)["cond_feat"]) * (2.0 * scale / 3.0)
    cot = {k: torch.from_numpy(synth.normal(seed, "vae_" + k, (B, 52, n))) for k, n in (("d_mu", 4), ("d_lv", 4), ("d_act", 2))}
    masks = tuple(torch.from_numpy(Y.mask(seed, n, B)) for n in ("vae_mask_enc", "vae_mask_dec"))
    return x6, z, cond, cot, masks


def _ref_grads(weights, x6, z, cond, cot, masks, dtype):
    w = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in weights.items()}
    xx, zz, cc = (a.to(dtype).requires_grad_(True) for a in (x6, z, cond))
    m = [None if a is None else a.to(dtype) for a in masks]
    mu, lv = Y.encode(w, xx, cc, m[0])
    act = Y.decode(w, zz, cc, m[1])
    ((mu * cot["d_mu"].to(dtype)).sum() + (lv * cot["d_lv"].to(dtype)).sum() + (act * cot["d_act"].to(dtype)).sum()).backward()
    g = {k: v.grad for k, v in w.items()}
    g["dx6"], g["dz"], g["dcond"] = xx.grad, zz.grad, cc.grad
    return (mu.detach(), lv.detach(), act.detach()), g


def _gpu_grads(vae, x6, z, cond, cot, masks):
    B = x6.shape[0]
    xg, zg, cg = (a.cuda().requires_grad_(True) for a in (x6, z, cond))
    vae.zero_grad()
    _, mu, lv = vae.traj2z(xg, cg, noise=torch.zeros(B, 52, 4), masks=masks[0])
    act = vae.lstm_dec(zg, cg, mask=masks[1])
    ((mu * cot["d_mu"].cuda()).sum() + (lv * cot["d_lv"].cuda()).sum() + (act * cot["d_act"].cuda()).sum()).backward()
    g = {k: p.grad.detach().cpu() for k, p in vae.named_parameters()}
    g["dx6"], g["dz"], g["dcond"] = xg.grad.cpu(), zg.grad.cpu(), cg.grad.cpu()
    return (mu.detach().cpu(), lv.detach().cpu(), act.detach().cpu()), g


def _check_all(tag, got, g64, g32):
    grad_bar.check_all("vae train", _RATIOS, tag, got, g64, g32)


@pytest.mark.parametrize("masked", [False, True], ids=["eval", "dropout"])
@pytest.mark.parametrize("B", SIZES)
def test_gradients_match_fp64(vae, weights, B, masked):
    x6, z, cond, cot, masks = _inputs(B)
    if not masked:
        masks = (None, None)
    out, got = _gpu_grads(vae, x6, z, cond, cot, masks)
    out64, g64 = _ref_grads(weights, x6, z, cond, cot, masks, torch.float64)
    _, g32 = _ref_grads(weights, x6, z, cond, cot, masks, torch.float32)
    for a, b in zip(out, out64):
        assert float((a.double() - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max()))
    _check_all(f"B={B} {'dropout' if masked else 'eval'}", got, g64, g32)


def test_forward_matches_goldens_and_inference_path(vae, golden):
    """Eval mode on the encoder / decoder fixtures recorded from the reference, with their weights: the existing parity bars (2e-5 for
    the encoder, 5e-6 for act), twice those against cld_traj2z / cld_lstm_decode, and all-ones masks equal NULL bit for bit."""
    from cld_amd.train import TrainableVae
    me, ge = golden("encode")
    md, gd = golden("decode")
    sd = dict(synth.make_encoder_weights(me["w_seed"]))
    sd.update(synth.make_decoder_weights(md["w_seed"]))
    tv = TrainableVae(sd, device="cuda:0").eval()
    vm = tv.to_vae_model()
    B = me["B"]
    fut = synth.make_future(B, me["in_seed"])
    x6s = O.state_to_state_and_action(torch.from_numpy(fut["target_positions"]), torch.from_numpy(fut["target_yaws"]),
                                      torch.from_numpy(fut["curr_speed"]), scaled=True)
    cond = torch.from_numpy(synth.make_inputs(B, me["in_seed"])["cond_feat"])
    nz = torch.from_numpy(synth.normal(me["noise_seed"], "enc_noise", (B, 52, 4)))
    with torch.no_grad():
        z, mu, lv = tv.traj2z(x6s, cond, noise=nz)
        zi, mui, lvi = vm.lstmvae.traj2z(x6s, cond, nz)
        _, mu1, lv1 = tv.traj2z(x6s, cond, noise=nz, masks=torch.ones(B, 52, 64))
    for got, inf, k in ((z, zi, "z"), (mu, mui, "mu"), (lv, lvi, "logvar")):
        assert np.abs(got.cpu().numpy() - ge[k]).max() <= 2e-5, k
        assert float((got - inf).abs().max()) <= 4e-5, k
    assert torch.equal(mu1, mu) and torch.equal(lv1, lv)
    B = md["B"]
    cond = torch.from_numpy(synth.make_inputs(B, md["in_seed"])["cond_feat"])
    zd = torch.from_numpy(synth.normal(md["in_seed"], "dec_z", (B, 52, 4)))
    with torch.no_grad():
        act = tv.lstm_dec(zd, cond)
        act_i = vm.lstmvae.lstm_dec(zd, cond)
        act1 = tv.lstm_dec(zd, cond, mask=torch.ones(B, 52, 64))
    assert np.abs(act.cpu().numpy() - gd["act_small"]).max() <= 5e-6
    assert float((act - act_i).abs().max()) <= 1e-5
    assert torch.equal(act1, act)


def test_compute_vae_loss_chain(vae, weights):
    """compute_vae_loss(...).backward() through encode -> reparametrise -> decode -> loss, with dropout, against the yardstick's step."""
    B, beta = 37, 0.3
    x6, _, cond, _, masks = _inputs(B, seed=7)
    noise = torch.from_numpy(synth.normal(7, "vae_noise", (B, 52, 4)))
    vae.zero_grad()
    xg, cg = x6.cuda(), cond.cuda().requires_grad_(True)
    act, mu, lv = vae(xg, cg, noise=noise, masks=masks)
    loss, recon, kld = vae.compute_vae_loss(xg, act, mu, lv, beta)
    loss.backward()
    got = {k: p.grad.detach().cpu() for k, p in vae.named_parameters()}
    got["dcond"] = cg.grad.cpu()
    ref = {}
    for dt in (torch.float64, torch.float32):
        w = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in weights.items()}
        cc = cond.to(dt).requires_grad_(True)
        lo = Y.step_loss(w, x6.to(dt), cc, noise.to(dt), beta, [m.to(dt) for m in masks])
        lo[0].backward()
        g = {k: v.grad for k, v in w.items()}
        g["dcond"] = cc.grad
        ref[dt] = ([float(v) for v in lo], g)
    for a, b in zip((loss, recon, kld), ref[torch.float64][0]):
        assert abs(float(a) - b) <= 1e-5 * abs(b)
    _check_all("compute_vae_loss", got, ref[torch.float64][1], ref[torch.float32][1])
    lt = vae.to_vae_model().compute_vae_loss(xg, act.detach(), mu.detach(), lv.detach(), beta)
    for a, b in zip((loss, recon, kld), lt):
        assert abs(float(a) - float(b)) <= 1e-6 * abs(float(b))


def test_deterministic_accumulate_and_row_independent(vae):
    B = 100
    x6, z, cond, cot, masks = _inputs(B, seed=13)
    e, flat = vae.engine, vae.flat

    def run(rows, d_params=None, accumulate=False):
        xx, zz, cc = x6[rows].cuda(), z[rows].cuda(), cond[rows].cuda()
        me, md = masks[0][rows].cuda(), masks[1][rows].cuda()
        dp = torch.zeros_like(flat) if d_params is None else d_params
        _, _, tape = e.vae_encode_train(flat, xx, cc, me)
        dx, dce = e.vae_encode_backward(flat, xx, cc, me, tape, cot["d_mu"][rows], cot["d_lv"][rows], d_params=dp, want_dcond=True,
                                        accumulate=accumulate)
        _, tape = e.vae_decode_train(flat, zz, cc, md)
        dz, dcd = e.vae_decode_backward(flat, zz, cc, md, tape, cot["d_act"][rows], d_params=dp, want_dcond=True, accumulate=accumulate)
        return dp, dx.cpu(), dz.cpu(), dce.cpu(), dcd.cpu()

    rows = torch.arange(B)
    a, b = run(rows), run(rows)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    perm = torch.from_numpy(np.random.default_rng(0).permutation(B))
    c = run(perm)
    for p, q in zip(a[1:], c[1:]):
        assert torch.equal(q, p[perm])
    # accumulate = 1 adds to what is there: the sum of the two halves' overwrites, bit for bit
    h0, h1 = rows[:B // 2], rows[B // 2:]
    d0, d1 = run(h0)[0], run(h1)[0]
    dacc = run(h0)[0]
    run(h1, d_params=dacc, accumulate=True)
    assert torch.equal(dacc, d0 + d1)
    # a NULL head cotangent is a zero one
    xx, cc, me = x6.cuda(), cond.cuda(), masks[0].cuda()
    _, _, tape = e.vae_encode_train(flat, xx, cc, me)
    dp_null, dp_zero = torch.zeros_like(flat), torch.zeros_like(flat)
    dx_null, _ = e.vae_encode_backward(flat, xx, cc, me, tape, cot["d_mu"], None, d_params=dp_null)
    dx_zero, _ = e.vae_encode_backward(flat, xx, cc, me, tape, cot["d_mu"], torch.zeros(B, 52, 4), d_params=dp_zero)
    assert torch.equal(dx_null, dx_zero) and torch.equal(dp_null, dp_zero)


def test_adam_steps_then_sampling_path(weights):
    """20 Adam steps (weight decay 1e-5, vae_trainer.py:27-50) of compute_vae_loss on a fixed B = 64 set with fixed masks and noise,
    against the same steps on the yardstick with float64 autograd on the CPU (bar: 1e-4 relative on every step's loss); then the
    sampling path on the updated weights."""
    from cld_amd.train import TrainableVae
    B, steps, lr, wd, beta = 64, 20, 1e-3, 1e-5, 0.3
    tv = TrainableVae(weights, device="cuda:0")
    x6, _, cond, _, masks = _inputs(B, seed=21)
    noise = torch.from_numpy(synth.normal(21, "vae_noise", (B, 52, 4)))
    opt = torch.optim.Adam(tv.parameters(), lr=lr, weight_decay=wd)
    w64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in weights.items()}
    opt64 = torch.optim.Adam(list(w64.values()), lr=lr, weight_decay=wd)
    m64 = [m.double() for m in masks]
    xc, cc, nc, mc = x6.cuda(), cond.cuda(), noise.cuda(), (masks[0].cuda(), masks[1].cuda())
    losses, losses64 = [], []
    for _ in range(steps):
        opt.zero_grad()
        act, mu, lv = tv(xc, cc, noise=nc, masks=mc)
        loss = tv.compute_vae_loss(xc, act, mu, lv, beta)[0]
        loss.backward()
        opt.step()
        losses.append(float(loss))
        opt64.zero_grad()
        l64 = Y.step_loss(w64, x6.double(), cond.double(), noise.double(), beta, m64)[0]
        l64.backward()
        opt64.step()
        losses64.append(float(l64))
    rel = [abs(a - b) / abs(b) for a, b in zip(losses, losses64)]
    print(f"\n[vae train] Adam losses {losses[0]:.6f} -> {losses[-1]:.6f}; worst relative step difference {max(rel):.3g}")
    assert max(rel) <= 1e-4
    assert losses[-1] < losses[0]
    # the sampling path with the updated weights: to_vae_model() against TrainableVae in eval mode
    tv.eval()
    vm = tv.to_vae_model()
    xs, zs, cs, _, _ = _inputs(8, seed=5, scale=1.0)
    nz = torch.from_numpy(synth.normal(5, "vae_noise", (8, 52, 4)))
    with torch.no_grad():
        for a, b in zip(tv.traj2z(xs, cs, noise=nz), vm.lstmvae.traj2z(xs, cs, nz)):
            assert float((a - b).abs().max()) <= 2e-5
        assert float((tv.lstm_dec(zs, cs) - vm.lstmvae.lstm_dec(zs, cs)).abs().max()) <= 2e-5


def test_report_ratios():
    for k, v in _RATIOS.items():
        print(f"[vae train] {k}: {v[0]:.3g} ({v[1]})")
