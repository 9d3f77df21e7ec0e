"""GPU tests of the U-Net training path (cld_unet_train_forward / cld_unet_backward, cld_amd.train).

Yardstick: autograd of the pinned oracle (oracle.cld_oracle.unet_forward / compute_losses / log_prob) on the CPU in float64 with the
same weights.  The bar is calibrated by the same autograd in float32 on the CPU: for every one of the 148 tensors, for dx and for dcond,
    max|g_gpu - g64| <= 4 max|g32 - g64| + 1e-7 max|g64|.
The ratios (left side over the bar) are printed with -s.  Batch sizes 1, 5, 37, 300 and 33: the weight gradients are split over at most
32 row chunks (train_kernels.hip kChunks), so 33 is the first size whose chunks hold two rows and whose last chunk is ragged.  Per-row
timesteps spread over 0..99 with 0 and 99 included.  In the f16x2 parametrisation the library refuses the training calls, which is
asserted; the rest of the module is skipped there.
"""
import numpy as np
import pytest
import torch

import grad_bar
from cld_amd import _lib, synth
from cld_amd.engine import Engine
from oracle import cld_oracle as O

pytestmark = pytest.mark.gpu

W_SEED = 3
SIZES = (1, 5, 33, 37, 300)
_RATIOS = {}


@pytest.fixture(scope="module")
def weights():
    return synth.make_unet_weights(W_SEED, affine_jitter=True)


@pytest.fixture(scope="module")
def dm(precision, weights):
    if precision != "f32":
        e = Engine(n_timesteps=100, device="cuda:0", precision=precision)
        e.load_state_dict(weights).finalize()
        table, nflat = e.unet_param_table()
        flat = torch.zeros(nflat, device="cuda:0")
        x = torch.zeros(2, 52, 4, device="cuda:0")
        with pytest.raises(_lib.CldError, match=r"\(-2\).*exact fp32"):
            e.unet_train_forward(flat, x, torch.zeros(2, 256, device="cuda:0"), torch.zeros(2, dtype=torch.long))
        pytest.skip("training is exact fp32 only: the f16x2 handle refuses it (asserted)")
    from cld_amd.train import TrainableDm
    return TrainableDm(weights, n_timesteps=100, device="cuda:0")


def _inputs(B, seed=11):
    x = torch.from_numpy(synth.normal(seed, "train_x", (B, 52, 4))) * 2.0
    cond = torch.from_numpy(synth.make_inputs(B, seed)["cond_feat"])
    t = torch.from_numpy((np.arange(B) * 37 + 99) % 100).long()
    if B > 1:
        t[0], t[1] = 0, 99
    d_eps = torch.from_numpy(synth.normal(seed, "train_deps", (B, 52, 4)))
    return x, cond, t, d_eps


def _oracle_grads(weights, x, cond, t, d_eps, dtype):
    w = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in weights.items()}
    xx = x.to(dtype).requires_grad_(True)
    cc = cond.to(dtype).requires_grad_(True)
    eps = O.unet_forward(w, xx, cc, t)
    (eps * d_eps.to(dtype)).sum().backward()
    g = {k: v.grad for k, v in w.items()}
    g["dx"], g["dcond"] = xx.grad, cc.grad
    return eps.detach(), g


def _check_all(tag, got, g64, g32):
    grad_bar.check_all("train", _RATIOS, tag, got, g64, g32)


def _gpu_grads(dm, x, cond, t, d_eps):
    xg = x.cuda().requires_grad_(True)
    cg = cond.cuda().requires_grad_(True)
    dm.zero_grad()
    eps = dm.model(xg, {"cond_feat": cg}, t.cuda())
    eps.backward(d_eps.cuda())
    g = {k: p.grad.detach().cpu() for k, p in dm.named_parameters()}
    g["dx"], g["dcond"] = xg.grad.cpu(), cg.grad.cpu()
    return eps.detach().cpu(), g


def test_parameter_table_matches_reference(dm, weights):
    table, nflat = dm.engine.unet_param_table()
    assert [n for n, *_ in table] == list(weights)
    assert sum(n for _, _, n, _ in table) == 4349284
    for (name, off, n, shape) in table:
        assert off % 64 == 0 and tuple(shape) == weights[name].shape and n == weights[name].size
    sd = dm.state_dict()
    assert list(sd) == list(weights)
    for k, v in sd.items():
        assert v.dtype == torch.float32 and torch.equal(v.cpu(), torch.from_numpy(weights[k]))
    # round trip with the dm. prefix (cld_load_weight accepts it)
    dm.load_state_dict({"dm." + k: v * 1.0 for k, v in sd.items()})
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), dm.state_dict().values()))


def test_refusals(dm, weights):
    e = Engine(n_timesteps=100, device="cuda:0").finalize()       # a handle without U-Net weights
    flat = torch.zeros(dm.flat.numel(), device="cuda:0")
    x, cond, t, _ = _inputs(2)
    with pytest.raises(_lib.CldError, match=r"\(-2\)"):
        e.unet_train_forward(flat, x, cond, t)
    lib = _lib.load()
    assert lib.cld_unet_tape_bytes(None, 0) == 0 and lib.cld_unet_train_workspace_bytes(None, 0) == 0
    tape_row = lib.cld_unet_tape_bytes(None, 1)
    assert lib.cld_unet_tape_bytes(None, 64) == 64 * tape_row
    print(f"\n[train] tape bytes per row: {tape_row}")


@pytest.mark.parametrize("B", SIZES)
def test_gradients_match_fp64(dm, weights, B):
    x, cond, t, d_eps = _inputs(B)
    eps, got = _gpu_grads(dm, x, cond, t, d_eps)
    eps64, g64 = _oracle_grads(weights, x, cond, t, d_eps, torch.float64)
    _, g32 = _oracle_grads(weights, x, cond, t, d_eps, torch.float32)
    assert float((eps.double() - eps64).abs().max()) <= 2e-5
    _check_all(f"d_eps cotangent B={B}", got, g64, g32)


def test_forward_matches_inference_path(dm, weights):
    B = 37
    x, cond, t, _ = _inputs(B, seed=5)
    eps_train, _ = dm.engine.unet_train_forward(dm.flat, x, cond, t)
    eps_inf = dm.engine.unet_forward_rows(x, cond, t)
    assert float((eps_train - eps_inf).abs().max()) <= 2e-5


def test_compute_losses(dm, weights):
    B = 37
    x, cond, t, _ = _inputs(B, seed=7)
    noise = torch.from_numpy(synth.normal(7, "train_noise", (B, 52, 4)))
    dm.zero_grad()
    loss = dm.compute_losses({"cond_feat": cond.cuda()}, x.cuda(), t=t.cuda(), noise=noise.cuda())
    loss.backward()
    got = {k: p.grad.detach().cpu() for k, p in dm.named_parameters()}
    sched = O.schedule(100)
    ref = {}
    for dt in (torch.float64, torch.float32):
        w = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in weights.items()}
        lo = O.compute_losses(w, sched, x.to(dt), cond.to(dt), t, noise.to(dt))
        lo.backward()
        ref[dt] = (float(lo), {k: v.grad for k, v in w.items()})
    assert abs(float(loss) - ref[torch.float64][0]) <= 1e-5 * abs(ref[torch.float64][0])
    _check_all("compute_losses", got, ref[torch.float64][1], ref[torch.float32][1])


def test_log_prob(dm, weights):
    B = 37
    x_t, cond, _, _ = _inputs(B, seed=9)
    x_tm1 = x_t * 0.97 + 0.05 * torch.from_numpy(synth.normal(9, "train_xtm1", (B, 52, 4)))
    sched = O.schedule(100)
    dm.zero_grad()
    lp = dm.log_prob(x_t.cuda(), x_tm1.cuda(), {"cond_feat": cond.cuda()}, torch.full((B,), 50))
    lp.mean().backward()
    got = {k: p.grad.detach().cpu() for k, p in dm.named_parameters()}
    ref = {}
    for dt in (torch.float64, torch.float32):
        w = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in weights.items()}
        v = O.log_prob(w, sched, x_t.to(dt), x_tm1.to(dt), cond.to(dt), 50)
        v.mean().backward()
        ref[dt] = (v.detach(), {k: a.grad for k, a in w.items()})
    v64 = ref[torch.float64][0]
    assert float((lp.detach().cpu().double() - v64).abs().max()) <= 1e-4 * max(1.0, float(v64.abs().max()))
    _check_all("log_prob t=50", got, ref[torch.float64][1], ref[torch.float32][1])
    # t = 0: sigma_0 = 1e-10, the value is huge and its gradient is finite (INTEGRATION.md "Training")
    dm.zero_grad()
    lp0 = dm.log_prob(x_t.cuda(), x_tm1.cuda(), {"cond_feat": cond.cuda()}, 0)
    lp0.mean().backward()
    assert torch.isfinite(lp0).all()
    assert all(torch.isfinite(p.grad).all() for p in dm.parameters())


def test_deterministic_and_row_independent(dm):
    B = 96
    x, cond, t, d_eps = _inputs(B, seed=13)
    e = dm.engine
    flat = dm.flat

    def run(xx, cc, tt, dd, d_params=None, accumulate=False):
        dp = torch.zeros_like(flat) if d_params is None else d_params
        eps, tape = e.unet_train_forward(flat, xx, cc, tt)
        dx, dcond = e.unet_backward(flat, xx, cc, tt, tape, dd, d_params=dp, want_dx=True, want_dcond=True, accumulate=accumulate)
        return dp, dx, dcond

    dp1, dx1, dc1 = run(x, cond, t, d_eps)
    dp2, dx2, dc2 = run(x, cond, t, d_eps)
    assert torch.equal(dp1, dp2) and torch.equal(dx1, dx2) and torch.equal(dc1, dc2)
    perm = torch.from_numpy(np.random.default_rng(0).permutation(B))
    _, dx3, dc3 = run(x[perm], cond[perm], t[perm], d_eps[perm])
    assert torch.equal(dx3.cpu(), dx1.cpu()[perm]) and torch.equal(dc3.cpu(), dc1.cpu()[perm])
    # two half batches with accumulate = 1 against the full batch, on the yardstick bar
    h = B // 2
    dpa = torch.zeros_like(flat)
    run(x[:h], cond[:h], t[:h], d_eps[:h], d_params=dpa)
    run(x[h:], cond[h:], t[h:], d_eps[h:], d_params=dpa, accumulate=True)
    _, g64 = _oracle_grads(dm_weights(dm), x, cond, t, d_eps, torch.float64)
    _, g32 = _oracle_grads(dm_weights(dm), x, cond, t, d_eps, torch.float32)
    table, _ = e.unet_param_table()
    got = {n: dpa[off:off + k].view(shape).cpu() for n, off, k, shape in table}
    full = {n: dp1[off:off + k].view(shape).cpu() for n, off, k, shape in table}
    g64 = {k: g64[k] for k in got}
    g32 = {k: g32[k] for k in got}
    _check_all("accumulate over two halves", got, g64, g32)
    _check_all("full batch (same inputs)", full, g64, g32)


def dm_weights(dm):
    return {k: v.cpu().numpy() for k, v in dm.state_dict().items()}


def test_adam_steps_then_sample(dm, weights):
    """20 Adam steps of compute_losses on a fixed B = 64 set against the same steps with fp64 oracle autograd on the CPU, then the
    sampler on the updated weights against oracle.sample."""
    from cld_amd.train import TrainableDm
    B, steps, lr = 64, 20, 1e-3
    tdm = TrainableDm(weights, n_timesteps=100, device="cuda:0")
    z0 = torch.from_numpy(synth.normal(21, "train_z0", (B, 52, 4))) * 1.5
    cond = torch.from_numpy(synth.make_inputs(B, 21)["cond_feat"])
    t = torch.from_numpy(np.random.default_rng(21).integers(0, 100, B)).long()
    noise = torch.from_numpy(synth.normal(21, "train_n", (B, 52, 4)))
    opt = torch.optim.Adam(tdm.parameters(), lr=lr)
    w64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in weights.items()}
    opt64 = torch.optim.Adam(list(w64.values()), lr=lr)
    sched = O.schedule(100)
    losses, losses64 = [], []
    for _ in range(steps):
        opt.zero_grad()
        loss = tdm.compute_losses({"cond_feat": cond.cuda()}, z0.cuda(), t=t.cuda(), noise=noise.cuda())
        loss.backward()
        opt.step()
        losses.append(float(loss))
        opt64.zero_grad()
        l64 = O.compute_losses(w64, sched, z0.double(), cond.double(), t, noise.double())
        l64.backward()
        opt64.step()
        losses64.append(float(l64))
    rel = [abs(a - b) / abs(b) for a, b in zip(losses, losses64)]
    print(f"\n[train] Adam losses {losses[0]:.6f} -> {losses[-1]:.6f}; worst relative step difference {max(rel):.3g}")
    assert max(rel) <= 1e-4
    assert losses[-1] < losses[0]
    # sampling with the updated weights: to_engine() against oracle.sample on the same weights
    n, Bs = 10, 8
    sampler = tdm.to_engine(n_timesteps=n).engine
    nz = synth.make_noise(Bs, n, 5)
    cs = torch.from_numpy(synth.make_inputs(Bs, 5)["cond_feat"])
    x0, _, _ = sampler.sample(torch.from_numpy(nz["x_T"]), cs, noise=torch.from_numpy(nz["noise"]))
    wnew = {k: v.cpu() for k, v in tdm.state_dict().items()}
    ref = O.sample(wnew, O.schedule(n), torch.from_numpy(nz["x_T"]), torch.from_numpy(nz["noise"]), cs)["pred_traj"]
    scale = float(ref.abs().max())
    assert float((x0.cpu() - ref).abs().max()) <= 1e-3 * max(scale, 1.0)


def test_report_ratios():
    for k, v in _RATIOS.items():
        print(f"[train] {k}: {v[0]:.3g} ({v[1]})")
