"""GPU tests of the ContextEncoder's ResNet-18 layer by layer and of its passes at the batch sizes the bench runs.

Per layer (cld_debug_context_layer): every layer in every form that exists for it -- the thirteen stride-1 3x3 layers as F(4x4, 3x3)
and the implicit GEMM, the stride-2 3x3 and 1x1/2 layers as the implicit GEMM, the stem fused with its max-pool and as two
launches -- against the float64 reference of oracle.resnet18_layer (conv, BatchNorm from its running statistics, + residual, ReLU; the stem's
max-pool).  The bar is per element: |y - y_ref| <= KAPPA[form] * 2^-24 * E_form with E = |scale| conv(|x|, |w|) + |shift| + |residual| and
E_form = E for the direct forms (the implicit GEMM, both stems) and E's maximum over the element's aligned 4x4 output tile for the Winograd
form: a Winograd tile rounds in the transform domain, and one rounding error reaches all of the
tile's outputs, including those that do not read the value it came from.  A wrong or dropped tap costs |w x| ~ E / (9 C_in) of one
element -- a ratio of ~2^24 / (9 C_in), ~3,600 at 512 input channels, more where the heavy border values sit --, so every KAPPA stays
below a tenth of that (CAP); the max-relative bars of the encoder tests average such an error over 49 pixels and the fc, this one cannot.

Measured on the MI355X (max ratio over the inputs and batch sizes of test_context_layer_vs_fp64, which prints them per layer and form):
  direct 4.7 - 13.4 per layer, 17.9 for the stem (both forms)     -> KAPPA 36
  F(4x4, 3x3) 20.8 - 35.6 (largest at 14x14 / 7x7)                -> KAPPA 72
Against E element by element (no tile maximum) F(4x4, 3x3) reaches 3,500 - 5,000 at 56x56 / 28x28 / 14x14 and 14,400 - 18,500 at 7x7
on the adversarial inputs (x64 border rows next to outputs that do not read them).
"""
import numpy as np
import pytest
import torch

from cld_amd import synth
from cld_amd.engine import CONTEXT_LAYERS

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CAP = 360.0                                                   # a tenth of the ratio one wrong tap of a 512-channel layer produces
KAPPA = {"direct": 36.0, "winograd": 72.0}       # about twice the ratios measured (module docstring)
assert all(k <= CAP for k in KAPPA.values())
NS = (1, 3, 17, 255, 256)                                     # ragged flat tile lists; 256 = the largest pass


def _forms(layer):
    kh, stride = CONTEXT_LAYERS[layer][:2]
    if layer == 0:
        return ["direct", "winograd"]                         # two launches / max-pool fused into the stem (the Winograd form)
    return ["direct", "winograd"] if (kh == 3 and stride == 1) else ["direct"]


def _out_size(layer):
    kh, stride, hin = CONTEXT_LAYERS[layer][:3]
    return 56 if layer == 0 else hin // stride


@pytest.fixture(scope="module")
def eng():
    from cld_amd.engine import Engine
    e = Engine(n_timesteps=10, device="cuda:0")
    e.load_state_dict(synth.make_unet_weights(0))
    e.load_state_dict(synth.make_context_weights(0))
    return e.finalize()


@pytest.fixture(scope="module")
def w64():
    from oracle import cld_oracle as O
    return O.to_torch(synth.make_context_weights(0), dtype=torch.float64)


def _structured_raster(B, g, dev="cuda"):
    """bench.py's raster: 31 history planes, zero but for a +1 agent pixel and six -1 neighbour pixels each, 3 planes of 16x16 0/1 blobs."""
    raster = torch.zeros(B, 34, 224, 224, device=dev)
    px = torch.randint(8, 216, (B, 31, 7, 2), device=dev, generator=g)
    bi = torch.arange(B, device=dev)[:, None, None].expand(B, 31, 7)
    pi = torch.arange(31, device=dev)[None, :, None].expand(B, 31, 7)
    val = torch.full((B, 31, 7), -1.0, device=dev)
    val[:, :, 0] = 1.0
    raster[bi, pi, px[..., 1], px[..., 0]] = val
    sem = (torch.rand(B, 3, 14, 14, device=dev, generator=g) > 0.5).float()
    raster[:, 31:] = sem.repeat_interleave(16, dim=2).repeat_interleave(16, dim=3)
    return raster


@pytest.fixture(scope="module")
def real(w64):
    """The oracle's own activations of three rasters (dense, sparse, bench-structured): calls[layer] = (x, residual, relu, y) in float64 NCHW."""
    from oracle import cld_oracle as O
    g = torch.Generator(device="cpu").manual_seed(3)
    img = torch.cat([torch.from_numpy(synth.make_raster(1, 21, dense=True)), torch.from_numpy(synth.make_raster(1, 22, dense=False)),
                     _structured_raster(1, g, dev="cpu")])
    calls, _ = O.resnet18_by_layers(w64, img)
    return calls


RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if RATIOS:
        print("\nmax |y - y_ref| / (2^-24 E) per layer and form:")
        for (layer, form), r in sorted(RATIOS.items()):
            print(f"  layer {layer:2d} {form:12s} {r:8.3f}")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _ratio(y, ref, e):
    """max over elements of |y - ref| / (2^-24 E); y on the device (NHWC, float32) or host, ref / E float64 NCHW on the host."""
    y = y.cpu().double()
    if y.shape[1:] != ref.shape[1:]:
        y = y.permute(0, 3, 1, 2)
    err = (y - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / (U * e))
    return float(r.max())


def _record(layer, form, r):
    RATIOS[(layer, form)] = max(RATIOS.get((layer, form), 0.0), r)


def _run(eng, form, layer, x, res, relu):
    try:
        eng.force_kernel("context", form)
        return eng.debug_context_layer(layer, x, res, relu)
    finally:
        eng.force_kernel("context", "auto")


def _agents(n, layer, rng):
    """The agents whose fp64 reference is computed: all of them up to 17; above that the first and last two, every agent of the last
    workgroup of the F(4x4) tile list (16 tiles: the ragged tail), six random neighbouring pairs (at these tile
    counts every pair of neighbours shares or borders a workgroup) and four random agents.  The reference is per agent, so exact."""
    if n <= 17:
        return list(range(n))
    ho = _out_size(layer)
    sel = {0, 1, n - 2, n - 1}
    tpa, wg = ((ho + 3) // 4) ** 2, 16
    sel |= set(range(((n * tpa - 1) // wg * wg) // tpa, n))
    for a in rng.choice(n - 1, 6, replace=False):
        sel |= {int(a), int(a) + 1}
    sel |= {int(a) for a in rng.choice(n, 4, replace=False)}
    return sorted(sel)


def _adversarial(layer, n, seed):
    """Signed U(-1, 1), each agent scaled by its own power of two (neighbours differ by 2^5 mod 2^9: a read of the wrong agent shows), the
    first and last map row and column x64 (where the masked and hanging tiles read); NHWC for the convolutions, NCHW images for the stem."""
    kh, stride, hin, cin, cout = CONTEXT_LAYERS[layer]
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (n, cin, hin, hin) if layer == 0 else (n, hin, hin, cin)
    x = torch.rand(shape, device="cuda", generator=g) * 2 - 1
    x *= torch.exp2((torch.arange(n, device="cuda") * 5 % 9 - 4).float()).view(n, 1, 1, 1)
    if layer == 0:
        x[:, :, 0] *= 64; x[:, :, -1] *= 64; x[:, :, :, 0] *= 64; x[:, :, :, -1] *= 64
    else:
        x[:, 0] *= 64; x[:, -1] *= 64; x[:, :, 0] *= 64; x[:, :, -1] *= 64
    return x


TILE = {"direct": 1, "winograd": 4}         # output tile of the form: the reach of one rounding error


def _tile_max(e, t):
    """E maximised over the aligned t x t output tiles (t = 1: E itself), broadcast back to every element of the tile."""
    if t == 1:
        return e
    h = e.shape[-1]
    m = torch.nn.functional.max_pool2d(e, t, t, ceil_mode=True)
    return m.repeat_interleave(t, dim=2).repeat_interleave(t, dim=3)[..., :h, :h]


def _check(layer, form, y, ref, e, what, fails):
    """Record the element-wise ratio and the ratio against E over the form's output tile; the latter is held to KAPPA[form]; plus the
    max-relative bar of the encoder tests."""
    _record(layer, form + "/elem", _ratio(y, ref, e))
    kind = "direct" if layer == 0 else form                   # both stems are direct convolutions
    r = _ratio(y, ref, _tile_max(e, TILE[kind]))
    _record(layer, form, r)
    if r > KAPPA[kind]:
        fails.append((layer, form, what, r))
    yd = y.cpu().double()
    if float((yd.permute(0, 3, 1, 2) - ref).abs().max()) > 1e-4 * float(ref.abs().max()):
        fails.append((layer, form, what, "max-relative"))


@pytest.mark.parametrize("layer", range(20))
def test_context_layer_vs_fp64(eng, w64, real, layer):
    """One layer, every form, against float64 per element: the oracle's activations of three rasters (non-negative, as in the network,
    with the network's residual and ReLU), then signed adversarial tensors for n = 1, 3, 17, 255, 256 without residual + ReLU and with a
    signed residual and no ReLU.  Besides the per-element bar, the max-relative bar of the encoder tests (1e-4 of max|y_ref|)."""
    from oracle import cld_oracle as O
    forms = _forms(layer)
    rng = np.random.default_rng(100 + layer)
    fails = []
    x, res, relu, _ = real[layer]
    x = x.float().double()                                    # the reference of the fp32 values the kernels read
    res = None if res is None else res.float().double()
    ref, e = O.resnet18_layer(w64, layer, x, res, relu, want_bound=True)
    xin = x.float().cuda() if layer == 0 else _nhwc(x.float()).cuda()
    rin = None if res is None else _nhwc(res.float()).cuda()
    for form in forms:
        _check(layer, form, _run(eng, form, layer, xin, rin, relu), ref, e, "real", fails)
    cout, ho = CONTEXT_LAYERS[layer][4], _out_size(layer)
    for n in NS:
        x = _adversarial(layer, n, 1000 * layer + n)
        g = torch.Generator(device="cuda").manual_seed(7 + n)
        rsd = (torch.rand(n, ho, ho, cout, device="cuda", generator=g) * 2 - 1) * 4.0
        sel = _agents(n, layer, rng)
        xs = x[sel].cpu().double()
        xs = xs if layer == 0 else xs.permute(0, 3, 1, 2)
        if layer == 0:
            variants = [(None, True)]
            z, e0 = O.resnet18_layer(w64, 0, xs, want_bound=True)
        else:
            variants = [(None, True), (rsd, False)]
            z, e0 = O.resnet18_layer(w64, layer, xs, relu=False, want_bound=True)      # pre-activation: both variants from one conv
        for rv, rl in variants:
            if layer == 0:
                ref, e = z, e0
            elif rv is None:
                ref, e = torch.relu(z), e0
            else:
                rs = rv[sel].cpu().double().permute(0, 3, 1, 2)
                ref, e = z + rs, e0 + rs.abs()
            for form in forms:
                _check(layer, form, _run(eng, form, layer, x, rv, rl)[sel], ref, e, (n, "residual" if rv is not None else "relu"), fails)
    print(f"layer {layer}: " + ", ".join(f"{f} {RATIOS[(layer, f)]:.2f} (element-wise {RATIOS[(layer, f + '/elem')]:.1f})" for f in forms))
    assert not fails, fails


def _one_hot_rasters():
    """Single +-1 pixels in the 31 history planes, one per plane, at: every image border (rows / columns 0..3, 220..223) against the
    column-block boundaries; both sides of every stem strip boundary (a strip of two output rows reads input rows 4 k - 3 .. 4 k + 5: rows
    4 k - 4 .. 4 k + 6 for every k); both sides of where one 16-column output block's receptive field ends and the next one's begins
    (block cb reads input columns 32 cb - 3 .. 32 cb + 33, context_kernels.hip).  -> [n,34,224,224] float32, one pattern per agent."""
    rng = np.random.default_rng(5)
    border = [0, 1, 2, 3, 220, 221, 222, 223]
    cblk = sorted({c for cb in range(7) for c in (32 * cb - 4, 32 * cb - 3, 32 * cb - 2, 32 * cb + 32, 32 * cb + 33, 32 * cb + 34)
                   if 0 <= c < 224})
    cols = sorted(set(border + cblk))
    pix = [(r, c) for r in border for c in cols]                                   # border rows x every column of interest
    pix += [(r, c) for c in border for r in rng.choice(224, 6, replace=False)]    # border columns
    strip_rows = sorted({r for k in range(57) for r in range(4 * k - 4, 4 * k + 7) if 0 <= r < 224})
    pix += [(r, cols[i % len(cols)]) for i, r in enumerate(strip_rows)]           # every strip boundary
    pix += [(int(rng.integers(224)), c) for c in cblk]                             # column blocks at an interior row
    n = (len(pix) + 30) // 31
    img = np.zeros((n, 34, 224, 224), np.float32)
    order = rng.permutation(len(pix))
    for k, i in enumerate(order):
        a, p = divmod(k, 31)
        img[a, p, pix[i][0], pix[i][1]] = 1.0 if rng.random() < 0.5 else -1.0
    return torch.from_numpy(img)


def test_context_stem_on_one_hot_sparse_rasters(eng, w64):
    """The stem's zero-strip shortcut (per plane and strip a 7-bit mask of the output column blocks that see a non-zero value, and the
    sparse-plane path that runs only those) where a strip or a column block touches the image edge or its neighbour: the fused and the
    two-launch stem against the float64 conv -> bn -> relu -> maxpool, per element, every agent."""
    from oracle import cld_oracle as O
    img = _one_hot_rasters()
    ref, e = O.resnet18_layer(w64, 0, img, want_bound=True)
    x = img.cuda()
    for form in ("direct", "winograd"):
        y = _run(eng, form, 0, x, None, True)
        r = _ratio(y, ref, e)
        _record(0, form + "/1hot", r)
        print(f"stem one-hot ({img.shape[0]} agents) {form}: max ratio {r:.3f}")
        assert r <= KAPPA["direct"], (form, r)


# ---------------------------------------------------------------------------------------------------------
# passes at the sizes the bench runs
# ---------------------------------------------------------------------------------------------------------
K = 17


@pytest.fixture(scope="module")
def k_agents(eng):
    """K distinct agents: 9 bench-structured rasters, 8 dense ones; their cond_feat / map_feat as one K-agent batch (one pass) in the default
    and the direct form, held to the oracle's bars (1e-4 of max|map_feat|, 1e-4 abs on cond_feat)."""
    from oracle import cld_oracle as O
    g = torch.Generator(device="cuda").manual_seed(17)
    img = torch.cat([_structured_raster(9, g), torch.from_numpy(synth.make_raster(K - 9, 29, dense=True)).cuda()])
    cs = torch.from_numpy(synth.make_inputs(K, 29)["curr_states"]).cuda()
    out = {}
    for form in ("auto", "direct"):
        try:
            eng.force_kernel("context", form)
            c, m = eng.context_encode(img, cs, want_map_feat=True)
        finally:
            eng.force_kernel("context", "auto")
        out[form] = (c.clone(), m.clone())
    taps = {}
    ref = O.context_encode(O.to_torch(synth.make_context_weights(0)), img.cpu(), cs.cpu(), taps)
    scale = float(taps["map_feat"].abs().max())
    for form, (c, m) in out.items():
        assert float((m.cpu() - taps["map_feat"]).abs().max()) <= 1e-4 * scale, form
        assert float((c.cpu() - ref).abs().max()) <= 1e-4, form
    return img, cs, out


def _pass_starts(eng, B, form):
    p = eng.lib.cld_debug_context_pass_size(B) if form != "direct" else min(B, 256)      # the direct form runs passes of 256 (include/cld.h)
    return list(range(0, B, p)), p


def _batch_rows(B, starts, rng):
    """B picks of the K agents: a random walk (no two neighbouring rows alike, no period), and around every pass boundary the rows
    b0 - 2 .. b0 + 1 four distinct agents, different from the rows outside them: a row offset by one lands on a different agent."""
    idx = np.cumsum(rng.integers(1, K, B)) % K
    for b0 in starts[1:] + [B]:
        lo, hi = max(b0 - 2, 0), min(b0 + 2, B)
        ban = {int(idx[lo - 1])} if lo > 0 else set()
        if hi < B:
            ban.add(int(idx[hi]))
        idx[lo:hi] = rng.choice([k for k in range(K) if k not in ban], hi - lo, replace=False)
    assert (idx[1:] != idx[:-1]).all()
    return torch.from_numpy(idx).cuda()


@pytest.mark.parametrize("B,form", [(511, "auto"), (511, "direct"), (1024, "auto"), (4096, "auto")])
def test_context_passes_at_bench_sizes(eng, k_agents, B, form):
    """B agents drawn from K = 17 distinct ones (bench-structured and dense rasters) cross every pass boundary cld_debug_context_pass_size
    gives: every row of cond_feat and map_feat is bit-identical to that agent's row of the K-agent batch (the 4,096 case holds a 28 GB
    raster, as bench configs[4] does)."""
    img, cs, out = k_agents
    starts, p = _pass_starts(eng, B, form)
    assert p == B if B <= 256 else 128 <= p <= 256
    print(f"B = {B} ({form}): passes of {p}, starts {starts}")
    idx = _batch_rows(B, starts, np.random.default_rng(B))
    big = img[idx]
    try:
        eng.force_kernel("context", form)
        c, m = eng.context_encode(big, cs[idx], want_map_feat=True)
    finally:
        eng.force_kernel("context", "auto")
        del big
        torch.cuda.empty_cache()
    c0, m0 = out[form]
    bad = (~(c == c0[idx]).all(dim=1) | ~(m == m0[idx]).all(dim=1)).nonzero().flatten().tolist()
    assert not bad, f"{len(bad)} rows differ, first {bad[:8]}"


# ---------------------------------------------------------------------------------------------------------
# configs[4]: the timed loop with its encoder and reward stages
# ---------------------------------------------------------------------------------------------------------
def test_configs4_closed_loop_with_encoder_and_reward(precision):
    """Sibling of test_configs4_closed_loop_at_per_gpu_size with the two stages bench.py times inside configs[4]'s loop: 4,096 agents,
    2 sim steps, 50 denoising steps, cond_feat = context_encode(bench-structured raster, curr_states) at every sim step and the PPO reward of
    every plan (drivable map, raster transform, 8 neighbours per agent).  At each sim step 40 rows spanning every pass: cond_feat is
    bit-identical to context_encode of those rows alone on the same curr_states, and reward / offroad / collision on the big batch's own plans
    equal the oracle's (flags exact, reward to the reward golden's 1e-5)."""
    from cld_amd.dm_model import DmModel
    from cld_amd.engine import Engine
    from cld_amd.policy import CldPolicy, closed_loop_rollout
    from cld_amd.vae_model import VaeModel
    from oracle import cld_oracle as O
    n, B, S = 50, 4096, 2
    e = Engine(n_timesteps=n, device="cuda:0", precision=precision)
    for sd in (synth.make_unet_weights(0, affine_jitter=True), synth.make_decoder_weights(0), synth.make_encoder_weights(0),
               synth.make_context_weights(0)):
        e.load_state_dict(sd)
    e.finalize()
    pol = CldPolicy(DmModel(None, None, n_timesteps=n, engine=e), VaeModel(engine=e))
    g = torch.Generator(device="cuda").manual_seed(45)
    raster = _structured_raster(B, g)
    xT = torch.randn(B, 52, 4, device="cuda", generator=g)
    nz = torch.randn(n, B, 52, 4, device="cuda", generator=g)
    cs = torch.zeros(B, 4, device="cuda"); cs[:, 2] = torch.rand(B, device="cuda", generator=g) * 15.0
    ctr = torch.randn(B, 2, device="cuda", generator=g) * 100.0
    yaw = (torch.rand(B, device="cuda", generator=g) - 0.5) * 6.0
    dmap = (torch.rand(B, 28, 28, device="cuda", generator=g) > 0.2).repeat_interleave(8, dim=1).repeat_interleave(8, dim=2).to(torch.uint8)
    rfa = torch.tensor([[2.0, 0.0, 56.0], [0.0, 2.0, 112.0], [0.0, 0.0, 1.0]], device="cuda").expand(B, 3, 3).contiguous()
    opos = torch.randn(B, 8, 52, 2, device="cuda", generator=g) * 20.0
    oav = (torch.rand(B, 8, 52, device="cuda", generator=g) > 0.1).to(torch.uint8)
    conds, states, plans = [], [], []

    def cond_fn(s, wld, c):
        conds.append(e.context_encode(raster, c))
        states.append(c)
        return conds[-1]

    def gather(traj):
        plans.append(traj)
        return traj
    try:
        closed_loop_rollout(pol, cond_fn, ctr, yaw, cs, n_sim_steps=S, gather=gather, noise={"x_T": xT, "noise": nz})
        starts, p = _pass_starts(e, B, "auto")
        rows = sorted({r for b0 in starts for r in (b0, min(b0 + p, B) - 1)})
        rows += [int(r) for r in np.random.default_rng(4).choice(sorted(set(range(B)) - set(rows)), 40 - len(rows), replace=False)]
        assert len(rows) == 40
        idx = torch.tensor(sorted(rows), device="cuda")
        for s in range(S):
            small = e.context_encode(raster[idx], states[s][idx].contiguous())
            assert torch.equal(small, conds[s][idx]), s
            traj = plans[s]
            sa = e.state_to_state_and_action(traj[..., :2].contiguous(), traj[..., 3:4].contiguous(), states[s][:, 2].contiguous(),
                                             scaled_output=True)
            r, off, col = e.compute_reward(traj, sa, rfa, dmap, opos, oav)
            rr, ro, rc = O.compute_reward(traj[idx].cpu(), sa[idx].cpu(), rfa[idx].cpu(), dmap[idx].cpu(), opos[idx].cpu(), oav[idx].cpu())
            assert torch.equal(off[idx].cpu(), ro) and torch.equal(col[idx].cpu(), rc), s
            assert float((r[idx].cpu() - rr).abs().max()) <= 1e-5 * max(1.0, float(rr.abs().max())), s
            assert bool(torch.isfinite(r).all())
    finally:
        del raster
        torch.cuda.empty_cache()
