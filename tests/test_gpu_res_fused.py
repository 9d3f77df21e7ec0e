"""GPU tests of the 1x1 residual projection folded into its block's second conv (wino1d_edge.hip, the RCIN > 0 instances).

Spans 1, 4 and 8 (downs.1.0 64 -> 128 @ 26, downs.2.0 128 -> 256 @ 13, ups.0.0 cat(256, 256) -> 128 @ 13) open with a block whose residual
is a 1x1 projection of the block input.  With whole Winograd items forced ("winograd_whole") Engine.res_fold picks where it is evaluated on
one handle: "fused" inside the second conv, behind its Mish, or "separate" as a launch of its own, as the library ran it before.

Sizes: 16 agents (one item at L = 13, two at L = 26), 24 (pad rows in the last item) and 40 (three items at L = 13, five -- an odd count
-- at L = 26).  Inputs as in test_gpu_unet_spans.py ("real"): a seeded random latent of scale 3 and seeded random cond rows, walked through the
float64 oracle up to the span; one timestep for all rows (the time row of the bias table is then a vector of its own, next to the per-agent
cond rows) -- the shuffled-batch test gives every row a timestep of its own instead (the time half folded into the per-agent rows).

Bar: the one test_gpu_unet_spans.py holds these spans to in the whole-item form on real inputs, |y - y64| <= 2 MEASURED u R_tile per element
(MEASURED[("f32", span, "auto/winograd_whole", "real")] = 1.5 / 2.66 / 2.99; R_tile: oracle.unet_span_bound(tile=True)), for the fused form
against float64 and, with the same right-hand side, for fused against separate.

Measured on the MI355X, largest ratio to u R_tile over the three sizes (the bar is 3.0 / 5.32 / 5.98):
  span                     1      4      8
  fused vs fp64        0.832   1.44   1.71
  separate vs fp64     0.814  0.916  0.823
  fused vs separate    0.929   1.51   2.19
(profiles/r05/res_fused_tests.txt has them per size.)  The fused form adds the projection's products one K step at a time onto the block's
activated output instead of onto the projection's own bias, so its partial sums are larger and its rounding with them; both forms stay
well under the bar.
"""
import pytest
import torch

from cld_amd import synth

import test_gpu_unet_spans as S

pytestmark = pytest.mark.gpu

SPANS = (1, 4, 8)
SIZES = (16, 24, 40)
SPAN_IO = {1: (6, None, 2), 4: (6, None, 2), 8: (3, 5, 2)}       # workspace buffers of a span: input, skip, output (cld_api.hip kSpanIn / kSpanSkip / kSpanOut)
ACT, NCB, LAT = 3328, 1792, 52 * 4                                 # floats per agent of an activation buffer, of the bias rows, of a latent


def _kappa(span):
    return 2.0 * S.MEASURED[("f32", span, "auto/winograd_whole", "real")]


@pytest.fixture(scope="module")
def eng():
    from cld_amd.engine import Engine
    e = Engine(n_timesteps=100, device="cuda:0", precision="f32")
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True))
    return e.finalize()


@pytest.fixture(scope="module")
def cases():
    """{B: (cond, t, {span: (x1, x2, y64, R_tile)})}: the float64 walk up to span 8, once per size."""
    from oracle import cld_oracle as O
    w64 = O.to_torch(synth.make_unet_weights(0, affine_jitter=True), dtype=torch.float64)
    out = {}
    for B in SIZES:
        g = torch.Generator().manual_seed(5000 + B)
        x = (torch.randn(B, 52, 4, generator=g, dtype=torch.float64) * 3.0).float()
        cond = torch.from_numpy(synth.make_inputs(B, 11)["cond_feat"]).float()
        t = torch.full((B,), 23 + B, dtype=torch.int64)
        tc, Rtc = O.unet_tc_bound(w64, cond.double(), t)
        real, per_span, h = [], {}, x
        for span in range(9):
            skip = real[O.UNET_SPAN_SKIP[span]] if span in O.UNET_SPAN_SKIP else None
            y64, R = O.unet_span_bound(w64, span, h.double(), None if skip is None else skip.double(), tc, tile=span in SPANS, Rtc=Rtc)
            if span in SPANS:
                per_span[span] = (h, skip, y64, R)
            real.append(y64.float())
            h = real[-1]
        out[B] = (cond, t, per_span)
    return out


def _run(eng, span, fold, x1, x2, cond, t):
    eng.force_kernel("conv5", "winograd_whole")
    eng.res_fold(fold)
    try:
        tt = t if len(set(t.tolist())) > 1 else int(t[0])
        return eng.debug_unet_span(span, x1.cuda(), cond.cuda(), tt, None if x2 is None else x2.cuda()).cpu()
    finally:
        eng.force_kernel("conv5", "auto")
        eng.res_fold("fused")


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("span", SPANS)
def test_fused_projection_vs_fp64_and_vs_separate(eng, cases, span, B):
    cond, t, per_span = cases[B]
    x1, x2, y64, R = per_span[span]
    ys = _run(eng, span, "separate", x1, x2, cond, t).double()
    yf = _run(eng, span, "fused", x1, x2, cond, t).double()
    assert torch.isfinite(yf).all() and torch.isfinite(ys).all()
    r_f, _ = S._ratio(yf, y64, R)
    r_s, _ = S._ratio(ys, y64, R)
    r_fs, nz = S._ratio(yf, ys, R)
    print(f"\nspan {span} B {B}: fused vs fp64 {r_f:.3g}, separate vs fp64 {r_s:.3g}, fused vs separate {r_fs:.3g} ({nz} elements differ), bar {_kappa(span):.3g}")
    assert nz > 0, "the two forms sum the residual in different orders: identical outputs mean the switch did nothing"
    assert r_f <= _kappa(span), (span, B, r_f)
    assert r_fs <= _kappa(span), (span, B, r_fs)


@pytest.mark.parametrize("span", SPANS)
def test_fused_row_does_not_depend_on_its_place_in_the_batch(eng, cases, span):
    """16 rows of the 40-row batch, shuffled, as a batch of their own: bit for bit the rows of the 40-row run (another item, another
    row of it, another half of an L = 26 item).  Every row has a timestep of its own here."""
    cond, _, per_span = cases[40]
    x1, x2, _, _ = per_span[span]
    g = torch.Generator().manual_seed(77 + span)
    t = torch.randint(0, 100, (40,), generator=g)
    pick = torch.randperm(40, generator=g)[:16]
    y40 = _run(eng, span, "fused", x1, x2, cond, t)
    y16 = _run(eng, span, "fused", x1[pick], None if x2 is None else x2[pick], cond[pick], t[pick])
    assert torch.equal(y16, y40[pick])


@pytest.mark.parametrize("span", SPANS)
def test_fused_leaves_pad_rows_and_the_projection_buffer_alone(eng, cases, span):
    """24 agents in a workspace of 32 rows, cleared first: behind the fused span the buffer the separate form keeps the projection in has not
    been written, and the separate form does write it -- the switch reaches the launches, and the fused form does not quietly run the
    separate one.  That the pad rows of the span's inputs are still zero is a sanity check only (no conv kernel writes its input).  The
    offsets are cld_api.hip's carve(): a change there shows as the input rows not being found where this test looks for them."""
    cond, t, per_span = cases[24]
    x1, x2, _, _ = per_span[span]
    bp = 32
    i_in, i_skip, _ = SPAN_IO[span]
    L, C = x1.shape[1], x1.shape[2]

    def buf(i):
        ws = eng._ws.view(torch.float32)
        o = bp * (3 * LAT + NCB + i * ACT)
        return ws[o:o + bp * ACT]

    _run(eng, span, "fused", x1, x2, cond, t)           # sizes the workspace
    eng._ws.zero_()
    y = _run(eng, span, "fused", x1, x2, cond, t)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    for i in (i_in, i_skip):
        if i is not None:
            rows = buf(i)[:bp * L * C].view(bp, L * C)
            assert torch.equal(rows[:24].cpu(), (x1 if i == i_in else x2).reshape(24, -1))
            assert not rows[24:].any(), "pad rows of the span's input"
    assert not buf(0).any(), "the fused form keeps no projection tensor"
    _run(eng, span, "separate", x1, x2, cond, t)
    torch.cuda.synchronize()
    assert buf(0).any()
