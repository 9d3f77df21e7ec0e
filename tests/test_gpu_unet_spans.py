"""GPU tests of the U-Net span by span, in every form each span has, against a float64 reference per element.

cld_debug_unet_span runs one of the 12 spans a U-Net evaluation is made of (include/cld.h; run_unet is the 12 spans in a row) with the
launches cld_unet_forward makes for it, in the form cld_debug_force_kernel holds:
  spans 0 (downs.0.*) and 11 (ups.1.*, final_conv.*): the layer launches ("layers"), the direct layer chains with one- / four-agent tiles
      ("chain1" / "chain4") and the Winograd chains with one- / two- / four-agent tiles ("chainw1" / "chainw2" / "chainw");
  spans 1-9 and 11 (the k5 layers at L = 13 / 26): the direct launches ("direct"), Winograd F(4, 5) by launch size ("winograd"), whole
      items ("winograd_whole", wino1d_edge.hip) and eight-wave whole items ("winograd_ksplit");
  and AUTO, which takes each of these by launch size.  The split-precision mode has the layer launches and the direct form only.
The sizes are chosen so that AUTO reaches every regime of every Winograd shape (cld_debug_conv5_items, asserted per size): direct below
384 rows, half items, eight-wave items (768-1,024 rows at 256 output channels / L = 13, 1,536-2,048 at 128), whole items at 2,048 / 4,096
(groups % 8 == 0) and 3,205 (a partly filled last generation, groups % 8 != 0, a ragged pad), half items again at 2,560 (a last generation
at most half full); 944 / 960 straddle the chain tile switch.

The reference is oracle.unet_span_bound: y in float64 and a running-error magnitude R (units of u = 2^-24) of an fp32 evaluation of
the span.  The bar is |y - y64| <= KAPPA * u * R_form per element, R_form = R for the direct forms and R's maximum over each
aligned 4-row tile (of every k5 output and of the span's output) for the forms that run a Winograd F(4, 5) layer: one transform-domain
rounding reaches the whole tile.  Inputs: "real" (the previous span's float64 output rounded to fp32, from a latent of scale 3) at every
size, and "adversarial" (the same with the border rows and the rows at F(4, 5) tile edges scaled by 64) at three sizes.

R propagates the rounding of a layer's input in quadrature, R_y = |W| |x| + sqrt(W^2 R_x^2) + |b| (the triangle form |W| (|x| + R_x)
compounds by ~sqrt(K) per layer: R / |y| reached ~2e6 on span 0 and ~3e9 on span 11, where a 2^-12 weight error hid under the bar).  It
is a model of the error, not a strict bound, so each bar is calibrated: KAPPA = twice the largest ratio measured for that precision, span,
form ("unet form/conv5 form") and kind of input, over all sizes (MEASURED, each under the span's KAPPA_CAP, a tenth of 2^24 / (5 C_in)).
test_host_logic.py test_unet_span_bound_holds_for_fp32_and_sees_a_wrong_tap shows on the CPU that R bounds the fp32 oracle within 8 u R
and that tap 0 of any one k5 layer scaled by 1 + 2^-12 lands more than 10x above twice the worst fp32 ratio on real inputs, in every
span, the chain head (0) and tail (11) included.

Injected faults (scratch builds), largest ratio over the bar on real inputs: a dropped direct-column tap in whole items at L = 13, 7.7e6;
one input-transform constant x (1 + 2^-12) in the second K half of eight-wave items, 121; the one-agent Winograd tail chain reading the
residual of its last tile one row off, 1.8e5; the GroupNorm mean of the last item of a partly filled generation over 12 of its 13 rows
(3,205 rows), 1.8e3; conv_pair's 1x1 projection adding the other layer's bias, 2.7e5.

Measured on the MI355X, largest ratio over the forms per span (MEASURED has them per form; _report_ratios prints them with -s):
  span                  0     1     2     3     4     5     6     7     8     9    10    11
  f32   real         0.44  2.85  2.91  4.15  3.69  3.29  3.09  3.28  4.33  2.85  6.49 0.0306
  f32   adversarial  4.22  3.31  2.96  5.29   4.3  2.57  2.67   2.5   3.5  2.59  4.54 0.788
  f16x2 real        0.276  2.48  5.56  4.32  2.43  5.95  4.55  6.07  2.89  5.79  5.22 0.021
  f16x2 adversarial  2.82  2.76  4.85   6.8  3.09  5.56  4.87  4.89  3.75  5.05  5.69 0.353
Module wall time on the GPU machine: ~250 s for both precision modes, most of it the float64 reference.
"""
import os

import pytest
import torch

from cld_amd import _lib, synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SIZES = (1, 37, 384, 768, 944, 960, 1536, 2048, 2560, 3205, 4096)
ADVERSARIAL = (37, 944, 3205)
PER_ROW_T = (37, 3205)
UNET_FORMS = ("layers", "chain1", "chain4", "chainw1", "chainw2", "chainw")
CONV5_FORMS = ("direct", "winograd", "winograd_whole", "winograd_ksplit")
WINO_SHAPES = {1: [(26, 64, 0, 128), (26, 128, 0, 128)], 2: [(26, 128, 0, 128)], 4: [(13, 128, 0, 256), (13, 256, 0, 256)],
               5: [(13, 256, 0, 256)], 6: [(13, 256, 0, 256)], 7: [(13, 256, 0, 256)], 8: [(13, 256, 256, 128), (13, 128, 0, 128)],
               9: [(13, 128, 0, 128)], 11: [(26, 128, 128, 64)]}       # the k5 layers of each span that have a Winograd launch

# the largest ratio measured per (precision, span, "unet form/conv5 form", inputs) over SIZES (module docstring); the bar of each is twice it
MEASURED = {
    ('f16x2', 0, 'auto/auto', 'adversarial'): 2.82,
    ('f16x2', 0, 'auto/auto', 'real'): 0.276,
    ('f16x2', 0, 'auto/direct', 'adversarial'): 2.82,
    ('f16x2', 0, 'auto/direct', 'real'): 0.276,
    ('f16x2', 0, 'layers/auto', 'adversarial'): 2.82,
    ('f16x2', 0, 'layers/auto', 'real'): 0.276,
    ('f16x2', 1, 'auto/auto', 'adversarial'): 2.76,
    ('f16x2', 1, 'auto/auto', 'real'): 2.48,
    ('f16x2', 1, 'auto/direct', 'adversarial'): 2.76,
    ('f16x2', 1, 'auto/direct', 'real'): 2.48,
    ('f16x2', 1, 'layers/auto', 'adversarial'): 2.76,
    ('f16x2', 1, 'layers/auto', 'real'): 2.48,
    ('f16x2', 2, 'auto/auto', 'adversarial'): 4.85,
    ('f16x2', 2, 'auto/auto', 'real'): 5.56,
    ('f16x2', 2, 'auto/direct', 'adversarial'): 4.85,
    ('f16x2', 2, 'auto/direct', 'real'): 5.56,
    ('f16x2', 2, 'layers/auto', 'adversarial'): 4.85,
    ('f16x2', 2, 'layers/auto', 'real'): 5.56,
    ('f16x2', 3, 'auto/auto', 'adversarial'): 6.8,
    ('f16x2', 3, 'auto/auto', 'real'): 4.32,
    ('f16x2', 3, 'auto/direct', 'adversarial'): 6.8,
    ('f16x2', 3, 'auto/direct', 'real'): 4.32,
    ('f16x2', 3, 'layers/auto', 'adversarial'): 6.8,
    ('f16x2', 3, 'layers/auto', 'real'): 4.32,
    ('f16x2', 4, 'auto/auto', 'adversarial'): 3.09,
    ('f16x2', 4, 'auto/auto', 'real'): 2.43,
    ('f16x2', 4, 'auto/direct', 'adversarial'): 3.09,
    ('f16x2', 4, 'auto/direct', 'real'): 2.43,
    ('f16x2', 4, 'layers/auto', 'adversarial'): 3.09,
    ('f16x2', 4, 'layers/auto', 'real'): 2.43,
    ('f16x2', 5, 'auto/auto', 'adversarial'): 5.56,
    ('f16x2', 5, 'auto/auto', 'real'): 5.95,
    ('f16x2', 5, 'auto/direct', 'adversarial'): 5.56,
    ('f16x2', 5, 'auto/direct', 'real'): 5.95,
    ('f16x2', 5, 'layers/auto', 'adversarial'): 5.56,
    ('f16x2', 5, 'layers/auto', 'real'): 5.95,
    ('f16x2', 6, 'auto/auto', 'adversarial'): 4.87,
    ('f16x2', 6, 'auto/auto', 'real'): 4.55,
    ('f16x2', 6, 'auto/direct', 'adversarial'): 4.87,
    ('f16x2', 6, 'auto/direct', 'real'): 4.55,
    ('f16x2', 6, 'layers/auto', 'adversarial'): 4.87,
    ('f16x2', 6, 'layers/auto', 'real'): 4.55,
    ('f16x2', 7, 'auto/auto', 'adversarial'): 4.89,
    ('f16x2', 7, 'auto/auto', 'real'): 6.07,
    ('f16x2', 7, 'auto/direct', 'adversarial'): 4.89,
    ('f16x2', 7, 'auto/direct', 'real'): 6.07,
    ('f16x2', 7, 'layers/auto', 'adversarial'): 4.89,
    ('f16x2', 7, 'layers/auto', 'real'): 6.07,
    ('f16x2', 8, 'auto/auto', 'adversarial'): 3.75,
    ('f16x2', 8, 'auto/auto', 'real'): 2.89,
    ('f16x2', 8, 'auto/direct', 'adversarial'): 3.75,
    ('f16x2', 8, 'auto/direct', 'real'): 2.89,
    ('f16x2', 8, 'layers/auto', 'adversarial'): 3.75,
    ('f16x2', 8, 'layers/auto', 'real'): 2.89,
    ('f16x2', 9, 'auto/auto', 'adversarial'): 5.05,
    ('f16x2', 9, 'auto/auto', 'real'): 5.79,
    ('f16x2', 9, 'auto/direct', 'adversarial'): 5.05,
    ('f16x2', 9, 'auto/direct', 'real'): 5.79,
    ('f16x2', 9, 'layers/auto', 'adversarial'): 5.05,
    ('f16x2', 9, 'layers/auto', 'real'): 5.79,
    ('f16x2', 10, 'auto/auto', 'adversarial'): 5.69,
    ('f16x2', 10, 'auto/auto', 'real'): 5.22,
    ('f16x2', 10, 'auto/direct', 'adversarial'): 5.69,
    ('f16x2', 10, 'auto/direct', 'real'): 5.22,
    ('f16x2', 10, 'layers/auto', 'adversarial'): 5.69,
    ('f16x2', 10, 'layers/auto', 'real'): 5.22,
    ('f16x2', 11, 'auto/auto', 'adversarial'): 0.353,
    ('f16x2', 11, 'auto/auto', 'real'): 0.021,
    ('f16x2', 11, 'auto/direct', 'adversarial'): 0.353,
    ('f16x2', 11, 'auto/direct', 'real'): 0.021,
    ('f16x2', 11, 'layers/auto', 'adversarial'): 0.353,
    ('f16x2', 11, 'layers/auto', 'real'): 0.021,
    ('f32', 0, 'auto/auto', 'adversarial'): 3.85,
    ('f32', 0, 'auto/auto', 'real'): 0.385,
    ('f32', 0, 'chain1/auto', 'adversarial'): 4.22,
    ('f32', 0, 'chain1/auto', 'real'): 0.44,
    ('f32', 0, 'chain4/auto', 'adversarial'): 4.22,
    ('f32', 0, 'chain4/auto', 'real'): 0.41,
    ('f32', 0, 'chainw/auto', 'adversarial'): 3.85,
    ('f32', 0, 'chainw/auto', 'real'): 0.385,
    ('f32', 0, 'chainw1/auto', 'adversarial'): 3.85,
    ('f32', 0, 'chainw1/auto', 'real'): 0.385,
    ('f32', 0, 'chainw2/auto', 'adversarial'): 3.85,
    ('f32', 0, 'chainw2/auto', 'real'): 0.385,
    ('f32', 0, 'layers/auto', 'adversarial'): 2.35,
    ('f32', 0, 'layers/auto', 'real'): 0.269,
    ('f32', 1, 'auto/auto', 'adversarial'): 3.1,
    ('f32', 1, 'auto/auto', 'real'): 1.5,
    ('f32', 1, 'auto/direct', 'adversarial'): 3.31,
    ('f32', 1, 'auto/direct', 'real'): 2.85,
    ('f32', 1, 'auto/winograd', 'adversarial'): 3.1,
    ('f32', 1, 'auto/winograd', 'real'): 1.5,
    ('f32', 1, 'auto/winograd_ksplit', 'adversarial'): 3.1,
    ('f32', 1, 'auto/winograd_ksplit', 'real'): 1.5,
    ('f32', 1, 'auto/winograd_whole', 'adversarial'): 3.1,
    ('f32', 1, 'auto/winograd_whole', 'real'): 1.5,
    ('f32', 2, 'auto/auto', 'adversarial'): 1.52,
    ('f32', 2, 'auto/auto', 'real'): 1.47,
    ('f32', 2, 'auto/direct', 'adversarial'): 2.96,
    ('f32', 2, 'auto/direct', 'real'): 2.91,
    ('f32', 2, 'auto/winograd', 'adversarial'): 1.3,
    ('f32', 2, 'auto/winograd', 'real'): 1.17,
    ('f32', 2, 'auto/winograd_ksplit', 'adversarial'): 0.983,
    ('f32', 2, 'auto/winograd_ksplit', 'real'): 1.05,
    ('f32', 2, 'auto/winograd_whole', 'adversarial'): 1.3,
    ('f32', 2, 'auto/winograd_whole', 'real'): 1.17,
    ('f32', 3, 'auto/auto', 'adversarial'): 5.29,
    ('f32', 3, 'auto/auto', 'real'): 4.15,
    ('f32', 4, 'auto/auto', 'adversarial'): 3.9,
    ('f32', 4, 'auto/auto', 'real'): 2.45,
    ('f32', 4, 'auto/direct', 'adversarial'): 4.3,
    ('f32', 4, 'auto/direct', 'real'): 3.69,
    ('f32', 4, 'auto/winograd', 'adversarial'): 3.9,
    ('f32', 4, 'auto/winograd', 'real'): 2.45,
    ('f32', 4, 'auto/winograd_ksplit', 'adversarial'): 3.9,
    ('f32', 4, 'auto/winograd_ksplit', 'real'): 2.66,
    ('f32', 4, 'auto/winograd_whole', 'adversarial'): 3.9,
    ('f32', 4, 'auto/winograd_whole', 'real'): 2.66,
    ('f32', 5, 'auto/auto', 'adversarial'): 1.78,
    ('f32', 5, 'auto/auto', 'real'): 2.53,
    ('f32', 5, 'auto/direct', 'adversarial'): 2.57,
    ('f32', 5, 'auto/direct', 'real'): 3.29,
    ('f32', 5, 'auto/winograd', 'adversarial'): 1.78,
    ('f32', 5, 'auto/winograd', 'real'): 2.53,
    ('f32', 5, 'auto/winograd_ksplit', 'adversarial'): 1.78,
    ('f32', 5, 'auto/winograd_ksplit', 'real'): 2.67,
    ('f32', 5, 'auto/winograd_whole', 'adversarial'): 1.78,
    ('f32', 5, 'auto/winograd_whole', 'real'): 2.85,
    ('f32', 6, 'auto/auto', 'adversarial'): 1.58,
    ('f32', 6, 'auto/auto', 'real'): 2.24,
    ('f32', 6, 'auto/direct', 'adversarial'): 2.67,
    ('f32', 6, 'auto/direct', 'real'): 3.09,
    ('f32', 6, 'auto/winograd', 'adversarial'): 1.35,
    ('f32', 6, 'auto/winograd', 'real'): 2.24,
    ('f32', 6, 'auto/winograd_ksplit', 'adversarial'): 0.979,
    ('f32', 6, 'auto/winograd_ksplit', 'real'): 2.53,
    ('f32', 6, 'auto/winograd_whole', 'adversarial'): 1.22,
    ('f32', 6, 'auto/winograd_whole', 'real'): 2.27,
    ('f32', 7, 'auto/auto', 'adversarial'): 1.59,
    ('f32', 7, 'auto/auto', 'real'): 2.44,
    ('f32', 7, 'auto/direct', 'adversarial'): 2.5,
    ('f32', 7, 'auto/direct', 'real'): 3.28,
    ('f32', 7, 'auto/winograd', 'adversarial'): 1.12,
    ('f32', 7, 'auto/winograd', 'real'): 2.44,
    ('f32', 7, 'auto/winograd_ksplit', 'adversarial'): 0.98,
    ('f32', 7, 'auto/winograd_ksplit', 'real'): 3.16,
    ('f32', 7, 'auto/winograd_whole', 'adversarial'): 1.12,
    ('f32', 7, 'auto/winograd_whole', 'real'): 2.44,
    ('f32', 8, 'auto/auto', 'adversarial'): 3.31,
    ('f32', 8, 'auto/auto', 'real'): 2.99,
    ('f32', 8, 'auto/direct', 'adversarial'): 3.5,
    ('f32', 8, 'auto/direct', 'real'): 4.33,
    ('f32', 8, 'auto/winograd', 'adversarial'): 3.31,
    ('f32', 8, 'auto/winograd', 'real'): 2.99,
    ('f32', 8, 'auto/winograd_ksplit', 'adversarial'): 3.28,
    ('f32', 8, 'auto/winograd_ksplit', 'real'): 3.16,
    ('f32', 8, 'auto/winograd_whole', 'adversarial'): 3.31,
    ('f32', 8, 'auto/winograd_whole', 'real'): 2.99,
    ('f32', 9, 'auto/auto', 'adversarial'): 1.75,
    ('f32', 9, 'auto/auto', 'real'): 2.51,
    ('f32', 9, 'auto/direct', 'adversarial'): 2.59,
    ('f32', 9, 'auto/direct', 'real'): 2.78,
    ('f32', 9, 'auto/winograd', 'adversarial'): 0.978,
    ('f32', 9, 'auto/winograd', 'real'): 2.51,
    ('f32', 9, 'auto/winograd_ksplit', 'adversarial'): 0.978,
    ('f32', 9, 'auto/winograd_ksplit', 'real'): 2.51,
    ('f32', 9, 'auto/winograd_whole', 'adversarial'): 0.978,
    ('f32', 9, 'auto/winograd_whole', 'real'): 2.85,
    ('f32', 10, 'auto/auto', 'adversarial'): 4.54,
    ('f32', 10, 'auto/auto', 'real'): 6.49,
    ('f32', 11, 'auto/auto', 'adversarial'): 0.645,
    ('f32', 11, 'auto/auto', 'real'): 0.0306,
    ('f32', 11, 'auto/direct', 'adversarial'): 0.466,
    ('f32', 11, 'auto/direct', 'real'): 0.0304,
    ('f32', 11, 'auto/winograd', 'adversarial'): 0.645,
    ('f32', 11, 'auto/winograd', 'real'): 0.0306,
    ('f32', 11, 'auto/winograd_ksplit', 'adversarial'): 0.749,
    ('f32', 11, 'auto/winograd_ksplit', 'real'): 0.0275,
    ('f32', 11, 'auto/winograd_whole', 'adversarial'): 0.788,
    ('f32', 11, 'auto/winograd_whole', 'real'): 0.0306,
    ('f32', 11, 'chain1/auto', 'adversarial'): 0.349,
    ('f32', 11, 'chain1/auto', 'real'): 0.0234,
    ('f32', 11, 'chain4/auto', 'adversarial'): 0.378,
    ('f32', 11, 'chain4/auto', 'real'): 0.0229,
    ('f32', 11, 'chainw/auto', 'adversarial'): 0.645,
    ('f32', 11, 'chainw/auto', 'real'): 0.0306,
    ('f32', 11, 'chainw1/auto', 'adversarial'): 0.645,
    ('f32', 11, 'chainw1/auto', 'real'): 0.0306,
    ('f32', 11, 'chainw2/auto', 'adversarial'): 0.645,
    ('f32', 11, 'chainw2/auto', 'real'): 0.0306,
    ('f32', 11, 'layers/auto', 'adversarial'): 0.325,
    ('f32', 11, 'layers/auto', 'real'): 0.0228,
}
SPAN_CIN = [64, 128, 128, 128, 256, 256, 256, 256, 512, 128, 128, 256]     # the widest layer input of each span
KAPPA_CAP = [2.0 ** 24 / (5 * c) / 10 for c in SPAN_CIN]                    # a tenth of the ratio one wrong tap produces against R ~ |W||x|


def _kappa(key):
    return 2.0 * MEASURED[key]


RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if RATIOS:
        print("\nmax |y - y64| / (u R_form) per precision, span, form and inputs:")
        for key, r in sorted(RATIOS.items()):
            print(f"    {key!r}: {r:.3g},")


@pytest.fixture(scope="module")
def w64():
    from oracle import cld_oracle as O
    return O.to_torch(synth.make_unet_weights(0, affine_jitter=True), dtype=torch.float64)


@pytest.fixture(scope="module")
def eng(precision):
    from cld_amd.engine import Engine
    e = Engine(n_timesteps=100, device="cuda:0", precision=precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True))
    return e.finalize()


def _inputs(B):
    g = torch.Generator().manual_seed(1000 + B)
    x = torch.randn(B, 52, 4, generator=g, dtype=torch.float64) * 3.0
    cond = torch.from_numpy(synth.make_inputs(B, 7)["cond_feat"]).double()
    t = torch.randint(0, 100, (B,), generator=g) if B in PER_ROW_T else torch.full((B,), 17 + B % 80, dtype=torch.int64)
    return x.float(), cond.float(), t


def _adversarial(x):
    """x [B, L, C] with the border rows and the rows at F(4, 5) tile edges (l = 0, 3, 4, 7, 8, 11, 12, L - 1) scaled by 64."""
    L = x.shape[1]
    rows = sorted({r for r in (0, 3, 4, 7, 8, 11, 12, L - 1) if r < L})
    s = torch.ones(L, dtype=x.dtype)
    s[rows] = 64.0
    return x * s[None, :, None]


def _forms(precision, span):
    """(unet form, conv5 form) pairs that exist for a span (the others: "auto")."""
    out = [("auto", "auto")]
    if precision == "f32":
        if span in (0, 11):
            out += [(u, "auto") for u in UNET_FORMS]
        if span in WINO_SHAPES:
            out += [("auto", c) for c in CONV5_FORMS]
    else:
        out += [("layers", "auto"), ("auto", "direct")]
    return out


def _takes_wino(precision, span, uform, cform, B):
    """Whether the span runs a Winograd F(4, 5) layer in this form at B rows (then R_form is tiled).  Spans 0 and 11: exact-fp32 handles
    run the layer chains at every size unless "layers" is forced (cld_api.hip use_chains), and their 64 -> 64 k5 layers in Winograd form
    unless a direct chain ("chain1" / "chain4") or the direct k5 form is forced (chain_wino): so AUTO always takes the Winograd chains.
    The other k5 layers: the library's own rule, cld_debug_conv5_form."""
    if precision != "f32":
        return False
    chain = span in (0, 11) and uform != "layers" and (uform.startswith("chainw") or (uform in ("auto", "chain") and cform != "direct"))
    f = _lib.load().cld_debug_conv5_form
    k5 = any(f(*s, B, _lib.form_id("conv5", cform)) == _lib.form_id("conv5", "winograd") for s in WINO_SHAPES.get(span, []))
    return chain or k5


def _run(eng, span, uform, cform, x1, x2, cond, t):
    eng.force_kernel("unet", uform)
    eng.force_kernel("conv5", cform)
    try:
        tt = t if len(set(t.tolist())) > 1 else int(t[0])
        y = eng.debug_unet_span(span, x1.cuda(), cond.cuda(), tt, None if x2 is None else x2.cuda())
        return y.cpu().double()
    finally:
        eng.force_kernel("unet", "auto")
        eng.force_kernel("conv5", "auto")


def _ratio(y, y64, R):
    err = (y - y64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / (U * R))
    return float(r.max()), int((r > 0).sum())


REGIME_SHAPES = [(26, 64, 128), (26, 128, 128), (13, 128, 256), (13, 256, 256), (13, 512, 128), (13, 128, 128), (26, 256, 64)]
# what AUTO takes at each size for each Winograd shape (L, C_in, C_out): -1 direct, 0 half items, 1 whole items, 2 eight-wave whole items
REGIMES = {1: (-1,) * 7, 37: (-1,) * 7, 384: (0,) * 7, 768: (2, 2, 2, 2, 0, 0, 0), 944: (2, 2, 2, 2, 0, 0, 0), 960: (2, 2, 2, 2, 0, 0, 0),
           1536: (0, 0, 0, 0, 2, 2, 2), 2048: (1, 1, 1, 1, 2, 2, 2), 2560: (0,) * 7, 3205: (1, 1, 1, 1, 0, 0, 0), 4096: (1,) * 7}


def _item_regimes(B):
    """{(L, C_in, C_out): the form AUTO takes at B rows} for the U-Net's Winograd shapes (cld_debug_conv5_form / cld_debug_conv5_items)."""
    lib = _lib.load()
    forms = {}
    for shapes in WINO_SHAPES.values():
        for (L, c1, c2, co) in shapes:
            wino = lib.cld_debug_conv5_form(L, c1, c2, co, B, 0) == _lib.form_id("conv5", "winograd")
            forms[(L, c1 + c2, co)] = lib.cld_debug_conv5_items(L, co, B, 0) if wino else -1
    return forms


def test_sizes_reach_every_item_regime():
    """Over SIZES, AUTO takes the direct form, half items, whole items and eight-wave items for every Winograd shape of the U-Net."""
    seen = {}
    for B in SIZES:
        for shape, f in _item_regimes(B).items():
            seen.setdefault(shape, set()).add(f)
    for shape, fs in seen.items():
        assert fs == {-1, 0, 1, 2}, (shape, fs)
    lib = _lib.load()
    assert lib.cld_debug_conv5_items(13, 256, 3205, 0) == 1 and ((3205 + 15) // 16) % 8 != 0        # whole items, groups % 8 != 0
    assert lib.cld_debug_conv5_items(13, 256, 2560, 0) == 0                                        # last generation at most half full


@pytest.mark.parametrize("B", SIZES)
def test_unet_spans_vs_fp64(eng, w64, precision, B):
    from oracle import cld_oracle as O
    regimes = _item_regimes(B)
    assert tuple(regimes[sh] for sh in REGIME_SHAPES) == REGIMES[B], regimes      # the regime this size is here for
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    x, cond, t = _inputs(B)
    tc, Rtc = O.unet_tc_bound(w64, cond.double(), t)
    kinds = ("real", "adversarial") if B in ADVERSARIAL else ("real",)
    real_out = []             # fp32-rounded fp64 outputs of the real chain: the next span's input and the skips
    fails = []
    h = x
    for span in range(12):
        skip = real_out[O.UNET_SPAN_SKIP[span]] if span in O.UNET_SPAN_SKIP else None
        forms = _forms(precision, span)
        tiles = {f: _takes_wino(precision, span, f[0], f[1], B) for f in forms}
        for kind in kinds:
            x1 = h if kind == "real" else _adversarial(h)
            x2 = skip if (skip is None or kind == "real") else _adversarial(skip)
            refs = {}
            for tile in sorted(set(tiles.values())):
                y64, R = O.unet_span_bound(w64, span, x1.double(), None if x2 is None else x2.double(), tc, tile=tile, Rtc=Rtc)
                refs[tile] = (y64, R)
            for f in forms:
                y64, R = refs[tiles[f]]
                y = _run(eng, span, f[0], f[1], x1, x2, cond, t)
                assert torch.isfinite(y).all(), (span, f)
                r, _ = _ratio(y, y64, R)
                key = (precision, span, "/".join(f), kind)
                RATIOS[key] = max(RATIOS.get(key, 0.0), r)
                k = _kappa(key)
                if r > k:
                    fails.append((span, f, kind, r, k))
            if kind == "real":
                y64 = refs[min(refs)][0]
                real_out.append(y64.float())
                del refs
        h = real_out[-1]
    assert not fails, fails


@pytest.mark.parametrize("B", (37, 3205))
def test_unet_spans_chain_to_unet_forward_bit_exactly(eng, precision, B):
    """The spans chained on the GPU reproduce cld_unet_forward's eps (AUTO): the debug entry runs the product dispatch.  The exact-fp32
    mode hands fp32 tensors across, so bit for bit; the split mode re-encodes the fp16 hi / lo planes, whose split of a tie may differ."""
    x, cond, t = _inputs(B)
    xc, cc = x.cuda(), cond.cuda()
    eps = eng.unet_forward_rows(xc, cc, t)
    outs = []
    h = xc
    tt = t
    for span in range(12):
        skip = outs[{8: 5, 11: 2}[span]] if span in (8, 11) else None
        h = eng.debug_unet_span(span, h, cc, tt, skip)
        outs.append(h)
    torch.cuda.synchronize()
    if precision == "f32":
        assert torch.equal(h, eps)
    else:
        assert float((h - eps).abs().max()) <= 1e-6 * max(1.0, float(eps.abs().max()))


def test_kappa_constants_under_their_caps():
    """Every (precision, span, form, inputs) the parity test runs has a measured ratio, and each bar stays under its span's cap."""
    keys = set()
    for prec in ("f32", "f16x2"):
        for B in SIZES:
            for span in range(12):
                for f in _forms(prec, span):
                    for kind in ("real", "adversarial") if B in ADVERSARIAL else ("real",):
                        keys.add((prec, span, "/".join(f), kind))
    assert keys == set(MEASURED)
    for (prec, span, form, kind), r in MEASURED.items():
        assert 0 < 2.0 * r <= KAPPA_CAP[span], (prec, span, form, kind)
