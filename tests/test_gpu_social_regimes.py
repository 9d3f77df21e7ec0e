"""The social-group kernel (csrc/social_kernels.hip) against the float64 yardstick (tests/social_yardstick.py) per group, in every
launch regime, and ON its ties and draws: the cases of tests/social_cases.py, whose claims tests/test_social_cases_host.py asserts on the
CPU.

The check (social_cases.ratios): errors are normalised before the maximum is taken -- gradient and values per group by the group's
max|g64| / max|v64| (the gradient per member in `hub`) -- and held to max(err / m) <= 4 max(err32 / m) + 1e-7, err32 the float32
yardstick on the scene translated back to the origin; the worst group counts.  `exact_ties` leaves nothing to rounding and is held to
55 x 2^-24 of its group's largest value and 8 x 2^-24 of its largest gradient element (`exact`), the factors counted from the kernel's
operation chain (tests/social_cases.py).  Also per case: columns 2..5, the rows of agents in no group and of leaders are exactly grad_in
(or 0), values outside the groups are 0, nothing is NaN, two calls give the same bits, want_grad=False gives the same values, and
through the C entry loss == NULL gives the same gradient bits and grad == grad_in (in place) the bits of the out-of-place call.
`exact_draws` also runs with its raw draws, outside [0, M - 2]: the bits of the clamped ones.

MEASURED (MI355X; error over the bar; f32 and f16x2 modes give the same bits):
    case            values  grad_x  grad_y   exact    over the bars relative to the global maximum: values / gradient
    m4               0.348   0.157   0.078            0.0029 / 0.0009
    m5_3_2           0.399   0.231   0.129            0.0072 / 0.0045
    m6               0.621   0.215   0.217            0.0069 / 0.0016
    m9_8_2           0.965   0.250   0.229            0.0034 / 0.0086
    m9_8_2_n3        0.288   0.243   0.238            0.0100 / 0.0084
    m16              0.154   0.256   0.253            0.0046 / 0.0288
    m64_7            0.610   0.254   0.114            0.0083 / 0.0015
    m85              0.431   0.162   0.087            0.0081 / 0.0010
    m86_16           0.573   0.255   0.144            0.0100 / 0.0010
    declared_128     0.413   0.221   0.126            0.0114 / 0.0016
    hub              0.410   0.292   0.200            0.0098 / 0.0050
    far              0.468   0.249   0.231            0.0079 / 0.0087
    exact_ties       0.000                   0.078    0      / 0.0002
    exact_draws      0.181   0.181   0.156            0.0051 / 0.0014
    The values of m9_8_2 sit closest to their bar: the kernel adds a member's 52 squared errors up one after another, the calibrator's
    mean is a pairwise sum.  The kernel was not changed: no case was over its bar and no rule at a tie or a draw was broken.
"""
import ctypes as C

import pytest
import torch

from cld_amd import synth
from tests import social_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(precision):
    from cld_amd.engine import Engine
    e = Engine(n_timesteps=100, device="cuda:0", precision=precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True))
    e.load_state_dict(synth.make_decoder_weights(0))
    return e.finalize()


def engine_term(term, r, u, N):
    """The yardstick's term and one evaluation's draws [A,N,52] as Engine.social_group_loss takes them."""
    A = r.shape[0]
    return dict(groups=term["groups"], leader=term["leader"], social_dist=term["social_dist"], cohesion=term["cohesion"], scale=term["scale"],
                world_from_agent=term["world_from_agent"].float(), num_samp=N, max_members=term.get("max_members"),
                draw_r=r.reshape(A * N, 52), draw_u=u.reshape(A * N, 52))


def c_entry(eng, flat, te, grad_in, loss, grad):
    """cld_social_group_loss itself, on device tensors (or None)."""
    B = flat.shape[0]
    cs, keep = eng._social(te, B)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    eng._check(eng.lib.cld_social_group_loss(eng._h, ptr(flat), C.byref(cs), ptr(grad_in), ptr(loss), ptr(grad), B, eng._stream()), "cld_social_group_loss")
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", K.NAMES)
def test_social_kernel_vs_yardstick_per_group(eng, name):
    c = K.reference(name)
    plans, term = c["plans"], c["term"]
    A, N = plans.shape[:2]
    te = engine_term(term, c["r"], c["u"], N)
    flat = plans.reshape(A * N, 52, 6)
    loss, grad = eng.social_group_loss(flat, te)
    assert not bool(torch.isnan(loss).any()) and not bool(torch.isnan(grad).any())
    ratios = K.ratios(name, loss, grad)
    old = K.old_bar(name, loss, grad)
    print(f"\n[social regimes] {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + f"; over the global bars: values {old[0]:.3g}, gradient {old[1]:.3g}")
    # exact properties: untouched columns, non-members, leaders; with and without grad_in
    g, v = grad.cpu().reshape(A, N, 52, 6), loss.cpu().reshape(A, N)
    member, quiet = K.quiet_rows(term, A)
    assert not bool((g[..., 2:] != 0).any()) and not bool((g[quiet] != 0).any()) and not bool((v[~member] != 0).any())
    gin = torch.from_numpy(synth.normal(3, "social_grad_in", (A * N, 52, 6)))
    loss2, grad2 = eng.social_group_loss(flat, te, grad_in=gin)
    g2, gi = grad2.cpu().reshape(A, N, 52, 6), gin.reshape(A, N, 52, 6)
    assert torch.equal(loss2, loss)
    assert torch.equal(g2[..., 2:], gi[..., 2:]) and torch.equal(g2[quiet], gi[quiet])
    assert float((g2 - (g + gi)).abs().max()) <= 1e-6
    # deterministic; values alone
    loss3, grad3 = eng.social_group_loss(flat, te)
    assert torch.equal(loss3, loss) and torch.equal(grad3, grad)
    assert torch.equal(eng.social_group_loss(flat, te, want_grad=False), loss)
    # the C entry as the sampler uses it: no values wanted, the gradient accumulated in place
    dev, gin_d = flat.cuda().contiguous(), gin.cuda()
    only = torch.full_like(grad, 7.0)
    c_entry(eng, dev, te, None, None, only)
    assert torch.equal(only, grad)
    in_place = gin_d.clone()
    c_entry(eng, dev, te, in_place, None, in_place)
    assert torch.equal(in_place, grad2)
    if c["r_raw"] is not None:                                              # a caller's r outside [0, M - 2]: the clamped draw's bits
        loss4, grad4 = eng.social_group_loss(flat, engine_term(term, c["r_raw"], c["u"], N))
        assert torch.equal(loss4, loss) and torch.equal(grad4, grad)
    bad = {k: x for k, x in ratios.items() if not x <= 1.0}
    assert not bad, f"{name}: over the bar: {bad}"
