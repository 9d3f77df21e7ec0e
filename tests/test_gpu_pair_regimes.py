"""The pair-relation kernel (csrc/pair_kernels.hip) against the float64 yardstick (tests/pair_yardstick.py) per agent, per step and per
pair, in every launch regime, frame form and decay, and ON its kinks: the cases of tests/pair_cases.py, whose claims
tests/test_pair_cases_host.py asserts on the CPU.

The check (pair_cases.ratios): errors are normalised before the maximum is taken -- the gradient per involved agent and channel by the
agent's max|g64| (in decay_mix also per (agent, step)), the values per pair by the scale of what is read before the clip -- and held to
max(err / m) <= 4 max(err32 / m) + 1e-7, err32 the float32 yardstick on the scene translated back to the origin.  `exact_kinks` leaves
nothing to rounding and is held to 53 x 2^-24 of each value and 8 x 2^-24 of each agent's largest gradient element (`exact`), the
factors counted from the kernel's operation chain (tests/pair_cases.py).  Also per case: columns 2..5 and the rows of agents in no pair
are exactly grad_in (or 0), nothing is NaN, two calls give the same bits, want_grad=False gives the same values, and through the C entry
value == NULL gives the same gradient bits and grad == grad_in (in place) the bits of the out-of-place call.

MEASURED (MI355X; error over the bar; f32 and f16x2 modes give the same bits):
    case            values  grad_x  grad_y  step_x  step_y   exact    over the bars relative to the global maximum: values / gradient
    fill_exact       0.310   0.022   0.039                                    0.0075 / 0.0021
    fill_plus_one    0.245   0.043   0.041                                    0.0063 / 0.0033
    samples_3        0.302   0.194   0.257                                    0.0060 / 0.0014
    roles            0.383   0.209   0.210                                    0.0071 / 0.0025
    decay_mix        0.226   0.194   0.301   0.153   0.274                    0.0064 / 0.0022
    quadrants        0.421   0.168   0.207                                    0.0069 / 0.0016
    given_frames     0.337   0.057   0.139                                    0.0065 / 0.0019
    far              0.355   0.258   0.155                                    0.0082 / 0.0024
    exact_kinks      0.211                                   0.160            0.0278 / 0.0006
    The kernel was not changed: no case was over its bar and no rule at a kink was broken.
"""
import ctypes as C

import pytest
import torch

from cld_amd import synth
from tests import pair_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(precision):
    from cld_amd.engine import Engine
    e = Engine(n_timesteps=100, device="cuda:0", precision=precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True))
    e.load_state_dict(synth.make_decoder_weights(0))
    return e.finalize()


def engine_term(term, N):
    """The yardstick's term as Engine.pair_loss takes it."""
    F = term.get("agent_from_world")
    return dict(target=term["target"], ref=term["ref"], kind=term["kind"], lo=term["lo"], hi=term["hi"], decay=term["decay"], scale=term["scale"],
                world_from_agent=term["world_from_agent"].float(), agent_from_world=None if F is None else F.float(), num_samp=N)


def c_entry(eng, flat, te, grad_in, value, grad):
    """cld_pair_loss itself, on device tensors (or None)."""
    B = flat.shape[0]
    cs, keep = eng._pair(te, B)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    eng._check(eng.lib.cld_pair_loss(eng._h, ptr(flat), C.byref(cs), ptr(grad_in), ptr(value), ptr(grad), B, eng._stream()), "cld_pair_loss")
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", K.NAMES)
def test_pair_kernel_vs_yardstick_per_agent(eng, name):
    r = K.reference(name)
    plans, term = r["plans"], r["term"]
    A, N = plans.shape[:2]
    te = engine_term(term, N)
    flat = plans.reshape(A * N, 52, 6)
    value, grad = eng.pair_loss(flat, te)
    assert not bool(torch.isnan(value).any()) and not bool(torch.isnan(grad).any())
    ratios = K.ratios(name, value, grad)
    old = K.old_bar(name, value, grad)
    print(f"\n[pair regimes] {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + f"; over the global bars: values {old[0]:.3g}, gradient {old[1]:.3g}")
    # exact properties: untouched columns, rows in no pair; with and without grad_in
    g = grad.cpu().reshape(A, N, 52, 6)
    quiet = torch.ones(A, dtype=torch.bool)
    quiet[K.involved(term)] = False
    assert not bool((g[..., 2:] != 0).any()) and not bool((g[quiet] != 0).any())
    gin = torch.from_numpy(synth.normal(3, "pair_grad_in", (A * N, 52, 6)))
    value2, grad2 = eng.pair_loss(flat, te, grad_in=gin)
    g2, gi = grad2.cpu().reshape(A, N, 52, 6), gin.reshape(A, N, 52, 6)
    assert torch.equal(value2, value)
    assert torch.equal(g2[..., 2:], gi[..., 2:]) and torch.equal(g2[quiet], gi[quiet])
    assert float((g2 - (g + gi)).abs().max()) <= 1e-6
    # deterministic; values alone
    value3, grad3 = eng.pair_loss(flat, te)
    assert torch.equal(value3, value) and torch.equal(grad3, grad)
    assert torch.equal(eng.pair_loss(flat, te, want_grad=False), value)
    # the C entry as the sampler uses it: no values wanted, the gradient accumulated in place
    dev, gin_d = flat.cuda().contiguous(), gin.cuda()
    only = torch.full_like(grad, 7.0)
    c_entry(eng, dev, te, None, None, only)
    assert torch.equal(only, grad)
    in_place = gin_d.clone()
    c_entry(eng, dev, te, in_place, None, in_place)
    assert torch.equal(in_place, grad2)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{name}: over the bar: {bad}"
