"""The agent-collision kernel (csrc/collision_kernels.hip) against the float64 yardstick (tests/collision_yardstick.py) in every launch
regime and parameter setting: the cases of tests/collision_cases.py, whose claims tests/test_collision_host.py asserts on the CPU.

The bar (tests/grad_bar.py), applied separately to the values and to each of the gradient channels x, y and yaw over the unflagged
elements:  max|got - ref64| <= 4 max|ref32 - ref64| + 1e-7 max|ref64|,  ref32 / ref64 the yardstick in float32 / float64.  An element is
flagged where float64 says that rounding may decide (a pair within 1e-4 of its bound, two disk pairs within 1e-4 of each other, a
distance below 0.05 m): its value is checked like any other, its gradient must lie in the interval the admissible alternatives span,
widened by the same bar (`interval`).  `exact_tie` leaves nothing to rounding and holds its tied elements to the first minimum (`exact`).
Also per case: channels 2, 4 and 5 and the rows of stationary, unguided and lone agents are exactly grad_in (or 0), nothing is NaN, two
calls give the same bits.

MEASURED (MI355X; error over the bar, worst of values / grad_x / grad_y / grad_yaw / interval; f32 and f16x2 modes give the same bits):
    case           values  grad_x  grad_y  grad_yaw  interval   flagged / gradient-carrying elements
    sizes_n1        0.182   0.223   0.250    0.244     0.028   5 / 462
    sizes_n3        0.259   0.224   0.273    0.129         0   22 / 1712
    lds_cap         0.132   0.284   0.272    0.177      0.04   85 / 6508
    disks_1         0.096   0.097   0.111    0.130         0   0 / 1941
    disks_2         0.237   0.156   0.121    0.138      0.13   14 / 2640
    disks_4         0.150   0.141   0.170    0.121     0.037   32 / 2893
    disks_5         0.153   0.324   0.174    0.137     0.003   73 / 3000
    disks_8         0.262   0.171   0.200    0.186     0.081   110 / 3008
    params_base     0.140   0.171   0.260    0.151         0   7 / 481
    buffer_0        0.122   0.172   0.262    0.150         0   6 / 428
    buffer_1        0.173   0.162   0.261    0.148   0.00059   8 / 672
    decay_1         0.144   0.434   0.491    0.353   0.00047   7 / 481
    decay_05        0.119   0.259   0.161    0.143     9e-11   7 / 481
    speed_th        0.140   0.172   0.118    0.099         0   2 / 271
    wide            0.061   0.290   0.350    0.475      0.06   16 / 1157
    frames          0.147   0.099   0.227    0.213         0   5 / 460
    masks           0.128   0.157   0.183    0.107         0   0 / 290
    kink_inside     0.185   0.195   0.387    0.492         0   0 / 312
    kink_outside    0.171   0.179   0.778    0.584         0   0 / 208
    exact_tie       0.371   0.000   0.000    0.000      0.11   104 / 104   (exact 0.012)
    Before the reach fix (signed half extents in the far-pair rejection) `wide` stood at values 6.2e4, grad_x 4.5e5, grad_y 2.4e5,
    grad_yaw 1.9e4, interval 4.3e5; with the step weights and the value sum in float, kink_inside / kink_outside at values 1.00 / 1.08.
"""
import ctypes as C

import pytest
import torch

from cld_amd import synth
from tests import collision_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(precision):
    from cld_amd.engine import Engine
    e = Engine(n_timesteps=100, device="cuda:0", precision=precision)
    e.load_state_dict(synth.make_unet_weights(0, affine_jitter=True))
    e.load_state_dict(synth.make_decoder_weights(0))
    return e.finalize()


@pytest.mark.parametrize("name", K.NAMES)
def test_agent_collision_kernel_vs_yardstick(eng, name):
    plans, term, r64, r32 = K.reference(name)
    B, N = plans.shape[:2]
    flat = plans.reshape(B * N, 52, 6)
    cfg = K.engine_cfg(term, N)
    loss, grad = eng.agent_collision(flat, cfg)
    assert not bool(torch.isnan(loss).any()) and not bool(torch.isnan(grad).any())
    ratios = K.ratios(name, loss, grad)
    print(f"\n[collision regimes] {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) +
          f"; {int(r64['flagged'].sum())} of {int(r64['carrying'].sum())} elements flagged")
    # exact properties: untouched channels, rows that receive nothing, the lone agent; with and without grad_in
    g = grad.cpu().reshape(B, N, 52, 6)
    quiet = K.quiet_rows(term, B)
    assert not bool((g[..., [2, 4, 5]] != 0).any()) and not bool((g[quiet] != 0).any())
    still = term["curr_speed"].abs() <= term["guide_moving_speed_th"]
    assert not bool((loss.cpu().reshape(B, N)[still] != 0).any())
    gin = torch.from_numpy(synth.normal(7, "collision_grad_in", (B * N, 52, 6)))
    loss2, grad2 = eng.agent_collision(flat, cfg, grad_in=gin)
    g2, gi = grad2.cpu().reshape(B, N, 52, 6), gin.reshape(B, N, 52, 6)
    assert torch.equal(loss2, loss)
    assert torch.equal(g2[..., [2, 4, 5]], gi[..., [2, 4, 5]]) and torch.equal(g2[quiet], gi[quiet])
    assert float((g2 - (g + gi)).abs().max()) <= 1e-6
    # deterministic; values alone
    loss3, grad3 = eng.agent_collision(flat, cfg)
    assert torch.equal(loss3, loss) and torch.equal(grad3, grad)
    assert torch.equal(eng.agent_collision(flat, cfg, want_grad=False), loss)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{name}: over the bar: {bad}"


def test_scenes_and_disk_counts_beyond_the_launch_are_refused_before_any_launch(eng):
    """A scene of 193 agents (164,512 bytes of LDS, 672 more than the 160 KiB) and num_disks 0 and 9: CldError, and the value and gradient
    buffers keep their sentinel -- the launcher returns before it launches anything."""
    from cld_amd._lib import CldError
    for sizes, disks in (([K.LDS_CAP + 1], 5), ([12, 5], 0), ([12, 5], 9)):
        plans, term = K.synth_case(sizes, 1, 3, 3.0, num_disks=disks)
        B = sum(sizes)
        traj = plans.reshape(B, 52, 6).cuda()
        cc, keep = eng._collision(K.engine_cfg(term, 1), B)
        loss = torch.full((B,), 7.0, device="cuda")
        grad = torch.full((B, 52, 6), 7.0, device="cuda")
        with pytest.raises(CldError):
            eng._check(eng.lib.cld_agent_collision(eng._h, C.c_void_p(traj.data_ptr()), C.byref(cc), None, C.c_void_p(loss.data_ptr()),
                                                   C.c_void_p(grad.data_ptr()), B, eng._stream()), "cld_agent_collision")
        torch.cuda.synchronize()
        assert bool((loss == 7.0).all()) and bool((grad == 7.0).all())
        with pytest.raises(CldError):
            eng.agent_collision(traj, K.engine_cfg(term, 1))
    # the largest scene that is not refused runs: covered by the case `lds_cap` above
