"""The open-loop sample metrics on the device (csrc/sample_metrics_kernels.hip: cld_sample_metrics; include/cld_eval.h) and
`cld_amd.metrics.SampleMetrics`.

Two references.  tests/golden/sample_metrics.npz holds the reference's own float32 values (tests/tools/record_sample_metrics_golden.py);
the bar against it is 2e-6 relative, upstream's own rounding (sample_metrics_yardstick.BAR).  tests/sample_metrics_yardstick.py is the
float64 restatement; the kernel is fp64 throughout, so the bar against it is 1e-12 relative (BAR64: at most T + 4 roundings per value,
~6e-14 at T = 256, the margin for FMA contraction and the order of the folds), and an exact zero of the yardstick is an exact zero of
the kernel.  Indices, `last` and the non-finite flag are compared exactly.  The batch means are also compared BIT FOR BIT with a host
replay of the documented fold tree on the kernel's own rows.  Every test runs in both precision modes of the library; the kernels are
plain fp64 in both."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sample_metrics_yardstick as Y

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_WORKSPACE = 0, -1, -3


@pytest.fixture(scope="module")
def eng(precision):
    from cld_amd.engine import Engine
    return Engine(n_timesteps=10, device="cuda:0", precision=precision)          # no weights: none of this needs any


def cap():
    from cld_amd import _lib
    return int(_lib.load().cld_debug_sample_metrics_max_blocks())


def make(B, N, T, C=2, seed=0, scale=10.0):
    """Seeded inputs: agent b carries availability pattern b mod 6 (all, tail cut, none, hole, only the first, only the last step)."""
    rng = np.random.default_rng([seed, B, N, T, C])
    pred, gt = Y.trajectories(rng, B, N, T, C, scale)
    avail = Y.availability_patterns(T)[np.arange(B) % 6]
    return pred, gt, avail


def run(eng, pred, gt, avail):
    out = eng.sample_metrics(torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(avail))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def fold_replay(rows):
    """The batch means of per-agent rows [B,10] in the library's documented order, in numpy float64 (IEEE adds, so the same bits):
    partials of 256 rows, then one workgroup over the partials; in a workgroup lane l adds rows l, l + 256, ... in ascending order,
    a wave folds its 64 lanes by halves (32, 16, ..., 1) and the four waves are (w0 + w1) + (w2 + w3)."""
    def group(r):
        acc = np.zeros((256, r.shape[1]))
        for k in range(0, r.shape[0], 256):
            part = r[k:k + 256]
            acc[:part.shape[0]] += part
        w = acc.reshape(4, 64, -1)
        for off in (32, 16, 8, 4, 2, 1):
            w = w[:, :off] + w[:, off:2 * off]
        w = w[:, 0]
        return (w[0] + w[1]) + (w[2] + w[3])
    B = rows.shape[0]
    partials = np.stack([group(rows[k:k + 256]) for k in range(0, B, 256)])
    return group(partials) / float(B)


def check_against_yardstick(got, pred, gt, avail, what):
    ref = Y.metrics(pred, gt, avail)
    e_rows, e_means = Y.rel_err(got["per_agent"], ref["per_agent"]), Y.rel_err(got["means"], ref["means"])
    print(f"{what}: per-agent {e_rows:.2e}, means {e_means:.2e} (bar {Y.BAR64:.0e})")
    assert e_rows <= Y.BAR64 and e_means <= Y.BAR64, what
    assert np.array_equal(got["index"], ref["index"]), what
    assert np.array_equal(bits(got["means"]), bits(fold_replay(got["per_agent"]))), what


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("case", ["n5", "n1"])
def test_the_recorded_reference_values(eng, golden, case):
    """The eight keys and every per-agent array of the reference's own functions, within upstream's float32 rounding."""
    _, g = golden("sample_metrics")
    rec = {k[3:]: v for k, v in g.items() if k.startswith(case + "_")}
    got = run(eng, rec["pred"], rec["gt"], rec["avail"])
    names = ("ade_mean", "ade_min", "fde_mean", "fde_min", "apd_mean", "apd_max", "fpd_mean", "fpd_max")
    for c, name in enumerate(names):
        err = Y.rel_err(got["per_agent"][:, c], rec[name])
        print(f"{case} {name}: {err:.2e}")
        assert err <= Y.BAR, name
    err = Y.rel_err(got["means"][:8], rec["keys"])
    print(f"{case} keys: {err:.2e}")
    assert err <= Y.BAR
    assert np.array_equal(got["index"][:, 0], np.argmin(rec["ade"], axis=1)) and np.array_equal(got["index"][:, 1], np.argmin(rec["fde"], axis=1))
    assert got["index"][:, 2].tolist() == [51, 25, 0, 51, 0, 51] and not got["index"][:, 3].any()
    check_against_yardstick(got, rec["pred"], rec["gt"], rec["avail"], case)


# N: one sample (no pair), one pair, an odd count, the bench's 20, one whole wave, one more (2,080 pairs: more than one pass of 256
# lanes); N T = 8,164, the last T = 52 shape inside the LDS cap, N T = 8,192 exactly and N = 256, one lane per sample; every T; C = 2
# and 6 (channels 2 .. 5 hold values that must not be read); B = 1, 3 and more than six, so that every availability pattern occurs
SHAPES = [(6, 1, 52, 2), (6, 2, 52, 6), (6, 3, 52, 2), (7, 20, 52, 6), (6, 64, 52, 2), (6, 65, 52, 6), (1, 157, 52, 2), (2, 128, 64, 6),
          (1, 256, 32, 2), (6, 5, 1, 2), (6, 5, 2, 6), (6, 5, 80, 2), (1, 5, 52, 6), (3, 5, 52, 2), (13, 8, 7, 3), (6, 4, 9, 8)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-N%d-T%d-C%d" % s)
def test_the_fp64_yardstick_at_every_shape(eng, shape):
    pred, gt, avail = make(*shape)
    check_against_yardstick(run(eng, pred, gt, avail), pred, gt, avail, str(shape))


@pytest.mark.parametrize("scale", [1e-3, 100.0])
def test_the_fp64_yardstick_at_other_scales(eng, scale):
    pred, gt, avail = make(6, 20, 52, 2, seed=3, scale=scale)
    check_against_yardstick(run(eng, pred, gt, avail), pred, gt, avail, f"scale {scale}")


@pytest.mark.parametrize("extra", [-1, 0, 1, 300])
def test_the_second_grid_stride_pass(eng, extra):
    """B on either side of the workgroup cap: agents beyond it are taken in a second pass and the partials of the batch mean by a
    second round of the fold's grid; rows, indices and means still meet the yardstick, and the means the replayed fold bit for bit."""
    B = cap() + extra
    pred, gt, avail = make(B, 3, 2, 2, seed=5)
    got = run(eng, pred, gt, avail)
    check_against_yardstick(got, pred, gt, avail, f"B = {B}")
    # padding with repeats of agent 0: the rows are the same bits, and the mean moves exactly as the yardstick's does
    k = 7
    padded = [np.concatenate([x, np.repeat(x[:1], k, axis=0)]) for x in (pred, gt, avail)]
    gp = run(eng, *padded)
    assert np.array_equal(bits(gp["per_agent"][:B]), bits(got["per_agent"])) and np.array_equal(bits(gp["per_agent"][B:]), bits(np.repeat(got["per_agent"][:1], k, axis=0)))
    ref = Y.metrics(pred, gt, avail)["per_agent"]
    want = (ref.sum(axis=0) + k * ref[0]) / (B + k)
    assert Y.rel_err(gp["means"], want) <= Y.BAR64


def test_the_reach_is_refused_and_the_last_shape_inside_it_runs(eng):
    """N = 157 at T = 52 (8,164 points) runs (SHAPES); N = 158 (8,216) and N = 257 are refused: CLD_ERR_ARG, no other path."""
    from cld_amd._lib import CldError
    for N, T in ((158, 52), (257, 1), (1, 8193)):
        pred, gt, avail = make(1, N, T)
        with pytest.raises(CldError, match="beyond"):
            run(eng, pred, gt, avail)
    pred, gt, avail = make(2, 1, 8192)
    check_against_yardstick(run(eng, pred, gt, avail), pred, gt, avail, "T = 8192")


def test_bool_and_float_availabilities_and_the_state_action_layout(eng):
    """avail as bool gives the bits of avail as float; pred [B,N,T,6] is read in place and gives the bits of its [..., :2] copy."""
    pred, gt, avail = make(7, 20, 52, 6, seed=9)
    a = run(eng, pred, gt, avail)
    out_b = eng.sample_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(avail > 0).cuda())
    out_2 = eng.sample_metrics(torch.from_numpy(np.ascontiguousarray(pred[..., :2])), gt, avail)
    for o in (out_b, out_2):
        assert np.array_equal(bits(o["per_agent"].cpu().numpy()), bits(a["per_agent"])) and np.array_equal(o["index"].cpu().numpy(), a["index"])
        assert np.array_equal(bits(o["means"].cpu().numpy()), bits(a["means"]))
    unread = pred.copy()
    unread[..., 2:4], unread[..., 4:] = np.nan, np.inf                       # channels the metrics do not read: no flag, the same bits
    u = run(eng, unread, gt, avail)
    assert not u["index"][:, 3].any() and np.array_equal(bits(u["per_agent"]), bits(a["per_agent"]))


# ---------------------------------------------------------------- decisions on exactly representable inputs
def test_decisions_on_dyadic_inputs(eng):
    T = 4
    gt = np.zeros((3, T, 2), np.float32)
    pred = np.zeros((3, 4, T, 2), np.float32)
    pred[:, 0, :, 0], pred[:, 1, :, 0], pred[:, 2, :, 0], pred[:, 3, :, 1] = 2.0, 0.5, 0.75, -0.5      # ade 2, 0.5, 0.75, 0.5: samples 1 and 3 tie
    pred[1, 1] = pred[1, 0]                                                                          # agent 1: samples 0 and 1 identical
    avail = np.ones((3, T), np.float32)
    avail[2] = 0                                                                                     # agent 2: nothing available
    got = run(eng, pred, gt, avail)
    rows, idx = got["per_agent"], got["index"]
    assert idx[0].tolist() == [1, 1, T - 1, 0]                               # the first of the tied samples
    assert rows[0, :4].tolist() == [(2 + 0.5 + 0.75 + 0.5) / 4, 0.5, (2 + 0.5 + 0.75 + 0.5) / 4, 0.5]
    ref = Y.metrics(pred, gt, avail)
    assert np.array_equal(rows[:, :4], ref["per_agent"][:, :4])             # sums of dyadic values: exact in any order
    assert Y.rel_err(rows, ref["per_agent"]) <= Y.BAR64
    assert np.array_equal(idx, ref["index"])
    # two identical samples: their pair distance is exactly 0, and the best index is the first of them
    one = run(eng, np.ascontiguousarray(pred[1:2, :2]), gt[1:2], avail[1:2])
    assert not one["per_agent"][0, 4:].any() and one["index"][0].tolist() == [0, 0, T - 1, 0]
    # nothing available: last = 0, every error exactly 0, best index 0; the diversity ignores avail
    assert idx[2].tolist() == [0, 0, 0, 0] and not rows[2, :4].any() and np.array_equal(rows[2, 4:], rows[0, 4:])


# ---------------------------------------------------------------- determinism
def test_same_bits_on_every_run_alone_in_a_batch_and_under_permutation(eng):
    B = cap() + 5
    pred, gt, avail = make(B, 20, 13, 2, seed=11)
    a, b = run(eng, pred, gt, avail), run(eng, pred, gt, avail)
    for k in ("per_agent", "means"):
        assert np.array_equal(bits(a[k]), bits(b[k]))
    assert np.array_equal(a["index"], b["index"])
    for r in (0, 1, cap() - 1, cap(), B - 1):                                # a first-pass and a second-pass agent, alone (B = 1)
        alone = run(eng, pred[r:r + 1], gt[r:r + 1], avail[r:r + 1])
        assert np.array_equal(bits(alone["per_agent"][0]), bits(a["per_agent"][r])) and np.array_equal(alone["index"][0], a["index"][r])
        assert np.array_equal(bits(alone["means"]), bits(a["per_agent"][r]))                          # the mean of one row is the row
    perm = np.random.default_rng(1).permutation(B)
    p = run(eng, pred[perm], gt[perm], avail[perm])
    assert np.array_equal(bits(p["per_agent"]), bits(a["per_agent"][perm])) and np.array_equal(p["index"], a["index"][perm])


def test_both_precision_modes_give_the_same_bits():
    from cld_amd.engine import Engine
    pred, gt, avail = make(7, 20, 52, 6, seed=13)
    res = [run(Engine(n_timesteps=10, device="cuda:0", precision=p), pred, gt, avail) for p in ("f32", "f16x2")]
    assert all(np.array_equal(bits(res[0][k]), bits(res[1][k])) for k in ("per_agent", "means")) and np.array_equal(res[0]["index"], res[1]["index"])


# ---------------------------------------------------------------- non-finite input
@pytest.mark.parametrize("where", ["pred", "pred_inf", "gt", "avail"])
def test_a_non_finite_value_flags_its_agent_alone(eng, where):
    from cld_amd.metrics import SampleMetrics
    pred, gt, avail = make(7, 5, 52, 6, seed=17)
    clean = run(eng, pred, gt, avail)
    assert not clean["index"][:, 3].any()
    pred, gt, avail = pred.copy(), gt.copy(), avail.copy()
    if where == "pred":
        pred[3, 2, 40, 1] = np.nan
    elif where == "pred_inf":
        pred[3, 4, 51, 0] = np.inf
    elif where == "gt":
        gt[3, 7, 0] = np.nan
    else:
        avail[3, 51] = np.nan
    got = run(eng, pred, gt, avail)
    assert got["index"][:, 3].tolist() == [0, 0, 0, 1, 0, 0, 0]
    keep = [0, 1, 2, 4, 5, 6]
    assert np.array_equal(bits(got["per_agent"][keep]), bits(clean["per_agent"][keep])) and np.array_equal(got["index"][keep], clean["index"][keep])
    m = SampleMetrics(eng)
    m.add(pred, gt, avail)
    with pytest.raises(ValueError, match="non-finite"):
        m.compute()


# ---------------------------------------------------------------- status codes
def test_status_codes(eng):
    lib, h = eng.lib, eng._h
    B, N, T, Cc = 300, 4, 6, 2
    dev = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda:0")
    pred, gt, avail = dev(B, 158, 52, 2), dev(B, 52, 2), dev(B, 52)          # large enough for every shape tried below
    rows, idx, means, ws = dev(B, 10, dt=torch.float64), dev(B, 4, dt=torch.int32), dev(10, dt=torch.float64), dev(64, dt=torch.float64)
    need = int(lib.cld_sample_metrics_workspace_bytes(B))
    assert need == 2 * 10 * 8 and ws.numel() * 8 >= need
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(pred=pred, Cc=Cc, gt=gt, avail=avail, B=B, N=N, T=T, rows=rows, idx=idx, means=means, ws=P(ws), wsn=512):
        rc = lib.cld_sample_metrics(h, P(pred), Cc, P(gt), P(avail), B, N, T, P(rows), P(idx), P(means), ws, wsn, None)
        torch.cuda.synchronize()
        return rc

    assert call() == OK
    assert call(means=None, ws=None, wsn=0) == OK                            # no means: no workspace
    for name in ("pred", "gt", "avail", "rows", "idx"):
        assert call(**{name: None}) == ERR_ARG, name
    assert b"null" in lib.cld_last_error(h)
    assert lib.cld_sample_metrics(None, P(pred), Cc, P(gt), P(avail), B, N, T, P(rows), P(idx), P(means), P(ws), 512, None) == ERR_ARG
    for kw in (dict(N=0), dict(T=0), dict(B=0), dict(N=-1), dict(B=(1 << 20) + 1), dict(Cc=1), dict(Cc=9), dict(N=158, T=52, B=1), dict(N=257, T=1, B=1),
               dict(N=1, T=8193, B=1)):
        assert call(**kw) == ERR_ARG, kw
    assert call(N=157, T=52, B=1) == OK
    assert call(ws=None) == ERR_WORKSPACE and call(wsn=need - 1) == ERR_WORKSPACE and call(wsn=0) == ERR_WORKSPACE
    assert call(ws=C.c_void_p(ws.data_ptr() + 4)) == ERR_WORKSPACE
    assert b"workspace" in lib.cld_last_error(h)
    assert call(wsn=need) == OK


# ---------------------------------------------------------------- the accumulator
def test_sample_metrics_accumulates_grows_and_answers_with_upstreams_keys(eng):
    from cld_amd.metrics import SampleMetrics, compute_sample_metrics
    p1, g1, a1 = make(5, 20, 52, 6, seed=21)
    p2, g2, a2 = make(9, 20, 52, 6, seed=22)
    m = SampleMetrics(eng, capacity=4)
    with pytest.raises(ValueError, match="nothing"):
        m.compute()
    m.add(p1, g1, a1)
    m.add(torch.from_numpy(p2).cuda(), torch.from_numpy(g2).cuda(), torch.from_numpy(a2 > 0).cuda())
    assert m.per_agent().shape == (14, 10) and m.index().shape == (14, 4) and m._rows.shape[0] >= 14          # grown past the capacity of 4
    whole = SampleMetrics(eng, capacity=32)
    whole.add(np.concatenate([p1, p2]), np.concatenate([g1, g2]), np.concatenate([a1, a2]))
    assert whole._rows.shape[0] == 32
    assert np.array_equal(bits(m.per_agent().cpu().numpy()), bits(whole.per_agent().cpu().numpy()))
    assert np.array_equal(m.index().cpu().numpy(), whole.index().cpu().numpy())
    ref = Y.metrics(np.concatenate([p1, p2]), np.concatenate([g1, g2]), np.concatenate([a1, a2]))
    got = m.compute()
    assert tuple(got) == Y.COLS and all(v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda for v in got.values())
    assert Y.rel_err([float(got[k]) for k in Y.COLS], ref["means"]) <= Y.BAR64
    # the last batch alone: upstream's _compute_metrics, in upstream's dict layout
    last = m.last_batch()
    one = compute_sample_metrics(eng, {"predictions": {"positions": torch.from_numpy(p2[..., :2].copy())}},
                                 {"target_positions": torch.from_numpy(g2), "target_availabilities": torch.from_numpy(a2 > 0)})
    assert tuple(last) == tuple(one) == Y.UPSTREAM_KEYS
    assert all(np.array_equal(bits(last[k].cpu().numpy()), bits(one[k].cpu().numpy())) for k in Y.UPSTREAM_KEYS)
    assert Y.rel_err([float(last[k]) for k in Y.UPSTREAM_KEYS], Y.metrics(p2, g2, a2)["means"][:8]) <= Y.BAR64
    m.reset()
    assert m.per_agent().shape == (0, 10)
    m.add(p1, g1, a1)
    assert np.array_equal(bits(m.per_agent().cpu().numpy()), bits(whole.per_agent()[:5].cpu().numpy()))
