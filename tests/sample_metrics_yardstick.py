"""A numpy float64 restatement of the open-loop sample metrics (include/cld_eval.h `cld_sample_metrics`; upstream:
src/tbsim/utils/metrics.py:201-358 as DiffuserTrafficModel._compute_metrics calls them), written from the formulas, not from upstream's
code: the yardstick of the kernel tests and of the recording tests/golden/sample_metrics.npz.

    pred [B,N,T,C >= 2] (channels 0, 1 = x, y), gt [B,T,2], avail [B,T] bool or float
    e[b,n,t] = sqrt(sum_c ((gt - pred) * avail)^2)        an unavailable step contributes 0 and still counts in the mean over T
    ade[b,n] = mean_t e;  last[b] = max_t((avail > 0) * t);  fde[b,n] = e[b,n,last[b]]
    apd[b,i,j] = mean_t |pred_i - pred_j|                 avail ignored
    fpd[b,i,j] = sqrt(sum_t (y_i - y_j)^2)                upstream's quirk: the last COORDINATE and the norm over time
    lpd[b,i,j] = |pred_i[T-1] - pred_j[T-1]|              the distance at the last time step (this library's two extra columns)

`VARIANTS` are deliberate mis-statements (mutants): tests/test_sample_metrics_host.py shows that each of them misses the recorded cases
by more than the bar, which is what makes the cases worth running against the kernel."""
import numpy as np

COLS = ("ego_avg_ADE", "ego_min_ADE", "ego_avg_FDE", "ego_min_FDE", "ego_avg_APD", "ego_max_APD", "ego_avg_FPD", "ego_max_FPD",
        "ego_avg_last_step_PD", "ego_max_last_step_PD")
UPSTREAM_KEYS = COLS[:8]
VARIANTS = ("avail_count", "last_step", "fpd_last_step", "pair_unbiased", "max_mean_swapped", "last_tie", "avail_ignored")
BAR = 2e-6          # upstream's float32 path against float64: at most 4 roundings per norm and a pairwise mean over T <= 256 of
                    # non-negative terms, under 8 * 2^-23 ~ 1e-6 relative
BAR64 = 1e-12       # the fp64 kernel against this file: at most T + 4 roundings per value, ~6e-14 at T = 256; the margin covers FMA
                    # contraction and the order of the folds


def availability_patterns(T):
    """The six availability rows of the recording, for any T: all ones, the tail cut at T/2, none, a hole over the second quarter,
    only step 0, only step T - 1."""
    a = np.zeros((6, T), np.float32)
    a[0] = 1
    a[1, :T // 2] = 1
    a[3] = 1
    a[3, T // 4:T // 2] = 0
    a[4, 0] = 1
    a[5, T - 1] = 1
    return a


def trajectories(rng, B, N, T, C=2, scale=10.0):
    """Seeded cumulative-sum trajectories of O(scale) metres: gt [B,T,2] and N samples around it, pred [B,N,T,C] (channels >= 2 are
    filled with values the metrics must not read)."""
    gt = np.cumsum(rng.normal(0.0, scale / np.sqrt(T), (B, T, 2)), axis=1)
    pred = gt[:, None] + np.cumsum(rng.normal(0.0, 0.3 * scale / np.sqrt(T), (B, N, T, 2)), axis=2)
    if C > 2:
        pred = np.concatenate([pred, rng.normal(0.0, 50.0, (B, N, T, C - 2))], axis=-1)
    return pred.astype(np.float32), gt.astype(np.float32)


def metrics(pred, gt, avail, variant=None):
    """-> dict: per_agent [B,10] float64 (columns COLS), index [B,4] int64 (best_ade, best_fde, last, nonfinite), means [10], and the
    intermediate arrays ade, fde [B,N], apd, fpd, lpd [B,N,N]."""
    assert variant is None or variant in VARIANTS, variant
    pred = np.asarray(pred)
    B, N, T = pred.shape[:3]
    p = pred[..., :2].astype(np.float64)
    g = np.asarray(gt).astype(np.float64)
    a = np.asarray(avail).astype(np.float64)
    assert g.shape == (B, T, 2) and a.shape == (B, T)
    w = np.ones_like(a) if variant == "avail_ignored" else a
    e = np.sqrt((((g[:, None] - p) * w[:, None, :, None]) ** 2).sum(axis=-1))                      # [B,N,T]
    if variant == "avail_count":
        ade = e.sum(axis=-1) / np.maximum((a > 0).sum(axis=-1), 1)[:, None]
    else:
        ade = e.sum(axis=-1) / T
    last = ((a > 0) * np.arange(T)).max(axis=-1)
    at = np.full(B, T - 1) if variant == "last_step" else last
    fde = e[np.arange(B), :, at]                                                                   # [B,N]
    diff = p[:, :, None] - p[:, None, :]                                                           # [B,N,N,T,2]
    apd = np.sqrt((diff ** 2).sum(axis=-1)).sum(axis=-1) / T
    lpd = np.sqrt((diff[:, :, :, -1] ** 2).sum(axis=-1))
    fpd = lpd if variant == "fpd_last_step" else np.sqrt((diff[..., 1] ** 2).sum(axis=-1))
    pairs = float(max(N * (N - 1), 1)) if variant == "pair_unbiased" else float(N * N)

    def mean_max(d):
        m, x = d.reshape(B, -1).sum(axis=-1) / pairs, d.reshape(B, -1).max(axis=-1)
        return (x, m) if variant == "max_mean_swapped" else (m, x)

    def argmin(v):
        return N - 1 - np.argmin(v[:, ::-1], axis=1) if variant == "last_tie" else np.argmin(v, axis=1)

    cols = [ade.sum(axis=1) / N, ade.min(axis=1), fde.sum(axis=1) / N, fde.min(axis=1), *mean_max(apd), *mean_max(fpd), *mean_max(lpd)]
    per_agent = np.stack(cols, axis=1)
    bad = ~(np.isfinite(p).all(axis=(1, 2, 3)) & np.isfinite(g).all(axis=(1, 2)) & np.isfinite(a).all(axis=1))
    index = np.stack([argmin(ade), argmin(fde), last, bad.astype(np.int64)], axis=1)
    return dict(per_agent=per_agent, index=index, means=per_agent.sum(axis=0) / B, ade=ade, fde=fde, apd=apd, fpd=fpd, lpd=lpd, last=last)


def keys(res):
    """Upstream's eight keys of a `metrics` result: the batch means of columns 0 .. 7."""
    return {k: float(res["means"][c]) for c, k in enumerate(UPSTREAM_KEYS)}


def rel_err(got, want):
    """The largest |got - want| / |want| over the elements; where `want` is exactly 0, `got` must be exactly 0 too (inf otherwise)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    zero = want == 0
    if (got[zero] != 0).any():
        return float("inf")
    return float(np.max(np.abs(got - want)[~zero] / np.abs(want[~zero]), initial=0.0))
