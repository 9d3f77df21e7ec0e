"""Record tests/golden/sample_metrics.npz from the reference's own open-loop metrics (src/tbsim/utils/metrics.py:201-358:
batch_average_displacement_error, batch_final_displacement_error, batch_average_diversity, batch_final_diversity), called the way
DiffuserTrafficModel._compute_metrics calls them (src/tbsim/algos/algos.py:1818-1852), on the CPU.

    python tests/tools/record_sample_metrics_golden.py          (needs the reference tree, see oracle/_refimport.py)

B = 6 agents, T = 52 steps, numpy float32 inputs as the trainer passes them: seeded cumulative-sum trajectories of O(10 m)
(sample_metrics_yardstick.trajectories), one availability pattern per agent (sample_metrics_yardstick.availability_patterns: all ones,
the tail cut at 26, none, a hole at 13..25, only step 0, only step 51).  Two cases: `n5` with N = 5 samples, `n1` with N = 1 (its only
sample is sample 0 of `n5`).  Stored per case: the inputs, the eight keys, every per-agent array the four functions return
([B] each; ADE in "mean" mode returns the batch scalar only, so its per-agent array is the function on one agent at a time), and
ade / fde per SAMPLE [B,N]: the same two functions on one sample at a time (N = 1, where "oracle" is that sample's value).  `meta`
holds the error of the reference's float32 results against the float64 yardstick."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import _refimport                          # noqa: E402
from tests import sample_metrics_yardstick as Y        # noqa: E402

B, N, T, SEED = 6, 5, 52, 20261021


def record(M, pred, gt, avail):
    """One case through the reference's functions -> arrays."""
    n = pred.shape[1]
    conf = np.ones(pred.shape[0:2]) / float(n)                      # as _compute_metrics forms it
    one = np.ones((1, n)) / float(n)
    out = {"pred": pred, "gt": gt, "avail": avail}
    out["ade_mean"] = np.array([M.batch_average_displacement_error(gt[b:b + 1], pred[b:b + 1], one, avail[b:b + 1], "mean") for b in range(B)])
    out["ade_min"] = M.batch_average_displacement_error(gt, pred, conf, avail, "oracle")
    out["fde_mean"] = M.batch_final_displacement_error(gt, pred, conf, avail, "mean")
    out["fde_min"] = M.batch_final_displacement_error(gt, pred, conf, avail, "oracle")
    out["apd_mean"] = M.batch_average_diversity(gt, pred, conf, avail, "mean")
    out["apd_max"] = M.batch_average_diversity(gt, pred, conf, avail, "max")
    out["fpd_mean"] = M.batch_final_diversity(gt, pred, conf, avail, "mean")
    out["fpd_max"] = M.batch_final_diversity(gt, pred, conf, avail, "max")
    c1 = np.ones((B, 1))
    out["ade"] = np.stack([M.batch_average_displacement_error(gt, pred[:, k:k + 1], c1, avail, "oracle") for k in range(n)], axis=1)
    out["fde"] = np.stack([M.batch_final_displacement_error(gt, pred[:, k:k + 1], c1, avail, "oracle") for k in range(n)], axis=1)
    keys = {"ego_avg_ADE": M.batch_average_displacement_error(gt, pred, conf, avail, "mean").mean(), "ego_min_ADE": out["ade_min"].mean(),
            "ego_avg_FDE": out["fde_mean"].mean(), "ego_min_FDE": out["fde_min"].mean(),
            "ego_avg_APD": out["apd_mean"].mean(), "ego_max_APD": out["apd_max"].mean(),
            "ego_avg_FPD": out["fpd_mean"].mean(), "ego_max_FPD": out["fpd_max"].mean()}
    assert tuple(keys) == Y.UPSTREAM_KEYS
    out["keys"] = np.array([keys[k] for k in Y.UPSTREAM_KEYS], dtype=np.float64)
    return out


def main():
    _refimport.install()
    with _refimport.redirect_stdout(_refimport.io.StringIO()):
        import tbsim.utils.metrics as M
    rng = np.random.default_rng(SEED)
    pred, gt = Y.trajectories(rng, B, N, T)
    avail = Y.availability_patterns(T)
    arrays, errs = {}, {}
    for case, p in (("n5", pred), ("n1", np.ascontiguousarray(pred[:, :1]))):
        rec = record(M, p, gt, avail)
        y = Y.metrics(p, gt, avail)
        per_agent = np.stack([rec[k] for k in ("ade_mean", "ade_min", "fde_mean", "fde_min", "apd_mean", "apd_max", "fpd_mean", "fpd_max")], axis=1)
        errs[case] = dict(keys=Y.rel_err(rec["keys"], y["means"][:8]), per_agent=Y.rel_err(per_agent, y["per_agent"][:, :8]),
                          ade=Y.rel_err(rec["ade"], y["ade"]), fde=Y.rel_err(rec["fde"], y["fde"]))
        print(case, {k: float(v) for k, v in zip(Y.UPSTREAM_KEYS, rec["keys"])}, "\n   float32 reference against the float64 yardstick:", errs[case])
        arrays.update({f"{case}_{k}": np.ascontiguousarray(v) for k, v in rec.items()})
    meta = dict(B=B, N=N, T=T, seed=SEED, cases=["n5", "n1"], keys=list(Y.UPSTREAM_KEYS), ref_err=errs, numpy=np.__version__,
                generator="tests/tools/record_sample_metrics_golden.py",
                source="the reference's batch_average_displacement_error, batch_final_displacement_error, batch_average_diversity, batch_final_diversity")
    path = os.path.join(ROOT, "tests", "golden", "sample_metrics.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f"sample_metrics: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
