"""Record tests/golden/realism.npz: the reference's realism deviation (src/trainers/guide_dm_trainer.py:222-247, 270-281) of two small
cases, evaluated as the reference evaluates it -- torch on the CPU for the six flattened arrays, scipy.stats.wasserstein_distance for
the three distances.  Needs scipy:  python -m tests.tools.record_realism_golden
The inputs are tests/realism_cases.golden_inputs(): "eq" (16 rows against 16) and "uneq" (the same 16 against 11: scipy's unequal-size form; its ground-truth side is stored once, under "eq").
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import realism_cases as RC  # noqa: E402


def flat_terms(state_and_action: torch.Tensor, dt: float):
    """test_step's lines, on one side."""
    long_acc = state_and_action[..., 4]
    lat_acc = state_and_action[..., 2] * state_and_action[..., 5]
    jerk = (long_acc[:, 1:] - long_acc[:, :-1]) / dt
    return [x.detach().cpu().numpy().flatten() for x in (long_acc, lat_acc, jerk)]


def main():
    from scipy.stats import wasserstein_distance
    import scipy
    out = {}
    for case, (sa_gt, sa_pred) in RC.golden_inputs().items():
        gt, pred = flat_terms(torch.from_numpy(sa_gt), RC.DT), flat_terms(torch.from_numpy(sa_pred), RC.DT)
        wd = [float(wasserstein_distance(g, p)) for g, p in zip(gt, pred)]
        out[f"{case}_sa_gt"], out[f"{case}_sa_pred"] = sa_gt, sa_pred
        for n, g, p in zip(RC.NAMES, gt, pred):
            out[f"{case}_{n}_gt"], out[f"{case}_{n}_pred"] = g, p
        out[f"{case}_wd"] = np.array(wd, np.float64)                                  # wd_long, wd_lat, wd_jerk
        out[f"{case}_realism_deviation"] = np.array((wd[0] + wd[1] + wd[2]) / 3.0, np.float64)
        print(case, sa_gt.shape, sa_pred.shape, "wd", wd, "realism_deviation", float(out[f"{case}_realism_deviation"]))
    meta = {"reference": "guide_dm_trainer.py:222-247 in torch (CPU), scipy.stats.wasserstein_distance", "scipy": scipy.__version__,
            "torch": torch.__version__, "dt": RC.DT}
    for k in [k for k in out if k.startswith("uneq_") and k.endswith("_gt")]:
        assert np.array_equal(out[k], out[k[2:]])
        del out[k]
    np.savez_compressed(RC.GOLDEN, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **out)
    print("wrote", RC.GOLDEN, os.path.getsize(RC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
