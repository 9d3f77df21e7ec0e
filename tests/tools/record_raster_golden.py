"""Record tests/golden/rasterize_agents.npz from the reference's own rasterize_agents (src/tbsim/utils/trajdata_utils.py:123-156).

Run where the reference tree is present:  python -m tests.tools.record_raster_golden
The inputs come from tests/raster_cases.golden_case(): the first agent of each scene stands at the world origin with heading 0, so
the world-frame histories ARE the agent-frame histories rasterize_agents expects for that agent.  Stored: the inputs and the 31
history planes of each scene's first agent as int8 (their values are -1, 0, 1).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import _refimport  # noqa: E402
from tests import raster_cases as RC  # noqa: E402


def main():
    _refimport.install()
    from tbsim.utils.trajdata_utils import rasterize_agents
    case = RC.golden_case()
    cfg = case["cfg"]
    H, W = cfg["height"], cfg["width"]
    ox, oy = RC.offsets(cfg)
    rfa = torch.tensor([[[cfg["px_per_m"], 0.0, ox], [0.0, cfg["px_per_m"], oy], [0.0, 0.0, 1.0]]], dtype=torch.float32)
    ss = case["scene_start"]
    planes = []
    for s in range(len(ss) - 1):
        hw = torch.from_numpy(case["hist_world"][ss[s]:ss[s + 1]])[None]                  # [1,A,T,3], agent 0 = the ego
        mask = torch.from_numpy(case["hist_avail"][ss[s]:ss[s + 1]] != 0)[None]
        out = rasterize_agents(torch.zeros(1, cfg["n_sem"], H, W), hw[..., :2].contiguous(), hw[..., 2:].contiguous(), mask, rfa, None)
        hist = out[0, :hw.shape[2]]
        assert set(np.unique(hist.numpy()).tolist()) <= {-1.0, 0.0, 1.0}
        planes.append(hist.numpy().astype(np.int8))
    meta = {"cfg": {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, "source": "tbsim.utils.trajdata_utils.rasterize_agents"}
    path = os.path.join(ROOT, "tests", "golden", "rasterize_agents.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), hist_world=case["hist_world"],
                        hist_avail=case["hist_avail"], scene_start=case["scene_start"], planes=np.stack(planes))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
