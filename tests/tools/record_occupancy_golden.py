"""Record tests/golden/occupancy.npz from the reference's own OccupancyCoverage and OccupancyDiversity (src/tbsim/envs/env_metrics.py:977-1218).

Run where the reference tree is present:  python -m tests.tools.record_occupancy_golden
The inputs are tests/occupancy_cases.build_case()'s `world_full` (every agent present; the default windows drop nothing) and `failed`.
Per step the classes get, for every agent, the drivable raster and raster_from_world raster_cases.restate builds for an agent standing at
its pose (occupancy_cases.RASTER: 64 x 64 at 2 px / m, the agent in the middle, so every grid point an agent writes lies inside its raster).
batch_utils().get_drivable_region_map is replaced by a function handing those rasters through, and OffRoadRate.compute_per_step /
CollisionRate.compute_per_step -- the calls inside CriticalFailure.add_step -- by functions returning the case's failed sets (an agent
that fails is off road at its first step), as record_metrics_golden.py patches them.  pyemd is not available: EM.emd is replaced by a
recorder that keeps every distr_i, distr_j and distance_matrix OccupancyDiversity passes to it.

Recorded: per scene the cells, values and lane flags of the coverage grid after both episodes and the three counts; per scene and
episode the cells, values and lane flags of the diversity grids; the recorder's arguments per scene (the distance matrix of a scene once:
the tool checks every pair of the scene passed the same one; it is stored as the integer squares of its upper triangle, "emd_s*_D2", after checking that it is symmetric with a zero diagonal
and that their float64 square root is the matrix bit for bit, which keeps the file small; occupancy_cases.distance_matrix undoes it) with the order of the cells they refer to.
Two assertions, either of which fails the recording: every writer of a cell saw the same lane flag, and that flag is the one
occupancy_cases.lane_of states for the cell."""
import json
import os
import sys
from collections import defaultdict
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import _refimport  # noqa: E402
from tests import occupancy_cases as OC  # noqa: E402
from tests import raster_cases as RC  # noqa: E402


def rasters(case, world_t):
    """raster_cases.restate for every agent standing at world_t [B,3] (a one-frame history) -> (drivable [B,H,W], raster_from_world [B,3,3])."""
    w = world_t.astype(np.float32)
    rc = dict(hist_world=w[:, None], hist_avail=np.ones((w.shape[0], 1), np.uint8), scene_start=case["scene_start"],
              cfg=dict(RC.DEFAULTS, **OC.RASTER), maps=case["maps"], scene_map=case["scene_map"], map_from_world=case["map_from_world"])
    r = RC.restate(rc)
    return r["drivable"], r["raster_from_world"]


class Logged(defaultdict):
    """OccupancyGrid.occupancy_grid with a log of the keys read: get_multi_episode_metrics reads every key of the union, in its order."""

    def __init__(self):
        super().__init__(lambda: 0)
        self.log = []

    def __getitem__(self, key):
        self.log.append(key)
        return super().__getitem__(key)


class Watch(dict):
    """OccupancyGrid.lane_flag with a record of every flag written per cell."""

    def __init__(self):
        super().__init__()
        self.seen = {}

    def __missing__(self, key):
        return 0

    def __setitem__(self, key, value):
        self.seen.setdefault(key, set()).add(int(value))
        super().__setitem__(key, value)


def main():
    _refimport.install()
    for n in ("transforms3d", "transforms3d.euler", "pyemd"):
        m = MagicMock(name=n)
        m.__path__ = []
        sys.modules[n] = m
    import tbsim.envs.env_metrics as EM
    case = OC.build_case()
    ss, world, failed = case["scene_start"], case["world_full"], case["failed"]
    E, T, B = world.shape[:3]
    S = len(ss) - 1
    scene = RC.scene_of_rows(ss, B)
    cov_cfg, div_cfg = OC.GRIDS["coverage"], OC.GRIDS["diversity"]
    gridinfo = lambda c: {"offset": np.array(c["offset"], np.float64), "step": np.array(c["step"], np.float64)}
    calls = []

    def record_emd(distr_i, distr_j, distance_matrix):
        calls.append((np.array(distr_i), np.array(distr_j), np.array(distance_matrix)))
        return 0.0

    class Grid(EM.OccupancyGrid):
        def __init__(self, gridinfo, sigma=1.0):
            super().__init__(gridinfo, sigma)
            self.lane_flag = Watch()
            self.occupancy_grid = Logged()

    stub = MagicMock()
    stub.get_drivable_region_map = lambda image: image
    saved = (EM.OffRoadRate.compute_per_step, EM.CollisionRate.compute_per_step, EM.batch_utils, EM.emd, EM.OccupancyGrid)
    try:
        EM.OffRoadRate.compute_per_step = staticmethod(lambda si, asi: si["_off"])
        EM.CollisionRate.compute_per_step = staticmethod(lambda si, asi: (si["_coll"], None))
        EM.batch_utils, EM.emd, EM.OccupancyGrid = (lambda: stub), record_emd, Grid
        cov = EM.OccupancyCoverage(gridinfo(cov_cfg), sigma=cov_cfg["sigma"], threshold=OC.THRESHOLD)
        div = EM.OccupancyDiversity(gridinfo(div_cfg), sigma=div_cfg["sigma"])
        cov.multi_episode_reset()
        div.multi_episode_reset()
        for e in range(E):
            cov.reset()
            div.reset()
            for t in range(T):
                w = world[e, t].astype(np.float64)
                drv, rfw = rasters(case, world[e, t])
                si = dict(scene_index=scene, track_id=np.arange(B), centroid=w[:, :2], yaw=w[:, 2], image=drv, raster_from_world=rfw,
                          _off=(failed[e] != 0) & (t == 0), _coll={"coll_any": np.zeros(B)})
                cov.add_step(si, np.arange(S))
                div.add_step(si, np.arange(S))
            div.get_episode_metrics()
            print("episode", e, "fed", flush=True)
        counts = cov.get_multi_episode_metrics()
        for grids in div.og.values():
            for og in grids:
                og.occupancy_grid.log.clear()
        div.get_multi_episode_metrics()
    finally:
        EM.OffRoadRate.compute_per_step, EM.CollisionRate.compute_per_step = staticmethod(saved[0]), staticmethod(saved[1])
        EM.batch_utils, EM.emd, EM.OccupancyGrid = saved[2:]

    out = {k: case[k] for k in OC.INPUT_KEYS}
    out["cov_counts"] = np.stack([counts["total"], counts["onroad"], counts["success"]], 1).astype(np.int64)

    def dump(prefix, og, cfg, s):
        # (get_multi_episode_metrics reads the union's keys from every episode's defaultdict, which inserts the missing ones: written cells only)
        keys = [k for k in og.occupancy_grid.keys() if k in og.lane_flag.seen]
        cells = np.array(keys, np.int64).reshape(-1, 2)
        lane = np.array([og.lane_flag[k] for k in keys], np.uint8)
        for k in keys:                                               # the two assertions of the recording
            assert len(og.lane_flag.seen[k]) == 1, (prefix, k, og.lane_flag.seen[k])
        assert np.array_equal(lane != 0, OC.lane_of(case, cfg, s, cells)), prefix
        out[prefix + "_cells"], out[prefix + "_lane"] = cells.astype(np.int32), lane
        out[prefix + "_values"] = np.array([dict.get(og.occupancy_grid, k) for k in keys], np.float64)      # (not through the log)

    for s in range(S):
        dump(f"cov_s{s}", cov.og[s], cov_cfg, s)
        for e in range(E):
            dump(f"div_s{s}_e{e}", div.og[s][e], div_cfg, s)
    # the recorder: OccupancyDiversity walks the scenes in order and, per scene, episode i against every earlier j
    pairs = [(i, j) for i in range(E) for j in range(i)]
    assert len(calls) == S * len(pairs)
    for s in range(S):
        mine = calls[s * len(pairs):(s + 1) * len(pairs)]
        order = div.og[s][0].occupancy_grid.log                       # the order upstream iterated the union in
        assert all(og.occupancy_grid.log == order for og in div.og[s]) and len(set(order)) == len(order) == mine[0][2].shape[0]
        out[f"emd_s{s}_cells"] = np.array(order, np.int32).reshape(-1, 2)
        assert all(np.array_equal(c[2], mine[0][2]) for c in mine)
        # the matrix is kept as its squares, which are integers (the cell points are integers), and is their square root bit for bit
        # (and symmetric with a zero diagonal: the upper triangle, row by row)
        D = mine[0][2]
        D2 = np.rint(D ** 2).astype(np.uint16)
        assert np.array_equal(np.sqrt(D2.astype(np.float64)), D) and np.array_equal(D, D.T) and not D.diagonal().any()
        out[f"emd_s{s}_D2"] = D2[np.triu_indices(D.shape[0], 1)]
        for (i, j), c in zip(pairs, mine):
            out[f"emd_s{s}_i{i}"], out[f"emd_s{s}_j{j}"] = c[0], c[1]
    meta = {"reference": "cov_* (cells, values, lane, counts), div_* per scene and episode, emd_* = the arguments of pyemd.emd",
            "grids": {k: OC.GRIDS[k] for k in ("coverage", "diversity")}, "threshold": OC.THRESHOLD, "raster": OC.RASTER,
            "pairs": pairs}
    path = os.path.join(ROOT, "tests", "golden", "occupancy.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **out)
    print("wrote", path, os.path.getsize(path), "bytes; counts", out["cov_counts"].tolist())


if __name__ == "__main__":
    main()
