"""Record tests/golden/rollout_metrics.npz from the reference's own metric code (src/tbsim/envs/env_metrics.py, src/tbsim/utils/metrics.py).

Run where the reference tree is present:  python -m tests.tools.record_metrics_golden
The inputs come from tests/metrics_cases.build_case().  For both rasters (224 x 224 and 64 x 64), from the reference:
  * off_road / off_road_disk per step: Metrics.batch_detect_off_road / batch_detect_off_road_disk on the drivable rasters
    raster_cases.restate builds for every valid agent at every step (centroid at the raster offsets, extents times px_per_m);
  * coll_disk per step: DiskCollisionRate.compute_per_step;
  * the episode values: add_step / get_episode_metrics of OffRoadRate, DiskOffRoadRate, CollisionRate, DiskCollisionRate,
    CriticalFailure and Comfort over the 21 steps, and CriticalFailure.get_per_agent_metrics.
From the float64 restatement (tests/metrics_cases.py), because shapely is not available here: the box collision flags, their type and
partner -- CollisionRate.compute_per_step is replaced by a function returning them for the duration of the recording, which also feeds
the class-level call inside CriticalFailure.add_step; OffRoadRate.compute_per_step / DiskOffRoadRate.compute_per_step are replaced by
functions returning the two Metrics results above.  The per-agent table is the restatement's, except its failure columns.
A second, small episode (metrics_cases.absent_scene_case: a one-agent scene that is NaN throughout beside a two-agent scene, no map) is
recorded the same way under "absent_*": it pins what pandas returns for a scene without a valid record.
"""
import json
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import _refimport  # noqa: E402
from tests import metrics_cases as MC  # noqa: E402
from tests import raster_cases as RC  # noqa: E402


def drivable_rasters(case, cfg, world_t):
    """raster_cases.restate's drivable [B,H,W] for every agent standing at world_t [B,3] (a one-frame history; invalid agents at 0)."""
    w = np.where(np.isnan(world_t), 0.0, world_t).astype(np.float32)
    rc = dict(hist_world=w[:, None], hist_avail=np.ones((w.shape[0], 1), np.uint8), scene_start=case["scene_start"],
              cfg=dict(RC.DEFAULTS, **cfg))
    if case.get("maps") is not None:
        rc.update(maps=case["maps"], scene_map=case["scene_map"], map_from_world=case["map_from_world"])
    return RC.restate(rc)["drivable"]


def record(case, name, cfg, out, EM, Metrics, CollisionType):
    """One episode of `case` on raster `cfg` through the reference's classes -> out[name + "_flags" / "_partner" / "_per_scene" / "_per_agent"]."""
    ss, world, extent = case["scene_start"], case["world"], case["extent"]
    T, B = world.shape[:2]
    S = len(ss) - 1
    scene = RC.scene_of_rows(ss, B)
    ox, oy = RC.offsets(cfg)
    rs = MC.restate(case, cfg)
    classes = dict(off=EM.OffRoadRate(), disk=EM.DiskOffRoadRate(), coll=EM.CollisionRate(), cdisk=EM.DiskCollisionRate(),
                   fail=EM.CriticalFailure(num_offroad_frames=2), comfort=EM.Comfort(sim_dt=MC.SIM_DT, stat_dt=MC.STAT_DT))
    for c in classes.values():
        c.reset()
    flags = np.zeros((T, B, 4), np.uint8)
    for t in range(T):
        w = world[t].astype(np.float64)
        valid = ~(np.isnan(w[:, 0]) | np.isnan(w[:, 1]))
        drv = torch.from_numpy(drivable_rasters(case, cfg, w)[valid])
        cen = torch.tensor([[ox, oy]], dtype=torch.float32).repeat(int(valid.sum()), 1)
        ext = torch.from_numpy(extent[valid, :2]) * cfg["px_per_m"]
        off, disk = np.full(B, np.nan), np.full(B, np.nan)
        off[valid] = Metrics.batch_detect_off_road(cen.clone(), drv).numpy()
        disk[valid] = Metrics.batch_detect_off_road_disk(cen.clone(), ext, drv).numpy()
        code = rs["steps"][t]["code"]
        coll = {k: (code == int(k) + 1).astype(np.float64) for k in CollisionType}
        coll["coll_any"] = (code > 0).astype(np.float64)
        si = dict(scene_index=scene, track_id=np.arange(B), centroid=w[:, :2], yaw=w[:, 2], extent=extent.astype(np.float64),
                  _off=off, _disk=disk, _coll=coll)
        cdisk = EM.DiskCollisionRate.compute_per_step(si, np.arange(S))[0]["coll_any"]
        flags[t] = np.stack([np.where(np.isnan(off), 255, off), np.where(np.isnan(disk), 255, disk), cdisk, code], -1).astype(np.uint8)
        for c in classes.values():
            c.add_step(si, np.arange(S))
    ep = {k: c.get_episode_metrics() for k, c in classes.items()}
    per_scene = np.stack([ep["off"]["rate"], ep["off"]["nframe"], ep["disk"]["rate"], ep["disk"]["nframe"],
                          ep["coll"]["CollisionType.FRONT"], ep["coll"]["CollisionType.REAR"], ep["coll"]["CollisionType.SIDE"],
                          ep["coll"]["coll_any"], ep["cdisk"]["coll_any"], ep["fail"]["failure_offroad"],
                          ep["fail"]["failure_collision"], ep["fail"]["failure_any"], ep["comfort"]["speed"], ep["comfort"]["lon_acc"],
                          ep["comfort"]["lat_acc"], ep["comfort"]["jerk"]], 1).astype(np.float64)
    pa = rs["per_agent"].copy()
    fa = classes["fail"].get_per_agent_metrics()
    pa[:, 9], pa[:, 10], pa[:, 11] = fa["offroad"].to_numpy(), fa["collision"].to_numpy(), fa["any"].to_numpy()
    out.update({f"{name}_flags": flags, f"{name}_partner": rs["partner"], f"{name}_per_scene": per_scene, f"{name}_per_agent": pa})
    print(name, "flags differ from the restatement at", int((flags != rs["flags"]).sum()), "places; per_scene max diff",
          np.nanmax(np.abs(per_scene - rs["per_scene"])))


def main():
    _refimport.install()
    for n in ("transforms3d", "transforms3d.euler", "pyemd"):
        m = MagicMock(name=n)
        m.__path__ = []
        sys.modules[n] = m
    import tbsim.envs.env_metrics as EM
    import tbsim.utils.metrics as Metrics
    from tbsim.utils.geometry_utils import CollisionType
    case = MC.build_case()
    B = case["world"].shape[1]
    absent = MC.absent_scene_case()
    out = dict(world=case["world"], extent=case["extent"], scene_start=case["scene_start"], absent_world=absent["world"],
               absent_extent=absent["extent"], absent_scene_start=absent["scene_start"], maps=case["maps"], scene_map=case["scene_map"],
               map_from_world=case["map_from_world"])
    saved = (EM.OffRoadRate.compute_per_step, EM.DiskOffRoadRate.compute_per_step, EM.CollisionRate.compute_per_step)
    try:
        EM.OffRoadRate.compute_per_step = staticmethod(lambda si, asi: si["_off"])
        EM.DiskOffRoadRate.compute_per_step = staticmethod(lambda si, asi: si["_disk"])
        EM.CollisionRate.compute_per_step = staticmethod(lambda si, asi: (si["_coll"], None))
        for name in MC.RASTERS:
            record(case, name, MC.cfg_of(name), out, EM, Metrics, CollisionType)
        record(absent, "absent", MC.cfg_of("r64"), out, EM, Metrics, CollisionType)
    finally:
        EM.OffRoadRate.compute_per_step, EM.DiskOffRoadRate.compute_per_step, EM.CollisionRate.compute_per_step = \
            (staticmethod(f) for f in saved)
    empty = MC.aggregate(case, [], np.zeros((B, 0, 3)))
    meta = {"reference": "off_road, off_road_disk, coll_disk flags; per_scene; per_agent columns 9-11 (of r224, r64 and absent)",
            "restatement": "box code (flags[..., 3]), partner, per_agent columns 0-8 and 12-15, empty_per_scene / empty_per_agent",
            "rasters": {n: MC.cfg_of(n) for n in MC.RASTERS}, "sim_dt": MC.SIM_DT, "stat_dt": MC.STAT_DT}
    out.update(empty_per_agent=empty[0], empty_per_scene=empty[1])
    path = os.path.join(ROOT, "tests", "golden", "rollout_metrics.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
