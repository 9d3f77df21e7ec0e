"""Record tests/golden/guide_metrics.npz from the reference's own guidance metric classes (src/tbsim/utils/guidance_metrics.py).

Run where the reference tree is present:  python -m tests.tools.record_guide_metrics_golden
The inputs come from tests/guide_metrics_cases.build_case() and small_case().  The reference's classes are built by
guidance_metrics_from_config / constraint_metrics_from_config and driven as the environment drives them: update_global_t(t), add_step,
and get_episode_metrics at the end.  What they are handed differs from the library's config in the ways GuidanceMetrics' docstring
names, converted here by cld_amd.metrics.guidance_metric_table: excluded_agents as scene-local indices, target_speed sliced to the
entry's rows, buffer_dist with guidance_from_config's default.
Stand-ins, for the duration of the recording:
  * geometry_utils.detect_collision needs shapely, which is not available here: the name guidance_metrics imported is replaced by a
    function that returns the float64 restatement's partner as a scene-local row (so `coll[1]` is the row itself, the first of the
    deliberate differences of include/cld.h);
  * MapCollisionGuidance / MapCollisionGuidanceDisk.compute_per_step read an observation raster: they are replaced by
    Metrics.batch_detect_off_road_boxes / batch_detect_off_road_disk on the drivable rasters raster_cases.restate builds for every agent
    standing at the step's pose (centroid at the raster offsets, yaw 0, extents times px_per_m); an absent agent records 0.
state_info carries agent_from_world built as the restatement builds it, and agent_hist with column 4 = the acceleration and column 7 = 1.
The recorder prints, per kind, the largest difference between the reference's values and the restatement's.
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
from tests import guide_metrics_cases as GC  # noqa: E402
from tests import raster_cases as RC  # noqa: E402
from tests.tools.record_metrics_golden import drivable_rasters  # noqa: E402


def reference_config(case, table):
    """The case's config with the parameters indexed as upstream's metric classes index them."""
    by_cfg = {}
    for ent in table:
        if ent["config"] is not None:
            by_cfg.setdefault((ent["scene"], ent["config"]), []).append(ent)
    out = []
    for si, cfgs in enumerate(case["config"]):
        lst = []
        for ci, cfg in enumerate(cfgs):
            ents = by_cfg[(si, ci)]
            prm = dict(cfg["params"])
            if cfg["name"] == "agent_collision":
                excl = next(e for e in ents if e["kind"] == "agent_collision")["excluded_local"]
                prm["excluded_agents"] = excl if cfg["params"].get("excluded_agents") is not None else None
                prm["buffer_dist"] = next(e for e in ents if e["kind"] == "social_dist")["params"][0]
            if cfg["name"] == "target_speed":
                p = ents[0]["params"]
                prm["target_speed"] = np.array(p[1:]).reshape(len(ents[0]["members"]), int(p[0]))
            lst.append(dict(name=cfg["name"], weight=cfg["weight"], params=prm, agents=cfg["agents"]))
        out.append(lst)
    return out


def record(case, GM, Metrics):
    """One episode of `case` through the reference's classes -> (keys, values [n_keys], per-key note)."""
    from cld_amd.metrics import guidance_metric_table
    ss, world, extent, cfg = case["scene_start"], case["world"].astype(np.float64), case["extent"], case["cfg"]
    T, B = world.shape[:2]
    S = len(ss) - 1
    rs = case["restated"]
    table = guidance_metric_table(case["config"], ss, case.get("constraint"))
    mets = GM.guidance_metrics_from_config(reference_config(case, table))
    if case.get("constraint") is not None:
        mets.update(GM.constraint_metrics_from_config(case["constraint"]))      # (it indexes every scene's entry: the case has one per scene)
    assert list(mets) == [e["key"] for e in table], (list(mets), [e["key"] for e in table])
    scene = RC.scene_of_rows(ss, B)
    ox, oy = RC.offsets(cfg)
    ctx = {}

    def fake_detect_collision(ego_pos, ego_yaw, ego_extent, other_pos, other_yaw, other_extent):
        j = ctx["j"]
        ctx["j"] += 1
        p = ctx["partner"][ctx["rows"][j]]
        return None if p < 0 else (None, int(p - ctx["rows"][0]))

    def map_step(which):
        def compute_per_step(self, state_info, all_scene_index):
            rows = np.flatnonzero(scene == self.scene_idx)
            if self.agents is not None:
                rows = rows[self.agents]
            return state_info[which][rows]
        return compute_per_step
    saved = (GM.detect_collision, GM.MapCollisionGuidance.compute_per_step, GM.MapCollisionGuidanceDisk.compute_per_step)
    GM.detect_collision = fake_detect_collision
    GM.MapCollisionGuidance.compute_per_step = map_step("_box")
    GM.MapCollisionGuidanceDisk.compute_per_step = map_step("_disk")
    try:
        for t in range(T):
            w = world[t]
            valid = ~(np.isnan(w[:, 0]) | np.isnan(w[:, 1]))
            drv = torch.from_numpy(drivable_rasters(case, cfg, w)[valid])
            cen = torch.tensor([[ox, oy]], dtype=torch.float32).repeat(int(valid.sum()), 1)
            ext = torch.from_numpy(extent[valid, :2]) * cfg["px_per_m"]
            box, disk = np.zeros(B), np.zeros(B)
            box[valid] = Metrics.batch_detect_off_road_boxes(cen.clone(), torch.zeros(int(valid.sum()), 1), ext, drv).numpy()
            disk[valid] = Metrics.batch_detect_off_road_disk(cen.clone(), ext, drv).numpy()
            hist = np.zeros((B, 1, 8))
            hist[:, 0, 4], hist[:, 0, 7] = case["acc"][t].astype(np.float64), 1.0
            si = dict(scene_index=scene, centroid=w[:, :2], yaw=w[:, 2], extent=extent.astype(np.float64),
                      curr_speed=case["speed"][t].astype(np.float64), agent_hist=hist, agent_from_world=GC.agent_from_world(w),
                      _box=box, _disk=disk)
            for key, m in mets.items():
                m.update_global_t(t)
                ctx.update(j=0, partner=rs["partner"][t], rows=np.flatnonzero(scene == m.scene_idx))
                m.add_step(si, np.arange(S))
        values, notes = [], {}
        for key, m in mets.items():
            try:
                values.append(float(m.get_episode_metrics()[m.scene_idx]))
            except IndexError:                                       # a target_time beyond the episode
                values.append(float(rs["values"][key]))
                notes[key] = "the reference raises IndexError; the restatement's value"
    finally:
        GM.detect_collision, GM.MapCollisionGuidance.compute_per_step, GM.MapCollisionGuidanceDisk.compute_per_step = saved
    keys = list(mets)
    worst = {}
    for key, v, ent in zip(keys, values, table):
        r = rs["values"][key]
        d = 0.0 if (np.isnan(v) and np.isnan(r)) or v == r else abs(v - r)
        worst[ent["kind"]] = max(worst.get(ent["kind"], 0.0), d)
    for kind, d in worst.items():
        print(f"  {kind:28s} max |reference - restatement| = {d:.3e}")
    return keys, np.array(values), notes


def main():
    _refimport.install()
    for n in ("transforms3d", "transforms3d.euler", "pyemd", "turtle"):
        m = MagicMock(name=n)
        m.__path__ = []
        sys.modules[n] = m
    import tbsim.utils.guidance_metrics as GM
    import tbsim.utils.metrics as Metrics
    out, meta = {}, {"cfg": GC.CFG, "notes": {}}
    for name in ("main", "small"):
        case = GC.case(name)
        print(name)
        keys, values, notes = record(case, GM, Metrics)
        rs = case["restated"]
        pre = "" if name == "main" else "small_"
        out.update({pre + k: case[k] for k in ("world", "speed", "acc", "extent", "scene_start")})
        out[pre + "values"] = values
        out[pre + "per_member"] = np.concatenate([rs["per_member"][k] for k in keys])      # the restatement's (the classes keep no such table)
        out[pre + "partner"] = rs["partner"].astype(np.int32)
        meta[pre + "keys"] = keys
        meta["notes"].update(notes)
    main_case = GC.case("main")
    out.update(maps=main_case["maps"], scene_map=main_case["scene_map"], map_from_world=main_case["map_from_world"])
    path = os.path.join(ROOT, "tests", "golden", "guide_metrics.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
