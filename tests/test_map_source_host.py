"""Host-side checks of the map source (include/cld.h `cld_set_map_source`): that the case the kernel tests run on (tests/map_source_cases.py)
is what they need it to be -- asserted with the fp64 restatement of the raster and the oracle's MapCollisionLoss --, the ctypes layout of
`cld_map_source`, the configuration adapter in map mode and `refresh_collision_terms`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import map_source_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("raster", list(MC.RASTERS))
def test_the_case_reaches_what_the_kernel_tests_lean_on(raster):
    c = MC.case(raster)
    assert tuple(c["sizes"]) == (3, 2, 2) and c["scene_map"].tolist() == [0, 1, -1] and c["maps"].shape == (2, MC.N_SEM, 48, 64)
    assert not np.array_equal(c["maps"][0], c["maps"][1]) and c["plans"].shape == (7, 2, 52, 6)
    H, W = c["cfg"]["height"], c["cfg"]["width"]
    assert ((H * W) % 4 == 0) == (raster == "vec")                          # "odd": raster_kernel's dword-store path
    for m in range(2):                                                      # a rotation and a non-unit scale
        A = c["map_from_world"][m, :2, :2].astype(np.float64)
        assert abs(np.sqrt(abs(np.linalg.det(A))) - 1.0) > 0.25 and abs(A[0, 1]) > 0.25
    assert (np.abs(c["curr_speed"]) <= MC.MOVING_SPEED_TH).sum() == 1
    for grid in MC.GRIDS:
        for fill in MC.FILLS:
            k = MC.conditions(c, grid, fill)
            print(f"{raster} {grid} fill {fill}: mixed share {k['mixed_share']:.3f}, plans sampling outside the map {k['outside_plans']}, "
                  f"pixels within {MC.RC.MAP_MARGIN} px of a rounding boundary {k['boundary_pixels']}, max value {k['values'].max():.3f}")
            assert k["mixed_share"] >= 0.25
            assert k["outside_plans"] >= 1
            assert k["boundary_pixels"] >= 8
            assert k["values"].max() > 0.5
            if fill == -1.0:
                assert float(np.abs(k["values"][c["scene_index"] == 2]).max()) == 0.0      # no map, fill -1: everything is drivable


def test_tiled_cases_cover_the_agents_whole_scene_wise():
    for agents in (64, 256):
        c = MC.tiled("vec", agents)
        assert c["poses"].shape == (agents, 3) and sum(c["sizes"]) == agents and int(c["scene_start"][-1]) == agents
        assert len(c["scene_map"]) == len(c["sizes"]) == len(c["weights"]) and set(c["scene_map"].tolist()) == {0, 1, -1}


def test_map_source_struct_layout_matches_the_header():
    """ctypes.CldMapSource against include/cld.h, field by field: (name, size, is-pointer)."""
    from cld_amd import _lib
    table = [("maps", 8, True), ("scene_map", 8, True), ("map_from_world", 8, True), ("world", 8, True),
             ("num_scenes", 4, False), ("num_maps", 4, False), ("n_sem", 4, False), ("map_h", 4, False), ("map_w", 4, False),
             ("drivable_layer", 4, False), ("px_per_m", 4, False), ("ego_center", 8, False), ("no_map_fill", 4, False)]
    hdr = open(os.path.join(ROOT, "include", "cld.h")).read()
    body = re.search(r"typedef struct cld_map_source \{(.*?)\} cld_map_source;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        is_ptr = "*" in stmt
        names = stmt.replace("*", " ").split(None, 2 if stmt.startswith("const") else 1)[-1]
        declared += [(re.sub(r"\[.*", "", n.strip()), is_ptr) for n in names.split(",")]
    assert declared == [(n, p) for n, _, p in table]
    assert [n for n, _ in _lib.CldMapSource._fields_] == [n for n, _, _ in table]
    off = 0
    for (name, size, is_ptr), (_, ctype) in zip(table, _lib.CldMapSource._fields_):
        assert (ctype is ctypes.c_void_p) == is_ptr and ctypes.sizeof(ctype) == size, name
        align = 8 if is_ptr else 4
        off = (off + align - 1) // align * align
        assert getattr(_lib.CldMapSource, name).offset == off, name
        off += size
    assert ctypes.sizeof(_lib.CldMapSource) == 72 and _lib.CldMapSource.num_scenes.offset == 32 and _lib.CldMapSource.no_map_fill.offset == 68
    # the structs whose layout is frozen are what they were
    assert ctypes.sizeof(_lib.CldGuidance) == 144 and ctypes.sizeof(_lib.CldCollision) == 88 and ctypes.sizeof(_lib.CldMapCollision) == 80
    assert "cld_set_map_source" in _lib.SIGNATURES and re.search(r"\bcld_set_map_source\s*\(", hdr)


def _configs():
    return [[{"name": "agent_collision", "weight": 2.0, "params": {}, "agents": None},
             {"name": "map_collision", "weight": 3.0, "params": {"num_points_lw": (5, 3)}, "agents": None}],
            [{"name": "map_collision", "weight": 0.5, "params": {"num_points_lw": (5, 3)}, "agents": None}]]


def test_guidance_from_config_in_map_mode():
    from cld_amd.policy import guidance_from_config, raster_frames
    scene_index = torch.tensor([0, 0, 0, 1, 1])
    B = 5
    db = {"extent": torch.ones(B, 3), "world_from_agent": torch.eye(3).expand(B, 3, 3), "curr_speed": torch.ones(B)}
    ms = dict(maps=torch.zeros(1, 3, 8, 8), scene_map=torch.tensor([0, -1]), map_from_world=torch.eye(3)[None], world=torch.zeros(B, 3),
              height=24, width=40)
    with pytest.raises(ValueError):                                          # raster mode still needs its raster
        guidance_from_config(_configs(), scene_index, data_batch=db)
    g = guidance_from_config(_configs(), scene_index, data_batch=db, map_source=ms)
    m = g["map_collision"]
    assert "drivable_map" not in m and m["map_source"] == ms and m["map_source"] is not ms
    assert m["weight"] == [3.0, 0.5] and tuple(m["num_points_lw"]) == (5, 3) and m["extent"] is db["extent"] and m["curr_speed"] is db["curr_speed"]
    assert torch.equal(m["raster_from_agent"], raster_frames(ms, B)) and m["raster_from_agent"].shape == (B, 3, 3)
    assert m["raster_from_agent"][0].tolist() == [[2.0, 0.0, 10.0], [0.0, 2.0, 12.0], [0.0, 0.0, 1.0]]
    assert g["agent_collision"]["weight"] == [2.0, 0.0]
    db2 = {"extent": torch.ones(B, 3), "world_from_agent": torch.eye(3).expand(B, 3, 3)}
    g2 = guidance_from_config([[_configs()[0][1]], []], scene_index, data_batch=db2, map_source=ms)      # curr_speed may come with the observation
    assert "curr_speed" not in g2["map_collision"]
    with pytest.raises(ValueError):
        guidance_from_config([[_configs()[0][1]], []], scene_index, data_batch={}, map_source=ms)


def test_refresh_collision_terms_replaces_the_observation_fields_and_nothing_else():
    from cld_amd.policy import guidance_from_config, refresh_collision_terms
    scene_index = torch.tensor([0, 0, 0, 1, 1])
    B = 5
    db = {"extent": torch.ones(B, 3), "world_from_agent": torch.eye(3).expand(B, 3, 3), "curr_speed": torch.ones(B),
          "raster_from_agent": torch.eye(3).expand(B, 3, 3), "drivable_map": torch.ones(B, 4, 4, dtype=torch.uint8)}
    ms = dict(maps=torch.zeros(1, 3, 8, 8), scene_map=torch.tensor([0, -1]), map_from_world=torch.eye(3)[None], world=torch.zeros(B, 3))
    obs = {"world_from_agent": torch.full((B, 3, 3), 2.0), "curr_speed": torch.full((B,), 3.0), "raster_from_agent": torch.full((B, 3, 3), 4.0),
           "drivable_map": torch.zeros(B, 4, 4, dtype=torch.uint8), "world": torch.full((B, 3), 5.0), "extent": torch.full((B, 3), 9.0)}
    col_fixed = ("extent", "scene_index", "weight", "agents", "num_disks", "buffer_dist", "decay_rate", "guide_moving_speed_th")
    map_fixed = ("extent", "scene_index", "weight", "num_points_lw", "decay_rate", "guide_moving_speed_th")
    for mode in ("raster", "map"):
        g = dict(guidance_from_config(_configs(), scene_index, data_batch=db, map_source=ms if mode == "map" else None), lr=0.1)
        before = {k: dict(v) for k, v in g.items() if isinstance(v, dict)}
        out = refresh_collision_terms(g, obs)
        assert out is not g and out["lr"] == 0.1 and set(out) == set(g)
        col, mcol = out["agent_collision"], out["map_collision"]
        assert col["world_from_agent"] is obs["world_from_agent"] and col["curr_speed"] is obs["curr_speed"]
        assert mcol["raster_from_agent"] is obs["raster_from_agent"] and mcol["curr_speed"] is obs["curr_speed"]
        if mode == "raster":
            assert mcol["drivable_map"] is obs["drivable_map"] and "map_source" not in mcol
        else:
            assert "drivable_map" not in mcol and mcol["map_source"]["world"] is obs["world"]
            assert all(mcol["map_source"][k] is ms[k] for k in ("maps", "scene_map", "map_from_world"))
            assert refresh_collision_terms(g, obs, world=db["extent"])["map_collision"]["map_source"]["world"] is db["extent"]      # the argument wins
        for k in col_fixed:
            assert col[k] is g["agent_collision"][k], k
        for k in map_fixed:
            assert mcol[k] is g["map_collision"][k], k
        assert set(col) == set(g["agent_collision"]) and set(mcol) == set(g["map_collision"])
        for k, v in before.items():                                          # nothing was modified in place
            assert set(g[k]) == set(v) and all(g[k][f] is v[f] for f in v), k
        # an observation that lacks a field leaves it alone
        part = refresh_collision_terms(g, {"curr_speed": obs["curr_speed"]})
        assert part["agent_collision"]["world_from_agent"] is g["agent_collision"]["world_from_agent"]
        assert part["map_collision"]["raster_from_agent"] is g["map_collision"]["raster_from_agent"]
        assert part["agent_collision"]["curr_speed"] is obs["curr_speed"] and part["map_collision"]["curr_speed"] is obs["curr_speed"]
        if mode == "raster":
            assert part["map_collision"]["drivable_map"] is g["map_collision"]["drivable_map"]
        else:
            assert part["map_collision"]["map_source"]["world"] is ms["world"]
    plain = {"target_speed": torch.zeros(B, 52), "loss_scale": torch.ones(B)}
    assert refresh_collision_terms(plain, obs) is plain and refresh_collision_terms(None, obs) is None


def test_set_guidance_options_default_to_frozen_frames():
    """set_guidance without the new options is what it was: the collision terms keep the data_batch they were configured with, and the
    options do not leak into the guidance dict."""
    from cld_amd.policy import CldPolicy
    pol = CldPolicy(dm=None, vae=None)
    scene_index = torch.tensor([0, 0, 0, 1, 1])
    B = 5
    db = {"extent": torch.ones(B, 3), "world_from_agent": torch.eye(3).expand(B, 3, 3), "curr_speed": torch.ones(B),
          "raster_from_agent": torch.eye(3).expand(B, 3, 3), "drivable_map": torch.ones(B, 4, 4, dtype=torch.uint8)}
    pol.set_guidance(_configs(), scene_index, data_batch=db, lr=0.1)
    assert pol._follow_observation is False and "map_source" not in pol._guidance["map_collision"] and pol._guidance["lr"] == 0.1
    assert "follow_observation" not in pol._guidance and "map_source" not in pol._guidance
    ms = dict(maps=torch.zeros(1, 3, 8, 8), scene_map=torch.tensor([0, -1]), map_from_world=torch.eye(3)[None], world=torch.zeros(B, 3))
    pol.set_guidance(_configs(), scene_index, data_batch={"extent": db["extent"], "world_from_agent": db["world_from_agent"], "curr_speed": db["curr_speed"]},
                     follow_observation=True, map_source=ms)
    assert pol._follow_observation is True and "drivable_map" not in pol._guidance["map_collision"]
    assert "follow_observation" not in pol._guidance and "map_source" not in pol._guidance
    pol.clear_guidance()
    assert pol._follow_observation is False


def test_scene_observer_map_source_is_what_the_engine_takes():
    """SceneObserver.map_source(): keys the engine accepts, the poses of this rank's rows, and the scene_map of the scenes those rows lie
    in -- for an observer over all agents and for one whose rows are a subset of the scenes (and cut one)."""
    import types
    from cld_amd.engine import MAP_SOURCE_DEFAULTS, RASTER_DEFAULTS, raster_frames
    from cld_amd import observe
    assert observe.RASTER_DEFAULTS is RASTER_DEFAULTS and {k: v for k, v in MAP_SOURCE_DEFAULTS.items() if k != "drivable_layer"} == RASTER_DEFAULTS
    fake = types.SimpleNamespace(device=torch.device("cpu"))
    sizes = [2, 3, 2]
    B_all, T = sum(sizes), 4
    hist = torch.arange(B_all * T * 3, dtype=torch.float32).reshape(B_all, T, 3)
    maps, scene_map, mfw = torch.rand(2, 3, 8, 12), torch.tensor([1, -1, 0]), torch.eye(3).repeat(2, 1, 1)
    allowed = set(MAP_SOURCE_DEFAULTS) | {"maps", "scene_map", "map_from_world", "world"}
    for row0, B, scenes in ((0, None, [1, -1, 0]), (2, 3, [-1]), (1, 5, [1, -1, 0]), (5, 2, [0]), (3, 3, [-1, 0])):
        ob = observe.SceneObserver(fake, [0, 2, 5, 7], hist, torch.ones(B_all, T), maps, scene_map, mfw, n_step_action=2, row0=row0, B=B,
                                   height=24, width=40)
        ms = ob.map_source()
        n = B_all - row0 if B is None else B
        assert set(ms) <= allowed and {"maps", "scene_map", "map_from_world", "world"} <= set(ms)
        assert ms["scene_map"].tolist() == scenes and ms["scene_map"].dtype == torch.int32
        assert ms["world"].shape == (n, 3) and torch.equal(ms["world"], hist[row0:row0 + n, -1])
        assert ms["maps"].shape == (2, 3, 8, 12) and ms["map_from_world"].shape == (2, 3, 3)
        assert (ms["height"], ms["width"], ms["n_sem"], ms["drivable_layer"]) == (24, 40, 3, 0)
        ms["world"][:] = -1.0                                                # a copy: the observer's poses are its own
        assert torch.equal(ob.poses, hist[:, -1])
        assert torch.equal(ob.raster_from_agent, raster_frames(ms, 1)[0]) and ob.raster_from_agent.tolist() == [[2.0, 0.0, 10.0], [0.0, 2.0, 12.0], [0.0, 0.0, 1.0]]
    ob = observe.SceneObserver(fake, [0, 2, 5, 7], hist, torch.ones(B_all, T), n_step_action=2)
    assert ob.map_source()["scene_map"] is None and ob.map_source()["maps"] is None
