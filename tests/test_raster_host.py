"""Host-side checks of the observation raster: the fp64 restatement (tests/raster_cases.py) against the recording made from the
reference's own rasterize_agents (tests/golden/rasterize_agents.npz, tests/tools/record_raster_golden.py), the margins every kernel
case relies on, `SceneObserver`'s history ring and pose bookkeeping, and the ctypes layout of `cld_raster`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import raster_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = RC.T_HIST


def golden_as_case(golden):
    meta, g = golden("rasterize_agents")
    cfg = dict(RC.DEFAULTS, **{k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["cfg"].items()})
    return dict(hist_world=g["hist_world"], hist_avail=g["hist_avail"], scene_start=g["scene_start"], cfg=cfg), g["planes"]


def test_restatement_equals_the_reference_recording(golden):
    """Exact: every history plane of every scene's first agent, painted from all five other agents (max_neighbor_dist = 0: the
    reference paints every agent it is given)."""
    case, planes = golden_as_case(golden)
    ss = case["scene_start"]
    assert planes.shape == (4, T, 24, 40) and planes.dtype == np.int8 and case["hist_world"].shape == (24, T, 3)
    for s in range(4):
        r = RC.restate(case, row0=int(ss[s]), B=1, max_neighbor_dist=0.0)
        assert r["pix_margin"] >= RC.PIX_MARGIN
        assert np.array_equal(r["image"][0, :T], planes[s].astype(np.float32)), s
    fresh = RC.golden_case()                                                 # the builder still makes the recorded inputs
    assert all(np.array_equal(fresh[k], case[k]) for k in ("hist_world", "hist_avail", "scene_start"))


def test_the_recording_holds_the_cases_it_is_meant_to(golden):
    case, planes = golden_as_case(golden)
    cfg, ss, av = case["cfg"], case["scene_start"], case["hist_avail"] != 0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "rasterize_agents.npz")) < 200 * 1024
    assert av[:, T - 1].all() and (~av[ss[:-1]]).any() and (~av[np.setdiff1d(np.arange(24), ss[:-1])]).any()     # masked ego and neighbour frames
    outside = on_ego = 0
    for s in range(4):
        ego = int(ss[s])
        assert np.array_equal(case["hist_world"][ego, T - 1], np.zeros(3, np.float32))
        for j in range(ego + 1, int(ss[s + 1])):
            rc = RC.raster_coords(case["hist_world"][j, :, :2].astype(np.float64), np.zeros(3), cfg)
            out = ((rc[:, 0] < 0) | (rc[:, 0] > cfg["width"] - 1) | (rc[:, 1] < 0) | (rc[:, 1] > cfg["height"] - 1)) & av[j]
            outside += int(out.sum())
            on_ego += int((av[j] & av[ego] & (np.abs(case["hist_world"][j, :, :2] - case["hist_world"][ego, :, :2]).max(-1) == 0)).sum())
        assert (planes[s][:, 0, 0] == 0).all() and (planes[s][:, -1, -1] == 0).all()
    assert outside >= 10 and on_ego >= 4
    assert (planes == 1).sum() > 50 and (planes == -1).sum() > 200
    border = np.zeros((24, 40), bool); border[[0, -1]] = True; border[:, [0, -1]] = True
    assert (planes[:, :, border] == -1).sum() > 0                              # an out-of-raster neighbour paints a border pixel


@pytest.mark.parametrize("name", RC.CASE_NAMES)
def test_case_margins_hold(name):
    """What lets an fp32 kernel be compared exactly with the fp64 restatement: both margins, under both neighbour rules the kernel
    tests use, and at most 1 % of the semantic pixels left out (about 0.4 % expected: two axes x 2e-3 px per pixel)."""
    case = RC.case(name)
    for D in (30.0, 0.0):
        r = RC.restate(case, max_neighbor_dist=D)
        print(f"{name} D={D}: pixel margin {r['pix_margin']:.4f} px, distance margin {r['dist_margin']:.4f} m, left out {r['left_out'].mean():.4%}")
        assert r["pix_margin"] >= RC.PIX_MARGIN and r["dist_margin"] >= RC.DIST_MARGIN
        assert r["left_out"].mean() <= 0.01
        if "maps" in case:
            assert 0 < r["left_out"].mean()
            assert np.abs(case["hist_world"][:, T - 1, :2]).max() <= 200.0


def test_cases_hold_what_the_kernel_tests_need():
    eight, sizes, small, odd = (RC.case(n) for n in RC.CASE_NAMES)
    assert np.diff(sizes["scene_start"]).tolist() == [1, 2, 65] and eight["hist_world"].shape[0] == 8
    for case in (eight, sizes):
        av, ss = case["hist_avail"] != 0, case["scene_start"]
        assert (~av[ss[:-1]]).any() and (~av[:, T - 1]).any() and (~av[:, :T - 1]).any()      # unavailable: ego frames, neighbours now, neighbours earlier
    r30, r0 = RC.restate(eight), RC.restate(eight, max_neighbor_dist=0.0)
    assert (r30["image"][:, :T] != r0["image"][:, :T]).any()                               # the neighbour rule decides something
    # paint edge cases: the first agent's frames 3 / 5 would paint flat pixels 0 / H W - 1 (they stay 0); agent 1 stands on agent 0's pixel at frame 7
    cfg = eight["cfg"]
    pose = eight["hist_world"][0, T - 1].astype(np.float64)
    rc = RC.raster_coords(eight["hist_world"][0, :, :2].astype(np.float64), pose, cfg)
    assert (rc[3] < 0).all() and rc[5, 0] > cfg["width"] - 1 and rc[5, 1] > cfg["height"] - 1
    assert (r0["image"][0, 3] != 1).all() and (r0["image"][0, 5] != 1).all()
    assert np.array_equal(eight["hist_world"][1, 7, :2], eight["hist_world"][0, 7, :2])
    y, x = np.argwhere(r0["image"][0, 7] == 1)[0]
    assert (r0["image"][1, 7] == -1).sum() >= 1 and r0["image"][0, 7, y, x] == 1               # the ego's +1 lies on top of the neighbour's -1
    # maps: scene 0 of `eight` has one, scene 1 has none; the small map leaves most of the crop to the fill value but not all
    assert eight["scene_map"].tolist() == [0, -1]
    assert (r30["image"][5:, T:] == -1).all() and (r30["image"][:5, T:] != -1).mean() > 0.3
    rs = RC.restate(small)
    share = (rs["image"][:, T:] == -1).mean()
    assert 0.5 < share < 0.99
    assert (rs["drivable"] == 1).any() and (rs["drivable"] == 0).any()
    assert (odd["cfg"]["height"] * odd["cfg"]["width"]) % 4 != 0


class _HostEngine:
    """What SceneObserver needs of an Engine for its bookkeeping, on the CPU: world_step with the kernel's arithmetic in fp32."""
    device = torch.device("cpu")

    def world_step(self, traj, centroid, yaw, k):
        c, s = torch.cos(yaw), torch.sin(yaw)
        world = torch.stack([traj[:, k, 0] * c - traj[:, k, 1] * s + centroid[:, 0], traj[:, k, 0] * s + traj[:, k, 1] * c + centroid[:, 1],
                             yaw + traj[:, k, 3]], -1)
        cs = torch.zeros(traj.shape[0], 4)
        cs[:, 2] = traj[:, k, 2]
        return world, cs


def test_scene_observer_ring_and_poses_follow_the_restatement():
    from cld_amd.observe import SceneObserver
    case = RC.case("eight")
    rng = np.random.default_rng(5)
    obs = SceneObserver(_HostEngine(), case["scene_start"], case["hist_world"], case["hist_avail"], n_step_action=5, row0=2, B=4)
    hw, av = case["hist_world"].astype(np.float64), case["hist_avail"]
    for step in range(3):
        plans = rng.normal(size=(8, 52, 6)).astype(np.float32) * np.array([3.0, 1.0, 5.0, 0.3, 1.0, 0.2], np.float32)
        obs.advance(torch.from_numpy(plans))
        hw, av = RC.advance(hw, av, plans, 5)
        assert np.array_equal(obs.hist_avail.numpy(), av)
        assert np.abs(obs.hist_world.numpy() - hw).max() <= 1e-4                             # fp32 against fp64 at |coordinates| < 200
        assert torch.equal(obs.poses, obs.hist_world[:, -1])
    assert obs.hist_avail[:, T - 15:].all() and np.array_equal(obs.hist_avail[:, :T - 15].numpy(), case["hist_avail"][:, 15:])
    # the agent-frame quantities of this rank's rows
    f = obs.frames()
    pose = hw[2:6, -1]
    assert f["history_positions"].shape == (4, T, 2) and f["history_yaws"].shape == (4, T, 1) and f["agent_hist"].shape == (4, T, 3)
    assert torch.allclose(f["history_positions"][:, -1], torch.zeros(4, 2), atol=1e-4) and torch.allclose(f["history_yaws"][:, -1], torch.zeros(4, 1), atol=1e-5)
    for i in range(4):
        c, s = np.cos(pose[i, 2]), np.sin(pose[i, 2])
        d = hw[2 + i, :, :2] - pose[i, :2]
        ref = np.stack([c * d[:, 0] + s * d[:, 1], c * d[:, 1] - s * d[:, 0]], -1) * (av[2 + i, :, None] != 0)
        assert np.abs(f["history_positions"][i].numpy() - ref).max() <= 1e-3
    assert torch.allclose(f["world_from_agent"] @ f["agent_from_world"], torch.eye(3).expand(4, 3, 3), atol=1e-4)
    assert f["raster_from_agent"][0].tolist() == [[2.0, 0.0, 56.0], [0.0, 2.0, 112.0], [0.0, 0.0, 1.0]]
    assert f["history_availabilities"].dtype == torch.bool
    # from step 1 on the observer must be fed every agent's plan
    from cld_amd._lib import CldError
    with pytest.raises(CldError, match="gather"):
        obs(1, None, torch.zeros(4, 4), None)
    with pytest.raises(CldError):
        obs.advance(torch.zeros(4, 52, 6))
    with pytest.raises(TypeError):
        SceneObserver(_HostEngine(), case["scene_start"], case["hist_world"], case["hist_avail"], pixels_per_metre=2.0)
    with pytest.raises(CldError):
        SceneObserver(_HostEngine(), [0, 5, 9], case["hist_world"], case["hist_avail"])


def test_cld_raster_layout_matches_the_header():
    """ctypes mirror of `cld_raster` against include/cld.h, field by field in declaration order, and the new symbol in both tables."""
    from cld_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cld.h")).read()
    body = re.search(r"typedef struct cld_raster \{(.*?)\} cld_raster;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const\s+)?([a-z0-9_]+)\s*(\*?)\s*(.*)", decl)
        ctype, is_ptr = m.group(2), bool(m.group(3))
        for name in (n.strip() for n in m.group(4).split(",")):
            arr = re.match(r"([a-zA-Z_]+)\[(\d+)\]", name)
            fields.append((arr.group(1), ctype, is_ptr, int(arr.group(2))) if arr else (name, ctype, is_ptr, 1))
    assert [f[0] for f in fields] == [n for n, _ in _lib.CldRaster._fields_]
    off = 0
    for (name, ctype, is_ptr, count), (_, mirror) in zip(fields, _lib.CldRaster._fields_):
        size = 8 if is_ptr else 4
        assert is_ptr or ctype in ("int32_t", "float"), name
        assert ctypes.sizeof(mirror) == size * count, name
        if is_ptr:
            assert mirror is ctypes.c_void_p
        else:
            base = mirror._type_ if count > 1 else mirror
            assert base is (ctypes.c_int32 if ctype == "int32_t" else ctypes.c_float), name
        off = (off + size - 1) // size * size
        assert getattr(_lib.CldRaster, name).offset == off, name
        off += size * count
    assert ctypes.sizeof(_lib.CldRaster) == 104 and _lib.CldRaster.num_scenes.offset == 48 and _lib.CldRaster.max_neighbor_dist.offset == 100
    assert "cld_rasterize" in _lib.SIGNATURES and re.search(r"\bcld_rasterize\s*\(", hdr)
    assert len(_lib.SIGNATURES["cld_rasterize"][1]) == 8
    assert "`cld_rasterize`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
