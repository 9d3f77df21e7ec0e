"""Inputs of the map-source tests (include/cld.h `cld_set_map_source`): the map term of the collision guidance evaluated on the scene's
semantic map instead of a per-agent drivable raster.

`case(raster)` is one seeded scene set: 3 scenes of 3, 2 and 2 agents -- scenes 0 and 1 on different 48 x 64 maps (two layers; the
drivable layer is made of 4 x 4-pixel patches, so road edges run through every box), scene 2 without a map -- under a
`map_from_world` with a rotation and a scale of 1.5 px / m, on one of two rasters: "vec" (24 x 40: a plane of a multiple of four pixels)
and "odd" (37 x 45: raster_kernel's dword-store path).  The first agent of scene 0 is the one the bit-identity test leans on: its heading
undoes the map's rotation and it stands where every fourth raster column ("vec") / row ("odd") maps EXACTLY onto a half-integer map
coordinate in exact arithmetic, so in fp32 those pixels sit within rounding of the boundary where a differently rounded lookup picks the
neighbouring map pixel.  The second agent of scene 1 stands at the map's border heading outwards: its later steps sample pixels outside
the map.  One agent is slower than the moving threshold.  Two plans per agent (num_samp = 2).

`conditions(case, grid, fill)` restates, on the CPU, what the tests need the case to be: tests/raster_cases.restate gives the fp64
drivable bytes at the case's poses and the pixels whose map coordinate lies within MAP_MARGIN of a rounding boundary, and
oracle.map_collision_loss the values on those bytes.  `tiled(raster, agents)` repeats the scene set (with shifted poses) up to a given
number of agents, for the tests inside the sampler.
"""
import numpy as np

from tests import raster_cases as RC

SIZES = (3, 2, 2)
NUM_SAMP = 2
MAP_H, MAP_W, N_SEM = 48, 64, 2
SCALE, THETA = (1.5, 1.5), (0.4, -0.7)                 # map_from_world of map 0, 1: pixels per metre, rotation
RASTERS = {"vec": dict(height=24, width=40), "odd": dict(height=37, width=45)}
GRIDS = ((10, 10), (5, 3))
FILLS = (-1.0, 0.0)
ANCHOR_MAP_XY = (20.0, 24.375)                         # where agent 0 stands on map 0 (map pixels): see the module docstring
MOVING_SPEED_TH = 0.5


def raster_cfg(raster, fill=-1.0):
    return dict(RC.DEFAULTS, **RASTERS[raster], n_sem=N_SEM, no_map_fill=float(fill))


def _map_from_world(m, centre):
    """Rotation THETA[m], scale SCALE[m]; the world point `centre` lands on the middle of the map."""
    A = SCALE[m] * np.array([[np.cos(THETA[m]), -np.sin(THETA[m])], [np.sin(THETA[m]), np.cos(THETA[m])]])
    M = np.eye(3)
    M[:2, :2] = A
    M[:2, 2] = np.array([MAP_W / 2.0, MAP_H / 2.0]) - A @ np.asarray(centre, np.float64)
    return M


def _world_of(M, map_xy):
    return np.linalg.solve(M[:2, :2], np.asarray(map_xy, np.float64) - M[:2, 2])


def _plans(rng, speed, n_agents):
    """[A,NUM_SAMP,52,6] descaled plans in the agent frame: forward at about `speed`, a lateral offset and drift, a little yaw."""
    dt, T = 0.1, 52
    out = np.zeros((n_agents, NUM_SAMP, T, 6))
    for a in range(n_agents):
        for n in range(NUM_SAMP):
            v = np.clip(speed[a] + np.cumsum(rng.normal(0.0, 0.15, T)), 0.0, 8.0)
            yaw = rng.uniform(-0.2, 0.2) + np.cumsum(rng.normal(0.0, 0.01, T))
            x, y = np.cumsum(v * np.cos(yaw) * dt), rng.uniform(-1.0, 1.0) + np.cumsum(v * np.sin(yaw) * dt)
            out[a, n] = np.stack([x, y, v, yaw, np.gradient(v, dt), np.gradient(yaw, dt)], -1)
    return out.astype(np.float32)


def _build(raster, copies=1, seed=41):
    rng = np.random.default_rng(seed)
    cfg = raster_cfg(raster)
    sizes = list(SIZES) * copies
    centres = [np.array([12.0, -7.0]), np.array([-15.0, 9.0])]
    mfw = np.stack([_map_from_world(m, centres[m]) for m in range(2)])
    patches = (rng.uniform(size=(2, N_SEM, MAP_H // 4, MAP_W // 4)) < 0.6).astype(np.float32)
    patches[:, 1] *= 0.5                                           # (the second layer holds other values: it must not be the one read)
    maps = np.kron(patches, np.ones((4, 4), np.float32))
    poses, scene_map = [], []
    for k in range(copies):
        jit = (lambda: rng.uniform(-1.5, 1.5, 2)) if k else (lambda: np.zeros(2))
        # scene 0 on map 0: the anchored agent, one beside it on converging headings, one further back
        p0 = _world_of(mfw[0], np.asarray(ANCHOR_MAP_XY) + (0.0 if k == 0 else 1.0) * rng.uniform(-6.0, 6.0, 2))
        h0 = -THETA[0] if k == 0 else rng.uniform(-np.pi, np.pi)
        R0 = np.array([[np.cos(h0), -np.sin(h0)], [np.sin(h0), np.cos(h0)]])
        poses += [[*p0, h0], [*(p0 + R0 @ np.array([1.0, 2.4]) + jit()), h0 - 0.25], [*(p0 + R0 @ np.array([-5.0, -2.0]) + jit()), h0 + 0.15]]
        # scene 1 on map 1: one agent inside, one at the map's border heading outwards
        inside = _world_of(mfw[1], [MAP_W / 2.0 + rng.uniform(-8, 8), MAP_H / 2.0 + rng.uniform(-6, 6)])
        border = _world_of(mfw[1], [MAP_W - 6.0, MAP_H / 2.0 + rng.uniform(-6, 6)])
        poses += [[*inside, rng.uniform(-np.pi, np.pi)], [*border, THETA[1] * -1.0 + rng.uniform(-0.3, 0.3)]]      # map +x = world heading -theta
        # scene 2: no map
        poses += [[*rng.uniform(-20, 20, 2), rng.uniform(-np.pi, np.pi)] for _ in range(2)]
        scene_map += [0, 1, -1]
    poses = np.asarray(poses, np.float32)
    A = poses.shape[0]
    speed = rng.uniform(1.5, 4.5, A).astype(np.float32)
    speed[2::7] = 0.2                                              # the third agent of every scene 0: below the moving threshold
    extent = np.stack([rng.uniform(3.8, 5.2, A), rng.uniform(1.7, 2.2, A), np.full(A, 1.6)], 1).astype(np.float32)
    ox, oy = RC.offsets(cfg)
    rfa = np.tile(np.array([[cfg["px_per_m"], 0.0, ox], [0.0, cfg["px_per_m"], oy], [0.0, 0.0, 1.0]], np.float32), (A, 1, 1))
    return dict(raster=raster, cfg=cfg, sizes=sizes, scene_start=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                scene_index=np.repeat(np.arange(len(sizes)), sizes), scene_map=np.asarray(scene_map, np.int32), maps=maps,
                map_from_world=mfw.astype(np.float32), poses=poses, extent=extent, curr_speed=speed, raster_from_agent=rfa,
                plans=_plans(rng, speed, A), weights=[1.5 - 0.1 * (s % 5) for s in range(len(sizes))])


_CASES = {}


def case(raster):
    """The 7-agent case on raster "vec" | "odd" (built once per process; never modified)."""
    if raster not in _CASES:
        _CASES[raster] = _build(raster)
    return _CASES[raster]


def tiled(raster, agents):
    """The scene set repeated until it holds at least `agents` agents, cut to exactly `agents` whole-scene-wise with a last scene that
    takes what is left (on no map)."""
    key = (raster, agents)
    if key not in _CASES:
        per = sum(SIZES)
        c = _build(raster, copies=agents // per + 1, seed=43)
        sizes, total = [], 0
        for s in c["sizes"]:
            if total + s > agents:
                break
            sizes.append(s)
            total += s
        scene_map = list(c["scene_map"][:len(sizes)])
        if total < agents:
            sizes.append(agents - total)
            scene_map.append(-1)
        out = dict(c, sizes=sizes, scene_start=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                   scene_index=np.repeat(np.arange(len(sizes)), sizes), scene_map=np.asarray(scene_map, np.int32),
                   weights=c["weights"][:len(sizes)])
        for k in ("poses", "extent", "curr_speed", "raster_from_agent", "plans"):
            out[k] = c[k][:agents]
        _CASES[key] = out
    return _CASES[key]


def raster_case(c, fill):
    """The case as tests/raster_cases.restate reads it: a one-frame history at the case's poses."""
    A = c["poses"].shape[0]
    return dict(hist_world=c["poses"][:, None, :], hist_avail=np.ones((A, 1), np.uint8), scene_start=c["scene_start"],
                cfg=dict(c["cfg"], no_map_fill=float(fill)), maps=c["maps"], scene_map=c["scene_map"], map_from_world=c["map_from_world"])


def sampled_pixels(c, grid):
    """The raster pixel (ix, iy) [A,N,52,P] of every sample point of every plan, as MapCollisionLoss forms them (float32; truncated,
    clamped)."""
    x = c["plans"]
    A = x.shape[0]
    lin = lambda n: np.linspace(-0.5, 0.5, n, dtype=np.float32) if n > 1 else np.array([-0.5], np.float32)
    loc = np.stack(np.meshgrid(lin(grid[0]), lin(grid[1]), indexing="ij"), -1).reshape(-1, 2)
    locs = loc[None] * c["extent"][:, None, :2]
    cy, sy = np.cos(x[..., 3])[..., None], np.sin(x[..., 3])[..., None]
    lx, wy = locs[:, None, None, :, 0], locs[:, None, None, :, 1]
    px, py = lx * cy - wy * sy + x[..., 0:1], lx * sy + wy * cy + x[..., 1:2]
    R = c["raster_from_agent"][:, None, None, None]
    ix = np.trunc(R[..., 0, 0] * px + R[..., 0, 1] * py + R[..., 0, 2]).astype(np.int64)
    iy = np.trunc(R[..., 1, 0] * px + R[..., 1, 1] * py + R[..., 1, 2]).astype(np.int64)
    return np.clip(ix, 0, c["cfg"]["width"] - 1), np.clip(iy, 0, c["cfg"]["height"] - 1)


def conditions(c, grid, fill):
    """-> dict(mixed_share: share of the (plan, step) pairs of moving agents with some but not all points off road; outside_plans: plans
    with a step that samples a pixel outside the map; boundary_pixels: distinct sampled pixels whose map coordinate lies within
    RC.MAP_MARGIN px of a rounding boundary; values [A,N]: oracle.map_collision_loss on the restated bytes; drivable [A,H,W])."""
    import torch
    from oracle import cld_oracle as O
    rc = raster_case(c, fill)
    r = RC.restate(rc)
    marked = RC.restate(rc, no_map_fill=7.0)["image"][:, 1] == 7.0            # plane T_hist + 0 of a one-frame history: fill = outside the map
    ix, iy = sampled_pixels(c, grid)
    A, N = ix.shape[:2]
    a = np.arange(A)[:, None, None, None]
    off = r["drivable"][a, iy, ix] == 0
    cnt, P = off.sum(-1), off.shape[-1]
    moving = np.abs(c["curr_speed"]) > MOVING_SPEED_TH
    mixed = (cnt > 0) & (cnt < P)
    has_map = c["scene_map"][c["scene_index"]] >= 0
    outside = (marked[a, iy, ix] & has_map[:, None, None, None]).any(-1).any(-1)                   # [A,N]
    near = r["left_out"][:, 0][a, iy, ix]
    flat = (a * 10**6 + iy * 10**3 + ix)[near]
    values = O.map_collision_loss(torch.from_numpy(c["plans"]), torch.from_numpy(c["extent"]), torch.from_numpy(c["raster_from_agent"]),
                                  torch.from_numpy(r["drivable"]), torch.from_numpy(c["curr_speed"]), num_points_lw=grid)
    return dict(mixed_share=float(mixed[moving].mean()), outside_plans=int(outside.sum()), boundary_pixels=int(np.unique(flat).size),
                values=values.numpy(), drivable=r["drivable"])


def loop_case(raster="vec"):
    """The closed-loop case: 2 scenes x 4 agents, each scene on a straight road band 3 m wide (scene s on map s, the band along the
    scene's heading), the agents in two rows left and right of the band's axis -- 2 m apart, so their disks touch from the first step,
    and each box hangs over a road edge -- on headings that converge on the axis.  -> dict(centroid [8,2], yaw [8], curr_states [8,4],
    extent, maps, scene_map, map_from_world, scene_start, scene_index, cfg)."""
    key = ("loop", raster)
    if key not in _CASES:
        cfg = raster_cfg(raster)
        centres, phis = [np.array([12.0, -7.0]), np.array([-15.0, 9.0])], [0.3, -1.1]
        mfw = np.stack([_map_from_world(m, centres[m]) for m in range(2)])
        maps = np.zeros((2, N_SEM, MAP_H, MAP_W), np.float32)
        yy, xx = np.meshgrid(np.arange(MAP_H, dtype=np.float64), np.arange(MAP_W, dtype=np.float64), indexing="ij")
        poses = []
        for m in range(2):
            Ai = np.linalg.inv(mfw[m][:2, :2])
            wx = Ai[0, 0] * (xx - mfw[m][0, 2]) + Ai[0, 1] * (yy - mfw[m][1, 2])
            wy = Ai[1, 0] * (xx - mfw[m][0, 2]) + Ai[1, 1] * (yy - mfw[m][1, 2])
            axis, normal = np.array([np.cos(phis[m]), np.sin(phis[m])]), np.array([-np.sin(phis[m]), np.cos(phis[m])])
            lateral = (wx - centres[m][0]) * normal[0] + (wy - centres[m][1]) * normal[1]
            maps[m, 0] = np.abs(lateral) < 1.5
            maps[m, 1] = 0.5
            for along, side, turn in ((0.0, 1.0, -0.15), (0.0, -1.0, 0.15), (-5.5, 1.05, -0.1), (-5.5, -0.95, 0.1)):
                poses.append([*(centres[m] + along * axis + side * normal), phis[m] + turn])
        poses = np.asarray(poses, np.float32)
        cs = np.zeros((8, 4), np.float32)
        cs[:, 2] = 2.0 + 0.25 * np.arange(8)
        extent = np.tile(np.array([[4.4, 2.0, 1.6]], np.float32), (8, 1))
        _CASES[key] = dict(cfg=cfg, centroid=poses[:, :2].copy(), yaw=poses[:, 2].copy(), curr_states=cs, extent=extent, maps=maps,
                           scene_map=np.array([0, 1], np.int32), map_from_world=mfw.astype(np.float32),
                           scene_start=np.array([0, 4, 8], np.int32), scene_index=np.repeat(np.arange(2), 4))
    return _CASES[key]
