"""fp64 restatement of the observation raster (include/cld.h `cld_rasterize`) and seeded case builders for its tests.

The restatement follows the header's definition literally in numpy float64.  The kernel computes in fp32, so a case is only
usable when no decision of the definition is within fp32's reach of flipping.  The builders therefore construct every case so
that two margins hold, and `restate` reports them for the tests to assert:
  * no history pixel coordinate (of a frame that is painted, in the raster of any row of its scene) lies within PIX_MARGIN px of
    a half-integer (where rounding flips) or of a clamp edge 0 / W - 1 / H - 1;
  * no current distance between two agents of a scene lies within DIST_MARGIN m of the neighbour threshold.
Sampling a whole scene until this holds would never end (a 65-agent scene has 260,000 coordinates, each with a 2 % chance of
violating), so the builder rejects and resamples piecewise: the current poses one agent after the other against the agents already
placed, then every earlier history point against all rasters of its scene, each until it passes.
For the semantic planes the maps are constant on 8 x 8-pixel blocks and a pixel whose fp64 map coordinate lies within MAP_MARGIN px
of a rounding boundary is reported in `left_out` and kept out of comparisons.
"""
import numpy as np

PIX_MARGIN = 0.01
DIST_MARGIN = 1e-3
MAP_MARGIN = 1e-3
T_HIST = 31
DEFAULTS = dict(height=224, width=224, px_per_m=2.0, ego_center=(-0.5, 0.0), no_map_fill=-1.0, max_neighbor_dist=30.0, n_sem=3)


def offsets(cfg):
    return (1.0 + cfg["ego_center"][0]) / 2.0 * cfg["width"], (1.0 + cfg["ego_center"][1]) / 2.0 * cfg["height"]


def raster_coords(pts, pose, cfg):
    """World points pts [...,2] in the raster of the agent at pose (x, y, h): R(-h) (p - p_i), then raster_from_agent.  float64."""
    ox, oy = offsets(cfg)
    c, s = np.cos(pose[2]), np.sin(pose[2])
    dx, dy = pts[..., 0] - pose[0], pts[..., 1] - pose[1]
    return np.stack([(c * dx + s * dy) * cfg["px_per_m"] + ox, (c * dy - s * dx) * cfg["px_per_m"] + oy], axis=-1)


def coord_margin(rc, cfg):
    """Distance [...] of raw raster coordinates rc [...,2] from the nearest place where fp32 could decide differently: a half-integer
    inside the raster, or a clamp edge."""
    out = np.full(rc.shape[:-1], np.inf)
    for a, lim in ((0, cfg["width"] - 1), (1, cfg["height"] - 1)):
        x = rc[..., a]
        xc = np.clip(x, 0.0, lim)
        m = np.minimum(np.abs(xc - np.floor(xc) - 0.5), np.minimum(np.abs(x), np.abs(x - lim)))
        out = np.minimum(out, m)
    return out


def scene_of_rows(scene_start, B_all):
    return np.searchsorted(np.asarray(scene_start), np.arange(B_all), side="right") - 1


def restate(case, row0=0, B=None, **override):
    """-> dict(image [B,T+n_sem,H,W] float32, drivable [B,H,W] uint8, raster_from_world [B,3,3] float64, left_out [B,n_sem,H,W] bool,
    pix_margin, dist_margin, plane_margin [B,T]) for rows [row0, row0 + B) of `case` (hist_world [B_all,T,3], hist_avail [B_all,T], scene_start, cfg and
    optionally maps, scene_map, map_from_world), every step in float64."""
    cfg = dict(case["cfg"], **override)
    hw, av, ss = case["hist_world"].astype(np.float64), case["hist_avail"] != 0, np.asarray(case["scene_start"])
    B_all, T = av.shape
    B = B_all - row0 if B is None else B
    H, W, n_sem, ppm, D = cfg["height"], cfg["width"], cfg["n_sem"], cfg["px_per_m"], cfg["max_neighbor_dist"]
    ox, oy = offsets(cfg)
    scene = scene_of_rows(ss, B_all)
    image = np.zeros((B, T + n_sem, H * W), np.float32)
    rfw = np.zeros((B, 3, 3))
    left_out = np.zeros((B, n_sem, H, W), bool)
    pix_margin, dist_margin = np.inf, np.inf
    plane_margin = np.full((B, T), np.inf)                        # per history plane: the smallest margin of a coordinate painted into it
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    maps = case.get("maps")
    for i in range(B):
        r = row0 + i
        pose = hw[r, T - 1]
        members = np.arange(ss[scene[r]], ss[scene[r] + 1])
        others = members[members != r]
        dist = np.hypot(*(hw[others, T - 1, :2] - pose[:2]).T) if len(others) else np.zeros(0)
        if D > 0 and len(others):
            dist_margin = min(dist_margin, np.abs(dist[av[others, T - 1]] - D).min(initial=np.inf))
        nbr = others[av[others, T - 1] & ((dist <= D) if D > 0 else np.ones(len(others), bool))]
        for group, value in ((nbr, -1.0), (np.array([r]), 1.0)):               # neighbours first, the ego on top
            if len(group) == 0:
                continue
            rc = raster_coords(hw[group][:, :, :2], pose, cfg)                   # [n,T,2]
            ok = av[group]
            if ok.any():
                cm = np.where(ok, coord_margin(rc, cfg), np.inf)
                pix_margin = min(pix_margin, cm.min())
                plane_margin[i] = np.minimum(plane_margin[i], cm.min(axis=0))
            rc = np.where(ok[..., None], rc, 0.0)                               # an unavailable frame: raster position (0, 0)
            x = np.rint(np.clip(rc[..., 0], 0, W - 1)).astype(np.int64)
            y = np.rint(np.clip(rc[..., 1], 0, H - 1)).astype(np.int64)
            flat = y * W + x
            for t in range(T):
                image[i, t, flat[:, t]] = value
        image[i, :T, 0] = 0.0
        image[i, :T, H * W - 1] = 0.0
        c, s = np.cos(pose[2]), np.sin(pose[2])
        rfw[i] = [[ppm * c, ppm * s, -ppm * (c * pose[0] + s * pose[1]) + ox], [-ppm * s, ppm * c, ppm * (s * pose[0] - c * pose[1]) + oy],
                  [0, 0, 1]]
        m = -1 if maps is None else int(case["scene_map"][scene[r]])
        if m < 0:
            image[i, T:] = cfg["no_map_fill"]
            continue
        ax, ay = (uu - ox) / ppm, (vv - oy) / ppm
        wx, wy = pose[0] + c * ax - s * ay, pose[1] + s * ax + c * ay
        M = case["map_from_world"][m].astype(np.float64)
        fx, fy = M[0, 0] * wx + M[0, 1] * wy + M[0, 2], M[1, 0] * wx + M[1, 1] * wy + M[1, 2]
        left_out[i] = (np.abs(fx - np.floor(fx) - 0.5) < MAP_MARGIN) | (np.abs(fy - np.floor(fy) - 0.5) < MAP_MARGIN)
        mx, my = np.rint(fx).astype(np.int64), np.rint(fy).astype(np.int64)
        mh, mw = maps.shape[2:]
        inside = (mx >= 0) & (mx < mw) & (my >= 0) & (my < mh)
        for layer in range(n_sem):
            vals = maps[m, layer][np.clip(my, 0, mh - 1), np.clip(mx, 0, mw - 1)]
            image[i, T + layer] = np.where(inside, vals, cfg["no_map_fill"]).reshape(-1)
    image = image.reshape(B, T + n_sem, H, W)
    drivable = (image[:, T] != 0).astype(np.uint8) if n_sem else None
    return dict(image=image, drivable=drivable, raster_from_world=rfw, left_out=left_out, pix_margin=float(pix_margin),
                dist_margin=float(dist_margin), plane_margin=plane_margin)


def _violations(points, poses, cfg):
    """points [n,K,2] world, poses [n,3] of one scene -> [n,K] bool: the point is within the margin in the raster of some row."""
    bad = np.zeros(points.shape[:2], bool)
    for pose in poses:
        bad |= coord_margin(raster_coords(points, pose, cfg), cfg) < 2.0 * PIX_MARGIN        # (built with twice the asserted margin)
    return bad


def build_case(seed, scene_sizes, cfg=None, mask_prob=0.15, ego_at_origin=False, all_present=False, edge_cases=False,
               spread=None, with_maps=None):
    """A seeded scene set: hist_world [B_all,31,3] float32, hist_avail [B_all,31] uint8, scene_start, cfg -- both margins hold with
    a factor 2 to spare (the values are rounded to float32 before they are checked).
    ego_at_origin: the first agent of every scene stands at (0, 0) heading 0 now, so its agent frame is the world frame.
    all_present:   every agent is available now (then every agent of a scene is a neighbour when max_neighbor_dist <= 0); otherwise the
                   last agent of every scene of >= 3 is absent now.
    edge_cases:    in every scene of >= 2 agents the first agent's frame 3 lies far behind / left of it (raster pixel (0, 0) = flat
                   pixel 0) and its frame 5 far ahead / right (flat pixel H W - 1), and the second agent's frame 7 is the first's.
    with_maps:     None, or a list of (map_h, map_w) -- maps constant on 8 x 8 blocks, scene s uses map s % (len + 1), the last of these meaning none (so
                   some scenes have no map), map_from_world a rotation, a scale of about 2 px / m and a shift that puts the scene on the map."""
    cfg = dict(DEFAULTS, **(cfg or {}))
    rng = np.random.default_rng(seed)
    T = T_HIST
    half = 0.5 * min(cfg["height"], cfg["width"]) / cfg["px_per_m"]
    spread = 1.2 * half if spread is None else spread
    D = cfg["max_neighbor_dist"]
    hist, avail, start = [], [], [0]
    centres = []
    for n in scene_sizes:
        centre = np.zeros(2) if ego_at_origin else rng.uniform(-30.0, 30.0, 2)
        centres.append(centre)
        poses = np.zeros((n, 3), np.float32)
        for k in range(n):                                           # the current poses, one agent after the other
            while True:                                              # (candidates are drawn and checked 256 at a time)
                cand = np.concatenate([centre + rng.uniform(-spread, spread, (256, 2)), rng.uniform(-np.pi, np.pi, (256, 1))], 1).astype(np.float32)
                if ego_at_origin and k == 0:
                    cand[:] = 0.0
                    break
                if k == 0:
                    break
                p64, c64 = poses[:k].astype(np.float64), cand.astype(np.float64)
                bad = _violations(c64[None, :, :2], p64, cfg)[0]                                   # the candidate in the placed agents' rasters
                rc = np.stack([raster_coords(p64[:, :2], c, cfg) for c in c64[~bad]]) if (~bad).any() else np.zeros((0, k, 2))
                bad[~bad] = (coord_margin(rc, cfg) < 2.0 * PIX_MARGIN).any(axis=1)                 # the placed agents in the candidate's raster
                if D > 0:
                    bad |= (np.abs(np.hypot(c64[:, None, 0] - p64[None, :, 0], c64[:, None, 1] - p64[None, :, 1]) - D) < 2.0 * DIST_MARGIN).any(axis=1)
                if not bad.all():
                    cand = cand[~bad]
                    break
            poses[k] = cand[0]
        # earlier frames: drive backwards from the pose at a constant speed and yaw rate, then jitter each point until it passes
        speed, yawrate = rng.uniform(0.0, 10.0, n), rng.uniform(-0.3, 0.3, n)
        back = 0.1 * np.arange(T - 1, -1, -1.0)                        # seconds before now, [T]
        yaw = poses[:, 2:3].astype(np.float64) - yawrate[:, None] * back
        base = poses[:, None, :2].astype(np.float64) - speed[:, None, None] * back[None, :, None] * np.stack([np.cos(yaw), np.sin(yaw)], -1)
        pts = base.astype(np.float32)
        if edge_cases and n >= 2:
            c, s = np.cos(np.float64(poses[0, 2])), np.sin(np.float64(poses[0, 2]))
            for t, (ax, ay) in ((3, (-300.0, -300.0)), (5, (300.0, 300.0))):
                pts[0, t] = (poses[0, :2].astype(np.float64) + np.array([c * ax - s * ay, s * ax + c * ay])).astype(np.float32)
        pts[:, T - 1] = poses[:, :2]
        fixed = np.zeros((n, T), bool)
        fixed[:, T - 1] = True
        for _ in range(2000):
            bad = _violations(pts.astype(np.float64), poses.astype(np.float64), cfg) & ~fixed
            if not bad.any():
                break
            pts[bad] = (pts[bad].astype(np.float64) + rng.uniform(-0.2, 0.2, (int(bad.sum()), 2))).astype(np.float32)
        else:
            raise RuntimeError("build_case: the history points did not settle")
        if edge_cases and n >= 2:
            pts[1, 7] = pts[0, 7]
        av = (rng.uniform(size=(n, T)) >= mask_prob).astype(np.uint8)
        if all_present:
            av[:, T - 1] = 1
        elif n >= 3:
            av[n - 1, T - 1] = 0                                     # the last agent of a scene is absent now: nobody's neighbour
        if edge_cases and n >= 2:
            av[0, [3, 5, 7]] = 1
            av[1, [7, T - 1]] = 1
        hist.append(np.concatenate([pts, yaw.astype(np.float32)[..., None]], -1))
        avail.append(av)
        start.append(start[-1] + n)
    case = dict(hist_world=np.concatenate(hist).astype(np.float32), hist_avail=np.concatenate(avail), scene_start=np.array(start, np.int32),
                cfg=cfg)
    if with_maps:
        n_sem, K = cfg["n_sem"], len(with_maps)
        mh, mw = max(h for h, _ in with_maps), max(w for _, w in with_maps)
        assert all((h, w) == (mh, mw) for h, w in with_maps), "one call takes maps of one size"
        blocks = rng.integers(0, 3, (K, n_sem, (mh + 7) // 8, (mw + 7) // 8)).astype(np.float32) * 0.5
        case["maps"] = np.kron(blocks, np.ones((8, 8), np.float32))[:, :, :mh, :mw].copy()
        case["scene_map"] = np.array([s % (K + 1) if s % (K + 1) < K else -1 for s in range(len(scene_sizes))], np.int32)
        mfw = np.zeros((K, 3, 3), np.float32)
        for m in range(K):
            users = [s for s in range(len(scene_sizes)) if case["scene_map"][s] == m]
            centre = centres[users[0]] if users else np.zeros(2)
            th, sc = rng.uniform(-np.pi, np.pi), rng.uniform(1.8, 2.2)
            A = sc * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
            mfw[m, :2, :2] = A
            mfw[m, :2, 2] = np.array([mw / 2.0, mh / 2.0]) - A @ centre + rng.uniform(-3.0, 3.0, 2)
            mfw[m, 2, 2] = 1.0
        case["map_from_world"] = mfw
    return case


def world_step(traj, centroid, yaw, k):
    """cld_world_step restated (float64): plan state k [B,52,6] at the pose (centroid [B,2], yaw [B]) -> world [B,3]."""
    traj, centroid, yaw = np.asarray(traj, np.float64), np.asarray(centroid, np.float64), np.asarray(yaw, np.float64)
    c, s = np.cos(yaw), np.sin(yaw)
    return np.stack([traj[:, k, 0] * c - traj[:, k, 1] * s + centroid[:, 0], traj[:, k, 0] * s + traj[:, k, 1] * c + centroid[:, 1],
                     yaw + traj[:, k, 3]], -1)


def advance(hist_world, hist_avail, plans, n_step_action=5):
    """The observer's ring shift restated (float64): -> (hist_world, hist_avail) after the first n_step_action states of `plans`."""
    hw = np.asarray(hist_world, np.float64)
    new = np.stack([world_step(plans, hw[:, -1, :2], hw[:, -1, 2], k) for k in range(n_step_action)], 1)
    av = np.concatenate([np.asarray(hist_avail)[:, n_step_action:], np.ones((hw.shape[0], n_step_action), np.uint8)], 1)
    return np.concatenate([hw[:, n_step_action:], new], 1), av


GOLDEN_CFG = dict(height=24, width=40)


def golden_case():
    """The inputs of tests/golden/rasterize_agents.npz (tests/tools/record_raster_golden.py): 4 scenes x 6 agents x 31 frames on a
    24 x 40 raster, the first agent of each scene at the origin, so that the histories handed to the reference's rasterize_agents
    (agent frame) are the world-frame ones; every agent present now, as the reference paints every agent it is given."""
    return build_case(2024, [6, 6, 6, 6], cfg=GOLDEN_CFG, mask_prob=0.2, ego_at_origin=True, all_present=True, edge_cases=True, spread=14.0)


_CASES = {}


def case(name):
    """The cases of the kernel tests (built once per process); the host tests assert their margins before any kernel runs on them."""
    if name not in _CASES:
        _CASES[name] = {
            # eight agents at the ContextEncoder's size; scene 0 on a map, scene 1 without one; paint edge cases; agents beyond 30 m
            "eight": lambda: build_case(11, [5, 3], edge_cases=True, with_maps=[(320, 256)]),
            # scenes of 1, 2 and 65 agents in one call (more neighbours than a wave has lanes), non-square raster, no maps at all
            "sizes": lambda: build_case(12, [1, 2, 65], cfg=dict(height=64, width=96), edge_cases=True),
            # a map smaller than the crop
            "small_map": lambda: build_case(13, [4], with_maps=[(96, 64)]),
            # a plane that is no multiple of four pixels: the dword-store path
            "odd": lambda: build_case(14, [3, 2], cfg=dict(height=22, width=37), with_maps=[(64, 72)], spread=8.0),
        }[name]()
    return _CASES[name]


CASE_NAMES = ("eight", "sizes", "small_map", "odd")
