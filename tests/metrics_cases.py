"""fp64 restatement of the closed-loop episode metrics (include/cld.h `cld_scene_metrics_step` / `cld_scene_metrics_read`) and the
seeded case of their tests.

The restatement follows the header's definitions literally in numpy float64.  The kernel computes in fp32, so the case is built so
that no discrete decision is within fp32's reach of flipping, and `restate_step` reports the margins for the host test to assert:
  * DIST_MARGIN (m): every disk distance against the radius sum, the deciding separating-axis gap / overlap of every pair, and the
    two longest clipped sides of every overlapping pair (unless both map to the same collision type);
  * PIX_MARGIN (px): every disk-sample coordinate and every map coordinate of a sampled pixel, from the nearest half-integer.
Positions are multiples of 2^-10 m and extents multiples of 2^-6 m, exact in fp32.  The builder places the agents of a scene one
after the other; a step of an agent's path that violates a margin against the agents already placed (or in its own raster) is
re-drawn with a small seeded shift until it passes -- nothing is left out.  (raster_cases.build_case is not used for the poses: its
history margins are not needed here; its map layout, `offsets` and `restate` are.)
"""
import numpy as np

from tests import raster_cases as RC

DIST_MARGIN = 1e-3
PIX_MARGIN = 1e-3
SCENE_SIZES = (1, 2, 5, 63, 64, 65, 130)
N_STEPS = 21
SIM_DT, STAT_DT, RATIO = 0.1, 0.5, 5
RASTERS = {"r224": dict(height=224, width=224), "r64": dict(height=64, width=64)}
BASE_CFG = dict(px_per_m=2.0, ego_center=(-0.5, 0.0), no_map_fill=-1.0, n_sem=3)
GIANT, FAR, CONSTRUCTED_SCENE, N_CONSTRUCTED = 1, 2, 5, 14      # scene 1: a giant agent (clamped disk) and a far one; scene 5 opens with the built pairs
DISK_ANGLES = np.linspace(0.0, 2.0 * np.pi, 13)
DISK_COS, DISK_SIN = np.cos(DISK_ANGLES), np.sin(DISK_ANGLES)
AGENT_COLS, SCENE_COLS = 16, 16


def cfg_of(name):
    return dict(BASE_CFG, **RASTERS[name])


# ------------------------------------------------------------------------------------------------ geometry (float64, broadcasting)
def sat_gaps(pi, ei, pj, ej):
    """The four separating-axis gaps [...,4] (<= 0 on every axis: the boxes overlap) of boxes at poses pi, pj [...,3] with extents
    ei, ej [...,2] (e0 along the heading)."""
    dx, dy = pj[..., 0] - pi[..., 0], pj[..., 1] - pi[..., 1]
    ci, si, cj, sj = np.cos(pi[..., 2]), np.sin(pi[..., 2]), np.cos(pj[..., 2]), np.sin(pj[..., 2])
    a0, a1, b0, b1 = ei[..., 0] / 2, ei[..., 1] / 2, ej[..., 0] / 2, ej[..., 1] / 2
    cc, cs = np.abs(ci * cj + si * sj), np.abs(ci * sj - si * cj)
    return np.stack([np.abs(dx * ci + dy * si) - (a0 + b0 * cc + b1 * cs), np.abs(dy * ci - dx * si) - (a1 + b0 * cs + b1 * cc),
                     np.abs(dx * cj + dy * sj) - (b0 + a0 * cc + a1 * cs), np.abs(dy * cj - dx * sj) - (b1 + a0 * cs + a1 * cc)], -1)


def _clip(x0, y0, x1, y1, L, b0, b1):
    t0, t1 = np.zeros_like(x0), np.ones_like(x0)
    alive = np.ones(x0.shape, bool)
    dx, dy = x1 - x0, y1 - y0
    for pp, qq in ((-dx, x0 + b0), (dx, b0 - x0), (-dy, y0 + b1), (dy, b1 - y0)):
        par = pp == 0
        alive &= ~(par & (qq < 0))
        r = qq / np.where(par, 1.0, pp)
        alive &= ~((pp < 0) & (r > t1))
        t0 = np.where(pp < 0, np.maximum(t0, r), t0)
        alive &= ~((pp > 0) & (r < t0))
        t1 = np.where(pp > 0, np.minimum(t1, r), t1)
    return np.where(alive, (t1 - t0) * L, 0.0)


def side_lengths(pi, ei, pj, ej):
    """[...,4]: the lengths of i's front (+e0/2), rear, left (+e1/2) and right sides inside j's box (each side clipped against the four
    half-planes of j's box in j's frame)."""
    ci, si, cj, sj = np.cos(pi[..., 2]), np.sin(pi[..., 2]), np.cos(pj[..., 2]), np.sin(pj[..., 2])
    a0, a1, b0, b1 = ei[..., 0] / 2, ei[..., 1] / 2, ej[..., 0] / 2, ej[..., 1] / 2
    q = []
    for f0, f1 in ((a0, a1), (a0, -a1), (-a0, a1), (-a0, -a1)):
        wx, wy = (pi[..., 0] - pj[..., 0]) + (f0 * ci - f1 * si), (pi[..., 1] - pj[..., 1]) + (f0 * si + f1 * ci)
        q.append((wx * cj + wy * sj, wy * cj - wx * sj))
    seg = lambda a, b, L: _clip(q[a][0], q[a][1], q[b][0], q[b][1], L, b0, b1)
    return np.stack([seg(0, 1, 2 * a1), seg(2, 3, 2 * a1), seg(0, 2, 2 * a0), seg(1, 3, 2 * a0)], -1)


def pair_tests(pi, ei, pj, ej):
    """-> dict(disk [...] bool, box [...] bool, side [...] int 0..3 (argmax, first wins), margin [...]) for pairs (i, j)."""
    d = np.hypot(pj[..., 0] - pi[..., 0], pj[..., 1] - pi[..., 1])
    rs = ei.min(-1) / 2 + ej.min(-1) / 2
    g = sat_gaps(pi, ei, pj, ej)
    box = (g <= 0).all(-1)
    L = side_lengths(pi, ei, pj, ej)
    side = L.argmax(-1)
    top = np.sort(L, -1)
    second = np.argsort(-L, -1, kind="stable")[..., 1]
    same_type = np.minimum(side, 2) == np.minimum(second, 2)
    m_side = np.where(same_type, np.inf, top[..., 3] - top[..., 2])
    margin = np.minimum(np.abs(d - rs), np.where(box, np.minimum((-g).min(-1), m_side), g.max(-1)))
    return dict(disk=d < rs, box=box, side=side, margin=margin)


def sample_pixels(extent2, cfg):
    """The 53 raster pixels of an agent with extent2 [2]: 52 disk samples (radius major) then the centroid -> (u [53], v [53] int, the
    smallest distance of a coordinate from a half-integer)."""
    ox, oy = RC.offsets(cfg)
    W, H = cfg["width"], cfg["height"]
    r = cfg["px_per_m"] * extent2.min() / 2.0
    rad = (r * np.arange(1, 5) / 4.0)[:, None]
    fu = np.clip((ox + rad * DISK_COS[None]).reshape(-1), 0, W - 1)
    fv = np.clip((oy + rad * DISK_SIN[None]).reshape(-1), 0, H - 1)
    fu, fv = np.append(fu, ox), np.append(fv, oy)
    margin = min(np.abs(fu - np.floor(fu) - 0.5).min(), np.abs(fv - np.floor(fv) - 0.5).min())
    return np.clip(np.rint(fu), 0, W - 1).astype(np.int64), np.clip(np.rint(fv), 0, H - 1).astype(np.int64), margin


def drv_at(case, cfg, scene, pose, u, v):
    """drv(i; u, v) of include/cld.h for pixels u, v [...] of an agent of `scene` at pose (x, y, h) -> (bytes [...], map margin, in_fill [...])."""
    m = -1 if case.get("maps") is None else int(case["scene_map"][scene])
    if m < 0:
        return np.full(u.shape, int(cfg["no_map_fill"] != 0), np.uint8), np.inf, np.ones(u.shape, bool)
    ox, oy = RC.offsets(cfg)
    ppm = cfg["px_per_m"]
    ax, ay = (u - ox) / ppm, (v - oy) / ppm
    c, s = np.cos(pose[2]), np.sin(pose[2])
    wx, wy = pose[0] + c * ax - s * ay, pose[1] + s * ax + c * ay
    M = case["map_from_world"][m].astype(np.float64)
    fx, fy = M[0, 0] * wx + M[0, 1] * wy + M[0, 2], M[1, 0] * wx + M[1, 1] * wy + M[1, 2]
    margin = min(np.abs(fx - np.floor(fx) - 0.5).min(), np.abs(fy - np.floor(fy) - 0.5).min())
    mx, my = np.rint(fx).astype(np.int64), np.rint(fy).astype(np.int64)
    mh, mw = case["maps"].shape[2:]
    inside = (mx >= 0) & (mx < mw) & (my >= 0) & (my < mh)
    vals = case["maps"][m, case.get("drivable_layer", 0)][np.clip(my, 0, mh - 1), np.clip(mx, 0, mw - 1)]
    return (np.where(inside, vals, cfg["no_map_fill"]) != 0).astype(np.uint8), margin, ~inside


# ------------------------------------------------------------------------------------------------ the restatement
def restate_step(case, cfg, world):
    """One step: world [B_all,3] float64 -> dict(off, disk [B] float (NaN: invalid), coll_disk, code, side, partner [B] int, samples
    [B,53] uint8 drivable bytes (255: invalid), dist_margin, pix_margin, fill_used)."""
    ss, ext = case["scene_start"], case["extent"].astype(np.float64)[:, :2]
    B = world.shape[0]
    valid = ~(np.isnan(world[:, 0]) | np.isnan(world[:, 1]))
    off, disk = np.full(B, np.nan), np.full(B, np.nan)
    coll_disk, code, side, partner = np.zeros(B, np.int64), np.zeros(B, np.int64), np.full(B, -1), np.full(B, -1)
    samples = np.full((B, 53), 255, np.uint8)
    dist_margin, pix_margin, fill_used = np.inf, np.inf, False
    for s in range(len(ss) - 1):
        idx = np.arange(ss[s], ss[s + 1])
        for i in idx[valid[idx]]:
            u, v, m1 = sample_pixels(ext[i], cfg)
            d, m2, fill = drv_at(case, cfg, s, world[i], u, v)
            samples[i] = d
            off[i], disk[i] = 1 - d[52], float((d[:52] == 0).any())
            pix_margin, fill_used = min(pix_margin, m1, m2), fill_used or bool(fill.any())
        ok = idx[valid[idx]]
        if len(ok) < 2:
            continue
        P, E = world[ok], ext[ok]
        t = pair_tests(P[:, None], E[:, None], P[None], E[None])
        other = ~np.eye(len(ok), dtype=bool)
        dist_margin = min(dist_margin, t["margin"][other].min())
        coll_disk[ok] = (t["disk"] & other).any(1)
        box = t["box"] & other
        first = box.argmax(1)
        hit = box.any(1)
        partner[ok] = np.where(hit, ok[first], -1)
        side[ok] = np.where(hit, t["side"][np.arange(len(ok)), first], -1)
        code[ok] = np.where(hit, 1 + np.minimum(t["side"][np.arange(len(ok)), first], 2), 0)
    return dict(off=off, disk=disk, coll_disk=coll_disk, code=code, side=side, partner=partner, samples=samples,
                dist_margin=float(dist_margin), pix_margin=float(pix_margin), fill_used=fill_used)


def comfort(traj, stat_dt=STAT_DT, ratio=RATIO):
    """Comfort.get_episode_metrics' per-agent part restated: traj [B,T,3] float64 -> (values [B,4] nanmean of speed, lon, lat, jerk;
    E [B,4] the mean absolute magnitude entering each: speed, |acc|, |acc|, (|acc_k| + |acc_k+1|) / dt)."""
    st = traj[:, ::ratio]
    vel = np.diff(st[..., :2], axis=1) / stat_dt
    speed = np.linalg.norm(vel, axis=-1)
    acc = np.linalg.norm(np.diff(vel, axis=1) / stat_dt, axis=-1)
    yaw = st[:, :acc.shape[1], 2]
    lon, lat = np.abs(acc * np.cos(yaw)), np.abs(acc * np.sin(yaw))
    jerk = np.abs(np.diff(acc, axis=1) / stat_dt)
    jmag = (acc[:, 1:] + acc[:, :-1]) / stat_dt
    amag_lon, amag_lat = np.where(np.isnan(lon), np.nan, acc), np.where(np.isnan(lat), np.nan, acc)

    def nm(x):
        n = (~np.isnan(x)).sum(1)
        return np.where(n > 0, np.nansum(x, 1) / np.maximum(n, 1), np.nan)
    return np.stack([nm(speed), nm(lon), nm(lat), nm(jerk)], 1), np.stack([nm(speed), nm(amag_lon), nm(amag_lat), nm(jmag)], 1)


def _nanmean(x):
    n = (~np.isnan(x)).sum()
    return np.nansum(x) / n if n else np.nan


def aggregate(case, steps, traj):
    """Per-step results (a list of restate_step dicts) and traj [B,T,3] -> (per_agent [B,16], per_scene [S,16], E_agent [B,4],
    E_scene [S,4]) as cld_scene_metrics_read defines them."""
    ss = case["scene_start"]
    B, S = traj.shape[0], len(ss) - 1
    col = lambda k: np.stack([s[k] for s in steps], 1) if steps else np.zeros((B, 0))
    off, disk, code, cdisk = col("off"), col("disk"), col("code"), col("coll_disk")
    pa = np.zeros((B, AGENT_COLS))
    pa[:, 0], pa[:, 1] = len(steps), (~np.isnan(off)).sum(1)
    pa[:, 2], pa[:, 3] = np.nansum(off, 1), np.nansum(disk, 1)
    pa[:, 4] = (code > 0).any(1)
    for k in range(3):
        pa[:, 5 + k] = (code == k + 1).any(1)
    pa[:, 8] = (cdisk > 0).any(1)
    pa[:, 9], pa[:, 10] = np.nansum(off, 1) > 0, pa[:, 4]
    pa[:, 11] = (pa[:, 9] > 0) | (pa[:, 10] > 0)
    E_agent = np.full((B, 4), np.nan)
    if traj.shape[1]:
        pa[:, 12:], E_agent = comfort(traj)
    else:
        pa[:, 12:] = np.nan
    ps, E_scene = np.zeros((S, SCENE_COLS)), np.zeros((S, 4))
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(S):
            r = slice(ss[s], ss[s + 1])
            n = ss[s + 1] - ss[s]
            ps[s, 0], ps[s, 1] = pa[r, 2].sum() / pa[r, 1].sum(), pa[r, 2].sum() / n
            ps[s, 2], ps[s, 3] = pa[r, 3].sum() / pa[r, 1].sum(), pa[r, 3].sum() / n
            ps[s, 4:7], ps[s, 7], ps[s, 8] = pa[r, 5:8].mean(0), pa[r, 4].mean(), pa[r, 8].mean()
            ps[s, 9:12] = pa[r, 9:12].mean(0)
            for k in range(4):
                ps[s, 12 + k], E_scene[s, k] = _nanmean(pa[r, 12 + k]), _nanmean(E_agent[r, k])
    return pa, ps, E_agent, E_scene


def restate(case, cfg, world=None):
    """All steps of `case` (world [T,B,3]; default: the case's) -> dict(steps, per_agent, per_scene, E_agent, E_scene, flags [T,B,4] uint8,
    partner [T,B] int32, dist_margin, pix_margin)."""
    world = case["world"] if world is None else world
    w64 = np.asarray(world, np.float64)
    steps = [restate_step(case, cfg, w64[t]) for t in range(w64.shape[0])]
    pa, ps, Ea, Es = aggregate(case, steps, np.transpose(w64, (1, 0, 2)))
    nan255 = lambda x: np.where(np.isnan(x), 255, x).astype(np.uint8)
    flags = np.stack([np.stack([nan255(s["off"]), nan255(s["disk"]), s["coll_disk"].astype(np.uint8), s["code"].astype(np.uint8)], -1)
                      for s in steps])
    return dict(steps=steps, per_agent=pa, per_scene=ps, E_agent=Ea, E_scene=Es, flags=flags,
                partner=np.stack([s["partner"] for s in steps]).astype(np.int32),
                dist_margin=min(s["dist_margin"] for s in steps), pix_margin=min(s["pix_margin"] for s in steps))


# ------------------------------------------------------------------------------------------------ the case
def _q(x, bits=10):
    return np.round(np.asarray(x, np.float64) * (1 << bits)) / (1 << bits)


def _maps(rng, centres, n_sem=3, size=96):
    """Two maps of 96 x 96 constant on 8 x 8 blocks in raster_cases.build_case's layout: scene s uses map s % 3, 2 meaning none."""
    S = len(centres)
    blocks = rng.integers(0, 3, (2, n_sem, size // 8, size // 8)).astype(np.float32) * 0.5
    maps = np.kron(blocks, np.ones((8, 8), np.float32)).copy()
    scene_map = np.array([s % 3 if s % 3 < 2 else -1 for s in range(S)], np.int32)
    mfw = np.zeros((2, 3, 3), np.float32)
    for m in range(2):
        centre = centres[[s for s in range(S) if scene_map[s] == m][0]]
        th, sc = rng.uniform(-np.pi, np.pi), rng.uniform(1.8, 2.2)
        A = sc * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        mfw[m, :2, :2], mfw[m, :2, 2], mfw[m, 2, 2] = A, np.array([size / 2.0, size / 2.0]) - A @ centre + rng.uniform(-3.0, 3.0, 2), 1.0
    return maps, scene_map, mfw


_BUILT = (  # (x, y) of the built pairs of scene 5 relative to its base, every heading 0, every box 4 x 2.125 (header of build_case below)
    (0.0, 0.0), (3.5, 0.25), (0.0, 20.0), (0.25, 21.5), (3.0, 40.5), (0.0, 40.0), (0.5, 41.0), (0.0, 60.0), (4.0 + 2.0 ** -8, 60.0),
    (0.0, 80.0), (0.0, 82.125 + 2.0 ** -8), (0.0, 100.0), (0.0, 102.125 - 2.0 ** -8), (0.0, 120.0))


def build_case(seed=2025):
    """-> dict(world [21,330,3] float32, extent [330,3] float32, scene_start, maps, scene_map, map_from_world, redrawn).
    Scene 1: agent 0 is 180 x 176 m, so its disk samples are clamped at all four borders of both rasters;
    agent 1 stands 250 m away.  Scene 5 (no map) opens with 14 standing agents, boxes 4 x 2.125 at heading 0 (a width whose disk samples keep the pixel margin): 0/1 front and rear, 2/3 left
    and right, 5 overlaps 4 (farther, the partner) and 6 (nearer), 7/8 a box gap of 2^-8 m, 9/10 a disk and box gap of 2^-8 m, 11/12 an
    overlap of 2^-8 m, 13 alone.  Every other agent drives an arc (speed, acceleration, yaw rate drawn), each step shifted (by up to
    1/16 m, more after 64 failed draws) until its margins hold.  Afterwards a few agents are NaN on some steps and the last agent of scene 4 on all of them."""
    rng = np.random.default_rng(seed)
    cfgs = [cfg_of(n) for n in RASTERS]
    S, T = len(SCENE_SIZES), N_STEPS
    ss = np.concatenate([[0], np.cumsum(SCENE_SIZES)]).astype(np.int32)
    centres = [_q(rng.uniform(-30.0, 30.0, 2)) for _ in range(S)]
    maps, scene_map, mfw = _maps(rng, centres)
    case = dict(scene_start=ss, maps=maps, scene_map=scene_map, map_from_world=mfw)
    B = int(ss[-1])
    world, extent = np.zeros((T, B, 3)), np.zeros((B, 3))
    redrawn = 0
    tt = SIM_DT * np.arange(T)
    for s, n in enumerate(SCENE_SIZES):
        for k in range(n):
            i = ss[s] + k
            built = s == CONSTRUCTED_SCENE and k < N_CONSTRUCTED
            while True:                                              # the extent: its disk samples keep the pixel margin in both rasters
                e = np.array([180.0, 176.0]) if (s == GIANT and k == 0) else np.array([4.0, 2.125]) if built else \
                    _q(np.array([rng.uniform(3.5, 5.5), rng.uniform(1.6, 2.4)]), 6)
                if min(sample_pixels(e, c)[2] for c in cfgs) >= 2 * PIX_MARGIN:
                    break
            extent[i] = [e[0], e[1], 1.5]
            if built:
                world[:, i, :2] = centres[s] + np.array([200.0, -60.0]) + np.array(_BUILT[k])
                continue
            p0 = centres[s] + (np.array([250.0, 250.0]) if (s == GIANT and k == 1) else rng.uniform(-28.0, 28.0, 2))
            h0, v0, a, w = rng.uniform(-np.pi, np.pi), rng.uniform(0.0, 10.0), rng.uniform(-2.0, 2.0), rng.uniform(-0.3, 0.3)
            h = np.float32(h0 + w * tt).astype(np.float64)
            dist = np.maximum(v0 * tt + 0.5 * a * tt * tt, 0.0)
            nominal = p0 + dist[:, None] * np.stack([np.cos(h0 + 0.5 * w * tt), np.sin(h0 + 0.5 * w * tt)], -1)
            world[:, i, 2] = h
            prev = np.arange(ss[s], i)
            for t in range(T):
                for attempt in range(10000):
                    amp = min(2.0 ** (attempt // 64) / 16.0, 8.0)                 # (a deep overlap with tied sides needs a larger shift)
                    p = _q(nominal[t] + (rng.uniform(-amp, amp, 2) if attempt else 0.0))
                    pose = np.array([p[0], p[1], h[t]])
                    ok = True
                    for c in cfgs:
                        u, v, _ = sample_pixels(e, c)
                        ok = ok and drv_at(case, c, s, pose, u, v)[1] >= 2 * PIX_MARGIN
                    if ok and len(prev):
                        Pj, Ej = world[t, prev], extent[prev, :2]
                        ok = min(pair_tests(pose[None], e[None], Pj, Ej)["margin"].min(),
                                 pair_tests(Pj, Ej, pose[None], e[None])["margin"].min()) >= 2 * DIST_MARGIN
                    if ok:
                        break
                    redrawn += 1
                else:
                    raise RuntimeError(f"metrics_cases.build_case: step {t} of agent {k} of scene {s} did not settle")
                world[t, i, :2] = p
    world = world.astype(np.float32)
    for i, steps in ((ss[2] + 1, (0,)), (ss[3] + 7, (5, 6)), (ss[3] + 20, (9, 10, 11)), (ss[5] + 30, (20,)), (ss[6] + 64, (15,)),
                     (ss[6] + 129, (3, 4))):
        world[list(steps), i, :2] = np.nan
    world[:, ss[5] - 1, :2] = np.nan                                 # the last agent of scene 4: absent throughout
    case.update(world=world, extent=extent.astype(np.float32), redrawn=redrawn)
    return case


def absent_scene_case():
    """A one-agent scene whose agent is NaN on every step, beside a scene of two agents that touch on some steps; 11 steps, no map."""
    T = 11
    world = np.zeros((T, 3, 3), np.float32)
    world[:, 0, :2] = np.nan
    world[:, 1, 0] = _q(0.75 * np.arange(T))                        # drives past the standing agent 2, 1.5 m to its side
    world[:, 1, 1] = 1.5
    world[:, 2, 0], world[:, 2, 2] = 4.0, 0.5
    extent = np.array([[4.0, 2.125, 1.5]] * 3, np.float32)
    return dict(world=world, extent=extent, scene_start=np.array([0, 1, 3], np.int32), maps=None)


_CASE = {}


def case():
    if "c" not in _CASE:
        _CASE["c"] = build_case()
    return _CASE["c"]


def load_golden(path):
    """tests/golden/rollout_metrics.npz -> (case dict from the stored inputs, the npz)."""
    z = np.load(path)
    return {k: z[k] for k in ("world", "extent", "scene_start", "maps", "scene_map", "map_from_world")}, z
