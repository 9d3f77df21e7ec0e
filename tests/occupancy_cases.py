"""fp64 restatement of the occupancy coverage and diversity metrics (include/cld.h `cld_occupancy_splat` / `cld_occupancy_mark` /
`cld_occupancy_read`) and the seeded case of their tests.

The restatement keeps upstream's sparse dicts (src/tbsim/envs/env_metrics.py:977-1218) and follows its arithmetic operation by operation in
numpy float64 -- the centre cell by np.round, the kernel as exp(-norm^2 / 2 / sigma), the dict sum in upstream's order of steps, agents
and window cells -- with this project's stated differences: an absent agent adds nothing, the lane flag is the map's value at the cell's
world point, and a cell outside the scene's window is dropped and counted.

The case: three scenes of 1, 40 and 20 agents (the last without a map), 21 steps, two episodes with different failed sets.  Coordinates
are multiples of 2^-10 m.  The one map is constant on blocks of 5 x 5 pixels at 2.5 px / m whose boundaries are the odd integers of the world
frame, and both grids' points are even integers: every drivable boundary is 1 m from every grid point, farther than the 0.71 m by which the
raster pixel upstream looks a grid point up in can miss it.  `world_full` has every agent present (what the golden was recorded from);
`world` is the same with one agent absent throughout and a few on some steps."""
import numpy as np

SCENE_SIZES = (1, 40, 20)
N_STEPS, N_EPISODES = 21, 2
GRIDS = {
    "coverage": dict(offset=(0.0, 0.0), step=(2.0, 2.0), sigma=1.0),
    "diversity": dict(offset=(2.0, -2.0), step=(4.0, 4.0), sigma=1.0),
    "wide": dict(offset=(0.0, 0.0), step=(2.0, 2.0), sigma=4.0),          # the 9 x 9 window: more cells than a wave has lanes
}
THRESHOLD = 1e-2
KERNEL_CUT = 0.1
NO_MAP_FILL = -1.0
N_SEM, MAP_SIZE, MAP_SCALE, MAP_SHIFT = 3, 128, 2.5, 63.0
GOLDEN_REACH, DROP_REACH = 100.0, 4.0      # the default window margin, and one small enough that agents drive out of their windows
RASTER = dict(height=64, width=64, px_per_m=2.0, ego_center=(0.0, 0.0), no_map_fill=NO_MAP_FILL, n_sem=N_SEM)      # the recording's rasters
LONE_FAILED, LONE_MIXED = 39, 40           # rows of scene 1's two isolated agents: failed in both episodes / in episode 0 only
ABSENT_ALWAYS, ABSENT_SOME = 17, ((5, (0, 1)), (23, (9, 10, 11)), (47, (20,)))
Q = float(1 << 40)
# the largest relative deviation of the default transport solver from the closed forms of
# tests/test_occupancy_host.py was 4.6e-15; ten times that for the termination tolerance of the LP
SOLVER_RTOL = 5e-14


def half_width(cfg):
    """OccupancyGrid.update + get_neighboring_grid_points: Nx = Ny = int(ceil(radius / xs)) + 1."""
    radius = np.sqrt(-2 * cfg["sigma"] * np.log(KERNEL_CUT))
    return int(np.ceil(radius / cfg["step"][0])) + 1


def _q(x, bits=10):
    return np.round(np.asarray(x, np.float64) * (1 << bits)) / (1 << bits)


def block_of(pixel):
    """The block a map pixel lies in: the boundary between pixels k and k + 1 is the world coordinate (k + 0.5 - 63) / 2.5, an odd integer
    exactly when k is a multiple of 5."""
    return (np.asarray(pixel) + 4) // 5


def build_case(seed=2026):
    """-> dict(scene_start, world_full [2,21,61,3] float32, world (the same with absences), failed [2,61] uint8, maps [1,3,128,128],
    scene_map, map_from_world)."""
    rng = np.random.default_rng(seed)
    ss = np.concatenate([[0], np.cumsum(SCENE_SIZES)]).astype(np.int32)
    B, T, E = int(ss[-1]), N_STEPS, N_EPISODES
    nb = int(block_of(MAP_SIZE - 1)) + 1
    blocks = rng.integers(0, 3, (1, N_SEM, nb, nb)).astype(np.float32) * 0.5
    blocks[0, 0, [0, -1], :] = 1.0                                   # the map's rim is drivable, as the fill outside it is: no boundary at its edge
    blocks[0, 0, :, [0, -1]] = 1.0
    idx = block_of(np.arange(MAP_SIZE))
    maps = blocks[:, :, idx][:, :, :, idx].copy()
    mfw = np.array([[[MAP_SCALE, 0.0, MAP_SHIFT], [0.0, MAP_SCALE, MAP_SHIFT], [0.0, 0.0, 1.0]]], np.float32)
    scene_map = np.array([0, 0, -1], np.int32)
    centres = (np.array([0.0, 0.0]), np.array([0.0, 0.0]), np.array([200.0, -100.0]))
    tt = 0.1 * np.arange(T)
    world = np.zeros((E, T, B, 3))
    for s, n in enumerate(SCENE_SIZES):
        start = _q(centres[s] + rng.uniform(-12.0, 12.0, (n, 2)))
        for e in range(E):
            for k in range(n):
                i = ss[s] + k
                h0, v0, a, w = rng.uniform(-np.pi, np.pi), rng.uniform(0.0, 5.0), rng.uniform(-1.0, 1.0), rng.uniform(-0.3, 0.3)
                dist = np.maximum(v0 * tt + 0.5 * a * tt * tt, 0.0)
                world[e, :, i, :2] = _q(start[k] + dist[:, None] * np.stack([np.cos(h0 + 0.5 * w * tt), np.sin(h0 + 0.5 * w * tt)], -1))
                world[e, :, i, 2] = _q(h0 + w * tt)
    # scene 0: one agent along y = -3 (a tie of the coverage grid: -1.5 -> -2) through x = 1, 3 (coverage ties) and x = 4, 8 (diversity ties)
    for e in range(E):
        world[e, :, 0, 0], world[e, :, 0, 1], world[e, :, 0, 2] = -1.0 + 0.5 * np.arange(T) + 2.0 * e, -3.0, 0.0
    # scene 1: rows 1 and 2 drive side by side, half a metre apart (several agents on one cell at one step)
    a, b = ss[1], ss[1] + 1
    world[:, :, b, :2], world[:, :, b, 2] = world[:, :, a, :2] + np.array([0.5, 0.0]), world[:, :, a, 2]
    # two agents that stand alone, far from the others and outside the map (fill: drivable): their cells have one writer each
    world[:, :, LONE_FAILED, :2], world[:, :, LONE_MIXED, :2] = np.array([-60.0, 40.0]), np.array([61.0, 41.0])
    world_full = world.astype(np.float32)
    assert np.array_equal(world_full[..., :2].astype(np.float64), world[..., :2])
    absent = world_full.copy()
    absent[:, :, ABSENT_ALWAYS, :2] = np.nan
    for row, steps in ABSENT_SOME:
        absent[:, list(steps), row, :2] = np.nan
    failed = (rng.uniform(size=(E, B)) < 0.3).astype(np.uint8)
    failed[:, LONE_FAILED] = 1
    failed[0, LONE_MIXED], failed[1, LONE_MIXED] = 1, 0
    failed[:, 0] = (0, 1)
    return dict(scene_start=ss, world_full=world_full, world=absent, failed=failed, maps=maps, scene_map=scene_map, map_from_world=mfw)


_CASE = {}


def case():
    if "c" not in _CASE:
        _CASE["c"] = build_case()
    return _CASE["c"]


INPUT_KEYS = ("scene_start", "world_full", "failed", "maps", "scene_map", "map_from_world")


def distance_matrix(upper_squares, n):
    """The distance matrix the golden keeps as the integer squares of its upper triangle (record_occupancy_golden.py) -> [n,n] float64."""
    D = np.zeros((n, n))
    D[np.triu_indices(n, 1)] = np.sqrt(np.asarray(upper_squares, np.float64))
    return D + D.T


def load_golden(path):
    """tests/golden/occupancy.npz -> (case dict from the stored inputs, the npz)."""
    z = np.load(path)
    c = {k: z[k] for k in INPUT_KEYS}
    return c, z


# ------------------------------------------------------------------------------------------------ the restatement
def windows(world0, scene_start, cfg, reach):
    """OccupancyMetrics' default windows: per scene the bounding box of its present agents in world0 +- reach, in cells ->
    [S,4] int64 (ix0, iy0, nx, ny)."""
    out = []
    o, st = np.asarray(cfg["offset"], np.float64), np.asarray(cfg["step"], np.float64)
    for s in range(len(scene_start) - 1):
        p = np.asarray(world0, np.float64)[scene_start[s]:scene_start[s + 1], :2]
        p = p[~np.isnan(p).any(1)]
        lo, hi = np.floor((p.min(0) - reach - o) / st), np.ceil((p.max(0) + reach - o) / st)
        out.append([lo[0], lo[1], hi[0] - lo[0] + 1, hi[1] - lo[1] + 1])
    return np.array(out, np.int64)


def lane_of(case, cfg, scene, cells):
    """The lane flag of cells [n,2] (int) of `scene`: the map's drivable value at the cell's world point, include/cld.h."""
    cells = np.asarray(cells, np.int64).reshape(-1, 2)
    m = int(case["scene_map"][scene]) if case.get("maps") is not None else -1
    if m < 0:
        return np.full(len(cells), NO_MAP_FILL != 0, bool)
    g = cells * np.asarray(cfg["step"], np.float64) + np.asarray(cfg["offset"], np.float64)
    M = case["map_from_world"][m].astype(np.float64)
    mx = np.rint(M[0, 0] * g[:, 0] + M[0, 1] * g[:, 1] + M[0, 2]).astype(np.int64)
    my = np.rint(M[1, 0] * g[:, 0] + M[1, 1] * g[:, 1] + M[1, 2]).astype(np.int64)
    mh, mw = case["maps"].shape[2:]
    inside = (mx >= 0) & (mx < mw) & (my >= 0) & (my < mh)
    vals = case["maps"][m, 0][np.clip(my, 0, mh - 1), np.clip(mx, 0, mw - 1)]
    return np.where(inside, vals, NO_MAP_FILL) != 0


def splat(cfg, coords):
    """OccupancyGrid.get_neighboring_grid_points for coords [n,2] float64 (no NaN) -> (cells [n,W*W,2] int64, kernel [n,W*W])."""
    N = half_width(cfg)
    o, st = np.asarray(cfg["offset"], np.float64), np.asarray(cfg["step"], np.float64)
    d = np.arange(-N, N + 1)
    grid = np.stack(np.meshgrid(d, d, indexing="ij"), -1).reshape(1, -1, 2)
    centre = np.round((coords - o) / st).astype(np.int64)
    cells = grid + centre[:, None]
    points = st * cells + o
    kernel = np.exp(-np.linalg.norm(coords[:, None] - points, axis=-1) ** 2 / 2 / cfg["sigma"])
    return cells, kernel


def restate_grid(case, cfg, world, episodes=None, win=None):
    """The sparse grids of every scene after the steps of `episodes` (default: all) of world [E,T,B,3] -> a list over scenes of
    dict(value {cell: float}, adds {cell: int}, touch {cell: set of (episode, row)}, dropped int).  win [S,4]: cells outside are dropped."""
    ss = case["scene_start"]
    episodes = range(world.shape[0]) if episodes is None else episodes
    out = []
    for s in range(len(ss) - 1):
        value, adds, touch, dropped = {}, {}, {}, 0
        rows = np.arange(ss[s], ss[s + 1])
        for e in episodes:
            for t in range(world.shape[1]):
                xy = world[e, t, rows, :2].astype(np.float64)
                ok = ~np.isnan(xy).any(1)
                if not ok.any():
                    continue
                cells, kernel = splat(cfg, xy[ok])
                for row, cc, kk in zip(rows[ok], cells, kernel):
                    for (ci, cj), k in zip(cc.tolist(), kk.tolist()):
                        if win is not None and not (win[s, 0] <= ci < win[s, 0] + win[s, 2] and win[s, 1] <= cj < win[s, 1] + win[s, 3]):
                            dropped += 1
                            continue
                        key = (ci, cj)
                        value[key] = value.get(key, 0) + k
                        adds[key] = adds.get(key, 0) + 1
                        touch.setdefault(key, set()).add((e, int(row)))
        out.append(dict(value=value, adds=adds, touch=touch, dropped=dropped))
    return out


def coverage_counts(case, cfg, grids, failed, threshold=THRESHOLD):
    """OccupancyCoverage.summarize_grid on restated grids -> ([S,3] int64: total, onroad, success; per scene dict(cells, value, lane, ok))."""
    counts, detail = [], []
    for s, g in enumerate(grids):
        cells = np.array(sorted(g["value"]), np.int64).reshape(-1, 2)
        v = np.array([g["value"][tuple(c)] for c in cells.tolist()])
        lane = lane_of(case, cfg, s, cells).astype(np.float64)
        ok = np.array([any(not failed[e, a] for e, a in g["touch"][tuple(c)]) for c in cells.tolist()], bool)
        counts.append([(v > threshold).sum(), (v * lane > threshold).sum(), (v * lane * ok > threshold).sum()])
        detail.append(dict(cells=cells, value=v, lane=lane, ok=ok, adds=np.array([g["adds"][tuple(c)] for c in cells.tolist()])))
    return np.array(counts, np.int64), detail


def distributions(case, cfg, world, win=None):
    """OccupancyDiversity.get_multi_episode_metrics up to the solver -> per scene dict(cells [n,2] the sorted union of touched cells,
    points [n,2], distr [E,n], adds [E,n], mass [E], D [n,n])."""
    E = world.shape[0]
    per_ep = [restate_grid(case, cfg, world, [e], win) for e in range(E)]
    out = []
    o, st = np.asarray(cfg["offset"], np.float64), np.asarray(cfg["step"], np.float64)
    for s in range(len(case["scene_start"]) - 1):
        keys = sorted(set().union(*[per_ep[e][s]["value"].keys() for e in range(E)]))
        cells = np.array(keys, np.int64).reshape(-1, 2)
        lane = lane_of(case, cfg, s, cells).astype(np.float64)
        v = np.array([[per_ep[e][s]["value"].get(k, 0) for k in keys] for e in range(E)], np.float64) * lane
        adds = np.array([[per_ep[e][s]["adds"].get(k, 0) for k in keys] for e in range(E)], np.int64)
        points = cells * st + o
        coords = np.tile(points, (points.shape[0], 1, 1))
        with np.errstate(invalid="ignore", divide="ignore"):
            distr = v / v.sum(1, keepdims=True)
        out.append(dict(cells=cells, points=points, distr=distr, adds=adds, mass=v.sum(1),
                        D=np.linalg.norm(coords - coords.transpose(1, 0, 2), axis=2)))
    return out


def diversity(dists, solver):
    """The mean over episode pairs, in upstream's order, per scene."""
    res = []
    for d in dists:
        E = d["distr"].shape[0]
        w = [solver(d["distr"][i], d["distr"][j], d["D"]) for i in range(E) for j in range(i)]
        res.append(np.mean(w) if w and not np.isnan(d["distr"]).any() else np.nan)
    return np.array(res)


def dense(win_row, cells, values, dtype=np.float64):
    """Scatter sparse cells [n,2] into the dense row-major [nx, ny] plane of a window (ix0, iy0, nx, ny) -> [nx * ny]."""
    ix0, iy0, nx, ny = (int(v) for v in win_row)
    out = np.zeros(nx * ny, dtype)
    c = np.asarray(cells, np.int64).reshape(-1, 2)
    out[(c[:, 0] - ix0) * ny + (c[:, 1] - iy0)] = values
    return out
