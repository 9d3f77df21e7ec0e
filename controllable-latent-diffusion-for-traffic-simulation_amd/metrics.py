"""The episode metrics of a closed-loop rollout on the device: `RolloutMetrics` scores every environment step where the poses are, in
HBM, and answers with upstream's registry names and keys (src/tbsim/evaluation/env_builders.py:37-50: OffRoadRate, DiskOffRoadRate,
CollisionRate, DiskCollisionRate, CriticalFailure, Comfort of src/tbsim/envs/env_metrics.py).

The arithmetic is `cld_scene_metrics_step` / `cld_scene_metrics_read` (csrc/metrics_kernels.hip; include/cld.h defines every
quantity).  The bookkeeping here is the state buffer, the step counter and the poses, which move with `cld_world_step` exactly as
`SceneObserver.advance` moves its own, so the scored poses are the observer's history frames bit for bit.

`OccupancyMetrics` is the registry's other two entries, all_coverage and all_diversity (env_builders.py:43-48: OccupancyCoverage,
OccupancyDiversity of env_metrics.py:977-1218): Q40 fixed-point occupancy planes filled with integer atomics, one launch per environment
step and grid (`cld_occupancy_splat` / `cld_occupancy_mark` / `cld_occupancy_read`; csrc/occupancy_kernels.hip).  Only the transport
problem of the diversity value leaves the device (`emd_linprog`).

`RealismDeviation` is the test stage's other number (src/trainers/guide_dm_trainer.py:204-295): the mean Wasserstein-1 distance between
ground truth and prediction of three quantities, accumulated and evaluated on the device (`cld_realism_terms`, `cld_sort_f32`,
`cld_wasserstein_f32`; csrc/realism_kernels.hip).

`GuidanceMetrics` says whether the guidance worked: upstream's guidance satisfaction metrics (src/tbsim/utils/guidance_metrics.py), one
to three per entry of the guidance config `set_guidance` takes, under upstream's keys `guide_<metric>_s<scene>g<config>`; one launch per
environment step (`cld_guide_metrics_step` / `cld_guide_metrics_read`; csrc/guide_metrics_kernels.hip).

`SampleMetrics` is the open-loop side: the ADE / FDE / APD / FPD keys upstream validates its diffusion model with
(DiffuserTrafficModel._compute_metrics, src/tbsim/algos/algos.py:1818-1852), per agent and as batch means in fp64 (`cld_sample_metrics`;
csrc/sample_metrics_kernels.hip, include/cld_eval.h).
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import CldError
from .observe import RASTER_DEFAULTS

_RASTER_KEYS = ("height", "width", "px_per_m", "ego_center", "no_map_fill", "n_sem")


class RolloutMetrics:
    """scene_start [num_scenes + 1]; extent [B_all,3] (length along the heading, width, height); world0 [B_all,3] the world poses
    (x, y, h) the first plans start from; maps / scene_map / map_from_world as `SceneObserver` takes them; `drivable_layer` the map
    layer that is the drivable area; `sim_dt`, `stat_dt` as upstream's Comfort; `raster_cfg`: height, width, px_per_m, ego_center,
    no_map_fill, n_sem (RASTER_DEFAULTS) -- the raster the off-road tests are defined on.  Pass it as `metrics=` to
    `closed_loop_rollout`, or feed it yourself with `add_step` / `add_plans`."""

    def __init__(self, engine, scene_start, extent, world0, maps=None, scene_map=None, map_from_world=None, drivable_layer: int = 0,
                 sim_dt: float = 0.1, stat_dt: float = 0.5, n_step_action: int = 5, **raster_cfg):
        unknown = sorted(set(raster_cfg) - set(_RASTER_KEYS))
        if unknown:
            raise TypeError(f"RolloutMetrics: unknown raster settings {unknown} (one of {sorted(_RASTER_KEYS)})")
        self.engine = engine
        self.cfg = {k: raster_cfg.get(k, RASTER_DEFAULTS[k]) for k in _RASTER_KEYS}
        if not float(stat_dt) >= float(sim_dt) > 0.0:
            raise CldError(f"RolloutMetrics: needs 0 < sim_dt <= stat_dt, got sim_dt = {sim_dt}, stat_dt = {stat_dt}")
        self.n_step_action = int(n_step_action)
        if not 1 <= self.n_step_action <= 52:
            raise CldError(f"RolloutMetrics: n_step_action = {n_step_action} (1 .. 52)")
        self._setup = engine.scene_metrics_setup(scene_start, extent, maps, scene_map, map_from_world, drivable_layer=drivable_layer, sim_dt=sim_dt,
                                                 stat_dt=stat_dt, **self.cfg)
        self.B_all, self.num_scenes = self._setup[1], self._setup[2]
        self.poses = torch.as_tensor(world0).to(engine.device, torch.float32).contiguous().clone()
        if tuple(self.poses.shape) != (self.B_all, 3):
            raise CldError(f"RolloutMetrics: world0 must be [{self.B_all},3], got {tuple(self.poses.shape)}")
        self.state = engine.scene_metrics_state(self.B_all)
        self.steps = 0

    def reset(self, world0=None):
        """Empty the state (and optionally set the poses the next plans start from)."""
        self.state.zero_()
        self.steps = 0
        if world0 is not None:
            w = torch.as_tensor(world0).to(self.engine.device, torch.float32).contiguous().clone()
            if tuple(w.shape) != (self.B_all, 3):
                raise CldError(f"RolloutMetrics: world0 must be [{self.B_all},3], got {tuple(w.shape)}")
            self.poses = w

    def add_step(self, world, want_flags: bool = False):
        """One environment step: world [B_all,3] (x, y, h), NaN x or y = the agent is absent.  No host synchronisation.  With
        want_flags -> (flags [B_all,4] uint8: off_road, off_road_disk (255: absent), coll_disk, box code 0 / 1 FRONT / 2 REAR /
        3 SIDE; partner [B_all] int32, -1: none)."""
        out = self.engine.scene_metrics_step(self._setup, world, self.state, self.steps, want_flags=want_flags)
        self.steps += 1
        return out

    def add_plans(self, plans_all):
        """The `n_step_action` executed states of every agent's plan [B_all,52,6] (agent frame at planning time), taken to the world
        as `SceneObserver.advance` takes them, each scored as one environment step; the poses move to the last of them.  These are the
        states AFTER each action; `GuidanceMetrics.add_plans` scores the states BEFORE each action, as upstream's environment feeds its
        guidance metrics."""
        plans = torch.as_tensor(plans_all).to(self.engine.device, torch.float32).contiguous()
        if tuple(plans.shape) != (self.B_all, 52, 6):
            raise CldError(f"RolloutMetrics: plans must cover all {self.B_all} agents as [{self.B_all},52,6], got {tuple(plans.shape)}")
        centroid, yaw = self.poses[:, :2].contiguous(), self.poses[:, 2].contiguous()
        world = None
        for k in range(self.n_step_action):
            world = self.engine.world_step(plans, centroid, yaw, k)[0]
            self.add_step(world)
        self.poses = world

    def per_agent(self):
        """-> the per-agent table [B_all,16] (include/cld.h `cld_scene_metrics_read`; the columns are _lib.METRICS_AGENT_COLS)."""
        return self.engine.scene_metrics_read(self._setup, self.state)[0]

    def get_episode_metrics(self):
        """Upstream's `get_episode_metrics()` of the six classes under their registry names; every value a [num_scenes] tensor on the
        device.  CriticalFailure counts one frame as a failure: upstream's class discards its num_*_frames arguments."""
        s = self.engine.scene_metrics_read(self._setup, self.state)[1]
        zero = torch.zeros_like(s[:, 0])
        return {
            "all_off_road_rate": {"rate": s[:, 0], "nframe": s[:, 1]},
            "all_disk_off_road_rate": {"rate": s[:, 2], "nframe": s[:, 3]},
            "all_collision_rate": {"CollisionType.FRONT": s[:, 4], "CollisionType.REAR": s[:, 5], "CollisionType.SIDE": s[:, 6],
                                   "coll_any": s[:, 7]},
            "all_disk_collision_rate": {"CollisionType.FRONT": zero, "CollisionType.REAR": zero, "CollisionType.SIDE": zero,
                                        "coll_any": s[:, 8]},
            "all_failure": {"failure_offroad": s[:, 9], "failure_collision": s[:, 10], "failure_any": s[:, 11]},
            "all_comfort": {"speed": s[:, 12], "lon_acc": s[:, 13], "lat_acc": s[:, 14], "jerk": s[:, 15]},
        }


COVERAGE_DEFAULTS = dict(offset=(0.0, 0.0), step=(2.0, 2.0), sigma=1.0, threshold=1e-2)      # env_builders.py:43-45
DIVERSITY_DEFAULTS = dict(offset=(0.0, 0.0), step=(4.0, 4.0), sigma=1.0)                    # env_builders.py:46-48
_DEFAULT = object()
EMD_MAX_CELLS = 1024      # the default transport solver refuses a pair with more cells of mass than this (an LP of EMD_MAX_CELLS^2 flows)


def emd_linprog(distr_i, distr_j, distance_matrix):
    """pyemd.emd's signature on scipy: the cost of the cheapest transport of distr_i onto distr_j under `distance_matrix`, by
    scipy.optimize.linprog(method="highs") with sparse constraints.  Only cells with mass in either distribution enter (the others carry
    no flow at the optimum).  scipy is imported here and nowhere else in the package."""
    import numpy as np
    try:
        from scipy.optimize import linprog
        from scipy.sparse import csr_matrix
    except ImportError as err:
        raise CldError("OccupancyMetrics.diversity: the default solver needs scipy (pass solver=, pyemd.emd's signature)") from err
    p, q, D = np.asarray(distr_i, np.float64), np.asarray(distr_j, np.float64), np.asarray(distance_matrix, np.float64)
    keep = np.flatnonzero((p > 0) | (q > 0))
    n = int(keep.size)
    if n > EMD_MAX_CELLS:
        raise CldError(f"OccupancyMetrics.diversity: {n} cells carry mass, the default solver takes at most {EMD_MAX_CELLS} (pass solver=)")
    if n == 0:
        return 0.0
    p, q, D = p[keep], q[keep], D[np.ix_(keep, keep)]
    flow = np.arange(n * n)                                          # flow f[a, b] from cell a of p to cell b of q, row-major
    A = csr_matrix((np.ones(2 * n * n), (np.concatenate([flow // n, n + flow % n]), np.concatenate([flow, flow]))), shape=(2 * n, n * n))
    res = linprog(D.reshape(-1), A_eq=A, b_eq=np.concatenate([p, q]), bounds=(0, None), method="highs")
    if res.status != 0:
        raise CldError(f"OccupancyMetrics.diversity: linprog did not converge ({res.message})")
    return float(res.fun)


class OccupancyMetrics:
    """Upstream's two occupancy metrics on the device (src/tbsim/envs/env_metrics.py:977-1218; include/cld.h `cld_occupancy_splat` defines
    every quantity): `all_coverage` = OccupancyCoverage, one grid over all episodes since `reset()`, and `all_diversity` =
    OccupancyDiversity, one grid per episode.

    scene_start [num_scenes + 1]; world0 [B_all,3] the world poses the first plans start from; maps / scene_map / map_from_world /
    drivable_layer / no_map_fill as `RolloutMetrics` takes them; `coverage`: dict(offset, step, sigma, threshold) and `diversity`:
    dict(offset, step, sigma) over COVERAGE_DEFAULTS / DIVERSITY_DEFAULTS, either may be None (not computed).  A scene's grid is a
    window of cells: by default the bounding box of its agents in world0 (absent ones left out) +- `reach` metres; `window` =
    [num_scenes,4] world boxes (x0, y0, x1, y1) instead.  What an agent's kernel window would add outside it is counted by `dropped()`.
    `max_episodes` bounds the episodes between two `reset()`s (the diversity planes are allocated up front).

    An episode: `begin_episode(world0)`, then `add_step(world)` per environment step or `add_plans(plans_all)` per plan (or pass the
    object in `metrics=` of `closed_loop_rollout`), then `end_episode(failed)`.  Nothing synchronises before a result is read."""

    def __init__(self, engine, scene_start, world0, maps=None, scene_map=None, map_from_world=None, drivable_layer: int = 0,
                 coverage=_DEFAULT, diversity=_DEFAULT, reach: float = 100.0, window=None, n_step_action: int = 5, max_episodes: int = 8,
                 no_map_fill: float = -1.0, n_sem: int = 3):
        self.engine = engine
        self.n_step_action = int(n_step_action)
        if not 1 <= self.n_step_action <= 52:
            raise CldError(f"OccupancyMetrics: n_step_action = {n_step_action} (1 .. 52)")
        self.max_episodes = int(max_episodes)
        if self.max_episodes < 1:
            raise CldError(f"OccupancyMetrics: max_episodes = {max_episodes} must be at least 1")
        host = torch.as_tensor(scene_start).to(torch.int64).reshape(-1).cpu()
        if host.numel() < 2 or int(host[0]) != 0 or bool((host[1:] <= host[:-1]).any()):
            raise CldError(f"OccupancyMetrics: scene_start {host.tolist()} does not split agents into scenes")
        self.B_all, self.num_scenes = int(host[-1]), int(host.numel()) - 1
        self._scene_start = host
        self._max_agents = int((host[1:] - host[:-1]).max())
        self.poses = self._world0(world0)
        boxes = self._boxes(window, float(reach))
        self._grids = {}
        for name, cfg, defaults in (("coverage", coverage, COVERAGE_DEFAULTS), ("diversity", diversity, DIVERSITY_DEFAULTS)):
            if cfg is None:
                continue
            cfg = dict(defaults, **({} if cfg is _DEFAULT else cfg))
            unknown = sorted(set(cfg) - set(defaults))
            if unknown:
                raise TypeError(f"OccupancyMetrics: unknown {name} settings {unknown} (one of {sorted(defaults)})")
            off, step = [float(v) for v in cfg["offset"]], [float(v) for v in cfg["step"]]
            if not (step[0] > 0.0 and step[1] > 0.0):
                raise CldError(f"OccupancyMetrics: the {name} grid needs a positive step, got {tuple(cfg['step'])}")
            lo = torch.floor((boxes[:, :2] - torch.tensor(off, dtype=torch.float64)) / torch.tensor(step, dtype=torch.float64))
            hi = torch.ceil((boxes[:, 2:] - torch.tensor(off, dtype=torch.float64)) / torch.tensor(step, dtype=torch.float64))
            if not bool(torch.isfinite(lo).all() and torch.isfinite(hi).all()) or bool((hi - lo >= 2 ** 30).any()):
                raise CldError(f"OccupancyMetrics: the {name} windows are not finite")
            win = torch.cat([lo, hi - lo + 1.0], 1).to(torch.int64)
            setup = engine.occupancy_setup(host, win, off, step, cfg["sigma"], 0.1, maps, scene_map, map_from_world, drivable_layer,
                                           no_map_fill, n_sem)
            if (2 * setup[4] + 1) ** 2 > _lib.OCCUPANCY_MAX_WINDOW_CELLS:
                raise CldError(f"OccupancyMetrics: the {name} kernel window is {2 * setup[4] + 1}^2 cells, above "
                               f"{_lib.OCCUPANCY_MAX_WINDOW_CELLS} (sigma too large for the step)")
            planes = self.max_episodes if name == "diversity" else 1
            self._grids[name] = dict(cfg=cfg, setup=setup, grid=torch.zeros(planes, setup[3], dtype=torch.int64, device=engine.device),
                                     dropped=torch.zeros(self.num_scenes, dtype=torch.int64, device=engine.device))
        if "coverage" in self._grids:
            self._success = torch.zeros(self._grids["coverage"]["setup"][3], dtype=torch.uint8, device=engine.device)
        self.episodes = 0            # episodes ended since reset()
        self._open = False
        self._steps = []             # the open episode's poses, replayed by end_episode
        self._adds = 0               # steps splatted into the coverage grid since reset()

    def _world0(self, world0):
        w = torch.as_tensor(world0).to(self.engine.device, torch.float32).contiguous().clone()
        if tuple(w.shape) != (self.B_all, 3):
            raise CldError(f"OccupancyMetrics: world0 must be [{self.B_all},3], got {tuple(w.shape)}")
        return w

    def _boxes(self, window, reach):
        """-> [num_scenes,4] float64 world boxes (x0, y0, x1, y1) on the host: `window`, or the agents of world0 +- reach."""
        S = self.num_scenes
        if window is not None:
            b = torch.as_tensor(window).to(torch.float64).cpu()
            if tuple(b.shape) != (S, 4) or not bool(torch.isfinite(b).all()) or bool((b[:, 2:] < b[:, :2]).any()):
                raise CldError(f"OccupancyMetrics: window must be [{S},4] finite world boxes (x0, y0, x1, y1)")
            return b
        if not reach >= 0.0:
            raise CldError(f"OccupancyMetrics: reach = {reach} must not be negative")
        xy = self.poses[:, :2].to(torch.float64).cpu()
        b = torch.zeros(S, 4, dtype=torch.float64)
        for s in range(S):
            p = xy[int(self._scene_start[s]):int(self._scene_start[s + 1])]
            p = p[~torch.isnan(p).any(1)]
            if p.numel() == 0:
                raise CldError(f"OccupancyMetrics: scene {s} has no present agent in world0 to place its window around (pass window=)")
            b[s, :2], b[s, 2:] = p.min(0).values - reach, p.max(0).values + reach
        return b

    # ---- feeding
    def reset(self):
        """Upstream's multi_episode_reset: every plane and counter is emptied (the poses stay)."""
        for g in self._grids.values():
            g["grid"].zero_()
            g["dropped"].zero_()
        if "coverage" in self._grids:
            self._success.zero_()
        self.episodes, self._open, self._steps, self._adds = 0, False, [], 0

    def begin_episode(self, world0=None):
        """Open the next episode (optionally setting the poses its first plans start from)."""
        if self._open:
            raise CldError("OccupancyMetrics.begin_episode: an episode is open (end_episode first)")
        if self.episodes >= self.max_episodes:
            raise CldError(f"OccupancyMetrics.begin_episode: max_episodes = {self.max_episodes} episodes have been fed (reset(), or build "
                           f"with a larger max_episodes)")
        if world0 is not None:
            self.poses = self._world0(world0)
        self._open, self._steps = True, []

    def add_step(self, world):
        """One environment step: world [B_all,3] (x, y, h), NaN x or y = the agent is absent.  One splat launch per grid, no host
        synchronisation.  Opens an episode when none is open."""
        if not self._open:
            self.begin_episode()
        if (self._adds + 1) * self._max_agents > 2 ** 24:
            raise CldError(f"OccupancyMetrics.add_step: {self._adds + 1} steps of a scene of {self._max_agents} agents could add more than "
                           f"2^24 times into one cell of the Q40 planes (reset() first)")
        world = self.engine._f32(world, (self.B_all, 3))
        for name, g in self._grids.items():
            plane = g["grid"][self.episodes if name == "diversity" else 0]
            self.engine.occupancy_splat(g["setup"], world, plane, g["dropped"])
        self._steps.append(world)
        self._adds += 1

    def add_plans(self, plans_all):
        """The `n_step_action` executed states of every agent's plan [B_all,52,6], taken to the world exactly as
        `RolloutMetrics.add_plans` takes them, each fed as one environment step; the poses move to the last of them."""
        plans = torch.as_tensor(plans_all).to(self.engine.device, torch.float32).contiguous()
        if tuple(plans.shape) != (self.B_all, 52, 6):
            raise CldError(f"OccupancyMetrics: plans must cover all {self.B_all} agents as [{self.B_all},52,6], got {tuple(plans.shape)}")
        centroid, yaw = self.poses[:, :2].contiguous(), self.poses[:, 2].contiguous()
        world = None
        for k in range(self.n_step_action):
            world = self.engine.world_step(plans, centroid, yaw, k)[0]
            self.add_step(world)
        self.poses = world

    def end_episode(self, failed):
        """Close the episode: failed [B_all] (non-zero: the agent failed in this episode, e.g. `rm.per_agent()[:, 11] != 0` of a
        `RolloutMetrics`).  The episode's poses are replayed once into the success plane (cld_occupancy_mark)."""
        if not self._open:
            raise CldError("OccupancyMetrics.end_episode: no episode is open")
        failed = torch.as_tensor(failed).to(self.engine.device).reshape(-1)
        if failed.numel() != self.B_all:
            raise CldError(f"OccupancyMetrics.end_episode: failed must be [{self.B_all}], got {failed.numel()} values")
        if "coverage" in self._grids and self._steps:
            self.engine.occupancy_mark(self._grids["coverage"]["setup"], torch.stack(self._steps), (failed == 0).to(torch.uint8),
                                       self._success)
        self.episodes += 1
        self._open, self._steps = False, []

    # ---- results
    def _grid(self, name: str, what: str):
        if name not in self._grids:
            raise CldError(f"OccupancyMetrics.{what}: built with {name}=None")
        if self._open:
            raise CldError(f"OccupancyMetrics.{what}: an episode is open (end_episode first)")
        return self._grids[name]

    def coverage(self):
        """OccupancyCoverage.summarize_grid over every episode since reset() -> {"total", "onroad", "success"}: int64 [num_scenes]
        device tensors."""
        g = self._grid("coverage", "coverage")
        c = self.engine.occupancy_read(g["setup"], g["grid"][0], self._success, threshold=g["cfg"]["threshold"])["counts"]
        return {"total": c[:, 0], "onroad": c[:, 1], "success": c[:, 2]}

    def dropped(self, grid: str = "coverage"):
        """-> [num_scenes] int64: the kernel-window cells that fell outside the scene's window since reset(), of grid "coverage" or
        "diversity".  Non-zero: the counts miss cells; build with a larger `reach` or `window`."""
        if grid not in self._grids:
            raise CldError(f"OccupancyMetrics.dropped: built with {grid}=None")
        return self._grids[grid]["dropped"]

    def cell_points(self, grid: str, scene: int):
        """-> [nx ny, 2] float64 device tensor: the world points of the cells of `scene`'s window, in the planes' order."""
        g = self._grids[grid]
        ix0, iy0, nx, ny = (int(v) for v in g["setup"][5][6][scene])
        dev = self.engine.device
        off, step = g["cfg"]["offset"], g["cfg"]["step"]
        gx = torch.arange(ix0, ix0 + nx, dtype=torch.float64, device=dev) * float(step[0]) + float(off[0])
        gy = torch.arange(iy0, iy0 + ny, dtype=torch.float64, device=dev) * float(step[1]) + float(off[1])
        return torch.stack([gx[:, None].expand(nx, ny), gy[None, :].expand(nx, ny)], -1).reshape(nx * ny, 2)

    def diversity_distributions(self):
        """-> per scene (points [n,2], distr [episodes,n]) float64 on the device: the world points of the scene's window cells and, per
        episode, OccupancyDiversity's distribution values lane / sum over them (a row without on-road mass is NaN).  Cells outside
        upstream's union of touched cells hold 0."""
        g = self._grid("diversity", "diversity_distributions")
        setup, E = g["setup"], self.episodes
        cs = g["setup"][5][7]
        rows = []
        for e in range(E):
            r = self.engine.occupancy_read(setup, g["grid"][e], counts=False, values=True, lane=True, mass=True)
            rows.append((r["values"] * r["lane"].to(torch.float64), r["mass"].to(torch.float64) / _lib.OCCUPANCY_Q))
        out = []
        for s in range(self.num_scenes):
            a, b = int(cs[s]), int(cs[s + 1])
            distr = torch.stack([v[a:b] / m[s] for v, m in rows]) if E else torch.zeros(0, b - a, dtype=torch.float64,
                                                                                      device=self.engine.device)
            out.append((self.cell_points("diversity", s), distr))
        return out

    def diversity(self, solver=None):
        """OccupancyDiversity.get_multi_episode_metrics -> [num_scenes] float64 (host): per scene the mean over episode pairs of the
        earth mover's distance of their distributions, ground distance Euclidean between cell points.  The transport problem is a
        linear programme and is solved on the host: `solver(distr_i, distr_j, distance_matrix)` with pyemd.emd's signature, default
        `emd_linprog`.  Fewer than two episodes, or an episode without on-road mass, give NaN, as upstream's arithmetic does."""
        import numpy as np
        solver = emd_linprog if solver is None else solver
        res = np.full(self.num_scenes, np.nan)
        for s, (pts, distr) in enumerate(self.diversity_distributions()):
            d = distr.cpu().numpy()
            if d.shape[0] < 2 or np.isnan(d).any():
                continue
            keep = np.flatnonzero((d > 0).any(0))                   # (cells without mass in any episode carry no flow)
            p, d = pts.cpu().numpy()[keep], d[:, keep]
            D = np.linalg.norm(p[:, None] - p[None], axis=2)
            res[s] = np.mean([solver(d[i], d[j], D) for i in range(d.shape[0]) for j in range(i)])
        return torch.from_numpy(res)


class RealismDeviation:
    """The realism deviation of the reference's test stage (src/trainers/guide_dm_trainer.py:204-295) on the device: the mean of the
    Wasserstein-1 distances between ground truth and prediction of the longitudinal acceleration, the lateral acceleration and the jerk
    of scaled [M,T,6] trajectories.  Six grow-by-doubling device buffers hold the values fed since `reset()`; their fill counts follow
    from the shapes and live on the host, so `add` issues no synchronisation.  `dt` is the config's step_time; `capacity` the values
    each buffer holds before it first grows.

    Upstream's `test_step` re-creates its list on every call, so its epoch value covers the LAST batch only; this accumulator covers
    everything fed since `reset()`.  `reset()` before every `add` reproduces upstream."""

    SIDES = ("gt", "pred")
    NAMES = ("lon", "lat", "jerk")

    def __init__(self, engine, dt: float = 0.1, capacity: int = 0):
        if not float(dt) > 0.0:
            raise CldError(f"RealismDeviation: dt = {dt} must be positive")
        self.engine = engine
        self.dt = float(dt)
        cap = max(int(capacity), 0)
        self._buf = {(s, n): torch.empty(cap, dtype=torch.float32, device=engine.device) for s in self.SIDES for n in self.NAMES}
        self._fill = {k: 0 for k in self._buf}

    def reset(self):
        """Empty the six buffers (their memory is kept)."""
        for k in self._fill:
            self._fill[k] = 0

    def _tail(self, key, count: int):
        """The next `count` slots of buffer `key`, after growing it (doubling, at least to fit) when they would overflow it."""
        buf, fill = self._buf[key], self._fill[key]
        if fill + count > buf.numel():
            grown = torch.empty(max(2 * buf.numel(), fill + count), dtype=torch.float32, device=self.engine.device)
            grown[:fill].copy_(buf[:fill])
            self._buf[key] = buf = grown
        return buf[fill:fill + count]

    def add(self, sa_gt, sa_pred):
        """One batch as `test_step` sees it: sa_gt = state_and_action, sa_pred = recon_state_and_action_scaled, each [M,T,6] scaled (the
        two may differ in M).  The terms kernel writes straight into the buffers' tails."""
        both = [self.engine._f32(sa) for sa in (sa_gt, sa_pred)]
        for sa in both:                                            # both sides are checked before either is appended
            if sa.dim() != 3 or sa.shape[2] != 6 or sa.shape[0] < 1 or sa.shape[1] < 2:
                raise CldError(f"RealismDeviation.add: expected [M >= 1, T >= 2, 6], got {tuple(sa.shape)}")
        for side, sa in zip(self.SIDES, both):
            M, T = int(sa.shape[0]), int(sa.shape[1])
            counts = dict(lon=M * T, lat=M * T, jerk=M * (T - 1))
            self.engine.realism_terms(sa, self.dt, out=tuple(self._tail((side, n), counts[n]) for n in self.NAMES))
            for n in self.NAMES:
                self._fill[(side, n)] += counts[n]

    def add_values(self, side: str, lon=None, lat=None, jerk=None):
        """Append ready-made values to one side ("gt" or "pred"): a closed loop compares simulated values with logged ones of another
        count this way."""
        if side not in self.SIDES:
            raise ValueError(f"RealismDeviation.add_values: side must be one of {self.SIDES}, got {side!r}")
        for n, vals in zip(self.NAMES, (lon, lat, jerk)):
            if vals is None:
                continue
            vals = self.engine._f32(vals).reshape(-1)
            if vals.numel():
                self._tail((side, n), vals.numel()).copy_(vals)
                self._fill[(side, n)] += vals.numel()

    def values(self):
        """-> {"gt": {"lon", "lat", "jerk"}, "pred": {...}}: the filled part of the six buffers (views).  A multi-rank caller all-gathers
        them and feeds another instance with `add_values`."""
        return {s: {n: self._buf[(s, n)][:self._fill[(s, n)]] for n in self.NAMES} for s in self.SIDES}

    def compute(self):
        """`on_test_epoch_end`: {"wd_long", "wd_lat", "wd_jerk", "realism_deviation"} as 0-d float64 device tensors: six sorts, three
        distances and their mean, all on the device.  The buffers are left as they are."""
        v = self.values()
        empty = [f"{s}/{n}" for s in self.SIDES for n in self.NAMES if v[s][n].numel() == 0]
        if empty:
            raise ValueError(f"RealismDeviation.compute: no values in {empty}")
        e = self.engine
        wd = [e.wasserstein_distance(e.sort(v["gt"][n]), e.sort(v["pred"][n]), presorted=True) for n in self.NAMES]
        return {"wd_long": wd[0], "wd_lat": wd[1], "wd_jerk": wd[2], "realism_deviation": (wd[0] + wd[1] + wd[2]) / 3.0}


# upstream's GUIDANCE_NAME_TO_METRICS (guidance_metrics.py:876-894) for the names built here, in its order; stop_sign and global_stop_sign
# need stlcg and the gpt* names a language-model front end: neither their losses nor their metrics are built
GUIDANCE_NAME_TO_METRICS = {
    "target_speed": ("target_speed",),
    "agent_collision": ("agent_collision_disk", "social_dist", "agent_collision"),
    "map_collision": ("map_collision", "map_collision_disk"),
    "target_pos_at_time": ("target_pos_at_time",),
    "target_pos": ("target_pos",),
    "global_target_pos_at_time": ("global_target_pos_at_time",),
    "global_target_pos": ("global_target_pos",),
    "social_group": ("social_group",),
    "speed_limit": ("speed_limit",),
    "acc_limit": ("acc_limit",),
}


def guidance_metric_names(guidance_config_list, constraint_config=None):
    """The keys `guidance_metrics_from_config(guidance_config_list)` registers, in its order, then those of
    `constraint_metrics_from_config(constraint_config)` (guidance_metrics.py:896-929).  Host only.  A name outside
    GUIDANCE_NAME_TO_METRICS raises ValueError("Unknown guidance metric: ..."), as upstream does."""
    keys = []
    for si, cfgs in enumerate(guidance_config_list):
        for ci, cfg in enumerate(cfgs):
            if cfg["name"] not in GUIDANCE_NAME_TO_METRICS:
                raise ValueError("Unknown guidance metric: {}".format(cfg["name"]))
            keys += ["guide_%s_s%dg%d" % (met, si, ci) for met in GUIDANCE_NAME_TO_METRICS[cfg["name"]]]
    for si, cfg in enumerate(constraint_config or ()):
        if cfg:
            keys.append("guide_constraint_s%d" % si)
    return keys


def guidance_metric_table(guidance_config_list, scene_start, constraint_config=None):
    """The entry table of `cld_guide_metrics` (include/cld.h) on the host: one dict per key of `guidance_metric_names`, in its order:
    `key`, `kind` (upstream's metric name), `scene`, `config` (index in the scene's list, None for a constraint), `members` (batch rows:
    the config's scene-local `agents` shifted by the scene's first row, or the whole scene), `excluded` (the batch rows of
    params['excluded_agents'] that lie in this scene, sorted), `excluded_local` (the same as scene-local indices, what upstream's metric
    classes take) and `params` (the flat float64 list of include/cld.h; a target_speed [B_all, L] indexed by batch row is sliced to the
    members' rows here, which is what upstream's TargetSpeedGuidance needs to be handed)."""
    import numpy as np
    ss = [int(v) for v in np.asarray(torch.as_tensor(scene_start).cpu()).reshape(-1)]
    S = len(ss) - 1
    if len(guidance_config_list) != S:
        raise ValueError(f"guidance config list must hold one entry per scene ({S}), got {len(guidance_config_list)}")
    if constraint_config is not None and len(constraint_config) != S:
        raise ValueError(f"constraint config must hold one entry per scene ({S}), got {len(constraint_config)}")
    guidance_metric_names(guidance_config_list, constraint_config)          # (unknown names raise before anything is built)

    def rows(si, agents):
        n = ss[si + 1] - ss[si]
        local = list(range(n)) if agents is None else [int(a) for a in agents]
        if not local or min(local) < 0 or max(local) >= n:
            raise ValueError(f"scene {si}: `agents` {agents} must name at least one of its {n} agents")
        return [ss[si] + a for a in local]

    def waypoints(si, name, pos, times, n):
        pos = np.asarray(pos, np.float64).reshape(-1, 2)
        if pos.shape[0] != n:
            raise ValueError(f"scene {si}: {name} needs one position per agent of the config ({n}), got {pos.shape[0]}")
        out = [float(v) for v in pos.reshape(-1)]
        if times is not None:
            t = np.asarray(times, np.float64).reshape(-1)
            if t.size not in (1, n):
                raise ValueError(f"scene {si}: {name} needs one time per agent of the config ({n}), got {t.size}")
            out += [float(v) for v in np.broadcast_to(t, (n,))]
        return out

    table = []
    for si, cfgs in enumerate(guidance_config_list):
        for ci, cfg in enumerate(cfgs):
            name, prm = cfg["name"], cfg.get("params") or {}
            members = rows(si, cfg.get("agents"))
            n = len(members)
            excl = sorted({int(b) for b in (prm.get("excluded_agents") or ()) if ss[si] <= int(b) < ss[si + 1]})
            for met in GUIDANCE_NAME_TO_METRICS[name]:
                params = []
                if met == "target_speed":
                    ts = np.asarray(torch.as_tensor(prm["target_speed"]).cpu(), np.float64)
                    if ts.ndim != 2 or ts.shape[0] < ss[-1]:
                        raise ValueError(f"scene {si}: target_speed must be [B_all = {ss[-1]}, L] (indexed by batch row), got {ts.shape}")
                    params = [float(ts.shape[1])] + [float(v) for v in ts[members].reshape(-1)]
                elif met in ("speed_limit", "acc_limit"):
                    params = [float(prm[met])]
                elif met == "social_dist":
                    params = [float(prm.get("buffer_dist", 0.2))]               # the default of guidance_from_config
                elif met == "social_group":
                    params = [float(prm["social_dist"])]
                elif met in ("target_pos", "global_target_pos"):
                    params = waypoints(si, met, prm["target_pos"], None, n)
                elif met in ("target_pos_at_time", "global_target_pos_at_time"):
                    params = waypoints(si, met, prm["target_pos"], prm["target_time"], n)
                uses_excl = met in ("agent_collision", "agent_collision_disk", "social_dist")
                table.append(dict(key="guide_%s_s%dg%d" % (met, si, ci), kind=met, scene=si, config=ci, members=members,
                                  excluded=excl if uses_excl else [], excluded_local=[b - ss[si] for b in excl] if uses_excl else [],
                                  params=params))
    for si, cfg in enumerate(constraint_config or ()):
        if not cfg:
            continue
        members = rows(si, cfg.get("agents"))
        table.append(dict(key="guide_constraint_s%d" % si, kind="target_pos_at_time", scene=si, config=None, members=members, excluded=[],
                          excluded_local=[], params=waypoints(si, "constraint", cfg["locs"], cfg["times"], len(members))))
    return table


class GuidanceMetrics:
    """Upstream's guidance satisfaction metrics on the device (src/tbsim/utils/guidance_metrics.py; include/cld.h
    `cld_guide_metrics_step` defines every quantity and the deliberate differences).

    `guidance_config_list` is exactly what `set_guidance` / `guidance_from_config` take: one list per scene (the scenes of other ranks
    included; a scene with an empty list has no entry) of {'name', 'weight', 'params', 'agents'}; `agents` are scene-local indices,
    params['excluded_agents'] are BATCH rows and params['target_speed'] is [B_all, L] indexed by batch row.  Upstream's metric classes
    index the last two by scene-local agent instead; the conversion happens here on the host, once (`guidance_metric_table`).
    `constraint_config`: per scene None or {'locs', 'times', 'agents'} (constraint_metrics_from_config).  scene_start, extent, maps /
    scene_map / map_from_world and `raster_cfg` as `RolloutMetrics` takes them; world0 [B_all,3], curr_speed0 / acc0 [B_all] (default
    zeros) are the state the first plans start from.

    Feed it with `add_step(world, speed, acc)` per environment step or `add_plans(plans_all)` per plan, or pass it in `metrics=` of
    `closed_loop_rollout` (e.g. `metrics=(rm, occ, gm)`).  Nothing synchronises before a value is read."""

    def __init__(self, engine, guidance_config_list, scene_start, extent, world0, curr_speed0=None, acc0=None, maps=None, scene_map=None,
                 map_from_world=None, constraint_config=None, n_step_action: int = 5, drivable_layer: int = 0, **raster_cfg):
        unknown = sorted(set(raster_cfg) - set(_RASTER_KEYS))
        if unknown:
            raise TypeError(f"GuidanceMetrics: unknown raster settings {unknown} (one of {sorted(_RASTER_KEYS)})")
        self.engine = engine
        self.cfg = {k: raster_cfg.get(k, RASTER_DEFAULTS[k]) for k in _RASTER_KEYS}
        self.n_step_action = int(n_step_action)
        if not 1 <= self.n_step_action <= 52:
            raise CldError(f"GuidanceMetrics: n_step_action = {n_step_action} (1 .. 52)")
        self.table = guidance_metric_table(guidance_config_list, scene_start, constraint_config)
        self.keys = [t["key"] for t in self.table]
        self._setup = engine.guide_metrics_setup(scene_start, extent, self.table, maps, scene_map, map_from_world,
                                                 drivable_layer=drivable_layer, **self.cfg)
        self.B_all, self.num_scenes = self._setup[1], self._setup[2]
        self._index = {k: n for n, k in enumerate(self.keys)}
        starts = [0]
        for t in self.table:
            starts.append(starts[-1] + len(t["members"]))
        self._member_start = starts
        self._entry_scene = torch.tensor([t["scene"] for t in self.table], dtype=torch.int64, device=engine.device)
        self.state = engine.guide_metrics_state(self._setup)
        self.steps = 0
        self.poses = self.speed = self.acc = None
        self._carry(world0, curr_speed0, acc0)

    def _carry(self, world, speed, acc):
        dev, B = self.engine.device, self.B_all
        if world is not None:
            w = torch.as_tensor(world).to(dev, torch.float32).contiguous().clone()
            if tuple(w.shape) != (B, 3):
                raise CldError(f"GuidanceMetrics: world0 must be [{B},3], got {tuple(w.shape)}")
            self.poses = w
        for name, v in (("speed", speed), ("acc", acc)):
            if v is None:
                if getattr(self, name) is None:
                    setattr(self, name, torch.zeros(B, dtype=torch.float32, device=dev))
                continue
            v = torch.as_tensor(v).to(dev, torch.float32).contiguous().clone()
            if tuple(v.shape) != (B,):
                raise CldError(f"GuidanceMetrics: curr_speed0 / acc0 must be [{B}], got {tuple(v.shape)}")
            setattr(self, name, v)

    def reset(self, world0=None, curr_speed0=None, acc0=None):
        """Empty the state (and optionally set the state the next plans start from)."""
        self.state.zero_()
        self.steps = 0
        self._carry(world0, curr_speed0, acc0)

    def add_step(self, world, speed, acc):
        """One environment step: world [B_all,3] (x, y, h; NaN x or y = the agent is absent), speed [B_all], acc [B_all].  One launch,
        global_t = the steps fed so far, no host synchronisation."""
        self.engine.guide_metrics_step(self._setup, world, speed, acc, self.state, self.steps)
        self.steps += 1

    def add_plans(self, plans_all):
        """One plan [B_all,52,6] in upstream's order: the environment scores the state BEFORE each of its `n_step_action` actions
        (env_trajdata._step:411-424), so this scores the current pose with its carried speed and acceleration, then the executed states
        0 .. n_step_action - 2 (speed = plans[:, k, 2], acc = plans[:, k, 4]), and carries state n_step_action - 1 into the next call.
        The first scored state of an episode is therefore the initial pose, which ConstraintGuidance's `times + 1` and
        TargetSpeedGuidance's global_t assume.  `RolloutMetrics.add_plans` scores the states AFTER each action instead."""
        plans = torch.as_tensor(plans_all).to(self.engine.device, torch.float32).contiguous()
        if tuple(plans.shape) != (self.B_all, 52, 6):
            raise CldError(f"GuidanceMetrics: plans must cover all {self.B_all} agents as [{self.B_all},52,6], got {tuple(plans.shape)}")
        centroid, yaw = self.poses[:, :2].contiguous(), self.poses[:, 2].contiguous()
        self.add_step(self.poses, self.speed, self.acc)
        n = self.n_step_action
        for k in range(n):
            world = self.engine.world_step(plans, centroid, yaw, k)[0]
            speed, acc = plans[:, k, 2].contiguous(), plans[:, k, 4].contiguous()
            if k < n - 1:
                self.add_step(world, speed, acc)
        self.poses, self.speed, self.acc = world, speed, acc

    def get_episode_metrics(self):
        """-> {key: [num_scenes] float64 device tensor, NaN except at the entry's scene}, upstream's keys in upstream's order."""
        per_entry = self.engine.guide_metrics_read(self._setup, self.state)[0]
        out = torch.full((len(self.keys), self.num_scenes), float("nan"), dtype=torch.float64, device=self.engine.device)
        out[torch.arange(len(self.keys), device=self.engine.device), self._entry_scene] = per_entry
        return {k: out[n] for n, k in enumerate(self.keys)}

    def per_member(self, key: str):
        """-> [members of the entry] float64 device tensor: the member's episode value (include/cld.h `cld_guide_metrics_read`), in the
        order of the config's `agents`."""
        if key not in self._index:
            raise KeyError(f"GuidanceMetrics.per_member: no metric {key!r} (one of {self.keys})")
        e = self._index[key]
        return self.engine.guide_metrics_read(self._setup, self.state)[1][self._member_start[e]:self._member_start[e + 1]]


class SampleMetrics:
    """The open-loop sample metrics upstream validates its diffusion model with (DiffuserTrafficModel._compute_metrics,
    src/tbsim/algos/algos.py:1818-1852, through src/tbsim/utils/metrics.py:201-358) on the device: how close the N sampled futures of
    an agent come to the logged one (ADE, FDE: mean over the samples and best sample) and how far they lie apart (APD, FPD: mean and
    max over all pairs).  include/cld_eval.h defines every column; the per-agent arithmetic is fp64 in `cld_sample_metrics`.

    Two things are upstream's and are reproduced as they are: a mean over time divides by T, not by the number of available steps; and
    FPD (`batch_final_diversity`) takes the last COORDINATE, y, and the norm over time -- not the distance at the last time step its
    docstring describes.  That distance is kept beside it as `ego_avg_last_step_PD` / `ego_max_last_step_PD`, keys of this library.
    Confidences are uniform (1 / N), as upstream passes them; nothing else is built.

    `add` appends the batch's per-agent rows to a grow-by-doubling device buffer (`capacity` rows before it first grows); the fill
    count follows from the shapes and lives on the host, so `add` issues no synchronisation.  Upstream's `_compute_metrics` covers one
    batch: that is `last_batch()`; `compute()` covers every agent added since `reset()`."""

    KEYS = _lib.SAMPLE_METRIC_COLS
    UPSTREAM_KEYS = _lib.SAMPLE_METRIC_COLS[:8]

    def __init__(self, engine, capacity: int = 0):
        self.engine = engine
        cap = max(int(capacity), 0)
        self._rows = torch.empty(cap, len(self.KEYS), dtype=torch.float64, device=engine.device)
        self._index = torch.empty(cap, 4, dtype=torch.int32, device=engine.device)
        self._fill = 0
        self._last = None

    def reset(self):
        """Forget the rows (the buffers' memory is kept)."""
        self._fill = 0
        self._last = None

    def add(self, pred, gt, avail):
        """One batch: pred [B,N,T,2] (or [B,N,T,6], positions in channels 0 and 1), gt [B,T,2], avail [B,T] bool or float.  N and T may
        differ between batches.  The kernel writes straight into the buffers' tails."""
        B, fill = int(pred.shape[0]), self._fill
        if fill + B > self._rows.shape[0]:
            cap = max(2 * self._rows.shape[0], fill + B)
            for name in ("_rows", "_index"):
                old = getattr(self, name)
                grown = torch.empty(cap, old.shape[1], dtype=old.dtype, device=old.device)
                grown[:fill].copy_(old[:fill])
                setattr(self, name, grown)
        self._last = self.engine.sample_metrics(pred, gt, avail, out=(self._rows[fill:], self._index[fill:]))["means"]
        self._fill = fill + B

    def per_agent(self):
        """-> [M,10] float64: the rows of every agent added since `reset()`, in the order added (a view; columns = `KEYS`)."""
        return self._rows[:self._fill]

    def index(self):
        """-> [M,4] int32 (a view): per agent the best sample by ADE, the best by FDE (the first among equals), the last available
        step (0 when none is) and the non-finite flag."""
        return self._index[:self._fill]

    def _refuse_nonfinite(self, what: str):
        bad = torch.nonzero(self.index()[:, 3]).reshape(-1)
        if bad.numel():
            raise ValueError(f"SampleMetrics.{what}: non-finite input at {bad.numel()} of {self._fill} agents (first: row {int(bad[0])}); "
                             f"upstream asserts finiteness")

    def compute(self):
        """-> {key: 0-d float64 device tensor}: upstream's eight keys and the two last-step ones, each the mean of its column over every
        agent added since `reset()` (an fp64 sum of the device rows).  ValueError when nothing was added or an agent's non-finite flag
        is set (this reads the flags back: the one synchronisation)."""
        if self._fill == 0:
            raise ValueError("SampleMetrics.compute: nothing was added")
        self._refuse_nonfinite("compute")
        means = self.per_agent().sum(dim=0) / float(self._fill)
        return {k: means[c] for c, k in enumerate(self.KEYS)}

    def last_batch(self):
        """-> upstream's eight keys for the last batch added alone (0-d float64 device tensors): what `_compute_metrics` returns.  The
        batch means come from the library's fixed-order fold.  No synchronisation, no finiteness check."""
        if self._last is None:
            raise ValueError("SampleMetrics.last_batch: nothing was added")
        return {k: self._last[c] for c, k in enumerate(self.UPSTREAM_KEYS)}


def compute_sample_metrics(engine, pred_batch, data_batch):
    """`DiffuserTrafficModel._compute_metrics(pred_batch, data_batch)` on the device: pred_batch["predictions"]["positions"] [B,N,T,2],
    data_batch["target_positions"] [B,T,2], data_batch["target_availabilities"] [B,T] -> upstream's eight keys as 0-d float64 device
    tensors.  ValueError on non-finite input, where upstream's `_assert_shapes` asserts."""
    m = SampleMetrics(engine, capacity=int(pred_batch["predictions"]["positions"].shape[0]))
    m.add(pred_batch["predictions"]["positions"], data_batch["target_positions"], data_batch["target_availabilities"])
    m._refuse_nonfinite("compute_sample_metrics")
    return m.last_batch()
