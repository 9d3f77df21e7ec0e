"""The episode metrics of a closed-loop rollout on the device: `RolloutMetrics` scores every environment step where the poses are, in
HBM, and answers with upstream's registry names and keys (src/tbsim/evaluation/env_builders.py:37-50: OffRoadRate, DiskOffRoadRate,
CollisionRate, DiskCollisionRate, CriticalFailure, Comfort of src/tbsim/envs/env_metrics.py).

The arithmetic is `cld_scene_metrics_step` / `cld_scene_metrics_read` (csrc/metrics_kernels.hip; include/cld.h defines every
quantity).  The bookkeeping here is the state buffer, the step counter and the poses, which move with `cld_world_step` exactly as
`SceneObserver.advance` moves its own, so the scored poses are the observer's history frames bit for bit.

`RealismDeviation` is the test stage's other number (src/trainers/guide_dm_trainer.py:204-295): the mean Wasserstein-1 distance between
ground truth and prediction of three quantities, accumulated and evaluated on the device (`cld_realism_terms`, `cld_sort_f32`,
`cld_wasserstein_f32`; csrc/realism_kernels.hip).
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
        as `SceneObserver.advance` takes them, each scored as one environment step; the poses move to the last of them."""
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
