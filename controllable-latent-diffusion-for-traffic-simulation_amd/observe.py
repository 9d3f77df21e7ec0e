"""The observation stage of the closed loop on the device: `SceneObserver` keeps every agent's world-frame history and rebuilds, at
each sim step, the batch the ContextEncoder path of `CldPolicy.get_action` reads -- the stage upstream runs in
`parse_node_centric` -> `rasterize_agents` (src/tbsim/utils/trajdata_utils.py:123-156, 381-420) on trajdata's output.

The raster itself is `cld_rasterize` (csrc/raster_kernels.hip); the bookkeeping here is the history ring, a handful of [B,3,3] frames
and the slicing into chunks.  The poses move with `cld_world_step`, the arithmetic `closed_loop_rollout` moves its own with, so the
observer's poses and the rollout's are the same bits.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from ._lib import CldError
from .engine import RASTER_DEFAULTS, raster_frames      # (RASTER_DEFAULTS: config.yaml:81-86, :96)
from .policy import frames_from_pose, invert_frames, transform_points


class SceneObserver:
    """A four-argument `cond_fn(step, world, cs, plans)` for `closed_loop_rollout`.

    scene_start [num_scenes + 1]: agents scene_start[s] .. scene_start[s + 1] - 1 form scene s; hist_world [B_all,T,3] world
    (x, y, yaw), oldest first, frame T - 1 = now; hist_avail [B_all,T]; maps [num_maps,n_sem,map_h,map_w] with scene_map
    [num_scenes] (< 0: none) and map_from_world [num_maps,3,3], or None.  `row0`, `B`: the rows this rank plans for (default: all);
    the history covers every rank's agents and is fed from `plans` = what the rollout's `gather` returned, [B_all,52,6] (a
    single rank passes `gather=lambda traj: traj`).  `raster_cfg`: height, width, px_per_m, ego_center, no_map_fill,
    max_neighbor_dist, n_sem (RASTER_DEFAULTS).

    From step 1 on a call first appends the `n_step_action` executed states of every agent's previous plan, taken to the world
    frame, to the ring (the oldest frames drop out), then returns the observation: `image`, `history_positions` [B,T,2] /
    `history_yaws` [B,T,1] (agent frame) / `history_availabilities` [B,T], `curr_speed` [B], and `drivable_map` [B,H,W] uint8,
    `raster_from_agent`, `raster_from_world`, `world_from_agent`, `agent_from_world` [B,3,3], `agent_hist` [B,T,3] -- what the
    built-in collision and goal losses read except `extent`.  With `encode=True` the raster is built and context-encoded in passes
    of `chunk_agents` rows through one reused image buffer and the dict holds `cond_feat`, `curr_states` instead of `image`."""

    def __init__(self, engine, scene_start, hist_world, hist_avail, maps=None, scene_map=None, map_from_world=None,
                 n_step_action: int = 5, chunk_agents: int = 256, row0: int = 0, B: Optional[int] = None, encode: bool = False,
                 **raster_cfg):
        unknown = sorted(set(raster_cfg) - set(RASTER_DEFAULTS))
        if unknown:
            raise TypeError(f"SceneObserver: unknown raster settings {unknown} (one of {sorted(RASTER_DEFAULTS)})")
        self.engine = engine
        self.cfg = dict(RASTER_DEFAULTS, **raster_cfg)
        dev = engine.device
        self.hist_world = torch.as_tensor(hist_world).to(dev, torch.float32).contiguous().clone()
        if self.hist_world.dim() != 3 or self.hist_world.shape[2] != 3:
            raise CldError(f"SceneObserver: hist_world must be [B_all,T,3], got {tuple(self.hist_world.shape)}")
        self.B_all, self.T_hist = int(self.hist_world.shape[0]), int(self.hist_world.shape[1])
        self.hist_avail = (torch.as_tensor(hist_avail) != 0).to(dev, torch.uint8).contiguous()
        if tuple(self.hist_avail.shape) != (self.B_all, self.T_hist):
            raise CldError(f"SceneObserver: hist_avail must be [{self.B_all},{self.T_hist}], got {tuple(self.hist_avail.shape)}")
        ss = torch.as_tensor(scene_start).to(torch.int64).reshape(-1).cpu()
        if ss.numel() < 2 or int(ss[0]) != 0 or int(ss[-1]) != self.B_all or bool((ss[1:] <= ss[:-1]).any()):
            raise CldError(f"SceneObserver: scene_start {ss.tolist()} does not split the {self.B_all} agents into scenes")
        self.scene_start = ss.to(dev, torch.int32)
        self._scene_bounds = ss                                    # (host copy: map_source() finds the scenes of this rank's rows)
        self.n_step_action = int(n_step_action)
        if not 1 <= self.n_step_action <= min(52, self.T_hist):
            raise CldError(f"SceneObserver: n_step_action = {n_step_action} (1 .. {min(52, self.T_hist)})")
        self.chunk_agents = int(chunk_agents)
        if self.chunk_agents < 1:
            raise CldError("SceneObserver: chunk_agents must be positive")
        self.row0 = int(row0)
        self.B = self.B_all - self.row0 if B is None else int(B)
        if self.row0 < 0 or self.B < 1 or self.row0 + self.B > self.B_all:
            raise CldError(f"SceneObserver: rows [{self.row0}, {self.row0 + self.B}) are not within the {self.B_all} agents")
        self.encode = bool(encode)
        self.maps = None if maps is None else torch.as_tensor(maps).to(dev, torch.float32).contiguous()
        self.scene_map = None if scene_map is None else torch.as_tensor(scene_map).to(dev, torch.int32).contiguous()
        self.map_from_world = None if map_from_world is None else torch.as_tensor(map_from_world).to(dev, torch.float32).contiguous()
        self.poses = self.hist_world[:, -1].clone()                # [B_all,3] world (x, y, h) now
        self.raster_from_agent = raster_frames(self.cfg, 1)[0].to(dev)
        self._buf = None                                           # the reused image buffer of encode=True

    # ------------------------------------------------------------------ history
    def advance(self, plans):
        """Append the `n_step_action` executed states of every agent's plan [B_all,52,6] (agent frame at planning time) to the ring,
        in the world frame, and move the poses to the last of them."""
        plans = torch.as_tensor(plans).to(self.engine.device, torch.float32).contiguous()
        if tuple(plans.shape) != (self.B_all, 52, 6):
            raise CldError(f"SceneObserver: plans must cover all {self.B_all} agents as [{self.B_all},52,6], got {tuple(plans.shape)}")
        n = self.n_step_action
        centroid, yaw = self.poses[:, :2].contiguous(), self.poses[:, 2].contiguous()
        new = torch.stack([self.engine.world_step(plans, centroid, yaw, k)[0] for k in range(n)], dim=1)      # [B_all,n,3]
        self.hist_world = torch.cat([self.hist_world[:, n:], new], dim=1).contiguous()
        self.hist_avail = torch.cat([self.hist_avail[:, n:], torch.ones(self.B_all, n, dtype=torch.uint8, device=new.device)], dim=1).contiguous()
        self.poses = new[:, -1].clone()

    def frames(self):
        """-> dict of the agent-frame quantities of this rank's rows from the current history (no raster)."""
        rows = slice(self.row0, self.row0 + self.B)
        pose = self.poses[rows]
        W = frames_from_pose(pose)
        M = invert_frames(W)
        av = self.hist_avail[rows] != 0
        pos = transform_points(self.hist_world[rows, :, :2], M) * av[..., None]
        dyaw = self.hist_world[rows, :, 2] - pose[:, 2:3]
        dyaw = (torch.remainder(dyaw + math.pi, 2.0 * math.pi) - math.pi) * av
        rfa = self.raster_from_agent.expand(self.B, 3, 3).contiguous()
        return {"history_positions": pos, "history_yaws": dyaw[..., None], "history_availabilities": av,
                "raster_from_agent": rfa, "world_from_agent": W, "agent_from_world": M,
                "agent_hist": torch.cat([pos, dyaw[..., None]], dim=-1)}

    def map_source(self):
        """The `map_source` of a map_collision term for this rank's rows (Engine._map_collision; `set_guidance(..., map_source=)`): the
        observer's own maps and raster settings and the poses the agents stand at now.  A policy that follows the observation takes
        the pose of every later step from the rollout.  `scene_map` holds the scenes this rank's rows lie in, in order -- the scenes a
        term configured with these rows' scene_index has (a scene cut by the rank's boundary is one of them) -- not every rank's."""
        first = int(torch.searchsorted(self._scene_bounds, self.row0, right=True)) - 1
        last = int(torch.searchsorted(self._scene_bounds, self.row0 + self.B - 1, right=True)) - 1
        scene_map = None if self.scene_map is None else self.scene_map[first:last + 1].contiguous()
        return dict(self.cfg, maps=self.maps, scene_map=scene_map, map_from_world=self.map_from_world,
                    world=self.poses[self.row0:self.row0 + self.B].clone(), drivable_layer=0)

    def _rasterize(self, row0, B, out=None):
        return self.engine.rasterize(self.hist_world, self.hist_avail, self.scene_start, self.maps, self.scene_map, self.map_from_world,
                                     row0=row0, B=B, out=out, **self.cfg)

    # ------------------------------------------------------------------ cond_fn
    def observe(self, curr_states):
        """The observation of this rank's rows from the current history; curr_states [B,4] = (0, 0, v, 0) as the rollout carries it."""
        cs = torch.as_tensor(curr_states).to(self.engine.device, torch.float32)
        if tuple(cs.shape) != (self.B, 4):
            raise CldError(f"SceneObserver: curr_states must be [{self.B},4], got {tuple(cs.shape)}")
        obs = self.frames()
        obs["curr_speed"] = cs[:, 2].contiguous()
        if not self.encode:
            obs["image"], obs["drivable_map"], obs["raster_from_world"] = self._rasterize(self.row0, self.B)
            return obs
        n_max = min(self.chunk_agents, self.B)
        shape = (n_max, self.T_hist + self.cfg["n_sem"], self.cfg["height"], self.cfg["width"])
        if self._buf is None or tuple(self._buf.shape) != shape:
            self._buf = torch.empty(shape, dtype=torch.float32, device=self.engine.device)
        cond, drv, rfw = [], [], []
        for a in range(0, self.B, n_max):
            n = min(n_max, self.B - a)
            image, d, r = self._rasterize(self.row0 + a, n, out=self._buf)
            cond.append(self.engine.context_encode(image, cs[a:a + n]))       # (stream order: the buffer is rewritten behind it)
            drv.append(d)
            rfw.append(r)
        obs["cond_feat"], obs["drivable_map"], obs["raster_from_world"] = torch.cat(cond), torch.cat(drv), torch.cat(rfw)
        obs["curr_states"] = cs
        return obs

    def __call__(self, step, world, cs, plans):
        if step > 0:
            if plans is None:
                raise CldError("SceneObserver needs every agent's executed plan: run closed_loop_rollout with gather= "
                               "(parallel.gather_trajectories, or `lambda traj: traj` on a single rank)")
            self.advance(plans)
        return self.observe(cs)
