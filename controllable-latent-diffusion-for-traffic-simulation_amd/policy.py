"""The policy surface the reference's rollout loop expects but CLD never implemented
(`rollout.py:95-100` calls `policy.get_action(obs)`; `DMLightningModule` has none -- SURVEY section 0).
The contract is upstream's `DiffuserTrafficModel.get_action` (`src/tbsim/algos/algos.py:2024-2099`):
returns `(Action(positions [B,T,2], yaws [B,T,1]), {"action_samples": {...}})`; the executed sample is sample 0, or -- with
guidance active -- the one `choose_action_from_guidance` picks from the per-sample guidance losses (`guide_as_filter_only`,
`guide_with_gt` honoured); stationary agents are zeroed; `Action` is `src/tbsim/policies/common.py:10-66`.

`obs_dict` is either the reference's observation batch (`image` [B,34,224,224], `history_positions`, `history_yaws`,
`curr_speed`: the `ContextEncoder` of `context_utils.py` turns it into `cond_feat` / `curr_states` on the device), or
already carries `cond_feat` [B,256] and `curr_states` [B,4]; a different `context_encoder` callable may be passed in.
Parity: CLD itself never implemented `get_action`; the sample selection by guidance loss is pinned by a golden recorded from the
reference's own `choose_action_from_guidance` (`tests/golden/select.npz`).  `choose_action_from_gt` is a restatement of the
evident intent and PARITY UNPINNED: the reference function reads an undefined name `T` and raises `NameError` as written
(`guidance_loss.py:67-99`), so nothing could be recorded from it.  The composition and the world update are tested against
`oracle/cld_oracle.py` (`get_action`, `world_step`: `env_trajdata.py:452-468`).
"""
from __future__ import annotations

from typing import Callable, Mapping, Optional

import numpy as np
import torch

from . import _lib
from ._lib import CldError
from .dm_model import DmModel, repeat_guidance
from .engine import parse_sampler, raster_frames      # noqa: F401  (raster_frames re-exported: the frames a map_source implies)
from .vae_model import VaeModel


class Action:
    """Container for sequences of 2-D positions and yaws (policies/common.py:10-66)."""

    def __init__(self, positions, yaws):
        assert positions.shape[:-1] == yaws.shape[:-1] and positions.shape[-1] == 2 and yaws.shape[-1] == 1
        self.positions, self.yaws = positions, yaws

    @property
    def trajectories(self):
        cat = np.concatenate if isinstance(self.positions, np.ndarray) else torch.cat
        return cat([self.positions, self.yaws], -1)

    def to_dict(self):
        return dict(positions=self.positions, yaws=self.yaws)

    @classmethod
    def from_dict(cls, d):
        return cls(**d)

    def to_numpy(self):
        f = lambda x: x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()
        return Action(f(self.positions), f(self.yaws))


SCENE_LEVEL_LOSSES = ("agent_collision", "social_group", "gptcollision", "gptkeepdistance", "gptlanefollowing", "gptchangetoleftlane", "gptfollowlane")
GOAL_KINDS = {"global_target_pos": 1, "global_target_pos_at_time": 2}       # cld_goal.kind (include/cld.h); per-agent selection: not scene-level
LOSS_COLUMN = {"target_speed": 0, "speed_limit": 1, "acc_limit": 2, "target_pos_at_time": 3, "target_pos": 3}   # cld_guidance_losses


def choose_action_from_guidance(guide_losses: Mapping, guide_config_names, per_scene: bool = False, scene_of_agent=None):
    """`choose_action_from_guidance` (src/tbsim/utils/guidance_loss.py:22-66), agent-centric layout: `guide_losses` maps
    '<name>_scene_%03d_%02d' -> [B,N] (NaN outside the loss's agents) in dict order, `guide_config_names` lists the loss names of
    every scene.  Per scene the losses are nansum-med and every agent takes the sample with the smallest sum.  As written
    upstream the result of EVERY scene overwrites the indices of the whole batch (the scene mask is commented out, :49-50,62-63),
    so the LAST scene's choice wins and agents outside it get sample 0; that is the default here too (parity with upstream).
    `per_scene=True` with `scene_of_agent` [B] applies each scene's choice to its own agents only -- the evident intent."""
    accum = torch.stack([v for v in guide_losses.values()], dim=2)
    B, N = accum.shape[:2]
    act_idx = torch.zeros(B, dtype=torch.long, device=accum.device)
    scount = 0
    for si, names in enumerate(guide_config_names):
        ends = scount + len(names)
        scene_loss = torch.nansum(accum[..., scount:ends], dim=-1)
        scount = ends
        if any(nm in SCENE_LEVEL_LOSSES for nm in names):
            idx = torch.argmin(scene_loss.sum(dim=0)).expand(B)
        else:
            idx = torch.argmin(scene_loss, dim=-1)
        if per_scene:
            mask = torch.as_tensor(scene_of_agent).to(accum.device) == si
            act_idx = torch.where(mask, idx, act_idx)
        else:
            act_idx = idx
    return act_idx


def choose_action_from_gt(positions, target_positions, target_availabilities):
    """`choose_action_from_gt` (guidance_loss.py:67-99): per agent the sample with the smallest average displacement from the
    ground-truth future over its valid steps; agents with a sample whose steps are all invalid keep sample 0."""
    B, N, T_ = positions.shape[:3]
    endT = min(T_, target_positions.shape[1])
    gt = torch.as_tensor(target_positions).to(positions.device, positions.dtype)[:, :endT].unsqueeze(1)
    valid = torch.as_tensor(target_availabilities).to(positions.device)[:, :endT].unsqueeze(1).expand(B, N, endT).bool()
    err = torch.norm(positions[:, :, :endT] - gt, dim=-1)
    err = torch.where(valid, err, torch.full_like(err, float("nan")))
    ade = torch.nanmean(err, dim=-1)
    ok = torch.isnan(ade).sum(dim=-1) == 0
    act_idx = torch.zeros(B, dtype=torch.long, device=positions.device)
    if bool(ok.any()):
        act_idx[ok] = torch.argmin(ade, dim=-1)[ok]
    return act_idx


def invert_frames(m):
    """Inverse of 2-D affine frames [...,3,3] (last row 0 0 1) in closed form: world_from_agent <-> agent_from_world."""
    a, b, tx, c, d, ty = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2], m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    out = torch.zeros_like(m)
    out[..., 0, 0], out[..., 0, 1], out[..., 0, 2] = ia, ib, -(ia * tx + ib * ty)
    out[..., 1, 0], out[..., 1, 1], out[..., 1, 2] = ic, id_, -(ic * tx + id_ * ty)
    out[..., 2, 2] = 1.0
    return out


def frames_from_pose(world):
    """world [B,3] = (x, y, heading) -> world_from_agent [B,3,3]."""
    c, s = torch.cos(world[:, 2]), torch.sin(world[:, 2])
    W = torch.zeros(world.shape[0], 3, 3, dtype=world.dtype, device=world.device)
    W[:, 0, 0], W[:, 0, 1], W[:, 0, 2] = c, -s, world[:, 0]
    W[:, 1, 0], W[:, 1, 1], W[:, 1, 2] = s, c, world[:, 1]
    W[:, 2, 2] = 1.0
    return W


def transform_points(pts, m):
    """pts [B,K,2] through the frames m [B,3,3] (GeoUtils.transform_points_tensor)."""
    return pts @ m[:, :2, :2].transpose(1, 2) + m[:, None, :2, 2]


def update_goal_reached(reached, goal: Mapping, world_from_agent, agent_hist, by: str = "any"):
    """have_reached_mask of the goal losses after one more observation (guidance_loss.py:1019-1029, :1122-1133) -> new mask [B]
    (a set flag stays set).  Per config with a tolerance: the last `action_num` history positions go to the world frame and an agent
    is flagged when one lies within the tolerance of its target.  by="any" reproduces the reference as written: only the FIRST of
    those points is kept after the transform, and its [M,2] - [M,1,2] broadcast takes the minimum over the points of ALL the config's
    agents, so agent i is flagged when any of them is near i's target.  by="own": the agent's own `action_num` points."""
    if by not in ("any", "own"):
        raise ValueError(f"goal_reached_by={by!r} (any | own)")
    reached = reached.clone()
    world_from_agent = world_from_agent.to(agent_hist.device)
    for idx, tol, action_num in goal["configs"]:
        if tol is None:
            continue
        idx_d = idx.to(agent_hist.device)
        hw = transform_points(agent_hist[idx_d][:, -int(action_num):, :2].float(), world_from_agent[idx_d].float())      # [M,K,2]
        tgt = goal["target_pos"][idx].to(hw.device, hw.dtype)
        if by == "any":
            dist = (hw[:, 0][None, :, :] - tgt[:, None, :]).norm(dim=-1).min(dim=-1)[0]
        else:
            dist = (hw - tgt[:, None, :]).norm(dim=-1).min(dim=-1)[0]
        reached[idx] |= (dist < float(tol)).cpu()
    return reached


def refresh_collision_terms(g: Optional[Mapping], obs: Mapping, world=None):
    """The guidance dict `g` with the observation-dependent fields of its collision terms taken from `obs`, each only where `obs` holds
    it -- what upstream's losses read from data_batch at every call (guidance_loss.py:506-510, :773-775):
      agent_collision: world_from_agent, curr_speed
      map_collision:   raster_from_agent, curr_speed, and drivable_map (raster mode) or map_source['world'] (map mode: `world` [B,3],
                       default obs['world'], the pose the agents' frames stand at)
    extent, weights, parameters and the scene structure stay as configured.  Nothing is modified in place; a dict without collision
    terms comes back as it is."""
    if g is None or (g.get("agent_collision") is None and g.get("map_collision") is None):
        return g
    out = dict(g)
    speed = obs.get("curr_speed")
    if g.get("agent_collision") is not None:
        col = dict(g["agent_collision"])
        if obs.get("world_from_agent") is not None:
            col["world_from_agent"] = obs["world_from_agent"]
        if speed is not None:
            col["curr_speed"] = speed
        out["agent_collision"] = col
    if g.get("map_collision") is not None:
        mcol = dict(g["map_collision"])
        if obs.get("raster_from_agent") is not None:
            mcol["raster_from_agent"] = obs["raster_from_agent"]
        if speed is not None:
            mcol["curr_speed"] = speed
        if mcol.get("map_source") is not None:
            pose = world if world is not None else obs.get("world")
            if pose is not None:
                mcol["map_source"] = dict(mcol["map_source"], world=pose)
        elif obs.get("drivable_map") is not None:
            mcol["drivable_map"] = obs["drivable_map"]
        out["map_collision"] = mcol
    return out


def refresh_pair_term(g: Optional[Mapping], obs: Mapping):
    """The guidance dict `g` with the frames of its pair term taken from `obs` where it holds them (upstream's losses read
    data_batch['world_from_agent'] and ['agent_from_world'] at every call, trajdata_utils.py:550-562): agent_from_world from `obs`,
    or, when `obs` has only world_from_agent, none -- the library then takes the inverse rotation; nothing is modified in place."""
    if g is None or g.get("pair") is None or obs.get("world_from_agent") is None:
        return g
    return dict(g, pair=dict(g["pair"], world_from_agent=obs["world_from_agent"], agent_from_world=obs.get("agent_from_world")))


def refresh_lane_term(g: Optional[Mapping], obs: Mapping):
    """The guidance dict `g` with its lane term brought to this observation (upstream's get_lane_projection reads the frames and the
    map at every call, trajdata_utils.py:590-643): agent_from_world from `obs` (or the inverse of its world_from_agent), so that the
    polylines are taken into the agents' frames of NOW when the term is next prepared, and new world polylines from
    obs['lane_points'] / ['left_lane_points'] where it carries them (the lane under an agent changes as it drives); nothing is
    modified in place."""
    if g is None or g.get("lane") is None or g["lane"].get("world_lines") is None:
        return g
    F = obs.get("agent_from_world")
    if F is None and obs.get("world_from_agent") is not None:
        F = invert_frames(torch.as_tensor(obs["world_from_agent"]).float())
    new = {} if F is None else {"agent_from_world": F}
    sources = g["lane"].get("sources")
    if sources is not None and all(obs.get(src) is not None for src, _ in sources):
        new["world_lines"] = gather_lane_lines(obs, sources)
    return dict(g, lane=dict(g["lane"], **new)) if new else g


def refresh_social_term(g: Optional[Mapping], obs: Mapping):
    """The guidance dict `g` with the frames of its social-group term taken from `obs` where it holds them (upstream's loss reads
    data_batch['world_from_agent'] at every call, guidance_loss.py:1156); nothing is modified in place."""
    if g is None or g.get("social_group") is None or obs.get("world_from_agent") is None:
        return g
    return dict(g, social_group=dict(g["social_group"], world_from_agent=obs["world_from_agent"]))


class CldPolicy:
    def __init__(self, dm: DmModel, vae: VaeModel, context_encoder: Optional[Callable] = None,
                 disable_control_on_stationary: bool = False, moving_speed_th: float = 0.5, select_per_scene: bool = False):
        self.dm, self.vae = dm, vae
        self.context_encoder = context_encoder
        self.disable_control_on_stationary = disable_control_on_stationary   # config.yaml:99
        self.moving_speed_th = moving_speed_th                               # config.yaml:101
        self.select_per_scene = select_per_scene      # False = upstream's sample selection as written (see choose_action_from_guidance)
        self._guidance = None
        self._guidance_cfg = None                     # (guidance_config_list, scene_index) behind self._guidance
        self._follow_observation = False              # set_guidance(follow_observation=True): the collision terms read every observation
        # closed-loop state of the goal losses (upstream keeps it on the loss objects): have_reached_mask [B], the rollout step of the
        # last get_action, and how the mask is updated ("any": the reference as written | "own", see update_goal_reached)
        self.goal_reached = None
        self.goal_global_t = None
        self.goal_reached_by = "any"
        self.social_iter = 0                          # evaluation index of the next plan's first loop iteration (social-group draws)
        self._reconstruction = None                   # enable_reconstruction_guidance: what guide_clean="video_diff" runs with

    def eval(self):
        return self

    def enable_reconstruction_guidance(self, descend: bool = False, lr: Optional[float] = None, perturb_th=None, weights: Optional[Mapping] = None):
        """Prepare `get_action(guide_clean="video_diff")`: upstream's reconstruction guidance (DiffuserModel.p_sample,
        diffuser.py:844-929, with perturb_video_diffusion, guidance_loss.py:2284-2330) -- the mode both shipped checkpoints configure.
        The mode differentiates the guidance loss through the DENOISER, so it holds a second copy of the U-Net weights on the
        device, in the training layout (17 MB), and per plan a tape of `cld_unet_tape_bytes(h, 1)` per row (twice that with
        classifier-free guidance); a policy does not allocate those unasked, hence this call.  `weights`: the U-Net state_dict the
        DmModel was loaded with (None: the tensors it was given, which must be unchanged).
        descend=False reproduces upstream AS WRITTEN: x0_hat + lr * grad (guidance_loss.py:2319-2324), which with upstream's positive
        loss totals ASCENDS the loss; descend=True is the evident intent.  lr None = sigma_t; perturb_th None = clip to sigma_t, a
        number > 0 = upstream's schedule towards it (diffuser.py:888-891), "none" = no clip.  The optimiser settings of
        `set_guidance` (lr / optimizer / perturb_th) are not read in this mode (scene_edit_config.py:74)."""
        self._reconstruction = dict(params=self.dm.engine.unet_flat_params(weights), lr=lr, perturb_th=perturb_th, descend=bool(descend))
        return self

    def set_guidance(self, guidance_config_list, scene_index, **opt):
        """Upstream `set_guidance` (algos.py; guidance_loss.py:2106-2175): keep a guidance configuration for the following
        `get_action` calls.  `opt`: lr / optimizer / perturb_th of the optimiser step (scene_edit_config.py:74-90), `output`
        (True | dict: guidance on the t = 0 output, upstream apply_guidance_output + final_step_opt_params), `intermediate`.
        `follow_observation=True`: the collision terms take their frames, speeds and drivable map (or pose) from the observation of
        every get_action, as upstream's losses read data_batch at every call (refresh_collision_terms); False (the default): they keep
        what `data_batch` held here -- frozen frames.  `map_source` (dict: maps, scene_map, map_from_world, world, raster settings;
        SceneObserver.map_source()): map_collision reads the scene maps instead of a per-agent drivable raster, and `data_batch` needs
        only extent (and curr_speed) for it.  `social_group` configs (guidance_loss.py:1137-1207) are taken out first
        (social_groups_from_config; `data_batch` needs world_from_agent) and kept as guidance['social_group']; with
        follow_observation their frames follow every observation too.  `social_seed` seeds their draws (default 0); every
        get_action moves their evaluation index on, so successive plans do not reuse draws.  The pair-relation configs
        (`gptcollision`, `gptkeepdistance`, ...; pair_terms_from_config) are taken out before them and kept as guidance['pair'];
        they read world_from_agent (and agent_from_world, when there) of `data_batch` and follow the observation likewise.  The lane
        configs (`gptlanefollowing`, `gptchangetoleftlane`, `gptfollowlane`; lane_terms_from_config) are taken out after the pair
        configs and kept as guidance['lane']; they read `lane_points` / `left_lane_points` and the frames of `data_batch`, and with
        follow_observation the polylines are taken into the frames (and from the lanes) of every observation (refresh_lane_term)."""
        data_batch = opt.pop("data_batch", None)         # observation fields scene-coupled losses read (agent_collision: extent, world_from_agent, curr_speed)
        follow = bool(opt.pop("follow_observation", False))
        map_source = opt.pop("map_source", None)
        by = opt.pop("goal_reached_by", "any")
        if by not in ("any", "own"):
            raise ValueError(f"goal_reached_by={by!r} (any | own)")
        social_seed = int(opt.pop("social_seed", 0))
        rest, pair = pair_terms_from_config(guidance_config_list, scene_index, data_batch)
        rest, lane = lane_terms_from_config(rest, scene_index, data_batch)
        rest, social = social_groups_from_config(rest, scene_index, data_batch)
        peeled = social is not None or pair is not None or lane is not None
        base = guidance_from_config(rest, scene_index, data_batch=data_batch, map_source=map_source) if not peeled or any(len(c) for c in rest) else {}
        if pair is not None:
            base["pair"] = pair
        if lane is not None:
            base["lane"] = lane
        if social is not None:
            base["social_group"] = dict(social, seed=social_seed)
        self._guidance = dict(base, **opt)
        self.social_iter = 0
        self._follow_observation = follow
        self._guidance_cfg = (guidance_config_list, torch.as_tensor(scene_index).reshape(-1).cpu())
        # a new configuration starts with nobody arrived (upstream builds new loss objects: have_reached_mask = None)
        self.goal_reached_by = by
        self.goal_global_t = None
        self.goal_reached = torch.zeros(self._guidance_cfg[1].numel(), dtype=torch.bool) if self._guidance.get("goal") is not None else None

    def clear_guidance(self):
        self._guidance = None
        self._guidance_cfg = None
        self._follow_observation = False
        self.goal_reached = None
        self.goal_global_t = None

    def _goal_for_step(self, goal: Mapping, obs_dict: Mapping, step_index: int, carry: bool):
        """The `goal` entry of a guidance dict completed for one get_action: global_t = step_index (upstream
        update_guidance(global_t=kwargs['step_index']), algos.py:2048), the frames of this observation, and -- `carry`: the goal was
        configured by set_guidance -- the reached mask, updated from obs_dict['agent_hist'] before sampling and kept for the next call."""
        W, M = obs_dict.get("world_from_agent"), obs_dict.get("agent_from_world")
        if goal.get("agent_from_world") is not None and not carry:
            M = goal["agent_from_world"]
        if W is None and M is None:
            raise ValueError("a goal loss needs obs_dict['agent_from_world'] or obs_dict['world_from_agent']")
        W = None if W is None else torch.as_tensor(W).float()
        M = invert_frames(W) if M is None else torch.as_tensor(M).float()
        out = dict(goal, agent_from_world=M, global_t=int(step_index))
        if carry:
            if any(tol is not None for _, tol, _ in goal["configs"]):
                if obs_dict.get("agent_hist") is None:
                    raise ValueError("a goal loss with a target_tolerance needs obs_dict['agent_hist']")
                self.goal_reached = update_goal_reached(self.goal_reached, goal, invert_frames(M) if W is None else W,
                                                        torch.as_tensor(obs_dict["agent_hist"]), self.goal_reached_by)
            self.goal_global_t = int(step_index)
            out["reached"] = self.goal_reached.clone()
        return out

    def _guide_losses(self, traj, g, B: int, N: int, from_cfg: bool):
        """-> (guide_losses dict name -> [B,N] as upstream keys them, per-scene loss names) from the library's per-agent values;
        `g`: the guidance dict with its per-agent tensors repeated num_samp times."""
        has_builtin = any(g.get(k) is not None for k in ("target_speed", "speed_limit", "acc_limit", "target_pos"))
        vals = (self.vae.engine.guidance_losses(traj.reshape(B * N, 52, 6), g).reshape(B, N, 4) if has_builtin
                else torch.full((B, N, 4), float("nan"), device=traj.device))
        nan = torch.full((B, N), float("nan"), device=vals.device)
        colv = mapv = goalv = socv = pairv = lanev = None
        if g.get("lane") is not None:                # per (entry, sample), unweighted
            lanev = self.vae.engine.lane_loss(traj.reshape(B * N, 52, 6), dict(g["lane"], num_samp=N), want_grad=False)
        if g.get("pair") is not None:                # per (pair, sample) as upstream's classes return them (unweighted)
            pairv = self.vae.engine.pair_loss(traj.reshape(B * N, 52, 6), dict(g["pair"], num_samp=N), want_grad=False)
        if g.get("social_group") is not None:        # unweighted per-row values (guidance_loss.py:1205); 0 outside the groups here, NaN below
            socv = self.vae.engine.social_group_loss(traj.reshape(B * N, 52, 6), dict(g["social_group"], num_samp=N), want_grad=False).reshape(B, N)
        if g.get("goal") is not None:                # unweighted per-row values, 0 for agents that have arrived (guidance_loss.py:1029,1133)
            goalv = self.vae.engine.goal_loss(traj.reshape(B * N, 52, 6), dict(g["goal"], num_samp=N), want_grad=False).reshape(B, N)
        if g.get("agent_collision") is not None:     # per-agent values as upstream files them (unweighted; :2166-2168)
            colv = self.vae.engine.agent_collision(traj.reshape(B * N, 52, 6), dict(g["agent_collision"], num_samp=N), want_grad=False).reshape(B, N)
        if g.get("map_collision") is not None:
            mapv = self.vae.engine.map_collision(traj.reshape(B * N, 52, 6), dict(g["map_collision"], num_samp=N), want_grad=False).reshape(B, N)
        out, names = {}, []
        if from_cfg:
            cfg_list, scene_index = self._guidance_cfg
            _, local = torch.unique_consecutive(scene_index, return_inverse=True)
            for si, cfgs in enumerate(cfg_list):
                members = torch.nonzero(local == si).reshape(-1)
                names.append([c["name"] for c in cfgs])
                for gi, c in enumerate(cfgs):
                    idx = members if c.get("agents") is None else members[torch.as_tensor(c["agents"], dtype=torch.long)]
                    mask = torch.zeros(B, dtype=torch.bool)
                    mask[idx] = True
                    mask = mask.to(vals.device)
                    if c["name"] in PAIR_NAMES:      # the [N] value under EVERY agent of the scene (indiv_loss[agt_mask] = cur_loss, :2171)
                        pv = pairv[g["pair"]["configs"].index((si, gi))]
                        out["%s_scene_%03d_%02d" % (c["name"], si, gi)] = torch.where(mask[:, None], pv[None, :].expand(B, N), nan)
                        continue
                    if c["name"] in LANE_NAMES:      # likewise; LaneFollowingLoss: the mean over its targets (:1626)
                        rows = [e for e, sg in enumerate(g["lane"]["configs"]) if sg == (si, gi)]
                        lv = lanev[rows].mean(dim=0)
                        out["%s_scene_%03d_%02d" % (c["name"], si, gi)] = torch.where(mask[:, None], lv[None, :].expand(B, N), nan)
                        continue
                    v = (colv if c["name"] == "agent_collision" else mapv if c["name"] == "map_collision" else
                         goalv if c["name"] in GOAL_KINDS else socv if c["name"] == "social_group" else vals[..., LOSS_COLUMN[c["name"]]])
                    out["%s_scene_%03d_%02d" % (c["name"], si, gi)] = torch.where(mask[:, None], v, nan)
        else:       # a plain `guidance=` dict: one scene, one entry per active term
            names.append([])
            for nm, col in (("target_speed", 0), ("speed_limit", 1), ("acc_limit", 2), ("target_pos", 3)):
                if bool((~torch.isnan(vals[..., col])).any()):
                    out["%s_scene_000_%02d" % (nm, len(names[0]))] = vals[..., col]
                    names[0].append(nm)
            if colv is not None:
                out["agent_collision_scene_000_%02d" % len(names[0])] = colv
                names[0].append("agent_collision")
            if mapv is not None:
                out["map_collision_scene_000_%02d" % len(names[0])] = mapv
                names[0].append("map_collision")
            if goalv is not None:
                kind = torch.as_tensor(g["goal"]["kind"]).to(goalv.device)
                for nm, k in GOAL_KINDS.items():
                    if bool((kind == k).any()):
                        out["%s_scene_000_%02d" % (nm, len(names[0]))] = torch.where((kind == k)[:, None], goalv, nan)
                        names[0].append(nm)
            if socv is not None:
                inside = torch.zeros(B, dtype=torch.bool)
                for grp in g["social_group"]["groups"]:
                    inside[torch.as_tensor(grp, dtype=torch.long)] = True
                out["social_group_scene_000_%02d" % len(names[0])] = torch.where(inside.to(socv.device)[:, None], socv, nan)
                names[0].append("social_group")
            if pairv is not None:                     # one scene: every pair's value under every agent, keyed by the relation's config name
                number = {v: k for k, v in _lib.PAIR_KINDS.items()}
                config_name = {spec[0]: nm for nm, spec in PAIR_NAMES.items()}
                kd = g["pair"]["kind"]
                kd = [kd] * pairv.shape[0] if isinstance(kd, (str, int)) else list(kd)
                for p in range(pairv.shape[0]):
                    nm = config_name[kd[p] if isinstance(kd[p], str) else number[int(kd[p])]]
                    out["%s_scene_000_%02d" % (nm, len(names[0]))] = pairv[p][None, :].expand(B, N).clone()
                    names[0].append(nm)
            if lanev is not None:                     # one scene: every entry's value under every agent, keyed by the kind's config name
                number = {v: k for k, v in _lib.LANE_KINDS.items()}
                config_name = {spec[0]: nm for nm, spec in LANE_NAMES.items()}
                kd = g["lane"]["kind"]
                kd = [kd] * lanev.shape[0] if isinstance(kd, (str, int)) else list(kd)
                for e in range(lanev.shape[0]):
                    nm = config_name[kd[e] if isinstance(kd[e], str) else number[int(kd[e])]]
                    out["%s_scene_000_%02d" % (nm, len(names[0]))] = lanev[e][None, :].expand(B, N).clone()
                    names[0].append(nm)
        return out, names

    @torch.no_grad()
    def get_action(self, obs_dict: Mapping, num_action_samples: int = 1, class_free_guide_w: float = 0.0,
                   guide_as_filter_only: bool = False, guide_with_gt: bool = False, guide_clean=False,
                   step_index: int = 0, noise: Optional[Mapping] = None, guidance: Optional[Mapping] = None, plan=None,
                   sampler: Optional[Mapping] = None, **kwargs):
        """`DiffuserTrafficModel.get_action` (src/tbsim/algos/algos.py:2024-2099).  With guidance active (`set_guidance` or
        `guidance=`) the guidance losses of every sample are evaluated on the final output (diffuser.py:924-926), returned as
        info['guide_losses'], and the executed sample is the one `choose_action_from_guidance` picks (algos.py:2057-2064);
        `guide_as_filter_only`: sample without guidance and only filter (algos.py:1815); `guide_with_gt`: the sample closest to
        obs_dict['target_positions'] (algos.py:2055-2056); `guide_clean=True`: the guidance steps act on the model's clean
        prediction (diffuser.py:866-873); `guide_clean="video_diff"`: reconstruction guidance, after enable_reconstruction_guidance().  A
        collision config (`agent_collision`, guidance_loss.py:442-630) is filed under guide_losses and makes the sample choice
        scene-level, as upstream's SCENE_LEVEL_LOSSES do.  A goal config (`global_target_pos`, `global_target_pos_at_time`,
        guidance_loss.py:930-1135) reads obs_dict['agent_from_world'] and / or ['world_from_agent'] [B,3,3] (one is computed from the
        other; ValueError without both) and, with a target_tolerance, obs_dict['agent_hist'] [B,Th,>=2]; `step_index` is its global_t
        (algos.py:2048); the arrival flags persist on the policy (`goal_reached`) and come back as info['goal_reached'].
        `sampler`: a few-step sampler for the plan (DmModel.sample_traj; include/cld_solver.h) -- sample selection, the guidance losses on
        the output, goal carry and follow_observation work as on the ancestral path; together with `guide_clean` it raises.
        Not built: `plan` -- it raises instead of being ignored."""
        if sampler is not None and guide_clean:
            raise NotImplementedError(f"sampler= together with guide_clean={guide_clean!r} is not built: the few-step samplers guide the mean form only")
        loop_steps = self.vae.engine.loop_steps if sampler is None else len(parse_sampler(sampler, self.dm.n_timesteps)[1])
        video_diff = isinstance(guide_clean, str) and guide_clean == "video_diff"
        if video_diff and self._reconstruction is None:
            raise NotImplementedError("guide_clean='video_diff' needs CldPolicy.enable_reconstruction_guidance() first: the mode keeps a "
                                      "second copy of the U-Net weights and a tape per row, which a policy does not allocate unasked")
        if not video_diff and guide_clean not in (False, True, 0, 1, None):
            raise NotImplementedError(f"guide_clean={guide_clean!r}: the boolean form and \"video_diff\" are built (diffuser.py:866-873)")
        if plan is not None:
            raise NotImplementedError("plan conditioning is not part of the CLD sampler")
        if kwargs:
            raise TypeError(f"get_action: unexpected arguments {sorted(kwargs)}")
        eng = self.vae.engine
        if "cond_feat" in obs_dict:
            aux = dict(obs_dict)
        else:                                                       # obs -> aux_info (vae_model.py:84-88 pre_vae)
            enc = self.context_encoder or self.vae.context_encoder
            aux = dict(enc(obs_dict, include_class_free_cond=True) if class_free_guide_w != 0.0 and enc is self.vae.context_encoder
                       else enc(obs_dict))
        cond, cs = aux["cond_feat"], aux["curr_states"]
        if class_free_guide_w != 0.0 and aux.get("non_cond_feat") is None:
            aux["non_cond_feat"] = eng.non_cond_feat(cs)            # upstream builds it itself (diffuser.py:390-411,459-471); raises without the ContextEncoder weights
        B, N = cond.shape[0], int(num_action_samples)
        g = guidance if guidance is not None else self._guidance
        set_by_config = g is self._guidance
        if g is not None and video_diff:      # without guidance the mode is upstream's no-op: the plain chain
            g = dict(g, reconstruction=self._reconstruction)
        elif g is not None and guide_clean:
            g = dict(g, guide_clean=True)
        from_cfg = (g is self._guidance or (video_diff and set_by_config)) and self._guidance_cfg is not None
        if guidance is None and self._follow_observation:           # the collision terms of set_guidance follow this observation
            g = refresh_lane_term(refresh_pair_term(refresh_social_term(refresh_collision_terms(g, obs_dict), obs_dict), obs_dict), obs_dict)
        if g is not None and g.get("social_group") is not None and guidance is None:
            # the plan's loop iterations take evaluation indices social_iter .. social_iter + loop_steps - 1, the values reported on the
            # final output (below) the one behind them
            g = dict(g, social_group=dict(g["social_group"], iter_base=self.social_iter))
            self.social_iter += loop_steps + 1
        if g is not None and g.get("goal") is not None:
            carry = guidance is None
            g = dict(g, goal=self._goal_for_step(g["goal"], obs_dict, step_index, carry))
        out = self.dm({"history_positions": cond}, {k: aux[k] for k in ("cond_feat", "curr_states", "non_cond_feat") if k in aux},
                      {"num_samp": N}, noise=noise, class_free_guide_w=class_free_guide_w,
                      guidance=None if guide_as_filter_only else g, **({} if sampler is None else {"sampler": sampler}))
        a = out["aux_info"]
        traj = eng.decode(out["pred_traj"], a["cond_feat"], a["curr_states"], descaled_output=True).reshape(B, N, 52, 6)
        pos, yaw = traj[..., :2].clone(), traj[..., 3:4].clone()
        act_idx = torch.zeros(B, dtype=torch.long, device=pos.device)      # "arbitrarily use the first sample", algos.py:2053-2054
        info = {}
        if guide_with_gt and "target_positions" in obs_dict:
            act_idx = choose_action_from_gt(pos, obs_dict["target_positions"], obs_dict["target_availabilities"])
        elif g is not None:
            g_rep = repeat_guidance({k: v for k, v in g.items() if k != "curr_states"}, N, a["curr_states"])
            if g_rep.get("social_group") is not None:
                sg = g_rep["social_group"]
                g_rep["social_group"] = dict(sg, iter_base=int(sg.get("iter_base", 0)) + loop_steps)
            losses, names = self._guide_losses(traj, g_rep, B, N, from_cfg)
            scene_of_agent = None
            if self.select_per_scene and from_cfg:
                _, scene_of_agent = torch.unique_consecutive(self._guidance_cfg[1], return_inverse=True)
            if losses:
                act_idx = choose_action_from_guidance(losses, names, per_scene=scene_of_agent is not None, scene_of_agent=scene_of_agent)
            info["guide_losses"] = losses
        ar = torch.arange(B, device=pos.device)
        executed = traj[ar, act_idx].clone()
        if self.disable_control_on_stationary:                      # algos.py:2076-2083
            still = (cs[:, 2].abs() < self.moving_speed_th).to(pos.device)
            pos[still] = 0
            yaw[still] = 0
            executed[still] = executed[still] * torch.tensor([0.0, 0.0, 1.0, 0.0, 1.0, 1.0], device=pos.device)   # x, y, yaw of the executed plan
        if g is not None and g.get("goal") is not None:
            info["goal_global_t"] = g["goal"]["global_t"]
            if g["goal"].get("reached") is not None:
                info["goal_reached"] = torch.as_tensor(g["goal"]["reached"]).clone()
        info.update(action_samples=Action(pos, yaw).to_dict(), trajectories=traj, act_idx=act_idx, executed_trajectory=executed)
        return Action(pos[ar, act_idx], yaw[ar, act_idx]), info


def closed_loop_rollout(policy: CldPolicy, cond_fn: Callable, centroid, yaw, curr_states, n_sim_steps: int,
                        n_step_action: int = 5, gather: Optional[Callable] = None, timers=None, metrics=None, sampler: Optional[Mapping] = None,
                        **get_action_kwargs):
    """The loop of `rollout_episodes` (`src/tbsim/utils/env_utils.py:255-304`) kept on the device:
    obs -> get_action -> take `n_step_action` steps of the plan -> new world pose -> re-plan.
    `cond_fn(step, world [B,3], curr_states [B,4], plans) -> cond_feat [B,256]` stands in for the observation +
    ContextEncoder stage (it may return the raw observation batch instead: a dict with `image`, `history_*`,
    `curr_speed`, which get_action runs through the ContextEncoder); `plans` is what `gather` returned for the previous
    sim step -- every rank's executed plans [B_all,52,6], the neighbour information the next observation is built from
    (None on the first step or without `gather`); three-argument callables are accepted too.  `gather(traj)` (e.g.
    `parallel.gather_trajectories`) runs once per sim step; `timers` (`cld_amd.timer.Timers`) collects the per-phase
    times under the reference's keys "obs" / "network" / "env_step" / "step" (env_utils.py:268-298).
    The world moves on the EXECUTED trajectory (the selected sample, stationary agents held in place).
    `metrics` (`cld_amd.metrics.RolloutMetrics`): after the environment step of each sim step the `n_step_action` executed states of every
    agent are scored on the device (`metrics.add_plans` on what `gather` returned, or on this rank's trajectories without `gather`;
    that tensor must cover the B_all agents of `metrics`); without it the loop is exactly what it was.  A tuple or list of scorers
    (anything with `B_all` and `add_plans`, e.g. a `RolloutMetrics` and a `cld_amd.metrics.OccupancyMetrics`) is fed in its order.
    With a goal loss configured (`global_target_pos`, `global_target_pos_at_time`) the observation must tell get_action where the
    agents are and where they have been; the fields `cond_fn`'s observation lacks are filled in here: `world_from_agent` /
    `agent_from_world` [B,3,3] from the current world pose, and `agent_hist` [B,n_step_action,2]: the `n_step_action` executed states
    of the previous plan taken into the new agent frame (the last one is the agent's position now), on the first step the current
    position repeated.  `step_index` = the sim step is the goal losses' global_t.
    With collision guidance that follows the observation (`set_guidance(..., follow_observation=True)`) the same holds for
    `world_from_agent` (from the world pose; a social-group, pair or lane term reads it too), `curr_speed` (`curr_states[:, 2]`) and `world`
    [B,3], the pose itself, which a map_collision term in map mode is evaluated at; a raster-mode term needs `drivable_map` from `cond_fn` (SceneObserver gives it).
    `sampler`: a few-step sampler every re-plan runs with (get_action's `sampler=`); None: the ancestral sampler.
    Returns the world poses after each sim step [n_sim_steps, B, 3]."""
    import inspect
    if sampler is not None:
        get_action_kwargs = dict(get_action_kwargs, sampler=sampler)
    from contextlib import nullcontext
    tm = (lambda k: timers.timed(k)) if timers is not None else (lambda k: nullcontext())
    eng = policy.vae.engine
    world = torch.cat([torch.as_tensor(centroid), torch.as_tensor(yaw)[:, None]], dim=1).to(eng.device, torch.float32)
    cs = torch.as_tensor(curr_states).to(eng.device, torch.float32)
    try:
        four = len(inspect.signature(cond_fn).parameters) >= 4
    except (TypeError, ValueError):
        four = False
    scorers = () if metrics is None else tuple(metrics) if isinstance(metrics, (tuple, list)) else (metrics,)
    poses, plans = [], None
    hist_world = None                             # executed states of the previous plan, world frame [B,n_step_action,2]
    for step in range(n_sim_steps):
        with tm("step"):
            with tm("obs"):
                o = cond_fn(step, world, cs, plans) if four else cond_fn(step, world, cs)
                obs = o if isinstance(o, Mapping) else {"cond_feat": o, "curr_states": cs}
                gk = get_action_kwargs.get("guidance")
                has_goal = (gk if gk is not None else (policy._guidance or {})).get("goal") is not None
                if has_goal:
                    obs = dict(obs)
                    W = frames_from_pose(world)
                    if "world_from_agent" not in obs and "agent_from_world" not in obs:
                        obs["world_from_agent"] = W
                    if "agent_from_world" not in obs:
                        obs["agent_from_world"] = invert_frames(obs["world_from_agent"])
                    if "world_from_agent" not in obs:
                        obs["world_from_agent"] = invert_frames(obs["agent_from_world"])
                    if "agent_hist" not in obs:
                        hw = world[:, None, :2].expand(-1, n_step_action, -1) if hist_world is None else hist_world
                        obs["agent_hist"] = transform_points(hw, torch.as_tensor(obs["agent_from_world"]).float().to(hw.device))
                pg = policy._guidance or {}
                if gk is None and policy._follow_observation and any(pg.get(k) is not None for k in ("agent_collision", "map_collision", "social_group", "pair", "lane")):
                    obs = dict(obs)                   # the collision terms follow the observation: what cond_fn's lacks, from the loop's own state
                    if "world_from_agent" not in obs:
                        obs["world_from_agent"] = frames_from_pose(world)
                    if "curr_speed" not in obs:
                        obs["curr_speed"] = cs[:, 2].contiguous()
                    if "world" not in obs:
                        obs["world"] = world
            with tm("network"):
                _, info = policy.get_action(obs, step_index=step, **get_action_kwargs)
                traj = info["executed_trajectory"].contiguous()
            with tm("env_step"):
                if gather is not None:
                    plans = gather(traj)
                if has_goal:
                    hist_world = transform_points(traj[:, :n_step_action, :2], frames_from_pose(world))
                world, cs = eng.world_step(traj, world[:, :2].contiguous(), world[:, 2].contiguous(), n_step_action - 1)
                for scorer in scorers:
                    scored = plans if gather is not None else traj
                    if tuple(scored.shape) != (scorer.B_all, 52, 6):
                        raise CldError(f"closed_loop_rollout: metrics= scores all {scorer.B_all} agents, the executed plans are "
                                       f"{tuple(scored.shape)} (pass gather= so that every rank's plans are there)")
                    scorer.add_plans(scored)
        poses.append(world)
    return torch.stack(poses)


# upstream's pair-relation losses: config name -> (cld_pair_term kind, parameter names of (lo, hi, decay) and their defaults).  The first
# two are upstream's GUIDANCE_FUNC_MAP names (CollisionLoss, KeepDistanceLoss); the other three are this project's names for classes
# upstream reaches only through its language-model front end (StayAwayLoss / KeepDistanceLoss2, FrontCollisionLoss, CollideLeftSideLoss)
PAIR_NAMES = {
    "gptkeepdistance": ("keep_distance", 20, 1, (("min_distance", 5.0), ("max_distance", 15.0), None)),
    "gptcollision": ("collision", 2, 3, (("collision_radius", 1.0), None, None)),
    "gptstayaway": ("stay_away", 8, 1, (("min_dist", 5.0), ("max_dist", 15.0), ("decay_rate", 0.9))),
    "gptfrontcollision": ("front_collision", 2, 3, (None, None, None)),
    "gptcollideleftside": ("collide_left", 2, 3, (None, None, None)),
}


def pair_terms_from_config(guidance_config_list, scene_index, data_batch: Optional[Mapping] = None, num_samp: Optional[int] = None):
    """Upstream's pair-relation configs taken out of a guidance configuration -> (the list without them, the `pair` entry of a
    guidance dict -- Engine._pair -- or None when there is none).

    Names and parameters (upstream's names and defaults, guidance_loss.py): `gptkeepdistance` (target_ind = 20, ref_ind = 1,
    min_distance = 5, max_distance = 15), `gptcollision` (target_ind = 2, ref_ind = 3, collision_radius = 1), and this project's
    names `gptstayaway` (StayAwayLoss: target_ind = 8, ref_ind = 1, min_dist = 5, max_dist = 15, decay_rate = 0.9; with other
    parameters it is KeepDistanceLoss2), `gptfrontcollision` and `gptcollideleftside` (target_ind = 2, ref_ind = 3).  target_ind /
    ref_ind index the agents of the config's scene and are mapped to batch indices here.  The term carries `weight` per pair --
    Engine._pair folds weight / num_samp into the kernel's scale -- and, when `num_samp` is given, that `scale` itself; `configs`
    [(scene, config index)] and `names` say where each pair came from.  agent_from_world is taken from `data_batch` when it is there.
    ValueError: no world_from_agent in `data_batch`, an index outside the scene, target_ind == ref_ind, min > max.
    NotImplementedError: an `agents` subset (upstream's classes index the masked plans with scene indices: a subset shifts them)."""
    scene_index = torch.as_tensor(scene_index).reshape(-1).cpu()
    _, local = torch.unique_consecutive(scene_index, return_inverse=True)
    rest, term = [], None
    for si, cfgs in enumerate(guidance_config_list):
        keep = []
        for gi, cfg in enumerate(cfgs):
            if cfg["name"] not in PAIR_NAMES:
                keep.append(cfg)
                continue
            if data_batch is None or data_batch.get("world_from_agent") is None:
                raise ValueError(f"{cfg['name']} needs data_batch with world_from_agent")
            if cfg.get("agents") is not None:
                raise NotImplementedError(f"{cfg['name']} on an `agents` subset")
            kind, d_target, d_ref, (p_lo, p_hi, p_decay) = PAIR_NAMES[cfg["name"]]
            prm = cfg.get("params") or {}
            members = torch.nonzero(local == si).reshape(-1)
            ti, ri = int(prm.get("target_ind", d_target)), int(prm.get("ref_ind", d_ref))
            for what, v in (("target_ind", ti), ("ref_ind", ri)):
                if not 0 <= v < members.numel():
                    raise ValueError(f"{cfg['name']}: {what} = {v} outside scene {si} of {members.numel()} agents")
            if ti == ri:
                raise ValueError(f"{cfg['name']}: target_ind == ref_ind = {ti}")
            lo, hi, decay = (0.0 if q is None else float(prm.get(q[0], q[1])) for q in (p_lo, p_hi, p_decay))
            if p_hi is not None and lo > hi:
                raise ValueError(f"{cfg['name']}: min {lo} > max {hi}")
            if term is None:
                term = dict(target=[], ref=[], kind=[], lo=[], hi=[], decay=[], weight=[], configs=[], names=[],
                            world_from_agent=data_batch["world_from_agent"], agent_from_world=data_batch.get("agent_from_world"))
            for k, v in (("target", int(members[ti])), ("ref", int(members[ri])), ("kind", kind), ("lo", lo), ("hi", hi), ("decay", decay),
                         ("weight", float(cfg["weight"])), ("configs", (si, gi)), ("names", cfg["name"])):
                term[k].append(v)
        rest.append(keep)
    if term is not None and num_samp is not None:
        term["scale"] = [w / int(num_samp) for w in term["weight"]]
    return rest, term


# upstream's lane-projection losses, classes it reaches only through its language-model front end (LaneFollowingLoss,
# ChangeToLeftLaneLoss, FollowLaneLoss): this project's config name -> (cld_lane_term kind, the data_batch field its polylines come
# from, the parameter that names the target(s) and upstream's default)
LANE_NAMES = {
    "gptlanefollowing": ("following", "lane_points", "target_inds", [1, 2, 3]),
    "gptchangetoleftlane": ("change_left", "left_lane_points", "target_ind", 6),
    "gptfollowlane": ("follow_decayed", "lane_points", "target_ind", 4),
}


def gather_lane_lines(data_batch: Mapping, sources):
    """The world-frame polylines of a lane term: `sources` [(field of data_batch, batch row)] -> [L,S,3] float64 on the CPU, S the
    widest field's, NaN-padded."""
    fields = {k: torch.as_tensor(data_batch[k]).detach().to("cpu", torch.float64) for k in {src for src, _ in sources}}
    S = max(int(v.shape[1]) for v in fields.values())
    out = torch.full((len(sources), S, 3), float("nan"), dtype=torch.float64)
    for l, (src, row) in enumerate(sources):
        v = fields[src]
        out[l, :v.shape[1]] = v[row]
    return out


def lane_terms_from_config(guidance_config_list, scene_index, data_batch: Optional[Mapping] = None, num_samp: Optional[int] = None):
    """Upstream's lane-projection configs taken out of a guidance configuration -> (the list without them, the `lane` entry of a
    guidance dict -- Engine._lane -- or None when there is none).

    Names and parameters (upstream's constructors, guidance_loss.py:1578, 1799, 1962): `gptlanefollowing` (target_inds = [1, 2, 3]:
    K entries of weight / K, the reported value their mean), `gptchangetoleftlane` (target_ind = 6, on the LEFT lane's polyline),
    `gptfollowlane` (target_ind = 4, decay_rate = 0.9, T = 52; another T is refused).  The indices are those of the config's scene
    and are mapped to batch indices here.  The polylines come from data_batch['lane_points'] / ['left_lane_points'] [B_all,S,3]
    (x, y, heading in the WORLD frame, NaN-padded, S <= 1024): per agent the current (left) lane already concatenated with its
    successors, as upstream's lines 617-639 would -- choosing the lane is the caller's.  Only targeted rows need be finite.  The
    term carries the world polylines of the targeted rows (`world_lines`, `sources`), `line_frame`, agent_from_world (from
    `data_batch`, or the inverse of its world_from_agent) -- Engine._lane prepares them once per call -- and per entry agent, line,
    kind, decay, `weight` (Engine._lane folds weight / num_samp into the kernel's scale; with `num_samp` given, that `scale` too),
    `configs` (scene, config index) and `names`; the entries are ordered by agent (stable), as the kernel wants them.
    ValueError: no frames or no polylines in `data_batch`, an index outside the scene, T != 52, a targeted row without a usable
    polyline (fewer than two distinct finite points).  NotImplementedError: an `agents` subset."""
    scene_index = torch.as_tensor(scene_index).reshape(-1).cpu()
    _, local = torch.unique_consecutive(scene_index, return_inverse=True)
    rest, entries, sources = [], [], []
    for si, cfgs in enumerate(guidance_config_list):
        keep = []
        for gi, cfg in enumerate(cfgs):
            if cfg["name"] not in LANE_NAMES:
                keep.append(cfg)
                continue
            kind, field, p_target, d_target = LANE_NAMES[cfg["name"]]
            if data_batch is None or (data_batch.get("agent_from_world") is None and data_batch.get("world_from_agent") is None):
                raise ValueError(f"{cfg['name']} needs data_batch with agent_from_world or world_from_agent")
            if data_batch.get(field) is None:
                raise ValueError(f"{cfg['name']} needs data_batch['{field}'] [B,S,3]")
            if cfg.get("agents") is not None:
                raise NotImplementedError(f"{cfg['name']} on an `agents` subset")
            prm = cfg.get("params") or {}
            if kind == "follow_decayed" and int(prm.get("T", 52)) != 52:
                raise ValueError(f"{cfg['name']}: T = {prm['T']} (only the full horizon, T = 52, is built)")
            members = torch.nonzero(local == si).reshape(-1)
            tg = prm.get(p_target, d_target)
            tg = [int(v) for v in (tg if isinstance(tg, (list, tuple)) else [tg])]
            if not tg:
                raise ValueError(f"{cfg['name']}: no target")
            pts = torch.as_tensor(data_batch[field])
            if pts.dim() != 3 or pts.shape[0] != scene_index.numel() or pts.shape[2] != 3 or not 2 <= pts.shape[1] <= _lib.LANE_MAX_PTS:
                raise ValueError(f"{cfg['name']}: data_batch['{field}'] must be [{scene_index.numel()}, 2..{_lib.LANE_MAX_PTS}, 3], got {tuple(pts.shape)}")
            for v in tg:
                if not 0 <= v < members.numel():
                    raise ValueError(f"{cfg['name']}: {p_target} = {v} outside scene {si} of {members.numel()} agents")
                a = int(members[v])
                xy = pts[a, :, :2].double()
                xy = xy[torch.isfinite(xy).all(dim=1)]
                if xy.shape[0] < 2 or bool((xy == xy[:1]).all()):
                    raise ValueError(f"{cfg['name']}: agent {v} of scene {si} has no usable polyline in data_batch['{field}']")
                if (field, a) not in sources:
                    sources.append((field, a))
                entries.append(dict(agent=a, line=sources.index((field, a)), kind=kind, decay=float(prm.get("decay_rate", 0.9)),
                                    weight=float(cfg["weight"]) / len(tg), configs=(si, gi), names=cfg["name"]))
        rest.append(keep)
    if not entries:
        return rest, None
    entries.sort(key=lambda e: e["agent"])                                # (stable: an agent's entries keep the configs' order)
    F = data_batch.get("agent_from_world")
    term = {k: [e[k] for e in entries] for k in ("agent", "line", "kind", "decay", "weight", "configs", "names")}
    term.update(world_lines=gather_lane_lines(data_batch, sources), sources=sources, line_frame=[a for _, a in sources],
                agent_from_world=F if F is not None else invert_frames(torch.as_tensor(data_batch["world_from_agent"]).float()))
    if num_samp is not None:
        term["scale"] = [w / int(num_samp) for w in term["weight"]]
    return rest, term


def social_groups_from_config(guidance_config_list, scene_index, data_batch: Optional[Mapping] = None):
    """Upstream's `social_group` configs (SocialGroupLoss, guidance_loss.py:1137-1207) taken out of a guidance configuration ->
    (the list without them, the `social_group` entry of a guidance dict -- Engine._social -- or None when there is none).

    One group per config: the config's `agents` (local indices into its scene) or the whole scene; params leader_idx = 0,
    social_dist = 1.5, cohesion = 0.8.  `leader_idx` is compared with the agents' BATCH indices, as upstream's code does (its
    docstring says "index in the scene"); one that names no member detaches nobody.  scale = weight / members, as for the goal
    losses.  ValueError:
    no world_from_agent in `data_batch`, a group of fewer than 2 members (upstream cannot run it: randint(0, 0)), an agent in two
    groups, cohesion outside [0, 1]."""
    scene_index = torch.as_tensor(scene_index).reshape(-1).cpu()
    _, local = torch.unique_consecutive(scene_index, return_inverse=True)
    rest, term = [], None
    taken = torch.zeros(scene_index.numel(), dtype=torch.bool)
    for si, cfgs in enumerate(guidance_config_list):
        keep = []
        for gi, cfg in enumerate(cfgs):
            if cfg["name"] != "social_group":
                keep.append(cfg)
                continue
            if data_batch is None or data_batch.get("world_from_agent") is None:
                raise ValueError("social_group needs data_batch with world_from_agent")
            members = torch.nonzero(local == si).reshape(-1)
            agents = cfg.get("agents")
            idx = members if agents is None else members[torch.as_tensor(agents, dtype=torch.long)]
            idx = torch.sort(idx)[0]
            if idx.numel() < 2:
                raise ValueError(f"social_group: a group needs at least 2 members, scene {si} config {gi} has {idx.numel()}")
            if idx.unique().numel() != idx.numel() or bool(taken[idx].any()):
                raise ValueError("social_group: an agent is in two groups")
            taken[idx] = True
            prm = cfg.get("params") or {}
            coh = float(prm.get("cohesion", 0.8))
            if not 0.0 <= coh <= 1.0:
                raise ValueError(f"social_group: cohesion {coh} outside [0, 1]")
            if term is None:
                term = dict(groups=[], leader=[], social_dist=[], cohesion=[], scale=[], world_from_agent=data_batch["world_from_agent"])
            term["groups"].append(idx.tolist())
            term["leader"].append(int(prm.get("leader_idx", 0)))
            term["social_dist"].append(float(prm.get("social_dist", 1.5)))
            term["cohesion"].append(coh)
            term["scale"].append(float(cfg["weight"]) / idx.numel())
        rest.append(keep)
    return rest, term


def guidance_from_config(guidance_config_list, scene_index, horizon: int = 52, data_batch: Optional[Mapping] = None,
                         map_source: Optional[Mapping] = None) -> dict:
    """Upstream's guidance configuration -> the `guidance=` dict of `DmModel.forward` / `Engine.sample`.

    `guidance_config_list` is what `DiffuserTrafficModel.set_guidance` takes (`src/tbsim/algos/algos.py`, built by
    `DiffuserGuidance`, `src/tbsim/utils/guidance_loss.py:2106-2175`): one list per scene of
    `{'name', 'weight', 'params', 'agents'}` dicts; `scene_index [B]` maps agents to scenes (consecutive runs).  Each loss
    is averaged over the agents it applies to within its scene and multiplied by its weight; that is folded into the
    per-agent scales of the kernel: weight / (agents * horizon) for the per-step losses, weight / agents for the waypoint
    losses.  Supported names: target_speed, speed_limit, acc_limit, target_pos_at_time, target_pos, agent_collision (needs
    `data_batch` with `extent`, `world_from_agent`, `curr_speed`: the observation fields upstream's loss reads,
    guidance_loss.py:506-510), map_collision (`extent`, `raster_from_agent`, `drivable_map`, `curr_speed`, :773-775; with `map_source`
    -- Engine._map_collision -- the entry carries that instead of a drivable_map, `data_batch` needs only `extent` (and `curr_speed`,
    unless every get_action's observation brings it) and raster_from_agent defaults to the source's raster settings) and the world-frame
    waypoint losses global_target_pos / global_target_pos_at_time (:930-1135; params target_pos, target_time, urgency, pref_speed = 1.42,
    dt = 0.1, min_progress_dist = 0.5, target_tolerance = None / 2, action_num = 5, all indexed by the config's `agents`; scale =
    weight / agents; at most one per agent, one dt and one min_progress_dist per call); at most
    one of each other loss per scene, one parameter set per call; the others (stop signs, lane keeping, ...) are not built, and
    `social_group` is refused HERE too: it is scene-coupled and random, and enters one level up (social_groups_from_config, which
    CldPolicy.set_guidance calls first); so do the pair-relation names (`gptcollision`, `gptkeepdistance`, ...: pair_terms_from_config) and the lane names (`gptlanefollowing`, ...: lane_terms_from_config).  One speed / acceleration limit value per call."""
    scene_index = torch.as_tensor(scene_index).reshape(-1).cpu()
    B = scene_index.numel()
    _, local = torch.unique_consecutive(scene_index, return_inverse=True)
    if len(guidance_config_list) != int(local.max()) + 1:
        raise ValueError("guidance config list must hold one entry per scene")
    out: dict = {}
    ts_scale = torch.zeros(B); ts = torch.zeros(B, horizon); has_ts = False
    sl_scale = torch.zeros(B); al_scale = torch.zeros(B); sl = al = None
    tp = torch.zeros(B, 2); tt = torch.zeros(B, dtype=torch.int32); tp_scale = torch.zeros(B); has_tp = False
    col = mcol = goal = None
    for si, cfgs in enumerate(guidance_config_list):
        members = torch.nonzero(local == si).reshape(-1)
        for cfg in cfgs:
            name, wgt, prm, agents = cfg["name"], float(cfg["weight"]), cfg["params"], cfg.get("agents")
            idx = members if agents is None else members[torch.as_tensor(agents, dtype=torch.long)]
            n = max(1, idx.numel())
            if name == "target_speed":       # params['target_speed'] is indexed by the whole batch (guidance_loss.py:231-241)
                if bool((ts_scale[idx] != 0).any()):
                    raise ValueError("two target_speed losses on one agent")
                full = torch.as_tensor(prm["target_speed"], dtype=torch.float32)
                ts[idx] = full[idx, :horizon]
                ts_scale[idx] = wgt / (n * horizon)
                has_ts = True
            elif name in ("speed_limit", "acc_limit"):
                val = float(prm[name])
                if name == "speed_limit":
                    if sl is not None and sl != val:
                        raise ValueError("one speed_limit value per call")
                    sl = val; sl_scale[idx] += wgt / (n * horizon)
                else:
                    if al is not None and al != val:
                        raise ValueError("one acc_limit value per call")
                    al = val; al_scale[idx] += wgt / (n * horizon)
            elif name in ("target_pos_at_time", "target_pos"):
                if bool((tp_scale[idx] != 0).any()):
                    raise ValueError("two waypoint losses on one agent")
                tp[idx] = torch.as_tensor(prm["target_pos"], dtype=torch.float32).reshape(-1, 2)
                if name == "target_pos_at_time":
                    tt[idx] = torch.as_tensor(prm["target_time"], dtype=torch.int32).reshape(-1)
                else:                        # any step >= int(min_target_time * horizon): encoded as -(m + 1)
                    tt[idx] = -(int(float(prm.get("min_target_time", 0.0)) * horizon) + 1)
                tp_scale[idx] = wgt / n
                has_tp = True
            elif name == "agent_collision":
                if data_batch is None or any(k not in data_batch for k in ("extent", "world_from_agent", "curr_speed")):
                    raise ValueError("agent_collision needs data_batch with extent, world_from_agent and curr_speed")
                S = int(local.max()) + 1
                key = (int(prm.get("num_disks", 5)), float(prm.get("buffer_dist", 0.2)), float(prm.get("decay_rate", 0.9)), float(prm.get("guide_moving_speed_th", 0.5)))
                if col is None:
                    col = dict(extent=data_batch["extent"], world_from_agent=data_batch["world_from_agent"], curr_speed=data_batch["curr_speed"],
                               scene_index=scene_index, weight=[0.0] * S, agents={}, num_disks=key[0], buffer_dist=key[1], decay_rate=key[2],
                               guide_moving_speed_th=key[3])
                elif (col["num_disks"], col["buffer_dist"], col["decay_rate"], col["guide_moving_speed_th"]) != key:
                    raise ValueError("one agent_collision parameter set per call")
                if col["weight"][si] != 0.0:
                    raise ValueError("two agent_collision losses on one scene")
                col["weight"][si] = wgt
                if agents is not None:
                    col["agents"][si] = list(agents)
                if prm.get("excluded_agents") is not None:
                    # batch indices, as upstream takes them (guidance_loss.py:447,586-593); each config's loss sees the pairs of ITS scene
                    # only, so a listed agent of another scene changes nothing there: keep this scene's
                    mem = set(int(b) for b in members)
                    col.setdefault("excluded_agents", []).extend(int(b) for b in prm["excluded_agents"] if int(b) in mem)
            elif name == "map_collision":
                if map_source is None:
                    need = ("extent", "raster_from_agent", "drivable_map", "curr_speed")
                    if data_batch is None or any(k not in data_batch for k in need):
                        raise ValueError("map_collision needs data_batch with extent, raster_from_agent, drivable_map and curr_speed")
                    fields = {k: data_batch[k] for k in need}
                else:
                    if data_batch is None or "extent" not in data_batch:
                        raise ValueError("map_collision with a map_source needs data_batch with extent")
                    rfa = data_batch["raster_from_agent"] if "raster_from_agent" in data_batch else raster_frames(map_source, B)
                    fields = dict(extent=data_batch["extent"], raster_from_agent=rfa, map_source=dict(map_source))
                    if "curr_speed" in data_batch:
                        fields["curr_speed"] = data_batch["curr_speed"]
                if agents is not None:
                    raise NotImplementedError("map_collision on an `agents` subset (upstream itself cannot run it: guidance_loss.py:857-859)")
                S = int(local.max()) + 1
                key = (tuple(int(v) for v in prm.get("num_points_lw", (10, 10))), float(prm.get("decay_rate", 0.9)), float(prm.get("guide_moving_speed_th", 0.5)))
                if mcol is None:
                    mcol = dict(fields, scene_index=scene_index, weight=[0.0] * S, num_points_lw=key[0], decay_rate=key[1],
                                guide_moving_speed_th=key[2])
                elif (tuple(mcol["num_points_lw"]), mcol["decay_rate"], mcol["guide_moving_speed_th"]) != key:
                    raise ValueError("one map_collision parameter set per call")
                if mcol["weight"][si] != 0.0:
                    raise ValueError("two map_collision losses on one scene")
                mcol["weight"][si] = wgt
            elif name in GOAL_KINDS:
                # GlobalTargetPosLoss / GlobalTargetPosAtTimeLoss (guidance_loss.py:930-1135): the parameters are indexed by the config's
                # `agents` (upstream asserts x.size(0) == target_pos.size(0) AFTER masking); frames, global_t and the reached mask
                # come with every get_action (CldPolicy._goal_for_step)
                M = idx.numel()
                if goal is None:
                    goal = dict(kind=torch.zeros(B, dtype=torch.int32), target_pos=torch.zeros(B, 2), target_time=torch.zeros(B, dtype=torch.int32),
                                urgency=torch.zeros(B), pref_speed=torch.full((B,), 1.42), scale=torch.zeros(B), dt=None, min_progress_dist=None,
                                configs=[])
                if bool((goal["kind"][idx] != 0).any()):
                    raise ValueError("two goal losses on one agent")

                def per_agent(key, default=None, dtype=torch.float32):
                    v = prm.get(key, default)
                    if v is None:
                        raise ValueError(f"{name} needs params['{key}']")
                    v = torch.as_tensor(v, dtype=dtype).reshape(-1)
                    if v.numel() not in (1, M):
                        raise ValueError(f"{name}: params['{key}'] must hold one entry per agent of the config ({M}), got {v.numel()}")
                    return v.expand(M)
                tpos = torch.as_tensor(prm["target_pos"], dtype=torch.float32).reshape(-1, 2)
                if tpos.shape[0] != M:
                    raise ValueError(f"{name}: params['target_pos'] must hold one position per agent of the config ({M}), got {tpos.shape[0]}")
                goal["kind"][idx] = GOAL_KINDS[name]
                goal["target_pos"][idx] = tpos
                goal["urgency"][idx] = per_agent("urgency")
                goal["pref_speed"][idx] = per_agent("pref_speed", 1.42)
                goal["scale"][idx] = wgt / n
                dt = float(prm.get("dt", 0.1))
                if goal["dt"] is not None and goal["dt"] != dt:
                    raise ValueError("one dt per call for the goal losses")
                goal["dt"] = dt
                if name == "global_target_pos":
                    mpd = float(prm.get("min_progress_dist", 0.5))
                    if goal["min_progress_dist"] is not None and goal["min_progress_dist"] != mpd:
                        raise ValueError("one min_progress_dist per call")
                    goal["min_progress_dist"] = mpd
                    tol = prm.get("target_tolerance", None)
                else:
                    goal["target_time"][idx] = per_agent("target_time", dtype=torch.int32)
                    tol = prm.get("target_tolerance", 2)
                goal["configs"].append((idx.clone(), None if tol is None else float(tol), int(prm.get("action_num", 5))))
            else:
                raise NotImplementedError(f"guidance loss '{name}' is not built (target_speed, speed_limit, acc_limit, "
                                          f"target_pos_at_time, target_pos, agent_collision, map_collision, global_target_pos, "
                                          f"global_target_pos_at_time are)")
    if has_ts:
        out["target_speed"], out["loss_scale"] = ts, ts_scale
    if sl is not None:
        out["speed_limit"] = (sl, sl_scale)
    if al is not None:
        out["acc_limit"] = (al, al_scale)
    if has_tp:
        out["target_pos"] = (tp, tt, tp_scale)
    if col is not None:
        col["agents"] = col["agents"] or None
        out["agent_collision"] = col
    if mcol is not None:
        out["map_collision"] = mcol
    if goal is not None:
        if goal["min_progress_dist"] is None:
            goal["min_progress_dist"] = 0.5
        out["goal"] = goal
    if not out:
        raise ValueError("no guidance loss configured")
    return out
