"""fp64 restatement of the guidance satisfaction metrics (include/cld.h `cld_guide_metrics_step` / `cld_guide_metrics_read`) and the
seeded cases of their tests.

The restatement follows the header's definitions (and upstream's classes, src/tbsim/utils/guidance_metrics.py) in numpy float64, one
function per kind.  The kernel decides its flags in fp32, so the cases keep every discrete decision out of fp32's reach and `restate`
reports the margins, which `build_case` asserts:
  * REL_MARGIN: every disk distance against its threshold (radius sum + buffer) relative to the threshold, and the deciding
    separating-axis gap / overlap of every pair relative to the sum of the four half extents (an upper bound of every axis threshold);
  * PIX_MARGIN (px): every sampled raster coordinate (box corners, disk samples) and the map coordinate of every sampled pixel, from
    the nearest half-integer.
Positions are multiples of 2^-10 m and extents multiples of 2^-6 m, exact in fp32.  A step of an agent whose pixels are sampled is
re-drawn with a small seeded shift until its pixel margin holds; the pair margins are asserted for the fixed seed.

The geometry (separating axes, disk samples, drivable pixel) is tests/metrics_cases.py's, which the existing scorer is held to.
"""
import numpy as np

from tests import metrics_cases as MC
from tests import raster_cases as RC

REL_MARGIN = 1e-4
PIX_MARGIN = 1e-3
SCENE_SIZES = (7, 70, 1)
N_STEPS = 11                                     # the initial pose plus two plans of five
CFG = dict(MC.BASE_CFG, height=64, width=64)
ABSENT = (5, (3, 4, 5, 6))                       # scene 0's agent 5 is NaN on these steps (a member of collision and map entries only)
FLAG_KINDS = ("agent_collision", "agent_collision_disk", "social_dist", "map_collision", "map_collision_disk")


# ------------------------------------------------------------------------------------------------ per-step pieces (float64)
def agent_from_world(pose):
    """[...,3] poses -> [...,3,3]: rows (c, s, -(c x) - (s y)), (-s, c, (s x) - (c y)), (0, 0, 1)."""
    c, s = np.cos(pose[..., 2]), np.sin(pose[..., 2])
    M = np.zeros(pose.shape[:-1] + (3, 3))
    M[..., 0, 0], M[..., 0, 1], M[..., 0, 2] = c, s, -(c * pose[..., 0]) - (s * pose[..., 1])
    M[..., 1, 0], M[..., 1, 1], M[..., 1, 2] = -s, c, (s * pose[..., 0]) - (c * pose[..., 1])
    M[..., 2, 2] = 1.0
    return M


def to_frame(M, xy):
    """(x m0 + y m1) + m2 per row: what batch_nd_transform_points_np computes for one point per matrix."""
    return np.stack([(xy[..., 0] * M[..., 0, 0] + xy[..., 1] * M[..., 0, 1]) + M[..., 0, 2],
                     (xy[..., 0] * M[..., 1, 0] + xy[..., 1] * M[..., 1, 1]) + M[..., 1, 2]], -1)


def norm2(d):
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])


def box_pixels(extent2, cfg):
    """The 4 corner pixels of an agent with extent2 [2] in its own raster (yaw 0), get_box_world_coords' order -> (u [4], v [4], margin)."""
    ox, oy = RC.offsets(cfg)
    W, H = cfg["width"], cfg["height"]
    h0, h1 = cfg["px_per_m"] * extent2[0] / 2.0, cfg["px_per_m"] * extent2[1] / 2.0
    fu = np.clip(ox + np.array([-h0, -h0, h0, h0]), 0, W - 1)
    fv = np.clip(oy + np.array([-h1, h1, h1, -h1]), 0, H - 1)
    margin = min(np.abs(fu - np.floor(fu) - 0.5).min(), np.abs(fv - np.floor(fv) - 0.5).min())
    return np.clip(np.rint(fu), 0, W - 1).astype(np.int64), np.clip(np.rint(fv), 0, H - 1).astype(np.int64), margin


def map_flags(case, scene, pose, extent2):
    """-> (box flag, disk flag, pixel margin) of one valid agent of `scene` at pose."""
    cfg = case["cfg"]
    ub, vb, m1 = box_pixels(extent2, cfg)
    ud, vd, m2 = MC.sample_pixels(extent2, cfg)
    db, m3, _ = MC.drv_at(case, cfg, scene, pose, ub, vb)
    dd, m4, _ = MC.drv_at(case, cfg, scene, pose, ud[:52], vd[:52])
    return float((db == 0).any()), float((dd == 0).any()), min(m1, m2, m3, m4)


def scene_pairs(case, scene, world_t):
    """All pairs of one scene at one step -> dict(rows, valid [n], disk_d [n,n], rsum [n,n], box [n,n] bool, rel_margin): NaN / False for
    pairs with an invalid agent and on the diagonal."""
    ss = case["scene_start"]
    rows = np.arange(ss[scene], ss[scene + 1])
    P, E = world_t[rows], case["extent"].astype(np.float64)[rows, :2]
    valid = ~(np.isnan(P[:, 0]) | np.isnan(P[:, 1]))
    n = len(rows)
    ok = valid[:, None] & valid[None] & ~np.eye(n, dtype=bool)
    Pz = np.where(valid[:, None], P, 0.0)
    d = norm2(Pz[None, :, :2] - Pz[:, None, :2])
    rsum = E.min(1)[:, None] / 2 + E.min(1)[None] / 2
    g = MC.sat_gaps(Pz[:, None], E[:, None], Pz[None], E[None])
    box = (g <= 0).all(-1) & ok
    decide = np.where((g <= 0).all(-1), (-g).min(-1), g.max(-1)) / (E.sum(1)[:, None] / 2 + E.sum(1)[None] / 2)
    return dict(rows=rows, valid=valid, ok=ok, d=d, rsum=rsum, box=box, rel_margin=float(np.where(ok, decide, np.inf).min()))


# ------------------------------------------------------------------------------------------------ the restatement
def restate(case):
    """-> dict(values {key: float}, per_member {key: [n]}, partner [T,B] (the box partner as a batch row, -1: none), n_terms {key},
    scale {key} (the largest |term| or |coordinate| entering the value), rel_margin, pix_margin) for every entry of the case's table."""
    from cld_amd.metrics import guidance_metric_table
    table = guidance_metric_table(case["config"], case["scene_start"], case.get("constraint"))
    ss = case["scene_start"]
    world, speed, acc = (np.asarray(case[k], np.float64) for k in ("world", "speed", "acc"))
    ext = case["extent"].astype(np.float64)[:, :2]
    T, B = world.shape[:2]
    S = len(ss) - 1
    pairs = [[scene_pairs(case, s, world[t]) for s in range(S)] for t in range(T)]
    rel_margin = min(p["rel_margin"] for row in pairs for p in row)
    pix_margin = np.inf
    partner = np.full((T, B), -1, np.int64)
    for t in range(T):
        for s in range(S):
            p = pairs[t][s]
            partner[t, p["rows"]] = np.where(p["box"].any(1), p["rows"][p["box"].argmax(1)], -1)
    mapf = {}                                                       # (t, row) -> (box, disk)
    values, members_out, n_terms, scale = {}, {}, {}, {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for ent in table:
            key, kind, s, mem, prm = ent["key"], ent["kind"], ent["scene"], np.array(ent["members"]), ent["params"]
            n, loc = len(mem), np.array(ent["members"]) - ss[s]
            excl = set(ent["excluded"])
            if kind == "target_speed":
                L = int(prm[0])
                ts = np.array(prm[1:]).reshape(n, L)
                terms = np.stack([np.abs(speed[t, mem] - ts[:, t]) if t < L else np.zeros(n) for t in range(T)])      # [T, n]
                cnt = (~np.isnan(terms)).sum(1)
                steps = np.where(cnt > 0, np.nansum(terms, 1) / np.maximum(cnt, 1), np.nan)
                values[key] = np.mean(steps)
                mcnt = (~np.isnan(terms)).sum(0)
                members_out[key] = np.where(mcnt > 0, np.nansum(terms, 0) / np.maximum(mcnt, 1), np.nan)
                n_terms[key], scale[key] = T * n, max(np.nanmax(np.abs(speed[:, mem])), np.abs(ts).max())
            elif kind in ("speed_limit", "acc_limit"):
                x = speed[:, mem] if kind == "speed_limit" else np.abs(acc[:, mem])
                terms = np.clip(x - prm[0], 0, None)
                values[key] = np.mean(np.mean(terms, 1))
                members_out[key] = np.mean(terms, 0)
                n_terms[key], scale[key] = T * n, max(np.nanmax(np.abs(x)), abs(prm[0]))
            elif kind in ("agent_collision", "agent_collision_disk", "social_dist"):
                flags = np.zeros((T, n))
                buffer = prm[0] if kind == "social_dist" else 0.0
                for t in range(T):
                    p = pairs[t][s]
                    if kind == "agent_collision":
                        for k, (i, li) in enumerate(zip(mem, loc)):
                            j = partner[t, i]
                            flags[t, k] = float(j >= 0 and not (i in excl and j in excl))
                    else:
                        keep = np.array([r not in excl for r in p["rows"]])
                        thr = p["rsum"] + buffer
                        use = p["ok"] & keep[None]
                        rel_margin = min(rel_margin, float(np.where(use, np.abs(p["d"] - thr) / thr, np.inf).min()))
                        hit = ((p["d"] < thr) & use).any(1)
                        flags[t] = [float(hit[li] and i not in excl) for i, li in zip(mem, loc)]
                members_out[key] = np.amax(flags, 0)
                values[key] = np.mean(members_out[key])
                n_terms[key], scale[key] = n, 1.0
            elif kind in ("map_collision", "map_collision_disk"):
                flags = np.zeros((T, n))
                for t in range(T):
                    for k, i in enumerate(mem):
                        if np.isnan(world[t, i, 0]) or np.isnan(world[t, i, 1]):
                            continue                                # absent: records 0, stays in the denominator
                        if (t, i) not in mapf:
                            bf, df, m = map_flags(case, s, world[t, i], ext[i])
                            mapf[(t, i)] = (bf, df)
                            pix_margin = min(pix_margin, m)
                        flags[t, k] = mapf[(t, i)][0 if kind == "map_collision" else 1]
                members_out[key] = np.sum(flags, 0) / float(T)
                values[key] = np.mean(members_out[key])
                n_terms[key], scale[key] = n, 1.0
            elif kind in ("target_pos", "global_target_pos", "target_pos_at_time", "global_target_pos_at_time"):
                pos = np.array(prm[:2 * n]).reshape(n, 2)
                xy = world[:, mem, :2]
                if kind.startswith("target_pos"):
                    xy = to_frame(agent_from_world(world[0, mem])[None], xy)
                d = norm2(xy - pos[None])                           # [T, n]
                if kind.endswith("at_time"):
                    tt = np.array(prm[2 * n:]).astype(np.int64) + 1
                    members_out[key] = np.array([d[tt[k], k] if 0 <= tt[k] < T else np.nan for k in range(n)])
                else:
                    cur = np.full(n, np.inf)
                    for t in range(T):
                        better = d[t] < cur
                        cur[better] = d[t][better]
                    members_out[key] = cur
                values[key] = np.mean(members_out[key])
                n_terms[key] = n
                scale[key] = max(np.nanmax(np.abs(world[:, mem, :2])), np.abs(pos).max(), np.nanmax(np.where(np.isinf(d), 0.0, d)))
            elif kind == "social_group":
                xy = world[:, mem, :2]
                err = np.zeros((T, n))
                for t in range(T):
                    pd = norm2(xy[t][None] - xy[t][:, None])
                    pd[np.arange(n), np.arange(n)] = np.inf
                    err[t] = np.abs(np.amin(pd, -1) - prm[0])
                members_out[key] = np.mean(err, 0)
                values[key] = np.mean(err.T)
                finite = err[np.isfinite(err)]
                n_terms[key], scale[key] = T * n, max(np.nanmax(np.abs(xy)), finite.max() if finite.size else 0.0)
            else:
                raise AssertionError(kind)
    return dict(table=table, values=values, per_member=members_out, partner=partner, n_terms=n_terms, scale=scale,
                rel_margin=float(rel_margin), pix_margin=float(pix_margin))


def pre_action_states(world0, speed0, acc0, plans_list, n_step_action=5):
    """`GuidanceMetrics.add_plans` restated (float64): the states scored for a list of plans [B,52,6], upstream's order -> (world [T,B,3],
    speed [T,B], acc [T,B], the carried (pose, speed, acc))."""
    pose, sp, ac = np.asarray(world0, np.float64), np.asarray(speed0, np.float64), np.asarray(acc0, np.float64)
    W, V, A = [], [], []
    for plans in plans_list:
        plans = np.asarray(plans, np.float64)
        W.append(pose); V.append(sp); A.append(ac)
        start = pose
        for k in range(n_step_action):
            pose, sp, ac = RC.world_step(plans, start[:, :2], start[:, 2], k), plans[:, k, 2], plans[:, k, 4]
            if k < n_step_action - 1:
                W.append(pose); V.append(sp); A.append(ac)
    return np.stack(W), np.stack(V), np.stack(A), (pose, sp, ac)


# ------------------------------------------------------------------------------------------------ the cases
def _q(x, bits=10):
    return np.round(np.asarray(x, np.float64) * (1 << bits)) / (1 << bits)


def configs(ss, rng, centres, world0):
    """The guidance config list and the constraint config of the main case (`agents` scene-local; excluded_agents and target_speed by
    batch row, as set_guidance takes them)."""
    B = int(ss[-1])
    s1 = int(ss[1])
    near = lambda s, k: [float(v) for v in _q(centres[s] + rng.uniform(-20.0, 20.0, (k, 2))).reshape(-1)]
    local = lambda rows, k: [float(v) for v in _q(rng.uniform(-4.0, 12.0, (k, 2))).reshape(-1)]
    ts_short = _q(rng.uniform(0.0, 12.0, (B, 8)), 6)                # shorter than the episode: zeros from step 8 on
    ts_long = _q(rng.uniform(0.0, 12.0, (B, 20)), 6)
    cfg0 = [
        dict(name="agent_collision", weight=1.0, agents=None, params=dict(excluded_agents=[0, 1, s1 + 2])),       # (s1 + 2: another scene's row)
        dict(name="map_collision", weight=1.0, agents=None, params=dict()),
        dict(name="target_speed", weight=1.0, agents=[2, 3, 4], params=dict(target_speed=ts_short)),
        dict(name="target_pos", weight=1.0, agents=[3, 4, 6], params=dict(target_pos=np.array(local(0, 3)).reshape(3, 2))),
        dict(name="target_pos_at_time", weight=1.0, agents=[3, 6],
             params=dict(target_pos=np.array(local(0, 2)).reshape(2, 2), target_time=[N_STEPS - 2, 4])),           # 9 + 1 = the last scored step
        dict(name="agent_collision", weight=1.0, agents=[0, 1, 2], params=dict(excluded_agents=[1, 0], buffer_dist=1.0)),
    ]
    cfg1 = [
        dict(name="agent_collision", weight=1.0, agents=None, params=dict(excluded_agents=[s1 + 69, s1 + 3, s1 + 10, s1 + 68], buffer_dist=0.5)),
        dict(name="map_collision", weight=1.0, agents=[1, 5, 64, 69, 30], params=dict()),
        dict(name="speed_limit", weight=1.0, agents=None, params=dict(speed_limit=4.0)),
        dict(name="acc_limit", weight=1.0, agents=list(range(10)), params=dict(acc_limit=1.0)),
        dict(name="social_group", weight=1.0, agents=[2, 7, 20, 65], params=dict(social_dist=3.0)),
        dict(name="global_target_pos", weight=1.0, agents=[0, 68], params=dict(target_pos=np.array(near(1, 2)).reshape(2, 2))),
        dict(name="global_target_pos_at_time", weight=1.0, agents=[4, 67],
             params=dict(target_pos=np.array(near(1, 2)).reshape(2, 2), target_time=[0, 6])),
        dict(name="target_speed", weight=1.0, agents=None, params=dict(target_speed=ts_long)),
    ]
    cfg2 = [
        dict(name="social_group", weight=1.0, agents=None, params=dict(social_dist=2.0)),                          # one agent: inf
        dict(name="map_collision", weight=1.0, agents=None, params=dict()),                                        # no map: drivable
        dict(name="agent_collision", weight=1.0, agents=None, params=dict()),
        dict(name="speed_limit", weight=1.0, agents=[0], params=dict(speed_limit=2.5)),
    ]
    constraint = [dict(locs=np.array(local(0, 1)).reshape(1, 2), times=[5], agents=[4]), dict(locs=np.array(local(1, 2)).reshape(2, 2), times=[3, 8], agents=[8, 9]),
                  dict(locs=np.array(local(2, 1)).reshape(1, 2), times=[2], agents=None)]
    return [cfg0, cfg1, cfg2], constraint


def build_case(seed=12):
    """-> dict(world [11,78,3], speed, acc [11,78] float32, extent [78,3] float32, scene_start, maps, scene_map, map_from_world, cfg,
    config, constraint).  Scenes of 7, 70 and 1 agents; a map on scenes 0 and 1.  Scene 0 opens with three standing agents of 4 x 2.125 m: 0 and 1
    overlap (both excluded: the partner of 0 is ABOVE it), 2 overlaps 1 only (so 1's lowest partner is the excluded 0 although it also
    touches 2).  In scene 1, agent 69 drives beside agent 68 (both excluded, partner in the second stride of 64).  Every other agent
    drives an arc.  Scene 0's agent 5 is NaN on steps 3 .. 6.  Both margins are asserted."""
    rng = np.random.default_rng(seed)
    cfg = dict(CFG)
    S, T = len(SCENE_SIZES), N_STEPS
    ss = np.concatenate([[0], np.cumsum(SCENE_SIZES)]).astype(np.int32)
    B = int(ss[-1])
    centres = [_q(rng.uniform(-30.0, 30.0, 2)) for _ in range(S)]
    maps, scene_map, mfw = MC._maps(rng, centres)                    # scene s uses map s % 3, 2 meaning none
    case = dict(scene_start=ss, maps=maps, scene_map=scene_map, map_from_world=mfw, cfg=cfg)
    world, extent = np.zeros((T, B, 3)), np.zeros((B, 3))
    tt = MC.SIM_DT * np.arange(T)
    for s, n in enumerate(SCENE_SIZES):
        for k in range(n):
            i = ss[s] + k
            while True:                                              # the extent: its own raster pixels keep the margin
                e = np.array([4.0, 2.125]) if (s == 0 and k < 3) else _q(np.array([rng.uniform(3.5, 5.5), rng.uniform(1.6, 2.4)]), 6)
                if min(MC.sample_pixels(e, cfg)[2], box_pixels(e, cfg)[2]) >= 2 * PIX_MARGIN:
                    break
            extent[i] = [e[0], e[1], 1.5]
            if s == 0 and k < 3:                                     # the standing group
                p0, h0, v0, a, w = centres[s] + np.array([[0.0, 0.0], [1.5, 0.75], [3.5, 3.25]][k]), [0.0, 0.25, 0.5][k], 0.0, 0.0, 0.0
            elif s == 1 and k == 69:                                 # beside agent 68
                world[:, i] = world[:, ss[s] + 68] + np.array([0.5, 1.25, 0.0])
                nominal, h = world[:, i, :2].copy(), world[:, i, 2].copy()
                p0 = None
            else:
                p0 = centres[s] + rng.uniform(-28.0, 28.0, 2)
                h0, v0, a, w = rng.uniform(-np.pi, np.pi), rng.uniform(0.0, 10.0), rng.uniform(-2.0, 2.0), rng.uniform(-0.3, 0.3)
            if p0 is not None:
                h = np.float32(h0 + w * tt).astype(np.float64)
                dist = np.maximum(v0 * tt + 0.5 * a * tt * tt, 0.0)
                nominal = p0 + dist[:, None] * np.stack([np.cos(h0 + 0.5 * w * tt), np.sin(h0 + 0.5 * w * tt)], -1)
            world[:, i, 2] = h
            for t in range(T):
                for attempt in range(10000):
                    p = _q(nominal[t] + (rng.uniform(-1.0 / 16, 1.0 / 16, 2) if attempt else 0.0))
                    if scene_map[s] < 0 or map_flags(case, s, np.array([p[0], p[1], h[t]]), e)[2] >= 2 * PIX_MARGIN:
                        break
                else:
                    raise RuntimeError(f"guide_metrics_cases.build_case: step {t} of agent {k} of scene {s} did not settle")
                world[t, i, :2] = p
    world = world.astype(np.float32)
    world[list(ABSENT[1]), ss[0] + ABSENT[0], :2] = np.nan
    speed = _q(rng.uniform(0.0, 12.0, (T, B)), 6).astype(np.float32)
    acc = _q(rng.uniform(-3.0, 3.0, (T, B)), 6).astype(np.float32)
    config, constraint = configs(ss, rng, centres, world[0])
    case.update(world=world, speed=speed, acc=acc, extent=extent.astype(np.float32), config=config, constraint=constraint)
    r = restate(case)
    assert r["rel_margin"] >= REL_MARGIN, f"a comparison lies within {r['rel_margin']:.2e} relative of its threshold (change the seed)"
    assert r["pix_margin"] >= PIX_MARGIN, f"a sampled pixel lies within {r['pix_margin']:.2e} px of a rounding boundary (change the seed)"
    case["restated"] = r
    return case


def small_case():
    """One scene of three agents, six scored steps, no map: a waypoint member absent at its target time (NaN), a target_time beyond the
    episode (NaN; upstream raises an IndexError there), a minimum that skips NaN distances, and a NaN speed under target_speed (skipped
    by the nanmean) and speed_limit (kept by np.mean)."""
    T = 6
    world = np.zeros((T, 3, 3), np.float32)
    world[:, 0, 0], world[:, 0, 1], world[:, 0, 2] = _q(1.25 * np.arange(T)), 2.0, 0.125
    world[:, 1, 0], world[:, 1, 1], world[:, 1, 2] = 10.0, _q(-0.75 * np.arange(T)), -1.5
    world[:, 2, 0], world[:, 2, 1], world[:, 2, 2] = -20.0, 30.0, 2.0
    world[[2, 4], 1, :2] = np.nan
    speed = np.tile(np.array([3.0, 5.5, 1.25], np.float32), (T, 1)) + np.float32(0.25) * np.arange(T, dtype=np.float32)[:, None]
    speed[3, 0] = np.nan
    acc = np.tile(np.array([0.5, -2.0, 1.5], np.float32), (T, 1))
    ts = np.full((3, T), 4.0)
    config = [[
        dict(name="global_target_pos_at_time", weight=1.0, agents=[0, 1], params=dict(target_pos=[[4.0, 2.5], [10.0, -3.0]], target_time=[2, 3])),
        dict(name="target_pos_at_time", weight=1.0, agents=[2], params=dict(target_pos=[[1.0, 1.0]], target_time=[20])),
        dict(name="global_target_pos", weight=1.0, agents=[1], params=dict(target_pos=[[10.0, -1.5]])),
        dict(name="target_speed", weight=1.0, agents=[0, 2], params=dict(target_speed=ts)),
        dict(name="speed_limit", weight=1.0, agents=[0, 1], params=dict(speed_limit=4.0)),
        dict(name="acc_limit", weight=1.0, agents=None, params=dict(acc_limit=1.0)),
    ]]
    case = dict(world=world, speed=speed, acc=acc, extent=np.array([[4.0, 2.125, 1.5]] * 3, np.float32), scene_start=np.array([0, 3], np.int32),
                maps=None, scene_map=None, map_from_world=None, cfg=dict(CFG), config=config, constraint=None)
    case["restated"] = restate(case)
    return case


_CASES = {}


def case(name="main"):
    if name not in _CASES:
        _CASES[name] = build_case() if name == "main" else small_case()
    return _CASES[name]
