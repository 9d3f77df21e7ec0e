"""Yardstick of the global waypoint guidance (tests/test_goal_host.py, tests/test_gpu_goal.py): a from-scratch restatement in torch
of upstream's GlobalTargetPosLoss / GlobalTargetPosAtTimeLoss (src/tbsim/utils/guidance_loss.py:876-1135), of their have_reached_mask
update and of the weighted total DiffuserGuidance builds from them (:2143-2172), so that autograd gives the gradients in float64 on
the CPU; `sgd_step` is the guided step written out over oracle.cld_oracle.decode.  tests/golden/global_goal.npz, recorded from the
reference's own classes (tests/tools/record_goal_golden.py), pins it.

A `goal` here is a dict of per-AGENT tensors: kind [A] (0 off, 1 global_target_pos, 2 global_target_pos_at_time), target_pos [A,2]
(world), target_time [A], urgency [A], pref_speed [A], scale [A], agent_from_world [A,3,3], reached [A] bool | None, and the scalars
global_t, dt, min_progress_dist.  Plans are [A,N,52,6].
"""
import numpy as np
import torch
import torch.nn.functional as F

H = 52


def local_target(goal):
    """target_pos taken into the agent frame (GeoUtils.transform_points_tensor: p R^T + t) -> [A,2]."""
    M = goal["agent_from_world"].to(goal["target_pos"].dtype)
    return torch.einsum("aij,aj->ai", M[:, :2, :2], goal["target_pos"]) + M[:, :2, 2]


def branches(goal):
    """Per agent the branch the value takes: 'off', 'reached', 'exact', 'progress', 'passed', 'at_time', 'on_time'."""
    p = local_target(goal)
    out = []
    for a in range(p.shape[0]):
        k = int(goal["kind"][a])
        if k == 0:
            out.append("off")
        elif goal.get("reached") is not None and bool(goal["reached"][a]):
            out.append("reached")
        elif k == 1:
            out.append("exact" if float(p[a].norm()) < float(H * goal["dt"] * goal["pref_speed"][a]) else "progress")
        else:
            lt = int(goal["target_time"][a]) - int(goal["global_t"])
            out.append("passed" if lt < 0 else ("at_time" if lt < H else "on_time"))
    return out


def _relu_arg(br, d, goal, a):
    """The argument of the relu of the two progress branches for agent a: d [N,52] -> [N]."""
    ps, u = goal["pref_speed"][a], goal["urgency"][a]
    if br == "progress":
        goal_dist = torch.maximum(u * (H * goal["dt"] * ps), torch.as_tensor(goal["min_progress_dist"], dtype=d.dtype))
        return goal_dist - (d[:, 0] - d[:, -1])
    lt = int(goal["target_time"][a]) - int(goal["global_t"])
    return d[:, -1] - lt * goal["dt"] * ps * (1.0 - u)


def values(traj, goal):
    """The unweighted per-(agent, sample) values [A,N] as upstream files them under guide_losses (0 where the term is off)."""
    p = local_target(goal).to(traj.dtype)
    br = branches(goal)
    out = []
    for a in range(traj.shape[0]):
        e = traj[a, :, :, :2] - p[a]
        d = e.norm(dim=-1)                                              # [N,52]
        if br[a] in ("off", "reached", "passed"):
            out.append(traj[a, :, 0, 0] * 0.0)
        elif br[a] == "exact":                                          # TargetPosLoss, min_target_time = 0 (:693-712)
            out.append((F.softmin(d, dim=-1) * (e ** 2).sum(dim=-1)).mean(dim=-1))
        elif br[a] == "at_time":                                        # TargetPosAtTimeLoss (:654-670)
            out.append(d[:, int(goal["target_time"][a]) - int(goal["global_t"])])
        else:                                                           # compute_progress_loss (:876-928)
            out.append(F.relu(_relu_arg(br[a], d, goal, a)))
    return torch.stack(out)


def total(traj, goal):
    """sum_a scale[a] sum_n value[a,n]: with scale = weight / (agents of the config x samples) this is DiffuserGuidance's
    sum over configs of weight * mean(loss of the config's agents)."""
    return (values(traj, goal) * goal["scale"].to(traj.dtype)[:, None]).sum()


def value_and_grad(traj, goal):
    x = traj.clone().requires_grad_(True)
    with torch.enable_grad():
        v = values(x, goal)
        (g,) = torch.autograd.grad((v * goal["scale"].to(x.dtype)[:, None]).sum(), x)
    return v.detach(), g


def margins(traj, goal):
    """(distance of the nearest row to a kink of the value in metres, smallest d_t any value reads): the kinks are the relu arguments
    and the exact / progress boundary |p| = H dt pref_speed."""
    p = local_target(goal).to(traj.dtype)
    br = branches(goal)
    kink, dmin = float("inf"), float("inf")
    for a in range(traj.shape[0]):
        if br[a] in ("off", "reached", "passed"):
            continue
        d = (traj[a, :, :, :2] - p[a]).norm(dim=-1)
        if int(goal["kind"][a]) == 1:
            kink = min(kink, abs(float(p[a].norm()) - float(H * goal["dt"] * goal["pref_speed"][a])))
        if br[a] == "exact":
            dmin = min(dmin, float(d.min()))
        elif br[a] == "at_time":
            dmin = min(dmin, float(d[:, int(goal["target_time"][a]) - int(goal["global_t"])].min()))
        else:
            kink = min(kink, float(_relu_arg(br[a], d, goal, a).abs().min()))
            dmin = min(dmin, float(d[:, -1].min()) if br[a] == "on_time" else float(d[:, [0, -1]].min()))
    return kink, dmin


def reached_update(reached, target_pos, world_from_agent, agent_hist, tolerance, action_num=5, by="any"):
    """have_reached_mask after one forward of a config on its agents (:1019-1029, :1122-1133): target_pos [M,2], world_from_agent
    [M,3,3], agent_hist [M,Th,>=2] (agent frame), reached [M] bool.  by="any" is the reference as written: of the last action_num
    history points only the FIRST is kept after the transform, and the [M,2] - [M,1,2] broadcast makes agent i's distance the minimum
    over the points of ALL M agents.  by="own": the agent's own last action_num points (the evident intent).
    -> (new mask [M], |distance - tolerance| of the nearest decision)."""
    reached = reached.clone()
    if tolerance is None:
        return reached, float("inf")
    W = world_from_agent.to(target_pos.dtype)
    hist = agent_hist[:, -action_num:, :2].to(target_pos.dtype)
    hw = torch.einsum("mij,mtj->mti", W[:, :2, :2], hist) + W[:, None, :2, 2]        # [M,action_num,2] world
    if by == "any":
        dist = (hw[:, 0][None, :, :] - target_pos[:, None, :]).norm(dim=-1).min(dim=-1)[0]      # [i,j] = |hist_j - target_i|
    elif by == "own":
        dist = (hw - target_pos[:, None, :]).norm(dim=-1).min(dim=-1)[0]
    else:
        raise ValueError(f"goal_reached_by={by!r} (any | own)")
    reached |= dist < tolerance
    return reached, float((dist - tolerance).abs().min())


def invert_frames(world_from_agent):
    """agent_from_world [A,3,3] of rigid world_from_agent frames, in float64."""
    return torch.linalg.inv(torch.as_tensor(world_from_agent).double())


def move_frames(world_from_agent, dxy, dth):
    """world_from_agent composed with a per-agent motion (dxy [A,2] in the agent frame, dth [A]) -> the moved frames, float64."""
    W = torch.as_tensor(world_from_agent).double()
    A = W.shape[0]
    L = torch.zeros(A, 3, 3, dtype=torch.float64)
    dth, dxy = torch.as_tensor(dth).double(), torch.as_tensor(dxy).double()
    L[:, 0, 0] = torch.cos(dth); L[:, 0, 1] = -torch.sin(dth); L[:, 1, 0] = torch.sin(dth); L[:, 1, 1] = torch.cos(dth)
    L[:, :2, 2] = dxy; L[:, 2, 2] = 1.0
    return W @ L


def sgd_step(wdec, mean, cond, cs, goal, lr, grad_steps=1, num_samp=1, extra=None):
    """grad_steps plain SGD steps of the guided mean [A N,52,4] on total(decode(x)) (+ extra(traj), another loss on the decoded
    plans [A N,52,6]) -> (guided mean, gradient of the first step)."""
    from oracle import cld_oracle as O
    x, g_first = mean.clone(), None
    for _ in range(grad_steps):
        xk = x.clone().requires_grad_(True)
        with torch.enable_grad():
            traj = O.decode(wdec, xk, cond, cs, True)
            loss = total(traj.reshape(-1, num_samp, H, 6), goal)
            if extra is not None:
                loss = loss + extra(traj)
            (g,) = torch.autograd.grad(loss, xk)
        g_first = g if g_first is None else g_first
        x = x - lr * g
    return x, g_first


def to64(goal):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in goal.items()}


def goal_from_meta(case, arrays, prefix, A, N):
    """The per-agent goal dict (float64) of one recorded case: `case` = meta['cases'][name] with name, agents (subset | None), weight,
    target_pos, target_time | None, urgency, pref_speed, dt, min_progress_dist, global_t; frames and flags from the arrays."""
    idx = list(range(A)) if case["agents"] is None else list(case["agents"])
    M = len(idx)
    g = dict(kind=torch.zeros(A, dtype=torch.int32), target_pos=torch.zeros(A, 2, dtype=torch.float64), target_time=torch.zeros(A, dtype=torch.int32),
             urgency=torch.zeros(A, dtype=torch.float64), pref_speed=torch.ones(A, dtype=torch.float64), scale=torch.zeros(A, dtype=torch.float64),
             reached=torch.zeros(A, dtype=torch.bool), global_t=int(case["global_t"]), dt=float(case["dt"]),
             min_progress_dist=float(case.get("min_progress_dist", 0.5)))
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).double()       # the reference holds its parameters in float32
    g["kind"][idx] = 1 if case["name"] == "global_target_pos" else 2
    g["target_pos"][idx] = f32(case["target_pos"])
    if case.get("target_time") is not None:
        g["target_time"][idx] = torch.tensor(case["target_time"], dtype=torch.int32)
    g["urgency"][idx] = f32(case["urgency"])
    g["pref_speed"][idx] = f32(case["pref_speed"])
    g["scale"][idx] = float(case["weight"]) / (M * N)
    g["agent_from_world"] = torch.from_numpy(arrays[prefix + "agent_from_world"]).double()
    return g, idx
