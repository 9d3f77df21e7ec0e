"""A plain restatement of upstream's AgentCollisionLoss (src/tbsim/utils/guidance_loss.py:442-630) and of what DiffuserGuidance
(:2143-2172) makes of it, the yardstick of the agent-collision kernel (csrc/collision_kernels.hip): what
oracle.cld_oracle.agent_collision_loss and scene_collision_total compute, scene by scene and step by step, so that a 192-agent scene
needs the [A,A,D,D] table of ONE step (15 MB in float64 at D = 5) instead of the oracle's [T,N,B,B,D,D] one.

Every operation runs in the dtype of `plans`: on float64 plans this is the reference, on the same plans in float32 the calibration of
the bar (tests/grad_bar.py).  The gradient is written out, not taken by autograd (tests/test_collision_host.py holds it to the oracle's
autograd in both dtypes):
    value[i, n] = [moving_i] (1 / B) sum_t w_t sum_j pen_ij(t),   pen = 1 - d / pd where d <= pd = r_i + r_j + buffer_dist,
    total       = sum_s weight_s * mean over the scene's guided agents and the samples of value,
    d total / d pose_i = [act_i] weight_s / (M_s N B) sum_t w_t sum_j (1 + [act_j]) d pen_ij / d pose_i,   act = guided and moving,
with d the smallest distance between a disk centre of i and one of j -- the FIRST smallest in (a, c) order, as torch.min and the kernel
take it -- and d pen / d c_i = -(c_i - c_j) / (d pd) applied at c_i = p_i + cx_a (cos, sin)(heading_i).

With record=True (float64) it also says which (agent, sample, step) elements of the gradient hang on a decision that rounding can take
either way, and the interval the admissible alternatives span there (FLAG RULE below), and returns every penalised pair.

`mutant`: the yardstick with one plausible kernel error built in (MUTANTS); tests/test_collision_host.py shows that the cases tell each
from the yardstick.
"""
import torch

T = 52
KINK = 1e-4            # |d - pd| <= KINK pd: the pair may count or not
TIE = 1e-4             # the two smallest disk distances within TIE (relative): rounding decides which disk pair is the first minimum
NEAR = 0.05            # d < NEAR metres: the direction (c_i - c_j) / d is ill-conditioned
MUTANTS = ("signed_reach", "last_minimum", "no_partner_factor", "decay_not_normalised", "lever_of_the_other", "no_heading_jacobian")


def disk_centres(extent, num_disks):
    """[B,D] positions of the disk centres along the agent's axis, as init_disks builds them (:481-492): a linspace per agent."""
    rad = extent[:, 1] / 2.0
    cmin, cmax = -(extent[:, 0] / 2.0) + rad, (extent[:, 0] / 2.0) - rad
    return torch.stack([torch.linspace(float(cmin[b]), float(cmax[b]), num_disks, dtype=extent.dtype) for b in range(extent.shape[0])])


def step_weights(decay_rate, dtype, normalised=True):
    w = torch.tensor([decay_rate ** t for t in range(T)], dtype=dtype)
    return w / w.sum() if normalised else w


def scene_masks(term, B):
    """-> per scene (first agent, size, weight, guided [A] bool), and excluded [B] bool."""
    ex = torch.zeros(B, dtype=torch.bool)
    if term.get("excluded_agents") is not None:
        ex[torch.as_tensor(list(term["excluded_agents"]), dtype=torch.long)] = True
    out, a0 = [], 0
    wts = term["weight"] if isinstance(term["weight"], (list, tuple)) else [term["weight"]] * len(term["sizes"])
    for s, A in enumerate(term["sizes"]):
        g = torch.zeros(A, dtype=torch.bool)
        if float(wts[s]) != 0.0:
            sub = (term.get("agents") or {}).get(s)
            if sub is None:
                g[:] = True
            else:
                g[torch.as_tensor(list(sub), dtype=torch.long)] = True
        out.append((a0, A, float(wts[s]), g))
        a0 += A
    assert a0 == B
    return out, ex


def run(plans, term, record=False, mutant=None):
    """plans [B,N,52,6] (float32 or float64), term: extent [B,3], world_from_agent [B,3,3], curr_speed [B], sizes, weight (scalar or
    per scene), agents {scene: local indices} | None, excluded_agents | None, num_disks, buffer_dist, decay_rate,
    guide_moving_speed_th.  -> dict(values [B,N], grad [B N,52,6]); with record=True also
        carrying [B,N,52]  the element receives a gradient: its agent is guided and moving and some pair of it is penalised,
        flagged  [B,N,52]  FLAG RULE: some pair of the element with d <= (1 + KINK) pd has |d - pd| <= KINK pd, or its two smallest disk
                           distances within TIE (relative), or d < NEAR,
        lo, hi   [B,N,52,3] the interval of d total / d (x, y, yaw): per pair the componentwise min / max over the admissible
                           alternatives -- every disk pair within TIE of the minimum; the pair on or off at a kink; any direction at
                           the pair's magnitude below NEAR -- summed over the pairs (lo == hi == the gradient on unflagged elements),
        pairs    dict of [K] tensors over the penalised (i, j, n, t), gradient-carrying or not: i, j, n, t, d1, d2 (the second smallest
                           over the disk pairs that are other points than the first minimum's; inf where there is none),
                           pd, centre (distance of the agents' centres), ei, ej (the signed half extents of the disk centres),
        ties     {(i, j, n, t): [m,3]} the alternatives of every flagged pair, in d total / d (x, y, yaw) of the plan,
        nearest_outside    the smallest d - pd over the pairs that are NOT penalised (metres)."""
    assert mutant is None or mutant in MUTANTS
    dt = plans.dtype
    B, N = plans.shape[:2]
    D = int(term.get("num_disks", 5))
    ext, W, spd = term["extent"].to(dt), term["world_from_agent"].to(dt), term["curr_speed"].to(dt)
    rad = ext[:, 1] / 2.0
    half = ext[:, 0] / 2.0 - rad
    cx_all = disk_centres(ext, D)
    moving_all = spd.abs() > float(term.get("guide_moving_speed_th", 0.5))
    w = step_weights(float(term.get("decay_rate", 0.9)), dt, mutant != "decay_not_normalised")
    buf = float(term.get("buffer_dist", 0.2))
    scenes, ex_all = scene_masks(term, B)
    values = torch.zeros(B, N, dtype=dt)
    grad = torch.zeros(B, N, T, 6, dtype=dt)
    if record:
        carrying, flagged = torch.zeros(B, N, T, dtype=torch.bool), torch.zeros(B, N, T, dtype=torch.bool)
        keys = ("i", "j", "n", "t", "d1", "d2", "pd", "centre", "ei", "ej")
        rec = {k: [] for k in keys}
        ties, widen, nearest_outside = {}, [], float("inf")
    for a0, A, wgt, guided in scenes:
        sl = slice(a0, a0 + A)
        R, tr, cx, r, hf = W[sl, :2, :2], W[sl, :2, 2], cx_all[sl], rad[sl], half[sl]
        moving, ex = moving_all[sl], ex_all[sl]
        act = guided & moving
        M = int(guided.sum())
        coef = wgt / (M * N * B) if M > 0 else 0.0
        pd = r[:, None] + r[None, :] + buf
        allowed = ~torch.eye(A, dtype=torch.bool) & ~(ex[:, None] & ex[None, :])
        fac = torch.ones(A, A, dtype=dt) if mutant == "no_partner_factor" else (1.0 + act.to(dt))[None, :].expand(A, A)
        ar = torch.arange(A)
        for n in range(N):
            acc = torch.zeros(A, dtype=dt)
            for t in range(T):
                x = plans[sl, n, t]
                pos = (R @ x[:, :2, None]).squeeze(-1) + tr
                cy, sy = torch.cos(x[:, 3]), torch.sin(x[:, 3])
                h = (R @ torch.stack([cy, sy], dim=-1)[..., None]).squeeze(-1)
                dh = (R @ torch.stack([-sy, cy], dim=-1)[..., None]).squeeze(-1)
                yw = torch.atan2(h[:, 1], h[:, 0])
                u = torch.stack([torch.cos(yw), torch.sin(yw)], dim=-1)                      # [A,2]
                dyaw = torch.ones(A, dtype=dt) if mutant == "no_heading_jacobian" else (h[:, 0] * dh[:, 1] - h[:, 1] * dh[:, 0]) / (h * h).sum(-1)
                cent = pos[:, None, :] + cx[:, :, None] * u[:, None, :]                       # [A,D,2]
                e = (cent[:, None, :, None, :] - cent[None, :, None, :, :]).reshape(A, A, D * D, 2)      # [i,j,(a,c)]
                d = e.norm(dim=-1)
                d1 = d.min(dim=-1)[0]
                same = d == d1[..., None]
                k1 = (D * D - 1 - same.flip(-1).int().argmax(dim=-1)) if mutant == "last_minimum" else same.int().argmax(dim=-1)
                ok = allowed & (d1 <= pd)
                if mutant == "signed_reach":
                    reach = pd + hf[:, None] + hf[None, :] + 1e-3
                    ok = ok & ~(((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1) > reach * reach)
                acc = acc + w[t] * torch.where(ok, 1.0 - d1 / pd, torch.zeros_like(d1)).sum(dim=1)
                eb = e[ar[:, None], ar[None, :], k1]                                          # [A,A,2]
                lever = cx[ar[None, :].expand(A, A), k1 % D] if mutant == "lever_of_the_other" else cx[ar[:, None].expand(A, A), k1 // D]
                live = ok & (d1 > 0)
                k = torch.where(live, -fac / (torch.where(live, d1, torch.ones_like(d1)) * pd), torch.zeros_like(d1))
                gc = k[..., None] * eb
                gyw = lever * (-u[:, None, 1] * gc[..., 0] + u[:, None, 0] * gc[..., 1])
                gpos, gyaw = gc.sum(dim=1), gyw.sum(dim=1)
                sc = coef * w[t] * act.to(dt)
                grad[sl, n, t, :2] = sc[:, None] * (R.transpose(1, 2) @ gpos[..., None]).squeeze(-1)
                grad[sl, n, t, 3] = sc * gyaw * dyaw
                if not record:
                    continue
                carrying[sl, n, t] = act & ok.any(dim=1)
                # the second smallest distance, over the disk pairs that are other POINTS than the first minimum's (the disks of a
                # square agent all sit on its centre: the same point under five names is no tie)
                qa, qc = torch.arange(D * D) // D, torch.arange(D * D) % D
                other = (cx[:, qa][:, None, :] != cx[ar[:, None].expand(A, A), k1 // D][..., None]) | (cx[:, qc][None, :, :] != cx[ar[None, :].expand(A, A), k1 % D][..., None])
                d2 = torch.where(other, d, torch.full_like(d, float("inf"))).min(dim=-1)[0]
                centre = (pos[:, None, :] - pos[None, :, :]).norm(dim=-1)
                pi, pj = torch.nonzero(ok, as_tuple=True)
                for key, v in (("i", pi + a0), ("j", pj + a0), ("n", torch.full_like(pi, n)), ("t", torch.full_like(pi, t)), ("d1", d1[pi, pj]), ("d2", d2[pi, pj]),
                               ("pd", pd[pi, pj]), ("centre", centre[pi, pj]), ("ei", hf[pi]), ("ej", hf[pj])):
                    rec[key].append(v)
                beyond = allowed & (d1 > pd)
                if bool(beyond.any()):
                    nearest_outside = min(nearest_outside, float((d1 - pd)[beyond].min()))
                near_pd = (d1 - pd).abs() <= KINK * pd
                odd = allowed & act[:, None] & (d1 <= (1.0 + KINK) * pd) & (near_pd | (d2 - d1 <= TIE * d1) | (d1 < NEAR))
                for i, j in zip(*[v.tolist() for v in torch.nonzero(odd, as_tuple=True)]):
                    flagged[a0 + i, n, t] = True

                    def plan_grad(gx, gy, arm):
                        gp = R[i].T @ torch.stack([gx, gy])
                        return torch.stack([gp[0], gp[1], arm * (-u[i, 1] * gx + u[i, 0] * gy) * dyaw[i]]) * sc[i]
                    base = plan_grad(gc[i, j, 0], gc[i, j, 1], lever[i, j])
                    alts = [base]
                    for q in torch.nonzero(d[i, j] <= d1[i, j] * (1.0 + TIE)).reshape(-1).tolist():
                        if d[i, j, q] > 0:
                            kq = -fac[i, j] / (d[i, j, q] * pd[i, j])
                            alts.append(plan_grad(kq * e[i, j, q, 0], kq * e[i, j, q, 1], cx[i, q // D]))
                    if bool(near_pd[i, j]):
                        alts.append(torch.zeros(3, dtype=dt))
                    if bool(d1[i, j] < NEAR):
                        mag = float(fac[i, j] / pd[i, j] * sc[i])
                        box = torch.tensor([mag, mag, float(hf[i].abs() * dyaw[i].abs()) * mag], dtype=dt)
                        alts += [box, -box]
                    alts = torch.stack(alts)
                    ties[(a0 + i, a0 + j, n, t)] = alts
                    widen.append((a0 + i, n, t, alts.min(dim=0)[0] - base, alts.max(dim=0)[0] - base))
            values[sl, n] = torch.where(moving, acc / B, torch.zeros_like(acc))
    out = dict(values=values, grad=grad.reshape(B * N, T, 6))
    if record:
        lo, hi = grad[..., [0, 1, 3]].clone(), grad[..., [0, 1, 3]].clone()
        for b, n, t, dlo, dhi in widen:
            lo[b, n, t] += dlo
            hi[b, n, t] += dhi
        pairs = {k: (torch.cat(v) if v else torch.zeros(0)) for k, v in rec.items()}
        out.update(carrying=carrying, flagged=flagged, lo=lo, hi=hi, pairs=pairs, ties=ties, nearest_outside=nearest_outside)
    return out


def total(values, term):
    """The DiffuserGuidance total of per-agent values [B,N]: sum over scenes of weight * mean over the guided agents and samples."""
    scenes, _ = scene_masks(term, values.shape[0])
    tot = values.sum() * 0.0
    for a0, A, wgt, guided in scenes:
        if guided.any():
            tot = tot + wgt * values[a0:a0 + A][guided].mean()
    return tot
