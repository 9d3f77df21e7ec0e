"""Yardstick of the lane guidance (tests/test_lane_host.py, tests/test_gpu_lane.py): a from-scratch restatement in float64 of upstream's
lane projection (get_lane_projection from the transform to the sort, src/tbsim/utils/trajdata_utils.py:573-664, and project_onto,
:726-821) and of LaneFollowingLoss, ChangeToLeftLaneLoss and FollowLaneLoss (src/tbsim/utils/guidance_loss.py:1574-1628, 1795-1841,
1958-2011), so that autograd gives the gradients in float64 on the CPU.  tests/golden/lane_guidance.npz, recorded from the
reference's own project_onto and classes (tests/tools/record_lane_golden.py), pins it.

A `term` here is a dict: agent, line (per entry an index), kind (per entry a name of KINDS), decay, scale (per entry, floats) and
lines [L,S,3]: agent-frame polylines (x, y, heading) sorted by x, NaN rows last.  Plans are [A,N,52,6].

Besides the losses it reports, per (entry, sample, step), the GAP of the projection: the distance to the nearest segment whose outcome
(projected point or heading) differs from the chosen one's, minus the chosen distance -- how far the argmin is from changing its
answer -- and the margins of the losses' kinks: |dx| + |dy| against the clip at 5, dx, dy and yaw - h against 0."""
import numpy as np
import torch

H = 52
KINDS = ("following", "change_left", "follow_decayed")
SAME = 1e-9         # two segments' outcomes count as one when their projected points agree to this and their headings are equal


def transform(world_lines, line_frame, agent_from_world):
    """numpy: world polylines [L,S,3] float64 -> agent-frame float32 polylines in the stored order.  x, y through the 3x3 matrix,
    heading' = atan2 of the rotated (cos h, sin h), all in float64, rounded once (this project's definition of trajdata's
    transform_xyh_np)."""
    wl = np.asarray(world_lines, np.float64)
    out = np.empty(wl.shape, np.float32)
    for l in range(wl.shape[0]):
        M = np.asarray(agent_from_world, np.float32)[int(line_frame[l])].astype(np.float64)
        x, y, h = wl[l, :, 0], wl[l, :, 1], wl[l, :, 2]
        c, s = np.cos(h), np.sin(h)
        out[l] = np.stack([M[0, 0] * x + M[0, 1] * y + M[0, 2], M[1, 0] * x + M[1, 1] * y + M[1, 2],
                           np.arctan2(M[1, 0] * c + M[1, 1] * s, M[0, 0] * c + M[0, 1] * s)], axis=1).astype(np.float32)
    return out


def sort_by_x(lines):
    """numpy [L,S,3] float32 -> the rows of every line sorted by (x, original index), NaN x last; -0 counts as +0."""
    out = np.empty_like(lines)
    for l in range(lines.shape[0]):
        key = lines[l, :, 0].copy()
        key[key == 0] = 0.0
        out[l] = lines[l][np.argsort(key, kind="stable")]
    return out


def prepare(world_lines, line_frame, agent_from_world):
    """What cld_lane_prepare computes: transform, then sort_by_x."""
    return sort_by_x(transform(world_lines, line_frame, agent_from_world))


def segments(line):
    """line [S,3] -> (p0 [S-1,2], d [S-1,2], heading of p0 [S-1], usable [S-1]: finite ends and a non-zero length)."""
    p0, p1 = line[:-1, :2], line[1:, :2]
    d = p1 - p0
    ok = torch.isfinite(p0).all(dim=1) & torch.isfinite(p1).all(dim=1) & ((d * d).sum(dim=1) > 0)
    return p0, d, line[:-1, 2], ok


def distances(xy, line):
    """xy [...,2] against every segment of line [S,3] -> (dist [...,S-1] (+inf where the segment is not usable), proj [...,S-1,2])."""
    p0, d, _, ok = segments(line)
    nn = (d * d).sum(dim=1)
    nn = torch.where(ok, nn, torch.ones_like(nn))
    dd = torch.where(ok[:, None], d, torch.zeros_like(d))
    pp = torch.where(ok[:, None], p0, torch.zeros_like(p0))
    u = torch.clip(((xy[..., None, :] - pp) * dd).sum(dim=-1) / nn, 0.0, 1.0)
    proj = pp + u[..., None] * dd
    dist = (xy[..., None, :] - proj).norm(dim=-1)
    return torch.where(ok, dist, torch.full_like(dist, float("inf"))), proj


def project(xy, line):
    """-> (projection [...,3] = (proj.x, proj.y, heading of the chosen segment's p0), chosen segment [...], gap [...])."""
    with torch.no_grad():
        dist, proj = distances(xy, line)
        head = segments(line)[2]
        best = dist.argmin(dim=-1)                                        # the first index among equals
        pb = torch.gather(proj, -2, best[..., None, None].expand(*best.shape, 1, 2)).squeeze(-2)
        db = torch.gather(dist, -1, best[..., None]).squeeze(-1)
        hb = head[best]
        differs = ((proj - pb[..., None, :]).abs().amax(dim=-1) > SAME) | (head != hb[..., None])
        other = torch.where(differs & torch.isfinite(dist), dist, torch.full_like(dist, float("inf")))
        gap = other.amin(dim=-1) - db
        return torch.cat([pb, hb[..., None]], dim=-1), best, gap


def candidates(xy, line, within):
    """The outcomes [..., S-1, 3] of all segments and the mask [..., S-1] of those whose distance is within `within` of the smallest."""
    with torch.no_grad():
        dist, proj = distances(xy, line)
        head = segments(line)[2]
        out = torch.cat([proj, head.expand(*proj.shape[:-1])[..., None]], dim=-1)
        return out, dist <= dist.amin(dim=-1, keepdim=True) + within


def _entry(traj, term, e):
    """-> (value [N], projection [N,52,3], gap [N,52], kink quantities [(tensor [N,52], bound)], clip active [N,52] | None)."""
    a, kind = int(term["agent"][e]), term["kind"][e]
    line = torch.as_tensor(term["lines"])[int(term["line"][e])].to(traj.dtype)
    xy, yaw = traj[a][..., :2], traj[a][..., 3]
    pr, _, gap = project(xy.detach(), line)
    dx, dy, dh = xy[..., 0] - pr[..., 0], xy[..., 1] - pr[..., 1], yaw - pr[..., 2]
    clip = None
    if kind == "following":
        e_t, kinks = dx * dx + dy * dy + dh * dh, []
    elif kind == "change_left":
        e_t, kinks = torch.stack([dx, dy], dim=-1).norm(dim=-1) + dh.abs(), [(torch.maximum(dx.abs(), dy.abs()), 0.0), (dh, 0.0)]
    else:
        m = dx.abs() + dy.abs()
        w = torch.tensor([float(term["decay"][e]) ** t for t in range(H)], dtype=traj.dtype)
        e_t, kinks, clip = torch.clip(m, max=5.0) * (w / w.sum()), [(m, 5.0), (dx, 0.0), (dy, 0.0)], m > 5.0
    return e_t.mean(dim=-1), pr, gap, kinks, clip


def values(traj, term):
    """The unweighted values [E,N]."""
    return torch.stack([_entry(traj, term, e)[0] for e in range(len(term["agent"]))])


def projections(traj, term):
    """-> (projections [E,N,52,3], gaps [E,N,52])."""
    rows = [_entry(traj, term, e) for e in range(len(term["agent"]))]
    return torch.stack([r[1] for r in rows]), torch.stack([r[2] for r in rows])


def total(traj, term):
    """sum over entries and samples of scale[e] * value: with scale = weight / (samples * targets) DiffuserGuidance's weight * mean."""
    tot = 0.0
    for e in range(len(term["agent"])):
        tot = tot + float(term["scale"][e]) * _entry(traj, term, e)[0].sum()
    return tot


def value_and_grad(traj, term):
    x = traj.clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(total(x, term), x)
    return values(traj, term).detach(), g


def margins(traj, term):
    """(smallest gap, smallest distance of a kink quantity from its kink) over all entries, samples and steps."""
    gap, kink = float("inf"), float("inf")
    with torch.no_grad():
        for e in range(len(term["agent"])):
            _, _, g, kinks, _ = _entry(traj, term, e)
            gap = min(gap, float(g.min()))
            for q, bound in kinks:
                kink = min(kink, float((q - bound).abs().min()))
    return gap, kink


def offenders(traj, term, gap_min, kink_min):
    """[(agent, sample, step)] whose gap or kink margin is below the bounds."""
    bad = set()
    with torch.no_grad():
        for e in range(len(term["agent"])):
            _, _, g, kinks, _ = _entry(traj, term, e)
            m = g < gap_min
            for q, bound in kinks:
                m = m | ((q - bound).abs() < kink_min)
            for n, t in torch.nonzero(m).tolist():
                bad.add((int(term["agent"][e]), n, t))
    return sorted(bad)


def clip_active(traj, term, e):
    """follow_decayed: per sample (active at some step, at every step)."""
    with torch.no_grad():
        c = _entry(traj, term, e)[4]
        return c.any(dim=-1), c.all(dim=-1)


def sgd_steps(wdec, mean, cond, cs, term, n_steps, lr, num_samp=1, extra=None):
    """n_steps plain SGD steps of the guided mean [A N,52,4] on total(decode(x)) (+ extra(traj)) -> (guided mean, gradient of the first
    step, the decoded plans [A,N,52,6] of every iterate the loss was evaluated on)."""
    from oracle import cld_oracle as O
    x, g_first, seen = mean.clone(), None, []
    for _ in range(n_steps):
        xk = x.clone().requires_grad_(True)
        with torch.enable_grad():
            traj = O.decode(wdec, xk, cond, cs, True)
            t4 = traj.reshape(-1, num_samp, H, 6)
            loss = total(t4, term)
            if extra is not None:
                loss = loss + extra(traj)
            (g,) = torch.autograd.grad(loss, xk)
        seen.append(t4.detach())
        g_first = g if g_first is None else g_first
        x = x - lr * g
    return x, g_first, seen


def term_from_meta(case, lines, N):
    """The yardstick term of one recorded case: `case` = meta['cases'][name] with a list `entries` of dicts (agent, line, kind, decay,
    weight, targets: how many entries share the config's weight)."""
    es = case["entries"]
    return dict(agent=[int(q["agent"]) for q in es], line=[int(q["line"]) for q in es], kind=[q["kind"] for q in es],
                decay=[float(q["decay"]) for q in es], scale=[float(q["weight"]) / (N * int(q["targets"])) for q in es],
                lines=torch.as_tensor(lines).double())
