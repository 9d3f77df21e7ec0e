"""Yardstick of the social-group guidance (tests/test_social_host.py, tests/test_gpu_social.py): a from-scratch restatement in torch
of upstream's SocialGroupLoss (src/tbsim/utils/guidance_loss.py:1137-1207) and of the weighted total DiffuserGuidance builds from it
(:2143-2173), with the random draws as inputs, so that autograd gives the gradients in float64 on the CPU; `sgd_steps` is the guided
step written out over oracle.cld_oracle.decode.  tests/golden/social_group.npz, recorded from the reference's own class
(tests/tools/record_social_golden.py), pins it.

A `term` here is a dict: groups (one list of agent indices per group, ascending), leader (per group an agent index or -1),
social_dist, cohesion, scale (per group, floats), world_from_agent [A,3,3].  Plans are [A,N,52,6]; the draws of one evaluation are
r (integers) and u (float32), both [A,N,52] -- entries of non-members are ignored.
"""
import torch

H = 52


MUTANTS = ("last_minimum", "cohesion_le", "draw_hits_self", "leader_receives", "leader_term_lost", "own_term_only", "world_difference",
           "small_group_off")


def _group(traj, term, g, r, u, mutant=None):
    """-> (value [M,N], nearest and second-nearest distance where the nearest neighbour is used [..] | None, distances read [M,N,52]).
    `mutant`: the yardstick with one plausible kernel error built in (MUTANTS; tests/test_social_cases_host.py shows that the cases
    of tests/social_cases.py tell each from the yardstick):
      last_minimum      the LAST of several equidistant nearest neighbours
      cohesion_le       the draw is used where u <= cohesion
      draw_hits_self    the drawn neighbour is r itself, not r stepped over the member's own index
      leader_receives   the leader's position is not detached
      leader_term_lost  the leader's own term gives its neighbour nothing
      own_term_only     a member receives the gradient of its own term only (no gather over the members it is the neighbour of)
      world_difference  every operation in float32 on the scene where it stands (value_and_grad)
      small_group_off   the gradient of a group of two is 1 % too large (value_and_grad)"""
    idx = torch.as_tensor(term["groups"][g], dtype=torch.long)
    M = idx.numel()
    W = term["world_from_agent"].to(traj.dtype)[idx]
    p = torch.einsum("mij,mntj->mnti", W[:, :2, :2], traj[idx][..., :2]) + W[:, None, None, :2, 2]          # [M,N,52,2] world
    lead = idx == int(term["leader"][g])
    if mutant != "leader_receives":
        p = torch.where(lead[:, None, None, None], p.detach(), p)          # the leader's position is detached (:1168-1171)
    with torch.no_grad():
        dm = (p[:, None] - p[None, :]).norm(dim=-1)                         # [i,j,N,52]
        dm = dm + torch.diag(torch.full((M,), float("inf"), dtype=traj.dtype))[:, :, None, None]
        near, min_nb = dm.min(dim=1)
        if mutant == "last_minimum":
            min_nb = M - 1 - dm.flip(1).min(dim=1)[1]
        second = dm.scatter(1, min_nb[:, None], float("inf")).min(dim=1)[0] if M > 2 else torch.full_like(near, float("inf"))
    ri = r[idx].long()
    ar = torch.arange(M)[:, None, None]
    rand_nb = ri + 0 * ar if mutant == "draw_hits_self" else torch.where(ri < ar, ri, ri + 1)
    coh = torch.tensor(float(term["cohesion"][g]), dtype=torch.float32)
    drop = u[idx].float() <= coh if mutant == "cohesion_le" else u[idx].float() < coh           # compared in fp32, as upstream's tensors are
    nb = torch.where(drop, rand_nb, min_nb)
    pn = torch.gather(p, 0, nb[..., None].expand(-1, -1, -1, 2))
    if mutant == "own_term_only":
        pn = pn.detach()
    elif mutant == "leader_term_lost":
        pn = torch.where(lead[:, None, None, None], pn.detach(), pn)
    d = (p - pn).norm(dim=-1)
    value = ((d - float(term["social_dist"][g])) ** 2).mean(dim=-1)
    gap = (second - near)[~drop]
    return value, gap, d.detach()


def values(traj, term, r, u, mutant=None):
    """The unweighted per-(agent, sample) values [A,N] as upstream files them under guide_losses (0 outside the groups)."""
    out = traj[:, :, 0, 0] * 0.0
    for g in range(len(term["groups"])):
        v, _, _ = _group(traj, term, g, r, u, mutant)
        out = out.index_add(0, torch.as_tensor(term["groups"][g], dtype=torch.long), v)
    return out


def total(traj, term, r, u, mutant=None):
    """sum over groups of scale[g] * sum over member rows of the value: with scale = weight / (members x samples) this is
    DiffuserGuidance's weight * mean(loss of the config's agents)."""
    tot = 0.0
    for g in range(len(term["groups"])):
        tot = tot + float(term["scale"][g]) * _group(traj, term, g, r, u, mutant)[0].sum()
    return tot


def value_and_grad(traj, term, r, u, mutant=None):
    assert mutant is None or mutant in MUTANTS
    if mutant == "world_difference":
        v, g = value_and_grad(traj.float(), term, r, u)
        return v.to(traj.dtype), g.to(traj.dtype)
    x = traj.clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(total(x, term, r, u, mutant), x)
    if mutant == "small_group_off":
        for grp in term["groups"]:
            if len(grp) == 2:
                g[grp] = g[grp] * 1.01
    return values(traj, term, r, u, mutant).detach(), g


def margins(traj, term, r, u):
    """(smallest lead of the nearest neighbour over the second-nearest where the nearest is used, smallest distance read, smallest
    |u - cohesion| over the members' draws): what keeps a float32 evaluation on the same side of every decision."""
    gap, dmin, umin = float("inf"), float("inf"), float("inf")
    for g in range(len(term["groups"])):
        _, gp, d = _group(traj, term, g, r, u)
        if gp.numel():
            gap = min(gap, float(gp.min()))
        dmin = min(dmin, float(d.min()))
        idx = torch.as_tensor(term["groups"][g], dtype=torch.long)
        umin = min(umin, float((u[idx].double() - float(torch.tensor(float(term["cohesion"][g]), dtype=torch.float32))).abs().min()))
    return gap, dmin, umin


def sgd_steps(wdec, mean, cond, cs, term, draws, lr, num_samp=1, extra=None):
    """len(draws) plain SGD steps of the guided mean [A N,52,4] on total(decode(x)) (+ extra(traj), another loss on the decoded plans
    [A N,52,6]); draws = [(r, u)] per step, each [A N,52] in plan rows -> (guided mean, gradient of the first step, the decoded
    plans [A,N,52,6] of every iterate the loss was evaluated on)."""
    from oracle import cld_oracle as O
    x, g_first, seen = mean.clone(), None, []
    for r, u in draws:
        xk = x.clone().requires_grad_(True)
        with torch.enable_grad():
            traj = O.decode(wdec, xk, cond, cs, True)
            t4 = traj.reshape(-1, num_samp, H, 6)
            loss = total(t4, term, r.reshape(-1, num_samp, H), u.reshape(-1, num_samp, H))
            if extra is not None:
                loss = loss + extra(traj)
            (g,) = torch.autograd.grad(loss, xk)
        seen.append(t4.detach())
        g_first = g if g_first is None else g_first
        x = x - lr * g
    return x, g_first, seen


def term_from_meta(case, world_from_agent, N):
    """The yardstick term of one recorded case: `case` = meta['cases'][name] with agents, leader_idx, social_dist, cohesion, weight."""
    M = len(case["agents"])
    return dict(groups=[list(case["agents"])], leader=[int(case["leader_idx"])], social_dist=[float(case["social_dist"])],
                cohesion=[float(case["cohesion"])], scale=[float(case["weight"]) / (M * N)], world_from_agent=torch.as_tensor(world_from_agent).double())
