"""Yardstick of the pair-relation guidance (tests/test_pair_host.py, tests/test_gpu_pair.py): a from-scratch restatement in torch of
upstream's KeepDistanceLoss, CollisionLoss, KeepDistanceLoss2 / StayAwayLoss, FrontCollisionLoss and CollideLeftSideLoss
(src/tbsim/utils/guidance_loss.py:1631-1791, 1844-1956, 2014-2082) and of the weighted total DiffuserGuidance builds from them
(:2143-2173), so that autograd gives the gradients in float64 on the CPU; `sgd_steps` is the guided step written out over
oracle.cld_oracle.decode.  tests/golden/pair_guidance.npz, recorded from the reference's own classes
(tests/tools/record_pair_golden.py), pins it.

A `term` here is a dict: target, ref (per pair an agent index), kind (per pair a name of KINDS), lo, hi, decay, scale (per pair,
floats), world_from_agent [A,3,3] and agent_from_world [A,3,3] or None (the inverse of the former).  Plans are [A,N,52,6].

`mutant`: the yardstick with one plausible kernel error built in (MUTANTS); tests/test_pair_cases_host.py shows that the cases of
tests/pair_cases.py tell each from the yardstick.
  world_difference             every operation in float32 on the scene where it stands (no difference of frame origins formed first)
  clip_strict                  clip(min=0) passes only where its argument is > 0
  abs_one_at_zero              abs has gradient 1 at 0
  decay_not_normalised         decay^t, not decay^t / sum_t decay^t
  decay_not_averaged           the weighted SUM over the steps of a decayed relation, not its mean
  stale_decay                  in an agent's gradient gather a pair takes the step weights of the agent's PREVIOUS incidence
  late_steps_off               the step weights of a decaying relation (0 < decay < 1) are 2 % too large from step 40 on
  ref_gets_nothing             the ref agent's position is detached
  ref_rotated_by_target        the ref agent's gradient is rotated back by the TARGET's R^T
  frame_inverse_not_transpose  d e / d q is taken to the world by M^-1, not M^T
  small_agent_off              the gradient rows of an agent that sits in exactly one pair are 1 % too large
"""
import torch

H = 52
KINDS = ("keep_distance", "collision", "stay_away", "front_collision", "collide_left")
MUTANTS = ("world_difference", "clip_strict", "abs_one_at_zero", "decay_not_normalised", "decay_not_averaged", "stale_decay", "late_steps_off",
           "ref_gets_nothing", "ref_rotated_by_target", "frame_inverse_not_transpose", "small_agent_off")


def invert_frames(W):
    """Inverse of 2-D rigid frames [A,3,3]."""
    R = W[:, :2, :2].transpose(1, 2)
    out = torch.zeros_like(W)
    out[:, :2, :2] = R
    out[:, :2, 2] = -torch.einsum("aij,aj->ai", R, W[:, :2, 2])
    out[:, 2, 2] = 1.0
    return out


def _frames(term, dtype):
    W = term["world_from_agent"].to(dtype)
    F = term.get("agent_from_world")
    return W, (invert_frames(W) if F is None else F.to(dtype))


def _forward_as(value, through):
    """`value` with the gradient of `through` (a mutant's backward rule under the yardstick's forward)."""
    return value.detach() + (through - through.detach())


def _pair(traj, term, p, mutant=None, decay=None):
    """-> (value [N], the per-step quantities that sit next to a kink [(name, tensor [N,52], bound)], distance read [N,52] | None);
    `decay`: the decay the step weights are built from, where it is not the pair's own (mutant stale_decay)."""
    i, j, kind = int(term["target"][p]), int(term["ref"][p]), term["kind"][p]
    lo, hi = float(term["lo"][p]), float(term["hi"][p])
    decay = float(term["decay"][p]) if decay is None else float(decay)
    W, F = _frames(term, traj.dtype)
    world = lambda a: torch.einsum("ij,ntj->nti", W[a, :2, :2], traj[a][..., :2]) + W[a, :2, 2]
    pi, pj = world(i), world(j)
    if mutant == "ref_gets_nothing":
        pj = pj.detach()
    elif mutant == "ref_rotated_by_target":
        xj = traj[j][..., :2]
        pj = _forward_as(pj, torch.einsum("ij,ntj->nti", W[i, :2, :2], xj))
    clip0 = (lambda x: torch.where(x > 0, x, torch.zeros_like(x))) if mutant == "clip_strict" else (lambda x: torch.clip(x, min=0))
    abs0 = (lambda x: torch.where(x >= 0, x, -x)) if mutant == "abs_one_at_zero" else torch.abs
    if kind == "collision":                                               # the world distance (:1724)
        d = (pi - pj).norm(dim=-1)
        e, kinks, dist = clip0(d - lo), [(d, lo)], d
    else:
        inref = lambda q: torch.einsum("ij,ntj->nti", F[j, :2, :2], q) + F[j, :2, 2]
        qi, qj = inref(pi), inref(pj)
        if mutant == "frame_inverse_not_transpose":                        # backward through M^-T in place of M
            back = torch.linalg.inv(F[j, :2, :2]).transpose(0, 1)
            qi, qj = (_forward_as(q, torch.einsum("ij,ntj->nti", back, w_)) for q, w_ in ((qi, pi), (qj, pj)))
        if kind in ("keep_distance", "stay_away"):
            d = (qi - qj).norm(dim=-1)
            e, kinks, dist = clip0(lo - d) + clip0(d - hi), [(d, lo), (d, hi)], d
        else:
            dev = qj - qi
            sy = -1.0 if kind == "front_collision" else 1.0
            e, kinks, dist = abs0(dev[..., 0]) + clip0(sy * dev[..., 1]), [(dev[..., 0], 0.0), (dev[..., 1], 0.0)], None
    if decay > 0:
        w = torch.tensor([decay ** t for t in range(H)], dtype=traj.dtype)
        w = w if mutant == "decay_not_normalised" else w / w.sum()
        if mutant == "late_steps_off" and decay < 1:
            w = torch.cat([w[:40], 1.02 * w[40:]])
        e = e * w
        if mutant == "decay_not_averaged":
            return e.sum(dim=-1), kinks, dist
    return e.mean(dim=-1), kinks, dist


def values(traj, term, mutant=None):
    """The unweighted values [P,N] as upstream's classes return them."""
    return torch.stack([_pair(traj, term, p, mutant)[0] for p in range(len(term["target"]))])


def total(traj, term, mutant=None):
    """sum over pairs and samples of scale[p] * value: with scale = weight / samples this is DiffuserGuidance's weight * mean(loss)."""
    tot = 0.0
    for p in range(len(term["target"])):
        tot = tot + float(term["scale"][p]) * _pair(traj, term, p, mutant)[0].sum()
    return tot


def incidences(term):
    """{agent: [(pair, role)] in ascending pair * 2 + role}: the order in which the kernel's gather walks an agent's pairs."""
    per = {}
    for p, (i, j) in enumerate(zip(term["target"], term["ref"])):
        per.setdefault(int(i), []).append((p, 0))
        per.setdefault(int(j), []).append((p, 1))
    return {a: sorted(v, key=lambda pr: 2 * pr[0] + pr[1]) for a, v in sorted(per.items())}


def _stale_total(traj, term):
    """A total whose gradient w.r.t. agent a's plans is the gather of a thread that reuses the previous incidence's step weights."""
    tot = 0.0
    rows = torch.arange(traj.shape[0])[:, None, None, None]
    for a, inc in incidences(term).items():
        xa = torch.where(rows == a, traj, traj.detach())
        for s, (p, _) in enumerate(inc):
            dec = max(float(term["decay"][inc[s - 1][0] if s else p]), 0.0)
            tot = tot + float(term["scale"][p]) * _pair(xa, term, p, None, decay=dec)[0].sum()
    return tot


def value_and_grad(traj, term, mutant=None):
    assert mutant is None or mutant in MUTANTS
    if mutant == "world_difference":
        v, g = value_and_grad(traj.float(), term)
        return v.to(traj.dtype), g.to(traj.dtype)
    x = traj.clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(_stale_total(x, term) if mutant == "stale_decay" else total(x, term, mutant), x)
    if mutant == "small_agent_off":
        once = [a for a, inc in incidences(term).items() if len(inc) == 1]
        g[once] = g[once] * 1.01
    return values(traj, term, None if mutant == "stale_decay" else mutant).detach(), g


def margins(traj, term):
    """(smallest distance read, smallest distance of a per-step quantity from its kink: |d - bound| for the distance bands and the
    collision radius, |Dx| and |Dy| for the frame relations): what keeps a float32 evaluation on the same side of every decision."""
    dmin, kink = float("inf"), float("inf")
    with torch.no_grad():
        for p in range(len(term["target"])):
            _, kinks, dist = _pair(traj, term, p)
            if dist is not None:
                dmin = min(dmin, float(dist.min()))
            for q, bound in kinks:
                kink = min(kink, float((q - bound).abs().min()))
    return dmin, kink


def branches(traj, term, p):
    """Per sample [N], which clip branches of pair p are active at some step / at every step -> dict name -> (any [N], all [N])."""
    with torch.no_grad():
        _, kinks, dist = _pair(traj, term, p)
        kind = term["kind"][p]
        if kind == "collision":
            act = {"above": kinks[0][0] > kinks[0][1]}
        elif kind in ("keep_distance", "stay_away"):
            act = {"below_min": kinks[0][0] < kinks[0][1], "above_max": kinks[1][0] > kinks[1][1]}
        else:
            sy = -1.0 if kind == "front_collision" else 1.0
            act = {"y": sy * kinks[1][0] > 0}
        return {k: (v.any(dim=-1), v.all(dim=-1)) for k, v in act.items()}


def sgd_steps(wdec, mean, cond, cs, term, n_steps, lr, num_samp=1, extra=None):
    """n_steps plain SGD steps of the guided mean [A N,52,4] on total(decode(x)) (+ extra(traj), another loss on the decoded plans
    [A N,52,6]) -> (guided mean, gradient of the first step, the decoded plans [A,N,52,6] of every iterate the loss was evaluated on)."""
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


def term_from_meta(case, world_from_agent, agent_from_world, N):
    """The yardstick term of one recorded case: `case` = meta['cases'][name] with a list `pairs` of dicts (target, ref, kind, lo, hi,
    decay, weight)."""
    ps = case["pairs"]
    return dict(target=[int(q["target"]) for q in ps], ref=[int(q["ref"]) for q in ps], kind=[q["kind"] for q in ps],
                lo=[float(q["lo"]) for q in ps], hi=[float(q["hi"]) for q in ps], decay=[float(q["decay"]) for q in ps],
                scale=[float(q["weight"]) / N for q in ps], world_from_agent=torch.as_tensor(world_from_agent).double(),
                agent_from_world=None if agent_from_world is None else torch.as_tensor(agent_from_world).double())
