"""The cases of the pair-relation regime tests (tests/test_gpu_pair_regimes.py), built on the CPU so that
tests/test_pair_cases_host.py can assert what they claim without a GPU, and the check both modules apply: the kernel on the GPU, the
yardstick's mutants (tests/pair_yardstick.py) on the CPU.

The kernel (csrc/pair_kernels.hip): kThreads = 256 (involved agent, sample, step) items per workgroup of the gradient role, kWaves = 4
(pair, sample) waves per workgroup of the value role; a gradient thread walks its agent's incidences in ascending order and keeps the
step weight of the last decay it saw.  Cases (A agents, N samples, P pairs):
  fill_exact     16 involved agents (of 18) x N = 4: 3328 gradient items = 13 full workgroups; P N = 48 = 12 full value workgroups
  fill_plus_one  17 involved agents, N = 1, P = 9: a third value workgroup with one live wave; the last gradient workgroup partly empty
  samples_3      N = 3
  roles          an agent that is only ever ref, one only ever target, the same (i, j) under all five kinds, (i, j) and (j, i), agent 0 in
                 64 pairs in both roles, one agent in a single pair of the smallest scale; scales spanning 100 x
  decay_mix      agent 0 in 35 pairs, every kind under every decay of -1, 0, 0.5, 0.9, 1.0, 1.05, interleaved so that consecutive
                 incidences of agent 0 differ (0.9, 0.5, 0, 0.9, -1, 1.0, 1.05, ...); also checked per (agent, step)
  quadrants      headings in all four quadrants and on both sides of +-pi; the second half of the agents has left-handed frames
  given_frames   agent_from_world passed, its 2 x 2 the transposed world rotation turned by 0.2 rad and scaled by 1.25: M^T != M^-1
  far            `roles` at (1500, 900) m: needs the calibrator on the translated scene
  exact_kinks    one pair per decision on exactly representable geometry (EXACT below)

The check (`ratios`).  ref64: the yardstick in float64 on the float32 inputs (the per-pair floats lo, hi, decay, scale are float32
values too).  ref32: the yardstick in float32 on the scene translated back to the origin -- the case's offset subtracted from every
frame translation in float64, a cast that is asserted exact -- so that the calibrator carries the rounding of the metres between two
agents, as the kernel's header promises, not of the scene's place in the world.  Errors are normalised BEFORE the maximum is taken:
  grad_x, grad_y   per involved agent and channel by the agent's max|g64| (over x and y: the rotation into the plan mixes them, and a
                   channel that is 0 in exact arithmetic would be normalised by float64's rounding):   max(err / m) <= 4 max(err32 / m) + 1e-7
  step_x, step_y   decay_mix only: per (agent, step) and channel by the max over the samples of |g64|, the same bar
  values           per pair by S_p = max_n sum_t w_t s_t, s_t = the distance read (|qx| + |qy| for the frame relations): the scale of
                   what is read before the clip, in float64, the same bar
Where a normaliser is 0 the element must be exactly 0 (ratio inf otherwise).

EXACT.  In `exact_kinks` every frame entry is 0 or +-1, every position dyadic, every distance read a 3-4-5 hypotenuse and the plans
stand, so float32 meets no rounding up to the decision and the calibrated bar would collapse to its floor.  Its elements are held to
k 2^-24 of the agent's max|g64| (the pair's |v64| for values), k counted from the kernel's operation chain (each rounding <= 2^-24
relative; a division or square root is correctly rounded in this build, counted double all the same):
  gradient  s = c / d (2), s * q (1), M^T and R^T with entries 0, +-1 (0), w = 1 / 52 (1), scale * w (1), c * u (1), one term per agent,
            added to 0 (0): 6 -> EXACT_GRAD_K = 8
  value     e exact, w = 1 / 52 (1), e * w (1), 51 additions in ascending t, each <= 2^-24 of the total (51): EXACT_VALUE_K = 53
"""
import functools
import math

import numpy as np
import torch

from tests import pair_yardstick as Y

OFFSET = (1500.0, 900.0)
DECAYS = (0.9, 0.5, 0.0, 0.9, -1.0, 1.0, 1.05)
EXACT_GRAD_K, EXACT_VALUE_K = 8, 53
KTHREADS, KWAVES = 256, 4
DMIN, KINK = 1e-2, 1e-3


def f32(v):
    return float(np.float32(v))


def frames_of(pos, th, mirror=None):
    W = np.zeros((len(th), 3, 3))
    W[:, 0, 0], W[:, 0, 1], W[:, 1, 0], W[:, 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    if mirror is not None:
        W[mirror, :2, 1] *= -1.0                                            # left-handed: y to the right, det = -1
    W[:, :2, 2], W[:, 2, 2] = pos, 1.0
    return torch.from_numpy(W.astype(np.float32)).double()


def scene(A, N, seed, offset=(0.0, 0.0), th=None, mirror=None, speed=3.0):
    """A agents on a jittered 6-m grid of five columns `offset` away from the world origin, plans that drive forward at 0..speed m/s
    with a wobble of centimetres -> (generator, world_from_agent [A,3,3] float64 of float32 values, plans [A,N,52,6] float32)."""
    rng = np.random.default_rng(seed)
    k = np.arange(A)
    pos = np.stack([6.0 * (k % 5), 6.0 * (k // 5)], axis=1) + rng.uniform(-1.0, 1.0, (A, 2)) + np.asarray(offset)
    th = rng.uniform(-0.5, 0.5, A) if th is None else np.asarray(th, np.float64)
    plans = np.zeros((A, N, 52, 6), np.float32)
    v = rng.uniform(0.0, speed, (A, N, 1))
    plans[..., 0] = v * 0.1 * (np.arange(52) + 1) + 0.02 * rng.standard_normal((A, N, 52))
    plans[..., 1] = 0.02 * rng.standard_normal((A, N, 52))
    plans[..., 2:] = rng.standard_normal((A, N, 52, 4))
    return rng, frames_of(pos, th, mirror), torch.from_numpy(plans)


def empty_term(W, F=None):
    return dict(target=[], ref=[], kind=[], lo=[], hi=[], decay=[], scale=[], world_from_agent=W, agent_from_world=F)


def settle(plans, W, F, i, j, kind):
    """(lo, hi) of pair (i, j) under `kind`, float32 values, or None when the pair cannot keep the margins (no distance read below
    1e-2 m, nothing within 1e-3 of a kink): the distance relations take the 30 % / 70 % quantiles of the distances the plans read,
    moved on in steps of 13.7 mm until they are clear; the frame relations have no bounds and keep the pair as it is or not at all."""
    one = dict(empty_term(W, F), target=[i], ref=[j], decay=[0.0], scale=[1.0], lo=[0.0], hi=[0.0])
    p64 = plans.double()
    if kind in ("front_collision", "collide_left"):
        return (0.0, 0.0) if Y.margins(p64, dict(one, kind=[kind]))[1] >= 1.1 * KINK else None
    d = Y._pair(p64, dict(one, kind=[kind]), 0)[2].reshape(-1)
    if float(d.min()) < DMIN:
        return None
    lo, hi = float(torch.quantile(d, 0.3)), float(torch.quantile(d, 0.7))
    for _ in range(400):
        lo, hi = f32(lo), f32(hi)
        if float(torch.minimum((d - lo).abs(), (d - hi).abs()).min()) >= 1.1 * KINK:
            return (lo, 0.0) if kind == "collision" else (lo, hi)
        lo, hi = lo + 0.0137, hi + 0.0137
    return None


def add_pair(term, plans, i, j, kind, decay, scale):
    """Append pair (i, j) if it can keep the margins -> whether it did."""
    b = settle(plans, term["world_from_agent"], term["agent_from_world"], i, j, kind)
    if b is None:
        return False
    for k, v in (("target", int(i)), ("ref", int(j)), ("kind", kind), ("lo", b[0]), ("hi", b[1]), ("decay", f32(decay)), ("scale", f32(scale))):
        term[k].append(v)
    return True


def fill(term, plans, ends, N, decay=lambda c, kind: 0.9 if kind == "stay_away" else 0.0):
    """One pair per entry of `ends` [(i, j)], the kinds in turn (a pair that cannot keep the margins under its kind takes the next one
    that can), scales 0.3 (1 + c % 7) / N."""
    for c, (i, j) in enumerate(ends):
        assert any(add_pair(term, plans, i, j, Y.KINDS[(c + s) % 5], decay(c, Y.KINDS[(c + s) % 5]), 0.3 * (1 + c % 7) / N) for s in range(5)), (i, j)
    return term


def fill_exact_case(N=4, seed=101):
    """18 agents, 16 of them in the 12 pairs (agents 0 and 17 in none)."""
    rng, W, plans = scene(18, N, seed)
    ends = [(1 + 2 * k, 2 + 2 * k) for k in range(8)] + [(1, 4), (6, 3), (9, 12), (16, 13)]
    return plans, fill(empty_term(W), plans, ends, N), (0.0, 0.0)


def fill_plus_one_case(N=1, seed=102):
    """19 agents, 17 of them in the 9 pairs (agents 0 and 9 in none)."""
    rng, W, plans = scene(19, N, seed)
    ends = [(1, 2), (3, 4), (5, 6), (7, 8), (10, 11), (12, 13), (14, 15), (16, 17), (18, 1)]
    return plans, fill(empty_term(W), plans, ends, N), (0.0, 0.0)


def samples_3_case(N=3, seed=103):
    rng, W, plans = scene(12, N, seed)
    ends = [tuple(int(a) for a in rng.choice(np.arange(1, 12), 2, replace=False)) for _ in range(20)]
    return plans, fill(empty_term(W), plans, ends, N), (0.0, 0.0)


ONLY_REF, ONLY_TARGET, SMALL, HUB = 18, 19, 20, 0


def roles_case(offset=(0.0, 0.0), N=2, seed=104):
    """22 agents, 83 pairs.  Agent 0 (HUB) with each of agents 1..16 as target and as ref under two kinds each: 64 pairs, 32 in either
    role.  The first pair (i, j) of agents 1..16 that keeps the margins under all five kinds takes all five, and (j, i) one.  Agent 18 is
    the ref of six pairs and never a target, agent 19 the target of six and never a ref, agent 20 (SMALL) sits in ONE pair, as target,
    at scale 0.01 / N; the other scales are 0.03 .. 1 / N (100 x in all).  Agents 17 and 21 are in no pair."""
    rng, W, plans = scene(22, N, seed, offset)
    term = empty_term(W)
    c = 0
    for k in range(1, 17):
        for role in (0, 1):
            n_ok = 0
            for s in range(5):
                kind = Y.KINDS[(c + s) % 5]
                i, j = (HUB, k) if role == 0 else (k, HUB)
                if n_ok < 2 and add_pair(term, plans, i, j, kind, 0.9 if kind == "stay_away" else 0.0, (0.03, 0.1, 0.3, 1.0)[c % 4] / N):
                    n_ok += 1
            assert n_ok == 2, (k, role)
            c += 1
    five = None
    for i in range(1, 17):
        for j in range(1, 17):
            if five is None and i != j and all(settle(plans, W, None, i, j, kind) is not None for kind in Y.KINDS) and settle(plans, W, None, j, i, "keep_distance"):
                five = (i, j)
    assert five is not None
    for kind in Y.KINDS:
        assert add_pair(term, plans, five[0], five[1], kind, 0.9 if kind == "stay_away" else 0.0, 0.5 / N)
    assert add_pair(term, plans, five[1], five[0], "keep_distance", 0.0, 0.5 / N)
    fill(term, plans, [(k, ONLY_REF) for k in (3, 5, 8, 11, 13, 16)] + [(ONLY_TARGET, k) for k in (2, 4, 7, 9, 12, 15)], N)
    assert add_pair(term, plans, SMALL, 14, "keep_distance", 0.0, 0.01 / N)
    return plans, term, tuple(offset)


def decay_mix_case(N=2, seed=105):
    """16 agents, 40 pairs: pair c = 0..34 joins agent 0 (target for even c, ref for odd c) and agent 1 + c % 14 under kind c % 5 and decay
    DECAYS[c % 7] -- 5 and 7 are coprime, so every kind meets every entry of DECAYS, and agent 0's ascending incidences are the pairs
    in this order; five more pairs among the others under decay 0.9, 0.5, 1.05."""
    rng, W, plans = scene(16, N, seed)
    term = empty_term(W)
    for c in range(35):
        kind, ok = Y.KINDS[c % 5], False
        for s in range(14):                                                 # (the first partner that keeps the margins under this kind)
            k = 1 + (c + s) % 14
            i, j = (0, k) if c % 2 == 0 else (k, 0)
            if add_pair(term, plans, i, j, kind, DECAYS[c % 7], 0.3 * (1 + c % 7) / N):
                ok = True
                break
        assert ok, c
    fill(term, plans, [(3, 7), (9, 4), (12, 2), (5, 13), (14, 6)], N, decay=lambda c, kind: (0.9, 0.5, 1.05)[c % 3])
    return plans, term, (0.0, 0.0)


def quadrants_case(N=2, seed=106):
    """20 agents: headings 0.8, 2.4, -2.4, -0.8 (+- 0.25) and pi (+- 0.04, agents 16 and 17 on either side of the branch cut); agents
    10..19 have left-handed frames.  30 pairs, right- and left-handed frames mixed in a pair."""
    rng = np.random.default_rng(seed)
    base = np.tile([0.8, 2.4, -2.4, -0.8, np.pi], 4)
    th = base + np.where(base > 3.0, rng.uniform(-0.04, 0.04, 20), rng.uniform(-0.25, 0.25, 20))
    th[4], th[9] = np.pi - 0.03, -np.pi + 0.02
    th[14], th[19] = np.pi - 0.02, -np.pi + 0.03
    _, W, plans = scene(20, N, seed, th=th, mirror=np.arange(10, 20), speed=1.0)
    ends = [tuple(int(a) for a in rng.choice(20, 2, replace=False)) for _ in range(26)] + [(4, 9), (9, 14), (14, 19), (19, 4)]
    return plans, fill(empty_term(W), plans, ends, N), (0.0, 0.0)


def given_frames_case(N=2, seed=107):
    """12 agents, 20 pairs; agent_from_world[a] = [[M_a, -M_a t_a], [0, 1]] with M_a = 1.25 Rot(0.2) R_a^T: q = M_j (p_i - p_j) as the
    kernel's header states it, gradient M_j^T (d e / d q); M^T and M^-1 differ by the factor 1.5625."""
    rng, W, plans = scene(12, N, seed)
    c, s = math.cos(0.2), math.sin(0.2)
    M = 1.25 * torch.tensor([[c, -s], [s, c]], dtype=torch.float64) @ W[:, :2, :2].transpose(1, 2)
    F = torch.zeros_like(W)
    F[:, :2, :2], F[:, 2, 2] = M, 1.0
    F[:, :2, 2] = -torch.einsum("aij,aj->ai", M, W[:, :2, 2])
    F = F.float().double()
    ends = [tuple(int(a) for a in rng.choice(12, 2, replace=False)) for _ in range(20)]
    return plans, fill(empty_term(W, F), plans, ends, N), (0.0, 0.0)


# exact_kinks: (kind, lo, hi, target position, ref position, rotation of both frames as (r00, r01, r10, r11)); standing plans, scale 1.
# q = R_j^T (p_i - p_j); expected value and target gradient x 52 in the target's plan columns (the ref's is R_j^T (-g)), derived by hand:
I2, ROT90, MIRROR = (1.0, 0.0, 0.0, 1.0), (0.0, -1.0, 1.0, 0.0), (1.0, 0.0, 0.0, -1.0)
EXACT_PAIRS = [
    # kind, lo, hi, p_i, p_j, R, value, target gradient x 52 (world), what it decides
    ("collision", 5.0, 0.0, (-3.0, -4.0), (0.0, 0.0), I2, 0.0, (-0.6, -0.8)),            # d == lo: clip passes at 0
    ("keep_distance", 5.0, 9.0, (3.0, 4.0), (0.0, 0.0), I2, 0.0, (-0.6, -0.8)),          # d == lo: relu(lo - d) passes at 0, relu(d - hi) idle
    ("keep_distance", 2.0, 5.0, (3.0, 4.0), (0.0, 0.0), I2, 0.0, (0.6, 0.8)),            # d == hi
    ("keep_distance", 5.0, 5.0, (3.0, 4.0), (0.0, 0.0), I2, 0.0, (0.0, 0.0)),            # lo == hi == d: both pass, cancels to 0
    ("keep_distance", 2.5, 9.0, (1.0, 2.0), (1.0, 2.0), I2, 2.5, (0.0, 0.0)),            # coincident, lo > 0: value lo, the norm's gradient at 0 is 0
    ("collision", 0.0, 0.0, (1.0, 2.0), (1.0, 2.0), I2, 0.0, (0.0, 0.0)),                # coincident, lo = 0
    ("front_collision", 0.0, 0.0, (0.0, 3.0), (0.0, 0.0), I2, 3.0, (0.0, 1.0)),          # qx == 0: abs gives 0; qy > 0
    ("front_collision", 0.0, 0.0, (2.0, 0.0), (0.0, 0.0), I2, 2.0, (1.0, 1.0)),          # qy == +0: clip passes
    ("front_collision", 0.0, 0.0, (2.0, 0.0), (0.0, 0.0), MIRROR, 2.0, (1.0, -1.0)),     # qy == -0 (R^T = diag(1, -1) on dy = +0)
    ("collide_left", 0.0, 0.0, (0.0, -3.0), (0.0, 0.0), I2, 3.0, (0.0, -1.0)),           # qx == 0; -qy > 0
    ("collide_left", 0.0, 0.0, (2.0, 0.0), (0.0, 0.0), I2, 2.0, (1.0, -1.0)),            # qy == +0: relu(-qy) passes at -0
    ("collide_left", 0.0, 0.0, (2.0, 0.0), (0.0, 0.0), MIRROR, 2.0, (1.0, 1.0)),         # qy == -0
    ("stay_away", 5.0, 9.0, (-4.0, 3.0), (0.0, 0.0), ROT90, 0.0, (0.8, -0.6)),           # d == lo in a turned frame
]


def exact_kinks_case():
    """Pair k joins agents 2 k (target) and 2 k + 1 (ref) of EXACT_PAIRS, 16 m apart from the next pair; both frames carry the pair's
    rotation, the positions are the frames' translations and the plans are 0 in x, y."""
    P = len(EXACT_PAIRS)
    W = torch.zeros(2 * P, 3, 3, dtype=torch.float64)
    term = empty_term(W)
    for k, (kind, lo, hi, pi, pj, R, _, _) in enumerate(EXACT_PAIRS):
        for a, pos in ((2 * k, pi), (2 * k + 1, pj)):
            W[a] = torch.tensor([[R[0], R[1], pos[0] + 16.0 * k], [R[2], R[3], pos[1] - 8.0 * k], [0.0, 0.0, 1.0]], dtype=torch.float64)
        for key, v in (("target", 2 * k), ("ref", 2 * k + 1), ("kind", kind), ("lo", lo), ("hi", hi), ("decay", 0.0), ("scale", 1.0)):
            term[key].append(v)
    plans = torch.zeros(2 * P, 1, 52, 6)
    plans[..., 2:] = torch.from_numpy(np.random.default_rng(108).standard_normal((2 * P, 1, 52, 4)).astype(np.float32))
    return plans, term, (0.0, 0.0)


# name -> (builder, exact)
CASES = {
    "fill_exact": (fill_exact_case, False),
    "fill_plus_one": (fill_plus_one_case, False),
    "samples_3": (samples_3_case, False),
    "roles": (roles_case, False),
    "decay_mix": (decay_mix_case, False),
    "quadrants": (quadrants_case, False),
    "given_frames": (given_frames_case, False),
    "far": (lambda: roles_case(OFFSET), False),
    "exact_kinks": (exact_kinks_case, True),
}
NAMES = list(CASES)
PER_STEP = ("decay_mix",)


def translated(term, offset):
    """The term with `offset` subtracted from every frame translation in float64 (agent_from_world's own translation cancels in every
    difference the relations form and is left as it is) -> (term, whether the float32 cast of the result is exact)."""
    W = term["world_from_agent"].clone()
    W[:, :2, 2] -= torch.tensor(offset, dtype=torch.float64)
    return dict(term, world_from_agent=W), bool(torch.equal(W.float().double(), W))


def value_scale(plans64, term):
    """S_p [P]: max over the samples of sum_t w_t s_t, s_t the distance read (|qx| + |qy| for the frame relations), float64."""
    out = []
    with torch.no_grad():
        for p in range(len(term["target"])):
            _, kinks, dist = Y._pair(plans64, term, p)
            s = dist if dist is not None else kinks[0][0].abs() + kinks[1][0].abs()
            dec = float(term["decay"][p])
            w = torch.tensor([dec ** t for t in range(52)], dtype=torch.float64) if dec > 0 else torch.ones(52, dtype=torch.float64)
            out.append(float(((s * (w / w.sum() if dec > 0 else w)).mean(dim=-1)).max()))
    return torch.tensor(out, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict(plans [A,N,52,6] float32, term, offset, v64 [P,N], g64 [A,N,52,6], v32, g32 (float64 tensors of the float32 run on the
    translated scene), S [P], exact_translation); computed once, not to be modified."""
    plans, term, offset = CASES[name][0]()
    v64, g64 = Y.value_and_grad(plans.double(), term)
    tt, exact = translated(term, offset)
    v32, g32 = Y.value_and_grad(plans.float(), tt)
    return dict(plans=plans, term=term, offset=offset, v64=v64, g64=g64, v32=v32.double(), g32=g32.double(), S=value_scale(plans.double(), term),
                exact_translation=exact)


def involved(term):
    return sorted(set(term["target"]) | set(term["ref"]))


def normalised(err, err32, m):
    """max(err / m) over 4 max(err32 / m) + 1e-7, m broadcast against err; where m == 0 the element must be exactly 0."""
    m = m.expand_as(err)
    zero = m == 0
    if bool((err[zero] != 0).any()):
        return math.inf
    if bool(zero.all()):
        return 0.0
    e, e32 = float((err / m)[~zero].max()), float((err32 / m)[~zero].max())
    return e / (4.0 * e32 + 1e-7)


def old_bar(name, values, grad):
    """The bars of tests/test_gpu_pair.py's check_kernel, relative to the GLOBAL maxima -> (value error over 2e-5 max(1, max|v64|),
    gradient error over 1e-4 max|g64|)."""
    r = reference(name)
    got_v, got_g = torch.as_tensor(values).double().cpu().reshape(r["v64"].shape), torch.as_tensor(grad).double().cpu().reshape(r["g64"].shape)
    return (float((got_v - r["v64"]).abs().max()) / (2e-5 * max(1.0, float(r["v64"].abs().max()))),
            float((got_g - r["g64"]).abs().max()) / (1e-4 * float(r["g64"].abs().max())))


def ratios(name, values, grad):
    """What both test modules hold a result (values [P,N], grad [A N,52,6]) to -> {check: error over its bar}; a result passes when every
    ratio is <= 1 (module docstring)."""
    r = reference(name)
    got_v, got_g = torch.as_tensor(values).double().cpu().reshape(r["v64"].shape), torch.as_tensor(grad).double().cpu().reshape(r["g64"].shape)
    rows = involved(r["term"])
    g, g64, g32 = got_g[rows][..., :2], r["g64"][rows][..., :2], r["g32"][rows][..., :2]           # [I,N,52,2]
    per_agent = g64.abs().amax(dim=(1, 2, 3), keepdim=True).expand(-1, -1, -1, 2)          # over both channels: a rotation mixes them
    if CASES[name][1]:
        ev, eg = (got_v - r["v64"]).abs(), (g - g64).abs()
        bad = bool((ev[r["v64"] == 0] != 0).any()) or bool((eg[per_agent.expand_as(eg) == 0] != 0).any())
        nz = r["v64"] != 0
        out = {"values": float((ev[nz] / r["v64"].abs()[nz]).max()) / (EXACT_VALUE_K * 2.0 ** -24),
               "exact": float((eg / per_agent.clamp(min=1e-300)).max()) / (EXACT_GRAD_K * 2.0 ** -24)}
        return {k: (math.inf if bad else v) for k, v in out.items()}
    out = {"values": normalised((got_v - r["v64"]).abs(), (r["v32"] - r["v64"]).abs(), r["S"][:, None])}
    for c, label in enumerate("xy"):
        out["grad_" + label] = normalised((g - g64)[..., c].abs(), (g32 - g64)[..., c].abs(), per_agent[..., c])
    if name in PER_STEP:
        per_step = g64.abs().amax(dim=(1, 3), keepdim=True).expand(-1, -1, -1, 2)
        for c, label in enumerate("xy"):
            out["step_" + label] = normalised((g - g64)[..., c].abs(), (g32 - g64)[..., c].abs(), per_step[..., c])
    return out


def launch_shape(name):
    """(gradient items, gradient workgroups, value items, value workgroups) from launch_pair's formulas."""
    r = reference(name)
    N = r["plans"].shape[1]
    gi, vi = len(involved(r["term"])) * N * 52, len(r["term"]["target"]) * N
    return gi, -(-gi // KTHREADS), vi, -(-vi // KWAVES)
