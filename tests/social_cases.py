"""The cases of the social-group regime tests (tests/test_gpu_social_regimes.py), built on the CPU so that
tests/test_social_cases_host.py can assert what they claim without a GPU, and the check both modules apply: the kernel on the GPU, the
yardstick's mutants (tests/social_yardstick.py) on the CPU.

The kernel (csrc/social_kernels.hip): a workgroup of the gradient role owns steps_per_wg = min(52, 256 / max_members) steps of one
(group, sample), one of the value role kOwn = 8 members; the rows of LDS have the odd stride Ms = M | 1.  Launch cases (groups named by
their sizes, non-members before, between and behind them, each at N = 1; m9_8_2_n3 at N = 3):
  m4            steps_per_wg 52: one run of steps                      m5_3_2   51: runs of 51 + 1; the group of 2 at 1 / 100 of the scale
  m6            42: runs of 42 + 10                                    m9_8_2   28; value chunks of 8 + 1 and of exactly 8; odd and even M
  m16           16; two full value chunks                              m64_7    4
  m85, m86_16   3 | 2: the two sides of 256 / 3                        declared_128   groups of 3 and 9 under max_members = 128: 2
Per group in turn: cohesion 0, 0.6, 1, 0.3; leader -1, a member, the FIRST member (whose frame origin the kernel shifts by), an agent
outside the group; scale 1, 0.1, 0.01 (/ members / samples).  Single groups start the turn at another place each.
  hub           110 members under cohesion 1 whose draws all name member 0: its gather sums 109 terms + its own.  (In the plane no
                member can be the NEAREST of more than six others that are nearer to it than to each other, so the draws name it.)
  far           m9_8_2 at (1500, 900) m: needs the calibrator on the translated scene
  exact_ties    identity frames, standing plans, cohesion 0, every distance exact: five members on a line 2 m apart under social_dist
                1.5 (gradient x 52: -2, 1, 0, 0, 1 -- the first minimum decides) and under 2.0 (all 0); two coincident members (d = 0:
                gradient 0, value sd^2); two coincident members and a third 4 m away, whose term goes to the first of them (-5, 0, 5)
  exact_draws   cohesion 0.5 with u exactly 0.5 (the nearest is used) and nextafter(0.5, 0) (the draw is); a group whose caller draws r
                lie outside [0, M - 2] (the reference takes the clamped ones, the GPU test runs both); M = 2 under cohesion 1

The check (`ratios`).  ref64: the yardstick in float64 on the float32 inputs.  ref32: the yardstick in float32 on the scene translated
back to the origin (the case's offset subtracted from every frame translation in float64, a cast that is asserted exact).  Errors are
normalised BEFORE the maximum is taken, so that no group hides behind another:
  grad_x, grad_y   per group and channel by the group's max|g64| over x and y (per MEMBER in `hub`):   max(err / m) <= 4 max(err32 / m) + 1e-7
  values           per group by the group's max|v64|, the same bar
Where a normaliser is 0 the element must be exactly 0 (ratio inf otherwise).

EXACT.  `exact_ties` leaves nothing to rounding -- float32 reproduces float64 to the rounding of scale / 52 -- so the calibrated bar
would collapse to its floor; it is held to k 2^-24 of the group's max|g64| / max|v64|, k counted from the kernel's operation chain
(each rounding <= 2^-24 relative; a division is correctly rounded in this build, counted double all the same):
  gradient  w = (d - sd) / d (2), w * dx (1), at most two additions of gathered terms (2), c = 2 scale / 52 (2), g * c (1), R^T = identity
            (0), added to 0 (0): EXACT_GRAD_K = 8
  value     e = d - sd exact, e * e (1), 51 additions in ascending t (51), / 52 (2): 54 -> EXACT_VALUE_K = 55
`exact_draws` fixes its decisions by exact float32 comparisons (u against cohesion) on generic geometry: it keeps the calibrated bar and
the margins on distances and neighbours, not the one on |u - cohesion|.
"""
import functools
import math

import numpy as np
import torch

from tests import social_yardstick as Y

OFFSET = (1500.0, 900.0)
EXACT_GRAD_K, EXACT_VALUE_K = 8, 55
KTHREADS, KOWN = 256, 8
COHESION = (0.0, 0.6, 1.0, 0.3)
SCALE = (1.0, 0.1, 0.01)


def f32(v):
    return float(np.float32(v))


def frames_of(pos, th):
    W = np.zeros((len(th), 3, 3))
    W[:, 0, 0], W[:, 0, 1], W[:, 1, 0], W[:, 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    W[:, :2, 2], W[:, 2, 2] = pos, 1.0
    return torch.from_numpy(W.astype(np.float32)).double()


def creeping_plans(rng, A, N):
    """Every plan creeps 0.2 m forward with a wobble of centimetres, so the neighbour order of the stance holds over the plan."""
    plans = np.zeros((A, N, 52, 6), np.float32)
    plans[..., 0] = 0.2 * (np.arange(52) + 1) / 52 + 0.02 * rng.standard_normal((A, N, 52))
    plans[..., 1] = 0.02 * rng.standard_normal((A, N, 52))
    plans[..., 2:] = rng.standard_normal((A, N, 52, 4))
    return torch.from_numpy(plans)


def clear_of(u, coh):
    """u moved 1e-5 past cohesion where it is within 2e-6 of it."""
    c = np.float32(coh)
    return np.where(np.abs(u.astype(np.float64) - float(c)) < 2e-6, np.float32(float(c) + 1e-5), u).astype(np.float32)


def groups_case(sizes, N, seed, offset=(0.0, 0.0), turn=0, max_members=None):
    """Groups of the given sizes.  A group's members stand along a line at spacings of 2, 2.4, 2.8, 3.2, 3.6 m in turn (two adjacent
    spacings differ by 0.4 m at least: the nearer side is the nearest neighbour by a margin), with staggered lateral offsets and
    headings of their own, the groups 45 m apart, `offset` away from the world origin.
    -> (plans [A,N,52,6] float32, yardstick term, caller draws r int32 / u float32 [A,N,52], offset)."""
    rng = np.random.default_rng(seed)
    groups, a = [], 0
    for gi, M in enumerate(sizes):
        a += 1 + gi % 2
        groups.append(list(range(a, a + M)))
        a += M
    A = a + 1
    pos = rng.uniform(-30.0, 30.0, (A, 2))
    th = rng.uniform(-0.3, 0.3, A)
    term = dict(groups=groups, leader=[], social_dist=[], cohesion=[], scale=[])
    if max_members is not None:
        term["max_members"] = max_members
    r, u = np.zeros((A, N, 52), np.int32), rng.uniform(0.0, 1.0, (A, N, 52)).astype(np.float32)
    for gi, grp in enumerate(groups):
        M = len(grp)
        i = np.arange(M)
        pos[grp, 0] = np.concatenate([[0.0], np.cumsum(2.0 + 0.4 * (i[:-1] % 5))])
        pos[grp, 1] = 45.0 * gi + 0.1 * ((5 * i) % 7)
        k = (gi + turn) % 4
        term["leader"].append((-1, grp[M // 2], grp[0], grp[0] - 1)[k])
        term["social_dist"].append(1.5 + 0.25 * gi)
        term["cohesion"].append(f32(COHESION[k]))
        term["scale"].append(f32(0.7 * SCALE[gi % 3] / (M * N)))
        r[grp] = rng.integers(0, M - 1, (M, N, 52))
        u[grp] = clear_of(u[grp], COHESION[k])
    term["world_from_agent"] = frames_of(pos + np.asarray(offset), th)
    return creeping_plans(rng, A, N), term, torch.from_numpy(r), torch.from_numpy(u), tuple(offset)


HUB_M = 110


def hub_case(seed=71):
    """One group of 110: member 0 in the middle, the others around it at 2 .. 7.5 m; cohesion 1 and r = 0 for every other member, so
    that each of them is paired with member 0 at every step (r < i: nb = r), member 0 itself with whom its draw says."""
    rng = np.random.default_rng(seed)
    A = HUB_M + 2
    grp = list(range(1, 1 + HUB_M))
    i = np.arange(HUB_M)
    pos = rng.uniform(-30.0, 30.0, (A, 2))
    rad, ang = 2.0 + 0.05 * i, 2.399963 * i
    pos[grp] = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    pos[grp[0]] = 0.0
    r = np.zeros((A, 1, 52), np.int32)
    r[grp[0]] = rng.integers(0, HUB_M - 1, (1, 52))
    u = rng.uniform(0.0, 0.999, (A, 1, 52)).astype(np.float32)
    term = dict(groups=[grp], leader=[-1], social_dist=[1.5], cohesion=[1.0], scale=[f32(1.0 / HUB_M)],
                world_from_agent=frames_of(pos, rng.uniform(-3.1, 3.1, A)))
    return creeping_plans(rng, A, 1), term, torch.from_numpy(r), torch.from_numpy(u), (0.0, 0.0)


# exact_ties: per group (social_dist, member positions, expected gradient x 52 in x at every step (y: 0), expected values)
EXACT_GROUPS = [
    (1.5, [(0.0, 0.0), (2.0, 0.0), (4.0, 0.0), (6.0, 0.0), (8.0, 0.0)], (-2.0, 1.0, 0.0, 0.0, 1.0), (0.25,) * 5),
    (2.0, [(0.0, 16.0), (2.0, 16.0), (4.0, 16.0), (6.0, 16.0), (8.0, 16.0)], (0.0,) * 5, (0.0,) * 5),
    (1.5, [(32.0, 0.0), (32.0, 0.0)], (0.0, 0.0), (2.25, 2.25)),
    (1.5, [(0.0, 32.0), (0.0, 32.0), (4.0, 32.0)], (-5.0, 0.0, 5.0), (2.25, 2.25, 6.25)),
]


def exact_ties_case():
    groups, pos, a = [], [], 0
    for _, pts, _, _ in EXACT_GROUPS:
        groups.append(list(range(a, a + len(pts))))
        pos += pts
        a += len(pts)
    pos.append((64.0, 64.0))                                                # one agent in no group
    A = a + 1
    W = torch.eye(3, dtype=torch.float64).repeat(A, 1, 1)
    W[:, :2, 2] = torch.tensor(pos, dtype=torch.float64)
    term = dict(groups=groups, leader=[-1] * 4, social_dist=[g[0] for g in EXACT_GROUPS], cohesion=[0.0] * 4, scale=[1.0] * 4, world_from_agent=W)
    plans = torch.zeros(A, 1, 52, 6)
    plans[..., 2:] = torch.from_numpy(np.random.default_rng(72).standard_normal((A, 1, 52, 4)).astype(np.float32))
    return plans, term, torch.zeros(A, 1, 52, dtype=torch.int32), torch.full((A, 1, 52), 0.5), (0.0, 0.0)


BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
R_OUTSIDE = (-3, -1, 2 ** 31 - 1, -2 ** 31)


def exact_draws_case(seed=73):
    """Groups of 4, 5 and 2 on the geometry of the launch cases.  Groups 0 and 1: cohesion 0.5, u = 0.5 where member + step is even and
    the float32 below 0.5 where it is odd.  Group 1's raw draws (`r_raw`) are -3, -1, 2^31 - 1, -2^31, M - 1 and M + 5 on every step
    that is no multiple of 3; the reference reads the clamped ones.  Group 2: M = 2 under cohesion 1, raw draws 0 and 7."""
    plans, term, r, u, offset = groups_case((4, 5, 2), 1, seed)
    term = dict(term, cohesion=[0.5, 0.5, 1.0], leader=[-1, term["groups"][1][2], -1])
    u, raw = u.clone(), r.clone().long()
    t = torch.arange(52)
    for grp in term["groups"][:2]:
        for i, a in enumerate(grp):
            u[a, 0] = torch.where((i + t) % 2 == 0, torch.tensor(0.5), torch.tensor(BELOW_HALF))
    M = len(term["groups"][1])
    outside = torch.tensor(R_OUTSIDE + (M - 1, M + 5))
    for i, a in enumerate(term["groups"][1]):
        raw[a, 0] = torch.where(t % 3 != 0, outside[(i + t) % len(outside)], raw[a, 0])
    raw[term["groups"][2][0], 0, ::2] = 7
    u[term["groups"][2]] = u[term["groups"][2]].clamp(max=0.999)
    size = torch.zeros(plans.shape[0], dtype=torch.long)
    for grp in term["groups"]:
        size[grp] = len(grp)
    clamped = torch.minimum(raw.clamp(min=0), (size - 2).clamp(min=0)[:, None, None])
    return plans, term, clamped.to(torch.int32), u, offset, raw.to(torch.int32)


# name -> (builder, exact)
CASES = {
    "m4": (lambda: groups_case((4,), 1, 51, turn=1), False),
    "m5_3_2": (lambda: groups_case((5, 3, 2), 1, 52), False),
    "m6": (lambda: groups_case((6,), 1, 53, turn=3), False),
    "m9_8_2": (lambda: groups_case((9, 8, 2), 1, 54), False),
    "m9_8_2_n3": (lambda: groups_case((9, 8, 2), 3, 55), False),
    "m16": (lambda: groups_case((16,), 1, 56), False),
    "m64_7": (lambda: groups_case((64, 7), 1, 57, turn=1), False),
    "m85": (lambda: groups_case((85,), 1, 58, turn=1), False),
    "m86_16": (lambda: groups_case((86, 16), 1, 59, turn=3), False),
    "declared_128": (lambda: groups_case((3, 9), 1, 60, turn=1, max_members=128), False),
    "hub": (hub_case, False),
    "far": (lambda: groups_case((9, 8, 2), 1, 54, offset=OFFSET), False),
    "exact_ties": (exact_ties_case, True),
    "exact_draws": (exact_draws_case, False),
}
NAMES = list(CASES)
LAUNCH = NAMES[:10]
PER_MEMBER = ("hub",)
NO_U_MARGIN = ("exact_ties", "exact_draws")


def translated(term, offset):
    """The term with `offset` subtracted from every frame translation in float64 -> (term, whether its float32 cast is exact)."""
    W = term["world_from_agent"].clone()
    W[:, :2, 2] -= torch.tensor(offset, dtype=torch.float64)
    return dict(term, world_from_agent=W), bool(torch.equal(W.float().double(), W))


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict(plans [A,N,52,6] float32, term, r, u [A,N,52], offset, v64 [A,N], g64 [A,N,52,6], v32, g32 (float64 tensors of the float32
    run on the translated scene), exact_translation, r_raw | None); computed once, not to be modified."""
    built = CASES[name][0]()
    plans, term, r, u, offset = built[:5]
    v64, g64 = Y.value_and_grad(plans.double(), term, r, u)
    tt, exact = translated(term, offset)
    v32, g32 = Y.value_and_grad(plans.float(), tt, r, u)
    return dict(plans=plans, term=term, r=r, u=u, offset=offset, v64=v64, g64=g64, v32=v32.double(), g32=g32.double(), exact_translation=exact,
                r_raw=built[5] if len(built) > 5 else None)


def max_members(term):
    return int(term.get("max_members") or max(len(g) for g in term["groups"]))


def launch_shape(term):
    """From launch_social_group's formulas -> (steps_per_wg, the runs of steps, per group the runs of members of the value role)."""
    mm = max_members(term)
    spw = min(52, max(1, KTHREADS // mm))
    runs = [min(spw, 52 - t0) for t0 in range(0, 52, spw)]
    return spw, runs, [[min(KOWN, len(g) - i0) for i0 in range(0, len(g), KOWN)] for g in term["groups"]]


def quiet_rows(term, A):
    """(member [A], quiet [A]): agents in a group; agents that receive no gradient -- in no group, or their group's leader."""
    member, quiet = torch.zeros(A, dtype=torch.bool), torch.ones(A, dtype=torch.bool)
    for grp, ld in zip(term["groups"], term["leader"]):
        member[grp] = True
        quiet[[a for a in grp if a != ld]] = False
    return member, quiet


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
    """The bars of tests/test_gpu_social.py's check_kernel, relative to the GLOBAL maxima -> (value error over 2e-5 max(1, max|v64|),
    gradient error over 1e-4 max|g64|)."""
    r = reference(name)
    got_v, got_g = torch.as_tensor(values).double().cpu().reshape(r["v64"].shape), torch.as_tensor(grad).double().cpu().reshape(r["g64"].shape)
    return (float((got_v - r["v64"]).abs().max()) / (2e-5 * max(1.0, float(r["v64"].abs().max()))),
            float((got_g - r["g64"]).abs().max()) / (1e-4 * float(r["g64"].abs().max())))


def ratios(name, values, grad):
    """What both test modules hold a result (values [A N], grad [A N,52,6]) to -> {check: error over its bar}; a result passes when
    every ratio is <= 1 (module docstring).  The worst group counts."""
    r = reference(name)
    got_v, got_g = torch.as_tensor(values).double().cpu().reshape(r["v64"].shape), torch.as_tensor(grad).double().cpu().reshape(r["g64"].shape)
    exact = CASES[name][1]
    out = {}

    def worst(key, v):
        out[key] = max(out.get(key, 0.0), v)
    for grp in r["term"]["groups"]:
        v, v64, v32 = got_v[grp], r["v64"][grp], r["v32"][grp]
        g, g64, g32 = got_g[grp][..., :2], r["g64"][grp][..., :2], r["g32"][grp][..., :2]           # [M,N,52,2]
        mv = v64.abs().max().reshape(1, 1)
        mg = g64.abs().amax(dim=(1, 2, 3), keepdim=True) if name in PER_MEMBER else g64.abs().amax(dim=(0, 1, 2, 3), keepdim=True)
        mg = mg.expand(-1, -1, -1, 2)                                       # over both channels: a rotation mixes them
        if exact:
            ev, eg = (v - v64).abs(), (g - g64).abs()
            bad = (float(mv) == 0 and bool((ev != 0).any())) or bool((eg[mg.expand_as(eg) == 0] != 0).any())
            worst("values", math.inf if bad else float(ev.max()) / (EXACT_VALUE_K * 2.0 ** -24 * max(float(mv), 1e-300)))
            worst("exact", math.inf if bad else float((eg / mg.clamp(min=1e-300)).max()) / (EXACT_GRAD_K * 2.0 ** -24))
            continue
        worst("values", normalised((v - v64).abs(), (v32 - v64).abs(), mv))
        for c, label in enumerate("xy"):
            worst("grad_" + label, normalised((g - g64)[..., c].abs(), (g32 - g64)[..., c].abs(), mg[..., c]))
    return out
