"""The random cases of the lane kernel tests (tests/test_gpu_lane.py), built on the CPU so that tests/test_lane_host.py can assert
their conditions without a GPU.  Unlike the recording's, these inputs are NOT settled: elements whose projection gap is below
NEAR = 1e-4 m are compared against every outcome within that gap, and values and gradients only on (entry, sample) rows free of them.

The kernel (csrc/lane_kernels.hip) stages a polyline's segments with a workgroup of 256 threads and walks them with 4 waves, wave w
taking segments w, w + 4, ...: the polyline sizes are those at which that logic changes -- 2 and 3 points (one and two segments: three
/ two waves idle), 4, 5, 6 (one below, at and one above 4 segments), 256, 257, 258 (likewise around 256 segments, the staging
stride) and 1024, the bound."""
import numpy as np
import torch

from tests import lane_yardstick as Y

NEAR = 1e-4
KINK = 1e-5            # above the fp32 rounding of a projected coordinate at 50 m (2^-24 * 64 m = 3.8e-6 m)
SIZES = (2, 3, 4, 5, 6, 256, 257, 258, 1024)
SAMPLES = (1, 3)
# (S, N) -> seed, where the default S * 10 + N does not keep the conditions tests/test_lane_host.py asserts (found by trying S * 10 + N +
# 1000 k for k = 1, 2, ... on the CPU; a row of 52 steps over 1-m segments is free of near-ties about one time in five)
SEEDS = {(4, 1): 2041, (6, 3): 1063, (256, 1): 49561, (256, 3): 4563, (257, 1): 41571, (257, 3): 5573, (258, 1): 275581, (258, 3): 20583,
         (1024, 1): 210241, (1024, 3): 16243}


def make_line(rng, S, n_valid=None, left=False):
    """An agent-frame polyline [S,3] float32 sorted by x: points about 1 m apart or, below 49 points, spread over 48 m (the reach
    of a plan); gentle curvature (the lateral offset stays within 15 m at the far end); NaN rows behind n_valid.  (Finer polylines
    make most elements near-ties: next to a vertex the distances to the two segments differ by a^2 / 2r only.)"""
    n = S if n_valid is None else n_valid
    step = max(1.0, 48.0 / max(n - 1, 1))
    x = -3.0 + np.concatenate([[0.0], np.cumsum(step * rng.uniform(0.9, 1.1, n - 1))])
    curv = rng.uniform(-0.004, 0.004) * min(1.0, (60.0 / (step * n)) ** 2)
    y0, slope = rng.uniform(-0.5, 0.5), rng.uniform(-0.04, 0.04)
    line = np.full((S, 3), np.nan, np.float32)
    line[:n] = np.stack([x, y0 + slope * x + curv * x * x + (3.5 if left else 0.0), np.arctan(slope + 2 * curv * x)], axis=1)
    return line


def make_plans(rng, A, N, drifting=()):
    plans = np.zeros((A, N, 52, 6), np.float32)
    t = np.arange(52) + 1
    speed = rng.uniform(3.0, 8.0, (A, N, 1))
    drift = rng.uniform(-0.02, 0.02, (A, N, 1))
    for a in drifting:                                                    # leaves its lane: the clip at 5 becomes active on the way
        drift[a] = rng.choice([-1.0, 1.0], (N, 1)) * rng.uniform(0.13, 0.2, (N, 1))
    plans[..., 0] = speed * 0.1 * t + 0.05 * rng.standard_normal((A, N, 52))
    plans[..., 1] = rng.uniform(-1.0, 1.0, (A, N, 1)) + drift * t + 0.05 * rng.standard_normal((A, N, 52))
    plans[..., 2] = speed
    plans[..., 3] = 0.1 * rng.standard_normal((A, N, 52))
    plans[..., 4:] = 0.1 * rng.standard_normal((A, N, 52, 2))
    return torch.from_numpy(plans)


def size_case(S, N):
    """Five agents, six polylines of S points: agent 0 carries no entry, agent 1 `following`, agent 2 TWO entries (`change_left` on a
    left polyline, then `follow_decayed` on its own), agent 3 `follow_decayed` while it drifts off its lane, agent 4 `following` on a
    polyline with NaN padding (from S = 6 on) -> (plans [5,N,52,6] float32, yardstick term)."""
    rng = np.random.default_rng(SEEDS.get((S, N), S * 10 + N))
    A = 5
    lines = np.stack([make_line(rng, S) for _ in range(4)] + [make_line(rng, S, n_valid=S - 2 if S >= 6 else None), make_line(rng, S, left=True)])
    term = dict(agent=[1, 2, 2, 3, 4], line=[1, 5, 2, 3, 4], kind=["following", "change_left", "follow_decayed", "follow_decayed", "following"],
                decay=[0.0, 0.0, 0.9, 0.8, 0.0], scale=[0.5 / N, 2.0 / N, 30.0 / N, 20.0 / N, 0.25 / N], lines=torch.from_numpy(lines).double())
    return make_plans(rng, A, N, drifting=(3,)), term


def scenes_case(N=2, seed=77):
    """Two scenes of 33 and 37 agents, 40-point polylines (one current, one left per agent): every third agent carries no entry, every
    seventh two; the kinds rotate -> (plans [70,N,52,6], term)."""
    rng = np.random.default_rng(seed)
    A, S = 70, 40
    lines = np.stack([make_line(rng, S) for _ in range(A)] + [make_line(rng, S, left=True) for _ in range(A)])
    term = dict(agent=[], line=[], kind=[], decay=[], scale=[], lines=torch.from_numpy(lines).double())
    drifting = []
    for a in range(A):
        if a % 3 == 0:
            continue
        kinds = [Y.KINDS[(a + k) % 3] for k in range(2 if a % 7 == 0 else 1)]
        for kind in kinds:
            if kind == "follow_decayed" and a % 2:
                drifting.append(a)
            for k, v in (("agent", a), ("line", a + (A if kind == "change_left" else 0)), ("kind", kind), ("decay", 0.85 if kind == "follow_decayed" else 0.0),
                         ("scale", {"following": 0.5, "change_left": 2.0, "follow_decayed": 25.0}[kind] / N)):
                term[k].append(v)
    return make_plans(rng, A, N, drifting=drifting), term


def conditions(plans, term):
    """-> (fraction of near-tie elements, per kind the number of (entry, sample) rows free of them, the smallest kink margin on those
    rows, the mask [E,N] of the checked rows)."""
    _, gap = Y.projections(plans.double(), term)
    near = gap < NEAR
    rows = ~near.any(dim=-1)
    per_kind = {k: int(sum(int(rows[e].sum()) for e in range(len(term["agent"])) if term["kind"][e] == k)) for k in Y.KINDS}
    kink = float("inf")
    with torch.no_grad():
        for e in range(len(term["agent"])):
            for q, bound in Y._entry(plans.double(), term, e)[3]:
                m = (q - bound).abs()[rows[e]]
                if m.numel():
                    kink = min(kink, float(m.min()))
    return float(near.double().mean()), per_kind, kink, rows
