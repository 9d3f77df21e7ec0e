"""The cases of the agent-collision regime tests (tests/test_gpu_collision_regimes.py), built on the CPU so that
tests/test_collision_host.py can assert what they claim without a GPU, and the check both modules apply: the kernel on the GPU, the
yardstick's mutants on the CPU.

The kernel (csrc/collision_kernels.hip): a workgroup owns kOwn = 4 agents of one (scene, sample), grid.y is sized from the largest scene
(workgroups past a smaller scene's end return early), the scene's poses sit in LDS, 160 KiB at the most: 192 agents.  Cases:
  sizes_n1, sizes_n3   scenes of 1, 3, 4, 5, 8, 9 agents in one batch (a lone agent; last workgroups owning 3, 4, 1, 4, 1 agents; early returns)
  lds_cap              one scene of 192 agents: 163,664 of the 163,840 bytes
  disks_1 .. disks_8   num_disks 1, 2, 4, 5, 8 on scenes of 33 and 17 agents 2 m apart (odd and even linspace, the single disk)
  buffer_*, decay_*    buffer_dist 0, 0.2 (params_base), 1.0; decay_rate 1.0, 0.9 (params_base), 0.5
  speed_th             guide_moving_speed_th = 4 m/s: a third of the agents stationary -- value 0, gradient 0, still obstacles
  wide                 pedestrians wider than long (0.6 x 0.7 m), square agents (0.7 x 0.7 m) and vehicles in one scene
  frames               headings in all four quadrants and on both sides of +-pi, world positions near (1500, 900) m
  masks                a guided subset, a scene of weight 0 between two guided ones, excluded_agents
  kink_inside/outside  a constructed pair whose closest disks are inside / outside the bound by 1e-3 of it
  exact_tie            two parallel agents whose five disk pairs are equidistant in exact arithmetic: the FIRST minimum's lever arm
"""
import functools

import numpy as np
import torch

from cld_amd import synth
from tests import collision_yardstick as Y
from tests import grad_bar

SIZES = [1, 3, 4, 5, 8, 9]
LDS_CAP = 192
KINK_MARGIN = 1e-3
OFFSET = (1500.0, 900.0)
# float32 world coordinates below 2048 m are 2^-13 m apart: a world position carries up to two half-ulp roundings (1.2e-4 m), the
# difference of two positions 2.4e-4 m per coordinate, a disk distance 3.5e-4 m.  `frames` keeps its unflagged pairs further than this from
# the bound; between two disk pairs of one agent pair the position error is common and cancels to first order, half of it is kept.
F32_KINK, F32_TIE = 4e-4, 2e-4
# 16 x 2^-24: a gradient element of `exact_tie` is a chain of fewer than 16 float32 operations on exactly representable geometry
EXACT_BAR = 16 * 2.0 ** -24


def make_term(sc, sizes, weight=1.0, **kw):
    term = dict(extent=torch.from_numpy(np.asarray(sc["extent"], np.float32)), world_from_agent=torch.from_numpy(np.asarray(sc["world_from_agent"], np.float32)),
                curr_speed=torch.from_numpy(np.asarray(sc["curr_speed"], np.float32)), sizes=list(sizes), weight=weight, agents=None, excluded_agents=None,
                num_disks=5, buffer_dist=0.2, decay_rate=0.9, guide_moving_speed_th=0.5)
    term.update(kw)
    return term


def synth_case(sizes, N, seed, spacing, weight=1.0, **kw):
    """synth.make_collision_scene / make_collision_trajectories: vehicles on a jittered grid, heading about the same way."""
    B = sum(sizes)
    sc = synth.make_collision_scene(sizes, seed, spacing=spacing)
    plans = torch.from_numpy(synth.make_collision_trajectories(B, N, sc["curr_speed"], seed))
    return plans, make_term(sc, sizes, weight, **kw)


def frames_of(pos, th):
    W = np.zeros((len(th), 3, 3))
    W[:, 0, 0], W[:, 0, 1], W[:, 1, 0], W[:, 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    W[:, :2, 2], W[:, 2, 2] = pos, 1.0
    return W


def wide_case(N=2, seed=11):
    """One scene: 10 pedestrians of 0.6 x 0.7 m (wider than long: the half extent of their disk centres is -0.05 m) and 3 square agents of
    0.7 x 0.7 m (all disks on the centre) about 0.85 m apart, walking the same way at 0.8 .. 1.6 m/s, with 4 vehicles around them."""
    rng = np.random.default_rng(seed)
    n_ped, n_sq, n_veh = 10, 3, 4
    A = n_ped + n_sq + n_veh
    ext = np.zeros((A, 3), np.float32)
    ext[:n_ped] = (0.6, 0.7, 1.7); ext[n_ped:n_ped + n_sq] = (0.7, 0.7, 1.7)
    ext[n_ped + n_sq:] = np.stack([rng.uniform(3.8, 5.2, n_veh), rng.uniform(1.7, 2.2, n_veh), np.full(n_veh, 1.6)], axis=1)
    th0 = 0.6
    k = rng.permutation(n_ped + n_sq)
    along, across = 0.85 * (k // 3), 0.95 * (k % 3)                     # files of walkers one behind another, 0.85 m apart
    walkers = np.stack([along * np.cos(th0) - across * np.sin(th0), along * np.sin(th0) + across * np.cos(th0)], axis=1) + rng.uniform(-0.04, 0.04, (n_ped + n_sq, 2))
    veh = np.array([[5.5, 2.0], [-3.0, -1.0], [1.0, -2.6], [0.5, 5.2]]) + rng.uniform(-0.3, 0.3, (n_veh, 2))
    pos = np.concatenate([walkers, veh])
    th = th0 + rng.uniform(-0.25, 0.25, A)
    speed = np.concatenate([rng.uniform(0.8, 1.6, n_ped + n_sq), rng.uniform(2.0, 8.0, n_veh)]).astype(np.float32)
    speed[[4, A - 1]] = 0.2
    sc = dict(extent=ext, world_from_agent=frames_of(pos, th), curr_speed=speed)
    plans = synth.make_collision_trajectories(A, N, speed, seed)
    plans[:n_ped + n_sq, ..., :2] *= 0.35                               # walkers keep their pace: the files stay together over the horizon
    return torch.from_numpy(plans), make_term(sc, [A], 1.0)


def frames_case(N=2, seed=1):
    """Five scenes of 4 agents 2.5 m apart near (1500, 900) m: scene headings 0.8, 2.4, -2.4, -0.8 (+- 0.25) and pi (+- 0.04, on both sides
    of the branch cut of atan2); the frames of the second scene are mirrored (y to the right), the only place where the factor
    d heading / d yaw is not 1."""
    rng = np.random.default_rng(seed)
    sizes = [4, 4, 4, 4, 4]
    A = sum(sizes)
    base = np.repeat([0.8, 2.4, -2.4, -0.8, np.pi], 4)
    th = base + np.where(base > 3.0, rng.uniform(-0.04, 0.04, A), rng.uniform(-0.25, 0.25, A))
    th[16], th[17] = np.pi - 0.03, -np.pi + 0.02
    kk = np.tile(np.arange(4), 5)
    pos = np.stack([60.0 * np.repeat(np.arange(5), 4) + 2.5 * (kk % 2), 2.5 * (kk // 2)], axis=1) + rng.uniform(-0.6, 0.6, (A, 2)) + np.asarray(OFFSET)
    speed = rng.uniform(1.0, 12.0, A).astype(np.float32)
    speed[::7] = 0.2
    ext = np.stack([rng.uniform(3.8, 5.2, A), rng.uniform(1.7, 2.2, A), np.full(A, 1.6)], axis=1).astype(np.float32)
    W = frames_of(pos, th)
    W[4:8, :2, 1] *= -1.0                                                 # scene 1: left-handed agent frames (det = -1), d heading / d yaw = -1
    sc = dict(extent=ext, world_from_agent=W, curr_speed=speed)
    plans = synth.make_collision_trajectories(A, N, speed, seed + 100)
    return torch.from_numpy(plans), make_term(sc, sizes, [1.0, 0.6, 1.4, 2.0, 0.8])


def closest_disks(W, ext, num_disks=5):
    """Smallest disk-centre distance of agents 0 and 1 standing at their frames' origins, float64."""
    cx = Y.disk_centres(torch.as_tensor(ext, dtype=torch.float64), num_disks).numpy()
    c = [W[b, :2, 2][None, :] + cx[b][:, None] * W[b, :2, 0][None, :] for b in (0, 1)]
    return float(np.linalg.norm(c[0][:, None, :] - c[1][None, :, :], axis=-1).min())


def kink_case(side, N=2):
    """Agent 0 at the origin, agent 1 beside it, turned by 0.3 rad, at the lateral offset that puts their closest disks at
    pd (1 - side 1e-3) (bisection in float64; side = +1 inside, -1 outside), agent 2 on the other side overlapping agent 0.  All three drive at
    the same world velocity, so the geometry holds over the 52 steps."""
    ext = np.array([[4.5, 2.0, 1.6], [4.2, 1.8, 1.6], [4.8, 2.1, 1.6]], np.float32)
    pd = 1.0 + 0.9 + 0.2
    target = pd * (1.0 - side * KINK_MARGIN)
    th = np.array([0.0, 0.3, -0.2])

    def frames(y):
        return frames_of(np.array([[0.0, 0.0], [0.4, y], [-0.3, -1.5]]), th)
    lo, hi = 1.0, 6.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if closest_disks(frames(mid), ext) < target else (lo, mid)
    W = frames(hi)
    plans = np.zeros((3, N, 52, 6), np.float32)
    s = 0.25 * (np.arange(52) + 1)                                        # 2.5 m/s along world x: exactly representable steps
    for b in range(3):
        for n in range(N):
            plans[b, n, :, 0], plans[b, n, :, 1] = s * np.cos(th[b]) * (1 + n), -s * np.sin(th[b]) * (1 + n)
            plans[b, n, :, 2] = 2.5 * (1 + n)
    sc = dict(extent=ext, world_from_agent=W, curr_speed=np.array([2.5, 2.5, 2.5], np.float32))
    return torch.from_numpy(plans), make_term(sc, [3], 1.0)


def exact_tie_case():
    """Two 4 x 2 m agents side by side 2 m apart, both heading along world x at the same speed, identity rotations: the disk pairs
    (a, a), a = 0 .. 4, are 2 m apart in exact arithmetic and every float32 operation up to the comparison is exact, so nothing is left to
    rounding: the first minimum is disk 0, whose lever arm is -1 m (the last one's is +1 m)."""
    ext = np.array([[4.0, 2.0, 1.6], [4.0, 2.0, 1.6]], np.float32)
    W = frames_of(np.array([[8.0, 3.0], [8.0, 5.0]]), np.zeros(2))
    plans = np.zeros((2, 1, 52, 6), np.float32)
    plans[..., 0] = 0.5 * (np.arange(52) + 1)
    plans[..., 2] = 5.0
    sc = dict(extent=ext, world_from_agent=W, curr_speed=np.array([5.0, 5.0], np.float32))
    return torch.from_numpy(plans), make_term(sc, [2], 1.0, decay_rate=1.0)


def masks_case(N=2, seed=5):
    """Scenes of 7, 6 and 9 agents: the first guides agents 0, 2, 3, 5 only, the second has weight 0, the third guides all; agents 1, 2 (scene 0),
    8 (scene 1) and 14, 15, 17 (scene 2) are excluded_agents."""
    return synth_case([7, 6, 9], N, seed, 2.5, weight=[1.5, 0.0, 0.8], agents={0: [0, 2, 3, 5]}, excluded_agents=[1, 2, 8, 14, 15, 17])


# name -> (builder, random: held to the 5 % cap on flagged elements)
CASES = {
    "sizes_n1": (lambda: synth_case(SIZES, 1, 21, 2.5, weight=[1.0, 0.5, 2.0, 1.5, 1.0, 0.7]), True),
    "sizes_n3": (lambda: synth_case(SIZES, 3, 23, 2.5, weight=[1.0, 0.5, 2.0, 1.5, 1.0, 0.7]), True),
    "lds_cap": (lambda: synth_case([LDS_CAP], 1, 41, 3.0), True),
    "disks_1": (lambda: synth_case([33, 17], 2, 31, 2.0, weight=[1.0, 2.0], num_disks=1), True),
    "disks_2": (lambda: synth_case([33, 17], 2, 32, 2.0, weight=[1.0, 2.0], num_disks=2), True),
    "disks_4": (lambda: synth_case([33, 17], 2, 33, 2.0, weight=[1.0, 2.0], num_disks=4), True),
    "disks_5": (lambda: synth_case([33, 17], 2, 34, 2.0, weight=[1.0, 2.0], num_disks=5), True),
    "disks_8": (lambda: synth_case([33, 17], 2, 35, 2.0, weight=[1.0, 2.0], num_disks=8), True),
    "params_base": (lambda: synth_case([12, 7], 2, 51, 2.5), True),
    "buffer_0": (lambda: synth_case([12, 7], 2, 51, 2.5, buffer_dist=0.0), True),
    "buffer_1": (lambda: synth_case([12, 7], 2, 51, 2.5, buffer_dist=1.0), True),
    "decay_1": (lambda: synth_case([12, 7], 2, 51, 2.5, decay_rate=1.0), True),
    "decay_05": (lambda: synth_case([12, 7], 2, 51, 2.5, decay_rate=0.5), True),
    "speed_th": (lambda: synth_case([12, 7], 2, 51, 2.5, guide_moving_speed_th=4.0), True),
    "wide": (wide_case, True),
    "frames": (frames_case, True),
    "masks": (masks_case, True),
    "kink_inside": (lambda: kink_case(+1), False),
    "kink_outside": (lambda: kink_case(-1), False),
    "exact_tie": (exact_tie_case, False),
}
NAMES = list(CASES)
SMALL = [n for n in NAMES if n not in ("lds_cap",) and not n.startswith("disks_")] + ["disks_2"]      # what the oracle's table handles quickly


def engine_cfg(term, N):
    """The term as Engine.agent_collision takes it."""
    return dict(extent=term["extent"], world_from_agent=term["world_from_agent"], curr_speed=term["curr_speed"], scene_sizes=term["sizes"],
                weight=term["weight"], agents=term["agents"], excluded_agents=term["excluded_agents"], num_samp=N, num_disks=term["num_disks"],
                buffer_dist=term["buffer_dist"], decay_rate=term["decay_rate"], guide_moving_speed_th=term["guide_moving_speed_th"])


def oracle_col(term, dtype):
    """The term as oracle.cld_oracle.scene_collision_total takes it, its float tensors in `dtype`."""
    S = len(term["sizes"])
    wts = term["weight"] if isinstance(term["weight"], (list, tuple)) else [term["weight"]] * S
    col = dict(extent=term["extent"].to(dtype), world_from_agent=term["world_from_agent"].to(dtype), curr_speed=term["curr_speed"].to(dtype),
               scene_index=torch.repeat_interleave(torch.arange(S), torch.tensor(term["sizes"])), scene_weight=list(wts), agents=term["agents"],
               num_disks=term["num_disks"], buffer_dist=term["buffer_dist"], decay_rate=term["decay_rate"], moving_speed_th=term["guide_moving_speed_th"])
    if term["excluded_agents"] is not None:
        col["excluded_agents"] = term["excluded_agents"]
    return col


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (plans [B,N,52,6] float32, term, the yardstick in float64 with its record, the yardstick in float32); computed once, not to be
    modified."""
    plans, term = CASES[name][0]()
    return plans, term, Y.run(plans.double(), term, record=True), Y.run(plans, term)


def quiet_rows(term, B):
    """[B] bool: agents that receive no gradient whatever the plans -- stationary, not guided, or alone in their scene."""
    scenes, _ = Y.scene_masks(term, B)
    moving = term["curr_speed"].abs() > term["guide_moving_speed_th"]
    quiet = torch.ones(B, dtype=torch.bool)
    for a0, A, _, guided in scenes:
        quiet[a0:a0 + A] = ~(guided & moving[a0:a0 + A]) | (A == 1)
    return quiet


def ratios(name, values, grad):
    """What both test modules hold a result (values [B N], grad [B N,52,6]) to -> {check: error over its bar}; a result passes when
    every ratio is <= 1.
      values, grad_x, grad_y, grad_yaw   tests/grad_bar.ratio over the unflagged elements (the values: all of them), per tensor
                                         max|got - ref64| <= 4 max|ref32 - ref64| + 1e-7 max|ref64|
      interval                           flagged elements: how far outside [lo, hi], over the same bar of the channel
      exact                              exact_tie only: its tied elements against the first minimum's gradient, over EXACT_BAR max|ref64|"""
    plans, term, r64, r32 = reference(name)
    B, N = plans.shape[:2]
    got_v = torch.as_tensor(values).double().cpu().reshape(B, N)
    got_g = torch.as_tensor(grad).double().cpu().reshape(B, N, 52, 6)
    g64, g32 = r64["grad"].reshape(B, N, 52, 6), r32["grad"].double().reshape(B, N, 52, 6)
    free = ~r64["flagged"]
    out = {"values": grad_bar.ratio(got_v, r64["values"], r32["values"])}
    worst_out = 0.0
    for k, (ch, label) in enumerate(((0, "grad_x"), (1, "grad_y"), (3, "grad_yaw"))):
        a, b, c = got_g[..., ch], g64[..., ch], g32[..., ch]
        out[label] = grad_bar.ratio(a[free], b[free], c[free]) if bool(free.any()) else 0.0
        if bool(r64["flagged"].any()):
            bar = 4 * float((c[free] - b[free]).abs().max()) + 1e-7 * float(b[free].abs().max()) if bool(free.any()) else 0.0
            bar = max(bar, 1e-7 * float(b.abs().max()))
            off = torch.maximum(r64["lo"][..., k] - a, a - r64["hi"][..., k]).clamp(min=0)[r64["flagged"]]
            worst_out = max(worst_out, float(off.max()) / bar if bar > 0 else (0.0 if float(off.max()) == 0 else float("inf")))
    out["interval"] = worst_out
    if name == "exact_tie":
        ch = [0, 1, 3]
        out["exact"] = float((got_g[..., ch] - g64[..., ch]).abs().max()) / (EXACT_BAR * float(g64.abs().max()))
    return out
