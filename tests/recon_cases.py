"""The cases of the reconstruction-guidance tests (tests/test_recon_host.py on the CPU, tests/test_gpu_recon.py on the GPU), built on the
CPU so that the host test can assert what they claim without a GPU.  A plain module.

A CORE is what steps 1-4 of the guided step depend on -- batch size, timestep, CFG on / off, the loss set, the seed -- and costs one
autograd pass through the U-Net per dtype; a VARIANT is what steps 5-7 add: the sign (`descend` 0 / 1) and the clip mode ("sigma":
perturb_th None, th_t = sigma_t; "sched": perturb_th = 1.0, upstream's sigmoid schedule; "none": no clip).  Every core runs under all six
variants; references are computed once per core and dtype and shared.

Batch sizes 1, 5, 33, 37: the sizes tests/test_gpu_train.py uses where the launch logic of the U-Net's training path changes; here they
also make 1 / 2 / 7 / 8 workgroups of the three elementwise kernels, the last one ragged in each.  Timesteps 99, 50, 1.  Loss sets:
  builtin    target_speed + speed_limit + target_pos (TargetPosAtTimeLoss on even rows, TargetPosLoss on odd rows), per-agent scales
  collision  agent_collision on 2 scenes x 3 agents x 2 samples (12 rows, sample-minor)
  pair       one handle-set term: two gptkeepdistance pairs among 5 agents, one of them with a decay
Every input is a pure function of (seed, name, row), so a row means the same in every batch size.

The learning rate.  With lr = None (sigma_t) the step is sigma_t * g, and whether the clip bites is decided by |g| alone; to have every clip
case both clipped and unclipped elements (tests/test_recon_host.py asserts at least 10 % of each) the two clipping variants take the
explicit lr of LR_CLIP: th_t over the 75th percentile of |dL/dx_t| of the core in float64, two significant digits, written down here, so
that a quarter of the elements is clipped.  (Not the median: the collision and pair gradients span four decades, and a larger lr
stretches the float32 yardstick's error on the largest elements to a band around th_t that swallows several per cent of the case.)
The "none" variant runs with lr = None, the path upstream's evaluation preset takes.
"""
import functools

import numpy as np
import torch

from cld_amd import synth
from tests import collision_cases as CC
from tests import pair_cases as PC
from tests import recon_yardstick as RY

T = 52
N_T = 100
W_SEED = 3
GW = 2.0                         # the CFG weight
SPEED_LIMIT = 6.0
PERTURB_TH = 1.0                 # of the "sched" variant

#        name              B   t   cfg    loss set     seed
CORES = {
    "b1_t99":            (1, 99, False, "builtin", 71),
    "b5_t50_cfg":        (5, 50, True, "builtin", 71),
    "b33_t1_cfg":        (33, 1, True, "builtin", 71),
    "b37_t50":           (37, 50, False, "builtin", 71),
    "col_t50_cfg":       (12, 50, True, "collision", 74),
    "col_t1":            (12, 1, False, "collision", 74),
    "pair_t99_cfg":      (5, 99, True, "pair", 73),
    "pair_t50":          (5, 50, False, "pair", 73),
}
VARIANTS = [(descend, clip) for descend in (0, 1) for clip in ("sigma", "sched", "none")]
CLIP_ARG = {"sigma": None, "sched": PERTURB_TH, "none": "none"}       # as Engine._recon and recon_yardstick.threshold take it
# explicit learning rates of the clipping variants, see the module docstring: {core: (lr for "sigma", lr for "sched")}
LR_CLIP = {
    "b1_t99": (120.0, 480.0), "b5_t50_cfg": (200.0, 4600.0), "b33_t1_cfg": (19.0, 1100.0), "b37_t50": (120.0, 2800.0),
    "col_t50_cfg": (3.4e5, 7.7e6), "col_t1": (1.5e6, 8.6e7), "pair_t99_cfg": (530.0, 2100.0), "pair_t50": (1.2e4, 2.8e5),
}
COLLISION_SIZES, COLLISION_SAMPLES = [3, 3], 2
PAIR_AGENTS = 5


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def unet_weights():
    return synth.make_unet_weights(W_SEED, affine_jitter=True)


@functools.lru_cache(maxsize=None)
def decoder_weights():
    return synth.make_decoder_weights(0)


def all_weights():
    w = dict(unet_weights())
    w.update(decoder_weights())
    return w


@functools.lru_cache(maxsize=None)
def collision_term(seed):
    sc = synth.make_collision_scene(COLLISION_SIZES, seed, spacing=3.5)
    sc["curr_speed"] = np.maximum(sc["curr_speed"], np.float32(2.0))            # everybody moves: every agent carries a gradient
    return CC.make_term(sc, COLLISION_SIZES, weight=1.0)


@functools.lru_cache(maxsize=None)
def pair_term(seed):
    """Agents 2 .. 3 m apart on a line, heading about the same way; agent 4 sits in no pair."""
    k = np.arange(PAIR_AGENTS)
    pos = np.stack([2.5 * k, 0.4 * k], axis=1) + synth.uniform(seed, "recon_pair_pos", (PAIR_AGENTS, 2), -0.3, 0.3)
    W = PC.frames_of(pos, synth.uniform(seed, "recon_pair_th", (PAIR_AGENTS,), -0.3, 0.3).astype(np.float64))
    return dict(target=[0, 3], ref=[1, 2], kind=["keep_distance", "keep_distance"], lo=[4.0, 1.0], hi=[9.0, 2.0], decay=[0.0, 0.9],
                scale=[1.0, 0.5], world_from_agent=W, agent_from_world=None)


@functools.lru_cache(maxsize=None)
def inputs(B: int, loss: str, seed: int):
    """dict: x_t, z [B,52,4], cond, non_cond [B,256], curr_states [B,4] (float32 tensors); `losses` as recon_yardstick.total takes them;
    `guidance`: the same as Engine takes it (without the reconstruction entry).  Do not write to the result."""
    u = lambda name, shape, lo, hi: synth.uniform(seed, name, shape, lo, hi)
    out = {"x_t": _t(synth.normal(seed, "recon_xt", (B, T, 4))), "z": _t(synth.normal(seed, "recon_z", (B, T, 4))),
           "cond": _t(synth.make_inputs(B, seed)["cond_feat"]), "non_cond": _t(synth.make_inputs(B, seed + 1000)["cond_feat"])}
    cs = synth.make_inputs(B, seed)["curr_states"]
    if loss == "builtin":
        row = np.arange(B)
        when = np.floor(u("recon_tp_time", (B,), 0.0, 51.999)).astype(np.int64)
        when = np.where(row % 2 == 0, when, -(when + 1))
        b = dict(target_speed=_t(u("recon_ts", (B, T), 0.0, 12.0)), loss_scale=_t(u("recon_ls", (B,), 0.5, 1.5) / np.float32(T)),
                 speed_limit=(SPEED_LIMIT, _t(u("recon_sl", (B,), 0.5, 1.5) / np.float32(T))),
                 target_pos=(_t(np.stack((u("recon_wp_x", (B,), -5.0, 25.0), u("recon_wp_y", (B,), -8.0, 8.0)), axis=1)), _t(when),
                             _t(u("recon_tp", (B,), 0.5, 1.5) / np.float32(32.0))))
        out["losses"] = {"builtin": b}
        out["guidance"] = dict(b)
    elif loss == "collision":
        term, N = collision_term(seed), COLLISION_SAMPLES
        assert B == sum(COLLISION_SIZES) * N
        cs = np.zeros((B, 4), np.float32)
        cs[:, 2] = np.repeat(term["curr_speed"].numpy(), N)
        out["losses"] = {"collision": (CC.oracle_col(term, torch.float64), N)}
        out["guidance"] = {"agent_collision": CC.engine_cfg(term, N)}
    else:
        term = pair_term(seed)
        assert loss == "pair" and B == PAIR_AGENTS
        cs[:, 2] = np.minimum(cs[:, 2], np.float32(6.0))
        out["losses"] = {"pair": (term, 1)}
        out["guidance"] = {"pair": dict(target=term["target"], ref=term["ref"], kind=term["kind"], lo=term["lo"], hi=term["hi"], decay=term["decay"],
                                        scale=term["scale"], world_from_agent=term["world_from_agent"].float(), agent_from_world=None, num_samp=1)}
    out["curr_states"] = _t(cs)
    out["guidance"]["curr_states"] = out["curr_states"]
    return out


def core_inputs(name):
    B, t, cfg, loss, seed = CORES[name]
    return inputs(B, loss, seed)


@functools.lru_cache(maxsize=None)
def core(name: str, dtype_name: str):
    """recon_yardstick.core of the case in "f64" or "f32"; computed once.  Do not write to the result."""
    torch.set_num_threads(8)
    B, t, cfg, loss, seed = CORES[name]
    inp = core_inputs(name)
    return RY.core(unet_weights(), decoder_weights(), N_T, t, inp["x_t"], inp["cond"], inp["non_cond"] if cfg else None, GW, inp["curr_states"],
                   inp["losses"], {"f64": torch.float64, "f32": torch.float32}[dtype_name])


def lr_of(name: str, clip: str):
    return None if clip == "none" else LR_CLIP[name][0 if clip == "sigma" else 1]


def reference(name: str, descend: int, clip: str, dtype_name: str):
    """(core, update) of one case at a dtype."""
    B, t, cfg, loss, seed = CORES[name]
    inp = core_inputs(name)
    dtype = {"f64": torch.float64, "f32": torch.float32}[dtype_name]
    c = core(name, dtype_name)
    return c, RY.update(c, N_T, t, inp["x_t"], inp["z"], lr_of(name, clip), CLIP_ARG[clip], bool(descend), dtype)


def engine_guidance(name: str, descend: int, clip: str, params):
    """The guidance dict of one case as Engine.recon_step / Engine.sample take it."""
    g = dict(core_inputs(name)["guidance"])
    g["reconstruction"] = dict(params=params, lr=lr_of(name, clip), perturb_th=CLIP_ARG[clip], descend=bool(descend))
    return g


# ------------------------------------------------------------------------------------------------------------- chains (10 timesteps)
CHAIN_N, CHAIN_B, CHAIN_SEED = 10, 4, 75
DIRECTION_LR = 300.0             # explicit: with lr = sigma_t the step is far too small to move the final loss visibly (tests/test_recon_host.py prints the three values)


@functools.lru_cache(maxsize=None)
def chain_inputs(B: int = CHAIN_B, seed: int = CHAIN_SEED, n: int = CHAIN_N):
    """dict: x_T [B,52,4], noise [n,B,52,4], cond, non_cond, curr_states and the target-speed term (weight 1 per agent) in both forms."""
    nz = synth.make_noise(B, n, seed)
    inp = synth.make_inputs(B, seed)
    b = dict(target_speed=_t(synth.uniform(seed, "recon_ts", (B, T), 0.0, 12.0)), loss_scale=torch.full((B,), 1.0 / T))
    cs = _t(inp["curr_states"])
    return {"x_T": _t(nz["x_T"]), "noise": _t(nz["noise"]), "cond": _t(inp["cond_feat"]), "non_cond": _t(synth.make_inputs(B, seed + 1000)["cond_feat"]),
            "curr_states": cs, "losses": {"builtin": b}, "guidance": dict(b, curr_states=cs)}


@functools.lru_cache(maxsize=None)
def direction_reference():
    """The float64 yardstick's 10-step chains under DIRECTION_LR without a clip: {"descend" | "upstream" | "unguided": (mean target-speed
    loss of the final output, x_0)}."""
    torch.set_num_threads(8)
    c = chain_inputs()
    out = {}
    for key, descend, guided in (("descend", True, True), ("upstream", False, True), ("unguided", False, False)):
        x0, _ = RY.chain(unet_weights(), decoder_weights(), CHAIN_N, c["x_T"], c["noise"], c["cond"], None, 0.0, c["curr_states"], c["losses"],
                         DIRECTION_LR, "none", descend, torch.float64, guided=guided)
        out[key] = (RY.loss_of(decoder_weights(), x0, c["cond"], c["curr_states"], c["losses"], torch.float64), x0)
    return out
