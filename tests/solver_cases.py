"""The cases of the few-step sampler tests (tests/test_solver_host.py on the CPU, tests/test_gpu_solver.py on the GPU), built on the CPU so
that the host test can assert what they claim without a GPU.  A plain module; references are computed once and shared -- do not write
to what it returns.

STEP CASES.  Two timestep lists hold the step pairs the tests ask for.  "top" = 99, 88, 0: k = 0 is 99 -> 88 (a first step), k = 1 a
middle step with history, k = 2 an output step.  "low" = 60, 50, 45, 22, 11, 0: k = 1 is 50 -> 45 and k = 4 is 11 -> 0 (middle steps
with history), k = 5 is 0 -> end (the output step).  The inputs of step k are what a float64 DPM-Solver++(2M) chain from X_T SEES
there -- its x_t and the x0_hat of its preceding step, both rounded to float32 -- so every x0_prev comes from a real preceding step; the
DDIM cases take the same x_t.  One chain per list and CFG setting at 37 rows; every input is a pure function of (seed, name, row) and
the U-Net treats rows independently, so the cases at 1, 5 and 33 rows are the first rows of it.
Why two lists: with synthetic weights the clean prediction at t = 99 is sqrt(1 / acp_99) = 2,029 times (x - eps), about 9e3, and every
later x0_hat of that chain repeats it to four digits -- the second-order correction, a multiple of x0_hat_k - x0_hat_{k-1}, then drowns in
the float32 rounding of a latent of 9e3 on the small 50 -> 45 step (2.6 x the bar), and no test could tell 2M from DDIM there.  A chain that
starts at t = 60 keeps O(1) latents, and consecutive clean predictions of an untrained denoiser differ by O(1).

GUIDED CASES.  Inputs from tests/guide_cases.py (rows of its regime batch: cond, curr_states, target_speed with its NaN rows, loss_scale
with its zero rows, z; x_t = its `mean` halved: unit scale, as a latent at t = 50 has) with the cool decoder; the collision scene of 12
rows is the one of tests/recon_cases.py.  GUIDE_TS = 50, 45, 0: k = 0 is an intermediate step (first order in both kinds: no history
needed), k = 2 the output step.  SGD runs with the clip at sigma^g and an explicit learning rate -- sigma^g over the 75th percentile of
|dL/dmu| in float64, two significant digits, written down in SGD_LR, so that a quarter of the elements is clipped (tests/test_solver_host.py
asserts 10 % .. 90 %); Adam runs as the reference's perturb() does, lr = sigma^g and no effective clip.  The output step takes
final_step_opt_params of its own (Adam lr 0.3 / SGD OUT_SGD_LR, no clip).
"""
import functools

import numpy as np
import torch

from cld_amd import synth
from tests import guide_cases as GC
from tests import recon_cases as RC
from tests import solver_yardstick as Y

T = 52
N_T = 100
GW = 2.0                                    # the CFG weight
W_SEED = 3
SEED = 81
STEP_LISTS = {"top": (99, 88, 0), "low": (60, 50, 45, 22, 11, 0)}
STEP_PAIRS = (("top", 0), ("low", 1), ("low", 4), ("low", 5))       # 99 -> 88, 50 -> 45, 11 -> 0, 0 -> end
HISTORY_STEPS = (("top", 1), ("low", 1), ("low", 2), ("low", 3), ("low", 4))      # every second-order step of the two lists
BATCHES = (1, 5, 33, 37)
B_MAX = 37
VARIANTS = (("ddim", 0.0), ("ddim", 0.5), ("ddim", 1.0), ("dpmpp_2m", 0.0))
F = {"f64": torch.float64, "f32": torch.float32}

GUIDE_TS = (50, 45, 0)
GUIDE_VARIANTS = (("ddim", 0.5), ("dpmpp_2m", 0.0))
#              name          B   loss           cfg
GUIDED = {
    "ts_b5_cfg":   (5, "target_speed", True),
    "ts_b33":      (33, "target_speed", False),
    "col_b12_cfg": (12, "collision", True),
}
# explicit SGD learning rates of the intermediate step, see the module docstring: {(case, kind): lr}
SGD_LR = {
    ("ts_b5_cfg", "ddim"): 460.0, ("ts_b5_cfg", "dpmpp_2m"): 460.0, ("ts_b33", "ddim"): 680.0, ("ts_b33", "dpmpp_2m"): 680.0,
    # the collision gradient is zero on 77 % of the elements (four of the twelve rows meet nobody): sigma^g over the 40th percentile of
    # the others, so that 60 % of those -- 14 % of the case -- are clipped
    ("col_b12_cfg", "ddim"): 1.0e6, ("col_b12_cfg", "dpmpp_2m"): 1.0e6,
}
OUT_SGD_LR = 100.0


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def sampler(kind, eta, ts):
    return {"kind": kind, "timesteps": list(ts), "eta": eta}


@functools.lru_cache(maxsize=None)
def unet_weights():
    return synth.make_unet_weights(W_SEED, affine_jitter=True)


def decoder_weights():
    return GC.decoder_weights("cool")


def all_weights():
    w = dict(unet_weights())
    w.update(decoder_weights())
    return w


@functools.lru_cache(maxsize=None)
def step_inputs():
    """x_T, z [37,52,4], cond, non_cond [37,256] (float32 tensors)."""
    B = B_MAX
    return {"x_T": _t(synth.normal(SEED, "solver_xT", (B, T, 4))), "z": _t(synth.normal(SEED, "solver_z", (B, T, 4))),
            "cond": _t(synth.make_inputs(B, SEED)["cond_feat"]), "non_cond": _t(synth.make_inputs(B, SEED + 1000)["cond_feat"])}


@functools.lru_cache(maxsize=None)
def seen(lst: str, cfg: bool):
    """[(x_t, x0_prev)] float32, per step of STEP_LISTS[lst]: what the float64 2M chain sees, each step continuing from the ROUNDED x_t."""
    torch.set_num_threads(8)
    inp = step_inputs()
    x, prev, out = inp["x_T"], None, []
    for k in range(len(STEP_LISTS[lst])):
        out.append((x, prev))
        o = Y.step(unet_weights(), None, N_T, "dpmpp_2m", STEP_LISTS[lst], 0.0, k, x, prev, None, inp["cond"], inp["non_cond"] if cfg else None, GW if cfg else 0.0)
        x, prev = o["x_next"].float(), o["x0_hat"].float()
    return out


@functools.lru_cache(maxsize=None)
def step_reference(kind: str, eta: float, lst: str, cfg: bool, k: int, dtype_name: str):
    """Y.step of the 37-row case at a dtype: dict(x_next, x0_hat, mu, ...)."""
    torch.set_num_threads(8)
    inp = step_inputs()
    x, prev = seen(lst, cfg)[k]
    return Y.step(unet_weights(), None, N_T, kind, STEP_LISTS[lst], eta, k, x, prev, inp["z"], inp["cond"], inp["non_cond"] if cfg else None, GW if cfg else 0.0,
                  dtype=F[dtype_name])


# ------------------------------------------------------------------------------------------------------------- guided cases
@functools.lru_cache(maxsize=None)
def guided_inputs(name: str):
    """dict: x_t, z [B,52,4], cond, non_cond [B,256], curr_states; `terms`: what both guidance dicts share."""
    B, loss, cfg = GUIDED[name]
    if loss == "target_speed":
        g = GC.inputs(B)
        return {"x_t": g["mean"] * 0.5, "z": g["z"], "cond": g["cond"], "non_cond": _t(synth.make_inputs(B, GC.SEED + 1000)["cond_feat"]),
                "curr_states": g["curr_states"], "yard": dict(target_speed=g["target_speed"], loss_scale=g["loss_scale"]),
                "engine": dict(target_speed=g["target_speed"], loss_scale=g["loss_scale"])}
    r = RC.inputs(B, "collision", 74)
    return {"x_t": r["x_t"], "z": r["z"], "cond": r["cond"], "non_cond": r["non_cond"], "curr_states": r["curr_states"],
            "yard": dict(collision=r["losses"]["collision"]), "engine": dict(agent_collision=r["guidance"]["agent_collision"])}


def guidance_dicts(name: str, kind: str, optimizer: str):
    """(the guidance as tests/solver_yardstick.guide takes it, the same as Engine takes it)."""
    inp = guided_inputs(name)
    if optimizer == "sgd":
        opt = dict(lr=SGD_LR[(name, kind)], perturb_th="sigma", optimizer="sgd", output=dict(lr=OUT_SGD_LR, optimizer="sgd"))
    else:
        opt = dict(lr=None, perturb_th=None, optimizer="adam", output=dict(lr=0.3, optimizer="adam"))
    return dict(inp["yard"], curr_states=inp["curr_states"], **opt), dict(inp["engine"], curr_states=inp["curr_states"], **opt)


@functools.lru_cache(maxsize=None)
def guided_output_x(name: str, kind: str, eta: float):
    """The float32 x_t of the output step (k = 2) of a guided case: the float64 UNGUIDED chain's, rounded -- the output step is first
    order in both kinds, so it reads no history."""
    torch.set_num_threads(8)
    B, loss, cfg = GUIDED[name]
    inp = guided_inputs(name)
    x, prev = inp["x_t"], None
    for k in range(2):
        o = Y.step(unet_weights(), None, N_T, kind, GUIDE_TS, eta, k, x, prev, inp["z"], inp["cond"], inp["non_cond"] if cfg else None, GW if cfg else 0.0)
        x, prev = o["x_next"].float(), o["x0_hat"].float()
    return x


@functools.lru_cache(maxsize=None)
def guided_reference(name: str, kind: str, eta: float, optimizer: str, k: int, dtype_name: str):
    torch.set_num_threads(8)
    B, loss, cfg = GUIDED[name]
    inp = guided_inputs(name)
    gy, _ = guidance_dicts(name, kind, optimizer)
    x = inp["x_t"] if k == 0 else guided_output_x(name, kind, eta)
    return Y.step(unet_weights(), decoder_weights(), N_T, kind, GUIDE_TS, eta, k, x, None, inp["z"], inp["cond"], inp["non_cond"] if cfg else None,
                  GW if cfg else 0.0, gy, F[dtype_name])


def guided_x(name: str, kind: str, eta: float, k: int):
    return guided_inputs(name)["x_t"] if k == 0 else guided_output_x(name, kind, eta)


def bar(y64, y32, keep=None):
    d, s = (y32.double() - y64).abs(), y64.abs()
    if keep is not None:
        d, s = d[keep], s[keep]
    return 4 * float(d.max()) + 1e-7 * float(s.max())


def clip_ambiguous(r64, r32):
    """[B,52,4] bool: the elements of an SGD step whose float64 |delta| (unclipped: -lr g) lies within the bar of delta of the threshold,
    and the unclipped float64 delta."""
    if r64.get("th") is None:
        return torch.zeros_like(r64["mu"], dtype=torch.bool), None
    lr = r64["lr_eff"]
    d64, d32 = -lr * r64["grad"], -lr * r32["grad"].double()
    return ((d64.abs() - r64["th"]).abs() <= bar(d64, d32)), d64


# ------------------------------------------------------------------------------------------------------------- chains
CHAIN_B, CHAIN_K, CHAIN_SEED = 5, 10, 83


@functools.lru_cache(maxsize=None)
def chain_inputs():
    B = CHAIN_B
    return {"x_T": _t(synth.normal(CHAIN_SEED, "solver_xT", (B, T, 4))), "noise": _t(synth.normal(CHAIN_SEED, "solver_noise", (CHAIN_K, B, T, 4))),
            "cond": _t(synth.make_inputs(B, CHAIN_SEED)["cond_feat"]), "non_cond": _t(synth.make_inputs(B, CHAIN_SEED + 1000)["cond_feat"])}


@functools.lru_cache(maxsize=None)
def free_chain(kind: str, dtype_name: str):
    """x0 of the K = 10 chain on solver_timesteps(100, 10) (DDIM: eta = 0), B = 5, no CFG."""
    torch.set_num_threads(8)
    from cld_amd.dm_model import solver_timesteps
    c = chain_inputs()
    x0, _ = Y.chain(unet_weights(), None, N_T, kind, solver_timesteps(N_T, CHAIN_K), 0.0, c["x_T"], None, c["cond"], dtype=F[dtype_name])
    return x0
