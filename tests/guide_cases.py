"""Inputs and references of the guidance-kernel tests (tests/test_guide_host.py on the CPU, tests/test_gpu_guide.py on the GPU): the three
formulations of the guidance kernel in csrc/guide_kernels.hip (guide_kernel, guide_mfma8_kernel, guide_quad_kernel) with the roll-out
gradient they share (chain_grad / chain_grad_group).  A plain module.

Yardstick: dL/dmean by autograd over `oracle.cld_oracle.guidance_step` -- its own total(), with the decoder plugged in and the ext_grad
term -- in float64, and in float32 to calibrate the bar of tests/grad_bar.py ("f32": torch's gates; "f32fast": the gates as the two MFMA
kernels document them, vae_infer_cases.lstm2(fast=True)).  Every input is a pure function of (seed, name, row), so a row means the same in
every batch size, and the reference of a few rows of a large batch is the reference of those rows as a small batch.

Weight sets (seed 0 of synth.make_decoder_weights):
  cool    as they come: no gate saturates, no acceleration is clipped, the yaw rate stays far inside its bound; the speed is clipped only
          for the agents that start outside [v_lo, v_hi], which stay there for the whole horizon.
  hot     vae_infer_cases.DEC_HOT: recurrence x 4, output head x 30.  A third of the accelerations clipped, speeds run into v_hi and (from
          the agents that start backwards) into v_lo.  One clipped step moves the speed by 1 m/s, so no agent stays slow.
  steer   the hot set with its output head scaled once more: acceleration row x 0.005, yaw-rate row x 2.  Agents keep the speed they start
          with for the whole horizon (accelerations within +-0.1 m/s^2) while the yaw rate (+-1.5 rad/s) is clipped on half the steps: the
          only way to hold agents below |v| = 0.2, where the 0.1 floor of the yaw-rate bound is in force, and to reach each of the three
          regimes of the bound on many steps of the same agent.

Rows repeat in classes of eight by their starting speed (row % 8): 0 slow (|v| < 0.15, either sign), 1 fast (4.5 .. 34, above
v_hi = 30 at the end), 2 backwards (-16 .. -0.5, below v_lo = -10 at the end), 3 crawling (0.25 .. 1.6: bound 0.5 |v|), 4 .. 7 U[0, 15]
as synth.make_inputs.  Rows with row % 8 == 5 carry NaN target speeds on a third of their steps, rows with row % 8 == 6 a zero scale on every per-agent term; row % 5 picks the waypoint time (0: first
step, 1: last step, else in between) and the first step m of TargetPosLoss likewise.
"""
import functools
import math

import numpy as np
import torch

import vae_infer_cases as VC
from cld_amd import synth
from oracle import cld_oracle as O

T = 52
SEED = 45                        # of the regime batch (rows up to 64); chosen with BIG_SEED so that the kink caps of test_guide_host.py hold
BIG_SEED = 51                    # of the large batches
B_REG = 41                       # 21 VALU groups (last half empty), 6 quad groups (last: one agent), 3 MFMA groups (last: nine)
KINDS = ("cool", "hot", "steer")
STEER = (0.005, 2.0)             # the hot set's lstm_dec.hid2act.* once more: (acceleration row, yaw-rate row)
CASES = ("target_speed", "speed_limit", "acc_limit", "waypoint", "target_pos", "ext_grad", "combined")
SPEED_LIMIT = 6.0
ACC_LIMIT = {"cool": 0.05, "hot": 3.0, "steer": 0.02}      # inside the range of each set's accelerations
LR = 1.0
GROUP = {"valu": 2, "quad": 8, "mfma": 16}                # agents per workgroup
GRID = {"valu": 512, "quad": 256, "mfma": 256}            # workgroups at most: groups per grid-stride pass
# (form, rows, passes, the form with fewer passes at that size); "auto" takes the 16-agent kernel above 2,048 rows
BIG_CASES = (("valu", 1025, 2, "quad"), ("valu", 2051, 3, "quad"), ("quad", 2049, 2, "mfma"), ("quad", 4100, 3, "mfma"),
             ("mfma", 4097, 2, "quad"), ("auto", 4097, 2, "quad"))
MIN_PAIRS = 20
MIN_AGENTS = 3


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------------------- weights, inputs
@functools.lru_cache(maxsize=None)
def decoder_weights(kind: str):
    if kind in ("cool", "hot"):
        return VC.decoder_weights(kind)
    assert kind == "steer"
    w = dict(VC.decoder_weights("hot"))
    f = np.array(STEER, np.float32)
    w["lstm_dec.hid2act.weight"] = (w["lstm_dec.hid2act.weight"] * f[:, None]).astype(np.float32)
    w["lstm_dec.hid2act.bias"] = (w["lstm_dec.hid2act.bias"] * f).astype(np.float32)
    return w


@functools.lru_cache(maxsize=None)
def inputs(B: int):
    """dict of float32 tensors (target_time int64), row b the same for every B > b: mean [B,52,4] = 2 x unit normal, cond [B,256],
    curr_states [B,4], target_speed [B,52] (U[0,12], some NaN), loss_scale, sl_scale, al_scale, tp_scale [B], waypoint [B,2],
    time_at / time_from [B] (target_time of TargetPosAtTimeLoss / TargetPosLoss), row [B] (the row's index in the batch), ext_grad [B,52,6], z [B,52,4]."""
    seed = SEED if B <= 64 else BIG_SEED
    u = lambda name, shape, lo, hi: synth.uniform(seed, name, shape, lo, hi)
    row = np.arange(B)
    cls = row % 8
    v = u("cs_v", (B,), 0.0, 15.0)
    r = u("cs_class", (B,), 0.0, 1.0)
    v = np.where(cls == 0, -0.15 + 0.3 * r, np.where(cls == 1, 4.5 + 29.5 * r, np.where(cls == 2, -16.0 + 15.5 * r,
                 np.where(cls == 3, 0.25 + 1.35 * r, v)))).astype(np.float32)
    cs = np.stack((u("cs_x", (B,), -5.0, 5.0), u("cs_y", (B,), -5.0, 5.0), v, u("cs_yaw", (B,), -3.0, 3.0)), axis=1)
    tgt = u("target_speed", (B, T), 0.0, 12.0)
    tgt[(cls == 5)[:, None] & (u("target_nan", (B, T), 0.0, 1.0) < 0.33)] = np.nan
    live = (cls != 6).astype(np.float32)
    scale = lambda name, den: (u(name, (B,), 0.5, 1.5) / den * live).astype(np.float32)
    mid = np.floor(u("tp_time", (B,), 1.0, 50.999)).astype(np.int64)
    when = np.where(row % 5 == 0, 0, np.where(row % 5 == 1, T - 1, mid))
    egs = np.array([1.0, 1.0, 1.0, 1.0, 0.3, 1.0], np.float32) / T
    return {"mean": _t(synth.normal(seed, "guide_mean", (B, T, 4)) * np.float32(2.0)),
            "cond": _t(synth.make_inputs(B, seed)["cond_feat"]), "curr_states": _t(cs.astype(np.float32)),
            "target_speed": _t(tgt), "loss_scale": _t(scale("ts_scale", T)), "sl_scale": _t(scale("sl_scale", T)),
            "al_scale": _t(scale("al_scale", T)), "tp_scale": _t(scale("tp_scale", 32.0)),
            "waypoint": _t(np.stack((u("wp_x", (B,), -5.0, 25.0), u("wp_y", (B,), -8.0, 8.0)), axis=1)),
            "time_at": _t(when), "time_from": _t(-(when + 1)), "row": _t(row),
            "ext_grad": _t(synth.normal(seed, "ext_grad", (B, T, 6)) * egs), "z": _t(synth.normal(seed, "step_z", (B, T, 4)))}


def take(inp, rows):
    return inp if rows is None else {k: v[list(rows)] for k, v in inp.items()}


def terms(case: str, kind: str, inp):
    """The terms of a case as {"target_speed", "loss_scale", "speed_limit", "acc_limit", "target_pos", "ext_grad"} (absent: off).  The
    combined case takes the waypoint time on even rows and TargetPosLoss on odd rows (a row of the batch, not of a subset: `row`)."""
    on = lambda *names: case in names or case == "combined"
    out = {}
    if on("target_speed"):
        out["target_speed"], out["loss_scale"] = inp["target_speed"], inp["loss_scale"]
    if on("speed_limit"):
        out["speed_limit"] = (SPEED_LIMIT, inp["sl_scale"])
    if on("acc_limit"):
        out["acc_limit"] = (ACC_LIMIT[kind], inp["al_scale"])
    if on("waypoint", "target_pos"):
        when = {"waypoint": inp["time_at"], "target_pos": inp["time_from"]}.get(case)
        if when is None:
            when = torch.where(inp["row"] % 2 == 0, inp["time_at"], inp["time_from"])
        out["target_pos"] = (inp["waypoint"], when, inp["tp_scale"])
    if on("ext_grad"):
        out["ext_grad"] = inp["ext_grad"]
    return out


def guidance(case: str, kind: str, inp, **over):
    """The case as Engine.guidance_step takes it (SGD, lr 1, no clip unless `over` says otherwise)."""
    g = {"curr_states": inp["curr_states"], "lr": LR, "perturb_th": None, "optimizer": "sgd"}
    g.update(terms(case, kind, inp))
    g.update(over)
    return g


# ------------------------------------------------------------------------------------------------------------- references
class _CumsumF32(torch.autograd.Function):
    """A running sum carried in float32, forwards and backwards: what a kernel's sequential float sum does (torch.cumsum on the CPU
    carries a float32 sum in float64 and rounds each output once)."""
    @staticmethod
    def forward(ctx, x, dim):
        ctx.dim = dim
        return torch.from_numpy(np.cumsum(x.detach().numpy(), axis=dim, dtype=np.float32))

    @staticmethod
    def backward(ctx, g):
        r = np.flip(np.cumsum(np.flip(g.numpy(), axis=ctx.dim), axis=ctx.dim, dtype=np.float32), axis=ctx.dim)
        return torch.from_numpy(np.ascontiguousarray(r)), None


def _decoder(fast: bool, float_sums: bool = False):
    """The decoder O.guidance_step plugs in: None (its own), the MFMA kernels' gate forms, and / or float32 running sums."""
    if not fast and not float_sums:
        return None
    lstm = (lambda w, x, cond: VC.lstm_decode(w, x, cond, fast=True)) if fast else O.lstm_decode
    if not float_sums:
        return lambda w, x, cond, cs: O.action_to_state_and_action(lstm(w, x, cond), cs, True, True)
    return lambda w, x, cond, cs: VC.action_to_state(lstm(w, x, cond), cs, True, True, cumsum=lambda t, dim: _CumsumF32.apply(t, dim))


def _cast(v, dtype):
    if isinstance(v, tuple):
        return tuple(_cast(a, dtype) for a in v)
    return v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v


def oracle_grad(kind, case, inp, dtype, fast=False, float_sums=False):
    """dL/dmean [B,52,4] of the case by autograd over O.guidance_step's total().  float_sums (float32 only): the roll-out's running sums
    and their adjoints carried in float32, as chain_grad carried them before tests/test_gpu_guide.py."""
    tm = {k: _cast(v, dtype) for k, v in terms(case, kind, inp).items()}
    w = O.to_torch(decoder_weights(kind), dtype)
    _, g = O.guidance_step(w, inp["mean"].to(dtype), inp["cond"].to(dtype), inp["curr_states"].to(dtype), tm.get("target_speed"),
                           tm.get("loss_scale"), LR, None, "sgd", speed_limit=tm.get("speed_limit"), acc_limit=tm.get("acc_limit"),
                           target_pos=tm.get("target_pos"), decoder=_decoder(fast, float_sums), ext_grad=tm.get("ext_grad"))
    return g


def chain(act, cs, dyn=O.DYN):
    """Every quantity the roll-out compares, from the scaled actions [B,52,2] in their dtype: acc, wr (descaled, unclipped) [B,52],
    v_raw, v [B,53] (index k = v_k, v_0 the current speed), ya, ybb, yb [B,52] (of v_k, k = 0 .. 51), traj [B,52,6] (the oracle's)."""
    mean, std = torch.tensor(O.NORM_MEAN, dtype=act.dtype), torch.tensor(O.NORM_STD, dtype=act.dtype)
    a = act * std[4:6] + mean[4:6]
    acc, wr = a[..., 0], a[..., 1]
    v_raw = torch.cumsum(torch.cat((cs[:, 2:3], acc.clamp(dyn["acce_lo"], dyn["acce_hi"]) * dyn["dt"]), dim=1), dim=1)
    v = v_raw.clamp(dyn["v_lo"], dyn["v_hi"])
    av = v[:, :-1].abs()
    ya, ybb = dyn["max_steer"] * av, dyn["max_yawvel"] / av.clamp(min=0.1)
    return {"acc": acc, "wr": wr, "v_raw": v_raw, "v": v, "ya": ya, "ybb": ybb, "yb": torch.minimum(ya, ybb).clamp(min=0.1),
            "traj": O.action_to_state_and_action(act, cs, True, True)}


def forward(kind, inp, dtype, fast=False):
    """`chain` of the decoded actions, 512 rows a call (forward only: cheap enough for every row of a large batch)."""
    w = O.to_torch(decoder_weights(kind), dtype)
    parts = []
    with torch.no_grad():
        for i in range(0, inp["mean"].shape[0], 512):
            z, cond, cs = (inp[k][i:i + 512].to(dtype) for k in ("mean", "cond", "curr_states"))
            parts.append(chain(VC.lstm_decode(w, z, cond, fast=True) if fast else O.lstm_decode(w, z, cond), cs))
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


PRECISIONS = (("f64", torch.float64, False), ("f32", torch.float32, False), ("f32fast", torch.float32, True))


@functools.lru_cache(maxsize=None)
def forwards(kind: str, B: int = B_REG, rows=None):
    """{"f64" | "f32" | "f32fast": chain(...)} on `rows` (a tuple; None: all) of the B-row inputs.  Do not write to the result."""
    torch.set_num_threads(8)
    inp = take(inputs(B), rows)
    return {p: forward(kind, inp, dt, fast) for p, dt, fast in PRECISIONS}


@functools.lru_cache(maxsize=None)
def grads(kind: str, case: str, B: int = B_REG, rows=None):
    """{"f64" | "f32" | "f32fast": dL/dmean} likewise (at most 64 rows)."""
    torch.set_num_threads(8)
    inp = take(inputs(B), rows)
    assert inp["mean"].shape[0] <= 64
    return {p: oracle_grad(kind, case, inp, dt, fast) for p, dt, fast in PRECISIONS}


# ------------------------------------------------------------------------------------------------------------- regimes, kinks
def regimes(kind: str, f):
    """Boolean masks [B,52] over (agent, step) of the branches chain_grad takes, from a `chain` result."""
    d = O.DYN
    acc, wr, vr, v, vp = f["acc"], f["wr"], f["v_raw"][:, 1:], f["v"][:, 1:], f["v"][:, :-1]
    lo = torch.minimum(f["ya"], f["ybb"])
    act, floor = wr.abs() > f["yb"], ~(lo > 0.1)
    steer, yawvel = ~floor & (f["ya"] < f["ybb"]), ~floor & ~(f["ya"] < f["ybb"])
    return {"acc_lo": acc < d["acce_lo"], "acc_hi": acc > d["acce_hi"], "acc_in": (acc >= d["acce_lo"]) & (acc <= d["acce_hi"]),
            "v_lo": vr < d["v_lo"], "v_hi": vr > d["v_hi"], "v_in": (vr >= d["v_lo"]) & (vr <= d["v_hi"]),
            "yaw_free": ~act, "yaw_steer": act & steer, "yaw_yawvel": act & yawvel, "yaw_floor": act & floor,
            "yaw_bound_backwards": act & ~floor & (vp < 0), "v_negative": v < 0,
            "sl_on": v.abs() > SPEED_LIMIT, "sl_off": ~(v.abs() > SPEED_LIMIT),
            "al_pos": acc > ACC_LIMIT[kind], "al_neg": acc < -ACC_LIMIT[kind], "al_off": ~(acc.abs() > ACC_LIMIT[kind])}


def comparisons(kind: str, case: str, f, inp):
    """{name: d [B,n]}: every difference whose sign (against 0) the chain branches on in this case, in the unit of the compared quantity,
    +inf where the agent's term is switched off or has no target."""
    d = O.DYN
    tm = terms(case, kind, inp)
    acc, wr, vr, v, vp = f["acc"], f["wr"], f["v_raw"][:, 1:], f["v"][:, 1:], f["v"][:, :-1]
    inf = torch.tensor(math.inf, dtype=acc.dtype)
    gate = lambda x, sc: torch.where((sc != 0)[:, None], x, inf)
    out = {"v_raw-v_lo": vr - d["v_lo"], "v_raw-v_hi": vr - d["v_hi"], "acc-acc_lo": acc - d["acce_lo"], "acc-acc_hi": acc - d["acce_hi"]}
    if "target_speed" in tm:
        df = v - tm["target_speed"].to(acc.dtype)
        out["v-target"] = gate(torch.where(torch.isnan(df), inf, df), tm["loss_scale"])
    if "speed_limit" in tm:
        out["|v|-speed_limit"] = gate(v.abs() - SPEED_LIMIT, tm["speed_limit"][1])
    if "acc_limit" in tm:
        out["|acc|-acc_limit"] = gate(acc.abs() - ACC_LIMIT[kind], tm["acc_limit"][1])
    if "target_pos" in tm or "ext_grad" in tm:
        # ya against ybb: ybb = max_yawvel / |v| moves by 600 rad/s per m/s at |v| = 0.1, far from where the two meet (|v| = 3.54), so the
        # largest float32 deviation of ya - ybb over a case says nothing about the crossing.  ya - ya*, with ya* the value of both at
        # the crossing, has the sign of ya - ybb for every |v| (ya rises, ybb does not), in ya's unit, and is as well conditioned as v.
        cross = d["max_steer"] * math.sqrt(d["max_yawvel"] / d["max_steer"])
        out.update({"wr-yb": wr - f["yb"], "wr+yb": wr + f["yb"], "ya-ybb": f["ya"] - cross,
                    "min(ya,ybb)-0.1": torch.minimum(f["ya"], f["ybb"]) - 0.1, "|v_k|-0.1": vp.abs() - 0.1, "v_k": vp})
    if "target_pos" in tm:
        wp, when, sc = tm["target_pos"]
        dist = (f["traj"][..., :2] - wp.to(acc.dtype)[:, None]).norm(dim=-1)
        step = torch.arange(T)[None]
        used = torch.where(when[:, None] >= 0, step == when[:, None], step >= -when[:, None] - 1)
        out["waypoint distance"] = gate(torch.where(used, dist, inf), sc)
    return out


def kink_margin(kind: str, case: str, f64, inp):
    """{name: [B]}: per agent the smallest distance, in float64, to each comparison the chain makes in this case."""
    return {k: v.abs().amin(dim=1) for k, v in comparisons(kind, case, f64, inp).items()}


def deviations(kind: str, case: str, fw, inp):
    """{name: max|float32 reference - float64 reference|} of every compared quantity of the case (the larger of the two float32
    references), over the rows that have references.  fw: `forwards` of those rows."""
    c64 = comparisons(kind, case, fw["f64"], inp)
    dev = {k: 0.0 for k in c64}
    for p in ("f32", "f32fast"):
        for k, v in comparisons(kind, case, fw[p], inp).items():
            both = torch.isfinite(v) & torch.isfinite(c64[k])
            if bool(both.any()):
                dev[k] = max(dev[k], float((v.double() - c64[k])[both].abs().max()))
    return dev


def kink_adjacent(kind: str, case: str, f64, inp, dev):
    """[B] bool: agents whose margin for some quantity is below 8 x that quantity's deviation, and {name: (deviation, agents)}.
    f64: `chain` in float64 of the rows in question (for a large batch: all of them, forward only; dev from its subset)."""
    record = {}
    adj = torch.zeros(f64["acc"].shape[0], dtype=torch.bool)
    for k, v in kink_margin(kind, case, f64, inp).items():
        hit = v < 8 * dev[k]
        record[k] = (dev[k], int(hit.sum()))
        adj |= hit
    return adj, record


@functools.lru_cache(maxsize=None)
def regime_kinks(kind: str, case: str):
    """(kink-adjacent [B_REG] bool, record) of the regime batch."""
    fw, inp = forwards(kind), inputs(B_REG)
    return kink_adjacent(kind, case, fw["f64"], inp, deviations(kind, case, fw, inp))


@functools.lru_cache(maxsize=None)
def big_forward64(kind: str, B: int):
    torch.set_num_threads(8)
    return forward(kind, inputs(B), torch.float64)


@functools.lru_cache(maxsize=None)
def big_kinks(form: str, B: int, kind: str = "hot", case: str = "combined"):
    """(kink-adjacent [B] bool, record) of every row of a large batch: margins from the forward-only float64 decode of all rows,
    deviations from the two references of the subset of `form`."""
    rows, _ = big_subset(form, B)
    dev = deviations(kind, case, forwards(kind, B, rows), take(inputs(B), rows))
    return kink_adjacent(kind, case, big_forward64(kind, B), inputs(B), dev)


# ------------------------------------------------------------------------------------------------------------- large batches
def big_groups(form: str, B: int):
    """The groups of `form` with a full reference: the first two, the last of pass one, the first of pass two, one in between and the
    ragged last one.  At most 64 rows: the 16-agent kernel keeps the first group only."""
    n, per = GROUP[form], GRID[form]
    last = (B - 1) // n
    groups = sorted({0, 1, per // 2, per - 1, per, last})
    if sum(min(n, B - g * n) for g in groups) > 64:
        groups.remove(1)
    return groups


def big_subset(form: str, B: int):
    """-> (rows, groups): whole groups, in order, so that the rows keep their slot when they are run as a small batch."""
    form = "mfma" if form == "auto" else form
    groups = big_groups(form, B)
    n = GROUP[form]
    rows = [r for g in groups for r in range(g * n, min((g + 1) * n, B))]
    assert len(rows) <= 64 and B - 1 in rows and all(a < b for a, b in zip(rows, rows[1:]))
    return tuple(rows), groups
