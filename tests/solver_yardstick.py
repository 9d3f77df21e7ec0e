"""Yardstick of the few-step samplers (include/cld_solver.h; tests/test_solver_host.py on the CPU, tests/test_gpu_solver.py on the GPU):
DDIM(eta) and DPM-Solver++(2M) on a timestep subset, restated in torch over the pinned oracle -- unet_forward for the noise prediction,
guidance_step on the deterministic part mu with the two scales.  A plain module.

The reference has no few-step sampler, so no recording pins this mode.  float64 is the reference; the same code in float32 calibrates the
bar of tests/grad_bar.py (per tensor max|got - f64| <= 4 max|f32 - f64| + 1e-7 max|f64|).  Two anchors that do not depend on this
restatement are asserted in tests/test_solver_host.py: DDIM with eta = 1 on the full consecutive sequence is the reference's ancestral
chain, and the second-order solver converges with order two on a problem with a closed-form solution.

The per-step coefficients are formed in float64 from the float32 alphas_cumprod table (oracle.cld_oracle.schedule) and cast to the
dtype once, as the library forms them on the host and rounds them to fp32 once.
"""
import functools
import math

import torch

from oracle import cld_oracle as O

T = 52
KINDS = ("ddim", "dpmpp_2m")
COLS = ("a", "b", "c0", "c1", "rc", "rm1", "sigma", "sigma_g")


@functools.lru_cache(maxsize=None)
def acp64(n: int):
    """alphas_cumprod of n timesteps: the float32 table promoted to float64."""
    return O.schedule(n)["alphas_cumprod"].double()


def _pairs(n, ts):
    """(acp_s, acp_p) [K] each in float64: step k goes from ts[k] to ts[k + 1], the last one to acp = 1."""
    ac = acp64(n)
    a_s = ac[torch.as_tensor(list(ts), dtype=torch.long)]
    return a_s, torch.cat([a_s[1:], torch.ones(1, dtype=torch.float64)])


def tables(n: int, kind: str, ts, eta: float = 0.0, last_is_final: bool = True):
    """The float64 coefficients of every step, {name: [K]} under COLS, plus "b_x0": the weight of x0_hat in the x0_hat form of the same
    update (DDIM: x' = sqrt(acp_p) x0_hat + sqrt(1 - acp_p - var) eps_hat; "dir": that second weight), and "h" (2M).
    last_is_final=False: the last entry of ts is a step like the others towards ... nothing: then ts has K + 1 entries and K steps are
    returned (the order-of-accuracy anchor integrates between two interior timesteps without a final jump)."""
    assert kind in KINDS
    ts = list(ts)
    if last_is_final:
        a_s, a_p = _pairs(n, ts)
    else:
        ac = acp64(n)[torch.as_tensor(ts, dtype=torch.long)]
        a_s, a_p = ac[:-1], ac[1:]
    K = a_s.shape[0]
    jump = (1.0 - a_p) / (1.0 - a_s) * (1.0 - a_s / a_p)
    out = {"rc": torch.sqrt(1.0 / a_s), "rm1": torch.sqrt(1.0 / a_s - 1.0), "sigma_g": torch.sqrt(jump.clamp(min=1e-20)),
           "c0": torch.ones(K, dtype=torch.float64), "c1": torch.zeros(K, dtype=torch.float64)}
    lam = lambda a: 0.5 * torch.log(a / (1.0 - a))
    if kind == "ddim":
        var = eta * eta * jump
        out["sigma"] = torch.sqrt(var)
        out["a"] = torch.sqrt(a_p / a_s)
        out["dir"] = torch.sqrt((1.0 - a_p - var).clamp(min=0.0))
        out["b"] = out["dir"] - torch.sqrt(a_p * (1.0 - a_s) / a_s)
        out["b_x0"] = torch.sqrt(a_p)
    else:
        assert eta == 0.0
        out["sigma"] = torch.zeros(K, dtype=torch.float64)
        h = lam(a_p) - lam(a_s)                                  # +inf on the final step: expm1(-inf) = -1
        out["h"] = h
        out["a"] = torch.sqrt((1.0 - a_p) / (1.0 - a_s))
        out["b"] = -torch.sqrt(a_p) * torch.expm1(-h)
        second = range(1, K - 1 if last_is_final else K)
        for k in second:
            r = h[k - 1] / h[k]
            out["c0"][k], out["c1"][k] = 1.0 + 1.0 / (2.0 * r), 1.0 / (2.0 * r)
    if last_is_final:
        out["sigma"][-1] = 0.0
    return out


def eps_of(w, x, cond, non_cond, guidance_w, t: int):
    """The (CFG-combined) noise prediction at timestep t; w: O.to_torch weights in x's dtype."""
    tt = torch.full((x.shape[0],), int(t), dtype=torch.long)
    eps = O.unet_forward(w, x, cond, tt)
    if non_cond is not None:
        eps = (1 + guidance_w) * eps - guidance_w * O.unet_forward(w, x, non_cond, tt)
    return eps


def update(tab, kind, k, K, x, eps, x0_prev, z):
    """The elementwise part of step k of K on (x, eps) with the coefficients `tab` (already in x's dtype)
    -> dict(x0_hat, mu [deterministic part], x_next [mu + sigma z; mu itself where sigma = 0 or z is None])."""
    x0 = tab["rc"][k] * x - tab["rm1"][k] * eps
    if k == K - 1:
        mu = x0
    elif kind == "ddim":
        mu = tab["a"][k] * x + tab["b"][k] * eps
    else:
        D = x0 if k == 0 else tab["c0"][k] * x0 - tab["c1"][k] * x0_prev
        mu = tab["a"][k] * x + tab["b"][k] * D
    sigma = float(tab["sigma"][k])
    return {"x0_hat": x0, "mu": mu, "x_next": mu if (sigma == 0.0 or z is None) else mu + tab["sigma"][k] * z}


def guide(wdec, mu, cond, g, sigma_g: float, last: bool, dtype):
    """The guidance step(s) on mu as the library runs them (upstream perturb(), oracle.guidance_step): g = dict(curr_states,
    target_speed | None, loss_scale | None, lr | None [sigma^g], perturb_th None | "sigma" [sigma^g] | number, optimizer,
    collision: (term, num_samp) | None, intermediate = True, output: None | dict(lr = 0.3, perturb_th, optimizer = "adam")).
    -> (mu_guided, grad, th, the learning rate in force) or None when this step is not guided."""
    if g is None:
        return None
    if last:
        fo = g.get("output")
        if not fo:
            return None
        fo = {} if fo is True else fo
        lr, th, opt = fo.get("lr", 0.3), fo.get("perturb_th"), fo.get("optimizer", "adam")
    else:
        if not g.get("intermediate", True):
            return None
        lr, th, opt = g.get("lr"), g.get("perturb_th"), g.get("optimizer", "adam")
    lr = sigma_g if not lr else float(lr)
    th = None if th is None else (sigma_g if th == "sigma" else float(th))
    c = lambda v: None if v is None else v.to(dtype)
    col, N = g.get("collision") or (None, 1)
    if col is not None:
        col = {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in col.items()}
    mg, grad = O.guidance_step(wdec, mu, cond, c(g["curr_states"]), c(g.get("target_speed")), c(g.get("loss_scale")), lr, th, opt,
                               collision=col, num_samp=N)
    return mg.detach(), grad.detach(), th, lr


def step(w_unet, w_dec, n, kind, ts, eta, k, x, x0_prev, z, cond, non_cond=None, guidance_w=0.0, guidance=None, dtype=torch.float64):
    """Step k of the sampler on x at `dtype` (weights as numpy dicts) -> dict(x_next, x0_hat, mu, sigma, sigma_g, and on a guided step
    mu_guided, grad = dL/dmu, th [the clip threshold or None], lr_eff [the learning rate in force])."""
    ts = list(ts)
    K = len(ts)
    tab64 = tables(n, kind, ts, eta)
    tab = {c: v.to(dtype) for c, v in tab64.items()}
    w = O.to_torch(w_unet, dtype)
    x = x.to(dtype)
    cond = cond.to(dtype)
    nc = None if non_cond is None else non_cond.to(dtype)
    with torch.no_grad():
        eps = eps_of(w, x, cond, nc, guidance_w, ts[k])
    u = update(tab, kind, k, K, x, eps, None if x0_prev is None else x0_prev.to(dtype), None if z is None else z.to(dtype))
    sigma, sigma_g = float(tab64["sigma"][k]), float(tab64["sigma_g"][k])
    out = dict(u, eps=eps, sigma=sigma, sigma_g=sigma_g)
    gd = guide(O.to_torch(w_dec, dtype) if guidance is not None else None, u["mu"], cond, guidance, sigma_g, k == K - 1, dtype)
    if gd is not None:
        mg, grad, th, lr = gd
        out.update(mu_guided=mg, grad=grad, th=th, lr_eff=lr)
        out["x_next"] = mg if (sigma == 0.0 or z is None) else mg + tab["sigma"][k] * z.to(dtype)
    return out


def chain(w_unet, w_dec, n, kind, ts, eta, x_T, noise, cond, non_cond=None, guidance_w=0.0, guidance=None, dtype=torch.float64):
    """The whole loop -> (x0, [(x_t, x0_prev) seen by step k]).  noise [K,B,52,4] or None."""
    x, prev, seen = x_T.to(dtype), None, []
    for k in range(len(ts)):
        seen.append((x, prev))
        o = step(w_unet, w_dec, n, kind, ts, eta, k, x, prev, None if noise is None else noise[k], cond, non_cond, guidance_w, guidance, dtype)
        x, prev = o["x_next"], o["x0_hat"]
    return x, seen


# ------------------------------------------------------------------------------------------------------------- the closed-form anchor
def gaussian_eps(n, s2: float):
    """For data ~ N(0, s2) the exact noise prediction eps(x, t) = sqrt(1 - acp_t) x / (acp_t s2 + 1 - acp_t)."""
    ac = acp64(n)
    return lambda x, t: math.sqrt(1.0 - float(ac[t])) * x / (float(ac[t]) * s2 + 1.0 - float(ac[t]))


def gaussian_flow(n, s2: float, x, t_from: int, t_to: int):
    """... and the exact probability-flow solution x_p = x_s sqrt((acp_p s2 + 1 - acp_p) / (acp_s s2 + 1 - acp_s))."""
    ac = acp64(n)
    v = lambda t: float(ac[t]) * s2 + 1.0 - float(ac[t])
    return x * math.sqrt(v(t_to) / v(t_from))


def integrate(n, kind, ts, eps_fn, x):
    """The deterministic sampler (eta = 0) between ts[0] and ts[-1] in float64 with an analytic eps_fn(x, t), no final jump."""
    tab = tables(n, kind, ts, 0.0, last_is_final=False)
    K = len(ts) - 1
    prev = None
    for k in range(K):
        eps = eps_fn(x, ts[k])
        x0 = tab["rc"][k] * x - tab["rm1"][k] * eps
        if kind == "ddim":
            x = tab["a"][k] * x + tab["b"][k] * eps
        else:
            D = x0 if k == 0 else tab["c0"][k] * x0 - tab["c1"][k] * prev
            x = tab["a"][k] * x + tab["b"][k] * D
        prev = x0
    return x
