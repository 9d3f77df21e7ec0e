"""Record tests/golden/recon_guidance.npz: one reconstruction-guided step (upstream guide_clean="video_diff") from the reference's own
code, on the CPU in float32.

    python tests/tools/record_recon_golden.py          (needs the reference tree, see oracle/_refimport.py)

Composed of the reference's pieces, each run unmodified:
  * DmModel.model, the U-Net (models/dm/dm_model.py:60-66), and DmModel's schedule buffers (:29-56): sqrt_recip_alphas_cumprod,
    sqrt_recipm1_alphas_cumprod, posterior_log_variance_clipped, posterior_mean_coef1 / 2;
  * LSTMVAE.lstm_dec and VaeModel.convert_action_to_state_and_action (scaled input, descaled output) as the `transform` of
  * PerturbationGuidance (src/tbsim/utils/guidance_loss.py:2179-2330) with DiffuserGuidance (:2106-2174) over a `target_speed` config
    (scene 0) and a `target_pos` config (scene 1), and its perturb_video_diffusion (:2284-2330), called verbatim with
    return_grad_of = x_t.
What is NOT the reference's code here are the lines of DiffuserModel.p_sample / p_mean_variance / predict_start_from_noise / q_posterior
(src/tbsim/models/diffuser.py) that join those pieces.  The module imports in this tree (no dependency is missing), but they are methods
of DiffuserModel, upstream's own network with its own encoders and configuration, not of CLD's DmModel whose U-Net and buffers are the
denoiser here; no DiffuserModel is built.  The lines are restated below, next to their line numbers: the CFG combine (diffuser.py:787),
x0_hat (:710-719), sigma, lr and perturb_th (:857, :888-902), the posterior mean (:911, :737-741 with dm_model.py:50-53).
One difference is deliberate and follows the definition in include/cld_recon.h: upstream's p_mean_variance forms x0_hat from a DETACHED
copy of x_t (x_tmp = x.detach(), :761-764, :792), so its x_t.grad holds only the path through the denoiser; here x0_hat is formed from
x_t itself and x_t.grad = sqrt_recip_acp[t] dL/dx0_hat + that path -- the gradient of the loss with respect to the noisy latent.

B = 4 agents in two scenes of two, N = 2 samples (8 rows, sample-minor), timesteps 99, 50, 1; with and without CFG (w = 2); lr = None;
perturb_th None and 1.0.  Stored: the inputs, and per case x0_hat, x_t.grad, the guided clean prediction and the posterior mean; `meta`
holds per case and output the reference's own float32 error against the float64 yardstick of tests/recon_yardstick.py."""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from cld_amd import synth                      # noqa: E402
from oracle import _refimport                  # noqa: E402
from tests import recon_yardstick as RY        # noqa: E402

A, N, SEED, T, N_T = 4, 2, 81, 52, 100
W_SEED, GW = 3, 2.0
TIMES = (99, 50, 1)
TS_WEIGHT, TP_WEIGHT, MIN_TARGET_TIME = 1.0, 0.5, 0.5
OUTPUTS = ("x0_hat", "grad_xt", "x0_guided", "mean")


def tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def yardstick_losses(tgt, wp):
    """The two configs as tests/recon_yardstick.total takes them: per-row scales of the scene means."""
    BN = A * N
    in0 = torch.tensor([1.0, 1.0, 0.0, 0.0]).repeat_interleave(N)
    m = int(MIN_TARGET_TIME * T)
    return {"builtin": dict(target_speed=tensor(tgt).repeat_interleave(N, dim=0), loss_scale=in0 * TS_WEIGHT / (2 * N * T),
                            target_pos=(torch.cat([torch.zeros(2, 2), tensor(wp)]).repeat_interleave(N, dim=0),
                                        torch.full((BN,), -(m + 1), dtype=torch.long), (1.0 - in0) * TP_WEIGHT / (2 * N)))}


def main():
    torch.set_num_threads(8)
    ref = _refimport.load()
    with _refimport.redirect_stdout(_refimport.io.StringIO()):
        import tbsim.utils.guidance_loss as gl
    from oracle import make_golden as MG
    algo = ref.algo
    w_unet, w_dec = synth.make_unet_weights(W_SEED, affine_jitter=True), synth.make_decoder_weights(0)
    dm = MG.build_dm(ref, N_T, True, weights=w_unet)
    vae = ref.LSTMVAE(6, 64, 4, 2, device=torch.device("cpu")).eval()
    sd = vae.state_dict()
    for k, v in w_dec.items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = tensor(v)
    vae.load_state_dict(sd)
    dyn = ref.dynamics.Unicycle("dynamics", max_steer=algo.dynamics["max_steer"], max_yawvel=algo.dynamics["max_yawvel"],
                                acce_bound=algo.dynamics["acce_bound"])
    fake = types.SimpleNamespace(add_coeffs=np.array(algo.nusc_norm_info.diffuser[0]).astype("float32"),
                                 div_coeffs=np.array(algo.nusc_norm_info.diffuser[1]).astype("float32"),
                                 default_chosen_inds=[0, 1, 2, 3, 4, 5], dyn=dyn, dt=0.1)
    fake.scale_traj = types.MethodType(ref.VaeModel.scale_traj, fake)
    fake.descale_traj = types.MethodType(ref.VaeModel.descale_traj, fake)
    conv = types.MethodType(ref.VaeModel.convert_action_to_state_and_action, fake)

    BN = A * N
    rep = lambda a: tensor(a).repeat_interleave(N, dim=0)
    inp, inp_u = synth.make_inputs(A, SEED), synth.make_inputs(A, SEED + 1000)
    cond, non_cond, cs = rep(inp["cond_feat"]), rep(inp_u["cond_feat"]), rep(inp["curr_states"])
    x_in = tensor(synth.normal(SEED, "recon_xt", (BN, T, 4)))
    tgt = synth.uniform(SEED, "recon_ts", (A, T), 0.0, 12.0)
    wp = np.stack((synth.uniform(SEED, "recon_wp_x", (2,), 5.0, 25.0), synth.uniform(SEED, "recon_wp_y", (2,), -4.0, 4.0)), axis=1)
    cfgs = [[{"name": "target_speed", "weight": TS_WEIGHT, "params": {"dt": 0.1, "target_speed": tgt, "fut_valid": np.ones((A, T), bool)}, "agents": None}],
            [{"name": "target_pos", "weight": TP_WEIGHT, "params": {"target_pos": wp, "min_target_time": MIN_TARGET_TIME}, "agents": None}]]
    data_batch = {"scene_index": torch.tensor([0, 0, 1, 1])}
    transform = lambda x, data_batch, params, bsize, num_samp: conv(vae.lstm_dec(x, cond), cs, scaled_input=True, descaled_output=True)
    losses = yardstick_losses(tgt, wp)

    out = {"x_t": x_in, "cond": cond, "non_cond": non_cond, "curr_states": cs, "target_speed": tgt.astype(np.float32), "waypoint": wp.astype(np.float32)}
    cases = {}
    o_gd = torch.Tensor.get_device
    torch.Tensor.get_device = lambda self: "cpu"       # scale_traj / descale_traj ask for it (-1 on the CPU -> error); nothing else does
    try:
        for t in TIMES:
            for cfg in (False, True):
                for th_name, th_in in (("sigma", None), ("sched", 1.0)):
                    name = f"t{t}_{'cfg' if cfg else 'plain'}_{th_name}"
                    pg = gl.PerturbationGuidance(transform=transform, transform_params=None)
                    pg.set_guidance(cfgs)
                    x = x_in.clone().requires_grad_(True)
                    tt = torch.full((BN,), t, dtype=torch.long)
                    with torch.enable_grad():
                        eps = dm.model(x, {"cond_feat": cond}, tt)
                        if cfg:                                                            # diffuser.py:766-789
                            eps = (1 + GW) * eps - GW * dm.model(x, {"cond_feat": non_cond}, tt)
                        x0_hat = dm.sqrt_recip_alphas_cumprod[t] * x - dm.sqrt_recipm1_alphas_cumprod[t] * eps       # :710-719
                    sigma = (0.5 * dm.posterior_log_variance_clipped[t]).exp()             # :857
                    tq = torch.tensor(t)
                    if th_in is not None:                                                  # :888-894 (t > 0: nonzero_mask = 1)
                        sig_scale = (torch.sigmoid(10 * tq / N_T) - 1 / 2) * 2
                        perturb_th = sig_scale * (4 - th_in) + th_in
                    else:                                                                  # :895-899
                        perturb_th = sigma
                    opt = {"optimizer": "adam", "lr": sigma, "grad_steps": 1, "perturb_th": perturb_th}       # :901-905 (lr None -> sigma)
                    xg, _ = pg.perturb_video_diffusion(x0_hat, data_batch, opt, num_samp=N, return_grad_of=x)
                    mean = dm.posterior_mean_coef1[t] * xg + dm.posterior_mean_coef2[t] * x                    # :911, q_posterior
                    got = {"x0_hat": x0_hat.detach(), "grad_xt": x.grad.detach().clone(), "x0_guided": xg.detach(), "mean": mean.detach()}
                    c = RY.core(w_unet, w_dec, N_T, t, x_in, cond, non_cond if cfg else None, GW, cs, losses, torch.float64)
                    u = RY.update(c, N_T, t, x_in, torch.zeros_like(x_in), None, th_in, False, torch.float64)
                    y = {"x0_hat": c["x0_hat"], "grad_xt": c["grad_xt"], "x0_guided": u["x0_guided"], "mean": u["mean"]}
                    err = {k: float((got[k].double() - y[k]).abs().max()) for k in OUTPUTS}
                    mx = {k: float(y[k].abs().max()) for k in OUTPUTS}
                    print(f"{name}: reference fp32 against the fp64 yardstick: " + ", ".join(f"{k} {err[k]:.2e} of {mx[k]:.3g}" for k in OUTPUTS)
                          + f"; clipped {float(u['clipped'].double().mean()):.3f}")
                    for k in OUTPUTS:
                        out[f"{name}_{k}"] = got[k]
                    cases[name] = dict(t=t, cfg=cfg, perturb_th=th_in, ref_err=err, max=mx, clipped_share=float(u["clipped"].double().mean()))
    finally:
        torch.Tensor.get_device = o_gd
    meta = dict(A=A, N=N, seed=SEED, w_seed=W_SEED, dec_seed=0, guidance_w=GW, n_timesteps=N_T, scenes=[2, 2], ts_weight=TS_WEIGHT, tp_weight=TP_WEIGHT,
                min_target_time=MIN_TARGET_TIME, cases=cases, torch=torch.__version__, generator="tests/tools/record_recon_golden.py",
                source="the reference's DmModel.model and buffers, LSTMVAE.lstm_dec, VaeModel.convert_action_to_state_and_action, DiffuserGuidance, "
                       "PerturbationGuidance.perturb_video_diffusion; the joining lines of DiffuserModel.p_sample restated")
    arrays = {k: np.ascontiguousarray(v.detach().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    path = os.path.join(ROOT, "tests", "golden", "recon_guidance.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f"recon_guidance: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
