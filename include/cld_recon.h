/* cld_recon.h -- reconstruction guidance of libcld_hip: upstream's guide_clean="video_diff" inside the sampler.  A header of its own
 * beside cld.h (whose table of entry points is pinned); everything of cld.h's conventions holds: DEVICE pointers, row-major, an int
 * return (CLD_OK / CLD_ERR_*), the message behind cld_last_error, `stream` a hipStream_t or NULL. */
#ifndef CLD_RECON_H
#define CLD_RECON_H

#include "cld.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Upstream's DiffuserModel.p_sample with guide_clean == "video_diff" (src/tbsim/models/diffuser.py:844-929) and
 * PerturbationGuidance.perturb_video_diffusion (src/tbsim/utils/guidance_loss.py:2284-2330): the mode both shipped checkpoints and
 * the evaluation preset ask for.  The guidance loss is evaluated on the decoded CLEAN prediction, but its gradient is taken with
 * respect to the NOISY latent x_t, through the denoiser; the posterior is then re-derived from the guided clean prediction
 * (q_posterior, diffuser.py:911).  One guided step at timestep t > 0, rows b < B, latent [52,4]:
 *   1. eps     = U-Net(x_t, cond, t)                  taped forward (the path of cld_unet_train_forward); with non_cond:
 *                eps = (1 + w) eps_c - w eps_u from ONE 2B-row batch, rows [B,2B) carrying non_cond and the same x_t
 *   2. x0_hat  = sqrt_recip_acp[t] x_t - sqrt_recipm1_acp[t] eps
 *   3. g0      = dL/dx0_hat, L the guidance total on decode(x0_hat): every term of `cld_guidance` (built-in losses, ext_grad,
 *                collision / map structs) and every term set on the handle (goal, social group, pair, lane), in the order and with
 *                the grad_in chaining of the mean-guided step; a social-group term takes one evaluation index per loop iteration
 *   4. g_xt    = dL/dx_t = sqrt_recip_acp[t] g0 + dx_c + dx_u, (dx_c, dx_u) the input gradients of the taped pass (the path of
 *                cld_unet_backward with d_params = NULL, dcond = NULL) for the cotangents
 *                d_eps_c = -sqrt_recipm1_acp[t] (1 + w) g0,  d_eps_u = +sqrt_recipm1_acp[t] w g0
 *   5. delta   = s lr_t g_xt,  lr_t = lr, or sigma_t when lr <= 0 (upstream `lr is None`, diffuser.py:901-902)
 *   6. delta_c = clip(delta, +-th_t): perturb_th == 0: th_t = sigma_t (diffuser.py:896-899); > 0: upstream's schedule
 *                th_t = s_t (4 - perturb_th) + perturb_th, s_t = 2 sigmoid(10 t / n_timesteps) - 1 (:888-891); < 0: no clip.
 *                Unlike perturb()'s, this clip is effective upstream (guidance_loss.py:2325-2328)
 *   7. x0_g    = x0_hat + delta_c;  mean = posterior_mean_coef1[t] x0_g + posterior_mean_coef2[t] x_t (dm_model.py:50-53);
 *                x_{t-1} = mean + sigma_t z
 * THE SIGN.  descend == 0 (s = +1) reproduces upstream AS WRITTEN: x_guidance = x_initial + lr * grad (guidance_loss.py:2319-2324).
 * With the positive totals of compute_guidance_loss (:2143-2174) that step ASCENDS the loss -- it moves the clean prediction away from
 * what the guidance asks for.  descend != 0 (s = -1) is the evident intent.  Both are built; the field is explicit so that neither is
 * a silent default.
 * Step t = 0 is the ordinary unguided iteration of cld_sample / cld_sample_cfg on the handle's own weights.
 * Upstream's loop cannot run grad_steps > 1 here (its second backward() goes through a freed graph): grad_steps > 1,
 * apply_output != 0 and no_intermediate != 0 are CLD_ERR_ARG.  cld_guidance.lr / perturb_th / optimizer / guide_clean (and the
 * final_* fields) are NOT read by the calls below ("ignored if video_diff", scene_edit_config.py:74); the loss terms, curr_states,
 * the collision / map pointers and the handle-set terms are.  Exact fp32 only: a CLD_PRECISION_F16X2 handle is CLD_ERR_STATE, as
 * for the training calls.  Deterministic: no atomics in the new kernels, each row's result independent of the other rows (terms
 * that couple rows -- collision, social, pair -- couple them as they do in the mean-guided step). */
typedef struct cld_recon {
    const float* params;   /* DEVICE: the flat U-Net buffer in the layout of cld_unet_param_info.  The caller guarantees that it holds
                            * the weights the handle was finalized with (the t = 0 step runs on the handle's own copy) */
    float lr;              /* <= 0: sigma_t */
    float perturb_th;      /* < 0: no clip; 0: sigma_t; > 0: upstream's schedule towards that value */
    int32_t descend;       /* 0: upstream's sign as written (ascends the loss); != 0: x0_hat - lr grad */
} cld_recon;

/* Bytes of the workspace of the two calls below for B rows, cfg != 0 when non_cond is given: the sampler workspace
 * (cld_workspace_bytes, 2 pad16(B) rows with cfg), the tape of B or 2B rows (cld_unet_tape_bytes), the training workspace
 * (cld_unet_train_workspace_bytes) and the step's own buffers.  The compute calls neither allocate nor synchronise.  0 on a bad
 * argument. */
size_t cld_recon_workspace_bytes(cld_handle h, int32_t B, int32_t cfg);

/* ONE iteration of cld_sample_recon at timestep t_idx, teacher-forced.  x_t [B,52,4], cond [B,256], non_cond [B,256] or NULL,
 * z [B,52,4] or NULL (the on-device generator keyed by (seed, salt, row): the value every other site draws for it); salt is also the
 * evaluation index of a social-group term.  Outputs [B,52,4], every one optional: x_next; x0_hat, grad_xt = dL/dx_t and x0_guided
 * are written on a guided step (t_idx > 0) only; mean = the posterior mean x_next was drawn around (at t_idx == 0 the unguided one).
 * *sigma_host receives sigma_t = exp(0.5 * logvar[t_idx]).  Same launches in the same order as the loop: stepping through the loop's
 * timesteps with its noise slabs and salts 0, 1, ... reproduces cld_sample_recon bit for bit. */
int cld_recon_step(cld_handle h, const float* x_t, const float* cond, const float* non_cond, float guidance_w,
                   const cld_guidance* guidance, const cld_recon* recon, int32_t t_idx, const float* z, float* x_next, float* x0_hat,
                   float* grad_xt, float* x0_guided, float* mean, float* sigma_host /*HOST*/, int32_t B, uint64_t seed, uint64_t salt,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The loop: cld_sample_guided's arguments (stride honoured, `steps` = its loop iterations, noise [steps,B,52,4] or NULL) with the
 * step above at every t > 0. */
int cld_sample_recon(cld_handle h, const float* x_T, const float* noise, const float* cond, const float* non_cond, float guidance_w,
                     const cld_guidance* guidance, const cld_recon* recon, int32_t steps, float* x0, float* x1, float* logp, int32_t B,
                     uint64_t seed, void* workspace, size_t workspace_bytes, void* stream);

/* posterior_mean_coef1 / posterior_mean_coef2 (dm_model.py:50-53) as the handle holds them, n_timesteps floats each (HOST; either
 * may be NULL). */
int cld_recon_get_posterior(cld_handle h, float* coef1, float* coef2);

/* Tests: the most workgroups a launch of the three elementwise kernels takes (they walk their rows in a grid-stride loop); cap < 1
 * restores the default.  Returns the cap in force. */
int32_t cld_debug_recon_grid_cap(int32_t cap);

#ifdef __cplusplus
}
#endif

#endif
