/*
 * cld.h -- C-ABI of the MI355X-native CLD latent-diffusion sampling path.
 *
 * The reference (RoboSafe-Lab/Controllable-Latent-Diffusion-for-Traffic-Simulation)
 * has no FFI layer: its seam is Python method calls on nn.Modules.  Each entry
 * point below replaces one of those calls (reference file:line given per
 * function); the Python host mirror in
 * `controllable-latent-diffusion-for-traffic-simulation_amd/` binds them with
 * ctypes and keeps the reference's method names and dict keys.
 *
 * Conventions
 *   - plain C types only; no torch / C++ types cross this boundary.
 *   - every `const float*` / `float*` that is not marked HOST is a DEVICE pointer
 *     to contiguous fp32; the caller owns all buffers (inputs and outputs).
 *   - `stream` is a hipStream_t passed as void*; work is enqueued on it and the
 *     call returns without synchronising.  Calls on one stream are ordered.
 *   - no allocation inside the compute calls: scratch comes from the caller
 *     (`cld_workspace_bytes`), so calls are capturable into a hipGraph.
 *   - return value: 0 = OK, negative = error (never throws);
 *     `cld_last_error` gives the message of the last failure on that handle.
 *   - one handle per device; distinct handles are independent.
 *
 * Fixed architecture (reference config.yaml:91-172; validated by cld_create):
 *   horizon T = 52, latent D = 4, cond C = 256, U-Net dims 4 -> 64 -> 128 -> 256
 *   (TemporalMapUnet, src/tbsim/models/temporal.py:49-180), LSTM decoder hidden 64.
 */
#ifndef CLD_H
#define CLD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cld_handle_s* cld_handle;

enum {
    CLD_OK = 0,
    CLD_ERR_ARG = -1,       /* bad argument / unsupported configuration      */
    CLD_ERR_STATE = -2,     /* weights missing / not finalized               */
    CLD_ERR_WORKSPACE = -3, /* workspace too small                            */
    CLD_ERR_HIP = -4        /* a HIP runtime call failed                      */
};

typedef struct cld_config {
    int32_t horizon;        /* 52   config.yaml:107                                   */
    int32_t latent_dim;     /* 4    config.yaml:133 vae.latent_size                   */
    int32_t cond_dim;       /* 256  config.yaml:118 cond_feat_dim                     */
    int32_t base_dim;       /* 32   config.yaml:106                                   */
    int32_t dim_mults[3];   /* 2,4,8 config.yaml:109-112                              */
    int32_t hidden;         /* 64   config.yaml:132 vae.hidden_size                   */
    int32_t n_timesteps;    /* 100  models/dm/dm_model.py:20 (ctor default)           */
    float step_time;        /* 0.1  models/vae/vae_model.py:43 (self.dt)              */
    float acce_bound[2];    /* -10, 8        config.yaml:138-140                      */
    float v_bound[2];       /* -10, 30       src/tbsim/dynamics/unicycle.py:10        */
    float max_steer;        /* 0.5           config.yaml:136                          */
    float max_yawvel;       /* 2*pi          config.yaml:137                          */
    float norm_mean[6];     /* config.yaml:162  (x - mean) / std convention,          */
    float norm_std[6];      /* config.yaml:163   models/vae/vae_model.py:152,170      */
    int32_t precision;      /* arithmetic of the U-Net convolutions, CLD_PRECISION_*; no reference counterpart */
} cld_config;

/* CLD_PRECISION_F32   : exact fp32 products on v_mfma_f32_16x16x4_f32 (default).
 * CLD_PRECISION_F16X2 : every activation and weight is carried as two fp16 planes hi + lo (22 mantissa bits in the
 *                       same 4 bytes), products hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_f16 with fp32
 *                       accumulation; GroupNorm / Mish / residuals / the DDPM update stay fp32.  The first convolution
 *                       (4-channel latent, unbounded range) keeps the exact-fp32 loop.  Values saturate at +-65504.
 *                       Same parity bars as F32 (tests run both); ~2x the throughput. */
enum { CLD_PRECISION_F32 = 0, CLD_PRECISION_F16X2 = 1 };

/* Fill `cfg` with the reference defaults listed above. */
void cld_default_config(cld_config* cfg);

/* Replaces DmModel.__init__ / LSTMVAE.__init__ (models/dm/dm_model.py:15-68,
 * models/vae/lstm_vae.py:55-84): builds the cosine schedule buffers
 * (dm_model.py:29-56) for cfg->n_timesteps on the current HIP device. */
int cld_create(const cld_config* cfg, cld_handle* out);
int cld_destroy(cld_handle h);
const char* cld_last_error(cld_handle h);

/* Replaces nn.Module.load_state_dict (src/trainers/dm_trainer.py:24-35,
 * utils/trainer_utils.py:59-72).  `name` is the reference state_dict key:
 * "model.*" for the U-Net (a leading "dm." is accepted and stripped),
 * "lstm_dec.*" for the VAE decoder (leading "vae.lstmvae." / "lstmvae." accepted).
 * `data` is a HOST pointer to `numel` fp32 values in the reference's layout
 * (Conv1d [C_out,C_in,k], ConvTranspose1d [C_in,C_out,k], Linear [out,in], ...).
 * Schedule buffer keys ("betas", ...) are accepted and ignored (rebuilt by cld_create).
 * Unknown keys or wrong sizes return CLD_ERR_ARG. */
int cld_load_weight(cld_handle h, const char* name, const float* data /*HOST*/, size_t numel);

/* Re-lays the loaded weights out for the kernels (MFMA fragment order), folds the
 * per-step time-embedding bias table, uploads everything.  Needs every "model.*"
 * tensor; the decoder tensors are optional (cld_decode then returns CLD_ERR_STATE). */
int cld_finalize(cld_handle h, void* stream);

/* Scratch bytes the compute calls need for up to B agents. */
size_t cld_workspace_bytes(cld_handle h, int32_t B);

/* Schedule read-back (HOST out, n_timesteps floats each; any pointer may be NULL):
 * x_t_cof, noise_cof, posterior_log_variance_clipped (dm_model.py:48-56). */
int cld_get_schedule(cld_handle h, float* x_t_cof, float* noise_cof, float* post_log_var);

/* eps = TemporalMapUnet.forward(x, {'cond_feat': cond}, t)
 * (src/tbsim/models/temporal.py:122-180; called from dm_model.py:87,147,166).
 * x [B,52,4], cond [B,256], t_idx: one timestep for all B rows (as in the sampler,
 * dm_model.py:122), eps [B,52,4]. */
int cld_unet_forward(cld_handle h, const float* x, const float* cond, int32_t t_idx, float* eps,
                     int32_t B, void* workspace, size_t workspace_bytes, void* stream);

/* cld_unet_forward with one timestep PER ROW (t_idx [B] DEVICE int32): TemporalMapUnet.forward accepts any `time [B]`
 * (temporal.py:122-146); training-style callers draw a different t per sample (dm_model.py:84). */
int cld_unet_forward_t(cld_handle h, const float* x, const float* cond, const int32_t* t_idx, float* eps, int32_t B,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The forward half of DmModel.compute_losses (dm_model.py:82-96; src/trainers/dm_trainer.py:84-90 validation_step):
 * z_t = q_sample(z0, t, noise) = sqrt(acp[t]) z0 + sqrt(1 - acp[t]) noise, eps = U-Net(z_t, cond, t) and
 * mse[b] = mean_{T,D} (noise - eps)^2, so that F.mse_loss(noise, eps) = mean_b mse[b].  z0, noise [B,52,4]; t_idx [B]
 * DEVICE int32 (values in [0, n_timesteps): the caller checks the range, the kernels index tables with them); z_noisy
 * [B,52,4] optional (NULL to skip); mse NULL (then cond may be NULL too) = q_sample alone, no U-Net evaluation
 * (DmModel.q_sample, dm_model.py:91-96).  Forward only: training itself is out of scope. */
int cld_denoise_loss(cld_handle h, const float* z0, const float* noise, const float* cond, const int32_t* t_idx, float* z_noisy,
                     float* mse, int32_t B, void* workspace, size_t workspace_bytes, void* stream);

/* (x_{t-1}, mean, sigma) = DmModel.x_Tminus1(x, t, aux_info)  (dm_model.py:144-163).
 * z [B,52,4] is the caller's N(0,1) draw (the reference's randn_like, :153); NULL = the on-device generator as cld_sample's
 * first iteration with seed 0 draws it (seed 0, step 0, row b * 52 + l).
 * x_next / mean [B,52,4] (either may be NULL); *sigma_host receives exp(0.5*logvar[t]). */
int cld_ddpm_step(cld_handle h, const float* x, const float* cond, int32_t t_idx, const float* z,
                  float* x_next, float* mean, float* sigma_host /*HOST*/, int32_t B,
                  void* workspace, size_t workspace_bytes, void* stream);

/* DmModel.stride (dm_model.py:25: 1; the loop of :119 visits i in reversed(range(0, n_timesteps, stride))).  Default 1. */
int cld_set_stride(cld_handle h, int32_t stride);

/* out = DmModel.forward(...)/sample_traj  (dm_model.py:98-142): the full ancestral
 * loop over i in reversed(range(0, n_timesteps, stride)); `steps` must equal the number of those iterations
 * (n_timesteps with the reference's stride 1).  With stride > 1 step 1 is never visited and x1 is left untouched (the
 * reference returns None).
 * x_T [B,52,4]; noise [steps,B,52,4], slab s feeds loop iteration s (i = (steps-1-s) * stride),
 * the reference RNG order (one randn_like per step incl. the masked t=0 one); if
 * noise == NULL a counter-based on-device generator seeded with `seed` is used
 * (throughput runs; not parity-comparable with torch's RNG).
 * Outputs (any may be NULL): x0 = 'pred_traj' [B,52,4], x1 = 'x1' [B,52,4],
 * logp = 'log_prob_final' [B]. */
int cld_sample(cld_handle h, const float* x_T, const float* noise, const float* cond, int32_t steps,
               float* x0, float* x1, float* logp, int32_t B, uint64_t seed,
               void* workspace, size_t workspace_bytes, void* stream);

/* cld_sample with classifier-free guidance.  CLD's DmModel has no CFG branch; the definition is the vendored
 * upstream DiffuserModel.p_mean_variance (src/tbsim/models/diffuser.py:766-789): a second U-Net pass on
 * aux_info['non_cond_feat'] (features of a map raster filled with -1, diffuser.py:390-411,459-471) and
 * eps = (1 + w) * eps_cond - w * eps_uncond, then the same DDPM update.  non_cond [B,256]; both passes run as
 * one 2B-agent batch per step; the workspace must cover 2 * (B rounded up to 16) agents
 * (cld_workspace_bytes(h, 2 * ((B + 15) / 16 * 16))).  Other arguments as cld_sample. */
int cld_sample_cfg(cld_handle h, const float* x_T, const float* noise, const float* cond, const float* non_cond,
                   float guidance_w, int32_t steps, float* x0, float* x1, float* logp, int32_t B, uint64_t seed,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Sampling-time guidance.  CLD's DmModel has none; the definition is the vendored upstream
 * DiffuserModel.p_sample (src/tbsim/models/diffuser.py:844-929) with PerturbationGuidance.perturb
 * (src/tbsim/utils/guidance_loss.py:2221-2282) and its `decoder` hook (:2259-2261) = LSTM decoder + unicycle roll-out:
 * at every step t > 0 the posterior mean mu is decoded to a trajectory, the guidance loss
 *     L = sum_agents loss_scale[b] * sum_t |v_t - target_speed[b,t]|         (TargetSpeedLoss, guidance_loss.py:219-254;
 *         loss_scale[b] = weight / (agents guided in b's scene * 52) reproduces DiffuserGuidance.compute_guidance_loss :2143-2175)
 *       [+ SpeedLimitLoss, AccLimitLoss and TargetPosAtTimeLoss terms, see the struct; any combination, as upstream sums its
 *          configured losses]
 * is differentiated through the roll-out and the decoder down to mu, ONE optimiser step is taken on mu
 * (Adam's first step: delta = -lr * g / (|g| + 1e-8); SGD: delta = -lr * g; scene_edit_config.py:74-90 defaults adam,
 * lr 0.3, grad_steps 1), and x_{t-1} = mu + delta + sigma_t z.  Step t = 0 is not guided (apply_guidance_output = False).
 * Clipping: upstream means to clip delta to +-perturb_th (sigma_t when None, diffuser.py:893-897), but perturb() takes
 * the delta between two names of the same tensor (x_guidance = x_initial, guidance_loss.py:2239,2275-2278), so its clip
 * never changes anything.  perturb_th < 0 reproduces that behaviour (what the golden vectors recorded from the
 * reference show); perturb_th = 0 clips to sigma_t and perturb_th > 0 to that value (the evident intent). */
enum { CLD_GUIDE_ADAM = 0, CLD_GUIDE_SGD = 1 };
typedef struct cld_guidance {
    const float* curr_states;   /* [B,4]  (x, y, v, yaw) the roll-out starts from                        */
    const float* target_speed;  /* [B,52] m/s, or NULL: no target-speed term                              */
    const float* loss_scale;    /* [B] or NULL (= 1/52 per agent): weight of the target-speed term        */
    float lr;                   /* <= 0: sigma_t  (upstream: `if lr is None: lr = sigma`, diffuser.py:899) */
    float perturb_th;           /* < 0: no clip (reference behaviour) ; 0: sigma_t ; > 0: that threshold    */
    int32_t optimizer;          /* CLD_GUIDE_ADAM | CLD_GUIDE_SGD                                          */
    /* two more losses on the same speed chain, each off when its scale pointer is NULL:
     *   SpeedLimitLoss (guidance_loss.py:1509-1538): sum_b speed_limit_scale[b] * sum_t relu(|v_t| - speed_limit)
     *   AccLimitLoss   (guidance_loss.py:1444-1467): sum_b acc_limit_scale[b]   * sum_t relu(|acc_t| - acc_limit), on the
     *                  descaled, unclipped acceleration channel of the decoded trajectory                            */
    float speed_limit;                 /* m/s   */
    float acc_limit;                   /* m/s^2 */
    const float* speed_limit_scale;    /* [B] or NULL */
    const float* acc_limit_scale;      /* [B] or NULL */
    /* TargetPosAtTimeLoss (guidance_loss.py:632-670): sum_b target_pos_scale[b] * |(x, y)[target_time[b]] - target_pos[b]|,
     * differentiated through the whole unicycle roll-out (positions, yaw, the speed-dependent yaw-rate bound);
     * off when target_pos_scale is NULL */
    const float* target_pos;           /* [B,2] waypoint in the agent frame */
    const int32_t* target_time;        /* [B] >= 0: index 0..51 of the trajectory state that should hit it;
                                        *     < 0: TargetPosLoss (:672-716) instead -- hit it at SOME state >= m = -(value + 1):
                                        *          target_pos_scale[b] * mean_{t >= m} softmin_t(dist) * dist_t^2 */
    const float* target_pos_scale;     /* [B] or NULL */
    /* Any other loss: ext_grad [B,52,6] = dL/dtraj on the DESCALED trajectory (x, y, v, yaw, acc, yaw-rate) that cld_decode
     * returns for this mean -- e.g. from autograd over upstream's own guidance losses (agent / map collision, ...), which
     * are torch code on that trajectory.  The step then uses J^T ext_grad, J = d traj / d mean (decoder + roll-out); with
     * cld_guidance_step(..., grad) this is the vector-Jacobian product itself.  NULL = no such term. */
    const float* ext_grad;
    /* Guidance on the t = 0 OUTPUT of the chain (upstream `apply_guidance_output`, diffuser.py:877-880; off in upstream's
     * defaults, scene_edit_config.py:84-91): when non-zero the final posterior mean takes one optimiser step with its own
     * settings (`final_step_opt_params`) and x0 is the guided mean (no noise is added at t = 0).  no_intermediate != 0
     * switches the per-step guidance at t > 0 off (upstream `apply_guidance_intermediate = False`); the struct zero-initialised
     * keeps the defaults: intermediate on, output off.  Fields follow lr / perturb_th / optimizer above; final_perturb_th < 0 = no
     * clip, which is what upstream's perturb() does (see the clipping note above).  The output step has no golden vector in the
     * reference (off in every shipped config): PARITY UNPINNED beyond the oracle's restatement. */
    int32_t apply_output;
    int32_t no_intermediate;
    float final_lr;
    float final_perturb_th;
    int32_t final_optimizer;
    /* Round 3 (appended: a struct zero-initialised below this line keeps every earlier behaviour).
     * grad_steps > 1: that many optimiser steps per guided denoising step, each on a fresh decode of the current iterate, with
     * the optimiser's state carried across them as upstream's perturb() does (guidance_loss.py:2247-2278: ONE torch.optim.Adam
     * per call -- moments and bias correction continue from step to step; the clip, when on, is taken around the initial mean).
     * 0 and 1 both mean one step.  final_grad_steps: the same for the output step (final_step_opt_params). */
    int32_t grad_steps;
    int32_t final_grad_steps;
    /* guide_clean != 0: upstream's `guide_clean=True` (diffuser.py:866-873): the optimiser steps act on the model's CLEAN
     * prediction x0_hat = sqrt(1 / acp_t) x_t - sqrt(1 / acp_t - 1) eps instead of on the posterior mean, and x_{t-1} is that
     * guided x0_hat + sigma_t z (upstream does not re-derive the posterior from it unless guide_clean == "video_diff": that mode,
     * reconstruction guidance, has calls of its own in include/cld_recon.h and does not read this field).  PARITY UNPINNED beyond the oracle's restatement: no shipped config turns it on. */
    int32_t guide_clean;
    /* AgentCollisionLoss (guidance_loss.py:442-630) as a term of the guidance loss: every guided step decodes the current
     * iterate, evaluates the loss and its gradient w.r.t. the decoded plans on the device (cld_agent_collision) and feeds it
     * to the step as ext_grad (added to a caller ext_grad).  NULL = no such term.  Counts as a loss term for the
     * "at least one term" rule. */
    const struct cld_collision* collision;
    /* MapCollisionLoss (guidance_loss.py:717-875) as a term, same mechanics (cld_map_collision_loss).  NULL = none. */
    const struct cld_map_collision* map_collision;
} cld_guidance;

/* Upstream's AgentCollisionLoss (src/tbsim/utils/guidance_loss.py:442-630) as configured through DiffuserGuidance
 * (:2143-2172): agents are `num_disks` disks of radius width / 2 along their axis; two agents of one scene collide at a step when
 * their closest disk centres are within r_i + r_j + buffer_dist; penalty 1 - dist / bound, weighted by decay_rate^t (normalised),
 * summed over the steps, averaged over ALL agents of the batch (upstream's .mean(-1) over B), zero for agents slower than
 * moving_speed_th.  total = sum over scenes of scene_weight[s] * mean over the scene's guided agents (x samples); stationary and
 * unguided agents receive no gradient (:512-534).  Agents A = B / num_samp; rows of traj are sample-minor (row = agent * num_samp
 * + sample), sample n of every agent living in scene copy n.  `excluded`: upstream's `excluded_agents` (:447,586-593) -- a pair whose agents are BOTH
 * flagged is not penalised.  Contract on max_scene_agents: the launch sizes its LDS and grid from it; a scene whose device-side
 * scene_start holds MORE agents is not evaluated -- its agents get NaN values and a gradient of grad_in (or 0). */
typedef struct cld_collision {
    const float* extent;            /* DEVICE [A,3] length, width, height                                                   */
    const float* world_from_agent;  /* DEVICE [A,3,3] row-major (rotation + translation of the agent frame in the world)     */
    const float* curr_speed;        /* DEVICE [A] m/s                                                                       */
    const int32_t* scene_start;     /* DEVICE [num_scenes + 1]: agents scene_start[s] .. scene_start[s + 1] - 1 form scene s
                                     * (consecutive blocks covering 0 .. A, as unique_consecutive(scene_index) implies)     */
    const float* scene_weight;      /* DEVICE [num_scenes]: weight of the scene's agent_collision config, 0 = not guided    */
    const uint8_t* guided;          /* DEVICE [A] or NULL: 1 = the agent is among the config's `agents` (NULL: all of them) */
    int32_t num_scenes;
    int32_t num_samp;
    int32_t num_disks;              /* 1..8 (upstream default 5)                                                            */
    int32_t max_scene_agents;       /* largest scene_start[s + 1] - scene_start[s] (sizes the kernel's LDS; <= 192)         */
    float buffer_dist;              /* upstream default 0.2                                                                 */
    float decay_rate;               /* 0.9                                                                                  */
    float moving_speed_th;          /* 0.5                                                                                  */
    const uint8_t* excluded;        /* DEVICE [A] or NULL: 1 = the agent is in the config's `excluded_agents`                */
} cld_collision;

/* The loss above on given plans: traj [B,52,6] descaled (what cld_decode returns) -> loss [B] = the per-agent values upstream
 * files under `guide_losses` (unweighted; 0 for stationary agents) and grad [B,52,6] = d total / d traj (+ grad_in when given).
 * Either output may be NULL. */
int cld_agent_collision(cld_handle h, const float* traj, const cld_collision* c, const float* grad_in, float* loss, float* grad,
                        int32_t B, void* stream);

/* Upstream's MapCollisionLoss (src/tbsim/utils/guidance_loss.py:717-875): the agent's box is sampled on a num_points_l x
 * num_points_w grid at every step of the plan; a sample is off road where the drivable map is 0 at its raster pixel (truncated,
 * clamped); steps where some but not all samples are off road contribute, per off-road sample, 1 - (distance to the nearest
 * on-road sample) / (box diagonal); steps weighted by decay_rate^t (normalised); agents slower than moving_speed_th contribute
 * nothing.  total = sum over scenes of scene_weight[s] * mean over the scene's agents (x samples) -- upstream itself can only
 * run this loss on a single-scene batch without an `agents` subset (it indexes the full-batch speeds with the masked batch size,
 * :857-859); scenes here are independent, which is the evident intent.  Rows of traj are sample-minor as in cld_collision. */
typedef struct cld_map_collision {
    const float* extent;             /* DEVICE [A,3]                                           */
    const float* raster_from_agent;  /* DEVICE [A,3,3] row-major                               */
    const uint8_t* drivable_map;     /* DEVICE [A,H,W], non-zero = drivable; NULL: cld_set_map_source */
    const float* curr_speed;         /* DEVICE [A]                                             */
    const int32_t* scene_start;      /* DEVICE [num_scenes + 1]                                */
    const float* scene_weight;       /* DEVICE [num_scenes], 0 = scene not guided              */
    int32_t num_scenes;
    int32_t num_samp;
    int32_t H, W;
    int32_t num_points_l, num_points_w;   /* upstream default (10, 10); product <= 256         */
    float decay_rate;                /* 0.9                                                    */
    float moving_speed_th;           /* 0.5                                                    */
} cld_map_collision;

/* traj [B,52,6] descaled -> loss [B] (per-plan values, as upstream files them) and grad [B,52,6] = d total / d traj
 * (+ grad_in when given; grad_in may be grad itself).  Either output may be NULL. */
int cld_map_collision_loss(cld_handle h, const float* traj, const cld_map_collision* c, const float* grad_in, float* loss,
                           float* grad, int32_t B, void* stream);

/* The map term without a per-agent raster: the scene's semantic maps, kept on the handle (the struct is copied by value; NULL clears it).
 * While a source is set, a cld_map_collision with drivable_map == NULL is legal -- in cld_map_collision_loss and, as a term, in
 * cld_guidance_step, cld_sample_step and cld_sample_guided -- and the flag of raster pixel (ix, iy) of agent a is drv(a; ix, iy) as defined
 * for cld_scene_metrics below, evaluated at the pose world[a]: the byte cld_rasterize writes to drivable[a, iy, ix] for an agent standing
 * there with this px_per_m / ego_center / no_map_fill and height, width = the term's H, W -- bit for bit, layer `drivable_layer` in place of
 * plane 0.  (ix, iy) is raster_from_agent applied to the sample point, truncated and clamped to H x W, exactly as in raster mode.  The map
 * of agent a is scene_map[s], s = a's scene in the term's OWN scene_start; num_scenes must agree with the term's (CLD_ERR_ARG).  Off
 * road = the map value == 0; a pixel outside the map, a scene with scene_map < 0 (or >= num_maps) and maps == NULL take no_map_fill
 * under the same rule, so the default fill of -1 is drivable.  world is read at every launch: refresh it (or set the source anew) when
 * the agents have moved.  With a non-NULL drivable_map the source is ignored and the results are what they are without one.  Without a
 * source drivable_map == NULL is CLD_ERR_ARG.  CLD_ERR_ARG at set time (nothing is skipped silently): NULL world, num_scenes < 1,
 * px_per_m <= 0, drivable_layer outside [0, n_sem), maps without their companions.  (A setter and not a field of cld_map_collision:
 * that struct's layout is frozen.) */
typedef struct cld_map_source {
    const float*   maps;            /* DEVICE [num_maps, n_sem, map_h, map_w] or NULL */
    const int32_t* scene_map;       /* DEVICE [num_scenes], < 0: no map (everything takes no_map_fill) */
    const float*   map_from_world;  /* DEVICE [num_maps,3,3] */
    const float*   world;           /* DEVICE [A,3] (x, y, h): the pose agent a's frame stands at */
    int32_t num_scenes, num_maps, n_sem, map_h, map_w, drivable_layer;
    float   px_per_m, ego_center[2], no_map_fill;
} cld_map_source;
int cld_set_map_source(cld_handle h, const cld_map_source* m);   /* NULL clears */

/* Upstream's GlobalTargetPosLoss (`global_target_pos`) and GlobalTargetPosAtTimeLoss (`global_target_pos_at_time`),
 * src/tbsim/utils/guidance_loss.py:876-1135: a waypoint in the WORLD frame, taken into the agent frame of the current plan
 * (p = agent_from_world[a] target_pos[a]), H = 52, d_t = |pos_t - p|.  Per agent, by kind[a]:
 *   0  off: value 0, no gradient
 *   1  |p| <  H dt pref_speed: TargetPosLoss with min_target_time = 0, mean_t(softmin_t(d) d_t^2)
 *      otherwise:              relu(max(urgency H dt pref_speed, min_progress_dist) - (d_0 - d_51))
 *   2  lt = target_time[a] - global_t:  lt < 0: 0;  0 <= lt < H: d_lt (TargetPosAtTimeLoss);
 *      lt >= H: relu(d_51 - lt dt pref_speed (1 - urgency))
 * Agents with reached[a] != 0 (upstream's have_reached_mask; the caller keeps it across plans) have value 0 and no gradient.
 * Agents A = B / num_samp; rows of traj are sample-minor as in cld_collision.  The arrays stay the caller's. */
typedef struct cld_goal {
    const float* target_pos;        /* DEVICE [A,2] world frame                                                           */
    const float* agent_from_world;  /* DEVICE [A,3,3] row-major                                                           */
    const int32_t* kind;            /* DEVICE [A] 0 / 1 / 2, see above                                                    */
    const int32_t* target_time;     /* DEVICE [A] target time of kind 2 in rollout steps (the same clock as global_t)     */
    const float* urgency;           /* DEVICE [A] in [0, 1]                                                               */
    const float* pref_speed;        /* DEVICE [A] m/s (upstream default 1.42)                                             */
    const float* scale;             /* DEVICE [A] d total / d value: weight / agents of the config                        */
    const uint8_t* reached;         /* DEVICE [A] or NULL                                                                 */
    int32_t num_samp;
    int32_t global_t;               /* rollout step of this plan (upstream update_guidance(global_t=step_index))          */
    float dt;                       /* 0.1                                                                                */
    float min_progress_dist;        /* 0.5                                                                                */
} cld_goal;

/* The loss above on given plans: traj [B,52,6] descaled -> loss [B] = the unweighted per-row values, as upstream files them
 * under `guide_losses`, and grad [B,52,6] = grad_in (when given; may be grad itself) + scale[agent] * d value / d traj: only the
 * x, y columns of the steps the value reads get a contribution.  Either output may be NULL.  Deterministic: no atomics. */
int cld_goal_loss(cld_handle h, const float* traj, const cld_goal* g, const float* grad_in, float* loss, float* grad,
                  int32_t B, void* stream);

/* Keep a goal term on the handle (the struct is copied by value; NULL clears it).  While one is set, every guided call
 * (cld_sample_guided, cld_sample_step, cld_guidance_step) adds it to the guidance loss: each optimiser step decodes the current
 * iterate as for the collision terms, and the gradient above joins the caller's ext_grad and the collision gradients as the
 * guidance kernel's ext_grad.  A set term counts as a loss term of the `cld_guidance` it is used with.  (A setter and not a
 * pointer in cld_guidance: that struct's layout is frozen.) */
int cld_set_goal_term(cld_handle h, const cld_goal* g);

/* Upstream's SocialGroupLoss (`social_group`, src/tbsim/utils/guidance_loss.py:1137-1207): the members of a group keep social_dist
 * to one another.  Group g holds the agents member[group_start[g] .. group_start[g + 1]) (ascending; M of them, an agent in at most
 * one group).  For every sample n and step t the members' positions go to the world frame (world_from_agent[a] (x, y)) and member i
 * (its position in the group) is paired with
 *     nb(i) = u < cohesion[g] ? (r < i ? r : r + 1) : argmin_{j != i} |p_i - p_j|      (lowest j on a tie)
 * where (r, u) is the draw of (row of the member's plan, t) in this evaluation: r uniform in [0, M - 2], u uniform in [0, 1), compared
 * in fp32.  value[i, n] = mean_t (|p_i - p_nb(i)| - social_dist[g])^2; the term's total is sum over member rows of scale[g] * value
 * (scale = d total / d value of a member row: weight / (M * samples) reproduces upstream's weight * mean over [M, N]).
 * The LEADER is the member whose agent index equals leader[g] (-1, or an index that names no member: nobody).  Upstream's docstring
 * calls leader_idx "the index in the scene", but its code compares it with the BATCH index of the agent (:1159-1170); the code is
 * followed here, so leader[] holds batch (agent) indices.  The leader's position is detached: it receives no gradient, neither for
 * its own term nor as somebody's neighbour; its value still counts, and its neighbour receives the gradient of the leader's term.
 * Every other pair term sends its gradient to both ends; the norm's gradient at distance 0 is 0; only the x, y columns receive
 * anything (rotated back by R_a^T).  Distances are differences of positions formed directly in fp32 (no matrix-product form).
 * Draws: draw_r / draw_u, both given or both NULL.  Given: DEVICE [n_iter, n_opt, B, 52] over ALL plan rows (sample-minor; rows of
 * non-members are ignored; r is clamped to [0, M - 2]) -- evaluation (it, k) of a guided call reads slab [it, k]: it = the loop
 * iteration of cld_sample_guided (0 in cld_sample_step / cld_guidance_step), k = the optimiser step - 1; cld_social_group_loss reads
 * slab [0, 0].  NULL: the library's counter-based generator, keyed by (seed, a stream tag of its own -- no value is shared with the
 * diffusion noise --, the evaluation index (iter_base + it, k), row * 52 + t); cohesion == 0 draws nothing.  A chain stepped through
 * cld_sample_step with iter_base = 0, 1, ... therefore draws what cld_sample_guided draws with iter_base = 0.
 * Contract on max_members (as cld_collision.max_scene_agents): the launch sizes its LDS and grid from it; a group whose device-side
 * group_start holds MORE members -- or fewer than 2, which upstream cannot run -- is not evaluated: its members get NaN values and a
 * gradient of grad_in (or 0).  2 <= max_members <= 128 (CLD_ERR_ARG beyond).  Rows outside every group: value 0, gradient grad_in.
 * Deterministic: no atomics, the same bits on every run.  Agents A = B / num_samp. */
typedef struct cld_social_group {
    const int32_t* group_start;     /* DEVICE [num_groups + 1] offsets into member                                          */
    const int32_t* member;          /* DEVICE [group_start[num_groups]] agent indices, ascending within a group             */
    const int32_t* leader;          /* DEVICE [num_groups] agent (batch) index of the group's leader, or -1                 */
    const float* social_dist;       /* DEVICE [num_groups] metres (upstream default 1.5)                                    */
    const float* cohesion;          /* DEVICE [num_groups] in [0, 1] (0.8)                                                  */
    const float* scale;             /* DEVICE [num_groups] d total / d value of a member row                                */
    const float* world_from_agent;  /* DEVICE [A,3,3] row-major                                                             */
    const int32_t* draw_r;          /* DEVICE [n_iter, n_opt, B, 52] or NULL                                                */
    const float* draw_u;            /* DEVICE [n_iter, n_opt, B, 52] or NULL                                                */
    uint64_t seed;                  /* generator seed (draws NULL)                                                          */
    int32_t num_groups;
    int32_t num_samp;
    int32_t max_members;            /* largest group (sizes the kernel's LDS; 2..128)                                       */
    int32_t iter_base;              /* evaluation index of the call's first loop iteration (generator only)                 */
    int32_t n_iter;                 /* leading extents of the caller draws                                                  */
    int32_t n_opt;
} cld_social_group;

/* The loss above on given plans: traj [B,52,6] descaled -> loss [B] = the unweighted per-row values (0 outside the groups) and
 * grad [B,52,6] = grad_in (when given; may be grad itself) + d total / d traj.  Either output may be NULL. */
int cld_social_group_loss(cld_handle h, const float* traj, const cld_social_group* term, const float* grad_in, float* loss,
                          float* grad, int32_t B, void* stream);

/* Keep a social-group term on the handle (the struct is copied by value; NULL clears it).  While one is set, every guided call
 * (cld_sample_guided, cld_sample_step, cld_guidance_step) decodes the current iterate at every optimiser step and adds the term's
 * gradient after the goal term's; it counts as a loss term of the `cld_guidance` it is used with.  Caller draws that do not cover
 * the call -- n_iter < its loop iterations (1 for the two step calls) or n_opt < max(grad_steps, final_grad_steps, 1) -- are
 * CLD_ERR_ARG, decided before anything is launched.  (A setter and not a pointer in cld_guidance: that struct's layout is frozen.) */
int cld_set_social_term(cld_handle h, const cld_social_group* term);

/* Upstream's pair-relation losses (src/tbsim/utils/guidance_loss.py): `gptkeepdistance` (KeepDistanceLoss, :1631-1688), `gptcollision`
 * (CollisionLoss, :1691-1734), and the four classes of the same family upstream reaches only through its language-model front end:
 * StayAwayLoss (:2014-2082) / KeepDistanceLoss2 (:1739-1791), FrontCollisionLoss (:1844-1896), CollideLeftSideLoss (:1899-1956).
 * Pair p = (target[p], ref[p]), agent (batch) indices.  For every sample n and step t the plan positions of both agents go to the
 * world frame (world_from_agent[a] (x, y)) and into the REF agent's static frame: q = M (p_target - p_ref), M the rotation of
 * agent_from_world[ref] (NULL: the transpose of world_from_agent[ref]'s); the frame does not follow the plan's yaw.  d = |q|
 * (CLD_PAIR_COLLISION: the world distance, as upstream takes it).  The step's term e_t:
 *     CLD_PAIR_KEEP_DISTANCE     relu(lo - d) + relu(d - hi)
 *     CLD_PAIR_COLLISION         relu(d - lo)                                  (lo = collision_radius; hi unused)
 *     CLD_PAIR_STAY_AWAY         relu(d - hi) + relu(lo - d)                   (KeepDistanceLoss2's `where` form equals it for lo <= hi)
 *     CLD_PAIR_FRONT_COLLISION   |Dx| + relu(-Dy),  D = -q = ref - target in the ref frame
 *     CLD_PAIR_COLLIDE_LEFT      |Dx| + relu(Dy)
 * value[p, n] = sum_t w_t e_t, w_t = 1 / 52, or with decay[p] > 0: decay^t / sum_t decay^t / 52 -- normalised AND divided by 52, as
 * upstream does.  The term's total is sum over (p, n) of scale[p] * value[p, n] (scale = weight / num_samp reproduces upstream's
 * weight * mean over the samples).  Both agents receive gradient, nothing is detached; only the x, y columns of the plans receive
 * anything.  relu passes the gradient where its argument is >= 0 (torch.clip), the norm's gradient at d = 0 is 0, abs at 0 gives 0.
 * An agent may sit in several pairs in either role, so the gradient is a gather: the caller lists, per involved agent, its
 * incidences pair * 2 + role (role 0 = target, 1 = ref) in ascending order -- agent_id[k]'s are incidence[agent_start[k] ..
 * agent_start[k + 1]); every agent_id once.  The order fixes the summation order.  Upstream runs these classes on a single-scene batch
 * only (it indexes full-batch frames with masked plans, the defect recorded for MapCollisionLoss above); here the pairs of all scenes
 * go into one launch.
 * Contract on the device-side indices (as cld_social_group.max_members): a pair whose target or ref lies outside [0, A), or with
 * target == ref, is not evaluated -- NaN value, no contribution; incidences that point outside the arrays or name a pair their agent
 * is not part of are skipped.  NOT checked: that agent_id lists every agent once -- a duplicated agent_id stays inside the arrays, but
 * two threads then add to one row and the bits of that row are no longer the same on every run.  Rows in no pair: gradient grad_in.  Deterministic: no atomics, the same bits on every run; plain fp32
 * in both precisions.  Agents A = B / num_samp. */
enum { CLD_PAIR_KEEP_DISTANCE = 0, CLD_PAIR_COLLISION = 1, CLD_PAIR_STAY_AWAY = 2, CLD_PAIR_FRONT_COLLISION = 3, CLD_PAIR_COLLIDE_LEFT = 4 };
typedef struct cld_pair_term {
    const int32_t* target;          /* DEVICE [num_pairs] agent (batch) index                                               */
    const int32_t* ref;             /* DEVICE [num_pairs]                                                                   */
    const int32_t* kind;            /* DEVICE [num_pairs] CLD_PAIR_*                                                        */
    const float* lo;                /* DEVICE [num_pairs] min distance, or the collision radius                             */
    const float* hi;                /* DEVICE [num_pairs] max distance                                                      */
    const float* decay;             /* DEVICE [num_pairs] <= 0: a plain mean over the steps                                 */
    const float* scale;             /* DEVICE [num_pairs] d total / d value of a (pair, sample)                             */
    const float* world_from_agent;  /* DEVICE [A,3,3] row-major                                                             */
    const float* agent_from_world;  /* DEVICE [A,3,3] or NULL                                                               */
    const int32_t* agent_start;     /* DEVICE [num_involved + 1] offsets into incidence                                     */
    const int32_t* agent_id;        /* DEVICE [num_involved] the agents that sit in a pair, each once                       */
    const int32_t* incidence;       /* DEVICE [num_incidences] pair * 2 + role, ascending per agent                         */
    int32_t num_pairs;
    int32_t num_samp;
    int32_t num_involved;
    int32_t num_incidences;
} cld_pair_term;

/* The losses above on given plans: traj [B,52,6] descaled -> value [num_pairs, num_samp] (unweighted, as upstream's classes return
 * them) and grad [B,52,6] = grad_in (when given; may be grad itself) + d total / d traj.  Either output may be NULL. */
int cld_pair_loss(cld_handle h, const float* traj, const cld_pair_term* term, const float* grad_in, float* value, float* grad,
                  int32_t B, void* stream);

/* Keep a pair term on the handle (the struct is copied by value; NULL clears it).  While one is set, every guided call
 * (cld_sample_guided, cld_sample_step, cld_guidance_step) adds its gradient after the social-group term's, on the same decoded
 * iterate; it counts as a loss term of the `cld_guidance` it is used with.  A malformed term is CLD_ERR_ARG, decided before anything
 * is launched.  (A setter and not a pointer in cld_guidance: that struct's layout is frozen.) */
int cld_set_pair_term(cld_handle h, const cld_pair_term* term);

/* cld_sample (non_cond == NULL) / cld_sample_cfg (non_cond != NULL) with the guidance step above inside the loop. */
int cld_sample_guided(cld_handle h, const float* x_T, const float* noise, const float* cond, const float* non_cond,
                      float guidance_w, const cld_guidance* guidance, int32_t steps, float* x0, float* x1, float* logp,
                      int32_t B, uint64_t seed, void* workspace, size_t workspace_bytes, void* stream);

/* ONE iteration of the loop of cld_sample / cld_sample_cfg / cld_sample_guided at timestep t_idx, teacher-forced: upstream's
 * DiffuserModel.p_sample (src/tbsim/models/diffuser.py:844-929), CLD's DmModel.x_Tminus1 (models/dm/dm_model.py:144-156) when
 * non_cond and guidance are NULL.  x_t [B,52,4] -> U-Net (twice with non_cond != NULL: eps = (1 + w) eps_c - w eps_u) ->
 * posterior mean -> [guidance step on the mean when `guidance` is given and applies at this timestep] -> x_next = mean' + sigma_t z
 * (no noise at t_idx == 0; z NULL = the on-device generator with seed 0, step 0).  Outputs [B,52,4], any may be NULL: x_next; mean = the posterior mean BEFORE the
 * guidance step; mean_guided and grad = dL/dmean are written only on a guided step; *sigma_host receives sigma_t = exp(0.5 *
 * logvar[t_idx]) as the loop uses it.  Same kernels in the same order as the
 * loop: stepping through t = n-1 .. 0 with the loop's noise slabs reproduces cld_sample* bit for bit.  Workspace as for the
 * corresponding cld_sample* call (2 * pad16(B) agents with non_cond). */
int cld_sample_step(cld_handle h, const float* x_t, const float* cond, const float* non_cond, float guidance_w,
                    const cld_guidance* guidance, int32_t t_idx, const float* z, float* x_next, float* mean, float* mean_guided,
                    float* grad, float* sigma_host /*HOST*/, int32_t B, void* workspace, size_t workspace_bytes, void* stream);

/* One guidance step on a given posterior mean [B,52,4] (teacher-forced form of the above, for tests and for callers that
 * drive the loop themselves): mean_guided = mean + clip(delta); x_next = mean_guided + sigma * z; grad = dL/dmean.
 * Outputs [B,52,4], any may be NULL. */
int cld_guidance_step(cld_handle h, const float* mean, const float* cond, const cld_guidance* guidance, float sigma,
                      const float* z, float* mean_guided, float* x_next, float* grad, int32_t B,
                      void* workspace, size_t workspace_bytes, void* stream);

/* out = DmModel.log_prob(x_t, x_{t-1}, aux_info, t)  (dm_model.py:165-174):
 * mean over (T, D) of log N(x_{t-1}; mean(x_t, eps), sigma_t).  Forward only. */
int cld_log_prob(cld_handle h, const float* x_t, const float* x_tm1, const float* cond, int32_t t_idx,
                 float* out /*[M]*/, int32_t M, void* workspace, size_t workspace_bytes, void* stream);

/* act = LSTMVAE.lstm_dec(z, cond)  (models/vae/lstm_vae.py:44-52), z [B,52,4],
 * cond [B,256] -> act [B,52,2] (scaled acceleration, yaw-rate). */
int cld_lstm_decode(cld_handle h, const float* z, const float* cond, float* act, int32_t B, void* stream);

/* traj = VaeModel.convert_action_to_state_and_action(act, curr_states,
 *        scaled_input, descaled_output)  (models/vae/vae_model.py:100-129) with
 * unicyle_forward_dynamics(mode='parallel') (src/tbsim/models/diffuser_helpers.py:541-639).
 * act [B,52,2], curr_states [B,4] = (x, y, v, yaw) -> traj [B,52,6]. */
int cld_action_to_state(cld_handle h, const float* act, const float* curr_states, float* traj,
                        int32_t B, int32_t scaled_input, int32_t descaled_output, void* stream);

/* Both of the above in one launch (guide_dm_trainer.py:97-98): z -> traj [B,52,6];
 * act_out [B,52,2] optional (NULL to skip). */
int cld_decode(cld_handle h, const float* z, const float* cond, const float* curr_states,
               float* traj, float* act_out, int32_t B, int32_t descaled_output, void* stream);

/* z, mu, logvar = LSTMVAE.traj2z(x, context)  (models/vae/lstm_vae.py:87-99; encoder :6-26): 2-layer LSTM(6->64)
 * with h0 = cond2hidden(context), mu / logvar heads 64->4, z = mu + noise * exp(0.5 * logvar).
 * x6_scaled [B,52,6] = scaled (x, y, v, yaw, acc, yaw-rate); noise [B,52,4] is the caller's randn_like draw
 * (lstm_vae.py:97; NULL -> z = mu); outputs [B,52,4], any may be NULL.  Weights: "lstm_enc.*", "mu.*", "logvar.*". */
int cld_traj2z(cld_handle h, const float* x6_scaled, const float* cond, const float* noise, float* z, float* mu,
               float* logvar, int32_t B, void* stream);

/* VaeModel.compute_vae_loss (models/vae/vae_model.py:89-99), forward only: recon = mse(x6_scaled[..., 4:6], act_out),
 * kld = -0.5 * sum(1 + logvar - mu^2 - exp(logvar)) / (B * 52), loss = recon + beta * kld.  out3 = (loss, recon, kld), DEVICE;
 * workspace >= 2 * B floats (cld_workspace_bytes(h, B) is more than enough). */
int cld_vae_loss(cld_handle h, const float* x6_scaled, const float* act_out, const float* mu, const float* logvar, float beta,
                 float* out3, int32_t B, void* workspace, size_t workspace_bytes, void* stream);

/* convert_state_to_state_and_action(traj_state, vel_init, dt)  (src/tbsim/models/diffuser_helpers.py:685-749) as
 * called by get_state_and_action_from_data_batch (models/context_utils.py:64-70): positions [B,52,2], yaws [B,52,1],
 * curr_speed [B] -> [B,52,6]; scaled_output != 0 also applies VaeModel.scale_traj (vae_model.py:131-155). */
int cld_state_to_state_and_action(cld_handle h, const float* positions, const float* yaws, const float* curr_speed,
                                  float* out6, int32_t B, int32_t scaled_output, void* stream);

/* aux_info['cond_feat'] = ContextEncoder.forward(data_batch)  (models/context_utils.py:40-61):
 *   process_cond_mlp([agent_state_encoder(curr_states) | map_encoder(image)])
 * image [B,34,224,224] fp32 NCHW (data_batch['image']: 31 history planes + 3 semantic planes,
 * src/tbsim/utils/trajdata_utils.py:409-420), read in place -- no re-layout pass; curr_states [B,4] = (x, y, v, yaw) as
 * batch_utils.get_current_states builds them (src/tbsim/utils/batch_utils.py:46-65); cond_feat [B,256];
 * map_feat [B,256] optional (NULL to skip): the resnet18 'fc' output MapEncoder returns (diffuser_helpers.py:313-341).
 * The map branch is torchvision's resnet18 (eval-mode BatchNorm) with the 34-channel stem and the 512 -> 256 fc of
 * RasterizedMapEncoder (src/tbsim/models/base_models.py:559-614).  Weights: "context_encoder.*" keys of
 * VaeModel.state_dict() (a leading "vae." is accepted); "*.num_batches_tracked" entries are ignored.
 * Agents are processed in passes of <= 256, so the scratch (cld_context_workspace_bytes) is bounded by ~1.4 GB. */
size_t cld_context_workspace_bytes(cld_handle h, int32_t B);
int cld_context_encode(cld_handle h, const float* image, const float* curr_states, float* cond_feat, float* map_feat,
                       int32_t B, void* workspace, size_t workspace_bytes, void* stream);

/* The state branch and the combine MLP of ContextEncoder.forward on a map feature that is already known:
 * cond = process_cond_mlp([agent_state_encoder(curr_states) | map_feat]).  Serves classifier-free guidance: upstream's
 * unconditional features (src/tbsim/models/diffuser.py:390-411,459-471) are exactly this with the map feature of a raster
 * filled with -1, which is the same row for every agent (broadcast != 0: map_feat is [1,256]; else [B,256]). */
int cld_context_combine(cld_handle h, const float* map_feat, int32_t broadcast, const float* curr_states, float* cond_feat,
                        int32_t B, void* stream);

/* PPO reward of the reference (models/rl/criticmodel.py:7-64), per agent:
 *   offroad   = -#timesteps whose position, mapped to the raster with raster_from_agent (transform_points_tensor, :88-112),
 *               rounded (half to even) and clamped, falls on a non-drivable pixel of drivable_map                  (:13-29)
 *   collision = -#(other agent, timestep < T_other) within collision_thresh (0.8 m) and available                  (:42-64)
 *   reward    = offroad + collision - 0.1 * mean_t |acc_{t+1} - acc_t| / 0.1 on traj_scaled[..., 4]                (:33-38)
 * traj [B,52,6] descaled, traj_scaled [B,52,6] (NULL: no jerk term), raster_from_agent [B,3,3], drivable_map [B,H,W] bytes
 * (non-zero = drivable), other_pos [B,S,T_other,2], other_avail [B,S,T_other] bytes; outputs [B], any may be NULL.
 * (The reference's compute_reward unpacks a 4-D trajectory and then calls 3-D-only helpers, so it cannot run as written;
 * this is the per-agent quantity its helpers define, num_samp = 1.) */
int cld_compute_reward(cld_handle h, const float* traj, const float* traj_scaled, const float* raster_from_agent,
                       const uint8_t* drivable_map, int32_t H, int32_t W, const float* other_pos, const uint8_t* other_avail,
                       int32_t S, int32_t T_other, float collision_thresh, float* reward, float* offroad, float* collision,
                       int32_t B, void* stream);

/* Per-agent values of the built-in guidance losses on decoded trajectories, as upstream reports them in `guide_losses`
 * (DiffuserGuidance.compute_guidance_loss, src/tbsim/utils/guidance_loss.py:2143-2172: the unweighted `(B, N)` value of each
 * loss; diffuser.py:924-926 evaluates them on the final output for sample selection, algos.py:2057-2064):
 *   losses[b,0] TargetSpeedLoss        mean_t |v_t - target_speed[b,t]|                    (guidance_loss.py:219-254)
 *   losses[b,1] SpeedLimitLoss         mean_t relu(|v_t| - speed_limit)                    (:1509-1538)
 *   losses[b,2] AccLimitLoss           mean_t relu(|acc_t| - acc_limit)                    (:1444-1467)
 *   losses[b,3] TargetPosAtTimeLoss    |(x, y)[target_time[b]] - target_pos[b]|            (:632-670), or for target_time < 0
 *               TargetPosLoss          mean_{t >= m} softmin_t(dist) dist_t^2              (:672-716)
 * A term that is off for agent b (its pointer NULL or its scale[b] == 0) is NaN, as upstream fills agents outside a loss's mask.
 * traj [B,52,6] descaled (x, y, v, yaw, acc, yaw-rate) as cld_decode returns it; losses [B,4]. */
int cld_guidance_losses(cld_handle h, const float* traj, const cld_guidance* guidance, float* losses, int32_t B, void* stream);

/* Closed-loop kinematic update of EnvUnifiedSimulation._step (src/tbsim/envs/env_trajdata.py:452-468) for plan step k
 * (the last of the n_step_action executed steps): traj [B,52,6] descaled (x, y, v, yaw, acc, yaw-rate) in the agent frame
 * at planning time, centroid [B,2], yaw [B] (world pose at planning time) -> world [B,3] = (x, y, h) with
 * xy = traj_xy[k] @ [[cos, sin], [-sin, cos]] + centroid, h = yaw + traj_yaw[k]; next_curr_states [B,4] (optional) =
 * (0, 0, v_k, 0), the agent-centric current state the next planning call conditions on (batch_utils.py:46-65). */
int cld_world_step(cld_handle h, const float* traj, const float* centroid, const float* yaw, int32_t k, float* world,
                   float* next_curr_states, int32_t B, void* stream);

/* The observation of the closed loop, built on the device from the scene: data_batch['image'] as upstream's parse_node_centric ->
 * rasterize_agents make it (src/tbsim/utils/trajdata_utils.py:123-156, 381-420), for rows [row0, row0 + B) of a scene set of B_all agents
 * (the rows of one rank; the histories cover every rank's agents).  Needs no weights.  For row r with pose (x, y, h) = hist_world[r, T_hist-1]:
 *   raster_from_agent = [[ppm, 0, (1 + ego_center[0]) / 2 * width], [0, ppm, (1 + ego_center[1]) / 2 * height], [0, 0, 1]]
 *   (config.yaml:81-86: ppm 2, ego_center (-0.5, 0), 224 x 224 -> offsets 56, 112).
 *   History planes t = 0 .. T_hist-1 (oldest first), rasterize_agents as written: a position goes to the agent frame, R(-h) (p - p_r), then
 *   through raster_from_agent, in fp32; an unavailable frame takes the raster position (0, 0); x is clamped to [0, width-1], y to
 *   [0, height-1], then rounded half to even; neighbours paint -1, the ego paints +1 on top; flat pixels 0 and height*width-1 are then set
 *   to 0.  A neighbour outside the raster therefore paints a border pixel (upstream's behaviour, kept).  Yaw is not drawn.
 *   Neighbours of r: the agents j != r of r's scene (scene_start, as in cld_collision) with hist_avail[j, T_hist-1] set and a current world
 *   distance <= max_neighbor_dist (config.yaml:96: 30; <= 0: the whole scene); each paints its own available frames.  This rule stands in for
 *   trajdata's neighbour selection, which is not part of the reference tree: PARITY UNPINNED.
 *   Semantic planes T_hist .. T_hist+n_sem-1, pixel (u, v): agent point ((u - ox) / ppm, (v - oy) / ppm), world point p_r + R(h) . it, map
 *   pixel rint(map_from_world[m] . world point), m = scene_map[scene]; value maps[m, layer, y, x] inside the map, else no_map_fill; every
 *   plane is no_map_fill when maps == NULL or m < 0.  Nearest-pixel sampling is this library's definition (trajdata's patch code is not part
 *   of the reference tree): PARITY UNPINNED.
 *   drivable [B, height, width] bytes = (plane T_hist != 0), upstream's .bool() of the drivable layer (trajdata_utils.py:185-196): fill
 *   pixels count as drivable.  raster_from_world [B,3,3] = raster_from_agent . agent_from_world.
 * Limits (CLD_ERR_ARG beyond them; nothing is skipped silently): a scene may hold any number of the B_all agents -- the neighbour loop
 * strides over the scene -- with B_all <= CLD_RASTER_MAX_AGENTS; height * width <= CLD_RASTER_MAX_PIXELS (the two paint masks of a plane
 * live in LDS); T_hist, n_sem <= CLD_RASTER_MAX_PLANES.  16-byte stores when height * width is a multiple of 4 and image is 16-byte
 * aligned (drivable 4-byte), dword stores otherwise.  The ContextEncoder itself still requires 34 x 224 x 224. */
#define CLD_RASTER_MAX_AGENTS (1 << 24)
#define CLD_RASTER_MAX_PIXELS (1 << 17)
#define CLD_RASTER_MAX_PLANES 1024
typedef struct cld_raster {
    const float*   hist_world;      /* DEVICE [B_all, T_hist, 3] world x, y, yaw; oldest first, frame T_hist-1 = now */
    const uint8_t* hist_avail;      /* DEVICE [B_all, T_hist] */
    const int32_t* scene_start;     /* DEVICE [num_scenes + 1] */
    const float*   maps;            /* DEVICE [num_maps, n_sem, map_h, map_w] or NULL */
    const int32_t* scene_map;       /* DEVICE [num_scenes], < 0: no map */
    const float*   map_from_world;  /* DEVICE [num_maps, 3, 3] */
    int32_t num_scenes, B_all, T_hist, n_sem, height, width, num_maps, map_h, map_w;
    float   px_per_m, ego_center[2], no_map_fill, max_neighbor_dist;
} cld_raster;

int cld_rasterize(cld_handle h, const cld_raster* r, int32_t row0, int32_t B,
                  float* image /*[B, T_hist+n_sem, H, W]*/, uint8_t* drivable /*[B,H,W] or NULL*/,
                  float* raster_from_world /*[B,3,3] or NULL*/, void* stream);

/* The episode metrics of a closed-loop rollout, kept on the device: what upstream registers for evaluation
 * (src/tbsim/evaluation/env_builders.py:37-50) as OffRoadRate, DiskOffRoadRate, CollisionRate, DiskCollisionRate, CriticalFailure and
 * Comfort (src/tbsim/envs/env_metrics.py:147-239, 241-311, 391-487, 489-580, 582-646, 1436-1501).  Needs no weights.
 * cld_scene_metrics_step is one environment step over all B_all agents of all scenes: world [B_all,3] (x, y, h) -> one accumulator row per
 * agent in `state` (cld_scene_metrics_state_bytes(B_all) bytes, 16-byte aligned, all-zero = empty, updated in place; opaque).
 * Agent i is VALID at a step when neither x nor y is NaN.  With ox, oy the raster offsets of cld_rasterize and drv(i; u, v) the byte
 * cld_rasterize writes to drivable[i, v, u] for an agent standing at this step's pose (agent point ((u - ox) / ppm, (v - oy) / ppm), rotated
 * by h, shifted to the world, map pixel rint(map_from_world . p) of layer `drivable_layer`, value != 0; fill and "no map" are drivable):
 *   off_road       (OffRoadRate.compute_per_step with use_center, tbsim/utils/metrics.py:451-481) valid: 1 - drv at the centroid's raster
 *                  pixel = (ox, oy) rounded half to even, then clamped to the raster; invalid: not counted (flags byte 255).
 *   off_road_disk  (DiskOffRoadRate, metrics.py:507-547) r = px_per_m min(e0, e1) / 2 (get_raster_pix2m() is px_per_m); 52 samples
 *                  (ox, oy) + (r k / 4) (cos a, sin a), k = 1 .. 4 (major), a = the 13 points of linspace(0, 2 pi, 13), both ends kept as
 *                  upstream does, (cos, sin) a constant table formed in double; each sample is clamped to the raster, rounded, clamped
 *                  again; 1 if any sample is not drivable.  Invalid: not counted (255).
 *   coll_disk      (DiskCollisionRate.compute_per_step) some valid j != i of i's scene has |p_i - p_j| < min(e_i) / 2 + min(e_j) / 2.
 *   coll_box, type (CollisionRate.compute_per_step -> geometry_utils.detect_collision:339-401) boxes with corners p +- (e0 / 2)(cos h, sin h)
 *                  +- (e1 / 2)(-sin h, cos h); the partner is the lowest-index valid j != i of the scene whose box overlaps i's
 *                  (separating-axis test on the four edge normals, touching counts); the type is the argmax (first wins) over the lengths
 *                  of i's front (+e0 / 2), rear, left (+e1 / 2) and right sides inside the partner's box (each segment clipped against the four
 *                  half-planes), remapped by min(index, 2): FRONT, REAR, SIDE.  PARITY UNPINNED: upstream decides both with shapely, which
 *                  is not available where the goldens are recorded; the two are held to a float64 restatement of this definition.
 *                  An invalid agent records 0 for the three collision quantities, as upstream does.
 *   comfort        (Comfort) R = ceil(stat_dt / sim_dt); on steps with step % R == 0 the pose joins a three-deep ring.  With dt = stat_dt:
 *                  vel = dpos / dt, speed = |vel|, acc = |dvel| / dt, lon = |acc cos h|, lat = |acc sin h| with the yaw of the FIRST of the
 *                  three positions (as upstream indexes it), jerk = |dacc| / dt.  Running sums (fp64) and counts; NaN terms are not counted.
 * flags [B_all,4] (optional): off_road, off_road_disk, coll_disk, box code 0 none / 1 FRONT / 2 REAR / 3 SIDE; partner [B_all] (optional):
 * the box partner's index, -1: none.  A scene may hold any number of agents (the partner loop strides over it).
 * cld_scene_metrics_read finalises the rows (either output may be NULL):
 *   per_agent [B_all, CLD_METRICS_AGENT_COLS]: steps seen, steps valid, off_road sum, off_road_disk sum, max over time of coll_any, FRONT,
 *     REAR, SIDE, coll_disk, any over time of off_road / of coll_any / of either, nanmean of speed, lon_acc, lat_acc, jerk (NaN: no term).
 *   per_scene [num_scenes, CLD_METRICS_SCENE_COLS], the values of get_episode_metrics:
 *     0, 1  OffRoadRate rate = flags summed over valid records / valid records (NaN for a scene without one), nframe = mean over the
 *           scene's agents of the per-agent sum (an agent without a valid record counts with 0, as pandas' sum does);
 *     2, 3  DiskOffRoadRate rate, nframe;  4 .. 7 CollisionRate FRONT, REAR, SIDE, coll_any: means over the scene's agents of the max over time;
 *     8     DiskCollisionRate coll_any;
 *     9 .. 11 CriticalFailure failure_offroad, failure_collision, failure_any: the share of the scene's agents that were off road / in a box
 *           collision / either at ANY step -- upstream's class discards its num_collision_frames / num_offroad_frames arguments
 *           (env_metrics.py:584-587), so one frame is a failure; NaN off_road records are skipped by pandas' any();
 *     12 .. 15 Comfort speed, lon_acc, lat_acc, jerk: nanmean over the scene's agents of the per-agent nanmean (NaN: no agent has a term).
 * CLD_ERR_ARG (nothing is skipped silently): NULL world / state / extent / scene_start, B_all or num_scenes < 1, height * width beyond
 * CLD_RASTER_MAX_PIXELS, px_per_m <= 0, maps without their companions, drivable_layer outside [0, n_sem), sim_dt <= 0 or stat_dt < sim_dt
 * (upstream's assert), step < 0.  The CONTENTS of scene_start are never validated by the library: it is device memory, and reading it
 * would need a synchronisation.  The caller guarantees 0 = scene_start[0] < ... < scene_start[num_scenes] = B_all (the Python layer checks
 * it on the host); the kernels clamp what they read from it, so a malformed split cannot make them read or write out of bounds, but
 * its metrics are then meaningless. */
#define CLD_METRICS_AGENT_COLS 16
#define CLD_METRICS_SCENE_COLS 16
typedef struct cld_scene_metrics {
    const float*   extent;          /* DEVICE [B_all, 3] length (along the heading), width, height: the layout of cld_collision */
    const int32_t* scene_start;     /* DEVICE [num_scenes + 1] */
    const float*   maps;            /* DEVICE [num_maps, n_sem, map_h, map_w] or NULL */
    const int32_t* scene_map;       /* DEVICE [num_scenes], < 0: no map */
    const float*   map_from_world;  /* DEVICE [num_maps, 3, 3] */
    double  sim_dt, stat_dt;
    int32_t num_scenes, B_all, n_sem, height, width, num_maps, map_h, map_w, drivable_layer;
    float   px_per_m, ego_center[2], no_map_fill;
} cld_scene_metrics;

size_t cld_scene_metrics_state_bytes(int32_t B_all);
int cld_scene_metrics_step(cld_handle h, const cld_scene_metrics* m, const float* world, void* state,
                           uint8_t* flags /*[B_all,4] or NULL*/, int32_t* partner /*[B_all] or NULL*/, int32_t step, void* stream);
int cld_scene_metrics_read(cld_handle h, const cld_scene_metrics* m, const void* state,
                           float* per_agent /*[B_all, CLD_METRICS_AGENT_COLS] or NULL*/,
                           float* per_scene /*[num_scenes, CLD_METRICS_SCENE_COLS] or NULL*/, void* stream);

/* The guidance satisfaction metrics of a closed-loop rollout, kept on the device: what upstream's guidance_metrics_from_config /
 * constraint_metrics_from_config register, one to three GuidanceMetric objects per entry of the guidance config
 * (src/tbsim/utils/guidance_metrics.py), fed once per 0.1 s environment step.  Needs no weights; one launch per step, no atomics (two runs
 * give the same bytes), no synchronisation.  All pointers are DEVICE.
 *
 * The entry table (built once by the caller; E = num_entries, one ENTRY per registered metric object):
 *   entry_kind [E]      CLD_GM_* below;  entry_scene [E] the scene the entry scores;
 *   member_start [E+1]  into members [num_members]: the batch rows the entry scores (the config's `agents`, or the whole scene), in the
 *                       config's order; a MEMBER is one (entry, row) slot, k = its index within the entry, n = the entry's member count;
 *   excl_start [E+1]    into excluded [num_excluded]: the entry's excluded batch rows, SORTED ASCENDING within the entry (binary search);
 *                       excluded may be NULL when num_excluded = 0;
 *   param_start [E+1]   into params [num_params] (double); per kind:
 *                         TARGET_SPEED  L, then ts[n, L] member-major (L = the row length);   SPEED_LIMIT, ACC_LIMIT  the limit;
 *                         SOCIAL_DIST  buffer_dist;   SOCIAL_GROUP  social_dist;   the two TARGET_POS kinds  pos[n, 2];
 *                         the two AT_TIME kinds  pos[n, 2], then target_time[n];   the other kinds none.
 *                       A parameter read past its entry's range is NaN; params may be NULL when num_params = 0.
 * Table CONTENTS are never validated (device memory): every index read from it is clamped into its array, so a malformed table cannot
 * make the kernels read or write out of bounds, but its metrics are then meaningless.
 *
 * cld_guide_metrics_step is one environment step: world [B_all,3] (x, y, h), speed [B_all], acc [B_all] (the executed state's speed and
 * acceleration columns), global_t = the index of this step in the episode.  `state` is cld_guide_metrics_state_bytes(E, num_members)
 * bytes, 16-byte aligned, all-zero = empty, updated in place, opaque.  Member row i is ABSENT at a step when its x or y is NaN.
 * Flags are decided in fp32 with the arithmetic of cld_scene_metrics_step (disk test, separating-axis test, partner rule, map pixel
 * lookup, the 52 disk samples): without exclusions and with whole-scene members, the disk and box flags equal coll_disk / coll_any /
 * off_road_disk of cld_scene_metrics_step bit for bit.  Distances, differences and sums are fp64 from the fp32 inputs, every operation
 * rounded on its own (no fused multiply-add); reductions run in a fixed order.  Per step and member:
 *   TARGET_SPEED (TargetSpeedGuidance)  |speed - ts[k, global_t]|, 0 once global_t >= L; the step value is the nanmean over members;
 *   SPEED_LIMIT, ACC_LIMIT (SpeedLimitGuidance, AccLimitGuidance)  max(speed - limit, 0), max(|acc| - limit, 0), a NaN kept (np.clip);
 *                 the step value is the mean over members (NaN if any is).  Episode value of the three: the mean of the step values.
 *   AGENT_COLLISION (AgentCollisionGuidance)  1 when the member's box overlaps a valid j != i of the scene, UNLESS the member and the
 *                 lowest-index such j are both excluded.  Absent: 0.  Episode: mean over members of the max over steps.
 *   AGENT_COLLISION_DISK, SOCIAL_DIST (AgentCollisionGuidanceDisk, SocialDistanceGuidance)  1 when some valid, not excluded j != i of
 *                 the scene has |p_i - p_j| < r_i + r_j (SOCIAL_DIST: (r_i + r_j) + buffer_dist, the buffer rounded to fp32);
 *                 an excluded or absent member records 0.  Episode: the same.
 *   MAP_COLLISION (MapCollisionGuidance -> Metrics.batch_detect_off_road_boxes)  the four corners (ox -+ ppm e0 / 2, oy -+ ppm e1 / 2) in
 *                 get_box_world_coords' order (-,-) (-,+) (+,+) (+,-) on the raster of an agent standing at this step's pose (yaw 0 in its
 *                 own raster), each clamped to the raster, rounded half to even, clamped again; 1 if drv(i; u, v) = 0 at any of them.
 *   MAP_COLLISION_DISK (MapCollisionGuidanceDisk)  off_road_disk of cld_scene_metrics_step.
 *                 Episode value of the two: mean over members of (flags summed over steps / steps).  An absent member records 0 and
 *                 stays in the denominator: PARITY UNPINNED, upstream casts a NaN pixel index there.
 *   GLOBAL_TARGET_POS (GlobalTargetPosGuidance)  d = |p - pos[k]|; the member keeps min d under a strict <, so a NaN never wins.
 *   TARGET_POS (TargetPosGuidance)  the same on p taken through agent_from_world of the member's pose at the state's FIRST step:
 *                 with c = cos h0, s = sin h0 in double, rows (c, s, -(c x0) - (s y0)) and (-s, c, (s x0) - (c y0)), applied as
 *                 (x m0 + y m1) + m2.  Episode value of the two: mean over members of the minimum (inf while none was taken).
 *   GLOBAL_TARGET_POS_AT_TIME, TARGET_POS_AT_TIME (GlobalConstraintGuidance, ConstraintGuidance; also the `constraint` entries)
 *                 at the step with global_t = target_time[k] + 1 (the first scored step is the initial state) the distance to pos[k]
 *                 (world / first-step frame) is captured.  Episode: mean over members; NaN when a member's step never came or it was
 *                 absent then (upstream raises an IndexError for a time beyond the episode).
 *   SOCIAL_GROUP (SocialGroupGuidance)  |min over the entry's other members of |p_i - p_j| - social_dist|; a NaN distance makes the minimum
 *                 NaN, an entry of one member gives inf.  Episode: mean over members of the mean over steps.
 * cld_guide_metrics_read finalises (either output may be NULL): per_member [num_members] the member's episode value (for the per-step-mean
 * kinds the mean of its own terms), per_entry [E] the episode value.  The mean over members is taken in numpy's add.reduce order (its
 * pairwise sum: halves down to blocks of at most 128, eight accumulators per block), so a mean of step fractions is np.mean's bits.  An empty state reads NaN (inf for the
 * two TARGET_POS kinds), an unknown kind NaN.
 * DIFFERENCES from upstream, deliberate: (1) AgentCollisionGuidance compares coll[1], an index into the OTHER-agents array, with
 * excluded_agents: off by one for partners above the agent; here the partner is its row.  (2) The map kinds read the raster of the agent
 * at the step's pose, as cld_scene_metrics does; upstream reads the observation raster, which may be stale.  (3) Box overlap is this
 * library's separating-axis test; upstream decides with shapely: PARITY UNPINNED as for cld_scene_metrics.  (4) ACC_LIMIT reads the executed
 * state's acceleration; upstream reads trajdata's agent_hist[..., 4] / agent_hist[..., 7].
 * CLD_ERR_ARG: NULL m / world / speed / acc / state / extent / scene_start / entry arrays, num_entries or num_members < 1, num_members or
 * B_all beyond CLD_RASTER_MAX_AGENTS, num_excluded or num_params < 0 or > 0 without their array, the raster and map checks of
 * cld_scene_metrics_step, global_t < 0, read without an output. */
#define CLD_GM_TARGET_SPEED 0
#define CLD_GM_SPEED_LIMIT 1
#define CLD_GM_ACC_LIMIT 2
#define CLD_GM_AGENT_COLLISION 3
#define CLD_GM_AGENT_COLLISION_DISK 4
#define CLD_GM_SOCIAL_DIST 5
#define CLD_GM_MAP_COLLISION 6
#define CLD_GM_MAP_COLLISION_DISK 7
#define CLD_GM_TARGET_POS 8
#define CLD_GM_GLOBAL_TARGET_POS 9
#define CLD_GM_TARGET_POS_AT_TIME 10
#define CLD_GM_GLOBAL_TARGET_POS_AT_TIME 11
#define CLD_GM_SOCIAL_GROUP 12
typedef struct cld_guide_metrics {
    const float*   extent;          /* DEVICE [B_all, 3] */
    const int32_t* scene_start;     /* DEVICE [num_scenes + 1] */
    const float*   maps;            /* DEVICE [num_maps, n_sem, map_h, map_w] or NULL */
    const int32_t* scene_map;       /* DEVICE [num_scenes], < 0: no map */
    const float*   map_from_world;  /* DEVICE [num_maps, 3, 3] */
    const int32_t* entry_kind;      /* DEVICE [num_entries] */
    const int32_t* entry_scene;     /* DEVICE [num_entries] */
    const int32_t* member_start;    /* DEVICE [num_entries + 1] */
    const int32_t* members;         /* DEVICE [num_members] */
    const int32_t* excl_start;      /* DEVICE [num_entries + 1] */
    const int32_t* excluded;        /* DEVICE [num_excluded] or NULL */
    const int32_t* param_start;     /* DEVICE [num_entries + 1] */
    const double*  params;          /* DEVICE [num_params] or NULL */
    int32_t num_entries, num_members, num_excluded, num_params;
    int32_t num_scenes, B_all, n_sem, height, width, num_maps, map_h, map_w, drivable_layer;
    float   px_per_m, ego_center[2], no_map_fill;
} cld_guide_metrics;

size_t cld_guide_metrics_state_bytes(int32_t num_entries, int32_t num_members);
int cld_guide_metrics_step(cld_handle h, const cld_guide_metrics* m, const float* world /*[B_all,3]*/, const float* speed /*[B_all]*/,
                           const float* acc /*[B_all]*/, void* state, int32_t global_t, void* stream);
int cld_guide_metrics_read(cld_handle h, const cld_guide_metrics* m, const void* state, double* per_entry /*[num_entries] or NULL*/,
                           double* per_member /*[num_members] or NULL*/, void* stream);

/* The occupancy metrics of a closed-loop evaluation, kept on the device: what upstream registers as all_coverage = OccupancyCoverage (grid
 * step 2 m) and all_diversity = OccupancyDiversity (grid step 4 m) (src/tbsim/evaluation/env_builders.py:35-52; the classes and their
 * OccupancyGrid: src/tbsim/envs/env_metrics.py:977-1218).  Needs no weights; plain fp64 / integers in both library precisions; none of the
 * three calls synchronises.  All pointers are DEVICE.
 *
 * The grid.  Cell (i, j) of a grid with offset (o0, o1) and step (s0, s1) is the world point g = (s0 i + o0, s1 j + o1).  Scene s owns the
 * cells of its window, i in [ix0, ix0 + nx), j in [iy0, iy0 + ny) (window[s] = ix0, iy0, nx, ny), stored row-major [nx, ny] from
 * cell_start[s] in every plane; a plane has `cells` = cell_start[num_scenes] elements.
 *
 * cld_occupancy_splat is one environment step over all B_all agents of all scenes: world [B_all,3] (x, y, h).  Agent a is VALID when
 * neither x nor y is NaN.  A valid agent at p = (x, y):
 *   centre cell   c = (rint((x - o0) / s0), rint((y - o1) / s1)) in fp64, half to even (np.round);
 *   half-width    N = ceil(sqrt(-2 sigma ln(kernel_cut)) / s0) + 1 for BOTH axes (upstream divides by the x step twice);
 *   every cell c + d, d in [-N, N]^2 -- no cut-off inside the window: 7 x 7 cells at sigma 1 / step 2, 5 x 5 at step 4, 9 x 9 at sigma 4 /
 *   step 2 -- receives k = exp(-|p - g|^2 / 2 / sigma) in fp64 (the divisor is sigma, not sigma^2, as upstream's is), added to grid[cell] as
 *   the unsigned 64-bit integer rint(k 2^40) with one ordinary vector integer atomic add.
 * grid is therefore Q40 fixed point: each add rounds by at most 2^-41, and integer adds commute, so the plane holds the same bits on every
 * run and under every permutation of agents and order of steps.  A cell of the agent's window outside the scene's window is not written;
 * it adds 1 to dropped[s] (unsigned 64-bit, one atomic add per agent).  The caller keeps the adds into one cell below 2^24 (each is at most
 * 2^40), or the sum wraps.
 *
 * cld_occupancy_mark replays the poses of one episode, world [n_steps, B_all, 3], once its failures are known: every cell of the window of
 * every valid pose of an agent with ok[a] != 0 that lies in the scene's window gets success[cell] = 1 (idempotent byte stores; other bytes
 * are left as they are).  After every episode has been marked, success[cell] = 1 exactly where upstream's per-cell set of (episode, agent)
 * pairs holds a pair that did not fail.
 *
 * cld_occupancy_read, any of the outputs (at least one; the others NULL):
 *   counts [num_scenes, 3] int64: total = #(grid > T), onroad = #(lane and grid > T), success = #(lane and success and grid > T) over the
 *                  scene's window, T = rint(threshold 2^40) compared on the integers (OccupancyCoverage.summarize_grid with v > threshold,
 *                  v lane > threshold, v lane ok > threshold; lane and ok are 0 / 1).  success == NULL counts no cell as a success.
 *   values [cells] fp64 = grid / 2^40 (exact below 2^53);  lane [cells] uint8;
 *   mass [num_scenes] uint64 = the sum of grid over the scene's on-road cells, exact: OccupancyDiversity's distribution of one episode is
 *                  values lane / (mass / 2^40).
 * lane(cell) is defined by this project: the drivable value of the map at the cell's world point g under the rule of drv in
 * cld_scene_metrics above -- g rounded to fp32, map pixel rint(map_from_world . g) of layer `drivable_layer`, value != 0; outside the map,
 * with scene_map[s] < 0 (or >= num_maps) and with maps == NULL it is no_map_fill != 0 -- evaluated by the same device function.  It is a
 * function of the cell alone and is evaluated at read time.
 *
 * Differences from upstream, on purpose:
 *   absent agents   contribute nothing.  Upstream maps NaN coordinates to cell (0, 0) and adds NaN there, which removes the cells around the
 *                   grid origin from every count.
 *   lane flag       from the map at the cell's point, not from the raster of the last agent that wrote the cell (upstream truncates the
 *                   point's raster coordinates in that agent's raster and keeps the last writer's answer).  The two agree wherever the cell
 *                   point is not within raster rounding (about 1 m at 2 px / m) of a drivable boundary.
 *   bounded window  a scene's grid is its window, with the dropped counter, not an unbounded dict.
 *   fixed point     values are Q40: a cell differs from upstream's fp64 sum by at most (adds into the cell) 2^-41 plus fp64 rounding.
 *   diversity       is evaluated by the caller from values, lane and mass (a transport problem; the Python layer solves it on the host);
 *                   fewer than two episodes or an episode without on-road mass give NaN, as upstream's arithmetic does.
 *
 * CLD_ERR_ARG (nothing is skipped silently): NULL o / world / grid / dropped / ok / success (mark) / scene_start / window / cell_start,
 * num_scenes or B_all < 1, num_scenes > B_all, cells < 1, step <= 0, sigma <= 0, kernel_cut outside (0, 1), a window of more than
 * CLD_OCCUPANCY_MAX_WINDOW_CELLS = (2 N + 1)^2 cells, non-finite offset / step / sigma, maps without their companions, drivable_layer
 * outside [0, n_sem) (n_sem >= 1 even without maps), n_steps < 1 or n_steps B_all >= 2^31 (mark), a threshold outside [0, 2^20] or no
 * output (read).  The CONTENTS of scene_start, window and cell_start are never validated by the library (device memory; the Python layer
 * checks them on the host): the caller guarantees the split of cld_scene_metrics, nx, ny >= 1 and cell_start[s + 1] = cell_start[s] + nx
 * ny from 0 to `cells`.  The kernels clamp what they read, and no index outside [0, cells) is ever touched. */
#define CLD_OCCUPANCY_MAX_WINDOW_CELLS 1024
typedef struct cld_occupancy {
    const int32_t* scene_start;     /* DEVICE [num_scenes + 1] */
    const int32_t* window;          /* DEVICE [num_scenes, 4] ix0, iy0, nx, ny */
    const int64_t* cell_start;      /* DEVICE [num_scenes + 1] flat offsets into the cell planes */
    const float*   maps;            /* DEVICE [num_maps, n_sem, map_h, map_w] or NULL */
    const int32_t* scene_map;       /* DEVICE [num_scenes], < 0: no map */
    const float*   map_from_world;  /* DEVICE [num_maps, 3, 3] */
    int64_t cells;                  /* the length of every cell plane */
    double  offset[2], step[2], sigma, kernel_cut;      /* kernel_cut: upstream's 0.1 */
    int32_t num_scenes, B_all, n_sem, num_maps, map_h, map_w, drivable_layer;
    float   no_map_fill;
} cld_occupancy;

int cld_occupancy_splat(cld_handle h, const cld_occupancy* o, const float* world /*[B_all,3]*/, uint64_t* grid /*[cells]*/,
                        uint64_t* dropped /*[num_scenes]*/, void* stream);
int cld_occupancy_mark(cld_handle h, const cld_occupancy* o, const float* world /*[n_steps,B_all,3]*/, int32_t n_steps,
                       const uint8_t* ok /*[B_all]*/, uint8_t* success /*[cells]*/, void* stream);
int cld_occupancy_read(cld_handle h, const cld_occupancy* o, const uint64_t* grid /*[cells]*/, const uint8_t* success /*[cells] or NULL*/,
                       double threshold, int64_t* counts /*[num_scenes,3] or NULL*/, double* values /*[cells] or NULL*/,
                       uint8_t* lane /*[cells] or NULL*/, uint64_t* mass /*[num_scenes] or NULL*/, void* stream);

/* The realism deviation of the test stage (src/trainers/guide_dm_trainer.py:204-295): the mean of three Wasserstein-1 distances between
 * ground-truth and predicted samples of the longitudinal acceleration, the lateral acceleration and the jerk.  Three primitives; none
 * needs weights, none depends on the handle's precision mode (plain fp32 / fp64 in both), none synchronises.  All pointers are DEVICE.
 *
 * cld_realism_terms: sa [M, T, 6] fp32 (x, y, vel, yaw, acc, yawvel; scaled, as test_step compares them) ->
 *   lon [M T]        = sa[m, t, 4]                                           (a copy)
 *   lat [M T]        = sa[m, t, 2] * sa[m, t, 5]                             (one fp32 product)
 *   jerk [M (T - 1)] = (sa[m, t + 1, 4] - sa[m, t, 4]) / dt, t < T - 1       (one fp32 difference, one correctly rounded fp32 division by
 *                                                                             dt; no reciprocal, no contraction)
 * each flattened row-major, written at the given destinations (an accumulator hands its buffers' tails).  Any of the three may be
 * NULL and is then not written; all three NULL is CLD_ERR_ARG.  Needs M >= 1, T >= 2, M T <= 2^30, 0 < dt < inf (else CLD_ERR_ARG).
 *
 * cld_sort_f32: out [n] = the n values of `in` ascending, key only, in numpy's order: -inf first, +inf before NaN, every NaN of
 * either sign last; -0.0 sorts before +0.0 (np.sort leaves equal keys in either order); denormals are ordered by value, not flushed.
 * Values are moved as bits, except that every NaN comes out as the quiet NaN 0x7fffffff.  The output is a function of the input values
 * alone: a stable LSD radix sort over the monotone integer image of the key, no atomics on global memory.  out == in is allowed;
 * any other overlap of the two, or of either with the workspace, is not.  1 <= n <= 2^30 (else CLD_ERR_ARG);
 * workspace >= cld_sort_workspace_bytes(n) bytes, 16-byte aligned (a second copy of the keys plus 1 KiB of digit counts per
 * cld_debug_sort_items_per_block() keys; 0 for an n out of range), else CLD_ERR_WORKSPACE.
 *
 * cld_wasserstein_f32: *out (fp64, 8-byte aligned) = the 1-D Wasserstein-1 distance of the empirical distributions of u_sorted [nu] and
 * v_sorted [nv], both ascending in cld_sort_f32's (or np.sort's) order: scipy.stats.wasserstein_distance without weights.
 *   nu == nv = n: (1 / n) sum_i |u_i - v_i|.
 *   nu != nv:     with a_0 <= ... <= a_{N-1} the merged values, N = nu + nv, cu_k and cv_k the numbers of values of u and v that are <= a_k,
 *                 (1 / (nu nv)) sum_k |cu_k nv - cv_k nu| (a_{k+1} - a_k) over the k with a_{k+1} != a_k.  A run of equal values -- inside
 *                 one sample or across both, -0 and +0 included -- contributes only at its last element, where the counts are the
 *                 inclusive ones: the right-continuous CDFs scipy evaluates.  The counts are integers (exact below 2^60).
 * Every difference and sum is fp64.  Each workgroup leaves one partial in the workspace, summed in a fixed order, and one workgroup folds the
 * partials in a fixed order and divides once: the result is bit-identical from run to run.  With every term non-negative its relative
 * error is within (nu + nv) 2^-53 of the exact sum of the rounded terms.  A NaN in either sample, or an inf - inf between neighbours,
 * gives NaN, as numpy's arithmetic does; that is not an error.  1 <= nu, nv <= 2^30 (else CLD_ERR_ARG);
 * workspace >= cld_wasserstein_workspace_bytes(nu, nv) bytes, 8-byte aligned (0 for sizes out of range), else CLD_ERR_WORKSPACE.
 * Unsorted input is not detected: the result is then meaningless (memory stays in bounds).
 *
 * NULL sa / in / out / u_sorted / v_sorted: CLD_ERR_ARG.  Nothing is skipped silently.
 * cld_debug_sort_items_per_block: the keys one workgroup of the sort ranks (no handle, no device call; tests straddle it). */
size_t cld_sort_workspace_bytes(int64_t n);
int cld_sort_f32(cld_handle h, const float* in, float* out, int64_t n, void* workspace, size_t workspace_bytes, void* stream);
size_t cld_wasserstein_workspace_bytes(int64_t nu, int64_t nv);
int cld_wasserstein_f32(cld_handle h, const float* u_sorted, int64_t nu, const float* v_sorted, int64_t nv, double* out,
                        void* workspace, size_t workspace_bytes, void* stream);
int cld_realism_terms(cld_handle h, const float* sa /*[M,T,6]*/, int64_t M, int32_t T, float dt, float* lon /*[M T] or NULL*/,
                      float* lat /*[M T] or NULL*/, float* jerk /*[M (T-1)] or NULL*/, void* stream);
int32_t cld_debug_sort_items_per_block(void);

/* Which form a Conv1d(k5) + GroupNorm + Mish launch takes (no handle, no device call; tests): CLD_FORM_WINOGRAD or CLD_FORM_DIRECT for a
 * layer with `c1` (+ `c2` concatenated) input channels, `c_out` output channels and `l_in` rows per agent in a launch set of `rows` agents
 * (padded to 16 inside), with `forced_form` = what cld_debug_force_kernel(CLD_KERNEL_CONV5, ...) would hold (CLD_FORM_AUTO: by size).
 * The Winograd kernels address their tensors with 32-bit byte offsets: a launch whose widest tensor reaches 2 GiB falls back to the
 * direct form whatever is forced.  Layers without a Winograd instance always answer CLD_FORM_DIRECT.  < 0: bad argument. */
int cld_debug_conv5_form(int32_t l_in, int32_t c1, int32_t c2, int32_t c_out, int64_t rows, int32_t forced_form);

/* The items a Winograd F(4, 5) launch of a k5 layer at `l_in` = 13 / 26 rows with `c_out` = 64 / 128 / 256 output channels runs in a launch
 * set of `rows` agents (padded to 16 inside), with `forced_form` as for cld_debug_conv5_form (no handle, no device call; tests): 0 half
 * items (wino1d_kernels.hip), 1 whole items (wino1d_edge.hip), 2 whole items of eight waves.  Whether the launch takes Winograd at all is
 * cld_debug_conv5_form's answer.  < 0: bad argument. */
int cld_debug_conv5_items(int32_t l_in, int32_t c_out, int64_t rows, int32_t forced_form);

/* Tests only: where the 1x1 residual projection of the blocks downs.1.0, downs.2.0 and ups.0.0 (spans 1, 4, 8) is evaluated on this handle.
 * Their second Conv1d(k5) + GroupNorm + Mish launch evaluates it itself, behind its Mish, wherever that launch runs four-wave whole
 * Winograd items (cld_debug_conv5_items == 1; exact-fp32 handles; every tensor below the kernel's 2 GiB of 32-bit byte offsets):
 * CLD_RES_FOLD_FUSED, the default, every such launch; CLD_RES_FOLD_SEPARATE none -- the projection is then a launch of its own next to
 * the block's first conv, as it is in every other form.  With cld_debug_force_kernel(CLD_KERNEL_CONV5, CLD_FORM_WINOGRAD_WHOLE) both forms
 * exist at every batch size. */
#define CLD_RES_FOLD_FUSED 0
#define CLD_RES_FOLD_SEPARATE 1
int cld_debug_res_fold(cld_handle h, int32_t mode);

/* The weights W [c_out][c_in] (HOST) of such a projection in the order the fused launch reads them (no handle, no device call; tests): per 16
 * input channels one plane [c_out / 16][64 lanes][4] = W[16 nt + (lane & 15)][16 chunk + 4 (lane >> 4) + s], and behind the last one plane of
 * zeros, which the kernel's one-chunk look-ahead lands on.  Returns the number of floats -- the bound the kernel gives its buffer resource
 * -- and fills out[0 .. n) (HOST, `capacity` floats); with w and out NULL only the size.  < 0: bad argument. */
int64_t cld_debug_pack_res_proj(const float* w, int32_t c_out, int32_t c_in, float* out, int64_t capacity);

/* One of the 12 spans a U-Net evaluation is run as (tests): the same launches cld_unet_forward makes for that span, in the form
 * cld_debug_force_kernel(CLD_KERNEL_UNET / CLD_KERNEL_CONV5, ...) holds.  Spans (input -> output per agent, [L, C] row-major):
 *   0 downs.0.* [52,4] -> [26,64]; 1 downs.1.0 -> [26,128]; 2 downs.1.1 -> [26,128]; 3 downs.1.2 -> [13,128]; 4 downs.2.0 -> [13,256];
 *   5 downs.2.1, 6 mid_block1, 7 mid_block2 -> [13,256]; 8 ups.0.0 cat(x1, x2 [13,256]) -> [13,128]; 9 ups.0.1 -> [13,128];
 *   10 ups.0.2 -> [26,128]; 11 ups.1.*, final_conv.* cat(x1, x2 [26,128]) -> eps [52,4].
 * x1 / x2 / y are DEVICE fp32 [B, L, C]; x2 (the skip) is given for spans 8 and 11 only.  The timestep is t_idx for every row, or
 * t_rows [B] (DEVICE int32) per row when non-null.  cond [B,256] gives the cond half of the blocks' bias as in cld_unet_forward.  The
 * entry packs x1 / x2 into the workspace's activation buffers (split fp16 hi / lo planes on CLD_PRECISION_F16X2 handles) and unpacks y. */
int cld_debug_unet_span(cld_handle h, int32_t span, const float* x1, const float* x2, const float* cond, int32_t t_idx,
                        const int32_t* t_rows, float* y, int32_t B, void* workspace, size_t workspace_bytes, void* stream);

/* Measurement aid for bench.py (no reference counterpart): while enabled, every launch of the
 * dominant kernel instance -- the Conv1d(k=5) + GroupNorm + Mish block producing 256 channels at
 * L = 13 (conv_block_kernel<13,13,1,5,32,*,*,1,32,1,0,0,0>: 7 launches per U-Net evaluation, all with 256 input
 * channels -- the 128 -> 256 block opens with a pair launch of its own kernel; temporal.py:16-45) -- in every 10th U-Net
 * evaluation is bracketed by HIP events on the
 * caller's stream (a sample: an event pair costs ~2 us of stream time, so timing all of them would slow the region measured).
 * cld_profile_read waits for the recorded events and returns the summed kernel time, the
 * number of launches and their algorithmic FLOP (2 * rows * K * N); enable(…, 1) resets. */
int cld_profile_enable(cld_handle h, int32_t on);
int cld_profile_read(cld_handle h, double* total_ms /*HOST*/, int64_t* launches /*HOST*/, double* total_flop /*HOST*/);
/* What the MFMA pipe executed, counted by the library for the form each launch actually took (no reference counterpart):
 * `timed_executed_flop` = FLOP issued by the MFMAs of the launches cld_profile_read timed (the Winograd F(4, 5) form of a k5 layer
 * runs 8 transform-domain GEMMs over 4 tiles per agent instead of 5 taps over 13 rows: 2.03x fewer than total_flop counts);
 * `eval_*` = the algorithmic FLOP, the executed MFMA FLOP and the number of kernel launches of the handle's most recent U-Net
 * evaluation (all of its launches, layer chains included).  bench.py's roofline.frac is executed FLOP / time / peak. */
int cld_profile_read_executed(cld_handle h, double* timed_executed_flop /*HOST*/, double* eval_algorithmic_flop /*HOST*/,
                              double* eval_executed_flop /*HOST*/, int32_t* eval_launches /*HOST*/);

/* Diagnostic builds only (-DCLD_STAMPS; a no-op in the shipped library): conv launch number `layer`
 * (0..36) of every following U-Net evaluation writes 16 u64 cycle stamps per workgroup into `buf`. */
int cld_debug_stamps(cld_handle h, void* buf /*DEVICE, u64[16 * workgroups]*/, int32_t layer);

/* Diagnostic builds only (-DCLD_STAMPS; leaves `out` untouched in the shipped library): shader-clock stamps of the phases of
 * the last guidance-kernel launch, 8 u64 per workgroup for workgroups 0..255 (scripts/guide_stamps.py). */
int cld_debug_guide_stamps(void* out /*HOST, u64[2048]*/);

/* Experiments only: every conv launch of this handle asks for at least `bytes` of dynamic LDS (0 = off), which steers how many
 * workgroups of which stream can share a CU when two handles run on two streams (scripts/exp_streams.py). */
int cld_debug_lds_floor(cld_handle h, size_t bytes);

/* Tests only: force the formulation of one of the three recurrent kernels (or of the U-Net's layer chains) of this handle instead of letting the batch size
 * pick it (all forms compute the same function; the parity tests run each against the oracle).  The shipped library reads
 * no environment variable: every behaviour switch is an explicit call like this one. */
#define CLD_KERNEL_GUIDE 0    /* guidance: LSTM forward + BPTT + roll-out backward (cld_sample_guided, cld_guidance_step) */
#define CLD_KERNEL_DECODE 1   /* cld_lstm_decode, cld_decode */
#define CLD_KERNEL_ENCODE 2   /* cld_traj2z */
#define CLD_KERNEL_UNET 3     /* the 64-channel levels of a U-Net evaluation: CLD_FORM_AUTO by batch size, CLD_FORM_LAYERS one launch
                               * per layer (conv_block.hip), CLD_FORM_CHAIN the LDS-resident layer chains (conv_chain.hip) */
#define CLD_KERNEL_CONTEXT 4  /* the 3x3 / stride-1 convolutions of the ContextEncoder: CLD_FORM_AUTO / CLD_FORM_WINOGRAD Winograd F(4x4, 3x3)
                               * at all four map sizes (wino44_kernels.hip), CLD_FORM_DIRECT the implicit-GEMM kernel the other convolutions
                               * use (and the stem with a separate max-pool launch) */
#define CLD_KERNEL_CONV5 5    /* the Conv1d(k5) + GroupNorm + Mish launches of the L = 13 / 26 levels of a U-Net evaluation (exact-fp32 handles): CLD_FORM_AUTO
                               * by batch size, CLD_FORM_DIRECT conv_block.hip, CLD_FORM_WINOGRAD Winograd F(4, 5) (wino1d_edge.hip / wino1d_kernels.hip by launch size),
                               * CLD_FORM_WINOGRAD_WHOLE wino1d_edge.hip at every size */
#define CLD_FORM_AUTO 0       /* by batch size (default) */
#define CLD_FORM_VALU 1       /* one or two agents per workgroup, gate rows in registers */
#define CLD_FORM_MFMA 2       /* 16 agents per workgroup, gate products as fp32 16x16x4 MFMA tiles */
#define CLD_FORM_MFMA_QUAD 3  /* guide only: 8 agents per workgroup on the 16-block 4x4x1 fp32 MFMA (the form 2,048 agents run in) */
#define CLD_FORM_LAYERS 1     /* CLD_KERNEL_UNET only */
#define CLD_FORM_CHAIN 2      /* CLD_KERNEL_UNET only: chains, form and tile by batch size (= CLD_FORM_AUTO for exact-fp32 handles) */
#define CLD_FORM_CHAIN_TILE1 3   /* CLD_KERNEL_UNET only: chains with one-agent tiles  */
#define CLD_FORM_CHAIN_TILE4 4   /* CLD_KERNEL_UNET only: chains with four-agent tiles, every layer in the direct form (conv_chain.hip) */
#define CLD_FORM_CHAIN_WINO 5    /* CLD_KERNEL_UNET only: chains with four-agent tiles, their 64 -> 64 k5 layers in Winograd F(4, 5) form
                                  * (chain_wino.hip) */
#define CLD_FORM_CHAIN_WINO2 6   /* CLD_KERNEL_UNET only: the Winograd chains with two-agent tiles (three workgroups per CU): what CLD_FORM_AUTO /
                                  * CLD_FORM_CHAIN take above 944 rows per launch set */
#define CLD_FORM_CHAIN_WINO1 7   /* CLD_KERNEL_UNET only: the Winograd chains with one-agent tiles: CLD_FORM_AUTO / CLD_FORM_CHAIN up to 944 rows */
#define CLD_FORM_DIRECT 1     /* CLD_KERNEL_CONTEXT, CLD_KERNEL_CONV5 */
#define CLD_FORM_WINOGRAD 2   /* CLD_KERNEL_CONTEXT, CLD_KERNEL_CONV5 */
#define CLD_FORM_WINOGRAD_KSPLIT 4  /* CLD_KERNEL_CONV5 only: whole items run by eight waves (the two halves of the input channels on four waves each) at every
                                     * launch size: what CLD_FORM_WINOGRAD takes by itself for launches of about one whole item per CU */
#define CLD_FORM_WINOGRAD_WHOLE 3   /* CLD_KERNEL_CONV5 only: Winograd with whole items at every launch size (wino1d_edge.hip: what CLD_FORM_WINOGRAD takes
                                     * by itself once a launch fills two workgroups per CU; below that it runs half items, wino1d_kernels.hip) */
int cld_debug_force_kernel(cld_handle h, int32_t which, int32_t form);

/* Tests only: one layer of the ContextEncoder's ResNet-18 on n agents (1 <= n <= 256, one pass of cld_context_encode), through the same
 * dispatch cld_context_encode uses, in the form cld_debug_force_kernel(CLD_KERNEL_CONTEXT, ...) holds: CLD_FORM_DIRECT the stem and a
 * separate max-pool launch and the implicit GEMM for every convolution; CLD_FORM_AUTO / CLD_FORM_WINOGRAD the stem with the fused max-pool
 * and F(4x4, 3x3) for the thirteen stride-1 3x3 layers.  `layer`:
 *   0       the stem: x = image [n,34,224,224] NCHW -> y = maxpool(relu(bn(conv7x7/2 x))) [n,56,56,64] NHWC (residual NULL, relu 1)
 *   1..16   rn_conv[li][b][c] in forward order (layer = 1 + 4 li + 2 b + c: layer{li+1}.{b}.conv{c+1} + bn{c+1})
 *   17..19  the 1x1/2 downsample convolutions + BatchNorm of layer2 / layer3 / layer4
 * x, residual (NULL: none) and y are DEVICE NHWC tensors of the layer's input / output shape, 16-byte aligned, y = [relu](bn(conv x) + residual).
 * Synchronous for the direct stem (it allocates its [n,112,112,64] scratch). */
int cld_debug_context_layer(cld_handle h, int32_t layer, const float* x, const float* residual, float* y, int32_t n, int32_t relu,
                            void* stream);
/* Agents per pass cld_context_encode takes for B agents in its Winograd form (no handle, no device call; tests): B for B <= 256, else a pass
 * size in [128, 256] -- passes of that size and a last one of the rest.  The direct form runs passes of 256.  < 0: bad argument. */
int cld_debug_context_pass_size(int32_t B);

/* ---- Training (exact fp32).  The reference optimises self.dm.parameters() with Adam in two loops: dm_trainer.py:72-80
 * (loss = self.dm.compute_losses(aux_info, z0), dm_model.py:82-89, then backward) and guide_dm_trainer.py:127-183 (ppo_update:
 * self.dm.log_prob(x1, x0, ...) at t = 0, manual_backward(loss), opt.step()).  These calls give the U-Net's half of both: a forward
 * from weights held in a DEVICE buffer (so an optimiser step needs no host round trip and no cld_finalize) that keeps a tape, and its
 * backward.  The optimiser stays the caller's.  A CLD_PRECISION_F16X2 handle, or one without finalized U-Net weights, refuses the
 * compute calls with CLD_ERR_STATE; the table and size queries need no handle (h may be NULL).
 *
 * Parameter table: the 148 U-Net tensors of the reference state_dict (temporal.py:48-120), in its order, each at an offset (in floats)
 * into one flat fp32 buffer, offsets multiples of 64 floats; the floats between tensors are never read or written.  Layouts as in the
 * reference: Conv1d [C_out,C_in,k], ConvTranspose1d [C_in,C_out,k], Linear [out,in].  `shape` gets 3 entries (1 past ndim). */
int cld_unet_param_count(cld_handle h);                  /* 148 */
int cld_unet_param_info(cld_handle h, int32_t i, const char** name, size_t* offset, size_t* numel, int32_t* shape, int32_t* ndim);
size_t cld_unet_param_floats(cld_handle h);              /* length of the flat buffer (> 4,349,284 values: alignment) */
/* Tape and workspace bytes of the two calls below for B rows (the workspace covers both). */
size_t cld_unet_tape_bytes(cld_handle h, int32_t B);
size_t cld_unet_train_workspace_bytes(cld_handle h, int32_t B);

/* eps = TemporalMapUnet.forward(x, {'cond_feat': cond}, t) (temporal.py:122-180) from the weights in `params` (DEVICE, the flat layout
 * above), one timestep per row (t_idx [B] DEVICE int32, dm_model.py:84).  x, eps [B,52,4], cond [B,256].  Writes the tape (DEVICE,
 * caller-owned, >= cld_unet_tape_bytes): the time MLP's activations, tc = [time_mlp(t) | cond], Mish(tc), and per residual block the
 * pre-GroupNorm convolution outputs, the per-(row, group) mean / rstd, the first block's output and the block output, the skip
 * concatenations and the up / down sampled tensors.  Not bit-identical to cld_unet_forward_t (a direct form with its own summation
 * order, no Winograd): within the forward parity bar of it. */
int cld_unet_train_forward(cld_handle h, const float* params, const float* x, const float* cond, const int32_t* t_idx, float* eps,
                           float* tape, size_t tape_bytes, int32_t B, void* workspace, size_t workspace_bytes, void* stream);

/* The backward of cld_unet_train_forward for the cotangent d_eps [B,52,4] (the autograd step of dm_trainer.py:72-80 and
 * guide_dm_trainer.py:127-183 through the U-Net).  Same params / x / tape as the forward (cond and t_idx are on the tape; they are
 * accepted for symmetry).  Any of d_params (flat layout), dx [B,52,4], dcond [B,256] may be NULL.  d_params gets the gradient of all
 * 148 tensors: accumulate = 0 overwrites them, 1 adds to them.  dx and dcond are always overwritten.  Weight gradients are split over
 * row chunks and summed in a fixed order: the result is bit-identical run to run, and each row's dx / dcond does not depend on the
 * other rows of the batch. */
int cld_unet_backward(cld_handle h, const float* params, const float* x, const float* cond, const int32_t* t_idx, const float* tape,
                      size_t tape_bytes, const float* d_eps, float* d_params, float* dx, float* dcond, int32_t accumulate, int32_t B,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- LSTM-VAE training (exact fp32): the reference's `vae` stage (train.py:10-20; src/trainers/vae_trainer.py: Adam over
 * self.vae.parameters() on VaeModel.compute_vae_loss, vae_model.py:65-99).  The encoder's and the decoder's forward from weights held in a
 * DEVICE buffer, each keeping a tape, and their backward: data gradients and the weight gradients of all 26 LSTMVAE tensors.  The
 * reparametrisation z = mu + noise exp(0.5 logvar), the loss and the optimiser stay the caller's.  The calls read no weights from the
 * handle (one without any weights trains); a CLD_PRECISION_F16X2 handle refuses them with CLD_ERR_STATE.  The table and size queries
 * need no handle (h may be NULL).
 *
 * Parameter table: the 26 tensors of LSTMVAE's state_dict (lstm_vae.py:54-80) in its order -- lstm_enc.lstm.{weight_ih, weight_hh,
 * bias_ih, bias_hh}_l{0,1}, lstm_enc.cond2hidden.*, the same 8 under lstm_dec.lstm.*, lstm_dec.cond2hidden.*, lstm_dec.hid2act.*, mu.*,
 * logvar.* (136,458 values) -- each at an offset (in floats, a multiple of 64) into one flat fp32 buffer, in the reference layouts
 * (weight_ih [256, in] and weight_hh [256, 64] with gate rows i, f, g, o; Linear [out, in]).  `shape` gets 3 entries (1 past ndim).
 *
 * Dropout: in training mode nn.LSTM(num_layers = 2, dropout = 0.2) drops layer 0's output where it enters layer 1, scaled by 1 / (1 - p);
 * the recurrence and the top layer's output are not dropped.  `drop_mask` [B,52,64] (DEVICE, or NULL = eval mode) holds that factor per
 * element (0 or 1 / (1 - p)); it is multiplied into layer 0's h on that path only.  The backward takes the same mask. */
#define CLD_VAE_ENCODER 0
#define CLD_VAE_DECODER 1
int cld_vae_param_count(cld_handle h);                   /* 26 */
int cld_vae_param_info(cld_handle h, int32_t i, const char** name, size_t* offset, size_t* numel, int32_t* shape, int32_t* ndim);
size_t cld_vae_param_floats(cld_handle h);               /* length of the flat buffer (> 136,458 values: alignment) */
/* Tape bytes of the encoder's (part CLD_VAE_ENCODER) or the decoder's (CLD_VAE_DECODER) forward for B rows: per step and layer the
 * activated gates and c, h of both layers from h0 on, and layer 1's masked input (173,568 bytes per row for either part; 0 for another
 * part or B < 1).  Workspace bytes of either backward. */
size_t cld_vae_tape_bytes(cld_handle h, int32_t part, int32_t B);
size_t cld_vae_train_workspace_bytes(cld_handle h, int32_t B);

/* (mu, logvar) [B,52,4] = the encoder and its heads (lstm_vae.py:6-26, 87-93) on x6 [B,52,6] (scaled state and action) and cond [B,256],
 * with the weights of `params` (DEVICE, the flat layout above).  Writes the tape (DEVICE, caller-owned, 16-byte aligned, >=
 * cld_vae_tape_bytes(h, CLD_VAE_ENCODER, B)).  Without a mask it agrees with cld_traj2z within the encoder's parity bar (not bit for bit:
 * libm sigmoid / tanh, a separate head sum). */
int cld_vae_encode_train(cld_handle h, const float* params, const float* x6, const float* cond, const float* drop_mask, float* mu,
                         float* logvar, float* tape, size_t tape_bytes, int32_t B, void* stream);
/* The backward of cld_vae_encode_train for the cotangents d_mu, d_logvar [B,52,4] (either may be NULL: zero), from its tape with the same
 * params / x6 / cond / drop_mask.  d_params (flat layout) gets the gradients of the encoder's 14 tensors (lstm_enc.*, mu.*, logvar.*; the
 * others are not touched): accumulate = 0 overwrites them, 1 adds to them.  b_ih and b_hh get the same gradient, sum dgates.  dx6
 * [B,52,6] and dcond [B,256] are overwritten.  Any of d_params, dx6, dcond may be NULL.  Weight gradients are summed over row chunks in a
 * fixed order (no float atomics): bit-identical run to run; a row's dx6 / dcond does not depend on the other rows. */
int cld_vae_encode_backward(cld_handle h, const float* params, const float* x6, const float* cond, const float* drop_mask,
                            const float* tape, size_t tape_bytes, const float* d_mu, const float* d_logvar, float* d_params, float* dx6,
                            float* dcond, int32_t accumulate, int32_t B, void* workspace, size_t workspace_bytes, void* stream);
/* act [B,52,2] = the decoder (lstm_vae.py:28-52) on z [B,52,4] and cond [B,256]; tape >= cld_vae_tape_bytes(h, CLD_VAE_DECODER, B).
 * Without a mask it agrees with cld_lstm_decode within the decoder's parity bar. */
int cld_vae_decode_train(cld_handle h, const float* params, const float* z, const float* cond, const float* drop_mask, float* act,
                         float* tape, size_t tape_bytes, int32_t B, void* stream);
/* The backward of cld_vae_decode_train for d_act [B,52,2]: the gradients of the decoder's 12 tensors (lstm_dec.*) into d_params, dz
 * [B,52,4], dcond [B,256]; the rules of cld_vae_encode_backward. */
int cld_vae_decode_backward(cld_handle h, const float* params, const float* z, const float* cond, const float* drop_mask,
                            const float* tape, size_t tape_bytes, const float* d_act, float* d_params, float* dz, float* dcond,
                            int32_t accumulate, int32_t B, void* workspace, size_t workspace_bytes, void* stream);

/* CLD_PRECISION_* the handle runs with. */
int cld_get_precision(cld_handle h);

/* Library build id (for the "native code loaded" check). */
const char* cld_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CLD_H */
