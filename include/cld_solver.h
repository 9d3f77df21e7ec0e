/* cld_solver.h -- few-step sampling of libcld_hip: DDIM(eta) and DPM-Solver++(2M) on a subset of the training timesteps.  A header
 * of its own beside cld.h (whose table of entry points is pinned); everything of cld.h's conventions holds: DEVICE pointers,
 * row-major, an int return (CLD_OK / CLD_ERR_*), the message behind cld_last_error, `stream` a hipStream_t or NULL.
 *
 * The reference has NO counterpart of this mode: its only shortcut is `stride` (cld_set_stride), the single-step DDPM coefficients on
 * a skipped sequence.  What pins this mode is a float64 restatement of the definitions below and two anchors: DDIM with eta = 1 on
 * the full consecutive sequence is algebraically the ancestral chain of cld_sample, and the second-order solver shows second-order
 * convergence on a problem with a closed-form solution.
 *
 * SCHEDULE.  acp_t is the handle's fp32 alphas_cumprod[t] promoted to double, acp_{-1} := 1.  A sampler is a kind, a strictly
 * decreasing list of timesteps tau_0 > tau_1 > ... > tau_{K-1} in [0, n_timesteps), K >= 1, and for DDIM an eta in [0, 1].  Step k
 * goes from s = tau_k to p = tau_{k+1}; the last step, k = K-1, goes to p = -1.  eps is the U-Net's prediction at (x, s), combined
 * as (1 + w) eps_c - w eps_u with classifier-free guidance; x0_hat = sqrt(1/acp_s) x - sqrt(1/acp_s - 1) eps.
 *
 * DDIM(eta).   var_k = eta^2 (1 - acp_p)/(1 - acp_s) (1 - acp_s/acp_p),  sigma_k = sqrt(var_k)
 *              x' = A_k x + B_k eps + sigma_k z,  A_k = sqrt(acp_p/acp_s),  B_k = sqrt(1 - acp_p - var_k) - sqrt(acp_p (1 - acp_s)/acp_s)
 *              (formed on (x, eps), so that no 2029 x - 2029 eps cancellation happens at run time at t = 99).  The last step has
 *              sigma = 0 and gives x' = x0_hat.
 * DPM-Solver++(2M)  (data prediction, multistep, deterministic, lower_order_final).
 *              lambda_t = 1/2 log(acp_t/(1 - acp_t)),  h_k = lambda_p - lambda_s
 *              D_k = x0_hat_k at k = 0 and k = K-1; otherwise r = h_{k-1}/h_k,  D_k = (1 + 1/(2r)) x0_hat_k - (1/(2r)) x0_hat_{k-1}
 *              x' = sqrt((1 - acp_p)/(1 - acp_s)) x - sqrt(acp_p) expm1(-h_k) D_k.  The last step gives x' = x0_hat.  No noise:
 *              eta != 0 is refused.
 * GUIDANCE (the mean form only: upstream's perturb() as the guided sampler runs it).  The deterministic part mu_k = x' - sigma_k z
 *              is the iterate.  Step size and clip scale are sigma^g_k = sqrt(max((1 - acp_p)/(1 - acp_s) (1 - acp_s/acp_p), 1e-20)),
 *              the DDPM posterior deviation of the jump (exp(1/2 plvc[s]) for consecutive steps; independent of eta); the noise added
 *              behind the guided step is sigma_k z.  Steps k < K-1 are "intermediate" (lr / perturb_th / optimizer / grad_steps,
 *              no_intermediate); step K-1 is the output step and follows apply_output / final_* as t = 0 does in cld_sample_guided.
 *              Plan-space terms set on the handle (goal, social group, pair, lane) and the collision / map structs work unchanged.
 *              guide_clean != 0 is refused (reconstruction guidance, cld_recon.h, and the clean-prediction form are not built here).
 * COEFFICIENTS. All per-step coefficients are formed in double on the host and rounded to fp32 once (cld_solver_tables reads them).
 * NOISE.       Slab k of a caller's [K,B,52,4] tensor feeds step k; without one the generator draws what cld_sample's iteration k
 *              draws for (seed, k, row, element).  eta = 0 and 2M draw nothing.
 * Both precision modes: the head's noise prediction (the path of cld_unet_forward) exists on CLD_PRECISION_F16X2 handles too.
 * Deterministic: one new elementwise kernel (solver_kernels.hip), no atomics; the working latent, x0_hat and mu are exact fp32
 * instruction sequences written down in csrc/solver_kernels.h. */
#ifndef CLD_SOLVER_H
#define CLD_SOLVER_H

#include "cld.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLD_SOLVER_DDIM 0
#define CLD_SOLVER_DPMPP_2M 1
#define CLD_SOLVER_TABLE_COLS 8

typedef struct cld_solver {
    int32_t kind;                 /* CLD_SOLVER_* */
    int32_t n_steps;              /* K >= 1 */
    const int32_t* timesteps;     /* HOST: K strictly decreasing timesteps in [0, n_timesteps) */
    float eta;                    /* DDIM: [0, 1]; 2M: 0 */
} cld_solver;

/* Bytes of the workspace of the two compute calls for B rows, cfg != 0 when non_cond is given: the sampler workspace
 * (cld_workspace_bytes, 2 pad16(B) rows with cfg) plus the history rows [B,52,4].  0 on a bad argument. */
size_t cld_solver_workspace_bytes(cld_handle h, int32_t B, int32_t cfg);

/* Host read-back of the fp32 per-step coefficients: table [K][CLD_SOLVER_TABLE_COLS] (HOST) receives per step
 *   0: A_k   1: B_k (DDIM) / -sqrt(acp_p) expm1(-h_k) (2M)   2: 1 + 1/(2r)   3: 1/(2r)   (2, 3: 1 and 0 on a first-order step)
 *   4: sqrt(1/acp_s)   5: sqrt(1/acp_s - 1)   6: sigma_k   7: sigma^g_k
 * On the last step the kernel writes x' = x0_hat itself; columns 0, 1 hold what the formulas give there (DDIM: col 4 and -col 5). */
int cld_solver_tables(cld_handle h, const cld_solver* solver, float* table /*HOST*/);

/* The loop: x_T [B,52,4], noise [K,B,52,4] or NULL, cond [B,256], non_cond [B,256] or NULL (classifier-free guidance with weight
 * guidance_w), guidance or NULL, x0 [B,52,4] out.  It is cld_solver_step's iteration called K times on the workspace: the two agree
 * bit for bit.  Neither allocates nor synchronises. */
int cld_sample_solver(cld_handle h, const cld_solver* solver, const float* x_T, const float* noise, const float* cond,
                      const float* non_cond, float guidance_w, const cld_guidance* guidance, float* x0, int32_t B, uint64_t seed,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Step k of `solver` on a given x_t [B,52,4], teacher-forced.  x0_prev [B,52,4] in/out (may be NULL): read by a second-order step
 * (2M, 0 < k < K-1; required there), and it receives this step's x0_hat.  z [B,52,4] or NULL (the generator keyed by (seed, k, row)).
 * Outputs [B,52,4], every one optional: x_next, x0_hat, mu (the deterministic part before guidance); mu_guided and grad = dL/dmu are
 * written on a guided step only.  Every tensor of this call and of cld_sample_solver is read and written 16 bytes at a time: a
 * pointer that is not 16-byte aligned is CLD_ERR_ARG. */
int cld_solver_step(cld_handle h, const cld_solver* solver, int32_t k, const float* x_t, float* x0_prev, const float* z,
                    const float* cond, const float* non_cond, float guidance_w, const cld_guidance* guidance, float* x_next,
                    float* x0_hat, float* mu, float* mu_guided, float* grad, int32_t B, uint64_t seed, void* workspace,
                    size_t workspace_bytes, void* stream);

/* Tests: the most workgroups a launch of the step kernel takes (it walks its rows in a grid-stride loop); cap < 1 restores the
 * default.  Returns the cap in force. */
int32_t cld_debug_solver_grid_cap(int32_t cap);

/* DEBUG ENTRY, for tests only (as cld_debug_solver_grid_cap; not part of the sampling surface): the step kernel ALONE, step k of `solver` on caller tensors [B,52,4]: x, eps_c, eps_u or NULL (with guidance_w), x0_prev (a
 * second-order step) and z or NULL (the generator keyed by (seed, k, row); read when sigma_k != 0) -> x_next, x0_hat, mu, every one
 * optional.  The U-Net picks the tiling of its launches by the padded batch size, so its noise prediction of a row differs in the
 * last bits between batch sizes; this call shows what the kernel itself does with one and the same noise prediction. */
int cld_debug_solver_kernel(cld_handle h, const cld_solver* solver, int32_t k, const float* x, const float* eps_c, const float* eps_u,
                            float guidance_w, const float* x0_prev, const float* z, float* x_next, float* x0_hat, float* mu, int32_t B,
                            uint64_t seed, void* stream);

#ifdef __cplusplus
}
#endif

#endif
