/* cld_eval.h -- open-loop sample metrics of libcld_hip: how close the N sampled futures of an agent come to the logged one (ADE / FDE)
 * and how far they lie apart (APD / FPD), where the trajectories are.  A header of its own beside cld.h (whose table of entry points
 * is pinned); everything of cld.h's conventions holds: DEVICE pointers, row-major, an int return (CLD_OK / CLD_ERR_*), the message
 * behind cld_last_error, `stream` a hipStream_t or NULL. */
#ifndef CLD_EVAL_H
#define CLD_EVAL_H

#include "cld.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Upstream validates its diffusion model with eight numbers (DiffuserTrafficModel._compute_metrics, src/tbsim/algos/algos.py:1818-1852):
 * ego_avg_ADE, ego_min_ADE, ego_avg_FDE, ego_min_FDE, ego_avg_APD, ego_max_APD, ego_avg_FPD, ego_max_FPD, from
 * batch_average_displacement_error, batch_final_displacement_error, batch_average_diversity and batch_final_diversity
 * (src/tbsim/utils/metrics.py:201-358) on numpy float32 arrays, through a [B,N,N,T,2] temporary.  Here:
 *
 * pred [B,N,T,C] fp32, 2 <= C <= 8: channels 0 and 1 are the positions (x, y), the others are not read -- C = 2 is upstream's
 * predictions["positions"], C = 6 the state-and-action tensor cld_decode writes, read in place.  gt [B,T,2] = target_positions,
 * avail [B,T] = target_availabilities as fp32 (0 / 1; any value is taken as the factor upstream multiplies by).  Confidences are
 * uniform, 1/N, as upstream passes them; nothing else is built.
 *
 *   e[b,n,t]  = sqrt(sum_c ((gt[b,t,c] - pred[b,n,t,c]) * avail[b,t])^2)
 *               an unavailable step contributes 0 and STILL COUNTS in every mean over t: the means divide by T, not by the number
 *               of available steps (upstream's np.mean over the time axis)
 *   ade[b,n]  = (sum_t e[b,n,t]) / T
 *   last[b]   = max_t ((avail[b,t] > 0) * t): the last available step, 0 when none is
 *   fde[b,n]  = e[b,n,last[b]]                      (so 0 when nothing is available: e is 0 there)
 *   d[b,i,j]  = (sum_t |pred[b,i,t] - pred[b,j,t]|) / T           avail is ignored
 *   f[b,i,j]  = sqrt(sum_t (y[b,i,t] - y[b,j,t])^2), y = channel 1
 *               UPSTREAM'S QUIRK, reproduced as it is: batch_final_diversity takes pred[..., -1], which is the last COORDINATE (y),
 *               not the last time step its docstring speaks of, and then the norm over the TIME axis
 *   l[b,i,j]  = |pred[b,i,T-1] - pred[b,j,T-1]|     what that docstring describes; this library's addition, no upstream key
 *
 * per_agent [B, CLD_SM_COLS] fp64, row b:
 *   CLD_SM_ADE_MEAN  (sum_n ade[b,n]) / N       CLD_SM_ADE_MIN  min_n ade[b,n]        "mean" / "oracle" mode before the batch mean
 *   CLD_SM_FDE_MEAN  (sum_n fde[b,n]) / N       CLD_SM_FDE_MIN  min_n fde[b,n]
 *   CLD_SM_APD_MEAN  (sum_ij d[b,i,j]) / N^2    CLD_SM_APD_MAX  max_ij d[b,i,j]       over ALL N N entries, the zero diagonal included:
 *   CLD_SM_FPD_MEAN  (sum_ij f[b,i,j]) / N^2    CLD_SM_FPD_MAX  max_ij f[b,i,j]       evaluated as 2 sum_{i<j} / N^2 (d, f, l are symmetric);
 *   CLD_SM_LAST_PD_MEAN, CLD_SM_LAST_PD_MAX     the same of l[b,i,j]                  N = 1: mean and max are 0
 * index [B,4] int32, row b: the first n with ade[b,n] = the minimum, the first n with fde[b,n] = the minimum, last[b], and the
 *   non-finite flag: 1 when a NaN or an infinity stands in channels 0, 1 of pred[b], in gt[b] or in avail[b] (upstream asserts
 *   finiteness of the whole batch in _assert_shapes; here the other agents' rows are what they are without it, and the flagged row
 *   holds whatever the arithmetic gives).
 * means [CLD_SM_COLS] fp64, or NULL: the batch means (sum_b per_agent[b, c]) / B -- upstream's eight keys are columns 0 .. 7:
 *   ego_avg_ADE, ego_min_ADE, ego_avg_FDE, ego_min_FDE, ego_avg_APD, ego_max_APD, ego_avg_FPD, ego_max_FPD.
 *
 * Arithmetic: the fp32 inputs are widened; every difference, product, square root and sum is fp64.  Sums over t are sequential in
 * ascending t; sums, minima and maxima over samples and pairs follow a fixed tree that depends on N alone, the batch means one that
 * depends on B alone (partials of 256 rows in the workspace, folded by one workgroup): no atomics, the same bits on every run, and
 * a row's bits do not depend on the batch it is computed in.  The handle's precision does not enter.
 *
 * Reach: one workgroup stages an agent's N T positions in LDS: N <= CLD_SM_MAX_SAMPLES and N T <= CLD_SM_MAX_POINTS; beyond that
 * CLD_ERR_ARG -- there is no other path.  B <= 2^20.
 * CLD_ERR_ARG: NULL pred / gt / avail / per_agent / index, B, N or T < 1, C outside 2 .. 8, the reach above, per_agent or means not
 * 8-byte aligned.  CLD_ERR_WORKSPACE (only with means): workspace NULL, not 8-byte aligned, or shorter than
 * cld_sample_metrics_workspace_bytes(B) (0 for a B out of range). */
enum {
    CLD_SM_ADE_MEAN = 0, CLD_SM_ADE_MIN = 1, CLD_SM_FDE_MEAN = 2, CLD_SM_FDE_MIN = 3, CLD_SM_APD_MEAN = 4, CLD_SM_APD_MAX = 5,
    CLD_SM_FPD_MEAN = 6, CLD_SM_FPD_MAX = 7, CLD_SM_LAST_PD_MEAN = 8, CLD_SM_LAST_PD_MAX = 9
};
#define CLD_SM_COLS 10
#define CLD_SM_MAX_SAMPLES 256
#define CLD_SM_MAX_POINTS 8192

size_t cld_sample_metrics_workspace_bytes(int32_t B);

int cld_sample_metrics(cld_handle h, const float* pred, int32_t C, const float* gt, const float* avail, int32_t B, int32_t N, int32_t T,
                       double* per_agent, int32_t* index, double* means, void* workspace, size_t workspace_bytes, void* stream);

/* The number of workgroups one launch of the per-agent kernel holds at most; agent b + k * that is taken by the workgroup of agent b
 * in pass k.  No handle, no device call: for tests that straddle it. */
int32_t cld_debug_sample_metrics_max_blocks(void);

#ifdef __cplusplus
}
#endif

#endif
