// goal_kernels.hip -- upstream's GlobalTargetPosLoss and GlobalTargetPosAtTimeLoss (src/tbsim/utils/guidance_loss.py:876-1135) and
// their gradient w.r.t. the decoded plans, as one launch: the two guidance losses that give an agent a destination in the WORLD
// frame, which is what a closed-loop rollout needs (the agent frame of the local waypoint losses moves at every re-plan).
//
// One wave per plan (row = agent * num_samp + sample), lane = time step: every term is a function of the 52 distances
// d_t = |pos_t - p| to the target taken into the agent frame, p = agent_from_world[a] target_pos[a].  Per agent the loss is one of
//   kind 1, |p| <  H dt pref_speed (target within reach of one plan): TargetPosLoss with min_target_time = 0 (:672-712),
//                                                                      mean_t(softmin_t(d) d_t^2) -- min, normaliser and the weighted
//                                                                      sum are wave reductions
//   kind 1, otherwise:   relu(max(urgency H dt pref_speed, min_progress_dist) - (d_0 - d_51))          (compute_progress_loss, :912-926)
//   kind 2, lt = target_time - global_t:  lt < 0: 0;  lt < H: d_lt (TargetPosAtTimeLoss, :632-670);
//                                         else relu(d_51 - lt dt pref_speed (1 - urgency))             (:900-911)
// and 0 for an agent whose `reached` flag is set (have_reached_mask, :1019-1029).  The gradient goes to the x, y columns of the steps
// the value reads, scaled by scale[a] (weight / agents of the config, as DiffuserGuidance averages), and is ADDED to grad_in: relu and
// the norm pass gradients as torch does (zero on the inactive side, zero at distance 0).  The reductions are butterflies in a fixed
// order and nothing is accumulated across waves: no atomics, the same bits on every run.  Plain fp32 in both library precisions.
#include "cld_kernels.h"

namespace cld {

namespace {
constexpr int TT = 52;
constexpr int kRowsPerWg = 4;              // one wave per plan

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(64 * kRowsPerWg) void goal_kernel(const GoalArgs p) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * kRowsPerWg + (threadIdx.x >> 6);
    if (row >= p.rows) return;                                       // (wave-uniform)
    const int a = row / p.num_samp;
    const bool on = lane < TT;
    const size_t o = ((size_t)row * TT + (on ? lane : 0)) * 6;
    const int kind = (p.reached && p.reached[a]) ? 0 : p.kind[a];
    float value = 0.f, gx = 0.f, gy = 0.f;                           // this lane's d value / d (x_t, y_t)
    if (kind == 1 || kind == 2) {
        const float* M = p.agent_from_world + (size_t)a * 9;
        const float tx = p.target_pos[a * 2 + 0], ty = p.target_pos[a * 2 + 1];
        const float px = M[0] * tx + M[1] * ty + M[2], py = M[3] * tx + M[4] * ty + M[5];
        const float ex = p.traj[o] - px, ey = p.traj[o + 1] - py;
        const float d = sqrtf(ex * ex + ey * ey);
        const float inv = d > 0.f ? 1.0f / d : 0.f;                  // torch.norm's backward is 0 at 0
        const float ux = ex * inv, uy = ey * inv;                    // d d_t / d pos_t
        const float ps = p.pref_speed[a], urg = p.urgency[a];
        const float d0 = __shfl(d, 0), d51 = __shfl(d, TT - 1);
        if (kind == 1) {
            const float reach = (float)TT * p.dt * ps;
            if (sqrtf(px * px + py * py) < reach) {
                const float dmin = wave_min(on ? d : 3.0e38f);
                const float e = on ? expf(-(d - dmin)) : 0.f;
                const float Z = wave_sum(e);
                const float S = wave_sum(e * d * d) / Z;             // sum_t w_t d_t^2
                const float w = e / Z;
                value = S / (float)TT;
                // d/d pos_k = (w_k / H) (2 (pos_k - p) + (S - d_k^2) (pos_k - p) / d_k): the squared term is differentiated as
                // a sum of squares, the softmin weights through the norm
                const float c = w / (float)TT;
                gx = c * (2.f * ex + (S - d * d) * ux);
                gy = c * (2.f * ey + (S - d * d) * uy);
            } else {
                const float arg = fmaxf(urg * reach, p.min_progress_dist) - (d0 - d51);
                value = fmaxf(arg, 0.f);
                if (arg > 0.f) {
                    const float sgn = lane == 0 ? -1.f : (lane == TT - 1 ? 1.f : 0.f);
                    gx = sgn * ux; gy = sgn * uy;
                }
            }
        } else {
            const int lt = p.target_time[a] - p.global_t;
            if (lt >= 0 && lt < TT) {
                value = __shfl(d, lt);
                if (lane == lt) { gx = ux; gy = uy; }
            } else if (lt >= TT) {
                const float arg = d51 - (float)lt * p.dt * ps * (1.0f - urg);
                value = fmaxf(arg, 0.f);
                if (arg > 0.f && lane == TT - 1) { gx = ux; gy = uy; }
            }
        }
    }
    if (p.loss && lane == 0) p.loss[row] = value;
    if (p.grad && on) {
        const float sc = kind ? p.scale[a] : 0.f;
        const float* gi = p.grad_in ? p.grad_in + o : nullptr;      // (may be grad itself: a lane reads its six values before it writes them)
        float v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = gi ? gi[k] : 0.f;
        if (kind) { v[0] += sc * gx; v[1] += sc * gy; }
#pragma unroll
        for (int k = 0; k < 6; ++k) p.grad[o + k] = v[k];
    }
}
}  // namespace

hipError_t launch_goal(const GoalArgs& a, hipStream_t s) {
    if (a.rows < 1 || a.num_samp < 1 || a.rows % a.num_samp) return hipErrorInvalidValue;
    hipLaunchKernelGGL(goal_kernel, dim3((a.rows + kRowsPerWg - 1) / kRowsPerWg), dim3(64 * kRowsPerWg), 0, s, a);
    return hipGetLastError();
}

}  // namespace cld
