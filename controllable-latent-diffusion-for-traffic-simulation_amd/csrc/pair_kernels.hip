// pair_kernels.hip -- upstream's pair-relation guidance losses (src/tbsim/utils/guidance_loss.py: KeepDistanceLoss :1631-1688,
// CollisionLoss :1691-1734, KeepDistanceLoss2 :1739-1791, FrontCollisionLoss :1844-1896, CollideLeftSideLoss :1899-1956, StayAwayLoss
// :2014-2082) and their gradient w.r.t. the decoded plans, as one launch over all pairs of all scenes and all samples.
//
// A pair is (target i, ref j).  Per (sample n, step t) the plan positions of both go to the world with each agent's own
// world_from_agent and from there into the REF agent's static frame, rotation M_j (agent_from_world[j], or R_j^T when none is given).
// With q = M_j (p_i - p_j), d = |q| (for kind COLLISION d = |p_i - p_j|, in the world, as upstream takes it) the step's term e_t is
//   KEEP_DISTANCE    relu(lo - d) + relu(d - hi)
//   COLLISION        relu(d - lo)
//   STAY_AWAY        relu(d - hi) + relu(lo - d)            weighted decay^t / sum_t decay^t
//   FRONT_COLLISION  |q.x| + relu(q.y)                      (upstream's Delta = p_j - p_i = -q: |Dx| + relu(-Dy))
//   COLLIDE_LEFT     |q.x| + relu(-q.y)                     (|Dx| + relu(Dy))
// and value[pair, n] = sum_t w_t e_t with w_t = 1 / 52, or decay^t / sum_t decay^t / 52 where decay > 0 (normalised AND averaged, as
// upstream does).  Both agents receive gradient: d e / d p_i = +g, d e / d p_j = -g in the world, each rotated back by the agent's own
// R_a^T into the x, y columns of its plan.  Backward rules as torch's: clip(min=0) passes where its argument is >= 0, the norm's
// gradient at d = 0 is 0, abs at 0 gives 0.
//
// Positions are formed relative to the REF agent's frame origin before they are differenced: p_j = R_j (x, y), p_i = R_i (x, y) +
// (t_i - t_j).  The translations enter as one difference of two frame origins of the same scene, so the fp32 differences carry the
// rounding of the metres between two agents and not of the scene's offset from the world origin (hundreds of metres).  The frame's
// own translation cancels in q, so it is never added.
//
// Launch: blockIdx.x < grad_blocks is the GRADIENT role, the rest the VALUE role; both spread over the chip by item, never one
// workgroup per pair (32 pairs would be 32 workgroups on an eighth of the chip -- the mistake social_kernels.hip's header records).
//   gradient  a thread owns (involved agent, sample, step).  An agent may sit in several pairs, in either role, so the gradient is a
//             GATHER: the host lists, per involved agent, its (pair, role) incidences in ascending order (CSR); the thread walks them
//             in that order, forms each pair term from the two plans, sums the world gradients, rotates the sum by its own R_a^T and
//             adds it to the row (which holds grad_in or 0 already: launch_pair).  Rows in no pair are never touched.
//   values    one wave per (pair, sample), lanes are steps; lane 0 adds the 52 weighted terms up in ascending t.
// Every output element is computed by one thread in a fixed order: no atomics, the same bits on every run and under every launch
// shape.  Plain fp32 in both library precisions.
//
// Device-side indices are never trusted: a pair whose target or ref lies outside [0, A), or with target == ref, is not evaluated
// (NaN value, no contribution); CSR entries that point outside the arrays, or name a pair the agent is not part of, are skipped.
// One thing is NOT checked: that agent_id lists every agent once.  A duplicated agent_id is no out-of-bounds access, but two threads
// then add to the same row, and the "same bits on every run" no longer holds for that row; the lists are the caller's contract
// (engine.pair_incidences builds them so).
#include "cld_kernels.h"

namespace cld {

namespace {
constexpr int TT = 52;
constexpr int kThreads = 256;              // gradient role: 256 (agent, sample, step) items; value role: 4 waves = 4 (pair, sample)
constexpr int kWaves = kThreads / 64;

// w_t of a pair: 1 / 52, or decay^t / sum_u decay^u / 52 (the powers by repeated multiplication, the sum in ascending u)
__device__ __forceinline__ float step_weight(float decay, int t) {
    if (!(decay > 0.f)) return 1.0f / (float)TT;
    float w = 1.f, sum = 0.f, wt = 0.f;
    for (int u = 0; u < TT; ++u) {
        sum += w;
        if (u == t) wt = w;
        w *= decay;
    }
    return wt / sum / (float)TT;
}

__device__ __forceinline__ bool pair_valid(int i, int j, int A) { return (unsigned)i < (unsigned)A && (unsigned)j < (unsigned)A && i != j; }

// the term of pair pr = (i, j) at (sample n, step t): returns e_t and (gx, gy) = d e_t / d p_i in the world frame (= -d e_t / d p_j)
__device__ __forceinline__ float pair_step(const PairArgs& p, int pr, int i, int j, int n, int t, float& gx, float& gy) {
    const float* Wi = p.world_from_agent + (size_t)i * 9;
    const float* Wj = p.world_from_agent + (size_t)j * 9;
    const float* qi = p.traj + (((size_t)i * p.num_samp + n) * TT + t) * 6;
    const float* qj = p.traj + (((size_t)j * p.num_samp + n) * TT + t) * 6;
    const float xi = qi[0], yi = qi[1], xj = qj[0], yj = qj[1];
    // relative to the ref agent's frame origin
    const float pix = Wi[0] * xi + Wi[1] * yi + (Wi[2] - Wj[2]), piy = Wi[3] * xi + Wi[4] * yi + (Wi[5] - Wj[5]);
    const float pjx = Wj[0] * xj + Wj[1] * yj, pjy = Wj[3] * xj + Wj[4] * yj;
    const float dx = pix - pjx, dy = piy - pjy;
    const int kind = p.kind[pr];
    const float lo = p.lo[pr], hi = p.hi[pr];
    if (kind == PAIR_COLLISION) {
        const float d = sqrtf(__fmaf_rn(dx, dx, dy * dy));
        const float s = (d - lo >= 0.f && d > 0.f) ? 1.0f / d : 0.f;
        gx = s * dx; gy = s * dy;
        return fmaxf(d - lo, 0.f);
    }
    float m00, m01, m10, m11;
    if (p.agent_from_world) {
        const float* F = p.agent_from_world + (size_t)j * 9;
        m00 = F[0]; m01 = F[1]; m10 = F[3]; m11 = F[4];
    } else {
        m00 = Wj[0]; m01 = Wj[3]; m10 = Wj[1]; m11 = Wj[4];
    }
    const float qx = m00 * dx + m01 * dy, qy = m10 * dx + m11 * dy;
    float e, ex, ey;                                                     // e_t and d e_t / d q
    if (kind == PAIR_FRONT_COLLISION || kind == PAIR_COLLIDE_LEFT) {
        const float sy = kind == PAIR_FRONT_COLLISION ? 1.f : -1.f;
        e = fabsf(qx) + fmaxf(sy * qy, 0.f);
        ex = qx > 0.f ? 1.f : (qx < 0.f ? -1.f : 0.f);
        ey = sy * qy >= 0.f ? sy : 0.f;
    } else {                                                             // KEEP_DISTANCE, STAY_AWAY
        const float d = sqrtf(__fmaf_rn(qx, qx, qy * qy));
        e = fmaxf(lo - d, 0.f) + fmaxf(d - hi, 0.f);
        const float c = (d - hi >= 0.f ? 1.f : 0.f) - (lo - d >= 0.f ? 1.f : 0.f);
        const float s = d > 0.f ? c / d : 0.f;
        ex = s * qx; ey = s * qy;
    }
    gx = m00 * ex + m10 * ey; gy = m01 * ex + m11 * ey;                 // M^T (d e / d q)
    return e;
}

__global__ __launch_bounds__(kThreads) void pair_kernel(const PairArgs p, int grad_blocks) {
    const int A = p.rows / p.num_samp;
    if ((int)blockIdx.x >= grad_blocks) {                                // value role
        const int lane = threadIdx.x & 63;
        const int item = ((int)blockIdx.x - grad_blocks) * kWaves + (threadIdx.x >> 6);
        if (item >= p.num_pairs * p.num_samp) return;                    // (wave-uniform)
        const int pr = item / p.num_samp, n = item - pr * p.num_samp;
        const int i = p.target[pr], j = p.ref[pr];
        if (!pair_valid(i, j, A)) {
            if (lane == 0) p.value[item] = __builtin_nanf("");
            return;
        }
        float v = 0.f;
        if (lane < TT) {
            float gx, gy;
            v = pair_step(p, pr, i, j, n, lane, gx, gy) * step_weight(p.decay[pr], lane);
        }
        float s = 0.f;
        for (int t = 0; t < TT; ++t) s += __shfl(v, t);                  // ascending t; every lane forms the same sum
        if (lane == 0) p.value[item] = s;
        return;
    }
    const int idx = blockIdx.x * kThreads + threadIdx.x;                 // gradient role: (involved agent, sample, step), step fastest
    if (idx >= p.num_involved * p.num_samp * TT) return;
    const int t = idx % TT, rest = idx / TT;
    const int ia = rest / p.num_samp, n = rest - ia * p.num_samp;
    const int a = p.agent_id[ia];
    if ((unsigned)a >= (unsigned)A) return;
    const int s0 = max(p.agent_start[ia], 0), s1 = min(p.agent_start[ia + 1], p.num_incidences);
    float gx = 0.f, gy = 0.f;
    float last_decay = 0.f, w = 1.0f / (float)TT;                        // w_t of the last decay seen: pairs of one config family share it,
    for (int s = s0; s < s1; ++s) {                                      // so an agent in many decayed pairs runs the 52-step sum once
        const int inc = p.incidence[s];
        const int pr = inc >> 1, role = inc & 1;
        if ((unsigned)pr >= (unsigned)p.num_pairs) continue;
        const int i = p.target[pr], j = p.ref[pr];
        if (!pair_valid(i, j, A) || (role ? j : i) != a) continue;
        float ux, uy;
        pair_step(p, pr, i, j, n, t, ux, uy);
        const float dec = p.decay[pr] > 0.f ? p.decay[pr] : 0.f;
        if (dec != last_decay) { w = step_weight(dec, t); last_decay = dec; }
        const float c = p.scale[pr] * w;
        gx += role ? -(c * ux) : c * ux;
        gy += role ? -(c * uy) : c * uy;
    }
    const float* W = p.world_from_agent + (size_t)a * 9;
    float* o = p.grad + (((size_t)a * p.num_samp + n) * TT + t) * 6;    // holds grad_in (or 0) already: launch_pair
    o[0] += W[0] * gx + W[3] * gy;
    o[1] += W[1] * gx + W[4] * gy;
}
}  // namespace

hipError_t launch_pair(const PairArgs& a, const float* grad_in, hipStream_t s) {
    if (a.rows < 1 || a.num_samp < 1 || a.rows % a.num_samp || a.num_pairs < 1 || a.num_involved < 0 || a.num_incidences < 0 || (!a.value && !a.grad))
        return hipErrorInvalidValue;
    const long long grad_items = a.grad ? (long long)a.num_involved * a.num_samp * TT : 0;
    const long long value_items = a.value ? (long long)a.num_pairs * a.num_samp : 0;
    const long long grad_blocks = (grad_items + kThreads - 1) / kThreads, value_blocks = (value_items + kWaves - 1) / kWaves;
    if (grad_items > INT32_MAX || value_items > INT32_MAX || grad_blocks + value_blocks > INT32_MAX) return hipErrorInvalidValue;
    if (const hipError_t e = seed_grad(a.grad, grad_in, a.rows, s); e != hipSuccess) return e;      // rows in no pair: the gradient of grad_in (or 0)
    if (grad_blocks + value_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(pair_kernel, dim3((unsigned)(grad_blocks + value_blocks)), dim3(kThreads), 0, s, a, (int)grad_blocks);
    return hipGetLastError();
}

}  // namespace cld
