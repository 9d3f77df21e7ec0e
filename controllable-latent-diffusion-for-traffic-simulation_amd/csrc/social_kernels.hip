// social_kernels.hip -- upstream's SocialGroupLoss (src/tbsim/utils/guidance_loss.py:1137-1207, `social_group`) and its gradient
// w.r.t. the decoded plans, as one launch over all groups of all scenes and all samples.
//
// Per (sample n, step t) member i of a group of M is paired with nb(i, t) = u < cohesion ? (r < i ? r : r + 1) : the nearest other
// member (squared distances, strict <, so the lowest index wins a tie, as torch.argmin); (r, u) is this evaluation's draw of
// (plan row, t); cohesion == 0 draws nothing.  value[i, n] = mean_t (d_{i,nb} - social_dist)^2.  The gradient of a pair term,
// 2 (d - social_dist) (p_k - p_other) / d (0 at d = 0, as torch.norm's backward), goes to both ends except to the leader -- the
// member whose AGENT index equals leader[g], detached upstream -- times scale[g] / 52, rotated back by R_k^T into the plan's x, y.
//
// World positions of the members sit in LDS as [step][member] float2 (8 B per pose, odd row stride), relative to the first member's
// frame origin: R_a (x, y) + (t_a - t_first).  Only differences of member positions are ever formed, and the shift keeps them at the
// group's own extent instead of at the world offset of the scene, so the fp32 differences carry the rounding of metres, not of
// hundreds of metres.
//
// A (group, sample) is blockIdx.x; blockIdx.y splits it over workgroups in two ROLES, because the two outputs split differently:
//   gradient  a workgroup owns a run of STEPS (all members).  Steps are independent of one another: pass 1, thread = (step, member
//             i), walks the group for nb and keeps it in LDS (one byte); pass 2, thread = (step, member k), is a GATHER: the member's
//             own term, then in ascending i the terms of the members whose neighbour at that step is k.
//   values    a workgroup owns a run of MEMBERS (all 52 steps): thread = (step, own member) walks the group for nb and leaves
//             (d - social_dist)^2 in LDS; one thread per own member adds the 52 up in ascending t.  No gather, so nothing but the own
//             members' neighbours is needed.
// The first form of this kernel did both in one workgroup per (group, sample): 32 groups of 64 members were 32 workgroups, one wave
// per SIMD on an eighth of the chip, and took 219 us (the agent-collision launch on the same scenes: 83 us).  The neighbour walk is
// done in both roles; it is the cheap part once it is spread out: 24.7 us.
//
// Every output element is computed by one thread in a fixed order that does not depend on the split, and nothing is accumulated
// across threads or workgroups: no atomics, the same bits on every run and under every launch shape.  Plain fp32 in both precisions.
//
// The draws are the caller's (draw_r, draw_u: one per plan row and step, non-members ignored) or, when both are null, the generator
// of cld_kernels.h under a stream tag of its own: k = splitmix64(seed ^ splitmix64(splitmix64(tag ^ eval) + row * 52 + t)),
// u = u01(splitmix64(k)), r = floor(bits32 (M - 1) / 2^32) with bits32 the high half of splitmix64(k + 1).
#include "cld_kernels.h"

namespace cld {

namespace {
constexpr int TT = 52;
constexpr int kThreads = 256;
constexpr int kOwn = 8;                    // members whose values one workgroup of the value role computes: 8 x 52 = 416 items
constexpr unsigned long long kSocialStream = 0x536F6369616C4772ull;      // no (seed, step, row) key of the diffusion noise maps here

__device__ __forceinline__ float pair_dist(const float2 a, const float2 b, float& dx, float& dy) {
    dx = a.x - b.x; dy = a.y - b.y;
    return sqrtf(__fmaf_rn(dx, dx, dy * dy));                           // (spelled out: the same rounding in both roles)
}

// world positions (relative to the group's origin) of all members at steps t0 .. t0 + nt - 1 -> pos[(t - t0) * Ms + i]
__device__ __forceinline__ void load_positions(const SocialArgs& p, float2* pos, int gs, int M, int Ms, int n, int t0, int nt) {
    const int a0 = p.member[gs];
    const float ox = p.world_from_agent[(size_t)a0 * 9 + 2], oy = p.world_from_agent[(size_t)a0 * 9 + 5];
    for (int idx = threadIdx.x; idx < M * nt; idx += kThreads) {         // (member-major: a member's steps are neighbours in memory)
        const int i = idx / nt, tt = idx - i * nt;
        const int a = p.member[gs + i];
        const float* W = p.world_from_agent + (size_t)a * 9;
        const float* q = p.traj + (((size_t)a * p.num_samp + n) * TT + t0 + tt) * 6;
        const float x = q[0], y = q[1];
        pos[tt * Ms + i] = make_float2(W[0] * x + W[1] * y + (W[2] - ox), W[3] * x + W[4] * y + (W[5] - oy));
    }
}

// nb(i, t): `row` = the M positions of step t, a = member i's agent index
__device__ __forceinline__ int neighbour(const SocialArgs& p, const float2* row, int M, int i, int a, int n, int t, float coh) {
    const float2 pi = row[i];
    float best = __builtin_inff();
    int nb = i == 0 ? 1 : 0;
#pragma unroll 4
    for (int j = 0; j < M; ++j) {
        const float dx = pi.x - row[j].x, dy = pi.y - row[j].y;
        const float d2 = __fmaf_rn(dx, dx, dy * dy);
        if (j != i && d2 < best) { best = d2; nb = j; }
    }
    if (coh > 0.f) {
        const size_t e = ((size_t)a * p.num_samp + n) * TT + t;
        float u;
        int r;
        if (p.draw_u) {
            u = p.draw_u[e]; r = p.draw_r[e];
        } else {
            const unsigned long long k = splitmix64(p.seed ^ splitmix64(splitmix64(kSocialStream ^ p.eval) + e));
            u = u01(splitmix64(k));
            r = (int)(((splitmix64(k + 1) >> 32) * (unsigned long long)(M - 1)) >> 32);
        }
        r = min(max(r, 0), M - 2);                                       // (a caller's draw outside [0, M - 2] must not index past the group)
        if (u < coh) nb = r < i ? r : r + 1;
    }
    return nb;
}

// grid (num_groups * num_samp, time_chunks + member_chunks): blockIdx.y < time_chunks is the gradient role on steps
// [y * steps_per_wg, ...), the rest the value role on members [(y - time_chunks) * kOwn, ...)
__global__ __launch_bounds__(kThreads) void social_group_kernel(const SocialArgs p, int time_chunks, int steps_per_wg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int g = blockIdx.x / p.num_samp, n = blockIdx.x - g * p.num_samp;
    const int gs = p.group_start[g], M = p.group_start[g + 1] - gs;
    const int A = p.rows / p.num_samp;
    const bool value_role = (int)blockIdx.y >= time_chunks;
    const int chunk = value_role ? (int)blockIdx.y - time_chunks : (int)blockIdx.y;
    // what the launch was not sized for (or upstream cannot run: fewer than two members) is not evaluated: NaN values, gradient untouched
    int bad = M < 2 || M > p.max_members;
    if (!bad)
        for (int i = threadIdx.x; i < M; i += kThreads) bad |= (unsigned)p.member[gs + i] >= (unsigned)A;
    if (__syncthreads_or(bad)) {
        if (value_role && chunk == 0)
            for (int i = threadIdx.x; i < M; i += kThreads) {
                const int a = p.member[gs + i];
                if ((unsigned)a < (unsigned)A) p.loss[(size_t)a * p.num_samp + n] = __builtin_nanf("");
            }
        return;
    }
    const int Ms = M | 1;                                                 // odd row stride: the rows of different steps start on different banks
    const float sd = p.social_dist[g], coh = p.cohesion[g];
    float2* pos = reinterpret_cast<float2*>(smem);
    if (value_role) {
        const int i0 = chunk * kOwn, own = min(kOwn, M - i0);
        if (own <= 0) return;
        float* esq = reinterpret_cast<float*>(pos + TT * Ms);             // [own][TT]
        load_positions(p, pos, gs, M, Ms, n, 0, TT);
        __syncthreads();
        for (int idx = threadIdx.x; idx < own * TT; idx += kThreads) {
            const int t = idx / own, io = idx - t * own, i = i0 + io;
            const float2* row = pos + t * Ms;
            const int nb = neighbour(p, row, M, i, p.member[gs + i], n, t, coh);
            float dx, dy;
            const float e = pair_dist(row[i], row[nb], dx, dy) - sd;
            esq[io * TT + t] = e * e;
        }
        __syncthreads();
        for (int io = threadIdx.x; io < own; io += kThreads) {
            float s = 0.f;
            for (int t = 0; t < TT; ++t) s += esq[io * TT + t];
            p.loss[(size_t)p.member[gs + i0 + io] * p.num_samp + n] = s / (float)TT;
        }
        return;
    }
    const int t0 = chunk * steps_per_wg, nt = min(steps_per_wg, TT - t0);
    unsigned char* nbs = reinterpret_cast<unsigned char*>(pos + nt * Ms);   // [nt][Ms]
    load_positions(p, pos, gs, M, Ms, n, t0, nt);
    __syncthreads();
    for (int idx = threadIdx.x; idx < M * nt; idx += kThreads) {
        const int tt = idx / M, i = idx - tt * M;
        nbs[tt * Ms + i] = (unsigned char)neighbour(p, pos + tt * Ms, M, i, p.member[gs + i], n, t0 + tt, coh);
    }
    __syncthreads();
    const float c = 2.0f * p.scale[g] / (float)TT;
    const int leader = p.leader[g];
    for (int idx = threadIdx.x; idx < M * nt; idx += kThreads) {
        const int tt = idx / M, k = idx - tt * M;
        const int a = p.member[gs + k];
        if (a == leader) continue;
        const float2* row = pos + tt * Ms;
        const unsigned char* nrow = nbs + tt * Ms;
        const float2 pk = row[k];
        float dx, dy;
        float d = pair_dist(pk, row[nrow[k]], dx, dy);
        float w = d > 0.f ? (d - sd) / d : 0.f;
        float gx = w * dx, gy = w * dy;
        for (int i = 0; i < M; ++i) {
            if (i == k || nrow[i] != k) continue;
            d = pair_dist(pk, row[i], dx, dy);
            w = d > 0.f ? (d - sd) / d : 0.f;
            gx += w * dx; gy += w * dy;
        }
        gx *= c; gy *= c;
        const float* W = p.world_from_agent + (size_t)a * 9;
        float* o = p.grad + (((size_t)a * p.num_samp + n) * TT + t0 + tt) * 6;    // holds grad_in (or 0) already: launch_social_group
        o[0] += W[0] * gx + W[3] * gy;
        o[1] += W[1] * gx + W[4] * gy;
    }
}
}  // namespace

hipError_t launch_social_group(const SocialArgs& a, const float* grad_in, hipStream_t s) {
    if (a.rows < 1 || a.num_samp < 1 || a.rows % a.num_samp || a.num_groups < 1 || a.max_members < 2 || a.max_members > kSocialMaxMembers ||
        (!a.loss && !a.grad))
        return hipErrorInvalidValue;
    // rows outside every group: value 0 and the gradient of grad_in; the kernel then adds to its members' rows in place
    if (a.loss) {
        const hipError_t e = hipMemsetAsync(a.loss, 0, (size_t)a.rows * sizeof(float), s);
        if (e != hipSuccess) return e;
    }
    if (const hipError_t e = seed_grad(a.grad, grad_in, a.rows, s); e != hipSuccess) return e;
    // about one (step, member) item per thread in the gradient role: 52 steps for a group of 4, 4 for one of 64, 2 for one of 128
    const int Ms = a.max_members | 1;
    const int steps_per_wg = std::min(TT, std::max(1, kThreads / a.max_members));
    const int time_chunks = a.grad ? (TT + steps_per_wg - 1) / steps_per_wg : 0;
    const int member_chunks = a.loss ? (a.max_members + kOwn - 1) / kOwn : 0;
    const size_t lds_grad = a.grad ? (size_t)steps_per_wg * Ms * (sizeof(float2) + 1) : 0;
    const size_t lds_value = a.loss ? (size_t)TT * Ms * sizeof(float2) + (size_t)kOwn * TT * sizeof(float) : 0;
    const size_t lds = (std::max(lds_grad, lds_value) + 15) / 16 * 16;
    hipLaunchKernelGGL(social_group_kernel, dim3(a.num_groups * a.num_samp, time_chunks + member_chunks), dim3(kThreads), lds, s, a, time_chunks,
                       steps_per_wg);
    return hipGetLastError();
}

}  // namespace cld
