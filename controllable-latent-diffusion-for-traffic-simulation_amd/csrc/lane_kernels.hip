// lane_kernels.hip -- upstream's lane-projection guidance losses (src/tbsim/utils/guidance_loss.py: LaneFollowingLoss :1574-1628,
// ChangeToLeftLaneLoss :1795-1841, FollowLaneLoss :1958-2011) and their gradient w.r.t. the decoded plans, from the polyline onward:
// the preparation of the polylines (get_lane_projection, trajdata_utils.py:573-664, from `transform_xyh_np` to the sort by x) and the
// projection of every plan point of every sample onto its agent's polyline (project_onto, :726-821).
//
// lane_prepare  one workgroup per polyline.  A thread transforms its points in fp64 (x, y through the 3x3 matrix, heading' = atan2 of
//               the rotated (cos h, sin h)), rounds once to fp32 and files the key (orderable bits of x, original index) in LDS; a
//               bitonic network over the next power of two >= max_pts sorts the 64-bit keys, NaN x last, equal x by original index
//               (-0 counts as +0); row r of the output is the point whose key came r-th.  Runs once per plan, not per denoising step.
//
// lane_loss     one workgroup of 4 waves per (entry, sample); an agent's entries are contiguous, and the workgroup of the FIRST entry
//               of an agent walks the agent's whole run in order (the others leave at once), so every gradient row has one writer and
//               a fixed summation order: no atomics, the same bits on every run.  Per entry the workgroup stages the polyline's segments
//               in LDS -- (p0, d = p1 - p0) as one 16-byte word, 1 / |d|^2 (NaN marks a segment with a NaN end or of zero length: it is
//               never chosen, as upstream's NaN distance -> +inf), the heading of p0 -- and finds the last usable segment, so the NaN
//               padding is not walked.  A LANE owns a plan step (52 of 64 busy) and a WAVE every 4th segment: all lanes of a wave read
//               the same LDS word (a broadcast), there is no cross-lane reduction inside the loop, and a polyline of 2 points leaves
//               no lane idle that a longer one would use -- only three waves without a segment.  Each lane keeps its (squared distance,
//               segment) minimum over ascending segments with a strict <, the four waves' minima meet in LDS and wave 0 takes the
//               lexicographic (distance, segment) minimum: ties go to the first segment, as torch's argmin.  Squared distances are
//               compared (the root is monotone; it is taken once, for the loss).  Wave 0 forms the step terms, the value
//               (ascending t, as pair_kernels.hip) and the gradient, which it adds to the agent's row after the run.
// The projection is a constant for the gradient (upstream detaches positions and yaws before projecting).  Plain fp32 in both
// library precisions.
//
// Device-side data is never trusted: an entry whose agent lies outside [0, A) or whose line lies outside [0, num_lines), or whose
// polyline has no segment with a finite, non-zero length, is not evaluated (NaN value, NaN projection, no contribution).  NOT checked:
// that an agent's entries are contiguous -- an agent in two separate runs stays inside the arrays, but two workgroups then add to
// one row and its bits are no longer the same on every run; the order is the caller's contract (Engine._lane refuses such a term).
#include "cld_kernels.h"
#include "lane_kernels.h"

namespace cld {

namespace {
constexpr int TT = 52;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;       // the stride at which a wave walks the segments

__device__ __forceinline__ unsigned long long sort_key(float x, int idx) {
    unsigned int u;
    if (x != x) {
        u = 0xFFFFFFFFu;                                                 // NaN last
    } else {
        u = x == 0.f ? 0u : __float_as_uint(x);                          // -0 counts as +0
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                  // ascending unsigned order = ascending float order
    }
    return ((unsigned long long)u << 32) | (unsigned int)idx;
}

__global__ __launch_bounds__(kThreads) void lane_prepare_kernel(const LanePrepareArgs p, int n2) {
    __shared__ unsigned long long key[kLaneMaxPts];
    __shared__ float px[kLaneMaxPts], py[kLaneMaxPts], ph[kLaneMaxPts];
    const int ln = blockIdx.x, S = p.max_pts;
    const int f = p.line_frame[ln];
    const bool frame_ok = (unsigned)f < (unsigned)p.num_frames;
    double m[6] = {0, 0, 0, 0, 0, 0};
    if (frame_ok)
        for (int k = 0; k < 6; ++k) m[k] = (double)p.agent_from_world[(size_t)f * 9 + k];
    const double* src = p.world_lines + (size_t)ln * S * 3;
    const float nanf_ = __builtin_nanf("");
    for (int i = threadIdx.x; i < n2; i += kThreads) {
        float x = nanf_, y = nanf_, h = nanf_;
        if (i < S && frame_ok) {
            const double wx = src[i * 3], wy = src[i * 3 + 1], wh = src[i * 3 + 2];
            const double c = cos(wh), s = sin(wh);
            x = (float)(m[0] * wx + m[1] * wy + m[2]);
            y = (float)(m[3] * wx + m[4] * wy + m[5]);
            h = (float)atan2(m[3] * c + m[4] * s, m[0] * c + m[1] * s);
        }
        if (i < S) { px[i] = x; py[i] = y; ph[i] = h; }
        key[i] = i < S ? sort_key(x, i) : ~0ull;                         // the padding of the network sorts behind every point
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += kThreads) {
                const int q = i ^ j;
                if (q > i) {
                    const unsigned long long a = key[i], b = key[q];
                    if ((a > b) == ((i & k) == 0)) { key[i] = b; key[q] = a; }
                }
            }
            __syncthreads();
        }
    }
    float* dst = p.lines + (size_t)ln * S * 3;
    for (int r = threadIdx.x; r < S; r += kThreads) {
        const int i = (int)(unsigned int)(key[r] & 0xFFFFFFFFull);       // < S: the S smallest keys are the points'
        const bool ok = (unsigned)i < (unsigned)S;
        dst[r * 3] = ok ? px[i] : nanf_; dst[r * 3 + 1] = ok ? py[i] : nanf_; dst[r * 3 + 2] = ok ? ph[i] : nanf_;
    }
}

// w_t of the decayed form: decay^t / sum_u decay^u / 52 (the powers by repeated multiplication, the sum in ascending u)
__device__ __forceinline__ float decayed_weight(float decay, int t) {
    float w = 1.f, sum = 0.f, wt = 0.f;
    for (int u = 0; u < TT; ++u) {
        sum += w;
        if (u == t) wt = w;
        w *= decay;
    }
    return wt / sum / (float)TT;
}

__global__ __launch_bounds__(kThreads) void lane_kernel(const LaneArgs p) {
    __shared__ float4 seg[kLaneMaxPts];                                  // (p0.x, p0.y, d.x, d.y) of segment j
    __shared__ float sinv[kLaneMaxPts];                                  // 1 / |d|^2, NaN: not a segment
    __shared__ float shead[kLaneMaxPts];                                 // heading of p0
    __shared__ float red_d[kWaves][64], red_x[kWaves][64], red_y[kWaves][64];
    __shared__ int red_j[kWaves][64];
    __shared__ int wave_last[kWaves];
    const int A = p.rows / p.num_samp, S = p.max_pts;
    const int e0 = blockIdx.x / p.num_samp, n = blockIdx.x - e0 * p.num_samp;
    const int a = p.agent[e0];
    if (e0 > 0 && p.agent[e0 - 1] == a) return;                          // not the first entry of its agent's run
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = lane;
    const bool agent_ok = (unsigned)a < (unsigned)A;
    const bool step = t < TT;
    const float nanf_ = __builtin_nanf("");
    float qx = 0.f, qy = 0.f, qh = 0.f;
    if (agent_ok && step) {
        const float* q = p.traj + (((size_t)a * p.num_samp + n) * TT + t) * 6;
        qx = q[0]; qy = q[1]; qh = q[3];
    }
    float gx = 0.f, gy = 0.f, gh = 0.f;                                  // wave 0: the run's gradient of (agent, sample, step t)
    for (int e = e0; e < p.num_entries && p.agent[e] == a; ++e) {
        const int ln = p.line[e];
        const bool line_ok = agent_ok && (unsigned)ln < (unsigned)p.num_lines;
        int nseg = 0;
        __syncthreads();                                                 // the previous entry's reads of LDS are over
        if (line_ok) {
            const float* L = p.lines + (size_t)ln * S * 3;
            int last = 0;
            for (int j = threadIdx.x; j < S - 1; j += kThreads) {
                const float x0 = L[j * 3], y0 = L[j * 3 + 1], x1 = L[j * 3 + 3], y1 = L[j * 3 + 4];
                const float dx = x1 - x0, dy = y1 - y0;
                const float nn = __fmaf_rn(dx, dx, dy * dy);
                const bool ok = nn > 0.f && nn < __builtin_inff();       // (false for NaN)
                seg[j] = make_float4(x0, y0, dx, dy);
                sinv[j] = ok ? 1.0f / nn : nanf_;
                shead[j] = L[j * 3 + 2];
                if (ok) last = j + 1;
            }
            for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o));
            if (lane == 0) wave_last[wv] = last;
            __syncthreads();
            for (int w = 0; w < kWaves; ++w) nseg = max(nseg, wave_last[w]);
        }
        if (nseg == 0) {                                                 // (block-uniform) not evaluated
            if (p.value && threadIdx.x == 0) p.value[(size_t)e * p.num_samp + n] = nanf_;
            if (p.proj && wv == 0 && step) {
                float* o = p.proj + (((size_t)e * p.num_samp + n) * TT + t) * 3;
                o[0] = nanf_; o[1] = nanf_; o[2] = nanf_;
            }
            continue;
        }
        float best = __builtin_inff(), bx = nanf_, by = nanf_;
        int bj = -1;
        for (int j = wv; j < nseg; j += kWaves) {                        // (j is wave-uniform: every read below is a broadcast)
            const float inv = sinv[j];
            if (inv != inv) continue;
            const float4 sg = seg[j];
            const float rx = qx - sg.x, ry = qy - sg.y;
            float u = __fmaf_rn(rx, sg.z, ry * sg.w) * inv;
            u = fminf(fmaxf(u, 0.f), 1.f);
            const float cx = __fmaf_rn(u, sg.z, sg.x), cy = __fmaf_rn(u, sg.w, sg.y);
            const float ex = qx - cx, ey = qy - cy;
            const float d2 = __fmaf_rn(ex, ex, ey * ey);
            if (d2 < best) { best = d2; bj = j; bx = cx; by = cy; }
        }
        red_d[wv][lane] = best; red_j[wv][lane] = bj; red_x[wv][lane] = bx; red_y[wv][lane] = by;
        __syncthreads();
        if (wv != 0) continue;                                           // (the loop's next barrier is the one at its top)
        for (int w = 1; w < kWaves; ++w) {
            const float d = red_d[w][lane];
            const int j = red_j[w][lane];
            if (j >= 0 && (bj < 0 || d < best || (d == best && j < bj))) { best = d; bj = j; bx = red_x[w][lane]; by = red_y[w][lane]; }
        }
        const float hd = bj >= 0 ? shead[bj] : nanf_;
        if (p.proj && step) {
            float* o = p.proj + (((size_t)e * p.num_samp + n) * TT + t) * 3;
            o[0] = bx; o[1] = by; o[2] = hd;
        }
        const float dx = qx - bx, dy = qy - by, dh = qh - hd;
        const int kind = p.kind[e];
        const float sc = p.scale[e];
        float v = 0.f;
        if (step) {
            if (kind == LANE_FOLLOWING) {
                const float w = 1.0f / (float)TT;
                v = (__fmaf_rn(dx, dx, dy * dy) + dh * dh) * w;
                const float c = 2.f * w * sc;
                gx += c * dx; gy += c * dy; gh += c * dh;
            } else if (kind == LANE_CHANGE_LEFT) {
                const float w = 1.0f / (float)TT;
                const float d = sqrtf(__fmaf_rn(dx, dx, dy * dy));
                v = (d + fabsf(dh)) * w;
                const float s = d > 0.f ? w * sc / d : 0.f;
                gx += s * dx; gy += s * dy;
                gh += dh > 0.f ? w * sc : (dh < 0.f ? -(w * sc) : 0.f * dh);
            } else {                                                     // LANE_FOLLOW_DECAYED
                const float w = decayed_weight(p.decay[e], t);
                const float m = fabsf(dx) + fabsf(dy);
                v = fminf(m, 5.f) * w;
                if (m != m) v = m;                                       // (fminf drops a NaN)
                const float c = m <= 5.f ? w * sc : (m != m ? m : 0.f);
                gx += dx > 0.f ? c : (dx < 0.f ? -c : 0.f * dx);
                gy += dy > 0.f ? c : (dy < 0.f ? -c : 0.f * dy);
            }
        }
        if (p.value) {
            float s = 0.f;
            for (int u = 0; u < TT; ++u) s += __shfl(v, u);              // ascending t; every lane forms the same sum
            if (lane == 0) p.value[(size_t)e * p.num_samp + n] = s;
        }
    }
    if (p.grad && wv == 0 && step && agent_ok) {
        float* o = p.grad + (((size_t)a * p.num_samp + n) * TT + t) * 6; // holds grad_in (or 0) already: launch_lane
        o[0] += gx; o[1] += gy; o[3] += gh;
    }
}
}  // namespace

hipError_t launch_lane_prepare(const LanePrepareArgs& a, hipStream_t s) {
    if (a.num_lines < 1 || a.max_pts < 1 || a.max_pts > kLaneMaxPts || a.num_frames < 1) return hipErrorInvalidValue;
    int n2 = 1;
    while (n2 < a.max_pts) n2 <<= 1;
    hipLaunchKernelGGL(lane_prepare_kernel, dim3((unsigned)a.num_lines), dim3(kThreads), 0, s, a, n2);
    return hipGetLastError();
}

hipError_t launch_lane(const LaneArgs& a, const float* grad_in, hipStream_t s) {
    if (a.rows < 1 || a.num_samp < 1 || a.rows % a.num_samp || a.num_entries < 1 || a.num_lines < 1 || a.max_pts < 2 || a.max_pts > kLaneMaxPts ||
        (!a.value && !a.grad && !a.proj))
        return hipErrorInvalidValue;
    const long long blocks = (long long)a.num_entries * a.num_samp;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    if (const hipError_t e = seed_grad(a.grad, grad_in, a.rows, s); e != hipSuccess) return e;      // rows without an entry: the gradient of grad_in (or 0)
    hipLaunchKernelGGL(lane_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace cld
