// sample_metrics_kernels.hip -- the open-loop sample metrics of N sampled futures per agent against the logged future: ADE / FDE
// (mean and best sample) and the pairwise diversity of the samples (include/cld_eval.h `cld_sample_metrics` for the definitions;
// upstream: src/tbsim/utils/metrics.py:201-358 as DiffuserTrafficModel._compute_metrics calls them, src/tbsim/algos/algos.py:1818-1852).
//
// One workgroup of 256 lanes per agent (agents beyond kSmMaxBlocks in further grid-stride passes).  The agent's N x T positions are
// staged once in LDS as two fp32 planes, TIME-major: plane[t * N + n].  In the pair loop every lane holds a pair (i, j) and all lanes
// read the same t, so the addresses of a wave differ in the sample index alone: consecutive lanes hold consecutive j of one i, that
// is consecutive banks for j and one broadcast address for i; lanes collide only where two sample indices of a 32-lane group differ
// by a multiple of 32.  (Sample-major, plane[n * T + t], puts T = 52 between neighbours: 52 mod 32 = 20 reaches 8 of the 32 banks,
// a 4-way conflict on every read.)  The price is the staging store, whose lanes follow the global layout (consecutive t) and are
// N words apart; it runs once per agent, the reads T times per pair.
//
// Inputs are fp32; every difference, square, square root and sum is fp64 (a difference of two fp32 values is exact in fp64).  Sums over
// t run in one lane in ascending t.  Sums, maxima and minima over samples and pairs: every lane folds its own items in ascending order
// (pair p = lane + 256 k), a wave folds its lanes by a shuffle tree (offsets 32 ... 1) and lane 0 of the workgroup the four waves as
// (w0 + w1) + (w2 + w3): nothing of that depends on the grid or on B, and there are no atomics, so a row has the same bits wherever
// and whenever it is computed.
#include <hip/hip_runtime.h>

#include <cmath>

#include "cld_kernels.h"
#include "sample_metrics_kernels.h"

namespace cld {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
// cld_eval.h CLD_SM_*
enum { SM_ADE_MEAN = 0, SM_ADE_MIN, SM_FDE_MEAN, SM_FDE_MIN, SM_APD_MEAN, SM_APD_MAX, SM_FPD_MEAN, SM_FPD_MAX, SM_LAST_PD_MEAN, SM_LAST_PD_MAX };
static_assert(SM_LAST_PD_MAX + 1 == kSmCols, "the columns of a per-agent row");
// slots of the cross-wave scratch: the six pair quantities, then the displacement half
enum { R_APD_SUM = 0, R_APD_MAX, R_FPD_SUM, R_FPD_MAX, R_LPD_SUM, R_LPD_MAX, R_ADE_SUM, R_ADE_MIN, R_FDE_SUM, R_FDE_MIN, R_SLOTS };
enum { I_ADE_ARG = 0, I_FDE_ARG, I_BAD, I_LAST, I_SLOTS };

__device__ inline bool finite32(float x) { return fabsf(x) < INFINITY; }

__device__ inline double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                                             // lane 0 holds the wave's sum
}
__device__ inline double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    return v;
}
__device__ inline int wave_max(int v) {
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_down(v, off, 64));
    return v;
}
// the lexicographic minimum of (value, index): the first index among equal values
__device__ inline void take_min(double& v, int& i, double v2, int i2) {
    if (v2 < v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}
__device__ inline void wave_argmin(double& v, int& i) {
    for (int off = 32; off > 0; off >>= 1) {
        const double v2 = __shfl_down(v, off, 64);
        const int i2 = __shfl_down(i, off, 64);
        take_min(v, i, v2, i2);
    }
}
__device__ inline double fold4(const double* r) { return (r[0] + r[1]) + (r[2] + r[3]); }
__device__ inline double max4(const double* r) { return fmax(fmax(r[0], r[1]), fmax(r[2], r[3])); }

// pairs (i, j = i + 1 + r), i < j < N, in row-major order: move `step` pairs on (i stops at N - 1, past the last pair)
__device__ inline void pair_advance(int& i, int& r, int step, int N) {
    r += step;
    while (i < N - 1 && r >= N - 1 - i) {
        r -= N - 1 - i;
        ++i;
    }
}

__global__ __launch_bounds__(kThreads) void sample_metrics_kernel(SampleMetricsArgs a) {
    extern __shared__ float planes[];                      // [2][T][N]
    __shared__ double red[R_SLOTS][kWaves];
    __shared__ int redi[I_SLOTS][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, T = a.T, C = a.C, NT = N * T;
    float* px = planes;
    float* py = planes + NT;
    const int total_pairs = N * (N - 1) / 2;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        // ---- stage the positions, time-major; the agent's non-finite flag and last available step on the way
        const float* pred = a.pred + (size_t)b * NT * C;
        const float* gt = a.gt + (size_t)b * T * 2;
        const float* avail = a.avail + (size_t)b * T;
        int bad = 0, last = 0;
        for (int k = tid; k < NT; k += kThreads) {
            const int n = k / T, t = k - n * T;
            const float x = pred[(size_t)k * C], y = pred[(size_t)k * C + 1];
            px[t * N + n] = x;
            py[t * N + n] = y;
            bad |= !(finite32(x) && finite32(y));
        }
        for (int t = tid; t < T; t += kThreads) {
            const float av = avail[t];
            bad |= !(finite32(gt[2 * t]) && finite32(gt[2 * t + 1]) && finite32(av));
            if (av > 0.f) last = t;                       // ascending t: the lane's largest
        }
        bad = __any(bad) ? 1 : 0;
        last = wave_max(last);
        if (lane == 0) {
            redi[I_BAD][wave] = bad;
            redi[I_LAST][wave] = last;
        }
        __syncthreads();
        last = max(max(redi[I_LAST][0], redi[I_LAST][1]), max(redi[I_LAST][2], redi[I_LAST][3]));

        // ---- displacement half: lane n owns sample n
        {
            double ade = 0.0, fde = 0.0, ade_m = INFINITY, fde_m = INFINITY;
            int ade_i = 0x7fffffff, fde_i = 0x7fffffff;
            if (tid < N) {
                double sum = 0.0;
                for (int t = 0; t < T; ++t) {
                    const double av = (double)avail[t];
                    const double ex = ((double)gt[2 * t] - (double)px[t * N + tid]) * av;
                    const double ey = ((double)gt[2 * t + 1] - (double)py[t * N + tid]) * av;
                    const double e = sqrt(ex * ex + ey * ey);
                    sum += e;
                    if (t == last) fde = e;
                }
                ade = sum / (double)T;
                ade_m = ade; fde_m = fde;
                ade_i = fde_i = tid;
            }
            ade = wave_sum(ade);
            fde = wave_sum(fde);
            wave_argmin(ade_m, ade_i);
            wave_argmin(fde_m, fde_i);
            if (lane == 0) {
                red[R_ADE_SUM][wave] = ade; red[R_ADE_MIN][wave] = ade_m; redi[I_ADE_ARG][wave] = ade_i;
                red[R_FDE_SUM][wave] = fde; red[R_FDE_MIN][wave] = fde_m; redi[I_FDE_ARG][wave] = fde_i;
            }
        }

        // ---- diversity half: lanes stride over the pairs i < j
        {
            double apd_s = 0.0, apd_m = 0.0, fpd_s = 0.0, fpd_m = 0.0, lpd_s = 0.0, lpd_m = 0.0;
            int i = 0, r = 0;
            pair_advance(i, r, tid, N);
            for (int p = tid; p < total_pairs; p += kThreads) {
                const int j = i + 1 + r;
                double sd = 0.0, f2 = 0.0, l2 = 0.0;
                const float* qx = px;
                const float* qy = py;
                for (int t = 0; t < T; ++t, qx += N, qy += N) {
                    const double dx = (double)qx[i] - (double)qx[j];
                    const double dy = (double)qy[i] - (double)qy[j];
                    l2 = dx * dx + dy * dy;                // the last step's stays
                    sd += sqrt(l2);
                    f2 += dy * dy;
                }
                const double d = sd / (double)T, f = sqrt(f2), l = sqrt(l2);
                apd_s += d; apd_m = fmax(apd_m, d);
                fpd_s += f; fpd_m = fmax(fpd_m, f);
                lpd_s += l; lpd_m = fmax(lpd_m, l);
                pair_advance(i, r, kThreads, N);
            }
            apd_s = wave_sum(apd_s); apd_m = wave_max(apd_m);
            fpd_s = wave_sum(fpd_s); fpd_m = wave_max(fpd_m);
            lpd_s = wave_sum(lpd_s); lpd_m = wave_max(lpd_m);
            if (lane == 0) {
                red[R_APD_SUM][wave] = apd_s; red[R_APD_MAX][wave] = apd_m;
                red[R_FPD_SUM][wave] = fpd_s; red[R_FPD_MAX][wave] = fpd_m;
                red[R_LPD_SUM][wave] = lpd_s; red[R_LPD_MAX][wave] = lpd_m;
            }
        }
        __syncthreads();
        if (tid == 0) {
            double* row = a.per_agent + (size_t)b * kSmCols;
            int* idx = a.index + (size_t)b * 4;
            const double n = (double)N, nn = n * n;
            double am = red[R_ADE_MIN][0], fm = red[R_FDE_MIN][0];
            int ai = redi[I_ADE_ARG][0], fi = redi[I_FDE_ARG][0];
            for (int w = 1; w < kWaves; ++w) {
                take_min(am, ai, red[R_ADE_MIN][w], redi[I_ADE_ARG][w]);
                take_min(fm, fi, red[R_FDE_MIN][w], redi[I_FDE_ARG][w]);
            }
            row[SM_ADE_MEAN] = fold4(red[R_ADE_SUM]) / n;
            row[SM_ADE_MIN] = am;
            row[SM_FDE_MEAN] = fold4(red[R_FDE_SUM]) / n;
            row[SM_FDE_MIN] = fm;
            // the mean over all N N entries of the symmetric matrix with a zero diagonal
            row[SM_APD_MEAN] = 2.0 * fold4(red[R_APD_SUM]) / nn;
            row[SM_APD_MAX] = max4(red[R_APD_MAX]);
            row[SM_FPD_MEAN] = 2.0 * fold4(red[R_FPD_SUM]) / nn;
            row[SM_FPD_MAX] = max4(red[R_FPD_MAX]);
            row[SM_LAST_PD_MEAN] = 2.0 * fold4(red[R_LPD_SUM]) / nn;
            row[SM_LAST_PD_MAX] = max4(red[R_LPD_MAX]);
            idx[0] = ai < N ? ai : 0;                      // a NaN in every sample leaves no minimum: the flag below says so
            idx[1] = fi < N ? fi : 0;
            idx[2] = last;
            idx[3] = redi[I_BAD][0] | redi[I_BAD][1] | redi[I_BAD][2] | redi[I_BAD][3];
        }
        __syncthreads();                                   // the scratch and the planes are free for the next agent
    }
}

// dst[w] = (the sum of rows [w chunk, (w + 1) chunk) of src) / denom, column by column: a lane adds its rows (lane, lane + 256, ...) in
// ascending order, then the tree of the kernel above.  chunk = kSmFoldTile over the per-agent rows gives the partials, chunk = all
// of the partials in one workgroup the batch mean: which workgroup computes a partial does not enter.
__global__ __launch_bounds__(kThreads) void sample_metrics_fold_kernel(const double* __restrict__ src, int rows, int chunk, double denom,
                                                                        double* __restrict__ dst) {
    __shared__ double red[kSmCols][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long w = blockIdx.x; w * chunk < rows; w += gridDim.x) {
        const long long r0 = w * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
        double acc[kSmCols];
        for (int c = 0; c < kSmCols; ++c) acc[c] = 0.0;
        for (long long r = r0 + tid; r < r1; r += kThreads)
            for (int c = 0; c < kSmCols; ++c) acc[c] += src[r * kSmCols + c];
        for (int c = 0; c < kSmCols; ++c) {
            const double v = wave_sum(acc[c]);
            if (lane == 0) red[c][wave] = v;
        }
        __syncthreads();
        if (tid < kSmCols) dst[w * kSmCols + tid] = fold4(red[tid]) / denom;
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_sample_metrics(const SampleMetricsArgs& a, double* means, double* ws, hipStream_t s) {
    static unsigned long long attr_done = 0;               // one bit per device
    const size_t lds_bytes = sizeof(float) * 2 * (size_t)a.N * a.T;
    if (a.N < 1 || a.T < 1 || a.N > kSmMaxN || (long long)a.N * a.T > kSmMaxNT || a.B < 1 || a.B > kSmMaxB) return hipErrorInvalidValue;
    if (hipError_t e = set_max_lds_once(reinterpret_cast<const void*>(sample_metrics_kernel), sizeof(float) * 2 * kSmMaxNT, &attr_done); e != hipSuccess)
        return e;
    const unsigned int blocks = (unsigned int)(a.B < kSmMaxBlocks ? a.B : kSmMaxBlocks);
    hipLaunchKernelGGL(sample_metrics_kernel, dim3(blocks), dim3(kThreads), lds_bytes, s, a);
    if (means) {
        const int tiles = (int)sm_fold_tiles(a.B);
        const unsigned int fb = (unsigned int)(tiles < kSmMaxBlocks ? tiles : kSmMaxBlocks);
        hipLaunchKernelGGL(sample_metrics_fold_kernel, dim3(fb), dim3(kThreads), 0, s, a.per_agent, a.B, kSmFoldTile, 1.0, ws);
        hipLaunchKernelGGL(sample_metrics_fold_kernel, dim3(1), dim3(kThreads), 0, s, ws, tiles, tiles, (double)a.B, means);
    }
    return hipGetLastError();
}

}  // namespace cld
