// realism_kernels.hip -- the realism deviation of the reference's test stage on the device (src/trainers/guide_dm_trainer.py:204-295):
// the three compared quantities of a batch of trajectories, an ascending sort of fp32 values and the 1-D Wasserstein-1 distance of two
// sorted samples (include/cld.h `cld_realism_terms`, `cld_sort_f32`, `cld_wasserstein_f32` for the definitions).
//
// realism_terms_kernel: one thread per (agent, step); a copy, one fp32 product, and one fp32 difference divided by dt (the IEEE division:
// the build has no fast-math, and nothing here may contract).
//
// The sort is an LSD radix sort, four passes of 8 bits over the monotone uint32 image of the key (sign flip for positives, complement
// for negatives, every NaN -> 0xffffffff).  A pass is three launches over tiles of SORT_TILE keys: sort_hist_kernel counts the digits of
// every tile into hist[digit][tile]; sort_scan_kernel (one workgroup per digit) turns each row into its exclusive scan and leaves the
// row totals; sort_scatter_kernel ranks every key of a tile among the tile's keys of the same digit -- per wave with eight ballots (the
// lanes holding the same digit), the wave's running count per digit in LDS (an integer LDS add by one lane of the group, only ever from
// that wave), then a prefix over the four waves -- stages the tile in digit order in LDS and writes it out in runs.  A key's rank
// counts the keys of its digit in earlier tiles, earlier waves, earlier rounds and lower lanes: the order of the input, so every pass is
// stable and the output is a function of the input values alone.  Passes ping-pong between the workspace and `out`; the first reads
// `in`, so out == in is allowed.
//
// The distance: equal sizes sum |u_i - v_i|; unequal sizes walk the merged sequence (merge path: every thread finds its start by a
// binary search on the diagonal, then merges eight steps) and sum |cu nv - cv nu| (a' - a) over consecutive merged values a < a', cu and cv
// the counts of values <= a -- inclusive counts at the last element of a run, so ties inside and across the samples contribute as
// scipy's right-continuous CDFs do.  fp64 partial per thread in a fixed order, a fixed LDS tree per workgroup, one partial per workgroup
// in the workspace, and one workgroup folds those in a fixed order: the same bits on every run.  No float atomics anywhere.
#include "cld_kernels.h"

namespace cld {

namespace {
__host__ __device__ inline long long lmin(long long a, long long b) { return a < b ? a : b; }
__host__ __device__ inline long long lmax(long long a, long long b) { return a > b ? a : b; }
constexpr int kThreads = 256;
constexpr int kSortItems = SORT_TILE / kThreads;      // keys per thread of a tile
constexpr int kWaveItems = 64 * kSortItems;           // keys per wave of a tile
constexpr int kW1Items = W1_TILE / kThreads;
static_assert(SORT_TILE % kThreads == 0 && W1_TILE % kThreads == 0, "tiles are whole rounds of the workgroup");

__global__ __launch_bounds__(kThreads) void realism_terms_kernel(const float* __restrict__ sa, long long M, int T, float dt, float* lon,
                                                                 float* lat, float* jerk) {
    const long long total = M * (long long)T;
    for (long long idx = (long long)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (long long)gridDim.x * kThreads) {
        const float* r = sa + idx * 6;
        const float a = r[4];
        if (lon) lon[idx] = a;
        if (lat) lat[idx] = __fmul_rn(r[2], r[5]);
        const int t = (int)(idx % T);
        if (jerk && t + 1 < T) jerk[idx - idx / T] = __fsub_rn(r[10], a) / dt;          // row m of jerk starts at m (T - 1) = m T - m
    }
}

// ---- sort ----
__device__ inline unsigned int to_key(unsigned int u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;                         // every NaN, of either sign, sorts last
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ inline unsigned int from_key(unsigned int k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// inclusive scan of v over the workgroup's 256 threads; *total = the sum.  wsum: 4 words of LDS, free again on return.
__device__ inline unsigned int block_scan_incl(unsigned int v, unsigned int* wsum, unsigned int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    unsigned int pre = 0u, tot = 0u;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) {
        const unsigned int s = wsum[i];
        if (i < w) pre += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return v + pre;
}

template <bool FIRST>
__global__ __launch_bounds__(kThreads) void sort_hist_kernel(const unsigned int* __restrict__ in, long long n, int shift,
                                                             unsigned int* __restrict__ hist, long long nb) {
    __shared__ unsigned int h[256];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * SORT_TILE;
    const int cnt = (int)lmin((long long)SORT_TILE, n - base);
    h[tid] = 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const int i = j * kThreads + tid;
        if (i < cnt) {
            unsigned int k = in[base + i];
            if (FIRST) k = to_key(k);
            atomicAdd(&h[(k >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    hist[(long long)tid * nb + blockIdx.x] = h[tid];
}

// workgroup d: hist[d][0 .. nb) -> its exclusive scan, tot[d] = the row's sum
__global__ __launch_bounds__(kThreads) void sort_scan_kernel(unsigned int* __restrict__ hist, long long nb, unsigned int* __restrict__ tot) {
    __shared__ unsigned int wsum[kThreads / 64];
    unsigned int* row = hist + (long long)blockIdx.x * nb;
    unsigned int carry = 0u;
    for (long long base = 0; base < nb; base += kThreads) {
        const long long i = base + threadIdx.x;
        const unsigned int v = i < nb ? row[i] : 0u;
        unsigned int total;
        const unsigned int incl = block_scan_incl(v, wsum, &total);
        if (i < nb) row[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kThreads) void sort_scatter_kernel(const unsigned int* __restrict__ in, unsigned int* __restrict__ out, long long n,
                                                                int shift, const unsigned int* __restrict__ hist, long long nb,
                                                                const unsigned int* __restrict__ tot) {
    __shared__ unsigned int wave_hist[kThreads / 64][256];
    __shared__ unsigned int staged[SORT_TILE];
    __shared__ unsigned int lstart[256], gbase[256], wsum[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long base = (long long)blockIdx.x * SORT_TILE;
    const int cnt = (int)lmin((long long)SORT_TILE, n - base);
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) wave_hist[i][tid] = 0u;
    __syncthreads();
    unsigned int key[kSortItems], rank[kSortItems];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < kSortItems; ++k) {
        const int i = w * kWaveItems + k * 64 + lane;                   // the tile in memory order: wave, round, lane
        const bool valid = i < cnt;
        unsigned int x = valid ? in[base + i] : 0xffffffffu;
        if (FIRST && valid) x = to_key(x);
        key[k] = x;
        const unsigned int d = (x >> shift) & 255u;
        unsigned long long peers = __ballot(valid);                      // the valid lanes of this round holding digit d
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        const int leader = peers ? __ffsll((long long)peers) - 1 : 0;
        unsigned int old = 0u;
        if (valid && lane == leader) old = atomicAdd(&wave_hist[w][d], (unsigned int)__popcll(peers));     // this wave's own row only
        old = __shfl(old, leader);
        rank[k] = old + (unsigned int)__popcll(peers & below);
    }
    __syncthreads();
    // thread d: the waves' counts of digit d -> their exclusive prefix; the tile's count of d -> where d starts in the staged tile
    unsigned int run = 0u;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) {
        const unsigned int t = wave_hist[i][tid];
        wave_hist[i][tid] = run;
        run += t;
    }
    unsigned int total;
    const unsigned int ls = block_scan_incl(run, wsum, &total) - run;
    const unsigned int dtot = tot[tid];
    const unsigned int dpre = block_scan_incl(dtot, wsum, &total) - dtot;     // the keys of lower digits in the whole array
    lstart[tid] = ls;
    gbase[tid] = dpre + hist[(long long)tid * nb + blockIdx.x] - ls;      // + position in the staged tile = position in `out` (mod 2^32)
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSortItems; ++k) {
        const int i = w * kWaveItems + k * 64 + lane;
        if (i < cnt) {
            const unsigned int d = (key[k] >> shift) & 255u;
            staged[lstart[d] + wave_hist[w][d] + rank[k]] = key[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const int i = j * kThreads + tid;
        if (i < cnt) {
            const unsigned int x = staged[i];
            const unsigned int dst = gbase[(x >> shift) & 255u] + (unsigned int)i;
            out[dst] = LAST ? from_key(x) : x;
        }
    }
}

// ---- Wasserstein-1 ----
// the workgroup's sum of v in a fixed tree; valid in thread 0
__device__ inline double block_sum(double v, double* part) {
    const int tid = threadIdx.x;
    part[tid] = v;
    __syncthreads();
    for (int s = kThreads >> 1; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    return part[0];
}

__global__ __launch_bounds__(kThreads) void w1_paired_kernel(const float* __restrict__ u, const float* __restrict__ v, long long n,
                                                             double* __restrict__ partial) {
    __shared__ double part[kThreads];
    const long long base = (long long)blockIdx.x * W1_TILE;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kW1Items; ++j) {
        const long long i = base + j * kThreads + threadIdx.x;
        if (i < n) acc += fabs((double)u[i] - (double)v[i]);
    }
    const double s = block_sum(acc, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// the order both samples are sorted in, as an integer: NaN last, -0 = +0
__device__ inline unsigned int order_key(float x) {
    unsigned int u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;
    return to_key(u);
}

__global__ __launch_bounds__(kThreads) void w1_cdf_kernel(const float* __restrict__ u, const float* __restrict__ v, long long nu, long long nv,
                                                          double* __restrict__ partial) {
    __shared__ double part[kThreads];
    const long long pairs = nu + nv - 1;                                // consecutive pairs (k, k + 1) of the merged sequence
    const long long k0 = (long long)blockIdx.x * W1_TILE + (long long)threadIdx.x * kW1Items;
    double acc = 0.0;
    if (k0 < pairs) {
        const long long k1 = lmin(k0 + kW1Items, pairs);
        // i = how many of the first k0 merged values come from u (ties take u first)
        long long lo = lmax(0ll, k0 - nv), hi = lmin(k0, nu);
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (order_key(u[mid]) <= order_key(v[k0 - mid - 1])) lo = mid + 1;
            else hi = mid;
        }
        long long i = lo, j = k0 - lo;
        float a;                                                        // merged value k0
        if (j >= nv || (i < nu && order_key(u[i]) <= order_key(v[j]))) a = u[i++];
        else a = v[j++];
        for (long long k = k0; k < k1; ++k) {                           // k <= nu + nv - 2: value k + 1 exists
            const long long cu = i, cv = j;                             // values <= a when the next one is greater
            float nx;
            if (j >= nv || (i < nu && order_key(u[i]) <= order_key(v[j]))) nx = u[i++];
            else nx = v[j++];
            const double delta = (double)nx - (double)a;
            if (!(delta == 0.0)) acc += fabs((double)(cu * nv - cv * nu)) * delta;       // NaN and inf - inf go through
            a = nx;
        }
    }
    const double s = block_sum(acc, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one workgroup: the partials in a fixed order, divided once
__global__ __launch_bounds__(kThreads) void w1_fold_kernel(const double* __restrict__ partial, long long np, double denom, double* out) {
    __shared__ double part[kThreads];
    double acc = 0.0;
    for (long long i = threadIdx.x; i < np; i += kThreads) acc += partial[i];
    const double s = block_sum(acc, part);
    if (threadIdx.x == 0) *out = s / denom;
}
}  // namespace

hipError_t launch_realism_terms(const float* sa, int64_t M, int T, float dt, float* lon, float* lat, float* jerk, hipStream_t s) {
    const long long total = (long long)M * T;
    const unsigned int blocks = (unsigned int)lmin((total + kThreads - 1) / kThreads, 1ll << 20);
    hipLaunchKernelGGL(realism_terms_kernel, dim3(blocks), dim3(kThreads), 0, s, sa, (long long)M, T, dt, lon, lat, jerk);
    return hipGetLastError();
}

hipError_t launch_sort_f32(const float* in, float* out, int64_t n, void* ws, hipStream_t s) {
    const long long nb = sort_tiles(n);
    unsigned int* tmp = static_cast<unsigned int*>(ws);
    unsigned int* hist = reinterpret_cast<unsigned int*>(static_cast<char*>(ws) + sort_tmp_bytes(n));
    unsigned int* tot = hist + 256 * nb;
    const unsigned int* src = reinterpret_cast<const unsigned int*>(in);
    unsigned int* o = reinterpret_cast<unsigned int*>(out);
    const dim3 grid((unsigned int)nb), block(kThreads);
    // in -> tmp -> out -> tmp -> out
    hipLaunchKernelGGL(sort_hist_kernel<true>, grid, block, 0, s, src, (long long)n, 0, hist, nb);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(256), block, 0, s, hist, nb, tot);
    hipLaunchKernelGGL((sort_scatter_kernel<true, false>), grid, block, 0, s, src, tmp, (long long)n, 0, hist, nb, tot);
    for (int pass = 1; pass < 4; ++pass) {
        const unsigned int* a = pass == 2 ? o : tmp;
        unsigned int* b = pass == 2 ? tmp : o;
        hipLaunchKernelGGL(sort_hist_kernel<false>, grid, block, 0, s, a, (long long)n, 8 * pass, hist, nb);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(256), block, 0, s, hist, nb, tot);
        if (pass < 3) hipLaunchKernelGGL((sort_scatter_kernel<false, false>), grid, block, 0, s, a, b, (long long)n, 8 * pass, hist, nb, tot);
        else hipLaunchKernelGGL((sort_scatter_kernel<false, true>), grid, block, 0, s, a, b, (long long)n, 8 * pass, hist, nb, tot);
    }
    return hipGetLastError();
}

hipError_t launch_wasserstein_f32(const float* u, int64_t nu, const float* v, int64_t nv, double* out, void* ws, hipStream_t s) {
    double* partial = static_cast<double*>(ws);
    const long long np = w1_tiles(nu, nv);
    if (nu == nv) {
        hipLaunchKernelGGL(w1_paired_kernel, dim3((unsigned int)np), dim3(kThreads), 0, s, u, v, (long long)nu, partial);
        hipLaunchKernelGGL(w1_fold_kernel, dim3(1), dim3(kThreads), 0, s, partial, np, (double)nu, out);
    } else {
        hipLaunchKernelGGL(w1_cdf_kernel, dim3((unsigned int)np), dim3(kThreads), 0, s, u, v, (long long)nu, (long long)nv, partial);
        hipLaunchKernelGGL(w1_fold_kernel, dim3(1), dim3(kThreads), 0, s, partial, np, (double)nu * (double)nv, out);
    }
    return hipGetLastError();
}

}  // namespace cld
