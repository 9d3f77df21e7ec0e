// train_kernels.hip -- exact-fp32 training path of the U-Net: a forward that reads the raw weights from a device buffer and keeps a
// tape, and its backward (data and weight gradients of all 148 tensors).  Every convolution, transposed convolution and Linear runs on
// two implicit-GEMM kernels on v_mfma_f32_16x16x4_f32 (direct form, no Winograd):
//   conv_gemm_kernel   out[b, lo, n] (+)= bias[n] + sum_{tap, c} in[b, li(lo, tap), c] * Wp[tap * C + c][n]
//                      li = lo s + tap - p (mode 0: Conv1d forward, ConvTranspose1d data gradient) or
//                      li = (lo + p - tap) / s when that divides (mode 1: Conv1d data gradient, ConvTranspose1d forward);
//                      Wp is the weight packed [K][N] by pack_kernel (a different packing for the forward and the data gradient).
//   wgrad_kernel       part[z][m][n] = sum over the rows of K-split chunk z, l of P[b, l, m] * G[b, l s + tap - p, c] (n = tap C + c),
//                      plus a column of ones (n = N - 1) that gives the bias gradient sum_{b, l} P[b, l, m];
//   wreduce_kernel     sums the chunks in a fixed order into the reference layout: no float atomics, bit-reproducible run to run.
// GroupNorm + Mish forward / backward are fused per (row, group).  Activations are channels-last [B, L, C] like the inference path.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "train.h"

namespace cld {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int BM = 64, BN = 64, BK = 16, LDS_LD = 80;   // LDS rows of 80 floats: the four 16-lane groups of an MFMA operand read
                                                         // land on four disjoint bank ranges
constexpr int NACC = BK / 4;                             // one accumulator set per k-step of a K tile, summed pairwise at the end: the
                                                         // fma chain of each set is a quarter of K long (rounding of the sums ~ sqrt(K / 4))
constexpr int kChunks = 32;                              // K-split of the weight gradients: at most this many row chunks
constexpr int kCat = 6656;                               // widest activation per row: the skip concatenations 13 x 512 / 26 x 256
constexpr int kAct = 3328;                               // 52 x 64 = 26 x 128 = 13 x 256
constexpr int kPart = 256 * (256 * 5 + 1);               // largest M x N of a weight gradient (with the bias column)
constexpr int NCB = 1792;                                // the 12 per-block Linear(288 -> C) outputs side by side

__device__ __forceinline__ float mish_fwd(float u) {
    const float e = expf(fminf(u, 20.0f));
    const float n = e * (e + 2.0f);
    return u * n / (n + 2.0f);
}
// d/du u tanh(softplus(u)) = tanh(sp) + u sigmoid(u) (1 - tanh(sp)^2), tanh(sp) = n / (n + 2), 1 - tanh(sp)^2 = 4 (n + 1) / (n + 2)^2
__device__ __forceinline__ float mish_grad(float u) {
    const float e = expf(fminf(u, 20.0f));
    const float n = e * (e + 2.0f);
    const float q = 1.0f / (n + 2.0f);
    return n * q + u * (e / (1.0f + e)) * (4.0f * (n + 1.0f) * q * q);
}

// The 64 x 64 tile core of the two GEMM kernels: 4 waves as 2 x 2, each with 2 x 2 MFMA tiles of 16 x 16 and NACC accumulator sets.
typedef v4f TileAcc[NACC][2][2];

__device__ __forceinline__ void tile_zero(TileAcc& acc) {
    for (int q = 0; q < NACC; ++q)
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) acc[q][i][j] = v4f{0.f, 0.f, 0.f, 0.f};
}

// acc += As^T Bs over one staged K tile (As[k][m], Bs[k][n]); k-step ks / 4 goes to accumulator set ks / 4
__device__ __forceinline__ void tile_mfma(TileAcc& acc, const float (&As)[BK][LDS_LD], const float (&Bs)[BK][LDS_LD], int lane, int wm, int wn) {
#pragma unroll
    for (int ks = 0; ks < BK; ks += 4) {
        const int kr = ks + (lane >> 4);
        float av[2], bv[2];
        for (int i = 0; i < 2; ++i) av[i] = As[kr][wm * 32 + i * 16 + (lane & 15)];
        for (int j = 0; j < 2; ++j) bv[j] = Bs[kr][wn * 32 + j * 16 + (lane & 15)];
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) acc[ks / 4][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[ks / 4][i][j], 0, 0, 0);
    }
}

// the pairwise sum of the four sets, left in acc[0]
__device__ __forceinline__ void tile_sum(TileAcc& acc) {
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) acc[0][i][j] = (acc[0][i][j] + acc[1][i][j]) + (acc[2][i][j] + acc[3][i][j]);
}

struct ConvGemm {
    const float* in; int lin, cin, in_ld, mode, s, p, ntap;
    const float* wp; const float* bias;
    float* out; int lout, N, out_ld, rows, accumulate;
};

__global__ __launch_bounds__(256) void conv_gemm_kernel(ConvGemm a) {
    __shared__ float As[BK][LDS_LD];
    __shared__ float Bs[BK][LDS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const long M = (long)a.rows * a.lout;
    const int K = a.ntap * a.cin;
    const long m0 = (long)blockIdx.y * BM;
    const int n0 = blockIdx.x * BN;
    TileAcc acc;
    tile_zero(acc);
    for (int k0 = 0; k0 < K; k0 += BK) {
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256, r = e >> 4, kq = e & 15;
            const long m = m0 + r;
            const int kk = k0 + kq;
            float v = 0.f;
            if (m < M && kk < K) {
                const long b = m / a.lout;
                const int lo = (int)(m - b * a.lout), tap = kk / a.cin, c = kk - tap * a.cin;
                int li;
                bool ok;
                if (a.mode == 0) {
                    li = lo * a.s + tap - a.p;
                    ok = li >= 0 && li < a.lin;
                } else {
                    const int q = lo + a.p - tap;
                    li = q >= 0 ? q / a.s : -1;
                    ok = q >= 0 && li * a.s == q && li < a.lin;
                }
                if (ok) v = a.in[(b * a.lin + li) * a.in_ld + c];
            }
            As[kq][r] = v;
        }
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256, kq = e >> 6, n = e & 63, kk = k0 + kq, nn = n0 + n;
            Bs[kq][n] = (kk < K && nn < a.N) ? a.wp[(long)kk * a.N + nn] : 0.f;
        }
        __syncthreads();
        tile_mfma(acc, As, Bs, lane, wm, wn);
        __syncthreads();
    }
    tile_sum(acc);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
            for (int r = 0; r < 4; ++r) {
                const long m = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;
                const int n = n0 + wn * 32 + j * 16 + (lane & 15);
                if (m < M && n < a.N) {
                    float v = acc[0][i][j][r];
                    if (a.bias) v += a.bias[n];
                    float* o = a.out + m * a.out_ld + n;
                    *o = a.accumulate ? *o + v : v;
                }
            }
}

struct Wgrad {
    const float* p; int lp, p_ld, M;                    // P[b, l, m] = p[(b lp + l) p_ld + m]
    const float* g; int lg, g_ld, gc, s, pd, ntap;      // G[b, li, c] = g[(b lg + li) g_ld + c]; N = ntap gc + 1 (the ones column)
    int rows, rows_per, N;
    float* part;
};

__global__ __launch_bounds__(256) void wgrad_kernel(Wgrad a) {
    __shared__ float As[BK][LDS_LD];
    __shared__ float Bs[BK][LDS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int z = blockIdx.z, b0 = z * a.rows_per, b1 = min(a.rows, b0 + a.rows_per);
    const long kbase = (long)b0 * a.lp, K = (long)(b1 - b0) * a.lp;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN, NG = a.ntap * a.gc;
    TileAcc acc;
    tile_zero(acc);
    for (long k0 = 0; k0 < K; k0 += BK) {
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256, kq = e >> 6, r = e & 63, mm = m0 + r;
            const long kr = k0 + kq;
            As[kq][r] = (kr < K && mm < a.M) ? a.p[(kbase + kr) * a.p_ld + mm] : 0.f;
        }
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256, kq = e >> 6, n = e & 63, nn = n0 + n;
            const long kr = k0 + kq;
            float v = 0.f;
            if (kr < K && nn < a.N) {
                if (nn < NG) {
                    const long kg = kbase + kr, b = kg / a.lp;
                    const int l = (int)(kg - b * a.lp), tap = nn / a.gc, c = nn - tap * a.gc, li = l * a.s + tap - a.pd;
                    if (li >= 0 && li < a.lg) v = a.g[(b * a.lg + li) * a.g_ld + c];
                } else {
                    v = 1.f;
                }
            }
            Bs[kq][n] = v;
        }
        __syncthreads();
        tile_mfma(acc, As, Bs, lane, wm, wn);
        __syncthreads();
    }
    tile_sum(acc);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r, n = n0 + wn * 32 + j * 16 + (lane & 15);
                if (m < a.M && n < a.N) a.part[((long)z * a.M + m) * a.N + n] = acc[0][i][j][r];
            }
}

struct WReduce {
    const float* part; int nchunk, M, N, gc, ntap;
    float* dw; long om, oc, ot;     // weight gradient of (m, tap, c) at dw[m om + c oc + tap ot]
    float* db;                      // the ones column: db[m] (null: dropped)
    int accumulate;
    float* db2;                     // a second copy of the ones column (LSTM b_ih / b_hh), or null
};

__global__ __launch_bounds__(256) void wreduce_kernel(WReduce a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)a.M * a.N) return;
    const int m = (int)(idx / a.N), n = (int)(idx - (long)m * a.N);
    float s = 0.f;
    for (int z = 0; z < a.nchunk; ++z) s += a.part[((long)z * a.M + m) * a.N + n];
    float* d;
    if (n < a.ntap * a.gc) {
        const int tap = n / a.gc, c = n - tap * a.gc;
        d = a.dw + m * a.om + c * a.oc + tap * a.ot;
    } else {
        if (a.db2) a.db2[m] = a.accumulate ? a.db2[m] + s : s;
        if (!a.db) return;
        d = a.db + m;
    }
    *d = a.accumulate ? *d + s : s;
}

// dst[(tap C + c) N + n] = src[tap st + c sc + n sn]
__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int ntap, int C, int N, long st,
                                                   long sc, long sn) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)ntap * C * N) return;
    const int n = (int)(idx % N);
    const long kk = idx / N;
    const int tap = (int)(kk / C), c = (int)(kk - (long)tap * C);
    dst[idx] = src[tap * st + c * sc + n * sn];
}

// block-wide sum in a fixed order (wave shuffles, then the 4 wave partials in order)
__device__ __forceinline__ float block_sum(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

struct GnFwd {
    const float* z; float* y; float* stats; const float* gam; const float* bet;
    const float* tb; int tb_ld;     // per-row vector added after Mish (the block's Linear(Mish(tc))), or null
    const float* res;               // residual [B, L, C] added after Mish, or null
    int L, C;
};

// one workgroup per (row, group of C / 8 channels): diffuser_helpers.py:50-67 GroupNorm(8, eps 1e-5) -> Mish (+ bias, + residual)
__global__ __launch_bounds__(256) void gn_mish_fwd_kernel(GnFwd a) {
    __shared__ float red[4];
    const int b = blockIdx.x >> 3, g = blockIdx.x & 7, cg = a.C >> 3, n = a.L * cg;
    const long base = (long)b * a.L * a.C + g * cg;
    float s = 0.f;
    for (int e = threadIdx.x; e < n; e += 256) s += a.z[base + (e / cg) * a.C + e % cg];
    const float mean = block_sum(s, red) / (float)n;
    float ss = 0.f;
    for (int e = threadIdx.x; e < n; e += 256) {
        const float d = a.z[base + (e / cg) * a.C + e % cg] - mean;
        ss += d * d;
    }
    const float rstd = 1.0f / sqrtf(block_sum(ss, red) / (float)n + 1e-5f);
    for (int e = threadIdx.x; e < n; e += 256) {
        const int l = e / cg, c = g * cg + e % cg;
        const long o = base + l * a.C + e % cg;
        float v = mish_fwd((a.z[o] - mean) * rstd * a.gam[c] + a.bet[c]);
        if (a.tb) v += a.tb[(long)b * a.tb_ld + c];
        if (a.res) v += a.res[o];
        a.y[o] = v;
    }
    if (threadIdx.x == 0) {
        a.stats[blockIdx.x * 2] = mean;
        a.stats[blockIdx.x * 2 + 1] = rstd;
    }
}

struct GnBwd {
    const float* dy; const float* z; const float* stats; const float* gam; const float* bet;
    float* dz; float* dgam; float* dbet; float* dsum;   // dgam / dbet / dsum: per-row [B, C] partials (dsum = sum_l dy, or null)
    int L, C;
};

// dz = GN^T (dy * mish'(u)), u = gam xh + bet, with the two per-group reductions; per-row gamma / beta partials
__global__ __launch_bounds__(256) void gn_mish_bwd_kernel(GnBwd a) {
    __shared__ float red[4];
    const int b = blockIdx.x >> 3, g = blockIdx.x & 7, cg = a.C >> 3, n = a.L * cg;
    const long base = (long)b * a.L * a.C + g * cg;
    const float mean = a.stats[blockIdx.x * 2], rstd = a.stats[blockIdx.x * 2 + 1];
    float s1 = 0.f, s2 = 0.f;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int c = g * cg + e % cg;
        const long o = base + (e / cg) * a.C + e % cg;
        const float xh = (a.z[o] - mean) * rstd;
        const float dxh = a.dy[o] * mish_grad(xh * a.gam[c] + a.bet[c]) * a.gam[c];
        s1 += dxh;
        s2 += dxh * xh;
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    const float inv_n = 1.0f / (float)n;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int c = g * cg + e % cg;
        const long o = base + (e / cg) * a.C + e % cg;
        const float xh = (a.z[o] - mean) * rstd;
        const float dxh = a.dy[o] * mish_grad(xh * a.gam[c] + a.bet[c]) * a.gam[c];
        a.dz[o] = rstd * (dxh - (s1 + xh * s2) * inv_n);
    }
    if ((int)threadIdx.x < cg) {
        const int c = g * cg + threadIdx.x;
        float sg = 0.f, sb = 0.f, sd = 0.f;
        for (int l = 0; l < a.L; ++l) {
            const long o = base + l * a.C + threadIdx.x;
            const float xh = (a.z[o] - mean) * rstd, gg = a.dy[o] * mish_grad(xh * a.gam[c] + a.bet[c]);
            sg += gg * xh;
            sb += gg;
            sd += a.dy[o];
        }
        a.dgam[(long)b * a.C + c] = sg;
        a.dbet[(long)b * a.C + c] = sb;
        if (a.dsum) a.dsum[(long)b * a.C + c] = sd;
    }
}

// te0[b, :] = [sin(t w_k), cos(t w_k)], k < 16 (diffuser_helpers.py:25-32); w_k as torch computes them in fp32
struct SinW { float w[16]; };
__global__ __launch_bounds__(256) void sinus_kernel(const int32_t* t, float* te0, SinW w, int B) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * 16) return;
    const int b = idx >> 4, k = idx & 15;
    const float e = (float)t[b] * w.w[k];
    te0[b * 32 + k] = sinf(e);
    te0[b * 32 + 16 + k] = cosf(e);
}

// tc[b] = [te | cond] (te already in tc[:, :32]), mt = Mish(tc) (temporal.py:141-146 and every block's time_mlp.0)
__global__ __launch_bounds__(256) void tc_fwd_kernel(float* tc, const float* cond, float* mt, int B) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * 288) return;
    const int b = idx / 288, j = idx - b * 288;
    float v = tc[idx];
    if (j >= 32) tc[idx] = v = cond[b * 256 + j - 32];
    mt[idx] = mish_fwd(v);
}

__global__ __launch_bounds__(256) void mish_fwd_kernel(const float* x, float* y, int n) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < n) y[idx] = mish_fwd(x[idx]);
}

__global__ __launch_bounds__(256) void mish_bwd_kernel(const float* x, const float* dy, float* dx, int n) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < n) dx[idx] = dy[idx] * mish_grad(x[idx]);
}

// dtc = dmt * mish'(tc) -> dte [B, 32], dcond [B, 256] (nullable)
__global__ __launch_bounds__(256) void tc_bwd_kernel(const float* tc, const float* dmt, float* dte, float* dcond, int B) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * 288) return;
    const int b = idx / 288, j = idx - b * 288;
    const float v = dmt[idx] * mish_grad(tc[idx]);
    if (j < 32) dte[b * 32 + j] = v;
    else if (dcond) dcond[b * 256 + j - 32] = v;
}

// dst[r dld + c] (+)= src[r sld + c], r < R, c < C
__global__ __launch_bounds__(256) void copy2d_kernel(const float* src, int sld, float* dst, int dld, long R, int C, int accumulate) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= R * C) return;
    const long r = idx / C;
    const int c = (int)(idx - r * C);
    float* d = dst + r * dld + c;
    const float v = src[r * sld + c];
    *d = accumulate ? *d + v : v;
}

// ------------------------------------------------------------------ parameter table
struct UnetTable : ParamTable {
    UnetTable() {
        add("model.time_mlp.1.weight", {128, 32}); add("model.time_mlp.1.bias", {128});
        add("model.time_mlp.3.weight", {32, 128}); add("model.time_mlp.3.bias", {32});
        // the blocks' execution order is the state_dict's; the re-sampling conv of a level follows its second block
        // (temporal.py:84-115: Downsample1d Conv1d k3 after downs.0 / downs.1, Upsample1d ConvTranspose1d k4 after ups.0 / ups.1)
        for (int k = 0; k < 12; ++k) {
            const std::string pre = kBlocks[k].name;
            const int cin = kBlocks[k].cin, c = kBlocks[k].cout;
            add(pre + ".time_mlp.1.weight", {c, 288}); add(pre + ".time_mlp.1.bias", {c});
            add(pre + ".blocks.0.block.0.weight", {c, cin, 5}); add(pre + ".blocks.0.block.0.bias", {c});
            add(pre + ".blocks.0.block.2.weight", {c}); add(pre + ".blocks.0.block.2.bias", {c});
            add(pre + ".blocks.1.block.0.weight", {c, c, 5}); add(pre + ".blocks.1.block.0.bias", {c});
            add(pre + ".blocks.1.block.2.weight", {c}); add(pre + ".blocks.1.block.2.bias", {c});
            if (cin != c) { add(pre + ".residual_conv.weight", {c, cin, 1}); add(pre + ".residual_conv.bias", {c}); }
            const int ktap = (k == 1 || k == 3) ? 3 : (k == 9 || k == 11) ? 4 : 0;
            if (ktap) {
                const std::string lvl = pre.substr(0, pre.size() - 1) + "2.conv";
                add(lvl + ".weight", {c, c, ktap}); add(lvl + ".bias", {c});
            }
        }
        add("model.final_conv.0.block.0.weight", {64, 64, 5}); add("model.final_conv.0.block.0.bias", {64});
        add("model.final_conv.0.block.2.weight", {64}); add("model.final_conv.0.block.2.bias", {64});
        add("model.final_conv.1.weight", {4, 64, 1}); add("model.final_conv.1.bias", {4});
    }
};

const ParamTable& table() {
    static const UnetTable t;
    return t;
}

// ------------------------------------------------------------------ the walk: tape layout and the launches
// per-row floats of the tape items, in tape order; every item is a [B, ...] array
struct Tape {
    size_t te0, a1, m1, tc, mt;
    size_t z0[12], st0[12], h1[12], z1[12], st1[12], out[12];
    size_t down[2], cat[2], up[2], zf, stf, yf, total;
    Tape() {
        size_t o = 0;
        auto take = [&](size_t n) { const size_t r = o; o += n; return r; };
        te0 = take(32); a1 = take(128); m1 = take(128); tc = take(288); mt = take(288);
        for (int k = 0; k < 12; ++k) {
            const size_t n = (size_t)kBlocks[k].L * kBlocks[k].cout;
            z0[k] = take(n); st0[k] = take(16); h1[k] = take(n); z1[k] = take(n); st1[k] = take(16); out[k] = take(n);
            if (k == 1) down[0] = take(26 * 64);
            if (k == 3) down[1] = take(13 * 128);
            if (k == 7) cat[0] = take(13 * 512);
            if (k == 9) { up[0] = take(26 * 128); cat[1] = take(26 * 256); }
            if (k == 11) up[1] = take(52 * 64);
        }
        zf = take(52 * 64); stf = take(16); yf = take(52 * 64);
        total = o;
    }
};

const Tape& tape_layout() {
    static const Tape t;
    return t;
}

int cb_offset(int k) {
    int o = 0;
    for (int i = 0; i < k; ++i) o += kBlocks[i].cout;
    return o;
}

struct Ctx {
    const float* P;     // raw parameters
    float* wp;          // packed weights (same offsets as P)
    int B;
    hipStream_t s;
    const float* prm(const std::string& n) const { return P + table().off(n); }
    float* pk(const std::string& n) const { return wp + table().off(n); }
};

hipError_t pack(const Ctx& c, const std::string& n, int ntap, int C, int N, long st, long sc, long sn) {
    const long tot = (long)ntap * C * N;
    pack_kernel<<<nblk(tot), 256, 0, c.s>>>(c.prm(n), c.pk(n), ntap, C, N, st, sc, sn);
    return hipGetLastError();
}

hipError_t gemm(const Ctx& c, const float* in, int lin, int cin, int in_ld, int mode, int s, int p, int ntap, const float* wp,
                const float* bias, float* out, int lout, int N, int out_ld, int accumulate) {
    ConvGemm a{in, lin, cin, in_ld, mode, s, p, ntap, wp, bias, out, lout, N, out_ld, c.B, accumulate};
    const long M = (long)c.B * lout;
    dim3 grid((N + BN - 1) / BN, (unsigned)((M + BM - 1) / BM));
    conv_gemm_kernel<<<grid, 256, 0, c.s>>>(a);
    return hipGetLastError();
}

// The K split of a weight gradient and its two launches: at most max_chunks chunks of whole rows, the partials of chunk z at
// part[z][M][N], summed in chunk order.  Fills a.rows_per and r.nchunk.
hipError_t launch_wgrad(Wgrad a, WReduce r, int max_chunks, hipStream_t s) {
    int nchunk = a.rows < max_chunks ? a.rows : max_chunks;
    a.rows_per = (a.rows + nchunk - 1) / nchunk;
    r.nchunk = (a.rows + a.rows_per - 1) / a.rows_per;
    dim3 grid((a.N + BN - 1) / BN, (a.M + BM - 1) / BM, r.nchunk);
    wgrad_kernel<<<grid, 256, 0, s>>>(a);
    TRY(hipGetLastError());
    wreduce_kernel<<<nblk((long)a.M * a.N), 256, 0, s>>>(r);
    return hipGetLastError();
}

struct Bwd {
    Ctx c;
    float* dP;          // parameter gradients (null: data gradients only)
    int accumulate;
    float* part;
};

// weight gradient of (m, tap, c) -> dP[name_w][m om + c oc + tap ot], the ones column -> dP[name_b][m]
hipError_t wgrad(const Bwd& w, const float* P, int lp, int p_ld, int M, const float* G, int lg, int g_ld, int gc, int s, int pd, int ntap,
                 const char* name_w, long om, long oc, long ot, const char* name_b) {
    if (!w.dP) return hipSuccess;
    const int N = (G ? ntap * gc : 0) + 1;
    if ((long)M * N > kPart) return hipErrorInvalidValue;
    const Wgrad a{P, lp, p_ld, M, G, lg, g_ld, G ? gc : 0, s, pd, G ? ntap : 0, w.c.B, 0, N, w.part};
    const WReduce r{w.part, 0, M, N, a.gc, a.ntap, name_w ? w.dP + table().off(name_w) : nullptr, om, oc, ot,
                    name_b ? w.dP + table().off(name_b) : nullptr, w.accumulate, nullptr};
    return launch_wgrad(a, r, kChunks, w.c.s);
}

// workspace: packed weights | per-block bias rows [B, 1792] | residual scratch [B, 3328]  (forward)
//            packed weights | partials | dA, dB [B, 6656] | T1, dZ, dskip1, dskip2 [B, 3328] | rows ...  (backward)
struct WsB {
    float *wp, *part, *dA, *dB, *T1, *dZ, *ds1, *ds2, *dgam, *dbet, *dsum, *dmt, *dte, *dm1, *da1, *dxt;
    size_t floats;
};
WsB carve_bwd(float* ws, int B) {
    WsB w{};
    size_t o = 0;
    auto take = [&](size_t n) { float* r = ws + o; o += (n + 63) / 64 * 64; return r; };
    w.wp = take(table().floats);
    w.part = take((size_t)kChunks * kPart);
    w.dA = take((size_t)B * kCat); w.dB = take((size_t)B * kCat);
    w.T1 = take((size_t)B * kAct); w.dZ = take((size_t)B * kAct); w.ds1 = take((size_t)B * kAct); w.ds2 = take((size_t)B * kAct);
    w.dgam = take((size_t)B * 256); w.dbet = take((size_t)B * 256); w.dsum = take((size_t)B * 256);
    w.dmt = take((size_t)B * 288); w.dte = take((size_t)B * 32); w.dm1 = take((size_t)B * 128); w.da1 = take((size_t)B * 128);
    w.dxt = take((size_t)B * 52 * 4);
    w.floats = o;
    return w;
}
size_t ws_bwd_floats(int B) {
    static float dummy;
    return carve_bwd(&dummy, B).floats;
}
size_t ws_fwd_floats(int B) { return table().floats + 64 + (size_t)B * NCB + 64 + (size_t)B * kAct; }

}  // namespace

const TrainParam* train_params() { return table().p.data(); }
size_t train_param_floats() { return table().floats; }
size_t train_tape_floats(int B) { return tape_layout().total * (size_t)B; }
size_t train_ws_floats(int B) {
    const size_t a = ws_fwd_floats(B), b = ws_bwd_floats(B);
    return a > b ? a : b;
}

hipError_t train_forward(const float* params, const float* x, const float* cond, const int32_t* t_idx, float* eps, float* tape, int B,
                         float* ws, hipStream_t s) {
    const Tape& T = tape_layout();
    const Ctx c{params, ws, B, s};
    float* tbs = ws + (table().floats + 63) / 64 * 64;
    float* rs = tbs + ((size_t)B * NCB + 63) / 64 * 64;
    auto tp = [&](size_t off) { return tape + off * (size_t)B; };
    // pack every weight as the forward GEMMs read it: [tap][c_in][c_out]
    for (int i = 0; i < kTrainParams; ++i) {
        const TrainParam& p = table().p[i];
        const std::string n = p.name;
        if (p.ndim == 1) continue;
        if (p.ndim == 2) TRY(pack(c, n, 1, p.shape[1], p.shape[0], 0, 1, p.shape[1]));                  // Linear [out, in]
        else if (n.find(".conv.weight") != std::string::npos && n.rfind("model.ups.", 0) == 0)
            TRY(pack(c, n, p.shape[2], p.shape[0], p.shape[1], 1, (long)p.shape[1] * p.shape[2], p.shape[2]));   // ConvTranspose1d [ci, co, k]
        else TRY(pack(c, n, p.shape[2], p.shape[1], p.shape[0], 1, p.shape[2], (long)p.shape[1] * p.shape[2]));  // Conv1d [co, ci, k]
    }
    // time embedding (temporal.py:141-146): te0 -> Linear -> Mish -> Linear, tc = [te | cond], mt = Mish(tc)
    SinW sw{};
    {
        const float step = (float)(-(std::log(10000.0) / 15.0));
        for (int k = 0; k < 16; ++k) sw.w[k] = std::exp((float)k * step);
    }
    sinus_kernel<<<nblk(B * 16), 256, 0, s>>>(t_idx, tp(T.te0), sw, B);
    TRY(hipGetLastError());
    TRY(gemm(c, tp(T.te0), 1, 32, 32, 0, 1, 0, 1, c.pk("model.time_mlp.1.weight"), c.prm("model.time_mlp.1.bias"), tp(T.a1), 1, 128, 128, 0));
    mish_fwd_kernel<<<nblk(B * 128), 256, 0, s>>>(tp(T.a1), tp(T.m1), B * 128);
    TRY(hipGetLastError());
    TRY(gemm(c, tp(T.m1), 1, 128, 128, 0, 1, 0, 1, c.pk("model.time_mlp.3.weight"), c.prm("model.time_mlp.3.bias"), tp(T.tc), 1, 32, 288, 0));
    tc_fwd_kernel<<<nblk(B * 288), 256, 0, s>>>(tp(T.tc), cond, tp(T.mt), B);
    TRY(hipGetLastError());
    for (int k = 0; k < 12; ++k) {
        const std::string pre = kBlocks[k].name;
        TRY(gemm(c, tp(T.mt), 1, 288, 288, 0, 1, 0, 1, c.pk(pre + ".time_mlp.1.weight"), c.prm(pre + ".time_mlp.1.bias"), tbs + cb_offset(k), 1,
                 kBlocks[k].cout, NCB, 0));
    }
    // residual blocks: out = Mish(GN(conv(Mish(GN(conv x)) + tb))) + res(x)
    auto block = [&](int k, const float* xin) -> hipError_t {
        const std::string pre = kBlocks[k].name;
        const int L = kBlocks[k].L, cin = kBlocks[k].cin, C = kBlocks[k].cout;
        TRY(gemm(c, xin, L, cin, cin, 0, 1, 2, 5, c.pk(pre + ".blocks.0.block.0.weight"), c.prm(pre + ".blocks.0.block.0.bias"), tp(T.z0[k]), L, C, C, 0));
        GnFwd g0{tp(T.z0[k]), tp(T.h1[k]), tp(T.st0[k]), c.prm(pre + ".blocks.0.block.2.weight"), c.prm(pre + ".blocks.0.block.2.bias"),
                 tbs + cb_offset(k), NCB, nullptr, L, C};
        gn_mish_fwd_kernel<<<B * 8, 256, 0, s>>>(g0);
        TRY(hipGetLastError());
        TRY(gemm(c, tp(T.h1[k]), L, C, C, 0, 1, 2, 5, c.pk(pre + ".blocks.1.block.0.weight"), c.prm(pre + ".blocks.1.block.0.bias"), tp(T.z1[k]), L, C, C, 0));
        const float* res = xin;
        if (cin != C) {
            TRY(gemm(c, xin, L, cin, cin, 0, 1, 0, 1, c.pk(pre + ".residual_conv.weight"), c.prm(pre + ".residual_conv.bias"), rs, L, C, C, 0));
            res = rs;
        }
        GnFwd g1{tp(T.z1[k]), tp(T.out[k]), tp(T.st1[k]), c.prm(pre + ".blocks.1.block.2.weight"), c.prm(pre + ".blocks.1.block.2.bias"),
                 nullptr, 0, res, L, C};
        gn_mish_fwd_kernel<<<B * 8, 256, 0, s>>>(g1);
        return hipGetLastError();
    };
    const long BL13 = (long)B * 13, BL26 = (long)B * 26;
    TRY(block(0, x));
    TRY(block(1, tp(T.out[0])));
    TRY(gemm(c, tp(T.out[1]), 52, 64, 64, 0, 2, 1, 3, c.pk("model.downs.0.2.conv.weight"), c.prm("model.downs.0.2.conv.bias"), tp(T.down[0]), 26, 64, 64, 0));
    TRY(block(2, tp(T.down[0])));
    TRY(block(3, tp(T.out[2])));
    TRY(gemm(c, tp(T.out[3]), 26, 128, 128, 0, 2, 1, 3, c.pk("model.downs.1.2.conv.weight"), c.prm("model.downs.1.2.conv.bias"), tp(T.down[1]), 13, 128, 128, 0));
    TRY(block(4, tp(T.down[1])));
    TRY(block(5, tp(T.out[4])));
    TRY(block(6, tp(T.out[5])));
    TRY(block(7, tp(T.out[6])));
    copy2d_kernel<<<nblk(BL13 * 256), 256, 0, s>>>(tp(T.out[7]), 256, tp(T.cat[0]), 512, BL13, 256, 0);        // temporal.py:164 cat(x, skip)
    copy2d_kernel<<<nblk(BL13 * 256), 256, 0, s>>>(tp(T.out[5]), 256, tp(T.cat[0]) + 256, 512, BL13, 256, 0);
    TRY(hipGetLastError());
    TRY(block(8, tp(T.cat[0])));
    TRY(block(9, tp(T.out[8])));
    TRY(gemm(c, tp(T.out[9]), 13, 128, 128, 1, 2, 1, 4, c.pk("model.ups.0.2.conv.weight"), c.prm("model.ups.0.2.conv.bias"), tp(T.up[0]), 26, 128, 128, 0));
    copy2d_kernel<<<nblk(BL26 * 128), 256, 0, s>>>(tp(T.up[0]), 128, tp(T.cat[1]), 256, BL26, 128, 0);
    copy2d_kernel<<<nblk(BL26 * 128), 256, 0, s>>>(tp(T.out[3]), 128, tp(T.cat[1]) + 128, 256, BL26, 128, 0);
    TRY(hipGetLastError());
    TRY(block(10, tp(T.cat[1])));
    TRY(block(11, tp(T.out[10])));
    TRY(gemm(c, tp(T.out[11]), 26, 64, 64, 1, 2, 1, 4, c.pk("model.ups.1.2.conv.weight"), c.prm("model.ups.1.2.conv.bias"), tp(T.up[1]), 52, 64, 64, 0));
    // final_conv (temporal.py:117-120): Conv1dBlock(64, 64, 5) -> Conv1d(64, 4, 1)
    TRY(gemm(c, tp(T.up[1]), 52, 64, 64, 0, 1, 2, 5, c.pk("model.final_conv.0.block.0.weight"), c.prm("model.final_conv.0.block.0.bias"), tp(T.zf), 52, 64, 64, 0));
    GnFwd gf{tp(T.zf), tp(T.yf), tp(T.stf), c.prm("model.final_conv.0.block.2.weight"), c.prm("model.final_conv.0.block.2.bias"), nullptr, 0, nullptr, 52, 64};
    gn_mish_fwd_kernel<<<B * 8, 256, 0, s>>>(gf);
    TRY(hipGetLastError());
    return gemm(c, tp(T.yf), 52, 64, 64, 0, 1, 0, 1, c.pk("model.final_conv.1.weight"), c.prm("model.final_conv.1.bias"), eps, 52, 4, 4, 0);
}

hipError_t train_backward(const float* params, const float* x, const float* tape_c, const float* d_eps, float* d_params, float* dx,
                          float* dcond, int accumulate, int B, float* ws, hipStream_t s) {
    const Tape& T = tape_layout();
    WsB w = carve_bwd(ws, B);
    const Bwd g{Ctx{params, w.wp, B, s}, d_params, accumulate, w.part};
    const Ctx& c = g.c;
    float* tape = const_cast<float*>(tape_c);
    auto tp = [&](size_t off) { return tape + off * (size_t)B; };
    // pack every weight as the data-gradient GEMMs read it: [tap][c_out][c_in] (the adjoint's reduction runs over c_out)
    for (int i = 0; i < kTrainParams; ++i) {
        const TrainParam& p = table().p[i];
        const std::string n = p.name;
        if (p.ndim == 1) continue;
        if (p.ndim == 2) TRY(pack(c, n, 1, p.shape[0], p.shape[1], 0, p.shape[1], 1));                  // Linear [out, in]
        else if (n.find(".conv.weight") != std::string::npos && n.rfind("model.ups.", 0) == 0)
            TRY(pack(c, n, p.shape[2], p.shape[1], p.shape[0], 1, p.shape[2], (long)p.shape[1] * p.shape[2]));   // ConvTranspose1d [ci, co, k]
        else TRY(pack(c, n, p.shape[2], p.shape[0], p.shape[1], 1, (long)p.shape[1] * p.shape[2], p.shape[2]));  // Conv1d [co, ci, k]
    }
    auto gnb = [&](const float* dy, const float* z, const float* st, const std::string& pre, float* dz, float* dsum, int L, int C) -> hipError_t {
        GnBwd a{dy, z, st, c.prm(pre + ".weight"), c.prm(pre + ".bias"), dz, w.dgam, w.dbet, dsum, L, C};
        gn_mish_bwd_kernel<<<B * 8, 256, 0, s>>>(a);
        TRY(hipGetLastError());
        TRY(wgrad(g, w.dgam, 1, C, C, nullptr, 0, 0, 0, 1, 0, 1, nullptr, 0, 0, 0, (pre + ".weight").c_str()));
        return wgrad(g, w.dbet, 1, C, C, nullptr, 0, 0, 0, 1, 0, 1, nullptr, 0, 0, 0, (pre + ".bias").c_str());
    };
    // Conv1d(k, stride s, pad p) with input xin [B, lin, cin] and output gradient dy [B, lout, co]: dW, db, and dx (+)= into dxo
    auto conv_bwd = [&](const std::string& pre, const float* xin, int lin, int cin, const float* dy, int lout, int co, int k, int st, int pd,
                        float* dxo, int acc) -> hipError_t {
        TRY(wgrad(g, dy, lout, co, co, xin, lin, cin, cin, st, pd, k, (pre + ".weight").c_str(), (long)cin * k, k, 1, (pre + ".bias").c_str()));
        return gemm(c, dy, lout, co, co, 1, st, pd, k, c.pk(pre + ".weight"), nullptr, dxo, lin, cin, cin, acc);
    };
    bool first_tb = true;
    // residual block k: d_out -> d_xin (written)
    auto block = [&](int k, const float* xin, const float* d_out, float* d_xin) -> hipError_t {
        const std::string pre = kBlocks[k].name;
        const int L = kBlocks[k].L, cin = kBlocks[k].cin, C = kBlocks[k].cout;
        TRY(gnb(d_out, tp(T.z1[k]), tp(T.st1[k]), pre + ".blocks.1.block.2", w.dZ, nullptr, L, C));
        TRY(conv_bwd(pre + ".blocks.1.block.0", tp(T.h1[k]), L, C, w.dZ, L, C, 5, 1, 2, w.T1, 0));
        TRY(gnb(w.T1, tp(T.z0[k]), tp(T.st0[k]), pre + ".blocks.0.block.2", w.dZ, w.dsum, L, C));
        TRY(conv_bwd(pre + ".blocks.0.block.0", xin, L, cin, w.dZ, L, C, 5, 1, 2, d_xin, 0));
        if (cin != C) {
            TRY(conv_bwd(pre + ".residual_conv", xin, L, cin, d_out, L, C, 1, 1, 0, d_xin, 1));
        } else {
            copy2d_kernel<<<nblk((long)B * L * C), 256, 0, s>>>(d_out, C, d_xin, C, (long)B * L, C, 1);
            TRY(hipGetLastError());
        }
        // the block's Linear(288 -> C) of Mish(tc): its output gradient is sum_l of the first GroupNorm block's output gradient
        TRY(wgrad(g, w.dsum, 1, C, C, tp(T.mt), 1, 288, 288, 1, 0, 1, (pre + ".time_mlp.1.weight").c_str(), 288, 1, 0,
                  (pre + ".time_mlp.1.bias").c_str()));
        TRY(gemm(c, w.dsum, 1, C, C, 0, 1, 0, 1, c.pk(pre + ".time_mlp.1.weight"), nullptr, w.dmt, 1, 288, 288, first_tb ? 0 : 1));
        first_tb = false;
        return hipSuccess;
    };
    // ConvTranspose1d(k 4, s 2, p 1) with input v [B, lin, ci], output gradient du [B, 2 lin, co] -> dv (written)
    auto convT_bwd = [&](const std::string& pre, const float* v, int lin, int ci, const float* du, int co, float* dv) -> hipError_t {
        TRY(wgrad(g, v, lin, ci, ci, du, 2 * lin, co, co, 2, 1, 4, (pre + ".weight").c_str(), (long)co * 4, 4, 1, nullptr));
        TRY(wgrad(g, du, 2 * lin, co, co, nullptr, 0, 0, 0, 1, 0, 1, nullptr, 0, 0, 0, (pre + ".bias").c_str()));
        return gemm(c, du, 2 * lin, co, co, 0, 2, 1, 4, c.pk(pre + ".weight"), nullptr, dv, lin, ci, ci, 0);
    };
    const long BL13 = (long)B * 13, BL26 = (long)B * 26;
    // final_conv.1 (1x1, 64 -> 4), final_conv.0 (Conv1dBlock 64 -> 64)
    TRY(conv_bwd("model.final_conv.1", tp(T.yf), 52, 64, d_eps, 52, 4, 1, 1, 0, w.dB, 0));
    TRY(gnb(w.dB, tp(T.zf), tp(T.stf), "model.final_conv.0.block.2", w.dZ, nullptr, 52, 64));
    TRY(conv_bwd("model.final_conv.0.block.0", tp(T.up[1]), 52, 64, w.dZ, 52, 64, 5, 1, 2, w.dA, 0));
    // ups.1: Upsample1d, the two blocks, the split of cat(u0, skip1)
    TRY(convT_bwd("model.ups.1.2.conv", tp(T.out[11]), 26, 64, w.dA, 64, w.dB));
    TRY(block(11, tp(T.out[10]), w.dB, w.dA));
    TRY(block(10, tp(T.cat[1]), w.dA, w.dB));
    copy2d_kernel<<<nblk(BL26 * 128), 256, 0, s>>>(w.dB, 256, w.dA, 128, BL26, 128, 0);
    copy2d_kernel<<<nblk(BL26 * 128), 256, 0, s>>>(w.dB + 128, 256, w.ds1, 128, BL26, 128, 0);
    TRY(hipGetLastError());
    // ups.0
    TRY(convT_bwd("model.ups.0.2.conv", tp(T.out[9]), 13, 128, w.dA, 128, w.dB));
    TRY(block(9, tp(T.out[8]), w.dB, w.dA));
    TRY(block(8, tp(T.cat[0]), w.dA, w.dB));
    copy2d_kernel<<<nblk(BL13 * 256), 256, 0, s>>>(w.dB, 512, w.dA, 256, BL13, 256, 0);
    copy2d_kernel<<<nblk(BL13 * 256), 256, 0, s>>>(w.dB + 256, 512, w.ds2, 256, BL13, 256, 0);
    TRY(hipGetLastError());
    // mid blocks, then downs.2 (its output is also skip 2)
    TRY(block(7, tp(T.out[6]), w.dA, w.dB));
    TRY(block(6, tp(T.out[5]), w.dB, w.dA));
    copy2d_kernel<<<nblk(BL13 * 256), 256, 0, s>>>(w.ds2, 256, w.dA, 256, BL13, 256, 1);
    TRY(hipGetLastError());
    TRY(block(5, tp(T.out[4]), w.dA, w.dB));
    TRY(block(4, tp(T.down[1]), w.dB, w.dA));
    // downs.1: Downsample1d (k3, s2, p1), skip 1, the two blocks
    TRY(conv_bwd("model.downs.1.2.conv", tp(T.out[3]), 26, 128, w.dA, 13, 128, 3, 2, 1, w.dB, 0));
    copy2d_kernel<<<nblk(BL26 * 128), 256, 0, s>>>(w.ds1, 128, w.dB, 128, BL26, 128, 1);
    TRY(hipGetLastError());
    TRY(block(3, tp(T.out[2]), w.dB, w.dA));
    TRY(block(2, tp(T.down[0]), w.dA, w.dB));
    // downs.0
    TRY(conv_bwd("model.downs.0.2.conv", tp(T.out[1]), 52, 64, w.dB, 26, 64, 3, 2, 1, w.dA, 0));
    TRY(block(1, tp(T.out[0]), w.dA, w.dB));
    TRY(block(0, x, w.dB, dx ? dx : w.dxt));
    // time embedding: dtc = dmt * Mish'(tc) -> dte, dcond; Linear(128 -> 32), Mish, Linear(32 -> 128)
    tc_bwd_kernel<<<nblk(B * 288), 256, 0, s>>>(tp(T.tc), w.dmt, w.dte, dcond, B);
    TRY(hipGetLastError());
    TRY(wgrad(g, w.dte, 1, 32, 32, tp(T.m1), 1, 128, 128, 1, 0, 1, "model.time_mlp.3.weight", 128, 1, 0, "model.time_mlp.3.bias"));
    TRY(gemm(c, w.dte, 1, 32, 32, 0, 1, 0, 1, c.pk("model.time_mlp.3.weight"), nullptr, w.dm1, 1, 128, 128, 0));
    mish_bwd_kernel<<<nblk(B * 128), 256, 0, s>>>(tp(T.a1), w.dm1, w.da1, B * 128);
    TRY(hipGetLastError());
    return wgrad(g, w.da1, 1, 128, 128, tp(T.te0), 1, 32, 32, 1, 0, 1, "model.time_mlp.1.weight", 32, 1, 0, "model.time_mlp.1.bias");
}

// The LSTM-VAE's weight gradients have at most 4 x 2 output tiles and K = 52 B: with 32 chunks a workgroup walks 208 K tiles at 2,048
// rows, one workgroup per CU, latency-bound (~650 us per launch).  Up to 256 chunks put 8 workgroups on a CU and 26 K tiles in each.
constexpr int kWgradChunks = 256;

size_t train_wgrad_part_floats(int M, int gc) { return (size_t)kWgradChunks * M * (gc + 1); }

hipError_t train_wgrad(const float* P, int lp, int p_ld, int M, const float* G, int lg, int g_ld, int gc, int pd, int rows, float* dw,
                       long om, float* db, float* db2, int accumulate, float* part, hipStream_t s) {
    const int N = gc + 1;
    const Wgrad a{P, lp, p_ld, M, G, lg, g_ld, gc, 1, pd, 1, rows, 0, N, part};
    const WReduce r{part, 0, M, N, gc, 1, dw, om, 1, 0, db, accumulate, db2};
    return launch_wgrad(a, r, kWgradChunks, s);
}

}  // namespace cld
