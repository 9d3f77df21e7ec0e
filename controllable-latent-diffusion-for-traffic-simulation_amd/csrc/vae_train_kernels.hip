// vae_train_kernels.hip -- exact-fp32 training path of the LSTM-VAE (models/vae/lstm_vae.py): the encoder (2-layer LSTM(6 -> 64) and
// the mu / logvar heads) and the decoder (2-layer LSTM(4 -> 64) and hid2act), both with h0 = cond2hidden(cond) for both layers, c0 = 0,
// and nn.LSTM's inter-layer dropout as a caller-given mask on layer 0's output where layer 1 reads it.
//   h0_kernel          h0 [B, 64] = cond2hidden(cond): step -1 of both layers' h on the tape
//   lstm_fwd_kernel    both layers over t = 0..51 on v_mfma_f32_16x16x4_f32 with the structure of encode_mfma_kernel / decode_mfma_kernel
//                      (16 rows per workgroup, wave w owns units 16w..16w+15 and their four gate N-tiles, the cell update in registers),
//                      the weights read raw from the flat buffer; it tapes the activated gates, c and h of both layers and layer 1's input
//   head_kernel        mu / logvar (or act) = Linear(64 -> k) of the top layer's h at every step
//   dhead_kernel       the heads' cotangent on the top layer's h: W_mu^T d_mu + W_lv^T d_logvar (or hid2act^T d_act)
//   lstm_bptt_kernel   t = 51..0 through both layers, top layer first: dgates (to the workspace), then dh_{t-1} = W_hh^T dgates and
//                      d_in = W_ih^T dgates as the GEMMs [16 rows x 256] x [256 x 64] on the same MFMA; layer 1's d_in, masked, joins
//                      layer 0's dh at the same t; after t = 0 the two layers' dh of h0 add into d(cond2hidden)
//   dcond_kernel       dcond = cond2hidden^T dh0
// The weight gradients (dW_ih = sum dgates x input, dW_hh = sum dgates x h_{t-1}, the biases, the heads, cond2hidden) run on the U-Net
// path's weight-gradient GEMM (train_wgrad: K split over whole rows, summed in a fixed order, no float atomics).
#include <hip/hip_runtime.h>

#include <string>

#include "train.h"

namespace cld {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int T = 52, H = 64, G4 = 256, AG = 16, COND = 256;

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// ------------------------------------------------------------------ parameter table (LSTMVAE state_dict order)
struct VaeTable : ParamTable {
    VaeTable() {
        auto stack = [&](const std::string& pre, int in) {      // lstm_vae.py:6-19 / 28-43
            add(pre + ".lstm.weight_ih_l0", {G4, in}); add(pre + ".lstm.weight_hh_l0", {G4, H});
            add(pre + ".lstm.bias_ih_l0", {G4});       add(pre + ".lstm.bias_hh_l0", {G4});
            add(pre + ".lstm.weight_ih_l1", {G4, H});  add(pre + ".lstm.weight_hh_l1", {G4, H});
            add(pre + ".lstm.bias_ih_l1", {G4});       add(pre + ".lstm.bias_hh_l1", {G4});
            add(pre + ".cond2hidden.weight", {H, COND}); add(pre + ".cond2hidden.bias", {H});
        };
        stack("lstm_enc", 6);
        stack("lstm_dec", 4);
        add("lstm_dec.hid2act.weight", {2, H}); add("lstm_dec.hid2act.bias", {2});
        add("mu.weight", {4, H});     add("mu.bias", {4});          // lstm_vae.py:79-80
        add("logvar.weight", {4, H}); add("logvar.bias", {4});
    }
};

const ParamTable& table() {
    static const VaeTable t;
    return t;
}

// per-row floats of the tape items, in tape order; every item is a [B, ...] array
struct Tape {
    size_t g[2], c[2], h[2], x1, total;   // activated gates [52, 256] (rows i, f, g, o), c [52, 64], h [53, 64] (h0 first, then
                                          // steps 0..51), layer 1's input (the mask times layer 0's h) [52, 64]
    Tape() {
        size_t o = 0;
        auto take = [&](size_t n) { const size_t r = o; o += n; return r; };
        g[0] = take(T * G4); g[1] = take(T * G4);
        c[0] = take(T * H);  c[1] = take(T * H);
        h[0] = take((T + 1) * H); h[1] = take((T + 1) * H);
        x1 = take(T * H);
        total = o;
    }
};

const Tape& tape_layout() {
    static const Tape t;
    return t;
}

struct LstmW {     // one LSTM stack in the flat buffer, reference layouts
    const float *w_ih0, *w_hh0, *b_ih0, *b_hh0, *w_ih1, *w_hh1, *b_ih1, *b_hh1, *w_c, *b_c;
};

LstmW lstm_w(const float* P, const std::string& pre) {
    auto q = [&](const char* n) { return P + table().off(pre + n); };
    return LstmW{q(".lstm.weight_ih_l0"), q(".lstm.weight_hh_l0"), q(".lstm.bias_ih_l0"), q(".lstm.bias_hh_l0"),
                 q(".lstm.weight_ih_l1"), q(".lstm.weight_hh_l1"), q(".lstm.bias_ih_l1"), q(".lstm.bias_hh_l1"),
                 q(".cond2hidden.weight"), q(".cond2hidden.bias")};
}

// h0 = cond2hidden(cond) (lstm_vae.py:22-23, 46-47), the same summation order as the inference kernels
__global__ __launch_bounds__(256) void h0_kernel(const float* __restrict__ wc, const float* __restrict__ bc, const float* __restrict__ cond,
                                                 float* __restrict__ h0a, float* __restrict__ h0b, int B) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * H) return;
    const int b = idx >> 6, u = idx & 63;
    float s = bc[u];
    const float* wr = wc + u * COND;
    const float* cr = cond + (size_t)b * COND;
    for (int k = 0; k < COND; ++k) s = fmaf(cr[k], wr[k], s);
    h0a[(size_t)b * (T + 1) * H + u] = s;
    h0b[(size_t)b * (T + 1) * H + u] = s;
}

struct Fwd {
    LstmW w;
    const float* x; const float* mask;     // x [B, 52, D], mask [B, 52, 64] or null
    float *G0, *G1, *C0, *C1, *H0, *H1, *X1;
    int B;
};

template <int D>
__global__ __launch_bounds__(256) void lstm_fwd_kernel(const Fwd a) {
    constexpr int HS = 68, KX = (D + 3) / 4;
    __shared__ __attribute__((aligned(16))) float hs[2][2][AG][HS];     // [layer][parity][row][unit]
    __shared__ __attribute__((aligned(16))) float hx[AG][HS];           // layer 1's input: the mask times layer 0's h
    __shared__ float xin[AG][T * D];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, rb = lane >> 4, u = 16 * wv + n;
    const LstmW& w = a.w;
    // B fragments: gate g, k-step (jj, e) -> W[col = 64 g + 16 wv + n][k = 16 jj + 4 rb + e]; the input product: k = 4 q + rb
    float f_hh0[4][4][4], f_ih1[4][4][4], f_hh1[4][4][4], f_ih0[4][KX], fb0[4], fb1[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int col = 64 * g + u;
#pragma unroll
        for (int q = 0; q < KX; ++q) f_ih0[g][q] = 4 * q + rb < D ? w.w_ih0[col * D + 4 * q + rb] : 0.f;
        fb0[g] = w.b_ih0[col] + w.b_hh0[col];
        fb1[g] = w.b_ih1[col] + w.b_hh1[col];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const v4f x0 = *reinterpret_cast<const v4f*>(w.w_hh0 + col * H + 16 * jj + 4 * rb);
            const v4f x1 = *reinterpret_cast<const v4f*>(w.w_ih1 + col * H + 16 * jj + 4 * rb);
            const v4f x2 = *reinterpret_cast<const v4f*>(w.w_hh1 + col * H + 16 * jj + 4 * rb);
#pragma unroll
            for (int e = 0; e < 4; ++e) { f_hh0[g][jj][e] = x0[e]; f_ih1[g][jj][e] = x1[e]; f_hh1[g][jj][e] = x2[e]; }
        }
    }
    const int ngroups = (a.B + AG - 1) / AG;
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int b0 = grp * AG;
        auto row = [&](int ag) { return (b0 + ag < a.B) ? b0 + ag : a.B - 1; };      // tail slots replay the last row; never stored
        for (int i = tid; i < AG * T * D; i += 256) xin[i / (T * D)][i % (T * D)] = a.x[(size_t)row(i / (T * D)) * T * D + i % (T * D)];
        for (int i = tid; i < AG * H; i += 256) {
            const int ag = i >> 6, uu = i & 63;
            hs[0][0][ag][uu] = a.H0[(size_t)row(ag) * (T + 1) * H + uu];
            hs[1][0][ag][uu] = a.H1[(size_t)row(ag) * (T + 1) * H + uu];
        }
        float c0[4] = {0.f, 0.f, 0.f, 0.f}, c1[4] = {0.f, 0.f, 0.f, 0.f};
        __syncthreads();
        for (int t = 0; t < T; ++t) {
            const int pr = t & 1;
            v4f acc[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = v4f{fb0[g], fb0[g], fb0[g], fb0[g]};
#pragma unroll
            for (int q = 0; q < KX; ++q) {
                const float xa = 4 * q + rb < D ? xin[n][D * t + 4 * q + rb] : 0.f;
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa, f_ih0[g][q], acc[g], 0, 0, 0);
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const v4f ha = *reinterpret_cast<const v4f*>(&hs[0][pr][n][16 * jj + 4 * rb]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[e], f_hh0[g][jj][e], acc[g], 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ag = 4 * rb + r, b = row(ag);
                const size_t rt = (size_t)b * T + t;
                const float ig = sigm(acc[0][r]), fg = sigm(acc[1][r]), gg = tanhf(acc[2][r]), og = sigm(acc[3][r]);
                const float c = fg * c0[r] + ig * gg;
                c0[r] = c;
                const float h = og * tanhf(c);
                const float hm = a.mask ? h * a.mask[rt * H + u] : h;
                hs[0][pr ^ 1][ag][u] = h;
                hx[ag][u] = hm;
                if (b0 + ag < a.B) {
                    float* gp = a.G0 + rt * G4;
                    gp[u] = ig; gp[64 + u] = fg; gp[128 + u] = gg; gp[192 + u] = og;
                    a.C0[rt * H + u] = c;
                    a.H0[((size_t)b * (T + 1) + t + 1) * H + u] = h;
                    a.X1[rt * H + u] = hm;
                }
            }
            __syncthreads();
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = v4f{fb1[g], fb1[g], fb1[g], fb1[g]};
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const v4f ha = *reinterpret_cast<const v4f*>(&hx[n][16 * jj + 4 * rb]);
                const v4f hb = *reinterpret_cast<const v4f*>(&hs[1][pr][n][16 * jj + 4 * rb]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[e], f_ih1[g][jj][e], acc[g], 0, 0, 0);
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(hb[e], f_hh1[g][jj][e], acc[g], 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ag = 4 * rb + r, b = row(ag);
                const size_t rt = (size_t)b * T + t;
                const float ig = sigm(acc[0][r]), fg = sigm(acc[1][r]), gg = tanhf(acc[2][r]), og = sigm(acc[3][r]);
                const float c = fg * c1[r] + ig * gg;
                c1[r] = c;
                const float h = og * tanhf(c);
                hs[1][pr ^ 1][ag][u] = h;
                if (b0 + ag < a.B) {
                    float* gp = a.G1 + rt * G4;
                    gp[u] = ig; gp[64 + u] = fg; gp[128 + u] = gg; gp[192 + u] = og;
                    a.C1[rt * H + u] = c;
                    a.H1[((size_t)b * (T + 1) + t + 1) * H + u] = h;
                }
            }
            __syncthreads();
        }
    }
}

// out0[b, t, k] = b0[k] + sum_j h[b, t, j] w0[k, j] (k < n0), out1 likewise with (w1, b1) (k < n1); h = the top layer's h, tape row t + 1
struct Head { const float* h1; const float *w0, *b0, *w1, *b1; float *out0, *out1; int n0, n1, B; };

__global__ __launch_bounds__(256) void head_kernel(const Head a) {
    const int nk = a.n0 + a.n1;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)a.B * T * nk) return;
    const long bt = idx / nk;
    const int k = (int)(idx - bt * nk), b = (int)(bt / T), t = (int)(bt - (long)b * T);
    const bool second = k >= a.n0;
    const int kk = second ? k - a.n0 : k;
    const float* wr = (second ? a.w1 : a.w0) + kk * H;
    const float* hr = a.h1 + ((size_t)b * (T + 1) + t + 1) * H;
    float s = (second ? a.b1 : a.b0)[kk];
    for (int j = 0; j < H; ++j) s = fmaf(hr[j], wr[j], s);
    if (second) a.out1[bt * a.n1 + kk] = s;
    else a.out0[bt * a.n0 + kk] = s;
}

// dh[b, t, u] = sum_k d0[b, t, k] w0[k, u] + sum_k d1[b, t, k] w1[k, u]   (d0 / d1 null: zero)
__global__ __launch_bounds__(256) void dhead_kernel(const float* __restrict__ d0, const float* __restrict__ w0, int n0,
                                                    const float* __restrict__ d1, const float* __restrict__ w1, int n1,
                                                    float* __restrict__ dh, int B) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * T * H) return;
    const long bt = idx >> 6;
    const int u = (int)(idx & 63);
    float s = 0.f;
    if (d0)
        for (int k = 0; k < n0; ++k) s = fmaf(d0[bt * n0 + k], w0[k * H + u], s);
    if (d1)
        for (int k = 0; k < n1; ++k) s = fmaf(d1[bt * n1 + k], w1[k * H + u], s);
    dh[idx] = s;
}

struct Bptt {
    LstmW w;
    const float* mask;                              // [B, 52, 64] or null
    const float *G0, *G1, *C0, *C1;                 // tape
    const float* dh;                                // the heads' cotangent on the top layer's h [B, 52, 64]
    float *dG0, *dG1;                               // dgates [B, 52, 256] per layer (pre-activation, rows i, f, g, o)
    float* dx;                                      // [B, 52, D] or null
    float* dh0;                                     // [B, 64]: the gradient of h0 = cond2hidden(cond), both layers
    int B;
};

// the LSTM cell backward of one (row, unit): gate activations and c_t / c_{t-1} from the tape, dh into h_t, dc the carry from t + 1
// (left as the carry into t - 1); q = the gate rows' gradients before the activations
__device__ __forceinline__ void cell_bwd(const float* __restrict__ gt, int u, float c, float cp, float dh, float& dc, float q[4]) {
    const float ig = gt[u], fg = gt[64 + u], gg = gt[128 + u], og = gt[192 + u];
    const float tc = tanhf(c);
    const float d = dc + dh * og * (1.0f - tc * tc);
    q[0] = d * gg * ig * (1.0f - ig);
    q[1] = d * cp * fg * (1.0f - fg);
    q[2] = d * ig * (1.0f - gg * gg);
    q[3] = dh * tc * og * (1.0f - og);
    dc = d * fg;
}

template <int D>
__global__ __launch_bounds__(256) void lstm_bptt_kernel(const Bptt a) {
    constexpr int GS = 260;
    __shared__ __attribute__((aligned(16))) float dg[2][AG][GS];      // [layer][row][gate row]: this step's dgates, the A operand
    __shared__ float xp[2][4][AG][16];                                 // [step parity][wave][row][input dim]: partials of W_ih0^T dgates
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, rb = lane >> 4, u = 16 * wv + n;
    const LstmW& w = a.w;
    // B fragments of d[row][unit] = sum_j dgates[row][j] W[j][unit]: k-step (jj, e) <-> j = 16 jj + 4 rb + e, unit 16 wv + n.
    // W_ih0^T has D columns (padded to 16): wave wv takes j in [64 wv, 64 wv + 64); the four partials are summed through LDS
    float f_hh1[16][4], f_ih1[16][4], f_hh0[16][4], f_x[4][4];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 16 * jj + 4 * rb + e;
            f_hh1[jj][e] = w.w_hh1[j * H + u];
            f_ih1[jj][e] = w.w_ih1[j * H + u];
            f_hh0[jj][e] = w.w_hh0[j * H + u];
        }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int e = 0; e < 4; ++e) f_x[jj][e] = n < D ? w.w_ih0[(64 * wv + 16 * jj + 4 * rb + e) * D + n] : 0.f;
    const int ngroups = (a.B + AG - 1) / AG;
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int b0 = grp * AG;
        auto row = [&](int ag) { return (b0 + ag < a.B) ? b0 + ag : a.B - 1; };      // tail slots replay the last row; never stored
        auto dx_out = [&](int q, int t) {      // dx of step t: the four waves' partials in wave order
            if (a.dx && tid < AG * D) {
                const int ag = tid / D, d = tid - ag * D;
                if (b0 + ag < a.B)
                    a.dx[((size_t)(b0 + ag) * T + t) * D + d] = ((xp[q][0][ag][d] + xp[q][1][ag][d]) + xp[q][2][ag][d]) + xp[q][3][ag][d];
            }
        };
        float dc0[4] = {0.f, 0.f, 0.f, 0.f}, dc1[4] = {0.f, 0.f, 0.f, 0.f};
        v4f rh0 = v4f{0.f, 0.f, 0.f, 0.f}, rh1 = v4f{0.f, 0.f, 0.f, 0.f};     // dh_t through the recurrence: [row 4 rb + r][unit u]
        for (int t = T - 1; t >= 0; --t) {
            const int pr = t & 1;
            // ---- layer 1: dh = the recurrence + the heads' cotangent
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ag = 4 * rb + r;
                const size_t rt = (size_t)row(ag) * T + t;
                float q[4];
                cell_bwd(a.G1 + rt * G4, u, a.C1[rt * H + u], t > 0 ? a.C1[(rt - 1) * H + u] : 0.f, rh1[r] + a.dh[rt * H + u], dc1[r], q);
#pragma unroll
                for (int k = 0; k < 4; ++k) dg[1][ag][64 * k + u] = q[k];
                if (b0 + ag < a.B)
#pragma unroll
                    for (int k = 0; k < 4; ++k) a.dG1[rt * G4 + 64 * k + u] = q[k];
            }
            __syncthreads();
            if (t < T - 1) dx_out((t + 1) & 1, t + 1);
            v4f p_hh = v4f{0.f, 0.f, 0.f, 0.f}, p_ih = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const v4f d = *reinterpret_cast<const v4f*>(&dg[1][n][16 * jj + 4 * rb]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    p_hh = __builtin_amdgcn_mfma_f32_16x16x4f32(d[e], f_hh1[jj][e], p_hh, 0, 0, 0);
                    p_ih = __builtin_amdgcn_mfma_f32_16x16x4f32(d[e], f_ih1[jj][e], p_ih, 0, 0, 0);
                }
            }
            rh1 = p_hh;
            // ---- layer 0: dh = the recurrence + layer 1's input gradient through the mask
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ag = 4 * rb + r;
                const size_t rt = (size_t)row(ag) * T + t;
                const float din = a.mask ? a.mask[rt * H + u] * p_ih[r] : p_ih[r];
                float q[4];
                cell_bwd(a.G0 + rt * G4, u, a.C0[rt * H + u], t > 0 ? a.C0[(rt - 1) * H + u] : 0.f, rh0[r] + din, dc0[r], q);
#pragma unroll
                for (int k = 0; k < 4; ++k) dg[0][ag][64 * k + u] = q[k];
                if (b0 + ag < a.B)
#pragma unroll
                    for (int k = 0; k < 4; ++k) a.dG0[rt * G4 + 64 * k + u] = q[k];
            }
            __syncthreads();
            v4f p_h0 = v4f{0.f, 0.f, 0.f, 0.f}, p_x = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const v4f d = *reinterpret_cast<const v4f*>(&dg[0][n][16 * jj + 4 * rb]);
#pragma unroll
                for (int e = 0; e < 4; ++e) p_h0 = __builtin_amdgcn_mfma_f32_16x16x4f32(d[e], f_hh0[jj][e], p_h0, 0, 0, 0);
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const v4f d = *reinterpret_cast<const v4f*>(&dg[0][n][64 * wv + 16 * jj + 4 * rb]);
#pragma unroll
                for (int e = 0; e < 4; ++e) p_x = __builtin_amdgcn_mfma_f32_16x16x4f32(d[e], f_x[jj][e], p_x, 0, 0, 0);
            }
            rh0 = p_h0;
#pragma unroll
            for (int r = 0; r < 4; ++r) xp[pr][wv][4 * rb + r][n] = p_x[r];
        }
        __syncthreads();
        dx_out(0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + 4 * rb + r;
            if (b < a.B) a.dh0[(size_t)b * H + u] = rh0[r] + rh1[r];
        }
        __syncthreads();
    }
}

// dcond[b, k] = sum_u dh0[b, u] W_c[u, k]
__global__ __launch_bounds__(256) void dcond_kernel(const float* __restrict__ wc, const float* __restrict__ dh0, float* __restrict__ dcond,
                                                    int B) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * COND) return;
    const int b = idx >> 8, k = idx & 255;
    float s = 0.f;
    for (int u = 0; u < H; ++u) s = fmaf(dh0[(size_t)b * H + u], wc[u * COND + k], s);
    dcond[idx] = s;
}

// workspace of the backward: dgates of both layers | the heads' cotangent | dh0 | zeros (a null head cotangent) | weight-gradient partials
struct Ws {
    float *dG0, *dG1, *dh, *dh0, *zero, *part;
    size_t floats;
};
Ws carve(float* ws, int B) {
    Ws w{};
    size_t o = 0;
    auto take = [&](size_t n) { float* r = ws + o; o += (n + 63) / 64 * 64; return r; };
    w.dG0 = take((size_t)B * T * G4); w.dG1 = take((size_t)B * T * G4);
    w.dh = take((size_t)B * T * H);
    w.dh0 = take((size_t)B * H);
    w.zero = take((size_t)B * T * 4);
    const size_t pa = train_wgrad_part_floats(G4, H), pb = train_wgrad_part_floats(H, COND);
    w.part = take(pa > pb ? pa : pb);
    w.floats = o;
    return w;
}

}  // namespace

const TrainParam* vae_params() { return table().p.data(); }
size_t vae_param_floats() { return table().floats; }
size_t vae_tape_floats(int B) { return tape_layout().total * (size_t)B; }
size_t vae_ws_floats(int B) {
    static float dummy;
    return carve(&dummy, B).floats;
}

hipError_t vae_train_forward(int part, const float* P, const float* x, const float* cond, const float* mask, float* out, float* out2,
                             float* tape, int B, hipStream_t s) {
    const Tape& L = tape_layout();
    auto tp = [&](size_t off) { return tape + off * (size_t)B; };
    const LstmW w = lstm_w(P, part ? "lstm_dec" : "lstm_enc");
    h0_kernel<<<nblk((long)B * H), 256, 0, s>>>(w.w_c, w.b_c, cond, tp(L.h[0]), tp(L.h[1]), B);
    TRY(hipGetLastError());
    const Fwd a{w, x, mask, tp(L.g[0]), tp(L.g[1]), tp(L.c[0]), tp(L.c[1]), tp(L.h[0]), tp(L.h[1]), tp(L.x1), B};
    const int groups = (B + AG - 1) / AG;
    const dim3 grid(groups < 1024 ? groups : 1024);
    if (part == 0) lstm_fwd_kernel<6><<<grid, 256, 0, s>>>(a);
    else lstm_fwd_kernel<4><<<grid, 256, 0, s>>>(a);
    TRY(hipGetLastError());
    auto q = [&](const char* n) { return P + table().off(n); };
    const Head hd = part == 0 ? Head{tp(L.h[1]), q("mu.weight"), q("mu.bias"), q("logvar.weight"), q("logvar.bias"), out, out2, 4, 4, B}
                              : Head{tp(L.h[1]), q("lstm_dec.hid2act.weight"), q("lstm_dec.hid2act.bias"), nullptr, nullptr, out, nullptr, 2, 0, B};
    head_kernel<<<nblk((long)B * T * (hd.n0 + hd.n1)), 256, 0, s>>>(hd);
    return hipGetLastError();
}

hipError_t vae_train_backward(int part, const float* P, const float* x, const float* cond, const float* mask, const float* tape_c,
                              const float* d_out, const float* d_out2, float* dP, float* dx, float* dcond, int accumulate, int B,
                              float* ws, hipStream_t s) {
    const Tape& L = tape_layout();
    float* tape = const_cast<float*>(tape_c);
    auto tp = [&](size_t off) { return tape + off * (size_t)B; };
    const Ws wk = carve(ws, B);
    const std::string pre = part ? "lstm_dec" : "lstm_enc";
    const LstmW w = lstm_w(P, pre);
    auto q = [&](const std::string& n) { return P + table().off(n); };
    const int D = part ? 4 : 6, n0 = part ? 2 : 4, n1 = part ? 0 : 4;
    const float* w0 = q(part ? "lstm_dec.hid2act.weight" : "mu.weight");
    const float* w1 = part ? nullptr : q("logvar.weight");
    if (part) d_out2 = nullptr;
    dhead_kernel<<<nblk((long)B * T * H), 256, 0, s>>>(d_out, w0, n0, d_out2, w1, n1, wk.dh, B);
    TRY(hipGetLastError());
    const Bptt a{w, mask, tp(L.g[0]), tp(L.g[1]), tp(L.c[0]), tp(L.c[1]), wk.dh, wk.dG0, wk.dG1, dx, wk.dh0, B};
    const int groups = (B + AG - 1) / AG;
    const dim3 grid(groups < 1024 ? groups : 1024);
    if (part == 0) lstm_bptt_kernel<6><<<grid, 256, 0, s>>>(a);
    else lstm_bptt_kernel<4><<<grid, 256, 0, s>>>(a);
    TRY(hipGetLastError());
    if (dcond) {
        dcond_kernel<<<nblk((long)B * COND), 256, 0, s>>>(w.w_c, wk.dh0, dcond, B);
        TRY(hipGetLastError());
    }
    if (!dP) return hipSuccess;
    auto dp = [&](const std::string& n) { return dP + table().off(n); };
    for (int l = 0; l < 2; ++l) {
        const std::string ls = std::to_string(l);
        const float* dG = l ? wk.dG1 : wk.dG0;
        const int in = l ? H : D;
        // dW_ih = sum dgates x the layer's input (x, or layer 1's masked input); the ones column, sum dgates, into b_ih and b_hh
        TRY(train_wgrad(dG, T, G4, G4, l ? tp(L.x1) : x, T, in, in, 0, B, dp(pre + ".lstm.weight_ih_l" + ls), in,
                        dp(pre + ".lstm.bias_ih_l" + ls), dp(pre + ".lstm.bias_hh_l" + ls), accumulate, wk.part, s));
        // dW_hh = sum dgates x h_{t-1}: the tape's h starts at step -1 (h0), so its row t is h_{t-1}
        TRY(train_wgrad(dG, T, G4, G4, tp(L.h[l]), T + 1, H, H, 0, B, dp(pre + ".lstm.weight_hh_l" + ls), H, nullptr, nullptr, accumulate,
                        wk.part, s));
    }
    // the heads read h_t of the top layer: tape row t + 1 (pd = -1); a null cotangent is a zero one
    if (!d_out || (part == 0 && !d_out2)) TRY(hipMemsetAsync(wk.zero, 0, (size_t)B * T * 4 * sizeof(float), s));
    const float* p0 = d_out ? d_out : wk.zero;
    if (part == 0) {
        const float* p1 = d_out2 ? d_out2 : wk.zero;
        TRY(train_wgrad(p0, T, 4, 4, tp(L.h[1]), T + 1, H, H, -1, B, dp("mu.weight"), H, dp("mu.bias"), nullptr, accumulate, wk.part, s));
        TRY(train_wgrad(p1, T, 4, 4, tp(L.h[1]), T + 1, H, H, -1, B, dp("logvar.weight"), H, dp("logvar.bias"), nullptr, accumulate, wk.part,
                        s));
    } else {
        TRY(train_wgrad(p0, T, 2, 2, tp(L.h[1]), T + 1, H, H, -1, B, dp("lstm_dec.hid2act.weight"), H, dp("lstm_dec.hid2act.bias"), nullptr,
                        accumulate, wk.part, s));
    }
    // cond2hidden: sum over rows of dh0 x cond
    return train_wgrad(wk.dh0, 1, H, H, cond, 1, COND, COND, 0, B, dp(pre + ".cond2hidden.weight"), COND, dp(pre + ".cond2hidden.bias"),
                       nullptr, accumulate, wk.part, s);
}

}  // namespace cld
