// cld_api.hip -- the C-ABI of libcld_hip (include/cld.h): handle, weight ingestion and
// re-layout, the per-step launch plan of the denoiser, and the sampling loop.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/cld.h"
#include "../../include/cld_eval.h"
#include "../../include/cld_lane.h"
#include "../../include/cld_recon.h"
#include "../../include/cld_solver.h"
#include "cld_kernels.h"
#include "lane_kernels.h"
#include "recon_kernels.h"
#include "sample_metrics_kernels.h"
#include "solver_kernels.h"
#include "train.h"

using namespace cld;

namespace {

constexpr int T = 52, D = 4, COND = 256, TE = 32, NCB = 1792, ACT = 3328;   // ACT floats/agent/buffer
constexpr int NBUF = 8;

struct ConvLayer {
    ConvGeom g{};        // kc / nwn / ks are filled per launch by pick_tiling()
    bool has_a = false, has_b = false;   // which tilings have a kernel instance
    float *wfrag = nullptr, *bias = nullptr, *gamma = nullptr, *beta = nullptr;
    float* ufrag_edge = nullptr;   // the same with the raw taps 0..3 behind them, 12 planes per chunk (wino1d_edge.hip: whole-item launches)
    float* ufrag = nullptr;   // Winograd-domain filters G g of a k5 layer that has a Winograd form (exact-fp32 handles): as a launch of its own
                              // (wino1d_kernels.hip: wino_launch) or inside the layer chains (chain_wino.hip: the 64 -> 64 layers at L = 52 / 26)
    bool wino_launch = false;
    float* rfrag = nullptr;   // a block's 1x1 projection that its second conv can evaluate itself (wino1d_edge.hip): pack_res_proj
    int c_out = 0, c1_real = 0, c1_pad = 0, c2 = 0, ly = 0, off0 = 0, orow0 = 0;
    int cb_off = -1;    // offset into the 1792-wide cond/time bias rows, -1 = none
};

struct ResBlock { ConvLayer c0, c1, res; bool has_res = false; };
constexpr long kProfStride = 10;
constexpr int kChainSmall = 944;      // launch sets of at most this many rows take the one-agent chain tiles (chain_tile): measured per U-Net
                                      // evaluation, one- vs four-agent tiles: 245 / 320 us at 64 rows, 630 / 676 at 512, 916 / 928 at 768,
                                      // 1,120 / 1,096 at 1,008, 1,081 / 1,052 at 1,024, 2,004 / 1,939 at 2,048
const char* const kResnet = "context_encoder.map_encoder.encoder_heads.map_model.";

}  // namespace

struct cld_handle_s {
    cld_config cfg{};
    int stride = 1;                                  // DmModel.stride (dm_model.py:25,119): the loop visits i = ..., 2 stride, stride, 0
    int precision = CLD_PRECISION_F32;               // cfg.precision
    int force_kernel[6] = {0, 0, 0, 0, 0, 0};           // cld_debug_force_kernel: formulation of the guide / decode / encode kernels, of the U-Net's layer chains and of the ContextEncoder's 3x3 convolutions (0 = the library's choice)
    std::string err;
    std::map<std::string, std::vector<float>> w;     // host copies keyed by reference state_dict name
    std::map<std::string, size_t> expect;            // name -> numel
    bool finalized = false, has_decoder = false, has_unet = false;
    cld_goal goal{};                                 // cld_set_goal_term: the goal term every guided call adds while has_goal
    bool has_goal = false;
    cld_social_group social{};                       // cld_set_social_term: the social-group term every guided call adds while has_social
    bool has_social = false;
    cld_pair_term pair{};                            // cld_set_pair_term: the pair-relation term every guided call adds while has_pair
    bool has_pair = false;
    cld_lane_term lane{};                            // cld_set_lane_term: the lane term every guided call adds while has_lane
    bool has_lane = false;
    cld_map_source map_source{};                     // cld_set_map_source: what a cld_map_collision without a drivable_map reads while has_map_source
    bool has_map_source = false;
    std::vector<void*> dev_allocs;
    // schedule (host, fp32 as in dm_model.py:29-56)
    std::vector<float> x_t_cof, noise_cof, plvc, sqrt_acp, sqrt_1m_acp, sqrt_recip_acp, sqrt_recipm1_acp;
    std::vector<float> post_coef1, post_coef2;       // posterior_mean_coef1 / 2 (dm_model.py:50-53; the reconstruction-guided step, cld_recon.h)
    std::vector<float> acp;                          // alphas_cumprod itself (what the few-step samplers form their coefficients from, cld_solver.h)
    float* qs_tab = nullptr;            // device [2][n_timesteps]: sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod) (q_sample, dm_model.py:91-96)
    // device-side model
    ResBlock blocks[12];
    ConvLayer down[2], upT[2][2], final_cb;
    float *wc = nullptr, *cbias_b = nullptr, *tb = nullptr, *head_w = nullptr, *head_b = nullptr, *res4_w = nullptr, *res4_b = nullptr;
    float* head_wfrag = nullptr;        // final_conv.1 as an MFMA N tile (the tail chain of conv_chain.hip)
    const HeadArgs* fuse_upd = nullptr; // set by the caller of run_unet: a DDPM update the tail chain may apply itself (plain steps, no CFG combine)
    bool upd_fused = false;             // ... and whether the last run_unet did
    bool eps_in_buf7 = false;           // the last run_unet left the noise prediction [b_pad,52,4] in buf[7] (chains) instead of final_conv.0's activations
    DecoderWeights dec{};
    EncoderWeights enc{};
    bool has_encoder = false;
    // ContextEncoder (optional): stem, 19 NHWC convolutions, head
    struct Conv2dLayer { float *wfrag = nullptr, *ufrag44 = nullptr, *scale = nullptr, *shift = nullptr; int kh = 3, stride = 1, hin = 56, cin = 64, cout = 64; };   // ufrag44: the Winograd-domain filters of a 3x3 / stride-1 layer (wino44_kernels.hip)
    bool has_context = false;
    float *stem_w = nullptr, *stem_scale = nullptr, *stem_shift = nullptr;
    Conv2dLayer rn_conv[4][2][2], rn_ds[4];
    ContextHeadArgs ctx_head{};
    DynParams dyn{};
    // optional HIP-event timing of the dominant conv kernel instance (k5 GN+Mish block -> 256 channels, L = 13)
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;     // pairs (start, stop)
    size_t prof_used = 0;
    double prof_flop = 0.0;              // algorithmic FLOP of the timed launches
    double prof_exec_flop = 0.0;         // FLOP their MFMAs executed in the form each launch took (Winograd F(4, 5): 8 x 4 k-steps per agent
                                         // and channel pair instead of 5 x 13)
    // the same two counts over ALL launches of the most recent U-Net evaluation (cld_profile_read_executed)
    double eval_alg_flop = 0.0, eval_exec_flop = 0.0;
    int eval_launches = 0;
    // diagnostic (-DCLD_STAMPS builds): launch index within a U-Net evaluation that receives the stamp buffer
    unsigned long long* stamp_buf = nullptr;
    int stamp_layer = -1, launch_counter = 0;
    size_t lds_floor = 0;                // experiments (cld_debug_lds_floor)
    int res_fold = CLD_RES_FOLD_FUSED;    // cld_debug_res_fold: the 1x1 projections inside their block's second conv, or as launches of their own
    long eval_counter = 0;               // U-Net evaluations since profile_enable: every kProfStride-th one is timed
};

namespace {

int fail(cld_handle h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}
#define HIPCK(h, expr)                                                                           \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess)                                                                   \
            return fail(h, CLD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));     \
    } while (0)

float* upload(cld_handle h, const std::vector<float>& v, hipStream_t s, hipError_t* err) {
    float* d = nullptr;
    *err = hipMalloc(reinterpret_cast<void**>(&d), v.size() * sizeof(float));
    if (*err != hipSuccess) return nullptr;
    h->dev_allocs.push_back(d);
    *err = hipMemcpyAsync(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice, s);
    return d;
}

void add_expect(cld_handle h) {
    auto& e = h->expect;
    auto lin = [&](const std::string& p, int o, int i) { e[p + ".weight"] = (size_t)o * i; e[p + ".bias"] = o; };
    auto gn = [&](const std::string& p, int c) { e[p + ".weight"] = c; e[p + ".bias"] = c; };
    // the U-Net and the LSTM-VAE: the tables of the training paths (train.h) are the reference's state_dicts
    for (int i = 0; i < kTrainParams; ++i) e[train_params()[i].name] = train_params()[i].numel;
    for (int i = 0; i < kVaeParams; ++i) e[vae_params()[i].name] = vae_params()[i].numel;
    // ContextEncoder (models/context_utils.py:8-38): two base_models.MLP (`_model` Sequential: Linear, LayerNorm, ReLU, ...)
    // and torchvision resnet18 under map_encoder.encoder_heads.map_model (base_models.py:559-614)
    auto mlp = [&](const std::string& p, int d_in, std::initializer_list<int> hidden, int d_out) {
        int i = 0, d = d_in;
        for (int hd : hidden) {
            lin(p + "._model." + std::to_string(i), hd, d);
            gn(p + "._model." + std::to_string(i + 1), hd);        // LayerNorm weight / bias
            i += 3; d = hd;
        }
        lin(p + "._model." + std::to_string(i), d_out, d);
    };
    auto bn = [&](const std::string& p, int c) {
        e[p + ".weight"] = c; e[p + ".bias"] = c; e[p + ".running_mean"] = c; e[p + ".running_var"] = c;
    };
    mlp("context_encoder.agent_state_encoder", 4, {64, 64}, 64);
    mlp("context_encoder.process_cond_mlp", 320, {320, 320, 256, 256}, 256);
    const std::string r = kResnet;
    e[r + "conv1.weight"] = (size_t)64 * 34 * 49;
    bn(r + "bn1", 64);
    int cin = 64;
    for (int li = 1; li <= 4; ++li) {
        const int c = 32 << li;
        for (int b = 0; b < 2; ++b) {
            const std::string p = r + "layer" + std::to_string(li) + "." + std::to_string(b);
            e[p + ".conv1.weight"] = (size_t)c * (b == 0 ? cin : c) * 9;
            bn(p + ".bn1", c);
            e[p + ".conv2.weight"] = (size_t)c * c * 9;
            bn(p + ".bn2", c);
            if (b == 0 && cin != c) { e[p + ".downsample.0.weight"] = (size_t)c * cin; bn(p + ".downsample.1", c); }
        }
        cin = c;
    }
    lin(r + "fc", 256, 512);
}

// dm_model.py:29-56 + diffuser_helpers.py:451-462, same op order in fp32
void build_schedule(cld_handle h) {
    const int n = h->cfg.n_timesteps;
    std::vector<double> ac(n + 1);
    const double s = 0.008;
    const int steps = n + 1;
    for (int i = 0; i <= n; ++i) {
        const double x = (double)steps * (double)i / (double)(steps - 1);      // np.linspace(0, steps, steps)
        const double c = std::cos(((x / steps) + s) / (1 + s) * M_PI * 0.5);
        ac[i] = c * c;
    }
    const double a0 = ac[0];
    for (auto& v : ac) v /= a0;
    std::vector<float> betas(n), alphas(n), acp(n), acp_prev(n);
    for (int i = 0; i < n; ++i) {
        double b = 1.0 - ac[i + 1] / ac[i];
        b = b < 0 ? 0 : (b > 0.999 ? 0.999 : b);
        betas[i] = (float)b;
        alphas[i] = 1.0f - betas[i];
    }
    // torch.cumprod on a CPU float tensor accumulates in DOUBLE and rounds every element to float (at::acc_type<float, false>):
    // a sequential float product differs from the reference's buffer by up to 3 ulp at n = 100, which the cancellation in
    // alphas - alphas_cumprod * alphas (noise_cof) then amplifies
    double run = 1.0;
    for (int i = 0; i < n; ++i) { run *= (double)alphas[i]; acp[i] = (float)run; acp_prev[i] = i ? acp[i - 1] : 1.0f; }
    h->acp = acp;
    h->x_t_cof.resize(n); h->noise_cof.resize(n); h->plvc.resize(n); h->sqrt_acp.resize(n); h->sqrt_1m_acp.resize(n);
    h->sqrt_recip_acp.resize(n); h->sqrt_recipm1_acp.resize(n); h->post_coef1.resize(n); h->post_coef2.resize(n);
    for (int i = 0; i < n; ++i) {
        h->sqrt_acp[i] = std::sqrt(acp[i]);                 // dm_model.py:36-37
        h->sqrt_1m_acp[i] = std::sqrt(1.0f - acp[i]);
        h->sqrt_recip_acp[i] = std::sqrt(1.0f / acp[i]);             // dm_model.py:40-41 (registered there, read by upstream's predict_start_from_noise)
        h->sqrt_recipm1_acp[i] = std::sqrt(1.0f / acp[i] - 1.0f);
        const float pv = betas[i] * (1.0f - acp_prev[i]) / (1.0f - acp[i]);
        h->plvc[i] = (float)std::log((double)(pv < 1e-20f ? 1e-20f : pv));      // correctly rounded: equals torch.log on every entry of the n = 10 / 50 / 100 tables
        h->x_t_cof[i] = std::sqrt(1.0f / alphas[i]);
        h->noise_cof[i] = betas[i] / std::sqrt(alphas[i] - acp[i] * alphas[i]);
        // dm_model.py:50-53, from the fp32 tables above in double, rounded once
        h->post_coef1[i] = (float)((double)betas[i] * std::sqrt((double)acp_prev[i]) / (1.0 - (double)acp[i]));
        h->post_coef2[i] = (float)((1.0 - (double)acp_prev[i]) * std::sqrt((double)alphas[i]) / (1.0 - (double)acp[i]));
    }
}

double mish_d(double x) { return x * std::tanh(std::log1p(std::exp(x))); }

// MFMA-fragment weight packing.  Slab (16-channel group kgg, tap t) holds, for every 16-column N tile nt
// and lane, the 4 values W[co = 16 nt + (lane & 15)][ci = 16 kgg + 4 (lane >> 4) + s][tap t]; the layout
// does not depend on the K-chunk size, so every tiling of a layer reads the same buffer.
template <class F>
std::vector<float> pack_conv_weights(F&& wget, int c_out, int cin_virtual, int ntaps) {
    const int ngrp = cin_virtual / 16, ntn = c_out / 16;
    std::vector<float> out((size_t)ngrp * ntaps * ntn * 256);
    size_t o = 0;
    for (int kgg = 0; kgg < ngrp; ++kgg)
        for (int t = 0; t < ntaps; ++t)
            for (int nt = 0; nt < ntn; ++nt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s = 0; s < 4; ++s)
                        out[o++] = wget(16 * nt + (lane & 15), 16 * kgg + 4 * (lane >> 4) + s, t);
    return out;
}

// The latent's convolution (4 -> 64 channels, k = 5): K folded over (tap, channel).  Per N tile and lane (n, kk) eight floats:
// [0..3] = W[co][channel s][tap kk], s = 0..3 (the B values of the four MFMAs that walk taps 0..3) and [4] = W[co][channel kk][tap 4].
template <class F>
std::vector<float> pack_latent_conv_weights(F&& wget, int c_out) {
    const int ntn = c_out / 16;
    std::vector<float> out((size_t)ntn * 64 * 8, 0.f);
    for (int nt = 0; nt < ntn; ++nt)
        for (int lane = 0; lane < 64; ++lane) {
            float* o = &out[((size_t)nt * 64 + lane) * 8];
            const int co = 16 * nt + (lane & 15), kk = lane >> 4;
            for (int s = 0; s < 4; ++s) o[s] = wget(co, s, kk);
            o[4] = wget(co, kk, 4);
        }
    return out;
}

// A residual block's 1x1 projection W [c_out][c_in] for the second conv that evaluates it (wino1d_edge.hip, ResProj::wfrag): the planes of
// pack_conv_weights (one tap) and behind them one chunk's worth of zeros -- the kernel requests its A fragment one chunk ahead, the last
// request included, and wino1d_edge_res_frag_floats() is both this buffer's length and the bound the kernel gives its buffer resource.
std::vector<float> pack_res_proj(const float* W, int c_out, int c_in) {
    std::vector<float> out = pack_conv_weights([&](int co, int ci, int) { return W[(size_t)co * c_in + ci]; }, c_out, c_in, 1);
    out.resize((size_t)wino1d_edge_res_frag_floats(c_in, c_out), 0.f);
    return out;
}

// Split-precision packing (CLD_PRECISION_F16X2).  Weights are scaled by kWScale (a power of two that lifts the lo parts
// out of the fp16 subnormal range; undone exactly in the epilogue) and split into hi = fp16(w), lo = fp16(w - hi).
// Slab (32-channel chunk c, tap t, N tile nt) = [hi: 64 lanes x 8 fp16][lo: 64 lanes x 8 fp16]; lane l holds
// W[co = 16 nt + (l & 15)][ci = 32 c + 8 (l >> 4) + j][tap t], j = 0..7 -- the B operand of v_mfma_f32_16x16x32_f16.
constexpr float kWScale = 64.0f;
template <class F>
std::vector<float> pack_conv_weights_split(F&& wget, int c_out, int cin_virtual, int ntaps) {
    const int nchunk = cin_virtual / 32, ntn = c_out / 16;
    std::vector<_Float16> out((size_t)nchunk * ntaps * ntn * 1024);
    size_t o = 0;
    for (int c = 0; c < nchunk; ++c)
        for (int t = 0; t < ntaps; ++t)
            for (int nt = 0; nt < ntn; ++nt) {
                for (int plane = 0; plane < 2; ++plane)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const float w = wget(16 * nt + (lane & 15), 32 * c + 8 * (lane >> 4) + j, t) * kWScale;
                            const _Float16 hi = (_Float16)w;
                            out[o++] = plane == 0 ? hi : (_Float16)(w - (float)hi);
                        }
            }
    std::vector<float> bytes(out.size() / 2);
    std::memcpy(bytes.data(), out.data(), out.size() * sizeof(_Float16));
    return bytes;
}

// Tiling policy: the MFMA/LDS/global-load mix of the conv loop reaches ~83 % of the fp32-MFMA rate with one
// wave per SIMD and ~89 % with two (scripts/ubench/mfma_issue.hip), so take the 64-column tile when it still
// puts two waves on every SIMD of the chip (256 CUs x 4 SIMDs x 2 = 2,048 waves) and the 32-column tile with a
// 2-way K split (twice the workgroups, two per CU) below that.  Measured at B = 1,024: B 813k vs A 716k
// step.agent/s; an 8-wave variant (32 columns, 4-way K split) was slower than B and is not built; the 8-wave
// variant C (64 columns, 2-way K split) is taken for the widest layers where it fills the chip (below).
inline bool c1c2_mult_of_64(const ConvLayer& l) { return l.c1_pad % 64 == 0 && l.c2 % 64 == 0; }     // 64-channel chunks never straddle the two sources

bool pick_tiling(const ConvLayer& l, int b_pad, ConvGeom* g, int roles = 1 /* layers sharing the launch (conv_pair_kernel: 2) */) {
    *g = l.g;
    const long waves_a = (long)(b_pad / (MT / l.g.lm)) * (l.c_out / 64) * 4;
    auto set = [&](int kc, int nwn, int ks) { g->kc = kc; g->nwn = nwn; g->ks = ks; return true; };
    if (l.g.ain == 1)      // split-precision loop: 64-column tiling only (no K split); 64-channel chunks where the images fit
        return l.has_a ? set(l.g.stride == 2 ? 32 : 64, 4, 1) : false;
#ifdef CLD_EXPERIMENTS      // -DCLD_EXPERIMENTS builds only (A/B scripts under scripts/): the shipped library reads no environment variable
    static const char* force = getenv("CLD_TILING");            // A / B / C
#else
    constexpr const char* force = nullptr;
#endif
    if (force && force[0] == 'C' && l.c_out == 256 && l.g.ntaps == 5 && l.g.stride == 1) return set(32, 4, 2);   // 8 waves: 64 columns x 2-way K split
    if (force && force[0] == 'A' && l.has_a) return set(32, 4, 1);
    if (force && force[0] == 'B' && l.has_b) return set(32, 2, 2);
    const bool skip_a = force && force[0] == 'b';      // experiments: 32-column tiles (with CLD_TILING_HALF's height) at every batch size
    if (l.has_a && ((waves_a >= 2048 && !skip_a) || !l.has_b)) return set(32, 4, 1);
    // tiling C for the 256-channel k5 blocks between 1,024 and 2,047 agents: 8-wave workgroups (64 columns x 2-way K split),
    // one per CU -- the same two waves per SIMD as B with half the A-image staging per MFMA (+1.4 % end to end at B = 1,024).
    // One C workgroup is two B workgroups' work on a CU, so in the units of the tile-height model below it costs
    // ceil(wgs_c / 256) * 2 * 13 / 0.92 / 1.014; it competes with the B heights on that cost (B = 1,536: 384 C workgroups are
    // 1.5 rounds of the chip, 768 B workgroups exactly 3 half-rounds).
    double cost_c = 1e30;
    {
        ConvGeom c = l.g; c.kc = 32; c.nwn = 4; c.ks = 2;
        const long wgs_c = (long)(b_pad / (MT / l.g.lm)) * (l.c_out / 64);
#ifdef CLD_EXPERIMENTS
        static const char* tc = getenv("CLD_TILING_C");       // "0" = never, "all" = every layer shape that has an instance
#else
        constexpr const char* tc = nullptr;
#endif
        const bool widest_only = !(tc && tc[0] == 'a');
        if ((!force || skip_a) && !(tc && tc[0] == '0') && l.g.ain == 0 && wgs_c >= 256 && (!widest_only || l.c_out == 256) && conv_geom_supported(c)) {
            cost_c = (double)((wgs_c + 255) / 256) * 2 * 13 / 0.92 / 1.014;
            if (!l.has_b) return set(32, 4, 2);     // (64-channel chunks with this tiling: 918k vs 949k step.agent/s, not built)
        }
    }
    if (l.has_b) {
        set(32, 2, 2);
        // Tile height (HM = 0 / 1 / 2: 208 / 104 / 52 GEMM rows = 13 / 7 / 4 M-tiles per wave): shorter tiles multiply the
        // workgroups and shorten each one's serial MFMA chain, at the price of a partly empty last M-tile.  Cost model (fits
        // the measured sweep B = 8 .. 2,048): a CU holds two workgroups at a time, so a launch takes ceil(n / 256) rounds of
        // NMT M-tiles, at ~0.85 of the MFMA rate when a CU only ever sees one wave per SIMD and ~0.92 otherwise; near-ties go
        // to the taller tile from 1,024 agents (narrow layers there: 945k vs 935k step.agent/s) and to the shorter one below
        // (B = 512: 817k vs 795k).  Sample latency 74 -> 31 ms at B <= 128;
        // throughput x2.4 at B = 64 (208k), x1.9 at 256 (650k), x1.2 at 512 (817k), x1.14 at 768.
#ifdef CLD_EXPERIMENTS
        static const char* th = getenv("CLD_TILING_HALF");        // "0" full tiles only, "1" / "2" force that height
#else
        constexpr const char* th = nullptr;
#endif
        const long wgs_b = (long)(b_pad / (MT / l.g.lm)) * (l.c_out / 32);
        int best = 0;
        double best_cost = 1e30;
        for (int hm = 0; hm <= 3; ++hm) {
            ConvGeom tg = *g; tg.half = hm;
            if (!conv_geom_supported(tg)) continue;
            if (th && th[0] != '0' + hm && (th[0] == '0' || th[0] == '1' || th[0] == '2' || th[0] == '3')) continue;
            const long n = wgs_b << hm, rounds = (n + 255) / 256;
            const int nmt = ((208 >> hm) + 15) / 16;
            double cost = (double)rounds * nmt / (rounds == 1 ? 0.85 : 0.92);
            // the full-height stride-2 tiles stage twice the rows (13 pieces per thread in flight) and still spill: measured
            // per layer at B = 1,024 (scripts/tile_height_ab.sh) 17.7 / 14.7 / 16.1 us (26 -> 13) and 11.6 / 9.9 / 10.2 us (52 -> 26)
            if (l.g.stride == 2 && hm == 0) cost *= 1.15;
            if (cost < best_cost * (b_pad >= 1024 ? 0.97 : 1.0)) { best_cost = cost; best = hm; }      // near-ties: taller tile from 1,024 agents
        }
        if (cost_c <= best_cost) return set(32, 4, 2);
        g->half = best;
        if (best == 3 && (wgs_b << 3) * roles <= 256 && c1c2_mult_of_64(l)) {     // tiling D: at most one workgroup per CU -> give it a second wave per SIMD
            ConvGeom d = *g; d.kc = 64; d.nwn = 2; d.ks = 4;
            if (conv_geom_supported(d)) return set(64, 2, 4);
        }
        return true;
    }
    return false;
}

struct Ws {
    float *xw, *xtmp, *meanb, *cb, *buf[NBUF], *guide;
    float *gcur, *adam_m, *adam_v;      // multi-step guidance: current iterate and Adam moments [b_pad,52,4] each
    float *col_traj, *col_grad;         // collision term: decoded plans and d total / d plans [b_pad,52,6] each
    float* col_act;                     // ... and the decoder's scaled actions [b_pad,52,2] of the forward launch of a split guidance step
};
size_t ws_floats(int b_pad) {
    return (size_t)b_pad * (3 * T * D + NCB + (size_t)NBUF * ACT) + guide_scratch_floats(b_pad) + (size_t)b_pad * (3 * T * D + 2 * T * 6 + T * 2);
}
Ws carve(void* ws, int b_pad) {
    Ws w;
    float* p = static_cast<float*>(ws);
    w.xw = p; p += (size_t)b_pad * T * D;
    w.xtmp = p; p += (size_t)b_pad * T * D;
    w.meanb = p; p += (size_t)b_pad * T * D;
    w.cb = p; p += (size_t)b_pad * NCB;
    for (int i = 0; i < NBUF; ++i) { w.buf[i] = p; p += (size_t)b_pad * ACT; }
    w.guide = p; p += guide_scratch_floats(b_pad);      // activations kept by the guidance kernel's LSTM forward
    w.gcur = p; p += (size_t)b_pad * T * D;
    w.adam_m = p; p += (size_t)b_pad * T * D;
    w.adam_v = p; p += (size_t)b_pad * T * D;
    w.col_traj = p; p += (size_t)b_pad * T * 6;
    w.col_grad = p; p += (size_t)b_pad * T * 6;
    w.col_act = p;
    return w;
}
inline int pad16(int b) { return (b + 15) / 16 * 16; }

ConvArgs make_args(cld_handle h, const ConvLayer& l, const float* x1, const float* x2, float* y, const float* res,
                   const float* cb, const float* tb_row) {
    ConvArgs a{};
    a.x1 = x1; a.x2 = x2; a.c1_real = l.c1_real; a.c1_pad = l.c1_pad; a.c2 = l.c2;
    a.wfrag = l.wfrag; a.bias = l.bias; a.gamma = l.gamma; a.beta = l.beta;
    if (l.cb_off >= 0) { a.cbias = cb + l.cb_off; a.cb_stride = NCB; a.tbias = tb_row ? tb_row + l.cb_off : nullptr; }
    a.res = res; a.y = y; a.c_out = l.c_out; a.ly = l.ly; a.off0 = l.off0; a.orow0 = l.orow0;
    a.wscale_inv = l.g.ain == 1 ? 1.0f / kWScale : 1.0f;
    a.stamps = nullptr;
    (void)h;
    return a;
}

// One conv launch; launches of the dominant kernel shape (k5 + GroupNorm + Mish block producing 256 channels at L = 13) are
// bracketed by HIP events in every kProfStride-th U-Net evaluation while profiling is on: an event pair costs ~2 us of stream
// time, and bracketing all 800 such launches of a 100-step sample call slowed the timed region itself by 5 %.
constexpr int kWino1dMinRows = 384;       // launch sets of at least this many rows take the Winograd form of the k5 layers at L = 13 / 26 (100-step sample,
                                          // direct / Winograd: 38.7 / 48.0 ms at 256 rows, 60.1 / 51.8 at 384, 60.7 / 53.3 at 512, 89.5 / 70.8 at 768, 102.3 / 75.1 at
                                          // 1,024, 189.8 / 134.3 at 2,048; launches of fewer than 512 whole items run as half items, wino1d_kernels.hip; below 384
                                          // rows a launch is a few workgroups' serial MFMA chain and the direct form's small tiles spread it wider)
// the rule itself, a function of the layer shape, the rows of the launch set and what a test forced (cld_debug_conv5_form exposes it)
bool conv5_takes_winograd(int l_in, int c1, int c2, int c_out, long b_pad, int forced) {
    if (!wino1d_supported(l_in, c1, c2, c_out) || forced == CLD_FORM_DIRECT) return false;
    const long widest = c1 > c_out ? c1 : c_out;      // the Winograd kernel addresses its tensors with 32-bit byte offsets (per source tensor)
    if (b_pad * l_in * widest * 4 >= (1L << 31)) return false;
    return forced == CLD_FORM_WINOGRAD || forced == CLD_FORM_WINOGRAD_WHOLE || forced == CLD_FORM_WINOGRAD_KSPLIT || b_pad >= kWino1dMinRows;
}
// what a test forced about the items of the Winograd launches: 0 = by size, 1 = whole items, 2 = whole items of eight waves
int wino_item_form(cld_handle h) {
    const int f = h->force_kernel[CLD_KERNEL_CONV5];
    return f == CLD_FORM_WINOGRAD_WHOLE ? 1 : f == CLD_FORM_WINOGRAD_KSPLIT ? 2 : 0;
}
bool use_wino1d(cld_handle h, const ConvLayer& l, int b_pad) {
    if (!l.ufrag || !l.wino_launch) return false;
    return conv5_takes_winograd(l.g.l_in, l.c1_real, l.c2, l.c_out, b_pad, h->force_kernel[CLD_KERNEL_CONV5]);
}
// FLOP a conv launch stands for (2 x output rows x K x N over the real channels) and FLOP its MFMAs execute in the form
// the launch takes: the direct form pads the 4-channel latent's K to (tap, channel) = 20; the Winograd form runs 8 GEMMs over
// wino1d_gemm_rows() rows (64 per item, idle rows of the L = 26 items included) x C_in x C_out
void count_flop(cld_handle h, const ConvLayer& l, int b_pad, double* alg, double* exec) {
    const double cin = (double)(l.c1_real + l.c2);
    *alg = 2.0 * (double)b_pad * l.g.lm * (l.g.ntaps * cin) * l.c_out;
    if (use_wino1d(h, l, b_pad)) *exec = 2.0 * (double)wino1d_row_planes(l.g.l_in, l.c_out, b_pad, wino_item_form(h)) * cin * l.c_out;
    else *exec = 2.0 * (double)b_pad * l.g.lm * (l.g.padc ? 20.0 : (double)(l.g.ntaps * (l.c1_pad + l.c2))) * l.c_out;
}
void count_launch(cld_handle h, const ConvLayer& l, int b_pad) {
    double alg, exec;
    count_flop(h, l, b_pad, &alg, &exec);
    h->eval_alg_flop += alg;
    h->eval_exec_flop += exec;
    h->eval_launches++;
}
// rp: the block's 1x1 projection, folded into this launch (res_folds: a four-wave whole-item Winograd launch)
hipError_t launch_one(cld_handle h, const ConvLayer& l, const ConvGeom& g, const ConvArgs& a, int b_pad, hipStream_t s, const ResProj* rp = nullptr) {
    count_launch(h, l, b_pad);
    if (use_wino1d(h, l, b_pad)) {
        ConvArgs w = a;
        w.wfrag = l.ufrag;
        w.wfrag_edge = l.ufrag_edge;
        if (rp) {
            w.wfrag = l.ufrag_edge;
            return w.wfrag ? launch_wino1d_edge(w, l.g.l_in, b_pad, false, s, rp) : hipErrorInvalidValue;
        }
        return launch_wino1d(w, l.g.l_in, b_pad, wino_item_form(h), s);
    }
    return rp ? hipErrorInvalidValue : launch_conv(g, a, b_pad, s);
}
hipError_t launch_maybe_timed(cld_handle h, const ConvLayer& l, const ConvGeom& g, const ConvArgs& a, int b_pad, hipStream_t s, const ResProj* rp = nullptr) {
    const bool timed = h->prof_on && g.l_in == 13 && g.ntaps == 5 && g.epi == EPI_GN_MISH && l.c_out == 256 && l.c1_real == 256 &&
                       (h->eval_counter % kProfStride) == 0;
    if (!timed) return launch_one(h, l, g, a, b_pad, s, rp);
    if (h->prof_used + 2 > h->prof_ev.size()) {
        for (int i = 0; i < 2; ++i) {
            hipEvent_t ev;
            hipError_t e = hipEventCreate(&ev);
            if (e != hipSuccess) return e;
            h->prof_ev.push_back(ev);
        }
    }
    hipError_t e = hipEventRecord(h->prof_ev[h->prof_used], s);
    if (e != hipSuccess) return e;
    e = launch_one(h, l, g, a, b_pad, s, rp);
    if (e != hipSuccess) return e;
    e = hipEventRecord(h->prof_ev[h->prof_used + 1], s);
    h->prof_used += 2;
    double alg, exec;
    count_flop(h, l, b_pad, &alg, &exec);
    h->prof_flop += alg;
    h->prof_exec_flop += exec;
    return e;
}

// two independent layers with one grid shape -> one launch (conv_pair_kernel); falls back to two launches
hipError_t run_pair(cld_handle h, const ConvLayer& la, const ConvArgs& aa, const ConvLayer& lb, const ConvArgs& ab,
                    int b_pad, hipStream_t s) {
    ConvGeom ga, gb;
    if (!pick_tiling(la, b_pad, &ga, 2) || !pick_tiling(lb, b_pad, &gb, 2)) return hipErrorInvalidValue;
#ifdef CLD_EXPERIMENTS      // diagnostics (tests/tools/debug_split.py): stop a U-Net evaluation after N launches
    static const int stop_after = getenv("CLD_DEBUG_STOP") ? atoi(getenv("CLD_DEBUG_STOP")) : 1 << 30;
    if (h->launch_counter >= stop_after) return hipSuccess;
#endif
    h->launch_counter += 2;
    if (use_wino1d(h, la, b_pad) || use_wino1d(h, lb, b_pad)) {      // the k5 conv in its Winograd form; the 1x1 projection beside it stays a direct launch
        hipError_t e = launch_maybe_timed(h, la, ga, aa, b_pad, s);
        return e != hipSuccess ? e : launch_maybe_timed(h, lb, gb, ab, b_pad, s);
    }
    if (ga.nwn == gb.nwn && ga.ks == gb.ks && conv_pair_supported(ga, gb)) {
        count_launch(h, la, b_pad);
        count_launch(h, lb, b_pad);
        h->eval_launches--;          // one launch for the two layers
        return launch_conv_pair(ga, aa, gb, ab, b_pad, s);
    }
    hipError_t e = launch_maybe_timed(h, la, ga, aa, b_pad, s);
    return e != hipSuccess ? e : launch_maybe_timed(h, lb, gb, ab, b_pad, s);
}

hipError_t run_args(cld_handle h, const ConvLayer& l, ConvArgs a, int b_pad, hipStream_t s, const ResProj* rp = nullptr);
hipError_t run_conv(cld_handle h, const ConvLayer& l, const float* x1, const float* x2, float* y, const float* res,
                    const float* cb, const float* tb_row, int b_pad, hipStream_t s) {
    return run_args(h, l, make_args(h, l, x1, x2, y, res, cb, tb_row), b_pad, s);
}
hipError_t run_args(cld_handle h, const ConvLayer& l, ConvArgs a, int b_pad, hipStream_t s, const ResProj* rp) {
#ifdef CLD_EXPERIMENTS
    static const int stop_after = getenv("CLD_DEBUG_STOP") ? atoi(getenv("CLD_DEBUG_STOP")) : 1 << 30;
    if (h->launch_counter >= stop_after) return hipSuccess;
#endif
    a.stamps = (h->stamp_buf && h->launch_counter == h->stamp_layer) ? h->stamp_buf : nullptr;
    h->launch_counter++;
    ConvGeom g;
    if (!pick_tiling(l, b_pad, &g)) return hipErrorInvalidValue;
    return launch_maybe_timed(h, l, g, a, b_pad, s, rp);
}

// Whether a residual block's second conv evaluates the block's 1x1 projection itself (wino1d_edge.hip) instead of reading the result of a
// launch of its own: exact-fp32 handles, where that conv runs as four-wave whole Winograd items and has such an instance (blocks 2, 4 and 8;
// block 10's second conv belongs to the tail chain).  Half items, eight-wave items and the direct form keep the separate launch.
bool res_folds(cld_handle h, const ResBlock& rb, int b_pad) {
    if (!rb.has_res || !rb.res.rfrag || h->precision != CLD_PRECISION_F32 || h->res_fold == CLD_RES_FOLD_SEPARATE) return false;
    if (!use_wino1d(h, rb.c1, b_pad) || wino1d_item_form(rb.c1.g.l_in, rb.c1.c_out, b_pad, wino_item_form(h)) != 1) return false;
    if ((long)b_pad * rb.c1.g.l_in * rb.res.c1_real * 4 >= (1L << 31)) return false;      // the kernel's 32-bit byte offsets into the block input (block 8: wider than the conv's own tensors)
    return wino1d_edge_res_supported(rb.c1.g.l_in, rb.c1.c_out, rb.res.c1_real, rb.res.c2);
}

// The 64-channel levels as LDS-resident layer chains (conv_chain.hip): exact-fp32 handles only (the split-precision mode keeps
// one launch per layer).
bool use_chains(cld_handle h, int b_pad) {
    if (h->precision != CLD_PRECISION_F32) return false;
    const int f = h->force_kernel[CLD_KERNEL_UNET];
    if (f == CLD_FORM_LAYERS) return false;
    if (f == CLD_FORM_CHAIN || f == CLD_FORM_CHAIN_TILE1 || f == CLD_FORM_CHAIN_TILE4 || f == CLD_FORM_CHAIN_WINO || f == CLD_FORM_CHAIN_WINO2 || f == CLD_FORM_CHAIN_WINO1) return true;
    (void)b_pad;
    return true;              // measured faster than one launch per layer at every batch size (profiles/r03/chain_check.txt)
}
// agents per chain workgroup: 4 (13 M-tiles per wave at L = 52: the throughput tile) or, for the small batches whose time is
// the LENGTH of the dependent launch sequence, 1 (a quarter of the serial MFMA chain per stage, four times the workgroups)
int chain_tile(cld_handle h, int b_pad) {
    const int f = h->force_kernel[CLD_KERNEL_UNET];
    if (f == CLD_FORM_CHAIN_TILE1) return 1;
    if (f == CLD_FORM_CHAIN_TILE4 || f == CLD_FORM_CHAIN_WINO) return 4;
    return b_pad <= kChainSmall ? 1 : 4;
}
// the chains run their 64 -> 64 k5 layers in Winograd F(4, 5) form (chain_wino.hip) unless a test forces the direct form of the k5 layers
// (CLD_KERNEL_CONV5) or of the chains (CLD_FORM_CHAIN_TILE1 / CLD_FORM_CHAIN_TILE4)
// agents per Winograd chain tile (chain_wino.hip): 4 (two workgroups per CU), 2 or 1 (three per CU)
// (per U-Net evaluation, one / two / four agents: 240 / 262 / 310 us at 64 rows, 536 / 539 / 586 at 512, 700 / 709 / 729 at 768, 768 / 749 / 767 at 1,024,
//  1,100 / 1,080 / 1,119 at 1,536, 1,344 / 1,314 / 1,314 at 2,048, 2,571 / 2,502 / 2,510 at 4,096; the direct one-agent tiles: 246 / 550 / 732 / 810)
int chain_wino_tile(cld_handle h, int b_pad) {
    const int f = h->force_kernel[CLD_KERNEL_UNET];
    if (f == CLD_FORM_CHAIN_WINO) return 4;
    if (f == CLD_FORM_CHAIN_WINO2) return 2;
    if (f == CLD_FORM_CHAIN_WINO1) return 1;
    return b_pad <= kChainSmall ? 1 : 2;
}
bool chain_wino(cld_handle h, int b_pad) {
    const int f = h->force_kernel[CLD_KERNEL_UNET];
    if (f == CLD_FORM_CHAIN_WINO || f == CLD_FORM_CHAIN_WINO2 || f == CLD_FORM_CHAIN_WINO1) return true;
    if (f == CLD_FORM_CHAIN_TILE1 || f == CLD_FORM_CHAIN_TILE4) return false;
    return h->force_kernel[CLD_KERNEL_CONV5] != CLD_FORM_DIRECT;
}

// One span of a U-Net evaluation (temporal.py:122-180): run_unet is the 12 spans in a row, and cld_debug_unet_span runs one of them
// alone.  Every form (one launch per layer, the layer chains, the Winograd launches) runs exactly these 12 spans, so the buffer a span
// writes holds the same tensor in every form.  Span k reads kSpanIn[k] (and the skip kSpanSkip[k]) and writes kSpanOut[k]; -1 is the
// padded latent w.xw.  Span 11 leaves final_conv.0's activations [b_pad,52,64] in w.buf[7], or the noise prediction itself (eps_in_buf7).
constexpr int kSpans = 12;
constexpr int kSpanIn[kSpans] = {-1, 6, 2, 4, 6, 2, 5, 2, 3, 2, 6, 3};
constexpr int kSpanSkip[kSpans] = {-1, -1, -1, -1, -1, -1, -1, -1, 5, -1, -1, 4};
constexpr int kSpanOut[kSpans] = {6, 2, 4, 6, 2, 5, 2, 3, 2, 6, 3, 7};
constexpr int kSpanL[kSpans + 1] = {52, 26, 26, 26, 13, 13, 13, 13, 13, 13, 13, 26, 52};      // rows of a span's input (and of span 11's skip: 26)
constexpr int kSpanC[kSpans + 1] = {4, 64, 128, 128, 128, 256, 256, 256, 256, 128, 128, 128, 4};   // ... its channels; entry 12: eps
hipError_t run_unet_span(cld_handle h, const Ws& w, const float* x, int t_idx, int b_pad, int span, hipStream_t s) {
    const float* tbr = t_idx >= 0 ? h->tb + (size_t)t_idx * NCB : nullptr;     // < 0: per-agent timesteps, time bias folded into w.cb
    float* const* b = w.buf;
    hipError_t e;
#define RC(...) do { e = run_conv(h, __VA_ARGS__, w.cb, tbr, b_pad, s); if (e != hipSuccess) return e; } while (0)
    auto resblock = [&](const ResBlock& rb, const float* in1, const float* in2, float* out) -> hipError_t {
        const float* r = in1;           // identity residual reads the block input
        if (res_folds(h, rb, b_pad)) {  // the second conv projects the block input itself: no pass over it here, no tensor in b[0]
            RC(rb.c0, in1, in2, b[1], nullptr);
            const ResProj rp{in1, in2, rb.res.rfrag, rb.res.bias, rb.res.c1_real, rb.res.c2};
            count_launch(h, rb.res, b_pad);      // its FLOP (the direct form's: the same MFMAs) ...
            h->eval_launches--;                  // ... but no launch
            h->launch_counter++;
            return run_args(h, rb.c1, make_args(h, rb.c1, b[1], nullptr, out, nullptr, w.cb, tbr), b_pad, s, &rp);
        }
        if (rb.has_res) {               // first conv and 1x1 projection both read only the block input: one launch
            e = run_pair(h, rb.c0, make_args(h, rb.c0, in1, in2, b[1], nullptr, w.cb, tbr),
                         rb.res, make_args(h, rb.res, in1, in2, b[0], nullptr, w.cb, tbr), b_pad, s);
            if (e != hipSuccess) return e;
            r = b[0];
        } else {
            RC(rb.c0, in1, in2, b[1], nullptr);
        }
        RC(rb.c1, b[1], nullptr, out, r);
        return hipSuccess;
    };
#define RB(...) do { e = resblock(__VA_ARGS__); if (e != hipSuccess) return e; } while (0)
    switch (span) {
    case 0:
    if (use_chains(h, b_pad)) {
        // downs.0 (five layers at 64 channels x 52 rows) as one launch, the tile resident in LDS (conv_chain.hip)
        ChainHeadArgs ca{};
        ca.x = x;
        auto stage = [&](const ConvLayer& l, int res_kind, int keep) {
            ChainStage st{};
            st.wfrag = l.wfrag; st.ufrag = l.ufrag; st.bias = l.bias; st.gamma = l.gamma; st.beta = l.beta; st.cb_off = l.cb_off;
            st.res_kind = res_kind; st.keep = keep;
            return st;
        };
        ca.st[0] = stage(h->blocks[0].c0, CHAIN_RES_NONE, 0);
        ca.st[1] = stage(h->blocks[0].c1, CHAIN_RES_LATENT, 1);
        ca.st[2] = stage(h->blocks[1].c0, CHAIN_RES_NONE, 0);
        ca.st[3] = stage(h->blocks[1].c1, CHAIN_RES_KEPT, 0);
        ca.st[4] = stage(h->down[0], CHAIN_RES_NONE, 0);
        ca.res4_w = h->res4_w; ca.res4_b = h->res4_b;
        ca.cbias = w.cb; ca.cb_stride = NCB; ca.tbias = tbr;
        // spill slots of the chain: b[2] -- and, with the one-agent tiles (4 M-tiles of 16 rows for 52: 4,096 floats per agent instead of
        // 3,328), the first 768 floats per agent of b[3], which follows it in the workspace; both are dead until the up path writes them
        ca.keep = b[2]; ca.y = b[6];
        ca.stamps = (h->stamp_buf && h->stamp_layer == 0) ? h->stamp_buf : nullptr;
        h->launch_counter += 5;
        h->eval_alg_flop += 2.0 * b_pad * 52.0 * 64 * (20 + 3 * 320) + 2.0 * b_pad * 26.0 * 64 * 192 + 2.0 * b_pad * 52.0 * 64 * 4;
        const bool cw = chain_wino(h, b_pad);
        h->eval_exec_flop += cw ? chain_head_wino_exec_flop(b_pad, chain_wino_tile(h, b_pad)) : chain_head_exec_flop(b_pad, chain_tile(h, b_pad));
        h->eval_launches++;
        e = cw ? launch_chain_head_wino(ca, b_pad, chain_wino_tile(h, b_pad), s) : launch_chain_head(ca, b_pad, chain_tile(h, b_pad), s);
        if (e != hipSuccess) return e;
    } else {
    {   // block 0: conv(4 -> 64) | conv(64 -> 64) + residual_conv(x), the 1x1 projection of the latent evaluated in the epilogue
        RC(h->blocks[0].c0, x, nullptr, b[1], nullptr);
        ConvArgs a1 = make_args(h, h->blocks[0].c1, b[1], nullptr, b[2], nullptr, w.cb, tbr);
        a1.res4_x = x; a1.res4_w = h->res4_w; a1.res4_b = h->res4_b;
        e = run_args(h, h->blocks[0].c1, a1, b_pad, s);
        if (e != hipSuccess) return e;
    }
    RB(h->blocks[1], b[2], nullptr, b[3]);
    RC(h->down[0], b[3], nullptr, b[6], nullptr);
    }
    break;
    case 1: RB(h->blocks[2], b[6], nullptr, b[2]); break;
    case 2: RB(h->blocks[3], b[2], nullptr, b[4]); break;            // skip 128@26
    case 3: RC(h->down[1], b[4], nullptr, b[6], nullptr); break;
    case 4: RB(h->blocks[4], b[6], nullptr, b[2]); break;
    case 5: RB(h->blocks[5], b[2], nullptr, b[5]); break;            // skip 256@13
    case 6: RB(h->blocks[6], b[5], nullptr, b[2]); break;
    case 7: RB(h->blocks[7], b[2], nullptr, b[3]); break;
    case 8: RB(h->blocks[8], b[3], b[5], b[2]); break;               // cat(x, skip) 512@13 -> 128@13
    case 9: RB(h->blocks[9], b[2], nullptr, b[6]); break;
    case 10:
    e = run_pair(h, h->upT[0][0], make_args(h, h->upT[0][0], b[6], nullptr, b[3], nullptr, w.cb, tbr),
                 h->upT[0][1], make_args(h, h->upT[0][1], b[6], nullptr, b[3], nullptr, w.cb, tbr), b_pad, s);   // 128@26
    if (e != hipSuccess) return e;
    break;
    case 11:
    h->eps_in_buf7 = false;
    h->upd_fused = false;
    if (use_chains(h, b_pad)) {
        // ups.1.0's first conv + residual projection as one pair launch (K = 256 x 5 from HBM), then everything behind it --
        // ups.1.0's second conv, ups.1.1, the transposed conv, final_conv.0 and final_conv.1 -- as one launch (conv_chain.hip)
        const ResBlock& rb = h->blocks[10];
        e = run_pair(h, rb.c0, make_args(h, rb.c0, b[3], b[4], b[1], nullptr, w.cb, tbr),
                     rb.res, make_args(h, rb.res, b[3], b[4], b[0], nullptr, w.cb, tbr), b_pad, s);
        if (e != hipSuccess) return e;
        auto stage = [&](const ConvLayer& l, int res_kind, int keep, const float* res) {
            ChainStage st{};
            st.wfrag = l.wfrag; st.ufrag = l.ufrag; st.bias = l.bias; st.gamma = l.gamma; st.beta = l.beta; st.cb_off = l.cb_off;
            st.res_kind = res_kind; st.keep = keep; st.res = res;
            return st;
        };
        ChainTailArgs ct{};
        ct.x = b[1];
        ct.st[0] = stage(rb.c1, CHAIN_RES_TENSOR, 1, b[0]);
        ct.st[1] = stage(h->blocks[11].c0, CHAIN_RES_NONE, 0, nullptr);
        ct.st[2] = stage(h->blocks[11].c1, CHAIN_RES_KEPT, 0, nullptr);
        ct.up_even = stage(h->upT[1][0], CHAIN_RES_NONE, 0, nullptr);
        ct.up_odd = stage(h->upT[1][1], CHAIN_RES_NONE, 0, nullptr);
        ct.fin = stage(h->final_cb, CHAIN_RES_NONE, 0, nullptr);
        ct.head_wfrag = h->head_wfrag; ct.head_b = h->head_b;
        ct.cbias = w.cb; ct.cb_stride = NCB; ct.tbias = tbr;
        ct.keep = b[2]; ct.eps = b[7];
        h->upd_fused = false;
        if (const HeadArgs* u = h->fuse_upd) {           // the step's DDPM update in the same launch
            ct.eps = nullptr;
            ct.upd_x = u->x; ct.upd_z = u->z; ct.upd_mean_out = u->mean_out; ct.upd_x_out = u->x_out;
            ct.xc = u->xc; ct.nc = u->nc; ct.sg = u->sg; ct.B = u->B; ct.seed = u->seed; ct.step_salt = u->step_salt;
            h->upd_fused = true;
        }
        h->launch_counter += 6;
        h->eval_alg_flop += 2.0 * b_pad * 26.0 * 64 * (3 * 320) + 2.0 * b_pad * 52.0 * 64 * 128 + 2.0 * b_pad * 52.0 * 64 * 320 + 2.0 * b_pad * 52.0 * 4 * 64;
        const bool cw = chain_wino(h, b_pad);
        h->eval_exec_flop += cw ? chain_tail_wino_exec_flop(b_pad, chain_wino_tile(h, b_pad)) : chain_tail_exec_flop(b_pad, chain_tile(h, b_pad));
        h->eval_launches++;
        e = cw ? launch_chain_tail_wino(ct, b_pad, chain_wino_tile(h, b_pad), s) : launch_chain_tail(ct, b_pad, chain_tile(h, b_pad), s);
        if (e != hipSuccess) return e;
        h->eps_in_buf7 = true;
    } else {
    RB(h->blocks[10], b[3], b[4], b[2]);              // cat(x, skip) 256@26 -> 64@26
    RB(h->blocks[11], b[2], nullptr, b[6]);
    e = run_pair(h, h->upT[1][0], make_args(h, h->upT[1][0], b[6], nullptr, b[3], nullptr, w.cb, tbr),
                 h->upT[1][1], make_args(h, h->upT[1][1], b[6], nullptr, b[3], nullptr, w.cb, tbr), b_pad, s);   // 64@52
    if (e != hipSuccess) return e;
    RC(h->final_cb, b[3], nullptr, b[7], nullptr);
    }
    break;
    default: return hipErrorInvalidValue;
    }
#undef RB
#undef RC
    return hipSuccess;
}

// One U-Net evaluation (temporal.py:122-180) on the padded latent `x` [b_pad,52,4]: the 12 spans in a row; leaves the
// final_conv.0 activations [b_pad,52,64] (or the noise prediction, eps_in_buf7) in w.buf[7].
hipError_t run_unet(cld_handle h, const Ws& w, const float* x, int t_idx, int b_pad, hipStream_t s) {
    h->launch_counter = 0;
    h->eval_counter++;
    h->eval_alg_flop = h->eval_exec_flop = 0.0;
    h->eval_launches = 0;
    set_lds_floor(h->lds_floor);
    for (int k = 0; k < kSpans; ++k)
        if (hipError_t e = run_unet_span(h, w, x, t_idx, b_pad, k, s); e != hipSuccess) return e;
    return hipSuccess;
}

// what the head kernel reads after run_unet: final_conv.0's activations, or the noise prediction itself when the tail chain ran
inline void head_source(cld_handle h, const Ws& w, HeadArgs& a) {
    if (h->eps_in_buf7) a.eps_in = w.buf[7];
    else a.f = w.buf[7];
}

// loop iterations of the sampler: len(range(0, n_timesteps, stride)) (dm_model.py:119)
inline int loop_steps(cld_handle h) { return (h->cfg.n_timesteps + h->stride - 1) / h->stride; }

const std::vector<float>* getw(cld_handle h, const std::string& k) {
    auto it = h->w.find(k);
    return it == h->w.end() ? nullptr : &it->second;
}

// what is behind every cld_set_*_term and cld_set_map_source: the handle keeps a COPY of *term for the guided calls that follow; NULL clears it
template <class Term>
int set_term(cld_handle h, const Term* term, Term cld_handle_s::*slot, bool cld_handle_s::*has) {
    if (!h) return CLD_ERR_ARG;
    h->*has = term != nullptr;
    h->*slot = term ? *term : Term{};
    return CLD_OK;
}

// The sampler's inputs into its workspace: the latent `x` packed into w.xw, the conditioning bias rows of `cond` into w.cb; with CFG
// once more behind them, rows [bp, 2 bp): the same latent, the bias rows of `non_cond`.  x / cond NULL: that part is there already.
int load_inputs(cld_handle h, const Ws& w, int B, int bp, const float* x, const float* cond, const float* non_cond, bool cfg, hipStream_t s) {
    for (int half = 0; half < (cfg ? 2 : 1); ++half) {
        if (x) HIPCK(h, launch_pack_latent(x, w.xw + (size_t)half * bp * T * D, B, bp, s));
        if (cond) HIPCK(h, launch_cond_bias(half ? non_cond : cond, h->wc, h->cbias_b, w.cb + (size_t)half * bp * NCB, B, bp, NCB, s));
    }
    return CLD_OK;
}

}  // namespace

// =============================================================================================
extern "C" {

const char* cld_version(void) { return "libcld_hip 0.1.0 gfx950 mfma_f32_16x16x4 / f16x2-split mfma_f32_16x16x32_f16"; }

int cld_get_precision(cld_handle h) { return h ? h->precision : CLD_ERR_ARG; }

void cld_default_config(cld_config* c) {
    if (!c) return;
    c->horizon = 52; c->latent_dim = 4; c->cond_dim = 256; c->base_dim = 32;
    c->dim_mults[0] = 2; c->dim_mults[1] = 4; c->dim_mults[2] = 8;
    c->hidden = 64; c->n_timesteps = 100; c->step_time = 0.1f;
    c->acce_bound[0] = -10.f; c->acce_bound[1] = 8.f;
    c->v_bound[0] = -10.f; c->v_bound[1] = 30.f;
    c->max_steer = 0.5f; c->max_yawvel = 6.283185307179586f;
    const float mean[6] = {13.162f, -0.13891f, 5.0223f, -0.0046415f, -0.0080072f, -0.0013546f};
    const float stdv[6] = {13.0717f, 2.2462f, 3.6187f, 0.2210f, 2.5770f, 0.0840f};
    for (int i = 0; i < 6; ++i) { c->norm_mean[i] = mean[i]; c->norm_std[i] = stdv[i]; }
    c->precision = CLD_PRECISION_F32;
}

int cld_create(const cld_config* cfg, cld_handle* out) {
    if (!cfg || !out) return CLD_ERR_ARG;
    *out = nullptr;
    if (cfg->horizon != 52 || cfg->latent_dim != 4 || cfg->cond_dim != 256 || cfg->base_dim != 32 ||
        cfg->dim_mults[0] != 2 || cfg->dim_mults[1] != 4 || cfg->dim_mults[2] != 8 || cfg->hidden != 64 ||
        cfg->n_timesteps < 1 || cfg->n_timesteps > 4096)
        return CLD_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return CLD_ERR_HIP;
    cld_handle h = new cld_handle_s();
    h->cfg = *cfg;
    h->precision = cfg->precision;
    if (h->precision != CLD_PRECISION_F32 && h->precision != CLD_PRECISION_F16X2) { delete h; return CLD_ERR_ARG; }
    add_expect(h);
    build_schedule(h);
    DynParams& d = h->dyn;
    d.dt = cfg->step_time; d.acc_lo = cfg->acce_bound[0]; d.acc_hi = cfg->acce_bound[1];
    d.v_lo = cfg->v_bound[0]; d.v_hi = cfg->v_bound[1]; d.max_steer = cfg->max_steer; d.max_yawvel = cfg->max_yawvel;
    for (int i = 0; i < 6; ++i) { d.mean[i] = cfg->norm_mean[i]; d.std[i] = cfg->norm_std[i]; }
    *out = h;
    return CLD_OK;
}

int cld_debug_stamps(cld_handle h, void* buf, int32_t layer) {
    if (!h) return CLD_ERR_ARG;
    h->stamp_buf = static_cast<unsigned long long*>(buf);
    h->stamp_layer = layer;
    return CLD_OK;
}

int cld_debug_guide_stamps(void* out_host) {
    if (!out_host) return CLD_ERR_ARG;
    read_guide_stamps(static_cast<unsigned long long*>(out_host));
    return CLD_OK;
}

int cld_set_stride(cld_handle h, int32_t stride) {
    if (!h || stride < 1 || stride > h->cfg.n_timesteps) return fail(h, CLD_ERR_ARG, "cld_set_stride: stride out of range");
    h->stride = stride;
    return CLD_OK;
}

int cld_debug_lds_floor(cld_handle h, size_t bytes) {
    if (!h) return CLD_ERR_ARG;
    h->lds_floor = bytes;
    return CLD_OK;
}

int cld_debug_force_kernel(cld_handle h, int32_t which, int32_t form) {
    if (!h || which < 0 || which > 5 || form < 0 || form > (which == CLD_KERNEL_GUIDE ? 3 : which == CLD_KERNEL_CONV5 ? 4 : (which == CLD_KERNEL_UNET ? 7 : 2))) return fail(h, CLD_ERR_ARG, "cld_debug_force_kernel: bad argument");
    h->force_kernel[which] = form;
    return CLD_OK;
}

int cld_debug_res_fold(cld_handle h, int32_t mode) {
    if (!h || mode < CLD_RES_FOLD_FUSED || mode > CLD_RES_FOLD_SEPARATE) return fail(h, CLD_ERR_ARG, "cld_debug_res_fold: bad argument");
    h->res_fold = mode;
    return CLD_OK;
}

int64_t cld_debug_pack_res_proj(const float* w, int32_t c_out, int32_t c_in, float* out, int64_t capacity) {
    if (c_out < 16 || c_out % 16 || c_in < 16 || c_in % 16) return CLD_ERR_ARG;
    const int64_t n = wino1d_edge_res_frag_floats(c_in, c_out);
    if (!w && !out) return n;
    if (!w || !out || capacity < n) return CLD_ERR_ARG;
    const std::vector<float> v = pack_res_proj(w, c_out, c_in);
    if ((int64_t)v.size() != n) return CLD_ERR_STATE;
    std::memcpy(out, v.data(), v.size() * sizeof(float));
    return n;
}

int cld_debug_conv5_form(int32_t l_in, int32_t c1, int32_t c2, int32_t c_out, int64_t rows, int32_t forced_form) {
    if (l_in < 1 || c1 < 1 || c2 < 0 || c_out < 1 || rows < 0 || forced_form < 0 || forced_form > 4) return CLD_ERR_ARG;
    return conv5_takes_winograd(l_in, c1, c2, c_out, (long)((rows + 15) / 16 * 16), forced_form) ? CLD_FORM_WINOGRAD : CLD_FORM_DIRECT;
}

int cld_debug_conv5_items(int32_t l_in, int32_t c_out, int64_t rows, int32_t forced_form) {
    if ((l_in != 13 && l_in != 26) || (c_out != 64 && c_out != 128 && c_out != 256) || rows < 0 || rows > (1L << 30) || forced_form < 0 || forced_form > 4) return CLD_ERR_ARG;
    const int forced = forced_form == CLD_FORM_WINOGRAD_WHOLE ? 1 : forced_form == CLD_FORM_WINOGRAD_KSPLIT ? 2 : 0;      // wino_item_form
    return wino1d_item_form(l_in, c_out, (int)((rows + 15) / 16 * 16), forced);
}

int cld_profile_enable(cld_handle h, int32_t on) {
    if (!h) return CLD_ERR_ARG;
    h->prof_on = on != 0;
    h->prof_used = 0;
    h->eval_counter = -1;
    h->prof_flop = 0.0;
    h->prof_exec_flop = 0.0;
    return CLD_OK;
}

int cld_profile_read(cld_handle h, double* total_ms, int64_t* launches, double* total_flop) {
    if (!h) return CLD_ERR_ARG;
    double ms = 0.0;
    for (size_t i = 0; i + 1 < h->prof_used; i += 2) {
        HIPCK(h, hipEventSynchronize(h->prof_ev[i + 1]));
        float t = 0.f;
        HIPCK(h, hipEventElapsedTime(&t, h->prof_ev[i], h->prof_ev[i + 1]));
        ms += t;
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = (int64_t)(h->prof_used / 2);
    if (total_flop) *total_flop = h->prof_flop;
    return CLD_OK;
}

int cld_profile_read_executed(cld_handle h, double* timed_executed_flop, double* eval_algorithmic_flop, double* eval_executed_flop,
                              int32_t* eval_launches) {
    if (!h) return CLD_ERR_ARG;
    if (timed_executed_flop) *timed_executed_flop = h->prof_exec_flop;
    if (eval_algorithmic_flop) *eval_algorithmic_flop = h->eval_alg_flop;
    if (eval_executed_flop) *eval_executed_flop = h->eval_exec_flop;
    if (eval_launches) *eval_launches = h->eval_launches;
    return CLD_OK;
}

int cld_destroy(cld_handle h) {
    if (!h) return CLD_ERR_ARG;
    for (hipEvent_t ev : h->prof_ev) (void)hipEventDestroy(ev);
    for (void* p : h->dev_allocs) (void)hipFree(p);
    delete h;
    return CLD_OK;
}

const char* cld_last_error(cld_handle h) { return h ? h->err.c_str() : "null handle"; }

int cld_load_weight(cld_handle h, const char* name, const float* data, size_t numel) {
    if (!h || !name || !data) return fail(h, CLD_ERR_ARG, "cld_load_weight: null argument");
    if (h->finalized) return fail(h, CLD_ERR_STATE, "cld_load_weight: handle already finalized");
    std::string k = name;
    for (const char* pre : {"dm.", "vae.", "lstmvae."})
        if (k.rfind(pre, 0) == 0) k = k.substr(std::strlen(pre));
    static const char* sched[] = {"betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
                                  "sqrt_one_minus_alphas_cumprod", "log_one_minus_alphas_cumprod",
                                  "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
                                  "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2",
                                  "x_t_cof", "noise_cof"};
    for (const char* sname : sched)
        if (k == sname) return CLD_OK;     // rebuilt from n_timesteps by cld_create
    if (k.size() > 20 && k.compare(k.size() - 20, 20, ".num_batches_tracked") == 0) return CLD_OK;   // BatchNorm counter: unused in eval
    auto it = h->expect.find(k);
    if (it == h->expect.end()) return fail(h, CLD_ERR_ARG, "cld_load_weight: unknown key '" + k + "'");
    if (it->second != numel)
        return fail(h, CLD_ERR_ARG, "cld_load_weight: '" + k + "' expects " + std::to_string(it->second) +
                                        " values, got " + std::to_string(numel));
    h->w[k].assign(data, data + numel);
    return CLD_OK;
}

int cld_finalize(cld_handle h, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (h->finalized) return fail(h, CLD_ERR_STATE, "cld_finalize: already finalized");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // The U-Net is optional as a whole (a VAE-only or ContextEncoder-only handle is legal: VaeModel without a DmModel), never in part
    size_t unet_have = 0, unet_want = 0;
    std::string unet_missing;
    for (const auto& kv : h->expect)
        if (kv.first.rfind("model.", 0) == 0) {
            ++unet_want;
            if (h->w.count(kv.first)) ++unet_have;
            else if (unet_missing.empty()) unet_missing = kv.first;
        }
    if (unet_have != 0 && unet_have != unet_want) return fail(h, CLD_ERR_STATE, "cld_finalize: missing weight '" + unet_missing + "'");
    h->has_unet = unet_have == unet_want;
    hipError_t e = hipSuccess;
#define UP(dst, vec) do { dst = upload(h, vec, s, &e); if (e != hipSuccess) return fail(h, CLD_ERR_HIP, std::string("upload: ") + hipGetErrorString(e)); } while (0)

    // ---- conv layers -------------------------------------------------------------------
    auto build_unet = [&]() -> int {
    auto make_conv = [&](ConvLayer& l, const std::string& wname, int c_out, int c1_real, int c2, int L_in, int lm,
                         int stride, int ntaps, const int* tapk, bool transposed, int off0, int orow0, int ostr,
                         int ly, int epi, const std::string& gn_name, bool in_f32 = false, bool out_f32 = false) -> int {
        const bool split = h->precision == CLD_PRECISION_F16X2;
        const int ain = (split && !in_f32) ? 1 : 0, aout = (split && !out_f32) ? 1 : 0;
        const std::vector<float>& W = *getw(h, wname + ".weight");
        const int c1_pad = (c1_real + 31) / 32 * 32;     // the 4-channel latent is padded to one 32-channel chunk
        const int cin_real = c1_real + c2;
        const int kw = (int)(W.size() / ((size_t)c_out * cin_real));
        auto wget = [&](int co, int civ, int t) -> float {
            int ci;
            if (civ < c1_pad) { if (civ >= c1_real) return 0.f; ci = civ; }
            else ci = c1_real + (civ - c1_pad);
            const int k = tapk[t];
            return transposed ? W[((size_t)ci * c_out + co) * kw + k]     // ConvTranspose1d [C_in, C_out, k]
                              : W[((size_t)co * cin_real + ci) * kw + k]; // Conv1d [C_out, C_in, k]
        };
        std::vector<float> packed = c1_real < 32 ? pack_latent_conv_weights(wget, c_out)
                                    : ain       ? pack_conv_weights_split(wget, c_out, c1_pad + c2, ntaps)
                                                : pack_conv_weights(wget, c_out, c1_pad + c2, ntaps);
        UP(l.wfrag, packed);
        const bool chain_k5 = (L_in == 52 || L_in == 26) && c1_real == 64 && c2 == 0 && c_out == 64;
        l.wino_launch = wino1d_supported(L_in, c1_real, c2, c_out);
        if (!split && !transposed && stride == 1 && ntaps == 5 && epi == EPI_GN_MISH && (l.wino_launch || chain_k5)) {
            // F(4, 5) at the points {0, +-1, +-2, +-1/2, inf}: U[xi][ci][co] = sum_k G[xi][k] w[co][ci][k], in double
            static const double Gm[8][5] = {{-1, 0, 0, 0, 0},
                                            {-2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9},
                                            {-2.0 / 9, 2.0 / 9, -2.0 / 9, 2.0 / 9, -2.0 / 9},
                                            {1.0 / 90, 1.0 / 45, 2.0 / 45, 4.0 / 45, 8.0 / 45},
                                            {1.0 / 90, -1.0 / 45, 2.0 / 45, -4.0 / 45, 8.0 / 45},
                                            {32.0 / 45, 16.0 / 45, 8.0 / 45, 4.0 / 45, 2.0 / 45},
                                            {32.0 / 45, -16.0 / 45, 8.0 / 45, -4.0 / 45, 2.0 / 45},
                                            {0, 0, 0, 0, 1}};
            auto uget = [&](int co, int ci, int xi) -> float {
                double u = 0.0;
                for (int k = 0; k < 5; ++k) u += Gm[xi][k] * (double)W[((size_t)co * cin_real + ci) * kw + k];
                return (float)u;
            };
            std::vector<float> upacked = pack_conv_weights(uget, c_out, cin_real, 8);
            UP(l.ufrag, upacked);
            if (l.wino_launch) {      // wino1d_edge.hip: 12 planes per 16-channel chunk -- xi 0 .. 7, then the raw taps 0 .. 3 of the direct column
                auto eget = [&](int co, int ci, int pl) -> float { return pl < 8 ? uget(co, ci, pl) : W[((size_t)co * cin_real + ci) * kw + (pl - 8)]; };
                std::vector<float> epacked = pack_conv_weights(eget, c_out, cin_real, 12);
                UP(l.ufrag_edge, epacked);
            }
        }
        UP(l.bias, *getw(h, wname + ".bias"));
        if (epi == EPI_GN_MISH) {
            UP(l.gamma, *getw(h, gn_name + ".weight"));
            UP(l.beta, *getw(h, gn_name + ".bias"));
        }
        l.c_out = c_out; l.c1_real = c1_real; l.c1_pad = c1_pad; l.c2 = c2; l.ly = ly; l.off0 = off0; l.orow0 = orow0;
        l.g = ConvGeom{L_in, lm, stride, ntaps, 32, 4, 1, epi, c_out / 8, ostr, c1_real < 32 ? 1 : 0, ain, aout, 0};
        if (c2 > 0 && c2 != c1_real) return fail(h, CLD_ERR_ARG, "cld_finalize: concatenated sources must have equal channel counts");
        ConvGeom t = l.g;
        if (ain == 1 && stride == 1) t.kc = 64;
        l.has_a = conv_geom_supported(t);
        t.nwn = 2; t.ks = 2;
        l.has_b = conv_geom_supported(t);
        if (!l.has_a && !l.has_b)
            return fail(h, CLD_ERR_ARG, "cld_finalize: no kernel instance for layer '" + wname + "'");
        return CLD_OK;
    };
    static const int k5[5] = {0, 1, 2, 3, 4}, k3[3] = {0, 1, 2}, k1[1] = {0};
    static const int kT_even[2] = {3, 1}, kT_odd[2] = {2, 0};   // out[2j] = x[j-1] W3 + x[j] W1 ; out[2j+1] = x[j] W2 + x[j+1] W0
    int cb_off = 0, rc;
    for (int i = 0; i < 12; ++i) {
        const BlockDef& bd = kBlocks[i];
        ResBlock& rb = h->blocks[i];
        const std::string p = bd.name;
        const bool cat = (i == 8 || i == 10);
        const int c1 = cat ? bd.cin / 2 : bd.cin, c2 = cat ? bd.cin / 2 : 0;
        const bool latent_in = (i == 0);     // the 4-channel latent stays fp32 (its range is unbounded): exact-fp32 loop
        if ((rc = make_conv(rb.c0, p + ".blocks.0.block.0", bd.cout, c1, c2, bd.L, bd.L, 1, 5, k5, false, -2, 0, 1, bd.L,
                            EPI_GN_MISH, p + ".blocks.0.block.2", latent_in)) != CLD_OK) return rc;
        rb.c0.cb_off = cb_off;
        if ((rc = make_conv(rb.c1, p + ".blocks.1.block.0", bd.cout, bd.cout, 0, bd.L, bd.L, 1, 5, k5, false, -2, 0, 1,
                            bd.L, EPI_GN_MISH, p + ".blocks.1.block.2")) != CLD_OK) return rc;
        rb.has_res = bd.cin != bd.cout && !latent_in;
        if (rb.has_res)
            if ((rc = make_conv(rb.res, p + ".residual_conv", bd.cout, c1, c2, bd.L, bd.L, 1, 1, k1, false, 0, 0, 1, bd.L,
                                EPI_BIAS, "", latent_in)) != CLD_OK) return rc;
        if (rb.has_res && h->precision == CLD_PRECISION_F32 && wino1d_edge_res_supported(bd.L, bd.cout, c1, c2))
            UP(rb.res.rfrag, pack_res_proj(getw(h, p + ".residual_conv.weight")->data(), bd.cout, c1 + c2));
        if (latent_in) {      // the first block's 1x1 residual projection of the 4-channel latent runs inside its second conv's epilogue
            UP(h->res4_w, *getw(h, p + ".residual_conv.weight"));      // [64, 4, 1]
            UP(h->res4_b, *getw(h, p + ".residual_conv.bias"));
        }
        cb_off += bd.cout;
    }
    if ((rc = make_conv(h->down[0], "model.downs.0.2.conv", 64, 64, 0, 52, 26, 2, 3, k3, false, -1, 0, 1, 26, EPI_BIAS, ""))) return rc;
    if ((rc = make_conv(h->down[1], "model.downs.1.2.conv", 128, 128, 0, 26, 13, 2, 3, k3, false, -1, 0, 1, 13, EPI_BIAS, ""))) return rc;
    for (int u = 0; u < 2; ++u) {
        const std::string p = u == 0 ? "model.ups.0.2.conv" : "model.ups.1.2.conv";
        const int c = u == 0 ? 128 : 64, L = u == 0 ? 13 : 26;
        if ((rc = make_conv(h->upT[u][0], p, c, c, 0, L, L, 1, 2, kT_even, true, -1, 0, 2, 2 * L, EPI_BIAS, ""))) return rc;
        if ((rc = make_conv(h->upT[u][1], p, c, c, 0, L, L, 1, 2, kT_odd, true, 0, 1, 2, 2 * L, EPI_BIAS, ""))) return rc;
    }
    if ((rc = make_conv(h->final_cb, "model.final_conv.0.block.0", 64, 64, 0, 52, 52, 1, 5, k5, false, -2, 0, 1, 52,
                        EPI_GN_MISH, "model.final_conv.0.block.2", false, /*out_f32: the head kernel reads fp32*/ true))) return rc;

    // ---- cond half of every block's time_mlp Linear, concatenated: wc [1792][256], bias [1792] ----
    // ---- time half folded with the timestep embedding into a table tb [n_timesteps][1792]       ----
    {
        std::vector<float> wc((size_t)NCB * COND), bb(NCB);
        std::vector<float> wt((size_t)NCB * TE);
        int off = 0;
        for (const auto& bd : kBlocks) {
            const std::vector<float>& W = *getw(h, std::string(bd.name) + ".time_mlp.1.weight");   // [cout, 288]: [0:32] time, [32:288] cond
            const std::vector<float>& Bv = *getw(h, std::string(bd.name) + ".time_mlp.1.bias");
            for (int n = 0; n < bd.cout; ++n) {
                for (int k = 0; k < TE; ++k) wt[(size_t)(off + n) * TE + k] = W[(size_t)n * (TE + COND) + k];
                for (int k = 0; k < COND; ++k) wc[(size_t)(off + n) * COND + k] = W[(size_t)n * (TE + COND) + TE + k];
                bb[off + n] = Bv[n];
            }
            off += bd.cout;
        }
        UP(h->wc, wc);
        UP(h->cbias_b, bb);
        const std::vector<float>& W1 = *getw(h, "model.time_mlp.1.weight");   // [128,32]
        const std::vector<float>& B1 = *getw(h, "model.time_mlp.1.bias");
        const std::vector<float>& W3 = *getw(h, "model.time_mlp.3.weight");   // [32,128]
        const std::vector<float>& B3 = *getw(h, "model.time_mlp.3.bias");
        const int n = h->cfg.n_timesteps;
        std::vector<float> tb((size_t)n * NCB);
        const int half = TE / 2;
        const float negc = (float)(-(std::log(10000.0) / (half - 1)));
        for (int t = 0; t < n; ++t) {
            float emb[TE];
            for (int k = 0; k < half; ++k) {              // diffuser_helpers.py:25-32, fp32 like the reference
                const float wk = std::exp((float)k * negc);
                const float ph = (float)t * wk;
                emb[k] = std::sin(ph);
                emb[half + k] = std::cos(ph);
            }
            double h1[128], te[TE];
            for (int j = 0; j < 128; ++j) {
                double a = B1[j];
                for (int k = 0; k < TE; ++k) a += (double)W1[j * TE + k] * emb[k];
                h1[j] = mish_d((double)(float)a);
            }
            for (int j = 0; j < TE; ++j) {
                double a = B3[j];
                for (int k = 0; k < 128; ++k) a += (double)W3[j * 128 + k] * (double)(float)h1[k];
                te[j] = mish_d((double)(float)a);          // the block's Mish on the [t_emb | cond] vector
            }
            for (int nn = 0; nn < NCB; ++nn) {
                double a = 0;
                for (int k = 0; k < TE; ++k) a += (double)wt[(size_t)nn * TE + k] * (double)(float)te[k];
                tb[(size_t)t * NCB + nn] = (float)a;
            }
        }
        UP(h->tb, tb);
    }
    {
        std::vector<float> qs(h->sqrt_acp);
        qs.insert(qs.end(), h->sqrt_1m_acp.begin(), h->sqrt_1m_acp.end());
        UP(h->qs_tab, qs);
    }
    UP(h->head_w, *getw(h, "model.final_conv.1.weight"));
    UP(h->head_b, *getw(h, "model.final_conv.1.bias"));
    {   // final_conv.1 [4,64,1] as one 16-column N tile of the chain kernel (columns 4..15 zero)
        const std::vector<float>& W = *getw(h, "model.final_conv.1.weight");
        UP(h->head_wfrag, pack_conv_weights([&](int co, int ci, int) { return co < 4 ? W[(size_t)co * 64 + ci] : 0.f; }, 16, 64, 1));
    }
    return CLD_OK;
    };
    if (h->has_unet) {
        const int rcu = build_unet();
        if (rcu != CLD_OK) return rcu;
    }
    int rc = CLD_OK;

    // ---- decoder (optional) ---------------------------------------------------------------
    h->has_decoder = true;
    for (const auto& kv : h->expect)
        if (kv.first.rfind("lstm_dec.", 0) == 0 && !h->w.count(kv.first)) h->has_decoder = false;
    if (h->has_decoder) {
        float* tmp;
        UP(tmp, *getw(h, "lstm_dec.lstm.weight_ih_l0")); h->dec.w_ih0 = tmp;
        UP(tmp, *getw(h, "lstm_dec.lstm.weight_hh_l0")); h->dec.w_hh0 = tmp;
        UP(tmp, *getw(h, "lstm_dec.lstm.weight_ih_l1")); h->dec.w_ih1 = tmp;
        UP(tmp, *getw(h, "lstm_dec.lstm.weight_hh_l1")); h->dec.w_hh1 = tmp;
        std::vector<float> b0(256), b1(256);
        for (int i = 0; i < 256; ++i) {
            b0[i] = (*getw(h, "lstm_dec.lstm.bias_ih_l0"))[i] + (*getw(h, "lstm_dec.lstm.bias_hh_l0"))[i];
            b1[i] = (*getw(h, "lstm_dec.lstm.bias_ih_l1"))[i] + (*getw(h, "lstm_dec.lstm.bias_hh_l1"))[i];
        }
        UP(tmp, b0); h->dec.b0 = tmp;
        UP(tmp, b1); h->dec.b1 = tmp;
        UP(tmp, *getw(h, "lstm_dec.cond2hidden.weight")); h->dec.w_c2h = tmp;
        UP(tmp, *getw(h, "lstm_dec.cond2hidden.bias")); h->dec.b_c2h = tmp;
        UP(tmp, *getw(h, "lstm_dec.hid2act.weight")); h->dec.w_h2a = tmp;
        UP(tmp, *getw(h, "lstm_dec.hid2act.bias")); h->dec.b_h2a = tmp;
        {   // B fragments of the backward products of guide_mfma8_kernel (guide_kernels.hip): wave wv owns units 8 wv .. 8 wv + 7;
            // tile 0 = layer 1: column n < 8 -> W_hh1[col][8 wv + n], n >= 8 -> W_ih1[col][8 wv + n - 8];
            // tile 1 = layer 0: column n < 8 -> W_hh0[col][8 wv + n], 8 <= n < 12 -> W_ih0[col][n - 8], else 0;
            // k-step (j, e) of lane (n, rb) is gate column col = 16 j + 4 rb + e.  One coalesced float4 per (tile, j) and lane.
            const std::vector<float>&hh1 = *getw(h, "lstm_dec.lstm.weight_hh_l1"), &ih1 = *getw(h, "lstm_dec.lstm.weight_ih_l1"),
                                    &hh0 = *getw(h, "lstm_dec.lstm.weight_hh_l0"), &ih0 = *getw(h, "lstm_dec.lstm.weight_ih_l0");
            std::vector<float> g((size_t)8 * 2 * 16 * 64 * 4);
            size_t o = 0;
            for (int wv = 0; wv < 8; ++wv)
                for (int tile = 0; tile < 2; ++tile)
                    for (int j = 0; j < 16; ++j)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int e = 0; e < 4; ++e) {
                                const int n = lane & 15, rb = lane >> 4, hi = n >> 3, m = n & 7, col = 16 * j + 4 * rb + e;
                                float v;
                                if (tile == 0) v = (hi ? ih1 : hh1)[(size_t)col * 64 + 8 * wv + m];
                                else v = hi ? (m < 4 ? ih0[(size_t)col * 4 + m] : 0.f) : hh0[(size_t)col * 64 + 8 * wv + m];
                                g[o++] = v;
                            }
            UP(tmp, g); h->dec.gfrag = tmp;
            // B operands of the backward products of guide_quad_kernel: waves wv and wv + 4 own units 16 wv .. 16 wv + 15; lane = 4 block + column,
            // block = (K half kh << 3) | (product m << 2) | unit quad ub; k-step (j, e) is gate column col = 128 kh + 4 j + e;
            // layer 1 (first): m = 0 -> W_hh1[col][16 wv + 4 ub + row], m = 1 -> W_ih1[col][same];
            // layer 0: m = 0 -> W_hh0[col][same], m = 1 and ub = 0 -> W_ih0[col][latent channel row], else 0
            std::vector<float> gq((size_t)4 * 2 * 32 * 64 * 4);
            o = 0;
            for (int wv = 0; wv < 4; ++wv)
                for (int layer = 1; layer >= 0; --layer)
                    for (int j = 0; j < 32; ++j)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int e = 0; e < 4; ++e) {
                                const int row = lane & 3, blk = lane >> 2, kh = blk >> 3, m = (blk >> 2) & 1, ub = blk & 3;
                                const int col = 128 * kh + 4 * j + e, unit = 16 * wv + 4 * ub + row;
                                float v;
                                if (layer == 1) v = (m ? ih1 : hh1)[(size_t)col * 64 + unit];
                                else v = m ? (ub == 0 ? ih0[(size_t)col * 4 + row] : 0.f) : hh0[(size_t)col * 64 + unit];
                                gq[o++] = v;
                            }
            UP(tmp, gq); h->dec.gqfrag = tmp;
        }
    }
    // ---- encoder (optional) ---------------------------------------------------------------
    h->has_encoder = true;
    for (const auto& kv : h->expect)
        if ((kv.first.rfind("lstm_enc.", 0) == 0 || kv.first.rfind("mu.", 0) == 0 || kv.first.rfind("logvar.", 0) == 0) &&
            !h->w.count(kv.first))
            h->has_encoder = false;
    if (h->has_encoder) {
        float* tmp;
        UP(tmp, *getw(h, "lstm_enc.lstm.weight_ih_l0")); h->enc.w_ih0 = tmp;
        UP(tmp, *getw(h, "lstm_enc.lstm.weight_hh_l0")); h->enc.w_hh0 = tmp;
        UP(tmp, *getw(h, "lstm_enc.lstm.weight_ih_l1")); h->enc.w_ih1 = tmp;
        UP(tmp, *getw(h, "lstm_enc.lstm.weight_hh_l1")); h->enc.w_hh1 = tmp;
        std::vector<float> b0(256), b1(256);
        for (int i = 0; i < 256; ++i) {
            b0[i] = (*getw(h, "lstm_enc.lstm.bias_ih_l0"))[i] + (*getw(h, "lstm_enc.lstm.bias_hh_l0"))[i];
            b1[i] = (*getw(h, "lstm_enc.lstm.bias_ih_l1"))[i] + (*getw(h, "lstm_enc.lstm.bias_hh_l1"))[i];
        }
        UP(tmp, b0); h->enc.b0 = tmp;
        UP(tmp, b1); h->enc.b1 = tmp;
        UP(tmp, *getw(h, "lstm_enc.cond2hidden.weight")); h->enc.w_c2h = tmp;
        UP(tmp, *getw(h, "lstm_enc.cond2hidden.bias")); h->enc.b_c2h = tmp;
        UP(tmp, *getw(h, "mu.weight")); h->enc.w_mu = tmp;
        UP(tmp, *getw(h, "mu.bias")); h->enc.b_mu = tmp;
        UP(tmp, *getw(h, "logvar.weight")); h->enc.w_lv = tmp;
        UP(tmp, *getw(h, "logvar.bias")); h->enc.b_lv = tmp;
    }
    // ---- ContextEncoder (optional) -----------------------------------------------------------
    h->has_context = true;
    for (const auto& kv : h->expect)
        if (kv.first.rfind("context_encoder.", 0) == 0 && !h->w.count(kv.first)) h->has_context = false;
    if (h->has_context) {
        // eval-mode BatchNorm2d folded to y = x * scale + shift (eps 1e-5, torchvision resnet.py norm_layer default)
        auto fold_bn = [&](const std::string& p, float** scale, float** shift) -> int {
            const std::vector<float>&g = *getw(h, p + ".weight"), &b = *getw(h, p + ".bias"), &m = *getw(h, p + ".running_mean"),
                                    &v = *getw(h, p + ".running_var");
            std::vector<float> sc(g.size()), sh(g.size());
            for (size_t i = 0; i < g.size(); ++i) {
                const double k = (double)g[i] / std::sqrt((double)v[i] + 1e-5);
                sc[i] = (float)k;
                sh[i] = (float)((double)b[i] - (double)m[i] * k);
            }
            UP(*scale, sc);
            UP(*shift, sh);
            return CLD_OK;
        };
        const std::string r = kResnet;
        {   // stem: per input plane c the 49 taps are 13 MFMA k-steps (k = 4 q + (lane >> 4)); lane holds 4 k-steps per float4
            const std::vector<float>& W = *getw(h, r + "conv1.weight");     // [64][34][7][7]
            std::vector<float> wq((size_t)34 * 4 * 4 * 64 * 4);
            size_t o = 0;
            for (int c = 0; c < 34; ++c)
                for (int qg = 0; qg < 4; ++qg)
                    for (int nt = 0; nt < 4; ++nt)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int sidx = 0; sidx < 4; ++sidx) {
                                const int k = 4 * (4 * qg + sidx) + (lane >> 4);
                                wq[o++] = k < 49 ? W[((size_t)(16 * nt + (lane & 15)) * 34 + c) * 49 + k] : 0.f;
                            }
            UP(h->stem_w, wq);
            if ((rc = fold_bn(r + "bn1", &h->stem_scale, &h->stem_shift)) != CLD_OK) return rc;
        }
        auto make2d = [&](cld_handle_s::Conv2dLayer& l, const std::string& wname, const std::string& bnname, int kh, int stride,
                          int hin, int cin, int cout) -> int {
            const std::vector<float>& W = *getw(h, wname);                  // [cout][cin][kh][kh]
            auto wget = [&](int co, int ci, int t) -> float { return W[((size_t)co * cin + ci) * kh * kh + t]; };
            std::vector<float> packed = pack_conv_weights(wget, cout, cin, kh * kh);
            UP(l.wfrag, packed);
            l.kh = kh; l.stride = stride; l.hin = hin; l.cin = cin; l.cout = cout;
            if (kh == 3 && stride == 1 && cin == cout && wino44_supported(hin, cout)) {
                // Winograd F(4x4, 3x3) at the points {0, 1, -1, 1/2, -2, inf} (wino44_kernels.hip): U[xi = 6 i + j] = (G g G^T)[i][j], in double
                static const double G6[6][3] = {{1, 0, 0}, {1.0 / 3, 1.0 / 3, 1.0 / 3}, {-1.0 / 3, 1.0 / 3, -1.0 / 3},
                                                {-16.0 / 15, -8.0 / 15, -4.0 / 15}, {1.0 / 15, -2.0 / 15, 4.0 / 15}, {0, 0, 1}};
                std::vector<float> U6((size_t)36 * cin * cout);
                for (int co = 0; co < cout; ++co)
                    for (int ci = 0; ci < cin; ++ci) {
                        const float* g = &W[((size_t)co * cin + ci) * 9];
                        double t[6][3];
                        for (int i = 0; i < 6; ++i)
                            for (int bb = 0; bb < 3; ++bb) t[i][bb] = G6[i][0] * g[bb] + G6[i][1] * g[3 + bb] + G6[i][2] * g[6 + bb];
                        for (int i = 0; i < 6; ++i)
                            for (int j = 0; j < 6; ++j)
                                U6[((size_t)(6 * i + j) * cin + ci) * cout + co] = (float)(t[i][0] * G6[j][0] + t[i][1] * G6[j][1] + t[i][2] * G6[j][2]);
                    }
                auto u6get = [&](int co, int ci, int xi) -> float { return U6[((size_t)xi * cin + ci) * cout + co]; };
                std::vector<float> u6packed = pack_conv_weights(u6get, cout, cin, 36);
                UP(l.ufrag44, u6packed);
            }
            return fold_bn(bnname, &l.scale, &l.shift);
        };
        int cin = 64, hin = 56;
        for (int li = 1; li <= 4; ++li) {
            const int c = 32 << li;
            for (int b = 0; b < 2; ++b) {
                const std::string p = r + "layer" + std::to_string(li) + "." + std::to_string(b);
                const int stride = (b == 0 && li > 1) ? 2 : 1;
                const int hout = hin / stride;
                if ((rc = make2d(h->rn_conv[li - 1][b][0], p + ".conv1.weight", p + ".bn1", 3, stride, hin, b == 0 ? cin : c, c))) return rc;
                if ((rc = make2d(h->rn_conv[li - 1][b][1], p + ".conv2.weight", p + ".bn2", 3, 1, hout, c, c))) return rc;
                if (b == 0 && cin != c)
                    if ((rc = make2d(h->rn_ds[li - 1], p + ".downsample.0.weight", p + ".downsample.1", 1, 2, hin, cin, c))) return rc;
                hin = hout;
            }
            cin = c;
        }
        // head: transposed Linear weights [in][out]
        auto upT = [&](const std::string& wname, const float** dst) -> int {
            const std::vector<float>& W = *getw(h, wname);
            const std::string bname = wname.substr(0, wname.size() - 6) + "bias";
            const size_t n_out = getw(h, bname)->size(), n_in = W.size() / n_out;
            std::vector<float> t(W.size());
            for (size_t o = 0; o < n_out; ++o)
                for (size_t i = 0; i < n_in; ++i) t[i * n_out + o] = W[o * n_in + i];
            float* d; UP(d, t); *dst = d;
            return CLD_OK;
        };
        auto up1 = [&](const std::string& name, const float** dst) -> int { float* d; UP(d, *getw(h, name)); *dst = d; return CLD_OK; };
        ContextHeadArgs& a = h->ctx_head;
        if ((rc = upT(r + "fc.weight", &a.fc_wt)) || (rc = up1(r + "fc.bias", &a.fc_b))) return rc;
        const std::string sp = "context_encoder.agent_state_encoder._model.", cp = "context_encoder.process_cond_mlp._model.";
        for (int i = 0; i < 3; ++i) {
            if ((rc = upT(sp + std::to_string(3 * i) + ".weight", &a.s_wt[i])) || (rc = up1(sp + std::to_string(3 * i) + ".bias", &a.s_b[i]))) return rc;
            if (i < 2 && ((rc = up1(sp + std::to_string(3 * i + 1) + ".weight", &a.s_g[i])) || (rc = up1(sp + std::to_string(3 * i + 1) + ".bias", &a.s_be[i])))) return rc;
        }
        for (int i = 0; i < 5; ++i) {
            if ((rc = upT(cp + std::to_string(3 * i) + ".weight", &a.c_wt[i])) || (rc = up1(cp + std::to_string(3 * i) + ".bias", &a.c_b[i]))) return rc;
            if (i < 4 && ((rc = up1(cp + std::to_string(3 * i + 1) + ".weight", &a.c_g[i])) || (rc = up1(cp + std::to_string(3 * i + 1) + ".bias", &a.c_be[i])))) return rc;
        }
    }
#undef UP
    HIPCK(h, hipStreamSynchronize(s));     // host staging vectors die with this scope
    h->w.clear();
    h->finalized = true;
    return CLD_OK;
}

size_t cld_workspace_bytes(cld_handle h, int32_t B) {
    if (!h || B < 1) return 0;
    return ws_floats(pad16(B)) * sizeof(float);
}

int cld_get_schedule(cld_handle h, float* x_t_cof, float* noise_cof, float* post_log_var) {
    if (!h) return CLD_ERR_ARG;
    const size_t n = h->x_t_cof.size() * sizeof(float);
    if (x_t_cof) std::memcpy(x_t_cof, h->x_t_cof.data(), n);
    if (noise_cof) std::memcpy(noise_cof, h->noise_cof.data(), n);
    if (post_log_var) std::memcpy(post_log_var, h->plvc.data(), n);
    return CLD_OK;
}

static int check_common(cld_handle h, const char* fn, int B, int t_idx, const void* ws, size_t ws_bytes) {
    if (!h) return CLD_ERR_ARG;
    if (!h->finalized) return fail(h, CLD_ERR_STATE, std::string(fn) + ": weights not finalized");
    if (!h->has_unet && std::string(fn) != "cld_guidance_step") return fail(h, CLD_ERR_STATE, std::string(fn) + ": U-Net weights (model.*) not loaded");
    if (B < 1) return fail(h, CLD_ERR_ARG, std::string(fn) + ": B < 1");
    if (t_idx < 0 || t_idx >= h->cfg.n_timesteps) return fail(h, CLD_ERR_ARG, std::string(fn) + ": timestep out of range");
    if (!ws || ws_bytes < cld_workspace_bytes(h, B)) return fail(h, CLD_ERR_WORKSPACE, std::string(fn) + ": workspace too small");
    if (reinterpret_cast<uintptr_t>(ws) % 16) return fail(h, CLD_ERR_ARG, std::string(fn) + ": workspace must be 16-byte aligned");
    return CLD_OK;
}

int cld_unet_forward(cld_handle h, const float* x, const float* cond, int32_t t_idx, float* eps, int32_t B,
                     void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_common(h, "cld_unet_forward", B, t_idx, workspace, workspace_bytes);
    if (rc) return rc;
    if (!x || !cond || !eps) return fail(h, CLD_ERR_ARG, "cld_unet_forward: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int bp = pad16(B);
    Ws w = carve(workspace, bp);
    if ((rc = load_inputs(h, w, B, bp, x, cond, nullptr, false, s)) != CLD_OK) return rc;
    HIPCK(h, run_unet(h, w, w.xw, t_idx, bp, s));
    HeadArgs a{};
    head_source(h, w, a); a.w = h->head_w; a.b = h->head_b; a.x = w.xw; a.eps_out = eps; a.B = B; a.b_pad = bp;
    HIPCK(h, launch_head(a, s));
    return CLD_OK;
}

int cld_unet_forward_t(cld_handle h, const float* x, const float* cond, const int32_t* t_idx, float* eps, int32_t B,
                       void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_common(h, "cld_unet_forward_t", B, 0, workspace, workspace_bytes);
    if (rc) return rc;
    if (!x || !cond || !t_idx || !eps) return fail(h, CLD_ERR_ARG, "cld_unet_forward_t: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int bp = pad16(B);
    Ws w = carve(workspace, bp);
    if ((rc = load_inputs(h, w, B, bp, x, cond, nullptr, false, s)) != CLD_OK) return rc;
    HIPCK(h, launch_add_time_bias(w.cb, h->tb, t_idx, h->cfg.n_timesteps, B, NCB, s));
    HIPCK(h, run_unet(h, w, w.xw, -1, bp, s));
    HeadArgs a{};
    head_source(h, w, a); a.w = h->head_w; a.b = h->head_b; a.x = w.xw; a.eps_out = eps; a.B = B; a.b_pad = bp;
    HIPCK(h, launch_head(a, s));
    return CLD_OK;
}

int cld_debug_unet_span(cld_handle h, int32_t span, const float* x1, const float* x2, const float* cond, int32_t t_idx,
                        const int32_t* t_rows, float* y, int32_t B, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_common(h, "cld_debug_unet_span", B, t_rows ? 0 : t_idx, workspace, workspace_bytes);
    if (rc) return rc;
    if (span < 0 || span >= kSpans) return fail(h, CLD_ERR_ARG, "cld_debug_unet_span: span must be 0..11");
    if (!x1 || !cond || !y || (kSpanSkip[span] >= 0) != (x2 != nullptr))
        return fail(h, CLD_ERR_ARG, "cld_debug_unet_span: null pointer (x2: spans 8 and 11 only, and required there)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int bp = pad16(B);
    Ws w = carve(workspace, bp);
    const bool s22 = h->precision == CLD_PRECISION_F16X2;
    const long n_in = (long)kSpanL[span] * kSpanC[span];
    if (span == 0) HIPCK(h, launch_pack_latent(x1, w.xw, B, bp, s));
    else HIPCK(h, launch_act_pack(x1, w.buf[kSpanIn[span]], B, bp, n_in, s22, s));
    if (x2) HIPCK(h, launch_act_pack(x2, w.buf[kSpanSkip[span]], B, bp, n_in, s22, s));
    HIPCK(h, launch_cond_bias(cond, h->wc, h->cbias_b, w.cb, B, bp, NCB, s));
    if (t_rows) HIPCK(h, launch_add_time_bias(w.cb, h->tb, t_rows, h->cfg.n_timesteps, B, NCB, s));
    h->launch_counter = 0;
    set_lds_floor(h->lds_floor);
    HIPCK(h, run_unet_span(h, w, w.xw, t_rows ? -1 : t_idx, bp, span, s));
    if (span == kSpans - 1) {
        HeadArgs a{};
        head_source(h, w, a); a.w = h->head_w; a.b = h->head_b; a.x = w.xw; a.eps_out = y; a.B = B; a.b_pad = bp;
        HIPCK(h, launch_head(a, s));
    } else {
        HIPCK(h, launch_act_unpack(w.buf[kSpanOut[span]], y, B, (long)kSpanL[span + 1] * kSpanC[span + 1], s22, s));
    }
    return CLD_OK;
}

int cld_denoise_loss(cld_handle h, const float* z0, const float* noise, const float* cond, const int32_t* t_idx, float* z_noisy,
                     float* mse, int32_t B, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_common(h, "cld_denoise_loss", B, 0, workspace, workspace_bytes);
    if (rc) return rc;
    if (!z0 || !noise || !t_idx || (!mse && !z_noisy) || (mse && !cond)) return fail(h, CLD_ERR_ARG, "cld_denoise_loss: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int bp = pad16(B);
    Ws w = carve(workspace, bp);
    // z_t = sqrt(acp[t]) z0 + sqrt(1 - acp[t]) noise  (q_sample, dm_model.py:91-96) straight into the padded latent buffer
    HIPCK(h, launch_q_sample(z0, noise, t_idx, h->qs_tab, h->cfg.n_timesteps, w.xw, z_noisy, B, bp, s));
    if (!mse) return CLD_OK;               // q_sample alone (dm_model.py:91-96): no U-Net evaluation
    HIPCK(h, launch_cond_bias(cond, h->wc, h->cbias_b, w.cb, B, bp, NCB, s));
    HIPCK(h, launch_add_time_bias(w.cb, h->tb, t_idx, h->cfg.n_timesteps, B, NCB, s));
    HIPCK(h, run_unet(h, w, w.xw, -1, bp, s));
    HeadArgs a{};
    head_source(h, w, a); a.w = h->head_w; a.b = h->head_b; a.x = w.xw; a.eps_out = w.xtmp; a.B = B; a.b_pad = bp;
    HIPCK(h, launch_head(a, s));
    HIPCK(h, launch_mse_rows(noise, w.xtmp, mse, B, s));
    return CLD_OK;
}

int cld_ddpm_step(cld_handle h, const float* x, const float* cond, int32_t t_idx, const float* z, float* x_next,
                  float* mean, float* sigma_host, int32_t B, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_common(h, "cld_ddpm_step", B, t_idx, workspace, workspace_bytes);
    if (rc) return rc;
    if (!x || !cond) return fail(h, CLD_ERR_ARG, "cld_ddpm_step: null pointer");      // z NULL: the generator, seed 0 / step 0 (a{} below)
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int bp = pad16(B);
    Ws w = carve(workspace, bp);
    const float sigma = std::exp(0.5f * h->plvc[t_idx]);
    if (sigma_host) *sigma_host = sigma;
    if ((rc = load_inputs(h, w, B, bp, x, cond, nullptr, false, s)) != CLD_OK) return rc;
    HIPCK(h, run_unet(h, w, w.xw, t_idx, bp, s));
    HeadArgs a{};
    head_source(h, w, a); a.w = h->head_w; a.b = h->head_b; a.x = w.xw; a.z = z; a.B = B; a.b_pad = bp;
    a.mean_out = w.meanb; a.x_out = w.xtmp;
    a.xc = h->x_t_cof[t_idx]; a.nc = h->noise_cof[t_idx];
    a.sg = (t_idx == 0) ? 0.f : sigma;       // nonzero_mask, dm_model.py:151
    HIPCK(h, launch_head(a, s));
    if (x_next) HIPCK(h, launch_unpack(w.xtmp, x_next, B, s));
    if (mean) HIPCK(h, launch_unpack(w.meanb, mean, B, s));
    return CLD_OK;
}

static int check_collision(cld_handle h, const char* fn, const cld_collision* c, int B) {
    if (!c->extent || !c->world_from_agent || !c->curr_speed || !c->scene_start) return fail(h, CLD_ERR_ARG, std::string(fn) + ": collision term: null pointer");
    if (c->num_scenes < 1 || c->num_samp < 1 || B % c->num_samp) return fail(h, CLD_ERR_ARG, std::string(fn) + ": collision term: B must be agents x num_samp, num_scenes >= 1");
    if (c->num_disks < 1 || c->num_disks > 8) return fail(h, CLD_ERR_ARG, std::string(fn) + ": collision term: num_disks must be 1..8");
    // 192: the largest scene whose poses fit launch_agent_collision's 160-KiB LDS request (163,664 B; 193 agents would need 164,512)
    if (c->max_scene_agents < 1 || c->max_scene_agents > 192) return fail(h, CLD_ERR_ARG, std::string(fn) + ": collision term: scenes of 1..192 agents");
    return CLD_OK;
}
static CollisionArgs collision_args(const cld_collision* c, const float* traj, const float* grad_in, float* loss, float* grad, int B) {
    CollisionArgs a{};
    a.traj = traj; a.extent = c->extent; a.world_from_agent = c->world_from_agent; a.curr_speed = c->curr_speed;
    a.scene_start = c->scene_start; a.scene_weight = c->scene_weight; a.guided = c->guided; a.excluded = c->excluded; a.max_scene_agents = c->max_scene_agents; a.grad_in = grad_in;
    a.loss = loss; a.grad = grad; a.B_agents = B / c->num_samp; a.num_scenes = c->num_scenes; a.num_samp = c->num_samp;
    a.num_disks = c->num_disks; a.buffer_dist = c->buffer_dist; a.decay_rate = c->decay_rate; a.moving_speed_th = c->moving_speed_th;
    return a;
}

static int check_map_collision(cld_handle h, const char* fn, const cld_map_collision* c, int B) {
    if (!c->extent || !c->raster_from_agent || !c->curr_speed || !c->scene_start)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": map collision term: null pointer");
    if (!c->drivable_map && !h->has_map_source)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": map collision term: drivable_map is NULL and no map source is set (cld_set_map_source)");
    if (!c->drivable_map && h->map_source.num_scenes != c->num_scenes)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": map collision term: the map source holds " + std::to_string(h->map_source.num_scenes) +
                                        " scenes, the term " + std::to_string(c->num_scenes));
    if (c->num_scenes < 1 || c->num_samp < 1 || B % c->num_samp || c->H < 1 || c->W < 1)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": map collision term: B must be agents x num_samp, a map of H x W >= 1");
    if (c->num_points_l < 1 || c->num_points_w < 1 || c->num_points_l * c->num_points_w > 256)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": map collision term: 1..256 sample points per box");
    return CLD_OK;
}
static MapCollisionArgs map_args(cld_handle h, const cld_map_collision* c, const float* traj, const float* grad_in, float* loss, float* grad) {
    MapCollisionArgs a{};
    if (!c->drivable_map && h->has_map_source) {     // map mode; with a drivable_map the source is ignored
        const cld_map_source& m = h->map_source;
        a.maps = m.maps; a.scene_map = m.scene_map; a.map_from_world = m.map_from_world; a.world = m.world;
        a.num_maps = m.num_maps; a.n_sem = m.n_sem; a.map_h = m.map_h; a.map_w = m.map_w; a.layer = m.drivable_layer;
        a.ppm = m.px_per_m; a.ox = (1.f + m.ego_center[0]) * 0.5f * (float)c->W; a.oy = (1.f + m.ego_center[1]) * 0.5f * (float)c->H;      // cld_rasterize's offsets
        a.fill = m.no_map_fill;
    }
    a.traj = traj; a.extent = c->extent; a.raster_from_agent = c->raster_from_agent; a.drivable_map = c->drivable_map;
    a.curr_speed = c->curr_speed; a.scene_start = c->scene_start; a.scene_weight = c->scene_weight; a.grad_in = grad_in;
    a.loss = loss; a.grad = grad; a.num_scenes = c->num_scenes; a.num_samp = c->num_samp; a.H = c->H; a.W = c->W;
    a.num_points_l = c->num_points_l; a.num_points_w = c->num_points_w; a.decay_rate = c->decay_rate; a.moving_speed_th = c->moving_speed_th;
    return a;
}

static int check_goal(cld_handle h, const char* fn, const cld_goal* g, int B) {
    if (!g->target_pos || !g->agent_from_world || !g->kind || !g->target_time || !g->urgency || !g->pref_speed || !g->scale)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": goal term: null pointer");
    if (g->num_samp < 1 || B % g->num_samp) return fail(h, CLD_ERR_ARG, std::string(fn) + ": goal term: B must be agents x num_samp");
    return CLD_OK;
}
static GoalArgs goal_args(const cld_goal* g, const float* traj, const float* grad_in, float* loss, float* grad, int B) {
    GoalArgs a{};
    a.traj = traj; a.target_pos = g->target_pos; a.agent_from_world = g->agent_from_world; a.kind = g->kind; a.target_time = g->target_time;
    a.urgency = g->urgency; a.pref_speed = g->pref_speed; a.scale = g->scale; a.reached = g->reached; a.grad_in = grad_in;
    a.loss = loss; a.grad = grad; a.rows = B; a.num_samp = g->num_samp; a.global_t = g->global_t; a.dt = g->dt;
    a.min_progress_dist = g->min_progress_dist;
    return a;
}

// `iters` / `opt_steps`: the evaluations (loop iterations x optimiser steps) caller draws have to cover; 0 = the stand-alone loss (slab [0, 0])
static int check_social(cld_handle h, const char* fn, const cld_social_group* t, int B, int iters, int opt_steps) {
    if (!t->group_start || !t->member || !t->leader || !t->social_dist || !t->cohesion || !t->scale || !t->world_from_agent)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": social-group term: null pointer");
    if (t->num_groups < 1 || t->num_samp < 1 || B % t->num_samp || (int64_t)t->num_groups * t->num_samp > INT32_MAX)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": social-group term: B must be agents x num_samp, num_groups >= 1");
    if (t->max_members < 2 || t->max_members > kSocialMaxMembers)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": social-group term: groups of 2.." + std::to_string(kSocialMaxMembers) + " members");
    if ((t->draw_r == nullptr) != (t->draw_u == nullptr))
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": social-group term: draw_r and draw_u go together (both or neither)");
    if (t->draw_r && (t->n_iter < std::max(iters, 1) || t->n_opt < std::max(opt_steps, 1)))
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": social-group term: caller draws [" + std::to_string(t->n_iter) + ", " + std::to_string(t->n_opt) +
                                        ", B, 52] do not cover the call's " + std::to_string(std::max(iters, 1)) + " iterations x " +
                                        std::to_string(std::max(opt_steps, 1)) + " optimiser steps");
    return CLD_OK;
}
// evaluation (it, k): loop iteration `it` of the call, optimiser step k (from 0)
static SocialArgs social_args(const cld_social_group* t, const float* traj, float* loss, float* grad, int B, int it, int k) {
    SocialArgs a{};
    a.traj = traj; a.world_from_agent = t->world_from_agent; a.group_start = t->group_start; a.member = t->member; a.leader = t->leader;
    a.social_dist = t->social_dist; a.cohesion = t->cohesion; a.scale = t->scale;
    if (t->draw_r) {
        const size_t off = ((size_t)it * t->n_opt + k) * B * 52;
        a.draw_r = t->draw_r + off; a.draw_u = t->draw_u + off;
    }
    a.loss = loss; a.grad = grad; a.rows = B; a.num_groups = t->num_groups; a.num_samp = t->num_samp; a.max_members = t->max_members;
    a.seed = t->seed; a.eval = ((unsigned long long)(uint32_t)(t->iter_base + it) << 16) | (unsigned long long)k;
    return a;
}

static int check_pair(cld_handle h, const char* fn, const cld_pair_term* t, int B) {
    if (!t->target || !t->ref || !t->kind || !t->lo || !t->hi || !t->decay || !t->scale || !t->world_from_agent || !t->agent_start || !t->agent_id || !t->incidence)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": pair term: null pointer");
    if (t->num_pairs < 1 || t->num_samp < 1 || B % t->num_samp)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": pair term: B must be agents x num_samp, num_pairs >= 1");
    // an agent is listed once and a pair has two ends: at most 2 num_pairs involved agents and incidences
    if (t->num_involved < 0 || t->num_incidences < 0 || t->num_involved > B / t->num_samp || (int64_t)t->num_involved > 2 * (int64_t)t->num_pairs ||
        (int64_t)t->num_incidences > 2 * (int64_t)t->num_pairs)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": pair term: num_involved / num_incidences exceed what num_pairs pairs of the batch's agents can give");
    if ((int64_t)t->num_pairs * t->num_samp > INT32_MAX / 64 || (int64_t)t->num_involved * t->num_samp * 52 > INT32_MAX)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": pair term: too many pairs for one launch");
    return CLD_OK;
}
static PairArgs pair_args(const cld_pair_term* t, const float* traj, float* value, float* grad, int B) {
    PairArgs a{};
    a.traj = traj; a.world_from_agent = t->world_from_agent; a.agent_from_world = t->agent_from_world; a.target = t->target; a.ref = t->ref;
    a.kind = t->kind; a.lo = t->lo; a.hi = t->hi; a.decay = t->decay; a.scale = t->scale; a.agent_start = t->agent_start; a.agent_id = t->agent_id;
    a.incidence = t->incidence; a.value = value; a.grad = grad; a.rows = B; a.num_pairs = t->num_pairs; a.num_samp = t->num_samp;
    a.num_involved = t->num_involved; a.num_incidences = t->num_incidences;
    return a;
}

static int check_lane(cld_handle h, const char* fn, const cld_lane_term* t, int B) {
    if (!t->lines || !t->agent || !t->line || !t->kind || !t->decay || !t->scale)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": lane term: null pointer");
    if (t->num_entries < 1 || t->num_lines < 1 || t->num_samp < 1 || B % t->num_samp)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": lane term: B must be agents x num_samp, num_entries >= 1, num_lines >= 1");
    if (t->max_pts < 2 || t->max_pts > CLD_LANE_MAX_PTS)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": lane term: max_pts must be 2 .. " + std::to_string(CLD_LANE_MAX_PTS));
    if ((int64_t)t->num_entries * t->num_samp > INT32_MAX)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": lane term: too many entries for one launch");
    return CLD_OK;
}
static LaneArgs lane_args(const cld_lane_term* t, const float* traj, float* value, float* proj, float* grad, int B) {
    LaneArgs a{};
    a.traj = traj; a.lines = t->lines; a.agent = t->agent; a.line = t->line; a.kind = t->kind; a.decay = t->decay; a.scale = t->scale;
    a.value = value; a.proj = proj; a.grad = grad; a.rows = B; a.num_entries = t->num_entries; a.num_lines = t->num_lines; a.max_pts = t->max_pts;
    a.num_samp = t->num_samp;
    return a;
}

// The plan-space terms -- functions of the decoded plans of the current iterate, chained through the gradient buffer in THIS order
// (run_guidance) -- that a guided call on (handle, guidance) evaluates.  A new term: a bit here, its *_args() builder and check_*()
// above, a line in check_guidance and a block in run_guidance's chain.
enum : unsigned { TERM_COLLISION = 1, TERM_MAP = 2, TERM_GOAL = 4, TERM_SOCIAL = 8, TERM_PAIR = 16, TERM_LANE = 32 };
static unsigned plan_terms(cld_handle h, const cld_guidance* gd) {
    return (gd->collision ? TERM_COLLISION : 0u) | (gd->map_collision ? TERM_MAP : 0u) | (h->has_goal ? TERM_GOAL : 0u) |
           (h->has_social ? TERM_SOCIAL : 0u) | (h->has_pair ? TERM_PAIR : 0u) | (h->has_lane ? TERM_LANE : 0u);
}

static int check_guidance(cld_handle h, const char* fn, const cld_guidance* gd, int B, int iters = 1) {
    if (!h->has_decoder) return fail(h, CLD_ERR_STATE, std::string(fn) + ": guidance needs the decoder weights");
    const unsigned terms = plan_terms(h, gd);
    if (!gd->curr_states || (!terms && !gd->target_speed && !gd->speed_limit_scale && !gd->acc_limit_scale && !gd->target_pos_scale && !gd->ext_grad))
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": guidance needs curr_states and at least one loss term");
    int rc;
    if ((terms & TERM_COLLISION) && (rc = check_collision(h, fn, gd->collision, B))) return rc;
    if ((terms & TERM_MAP) && (rc = check_map_collision(h, fn, gd->map_collision, B))) return rc;
    if ((terms & TERM_GOAL) && (rc = check_goal(h, fn, &h->goal, B))) return rc;
    if (gd->grad_steps < 0 || gd->final_grad_steps < 0 || gd->grad_steps > 64 || gd->final_grad_steps > 64)      // (what the social term's draws are checked against)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": grad_steps out of range (0..64)");
    if ((terms & TERM_SOCIAL) && (rc = check_social(h, fn, &h->social, B, iters, std::max(gd->grad_steps, gd->final_grad_steps)))) return rc;
    if ((terms & TERM_PAIR) && (rc = check_pair(h, fn, &h->pair, B))) return rc;
    if ((terms & TERM_LANE) && (rc = check_lane(h, fn, &h->lane, B))) return rc;
    if (gd->optimizer != CLD_GUIDE_ADAM && gd->optimizer != CLD_GUIDE_SGD) return fail(h, CLD_ERR_ARG, std::string(fn) + ": unknown optimizer");
    if (gd->apply_output && gd->final_optimizer != CLD_GUIDE_ADAM && gd->final_optimizer != CLD_GUIDE_SGD)
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": unknown optimizer for the output step");
    if (gd->target_pos_scale && (!gd->target_pos || !gd->target_time)) return fail(h, CLD_ERR_ARG, std::string(fn) + ": target_pos_scale needs target_pos and target_time");
    return CLD_OK;
}

// the terms the guidance kernel evaluates itself: target speed, speed and acceleration limits, waypoint
static GuideArgs builtin_terms(const cld_guidance* gd) {
    GuideArgs g{};
    g.target_speed = gd->target_speed; g.loss_scale = gd->loss_scale;
    g.speed_limit_scale = gd->speed_limit_scale; g.acc_limit_scale = gd->acc_limit_scale;
    g.speed_limit = gd->speed_limit; g.acc_limit = gd->acc_limit;
    g.target_pos = gd->target_pos; g.target_time = gd->target_time; g.target_pos_scale = gd->target_pos_scale;
    return g;
}

// The guidance step(s) of one denoising iteration on the posterior mean `mean0` (upstream perturb(), guidance_loss.py:2221-2282):
// grad_steps optimiser steps, each one guidance-kernel launch (decoder forward + roll-out + loss gradients + BPTT + update) on the
// current iterate; with plan-space terms (plan_terms) each step first decodes the iterate and runs their loss kernels in the chain's
// order, whose summed gradient w.r.t. the plans enters the guidance kernel as ext_grad.  The last step adds sigma z and writes x_out (/ x_out2).
// `intermediate`: a t > 0 step (lr / perturb_th / optimizer / grad_steps) or the output step (final_*).
static int run_guidance(cld_handle h, const Ws& w, const cld_guidance* gd, int B, bool intermediate, float sigma_t, float sigma_noise,
                        const float* mean0, const float* cond, const float* z, uint64_t seed, unsigned long long salt,
                        float* mean_out, float* x_out, float* x_out2, float* grad_out, hipStream_t s) {
    const unsigned terms = plan_terms(h, gd);
    GuideArgs g = builtin_terms(gd);
    g.cond = cond; g.curr_states = gd->curr_states;
    // t = 0 (apply_guidance_output): the step's own optimiser settings, and no noise behind it (nonzero_mask, diffuser.py:929)
    const float lr_in = intermediate ? gd->lr : gd->final_lr, th_in = intermediate ? gd->perturb_th : gd->final_perturb_th;
    g.scratch = w.guide; g.lr = lr_in > 0.f ? lr_in : sigma_t; g.perturb_th = th_in > 0.f ? th_in : (th_in == 0.f ? sigma_t : -1.f);
    g.optimizer = intermediate ? gd->optimizer : gd->final_optimizer; g.B = B; g.seed = seed; g.step_salt = salt;
    const int steps_in = intermediate ? gd->grad_steps : gd->final_grad_steps;
    const int steps = steps_in > 1 ? steps_in : 1;
    g.opt_steps = steps; g.mean0 = mean0; g.adam_m = w.adam_m; g.adam_v = w.adam_v;
    for (int k = 1; k <= steps; ++k) {
        const bool last = k == steps;
        g.opt_step = k;
        g.mean = k == 1 ? mean0 : w.gcur;
        const float* gin = gd->ext_grad;                 // the gradient w.r.t. the plans so far: the caller's, then w.col_grad, to which every term adds its own
        if (terms) {                                     // the plan-space terms are functions of the decoded plans of the current iterate
            if (B >= 256 && guide_forward_available(B, h->force_kernel[CLD_KERNEL_GUIDE]) && h->force_kernel[CLD_KERNEL_DECODE] == FORM_AUTO) {
                // (from the batch size at which cld_decode itself would take its 16-agent MFMA form, ~0.3 ms; below that the
                //  one-agent-per-workgroup decoder is the shorter chain: 64 agents 579 vs 616 us per collision-guided step)
                // the guidance kernel's own forward sweep as the decoder (8 agents per workgroup: the whole chip at 2,048 agents), then
                // the O(T) roll-out.  Up to 2,048 agents every agent group has a workgroup and a scratch slot of its own in that launch: the
                // guidance kernel behind the loss kernels then runs its BACKWARD half only (GuideArgs::act_in), from the activations the
                // forward launch kept -- the sweep is not repeated (a collision-guided step 711 -> 6xx us at 2,048 agents)
                GuideArgs gf{};
                gf.mean = g.mean; gf.cond = cond; gf.curr_states = gd->curr_states; gf.scratch = w.guide; gf.B = B; gf.act_out = w.col_act;
                HIPCK(h, launch_guide_forward(h->dec, h->dyn, gf, s));
                HIPCK(h, launch_action_to_state(h->dyn, w.col_act, gd->curr_states, w.col_traj, B, 1, 1, s));
                g.act_in = guide_split_available(B, h->force_kernel[CLD_KERNEL_GUIDE]) && h->force_kernel[CLD_KERNEL_GUIDE] == FORM_AUTO ? w.col_act : nullptr;
            } else {
                HIPCK(h, launch_decode(h->dec, h->dyn, g.mean, cond, gd->curr_states, nullptr, w.col_traj, B, 1, s, h->force_kernel[CLD_KERNEL_DECODE]));
            }
        }
        if (terms & TERM_COLLISION) {
            HIPCK(h, launch_agent_collision(collision_args(gd->collision, w.col_traj, gin, nullptr, w.col_grad, B), s));
            gin = w.col_grad;
        }
        if (terms & TERM_MAP) {
            HIPCK(h, launch_map_collision(map_args(h, gd->map_collision, w.col_traj, gin, nullptr, w.col_grad), B, s));
            gin = w.col_grad;
        }
        if (terms & TERM_GOAL) {
            HIPCK(h, launch_goal(goal_args(&h->goal, w.col_traj, gin, nullptr, w.col_grad, B), s));
            gin = w.col_grad;
        }
        if (terms & TERM_SOCIAL) {                       // evaluation (loop iteration, optimiser step) picks the draws
            HIPCK(h, launch_social_group(social_args(&h->social, w.col_traj, nullptr, w.col_grad, B, (int)salt, k - 1), gin, s));
            gin = w.col_grad;
        }
        if (terms & TERM_PAIR) {
            HIPCK(h, launch_pair(pair_args(&h->pair, w.col_traj, nullptr, w.col_grad, B), gin, s));
            gin = w.col_grad;
        }
        if (terms & TERM_LANE) {
            HIPCK(h, launch_lane(lane_args(&h->lane, w.col_traj, nullptr, nullptr, w.col_grad, B), gin, s));
            gin = w.col_grad;
        }
        g.ext_grad = gin;
        g.z = last ? z : nullptr;
        g.sigma = last ? sigma_noise : 0.f;
        g.mean_out = last ? mean_out : w.gcur;           // in place from step 2 on: a workgroup reads its agents' rows before it writes them
        g.x_out = last ? x_out : nullptr;
        g.x_out2 = last ? x_out2 : nullptr;
        g.grad_out = k == 1 ? grad_out : nullptr;        // dL/dmean of the FIRST step (what the single-step call reports)
        HIPCK(h, launch_guide(h->dec, h->dyn, g, s, h->force_kernel[CLD_KERNEL_GUIDE]));
    }
    return CLD_OK;
}

// One iteration of the ancestral loop at timestep i on the latent in w.xw (CFG: rows [bp, 2 bp) hold the same latent, w.cb the
// conditional / unconditional bias rows): U-Net, head (noise prediction -> posterior mean -> + sigma z), optional guidance step on
// the mean.  Leaves x_{i-1} in w.xw (both halves) and, at i == 0 or on a guided step, the unguided posterior mean in w.meanb.
// `z` is this step's noise slab (NULL: on-device generator keyed by (seed, salt)); mean_guided / grad (optional, [B,52,4]) receive
// the guided mean and dL/dmean of a guided step.
static int sample_iteration(cld_handle h, const Ws& w, bool cfg, int B, int bp, int i, const float* z, uint64_t seed,
                            unsigned long long salt, const float* cond, float guidance_w, const cld_guidance* gd,
                            float* mean_guided, float* grad, bool want_mean, hipStream_t s) {
    const int bpn = cfg ? 2 * bp : bp;
    float* x_hi = w.xw + (size_t)bp * T * D;
    const float sigma = std::exp(0.5f * h->plvc[i]);
    // upstream defaults: apply_guidance_intermediate on, apply_guidance_output off (diffuser.py:876-881, scene_edit_config.py:84-85)
    const bool guide = gd && (i > 0 ? !gd->no_intermediate : gd->apply_output != 0);
    HeadArgs a{};
    a.w = h->head_w; a.b = h->head_b; a.x = w.xw; a.B = B; a.b_pad = bp;
    a.z = z;
    a.seed = seed; a.step_salt = salt;
    a.xc = h->x_t_cof[i]; a.nc = h->noise_cof[i];
    a.sg = (i == 0) ? 0.f : sigma;           // nonzero_mask, dm_model.py:151
    if (guide) {
        a.mean_out = w.meanb;                            // the guidance kernel perturbs the mean and adds the noise
        if (gd->guide_clean) {                           // ... or the model's clean prediction x0_hat (diffuser.py:866-873, :710-719)
            a.xc = h->sqrt_recip_acp[i]; a.nc = h->sqrt_recipm1_acp[i];
        }
    } else {
        a.x_out = w.xw;                                  // in place: each thread rewrites the row it read
        a.x_out2 = cfg ? x_hi : nullptr;
        a.mean_out = (i == 0 || want_mean) ? w.meanb : nullptr;
    }
    h->fuse_upd = cfg ? nullptr : &a;                    // without the CFG combine the tail chain applies the update itself
    const hipError_t eu = run_unet(h, w, w.xw, i, bpn, s);
    h->fuse_upd = nullptr;
    HIPCK(h, eu);
    if (!h->upd_fused) {
        head_source(h, w, a);
        if (cfg) {
            if (a.eps_in) a.eps_in_uncond = a.eps_in + (size_t)bp * T * D;
            else a.f_uncond = w.buf[7] + (size_t)bp * T * 64;
            a.cfg_w = guidance_w;
        }
        HIPCK(h, launch_head(a, s));
    }
    if (guide) {
        // a guided t = 0 step (apply_output): x0 IS the guided mean, and log_prob_final is taken around it (w.xtmp), not around the
        // unguided mean it was stepped away from -- sigma_0 = 1e-10 would turn that step into ~ -1e18
        int rcg = run_guidance(h, w, gd, B, i > 0, sigma, a.sg, w.meanb, cond, a.z, seed, salt, mean_guided ? mean_guided : (i == 0 ? w.xtmp : nullptr),
                               w.xw, cfg ? x_hi : nullptr, grad, s);
        if (rcg) return rcg;
    }
    return CLD_OK;
}

static int sample_impl(cld_handle h, const char* fn, const float* x_T, const float* noise, const float* cond,
                       const float* non_cond, float guidance_w, const cld_guidance* gd, int32_t steps, float* x0, float* x1,
                       float* logp, int32_t B, uint64_t seed, void* workspace, size_t workspace_bytes, void* stream) {
    const bool cfg = non_cond != nullptr;
    int rc = check_common(h, fn, cfg ? 2 * pad16(B) : B, 0, workspace, workspace_bytes);
    if (rc) return rc;
    if (!x_T || !cond) return fail(h, CLD_ERR_ARG, std::string(fn) + ": null pointer");
    if (steps != loop_steps(h))
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": steps must equal len(range(0, n_timesteps, stride)) = " + std::to_string(loop_steps(h)));
    if (gd && (rc = check_guidance(h, fn, gd, B, steps)) != CLD_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // CFG: one 2B-agent batch per step: rows [0, bp) carry cond_feat, rows [bp, 2bp) the unconditional features,
    // both halves the same latent; the head combines the two noise predictions and rewrites both halves.
    const int bp = pad16(B), bpn = cfg ? 2 * bp : bp;
    Ws w = carve(workspace, bpn);
    if ((rc = load_inputs(h, w, B, bp, x_T, cond, non_cond, cfg, s)) != CLD_OK) return rc;
    for (int it = 0; it < steps; ++it) {
        const int i = (steps - 1 - it) * h->stride;
        rc = sample_iteration(h, w, cfg, B, bp, i, noise ? noise + (size_t)it * B * T * D : nullptr, seed, (unsigned long long)it, cond,
                              guidance_w, gd, nullptr, nullptr, false, s);
        if (rc) return rc;
        if (i == 1 && x1) HIPCK(h, launch_unpack(w.xw, x1, B, s));
        if (i == 0) {
            if (x0) HIPCK(h, launch_unpack(w.xw, x0, B, s));
            if (logp) HIPCK(h, launch_logprob(w.xw, (gd && gd->apply_output) ? w.xtmp : w.meanb, std::exp(0.5f * h->plvc[0]), logp, B, s));
        }
    }
    return CLD_OK;
}

int cld_sample_step(cld_handle h, const float* x_t, const float* cond, const float* non_cond, float guidance_w,
                    const cld_guidance* gd, int32_t t_idx, const float* z, float* x_next, float* mean, float* mean_guided,
                    float* grad, float* sigma_host, int32_t B, void* workspace, size_t workspace_bytes, void* stream) {
    const bool cfg = non_cond != nullptr;
    int rc = check_common(h, "cld_sample_step", cfg ? 2 * pad16(B) : B, t_idx, workspace, workspace_bytes);
    if (rc) return rc;
    if (!x_t || !cond) return fail(h, CLD_ERR_ARG, "cld_sample_step: null pointer");      // z NULL: the generator, seed 0 / step 0
    if (gd && (rc = check_guidance(h, "cld_sample_step", gd, B)) != CLD_OK) return rc;
    if (sigma_host) *sigma_host = std::exp(0.5f * h->plvc[t_idx]);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int bp = pad16(B), bpn = cfg ? 2 * bp : bp;
    Ws w = carve(workspace, bpn);
    if ((rc = load_inputs(h, w, B, bp, x_t, cond, non_cond, cfg, s)) != CLD_OK) return rc;
    rc = sample_iteration(h, w, cfg, B, bp, t_idx, z, 0, 0, cond, guidance_w, gd, mean_guided, grad, mean != nullptr, s);
    if (rc) return rc;
    if (x_next) HIPCK(h, launch_unpack(w.xw, x_next, B, s));
    if (mean) HIPCK(h, launch_unpack(w.meanb, mean, B, s));
    return CLD_OK;
}

int cld_sample(cld_handle h, const float* x_T, const float* noise, const float* cond, int32_t steps, float* x0,
               float* x1, float* logp, int32_t B, uint64_t seed, void* workspace, size_t workspace_bytes, void* stream) {
    return sample_impl(h, "cld_sample", x_T, noise, cond, nullptr, 0.f, nullptr, steps, x0, x1, logp, B, seed, workspace,
                       workspace_bytes, stream);
}

int cld_sample_cfg(cld_handle h, const float* x_T, const float* noise, const float* cond, const float* non_cond,
                   float guidance_w, int32_t steps, float* x0, float* x1, float* logp, int32_t B, uint64_t seed,
                   void* workspace, size_t workspace_bytes, void* stream) {
    if (h && !non_cond) return fail(h, CLD_ERR_ARG, "cld_sample_cfg: null pointer");
    return sample_impl(h, "cld_sample_cfg", x_T, noise, cond, non_cond, guidance_w, nullptr, steps, x0, x1, logp, B, seed,
                       workspace, workspace_bytes, stream);
}

int cld_sample_guided(cld_handle h, const float* x_T, const float* noise, const float* cond, const float* non_cond,
                      float guidance_w, const cld_guidance* guidance, int32_t steps, float* x0, float* x1, float* logp,
                      int32_t B, uint64_t seed, void* workspace, size_t workspace_bytes, void* stream) {
    if (h && !guidance) return fail(h, CLD_ERR_ARG, "cld_sample_guided: null guidance");
    return sample_impl(h, "cld_sample_guided", x_T, noise, cond, non_cond, guidance_w, guidance, steps, x0, x1, logp, B, seed,
                       workspace, workspace_bytes, stream);
}

int cld_guidance_step(cld_handle h, const float* mean, const float* cond, const cld_guidance* gd, float sigma, const float* z,
                      float* mean_guided, float* x_next, float* grad, int32_t B, void* workspace, size_t workspace_bytes,
                      void* stream) {
    int rc = check_common(h, "cld_guidance_step", B, 0, workspace, workspace_bytes);
    if (rc) return rc;
    if (!h->has_decoder) return fail(h, CLD_ERR_STATE, "cld_guidance_step: decoder weights not loaded");
    if (!mean || !cond || !gd || (x_next && sigma != 0.f && !z)) return fail(h, CLD_ERR_ARG, "cld_guidance_step: null pointer");
    if ((rc = check_guidance(h, "cld_guidance_step", gd, B)) != CLD_OK) return rc;
    Ws w = carve(workspace, pad16(B));
    return run_guidance(h, w, gd, B, true, sigma, sigma, mean, cond, z, 0, 0, mean_guided, x_next, nullptr, grad, static_cast<hipStream_t>(stream));
}

int cld_guidance_losses(cld_handle h, const float* traj, const cld_guidance* gd, float* losses, int32_t B, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!traj || !gd || !losses || B < 1) return fail(h, CLD_ERR_ARG, "cld_guidance_losses: bad argument");
    if (gd->target_pos_scale && (!gd->target_pos || !gd->target_time)) return fail(h, CLD_ERR_ARG, "cld_guidance_losses: target_pos_scale needs target_pos and target_time");
    GuideArgs g = builtin_terms(gd);
    g.B = B;
    HIPCK(h, launch_guide_losses(g, traj, losses, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_log_prob(cld_handle h, const float* x_t, const float* x_tm1, const float* cond, int32_t t_idx, float* out,
                 int32_t M, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_common(h, "cld_log_prob", M, t_idx, workspace, workspace_bytes);
    if (rc) return rc;
    if (!x_t || !x_tm1 || !cond || !out) return fail(h, CLD_ERR_ARG, "cld_log_prob: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int bp = pad16(M);
    Ws w = carve(workspace, bp);
    if ((rc = load_inputs(h, w, M, bp, x_t, cond, nullptr, false, s)) != CLD_OK) return rc;
    HIPCK(h, run_unet(h, w, w.xw, t_idx, bp, s));
    HeadArgs a{};
    head_source(h, w, a); a.w = h->head_w; a.b = h->head_b; a.x = w.xw; a.B = M; a.b_pad = bp;
    a.mean_out = w.meanb; a.xc = h->x_t_cof[t_idx]; a.nc = h->noise_cof[t_idx];
    HIPCK(h, launch_head(a, s));
    HIPCK(h, launch_logprob(x_tm1, w.meanb, std::exp(0.5f * h->plvc[t_idx]), out, M, s));
    return CLD_OK;
}

int cld_lstm_decode(cld_handle h, const float* z, const float* cond, float* act, int32_t B, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!h->finalized || !h->has_decoder) return fail(h, CLD_ERR_STATE, "cld_lstm_decode: decoder weights not loaded");
    if (!z || !cond || !act || B < 1) return fail(h, CLD_ERR_ARG, "cld_lstm_decode: bad argument");
    HIPCK(h, launch_decode(h->dec, h->dyn, z, cond, nullptr, act, nullptr, B, 1, static_cast<hipStream_t>(stream), h->force_kernel[CLD_KERNEL_DECODE]));
    return CLD_OK;
}

int cld_action_to_state(cld_handle h, const float* act, const float* curr_states, float* traj, int32_t B,
                        int32_t scaled_input, int32_t descaled_output, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!act || !curr_states || !traj || B < 1) return fail(h, CLD_ERR_ARG, "cld_action_to_state: bad argument");
    HIPCK(h, launch_action_to_state(h->dyn, act, curr_states, traj, B, scaled_input, descaled_output,
                                    static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_decode(cld_handle h, const float* z, const float* cond, const float* curr_states, float* traj, float* act_out,
               int32_t B, int32_t descaled_output, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!h->finalized || !h->has_decoder) return fail(h, CLD_ERR_STATE, "cld_decode: decoder weights not loaded");
    if (!z || !cond || !curr_states || !traj || B < 1) return fail(h, CLD_ERR_ARG, "cld_decode: bad argument");
    HIPCK(h, launch_decode(h->dec, h->dyn, z, cond, curr_states, act_out, traj, B, descaled_output,
                           static_cast<hipStream_t>(stream), h->force_kernel[CLD_KERNEL_DECODE]));
    return CLD_OK;
}

int cld_traj2z(cld_handle h, const float* x6_scaled, const float* cond, const float* noise, float* z, float* mu,
               float* logvar, int32_t B, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!h->finalized || !h->has_encoder) return fail(h, CLD_ERR_STATE, "cld_traj2z: encoder weights not loaded");
    if (!x6_scaled || !cond || B < 1 || (!z && !mu && !logvar)) return fail(h, CLD_ERR_ARG, "cld_traj2z: bad argument");
    HIPCK(h, launch_encode(h->enc, x6_scaled, cond, noise, z, mu, logvar, B, static_cast<hipStream_t>(stream), h->force_kernel[CLD_KERNEL_ENCODE]));
    return CLD_OK;
}

int cld_vae_loss(cld_handle h, const float* x6_scaled, const float* act_out, const float* mu, const float* logvar, float beta,
                 float* out3, int32_t B, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!x6_scaled || !act_out || !mu || !logvar || !out3 || B < 1) return fail(h, CLD_ERR_ARG, "cld_vae_loss: bad argument");
    if (!workspace || workspace_bytes < (size_t)B * 2 * sizeof(float)) return fail(h, CLD_ERR_WORKSPACE, "cld_vae_loss: workspace too small");
    HIPCK(h, launch_vae_loss(x6_scaled, act_out, mu, logvar, beta, static_cast<float*>(workspace), out3, B,
                             static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_state_to_state_and_action(cld_handle h, const float* positions, const float* yaws, const float* curr_speed,
                                  float* out6, int32_t B, int32_t scaled_output, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!positions || !yaws || !curr_speed || !out6 || B < 1)
        return fail(h, CLD_ERR_ARG, "cld_state_to_state_and_action: bad argument");
    HIPCK(h, launch_state_to_state_action(h->dyn, positions, yaws, curr_speed, out6, B, scaled_output,
                                          static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

// ---- ContextEncoder ---------------------------------------------------------------------------------------
namespace {
constexpr int kCtxChunk = 256;                               // agents per pass: bounds the activation scratch
constexpr size_t kStemFloats = (size_t)112 * 112 * 64;       // per agent
constexpr size_t kActFloats = (size_t)56 * 56 * 64;          // largest post-pool activation per agent

// Agents per pass of the ContextEncoder.  The Winograd kernels (wino44_kernels.hip, 4x4 tiles) run equal workgroups of 16 tiles x 64 channels, two
// to a CU: n * (196 | 49 | 16 | 4) / 16 * (C / 64) at 56x56 / 28x28 / 14x14 / 7x7 -- at n = 256 that is 6.125 / 3.06 / 2 / 1 generations of 512; a last
// generation that is 6 % full costs a whole one.  The pass size is the one that minimises the modelled generation count of the whole batch (a
// generation of the four launch kinds lasts 1.5 / 2.7 / 4.3 / 8.5 units -- measured: 36 / 65 / 103 / 202 us --), with a fixed cost per pass for its
// 27 launches.  (The pass size is a speed choice only: a row's result does not depend on it.)
int context_pass_size(int B) {
    if (B <= kCtxChunk) return B;
    auto cost = [](int n) {
        auto gens = [&](int tiles_per_agent, int ncb) { return (long)((n * tiles_per_agent + 15) / 16 * ncb + 511) / 512; };
        return 4 * gens(196, 1) * 15 + 3 * gens(49, 2) * 27 + 3 * gens(16, 4) * 43 + 3 * gens(4, 8) * 85 + 60;
    };
    int best = kCtxChunk;
    long best_cost = -1;
    for (int p = kCtxChunk; p >= 128; --p) {
        long c = (long)(B / p) * cost(p) + (B % p ? cost(B % p) : 0);
        if (best_cost < 0 || c < best_cost) { best_cost = c; best = p; }
    }
    return best;
}

// The one dispatch of the encoder's convolutions, shared by cld_context_encode and cld_debug_context_layer: F(4x4, 3x3) for the stride-1
// 3x3 layers unless a test forced the direct form (cld_debug_force_kernel(CLD_KERNEL_CONTEXT)), the implicit GEMM otherwise and for the
// stride-2 3x3 and the 1x1/2 layers.
hipError_t context_conv(cld_handle h, const cld_handle_s::Conv2dLayer& l, const float* x, const float* res, float* y, int relu, int n, hipStream_t s) {
    if (h->force_kernel[CLD_KERNEL_CONTEXT] != CLD_FORM_DIRECT && l.ufrag44)
        return launch_wino44_conv(l.hin, l.cout, WinoArgs{x, l.ufrag44, l.scale, l.shift, res, y, n, relu}, s);
    return launch_conv2d(l.kh, l.stride, l.hin, x, l.wfrag, l.scale, l.shift, res, y, n, l.cin, l.cout, relu, s);
}

// stem + max-pool of n agents: image [n,34,224,224] NCHW -> pooled [n,56,56,64] NHWC; y1 [n,112,112,64] is the direct form's scratch
hipError_t context_stem(cld_handle h, const float* image, float* y1, float* pooled, int n, hipStream_t s) {
    if (h->force_kernel[CLD_KERNEL_CONTEXT] == CLD_FORM_DIRECT) {      // the direct form of the encoder: stem and max-pool as two launches
        hipError_t e = launch_stem_conv(image, h->stem_w, h->stem_scale, h->stem_shift, y1, nullptr, n, s);
        return e != hipSuccess ? e : launch_maxpool(y1, pooled, n, s);
    }
    // max-pool inside the stem's epilogue: [n,112,112,64] is never written
    return launch_stem_conv(image, h->stem_w, h->stem_scale, h->stem_shift, nullptr, pooled, n, s);
}
}
size_t cld_context_workspace_bytes(cld_handle h, int32_t B) {
    if (!h || B < 1) return 0;
    const size_t cb = (size_t)(B < kCtxChunk ? B : kCtxChunk);
    return cb * (kStemFloats + 3 * kActFloats) * sizeof(float);
}

int cld_context_encode(cld_handle h, const float* image, const float* curr_states, float* cond_feat, float* map_feat,
                       int32_t B, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!h->finalized || !h->has_context) return fail(h, CLD_ERR_STATE, "cld_context_encode: context_encoder weights not loaded");
    if (!image || !curr_states || !cond_feat || B < 1) return fail(h, CLD_ERR_ARG, "cld_context_encode: bad argument");
    if (!workspace || workspace_bytes < cld_context_workspace_bytes(h, B))
        return fail(h, CLD_ERR_WORKSPACE, "cld_context_encode: workspace too small");
    if (reinterpret_cast<uintptr_t>(workspace) % 16 || reinterpret_cast<uintptr_t>(image) % 16)
        return fail(h, CLD_ERR_ARG, "cld_context_encode: image and workspace must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cb = B < kCtxChunk ? B : kCtxChunk;
    float* y1 = static_cast<float*>(workspace);
    float* buf[3];
    for (int i = 0; i < 3; ++i) buf[i] = y1 + (size_t)cb * kStemFloats + (size_t)i * cb * kActFloats;
    const bool wino = h->force_kernel[CLD_KERNEL_CONTEXT] != CLD_FORM_DIRECT;
    auto run = [&](const cld_handle_s::Conv2dLayer& l, const float* x, const float* res, float* y, int relu, int n) {
        return context_conv(h, l, x, res, y, relu, n, s);
    };
    const int pass = wino ? context_pass_size(B) : cb;
    for (int b0 = 0; b0 < B; b0 += pass) {
        const int n = (B - b0) < pass ? (B - b0) : pass;
        HIPCK(h, context_stem(h, image + (size_t)b0 * 34 * 224 * 224, y1, buf[0], n, s));
        int xi = 0;                                            // buffer holding the current block input
        for (int li = 0; li < 4; ++li)
            for (int b = 0; b < 2; ++b) {                      // BasicBlock: relu(bn2(conv2(relu(bn1(conv1 x)))) + identity)
                const int ti = (xi + 1) % 3, yi = (xi + 2) % 3;
                HIPCK(h, run(h->rn_conv[li][b][0], buf[xi], nullptr, buf[ti], 1, n));
                if (b == 0 && li > 0) {                        // identity = bn(conv1x1/2 x); x's buffer is free afterwards
                    HIPCK(h, run(h->rn_ds[li], buf[xi], nullptr, buf[yi], 0, n));
                    HIPCK(h, run(h->rn_conv[li][b][1], buf[ti], buf[yi], buf[xi], 1, n));
                } else {
                    HIPCK(h, run(h->rn_conv[li][b][1], buf[ti], buf[xi], buf[yi], 1, n));
                    xi = yi;
                }
            }
        ContextHeadArgs a = h->ctx_head;
        a.feat = buf[xi]; a.curr_states = curr_states + (size_t)b0 * 4; a.cond_out = cond_feat + (size_t)b0 * 256;
        a.map_feat_out = map_feat ? map_feat + (size_t)b0 * 256 : nullptr; a.B = n;
        HIPCK(h, launch_context_head(a, s));
    }
    return CLD_OK;
}

int cld_context_combine(cld_handle h, const float* map_feat, int32_t broadcast, const float* curr_states, float* cond_feat,
                        int32_t B, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!h->finalized || !h->has_context) return fail(h, CLD_ERR_STATE, "cld_context_combine: context_encoder weights not loaded");
    if (!map_feat || !curr_states || !cond_feat || B < 1) return fail(h, CLD_ERR_ARG, "cld_context_combine: bad argument");
    ContextHeadArgs a = h->ctx_head;
    a.feat = nullptr; a.map_feat_in = map_feat; a.map_feat_stride = broadcast ? 0 : 256;
    a.curr_states = curr_states; a.cond_out = cond_feat; a.map_feat_out = nullptr; a.B = B;
    HIPCK(h, launch_context_head(a, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_debug_context_layer(cld_handle h, int32_t layer, const float* x, const float* residual, float* y, int32_t n, int32_t relu, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!h->finalized || !h->has_context) return fail(h, CLD_ERR_STATE, "cld_debug_context_layer: context_encoder weights not loaded");
    if (layer < 0 || layer > 19 || !x || !y || n < 1 || n > kCtxChunk || (layer == 0 && (residual || !relu)))
        return fail(h, CLD_ERR_ARG, "cld_debug_context_layer: bad argument");
    if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(y) % 16 || reinterpret_cast<uintptr_t>(residual) % 16)
        return fail(h, CLD_ERR_ARG, "cld_debug_context_layer: tensors must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (layer == 0) {
        float* y1 = nullptr;      // the direct form's [n,112,112,64] scratch
        if (h->force_kernel[CLD_KERNEL_CONTEXT] == CLD_FORM_DIRECT) HIPCK(h, hipMalloc(reinterpret_cast<void**>(&y1), (size_t)n * kStemFloats * sizeof(float)));
        const hipError_t e = context_stem(h, x, y1, y, n, s);
        if (y1) {
            const hipError_t es = hipStreamSynchronize(s);
            (void)hipFree(y1);
            HIPCK(h, es);
        }
        HIPCK(h, e);
        return CLD_OK;
    }
    const int li = layer <= 16 ? (layer - 1) / 4 : layer - 16;
    const cld_handle_s::Conv2dLayer& l = layer <= 16 ? h->rn_conv[li][((layer - 1) / 2) % 2][(layer - 1) % 2] : h->rn_ds[li];
    HIPCK(h, context_conv(h, l, x, residual, y, relu ? 1 : 0, n, s));
    return CLD_OK;
}

int cld_debug_context_pass_size(int32_t B) { return B < 1 ? CLD_ERR_ARG : context_pass_size(B); }

int cld_compute_reward(cld_handle h, const float* traj, const float* traj_scaled, const float* raster_from_agent,
                       const uint8_t* drivable_map, int32_t H, int32_t W, const float* other_pos, const uint8_t* other_avail,
                       int32_t S, int32_t T_other, float collision_thresh, float* reward, float* offroad, float* collision,
                       int32_t B, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!traj || !raster_from_agent || !drivable_map || B < 1 || H < 1 || W < 1 || S < 0 || T_other < 0 ||
        (S > 0 && T_other > 0 && (!other_pos || !other_avail)) || (!reward && !offroad && !collision))
        return fail(h, CLD_ERR_ARG, "cld_compute_reward: bad argument");
    RewardArgs a{};
    a.traj = traj; a.traj_scaled = traj_scaled; a.raster_from_agent = raster_from_agent; a.drivable_map = drivable_map;
    a.other_pos = other_pos; a.other_avail = other_avail; a.reward = reward; a.offroad = offroad; a.collision = collision;
    a.collision_thresh = collision_thresh; a.B = B; a.H = H; a.W = W; a.S = S; a.To = T_other < T ? T_other : T;
    HIPCK(h, launch_reward(a, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_agent_collision(cld_handle h, const float* traj, const cld_collision* c, const float* grad_in, float* loss, float* grad,
                        int32_t B, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!traj || !c || B < 1 || (!loss && !grad)) return fail(h, CLD_ERR_ARG, "cld_agent_collision: bad argument");
    int rc = check_collision(h, "cld_agent_collision", c, B);
    if (rc) return rc;
    HIPCK(h, launch_agent_collision(collision_args(c, traj, grad_in, loss, grad, B), static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_map_collision_loss(cld_handle h, const float* traj, const cld_map_collision* c, const float* grad_in, float* loss,
                           float* grad, int32_t B, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!traj || !c || B < 1 || (!loss && !grad)) return fail(h, CLD_ERR_ARG, "cld_map_collision_loss: bad argument");
    int rc = check_map_collision(h, "cld_map_collision_loss", c, B);
    if (rc) return rc;
    HIPCK(h, launch_map_collision(map_args(h, c, traj, grad_in, loss, grad), B, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_goal_loss(cld_handle h, const float* traj, const cld_goal* g, const float* grad_in, float* loss, float* grad, int32_t B,
                  void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!traj || !g || B < 1 || (!loss && !grad)) return fail(h, CLD_ERR_ARG, "cld_goal_loss: bad argument");
    int rc = check_goal(h, "cld_goal_loss", g, B);
    if (rc) return rc;
    HIPCK(h, launch_goal(goal_args(g, traj, grad_in, loss, grad, B), static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_social_group_loss(cld_handle h, const float* traj, const cld_social_group* term, const float* grad_in, float* loss, float* grad,
                          int32_t B, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!traj || !term || B < 1 || (!loss && !grad)) return fail(h, CLD_ERR_ARG, "cld_social_group_loss: bad argument");
    int rc = check_social(h, "cld_social_group_loss", term, B, 0, 0);
    if (rc) return rc;
    HIPCK(h, launch_social_group(social_args(term, traj, loss, grad, B, 0, 0), grad_in, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_set_social_term(cld_handle h, const cld_social_group* term) { return set_term(h, term, &cld_handle_s::social, &cld_handle_s::has_social); }

int cld_pair_loss(cld_handle h, const float* traj, const cld_pair_term* term, const float* grad_in, float* value, float* grad, int32_t B,
                  void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!traj || !term || B < 1 || (!value && !grad)) return fail(h, CLD_ERR_ARG, "cld_pair_loss: bad argument");
    int rc = check_pair(h, "cld_pair_loss", term, B);
    if (rc) return rc;
    HIPCK(h, launch_pair(pair_args(term, traj, value, grad, B), grad_in, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_set_pair_term(cld_handle h, const cld_pair_term* term) { return set_term(h, term, &cld_handle_s::pair, &cld_handle_s::has_pair); }

int cld_lane_prepare(cld_handle h, const double* world_lines, const int32_t* line_frame, const float* agent_from_world, float* lines,
                     int32_t num_lines, int32_t max_pts, int32_t num_frames, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!world_lines || !line_frame || !agent_from_world || !lines || num_lines < 1 || num_frames < 1)
        return fail(h, CLD_ERR_ARG, "cld_lane_prepare: bad argument");
    if (max_pts < 1 || max_pts > CLD_LANE_MAX_PTS)
        return fail(h, CLD_ERR_ARG, "cld_lane_prepare: max_pts must be 1 .. " + std::to_string(CLD_LANE_MAX_PTS));
    LanePrepareArgs a{};
    a.world_lines = world_lines; a.line_frame = line_frame; a.agent_from_world = agent_from_world; a.lines = lines;
    a.num_lines = num_lines; a.max_pts = max_pts; a.num_frames = num_frames;
    HIPCK(h, launch_lane_prepare(a, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_lane_loss(cld_handle h, const float* traj, const cld_lane_term* term, const float* grad_in, float* value, float* proj,
                  float* grad, int32_t B, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!traj || !term || B < 1 || (!value && !proj && !grad)) return fail(h, CLD_ERR_ARG, "cld_lane_loss: bad argument");
    int rc = check_lane(h, "cld_lane_loss", term, B);
    if (rc) return rc;
    HIPCK(h, launch_lane(lane_args(term, traj, value, proj, grad, B), grad_in, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_set_lane_term(cld_handle h, const cld_lane_term* term) { return set_term(h, term, &cld_handle_s::lane, &cld_handle_s::has_lane); }

int cld_set_goal_term(cld_handle h, const cld_goal* g) { return set_term(h, g, &cld_handle_s::goal, &cld_handle_s::has_goal); }

int cld_set_map_source(cld_handle h, const cld_map_source* m) {
    if (!h) return CLD_ERR_ARG;
    if (m) {
        if (!m->world) return fail(h, CLD_ERR_ARG, "cld_set_map_source: null argument (world)");
        if (m->num_scenes < 1) return fail(h, CLD_ERR_ARG, "cld_set_map_source: num_scenes < 1");
        if (!(m->px_per_m > 0.f)) return fail(h, CLD_ERR_ARG, "cld_set_map_source: px_per_m must be positive");
        if (m->n_sem < 1 || m->n_sem > CLD_RASTER_MAX_PLANES || m->drivable_layer < 0 || m->drivable_layer >= m->n_sem)
            return fail(h, CLD_ERR_ARG, "cld_set_map_source: drivable_layer must be one of the n_sem >= 1 layers");
        if (m->maps && (!m->scene_map || !m->map_from_world || m->num_maps < 1 || m->map_h < 1 || m->map_w < 1 ||
                        (int64_t)m->map_h * m->map_w > INT32_MAX))
            return fail(h, CLD_ERR_ARG, "cld_set_map_source: maps need scene_map, map_from_world, num_maps, map_h and map_w");
    }
    return set_term(h, m, &cld_handle_s::map_source, &cld_handle_s::has_map_source);
}

int cld_world_step(cld_handle h, const float* traj, const float* centroid, const float* yaw, int32_t k, float* world,
                   float* next_curr_states, int32_t B, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!traj || !centroid || !yaw || !world || B < 1 || k < 0 || k >= T) return fail(h, CLD_ERR_ARG, "cld_world_step: bad argument");
    HIPCK(h, launch_world_step(traj, centroid, yaw, k, world, next_curr_states, B, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_rasterize(cld_handle h, const cld_raster* r, int32_t row0, int32_t B, float* image, uint8_t* drivable, float* raster_from_world,
                  void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!r || !image || !r->hist_world || !r->hist_avail || !r->scene_start) return fail(h, CLD_ERR_ARG, "cld_rasterize: null argument");
    if (r->num_scenes < 1 || r->B_all < 1 || r->B_all > CLD_RASTER_MAX_AGENTS || r->T_hist < 1 || r->T_hist > CLD_RASTER_MAX_PLANES ||
        r->n_sem < 0 || r->n_sem > CLD_RASTER_MAX_PLANES)
        return fail(h, CLD_ERR_ARG, "cld_rasterize: num_scenes / B_all / T_hist / n_sem out of range (include/cld.h CLD_RASTER_MAX_*)");
    if (B < 1 || row0 < 0 || (int64_t)row0 + B > r->B_all) return fail(h, CLD_ERR_ARG, "cld_rasterize: rows [row0, row0 + B) are not within B_all");
    if (r->height < 1 || r->width < 1 || (int64_t)r->height * r->width > CLD_RASTER_MAX_PIXELS)
        return fail(h, CLD_ERR_ARG, "cld_rasterize: height x width out of range (include/cld.h CLD_RASTER_MAX_PIXELS)");
    if (!(r->px_per_m > 0.f)) return fail(h, CLD_ERR_ARG, "cld_rasterize: px_per_m must be positive");
    if (r->maps && (!r->scene_map || !r->map_from_world || r->num_maps < 1 || r->map_h < 1 || r->map_w < 1 || r->n_sem < 1 ||
                    (int64_t)r->map_h * r->map_w > INT32_MAX))
        return fail(h, CLD_ERR_ARG, "cld_rasterize: maps need scene_map, map_from_world, num_maps, map_h, map_w and n_sem");
    if (drivable && r->n_sem < 1) return fail(h, CLD_ERR_ARG, "cld_rasterize: the drivable map is the first semantic plane (n_sem >= 1)");
    if ((int64_t)B * (r->T_hist + r->n_sem) > INT32_MAX) return fail(h, CLD_ERR_ARG, "cld_rasterize: too many planes for one launch");
    RasterArgs a{};
    a.hist_world = r->hist_world; a.hist_avail = r->hist_avail; a.scene_start = r->scene_start; a.maps = r->maps; a.scene_map = r->scene_map;
    a.map_from_world = r->map_from_world; a.image = image; a.drivable = drivable; a.raster_from_world = raster_from_world;
    a.num_scenes = r->num_scenes; a.B_all = r->B_all; a.T = r->T_hist; a.n_sem = r->n_sem; a.H = r->height; a.W = r->width;
    a.num_maps = r->num_maps; a.map_h = r->map_h; a.map_w = r->map_w; a.row0 = row0; a.B = B;
    a.ppm = r->px_per_m; a.ox = (1.f + r->ego_center[0]) * 0.5f * (float)r->width; a.oy = (1.f + r->ego_center[1]) * 0.5f * (float)r->height;
    a.fill = r->no_map_fill; a.max_dist = r->max_neighbor_dist;
    HIPCK(h, launch_raster(a, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

/* ---- closed-loop episode metrics (metrics_kernels.hip) ---- */
static_assert(CLD_METRICS_AGENT_COLS == METRICS_AGENT_COLS && CLD_METRICS_SCENE_COLS == METRICS_SCENE_COLS, "include/cld.h");

size_t cld_scene_metrics_state_bytes(int32_t B_all) { return B_all < 1 ? 0 : (size_t)B_all * METRICS_ROW_BYTES; }

static int check_scene_metrics(cld_handle h, const char* fn, const cld_scene_metrics* m, const void* state, MetricsArgs* a) {
    const std::string f(fn);
    if (!m || !state || !m->extent || !m->scene_start) return fail(h, CLD_ERR_ARG, f + ": null argument");
    if (reinterpret_cast<uintptr_t>(state) % 16) return fail(h, CLD_ERR_ARG, f + ": state must be 16-byte aligned");
    if (m->num_scenes < 1 || m->B_all < 1 || m->B_all > CLD_RASTER_MAX_AGENTS || m->num_scenes > m->B_all)
        return fail(h, CLD_ERR_ARG, f + ": num_scenes / B_all out of range (1 <= num_scenes <= B_all <= CLD_RASTER_MAX_AGENTS)");
    if (m->height < 1 || m->width < 1 || (int64_t)m->height * m->width > CLD_RASTER_MAX_PIXELS)
        return fail(h, CLD_ERR_ARG, f + ": height x width out of range (include/cld.h CLD_RASTER_MAX_PIXELS)");
    if (!(m->px_per_m > 0.f)) return fail(h, CLD_ERR_ARG, f + ": px_per_m must be positive");
    if (m->n_sem < 1 || m->n_sem > CLD_RASTER_MAX_PLANES || m->drivable_layer < 0 || m->drivable_layer >= m->n_sem)
        return fail(h, CLD_ERR_ARG, f + ": drivable_layer must be one of the n_sem >= 1 layers");
    if (m->maps && (!m->scene_map || !m->map_from_world || m->num_maps < 1 || m->map_h < 1 || m->map_w < 1 ||
                    (int64_t)m->map_h * m->map_w > INT32_MAX))
        return fail(h, CLD_ERR_ARG, f + ": maps need scene_map, map_from_world, num_maps, map_h and map_w");
    if (!(m->sim_dt > 0.0) || !(m->stat_dt >= m->sim_dt) || !(m->stat_dt / m->sim_dt < 1e6))
        return fail(h, CLD_ERR_ARG, f + ": comfort needs 0 < sim_dt <= stat_dt");
    *a = MetricsArgs{};
    a->extent = m->extent; a->scene_start = m->scene_start; a->maps = m->maps; a->scene_map = m->scene_map;
    a->map_from_world = m->map_from_world; a->state = const_cast<void*>(state);
    a->num_scenes = m->num_scenes; a->B_all = m->B_all; a->n_sem = m->n_sem; a->num_maps = m->num_maps; a->map_h = m->map_h;
    a->map_w = m->map_w; a->H = m->height; a->W = m->width; a->layer = m->drivable_layer;
    a->ratio = (int)std::ceil(m->stat_dt / m->sim_dt);            // Comfort.get_episode_metrics: int(math.ceil(stat_dt / sim_dt))
    a->ppm = m->px_per_m; a->ox = (1.f + m->ego_center[0]) * 0.5f * (float)m->width; a->oy = (1.f + m->ego_center[1]) * 0.5f * (float)m->height;
    a->fill = m->no_map_fill; a->dt = (float)m->stat_dt;
    return CLD_OK;
}

int cld_scene_metrics_step(cld_handle h, const cld_scene_metrics* m, const float* world, void* state, uint8_t* flags, int32_t* partner,
                           int32_t step, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!world) return fail(h, CLD_ERR_ARG, "cld_scene_metrics_step: null argument (world)");
    if (step < 0) return fail(h, CLD_ERR_ARG, "cld_scene_metrics_step: step < 0");
    MetricsArgs a;
    int rc = check_scene_metrics(h, "cld_scene_metrics_step", m, state, &a);
    if (rc) return rc;
    a.world = world; a.flags = flags; a.partner = partner; a.step = step;
    HIPCK(h, launch_scene_metrics_step(a, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_scene_metrics_read(cld_handle h, const cld_scene_metrics* m, const void* state, float* per_agent, float* per_scene, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!per_agent && !per_scene) return fail(h, CLD_ERR_ARG, "cld_scene_metrics_read: no output");
    MetricsArgs a;
    int rc = check_scene_metrics(h, "cld_scene_metrics_read", m, state, &a);
    if (rc) return rc;
    a.per_agent = per_agent; a.per_scene = per_scene;
    HIPCK(h, launch_scene_metrics_read(a, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

/* ---- guidance satisfaction metrics (guide_metrics_kernels.hip) ---- */
size_t cld_guide_metrics_state_bytes(int32_t num_entries, int32_t num_members) {
    if (num_entries < 1 || num_members < 1) return 0;
    return (size_t)num_entries * GUIDE_METRICS_ENTRY_BYTES + (size_t)num_members * GUIDE_METRICS_MEMBER_BYTES;
}

static int check_guide_metrics(cld_handle h, const char* fn, const cld_guide_metrics* m, const void* state, GuideMetricsArgs* a) {
    const std::string f(fn);
    if (!m || !state || !m->extent || !m->scene_start || !m->entry_kind || !m->entry_scene || !m->member_start || !m->members ||
        !m->excl_start || !m->param_start)
        return fail(h, CLD_ERR_ARG, f + ": null argument");
    if (reinterpret_cast<uintptr_t>(state) % 16) return fail(h, CLD_ERR_ARG, f + ": state must be 16-byte aligned");
    if (m->num_scenes < 1 || m->B_all < 1 || m->B_all > CLD_RASTER_MAX_AGENTS || m->num_scenes > m->B_all)
        return fail(h, CLD_ERR_ARG, f + ": num_scenes / B_all out of range (1 <= num_scenes <= B_all <= CLD_RASTER_MAX_AGENTS)");
    if (m->num_entries < 1 || m->num_members < 1 || m->num_members > CLD_RASTER_MAX_AGENTS || m->num_entries > CLD_RASTER_MAX_AGENTS)
        return fail(h, CLD_ERR_ARG, f + ": num_entries / num_members out of range (1 .. CLD_RASTER_MAX_AGENTS)");
    if (m->num_excluded < 0 || (m->num_excluded > 0 && !m->excluded) || m->num_params < 0 || (m->num_params > 0 && !m->params))
        return fail(h, CLD_ERR_ARG, f + ": num_excluded / num_params need their arrays");
    if (m->height < 1 || m->width < 1 || (int64_t)m->height * m->width > CLD_RASTER_MAX_PIXELS)
        return fail(h, CLD_ERR_ARG, f + ": height x width out of range (include/cld.h CLD_RASTER_MAX_PIXELS)");
    if (!(m->px_per_m > 0.f)) return fail(h, CLD_ERR_ARG, f + ": px_per_m must be positive");
    if (m->n_sem < 1 || m->n_sem > CLD_RASTER_MAX_PLANES || m->drivable_layer < 0 || m->drivable_layer >= m->n_sem)
        return fail(h, CLD_ERR_ARG, f + ": drivable_layer must be one of the n_sem >= 1 layers");
    if (m->maps && (!m->scene_map || !m->map_from_world || m->num_maps < 1 || m->map_h < 1 || m->map_w < 1 ||
                    (int64_t)m->map_h * m->map_w > INT32_MAX))
        return fail(h, CLD_ERR_ARG, f + ": maps need scene_map, map_from_world, num_maps, map_h and map_w");
    *a = GuideMetricsArgs{};
    a->extent = m->extent; a->scene_start = m->scene_start; a->maps = m->maps; a->scene_map = m->scene_map;
    a->map_from_world = m->map_from_world; a->entry_kind = m->entry_kind; a->entry_scene = m->entry_scene;
    a->member_start = m->member_start; a->members = m->members; a->excl_start = m->excl_start;
    a->excluded = m->num_excluded > 0 ? m->excluded : nullptr; a->param_start = m->param_start;
    a->params = m->num_params > 0 ? m->params : nullptr; a->state = const_cast<void*>(state);
    a->num_entries = m->num_entries; a->num_members = m->num_members; a->num_excluded = m->num_excluded; a->num_params = m->num_params;
    a->num_scenes = m->num_scenes; a->B_all = m->B_all; a->n_sem = m->n_sem; a->num_maps = m->num_maps; a->map_h = m->map_h;
    a->map_w = m->map_w; a->H = m->height; a->W = m->width; a->layer = m->drivable_layer;
    a->ppm = m->px_per_m; a->ox = (1.f + m->ego_center[0]) * 0.5f * (float)m->width; a->oy = (1.f + m->ego_center[1]) * 0.5f * (float)m->height;
    a->fill = m->no_map_fill;
    return CLD_OK;
}

int cld_guide_metrics_step(cld_handle h, const cld_guide_metrics* m, const float* world, const float* speed, const float* acc, void* state,
                           int32_t global_t, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!world || !speed || !acc) return fail(h, CLD_ERR_ARG, "cld_guide_metrics_step: null argument (world / speed / acc)");
    if (global_t < 0) return fail(h, CLD_ERR_ARG, "cld_guide_metrics_step: global_t < 0");
    GuideMetricsArgs a;
    int rc = check_guide_metrics(h, "cld_guide_metrics_step", m, state, &a);
    if (rc) return rc;
    a.world = world; a.speed = speed; a.acc = acc; a.global_t = global_t;
    HIPCK(h, launch_guide_metrics_step(a, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_guide_metrics_read(cld_handle h, const cld_guide_metrics* m, const void* state, double* per_entry, double* per_member, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!per_entry && !per_member) return fail(h, CLD_ERR_ARG, "cld_guide_metrics_read: no output");
    GuideMetricsArgs a;
    int rc = check_guide_metrics(h, "cld_guide_metrics_read", m, state, &a);
    if (rc) return rc;
    a.per_entry = per_entry; a.per_member = per_member;
    HIPCK(h, launch_guide_metrics_read(a, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

/* ---- occupancy coverage and diversity (occupancy_kernels.hip) ---- */
static_assert(CLD_OCCUPANCY_MAX_WINDOW_CELLS == OCC_MAX_WINDOW_CELLS, "include/cld.h");

static int check_occupancy(cld_handle h, const char* fn, const cld_occupancy* o, OccArgs* a) {
    const std::string f(fn);
    if (!o || !o->scene_start || !o->window || !o->cell_start) return fail(h, CLD_ERR_ARG, f + ": null argument");
    if (o->num_scenes < 1 || o->B_all < 1 || o->B_all > CLD_RASTER_MAX_AGENTS || o->num_scenes > o->B_all || o->cells < 1)
        return fail(h, CLD_ERR_ARG, f + ": num_scenes / B_all / cells out of range (1 <= num_scenes <= B_all <= CLD_RASTER_MAX_AGENTS, cells >= 1)");
    if (!std::isfinite(o->offset[0]) || !std::isfinite(o->offset[1])) return fail(h, CLD_ERR_ARG, f + ": offset must be finite");
    if (!(o->step[0] > 0.0) || !(o->step[1] > 0.0) || !std::isfinite(o->step[0]) || !std::isfinite(o->step[1]))
        return fail(h, CLD_ERR_ARG, f + ": step must be positive");
    if (!(o->sigma > 0.0) || !std::isfinite(o->sigma)) return fail(h, CLD_ERR_ARG, f + ": sigma must be positive");
    if (!(o->kernel_cut > 0.0) || !(o->kernel_cut < 1.0)) return fail(h, CLD_ERR_ARG, f + ": kernel_cut must be inside (0, 1)");
    // OccupancyGrid.update / get_neighboring_grid_points: radius = sqrt(-2 sigma ln(threshold)), Nx = Ny = int(ceil(radius / xs)) + 1
    const double half = std::ceil(std::sqrt(-2.0 * o->sigma * std::log(o->kernel_cut)) / o->step[0]) + 1.0;
    if (!(half >= 1.0) || (2.0 * half + 1.0) * (2.0 * half + 1.0) > (double)OCC_MAX_WINDOW_CELLS)
        return fail(h, CLD_ERR_ARG, f + ": the kernel window exceeds CLD_OCCUPANCY_MAX_WINDOW_CELLS cells");
    if (o->n_sem < 1 || o->n_sem > CLD_RASTER_MAX_PLANES || o->drivable_layer < 0 || o->drivable_layer >= o->n_sem)
        return fail(h, CLD_ERR_ARG, f + ": drivable_layer must be one of the n_sem >= 1 layers");
    if (o->maps && (!o->scene_map || !o->map_from_world || o->num_maps < 1 || o->map_h < 1 || o->map_w < 1 ||
                    (int64_t)o->map_h * o->map_w > INT32_MAX))
        return fail(h, CLD_ERR_ARG, f + ": maps need scene_map, map_from_world, num_maps, map_h and map_w");
    *a = OccArgs{};
    a->scene_start = o->scene_start; a->window = o->window; a->cell_start = reinterpret_cast<const long long*>(o->cell_start);
    a->maps = o->maps; a->scene_map = o->scene_map; a->map_from_world = o->map_from_world;
    a->cells = o->cells; a->o0 = o->offset[0]; a->o1 = o->offset[1]; a->s0 = o->step[0]; a->s1 = o->step[1]; a->sigma = o->sigma;
    a->num_scenes = o->num_scenes; a->B_all = o->B_all; a->n_sem = o->n_sem; a->num_maps = o->num_maps; a->map_h = o->map_h;
    a->map_w = o->map_w; a->layer = o->drivable_layer; a->N = (int)half; a->fill = o->no_map_fill;
    return CLD_OK;
}

int cld_occupancy_splat(cld_handle h, const cld_occupancy* o, const float* world, uint64_t* grid, uint64_t* dropped, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!world || !grid || !dropped) return fail(h, CLD_ERR_ARG, "cld_occupancy_splat: null argument (world, grid or dropped)");
    OccArgs a;
    int rc = check_occupancy(h, "cld_occupancy_splat", o, &a);
    if (rc) return rc;
    a.world = world; a.grid = reinterpret_cast<unsigned long long*>(grid); a.dropped = reinterpret_cast<unsigned long long*>(dropped);
    HIPCK(h, launch_occupancy_splat(a, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_occupancy_mark(cld_handle h, const cld_occupancy* o, const float* world, int32_t n_steps, const uint8_t* ok, uint8_t* success,
                       void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!world || !ok || !success) return fail(h, CLD_ERR_ARG, "cld_occupancy_mark: null argument (world, ok or success)");
    OccArgs a;
    int rc = check_occupancy(h, "cld_occupancy_mark", o, &a);
    if (rc) return rc;
    if (n_steps < 1 || (int64_t)n_steps * o->B_all > INT32_MAX) return fail(h, CLD_ERR_ARG, "cld_occupancy_mark: n_steps out of range");
    a.world = world; a.n_steps = n_steps; a.ok = ok; a.success = success;
    HIPCK(h, launch_occupancy_mark(a, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_occupancy_read(cld_handle h, const cld_occupancy* o, const uint64_t* grid, const uint8_t* success, double threshold,
                       int64_t* counts, double* values, uint8_t* lane, uint64_t* mass, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!grid) return fail(h, CLD_ERR_ARG, "cld_occupancy_read: null argument (grid)");
    if (!counts && !values && !lane && !mass) return fail(h, CLD_ERR_ARG, "cld_occupancy_read: no output");
    if (!(threshold >= 0.0) || !(threshold <= 1048576.0)) return fail(h, CLD_ERR_ARG, "cld_occupancy_read: threshold must be in [0, 2^20]");
    OccArgs a;
    int rc = check_occupancy(h, "cld_occupancy_read", o, &a);
    if (rc) return rc;
    a.grid_in = reinterpret_cast<const unsigned long long*>(grid); a.success_in = success;
    a.thr_q = (unsigned long long)std::rint(threshold * 1099511627776.0);
    a.counts = reinterpret_cast<long long*>(counts); a.values = values; a.lane = lane; a.mass = reinterpret_cast<unsigned long long*>(mass);
    HIPCK(h, launch_occupancy_read(a, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

/* ---- realism deviation: terms, fp32 sort, Wasserstein-1 (realism_kernels.hip) ---- */
int32_t cld_debug_sort_items_per_block(void) { return SORT_TILE; }

size_t cld_sort_workspace_bytes(int64_t n) { return n < 1 || n > SORT_MAX_N ? 0 : sort_ws_bytes(n); }

int cld_sort_f32(cld_handle h, const float* in, float* out, int64_t n, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!in || !out) return fail(h, CLD_ERR_ARG, "cld_sort_f32: null pointer");
    if (n < 1 || n > SORT_MAX_N) return fail(h, CLD_ERR_ARG, "cld_sort_f32: n must be in [1, 2^30]");
    if (!workspace || workspace_bytes < sort_ws_bytes(n)) return fail(h, CLD_ERR_WORKSPACE, "cld_sort_f32: workspace too small");
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(h, CLD_ERR_ARG, "cld_sort_f32: workspace must be 16-byte aligned");
    HIPCK(h, launch_sort_f32(in, out, n, workspace, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

size_t cld_wasserstein_workspace_bytes(int64_t nu, int64_t nv) {
    return nu < 1 || nv < 1 || nu > SORT_MAX_N || nv > SORT_MAX_N ? 0 : (size_t)w1_tiles(nu, nv) * sizeof(double);
}

int cld_wasserstein_f32(cld_handle h, const float* u_sorted, int64_t nu, const float* v_sorted, int64_t nv, double* out, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!u_sorted || !v_sorted || !out) return fail(h, CLD_ERR_ARG, "cld_wasserstein_f32: null pointer");
    if (nu < 1 || nv < 1 || nu > SORT_MAX_N || nv > SORT_MAX_N) return fail(h, CLD_ERR_ARG, "cld_wasserstein_f32: nu and nv must be in [1, 2^30]");
    if (!workspace || workspace_bytes < cld_wasserstein_workspace_bytes(nu, nv))
        return fail(h, CLD_ERR_WORKSPACE, "cld_wasserstein_f32: workspace too small");
    if (reinterpret_cast<uintptr_t>(workspace) % 8 || reinterpret_cast<uintptr_t>(out) % 8)
        return fail(h, CLD_ERR_ARG, "cld_wasserstein_f32: out and workspace must be 8-byte aligned");
    HIPCK(h, launch_wasserstein_f32(u_sorted, nu, v_sorted, nv, out, workspace, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_realism_terms(cld_handle h, const float* sa, int64_t M, int32_t T, float dt, float* lon, float* lat, float* jerk, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!sa || (!lon && !lat && !jerk)) return fail(h, CLD_ERR_ARG, "cld_realism_terms: null pointer (sa, or no output)");
    if (M < 1 || T < 2 || M > SORT_MAX_N / T) return fail(h, CLD_ERR_ARG, "cld_realism_terms: needs M >= 1, T >= 2 and M T <= 2^30");
    if (!(dt > 0.f) || !(dt < INFINITY)) return fail(h, CLD_ERR_ARG, "cld_realism_terms: dt must be positive and finite");
    HIPCK(h, launch_realism_terms(sa, M, T, dt, lon, lat, jerk, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

/* ---- open-loop sample metrics: ADE / FDE and diversity (sample_metrics_kernels.hip; include/cld_eval.h) ---- */
static_assert(CLD_SM_COLS == kSmCols && CLD_SM_MAX_SAMPLES == kSmMaxN && CLD_SM_MAX_POINTS == kSmMaxNT, "cld_eval.h and sample_metrics_kernels.h");

int32_t cld_debug_sample_metrics_max_blocks(void) { return kSmMaxBlocks; }

size_t cld_sample_metrics_workspace_bytes(int32_t B) { return B < 1 || B > kSmMaxB ? 0 : sm_fold_tiles(B) * kSmCols * sizeof(double); }

int cld_sample_metrics(cld_handle h, const float* pred, int32_t C, const float* gt, const float* avail, int32_t B, int32_t N, int32_t T,
                       double* per_agent, int32_t* index, double* means, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CLD_ERR_ARG;
    if (!pred || !gt || !avail || !per_agent || !index) return fail(h, CLD_ERR_ARG, "cld_sample_metrics: null pointer");
    if (B < 1 || B > kSmMaxB) return fail(h, CLD_ERR_ARG, "cld_sample_metrics: B out of range [1, 2^20]");
    if (N < 1 || T < 1) return fail(h, CLD_ERR_ARG, "cld_sample_metrics: N and T must be at least 1");
    if (C < 2 || C > 8) return fail(h, CLD_ERR_ARG, "cld_sample_metrics: C must be 2 .. 8 (channels 0 and 1 are the positions)");
    if (N > kSmMaxN || (int64_t)N * T > kSmMaxNT)
        return fail(h, CLD_ERR_ARG, "cld_sample_metrics: N = " + std::to_string(N) + ", T = " + std::to_string(T) + " is beyond N <= " +
                                        std::to_string(kSmMaxN) + ", N T <= " + std::to_string(kSmMaxNT) + " (an agent's samples are staged in LDS)");
    if (reinterpret_cast<uintptr_t>(per_agent) % 8 || reinterpret_cast<uintptr_t>(means) % 8)
        return fail(h, CLD_ERR_ARG, "cld_sample_metrics: per_agent and means must be 8-byte aligned");
    if (means && (!workspace || workspace_bytes < cld_sample_metrics_workspace_bytes(B) || reinterpret_cast<uintptr_t>(workspace) % 8))
        return fail(h, CLD_ERR_WORKSPACE, "cld_sample_metrics: workspace missing, misaligned or too small");
    SampleMetricsArgs a{pred, gt, avail, per_agent, index, B, N, T, C};
    HIPCK(h, launch_sample_metrics(a, means, static_cast<double*>(workspace), static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

/* ---- training: what the U-Net and the LSTM-VAE entry points share ---- */
static int param_info(cld_handle h, const char* fn, const TrainParam* table, int count, int32_t i, const char** name, size_t* offset,
                      size_t* numel, int32_t* shape, int32_t* ndim) {
    if (i < 0 || i >= count) return fail(h, CLD_ERR_ARG, std::string(fn) + ": index out of range");
    const TrainParam& p = table[i];
    if (name) *name = p.name;
    if (offset) *offset = p.offset;
    if (numel) *numel = p.numel;
    if (ndim) *ndim = p.ndim;
    if (shape)
        for (int d = 0; d < 3; ++d) shape[d] = d < p.ndim ? p.shape[d] : 1;
    return CLD_OK;
}

// the checks every training call starts with: a handle, exact fp32
static int check_f32(cld_handle h, const char* fn) {
    if (!h) return CLD_ERR_ARG;
    if (h->precision != CLD_PRECISION_F32)
        return fail(h, CLD_ERR_STATE, std::string(fn) + ": training runs in exact fp32 only (this handle is CLD_PRECISION_F16X2)");
    return CLD_OK;
}
static int check_rows(cld_handle h, const char* fn, int B) {
    if (B < 1 || B > (1 << 20)) return fail(h, CLD_ERR_ARG, std::string(fn) + ": B out of range [1, 2^20]");
    return CLD_OK;
}
static bool misaligned(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) % 16) return true;
    return false;
}

/* ---- U-Net training (train_kernels.hip) ---- */
int cld_unet_param_count(cld_handle) { return kTrainParams; }

int cld_unet_param_info(cld_handle h, int32_t i, const char** name, size_t* offset, size_t* numel, int32_t* shape, int32_t* ndim) {
    return param_info(h, "cld_unet_param_info", train_params(), kTrainParams, i, name, offset, numel, shape, ndim);
}

size_t cld_unet_param_floats(cld_handle) { return train_param_floats(); }

size_t cld_unet_tape_bytes(cld_handle, int32_t B) { return B < 1 ? 0 : train_tape_floats(B) * sizeof(float); }

size_t cld_unet_train_workspace_bytes(cld_handle, int32_t B) { return B < 1 ? 0 : train_ws_floats(B) * sizeof(float); }

static int check_train(cld_handle h, const char* fn, int B, const void* tape, size_t tape_bytes, const void* ws, size_t ws_bytes) {
    if (int rc = check_f32(h, fn)) return rc;
    if (!h->finalized || !h->has_unet) return fail(h, CLD_ERR_STATE, std::string(fn) + ": the handle has no finalized U-Net weights (model.*)");
    if (int rc = check_rows(h, fn, B)) return rc;
    if (!tape || tape_bytes < cld_unet_tape_bytes(h, B)) return fail(h, CLD_ERR_WORKSPACE, std::string(fn) + ": tape too small");
    if (!ws || ws_bytes < cld_unet_train_workspace_bytes(h, B)) return fail(h, CLD_ERR_WORKSPACE, std::string(fn) + ": workspace too small");
    if (misaligned({ws, tape}))
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": workspace and tape must be 16-byte aligned");
    return CLD_OK;
}

int cld_unet_train_forward(cld_handle h, const float* params, const float* x, const float* cond, const int32_t* t_idx, float* eps,
                           float* tape, size_t tape_bytes, int32_t B, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_train(h, "cld_unet_train_forward", B, tape, tape_bytes, workspace, workspace_bytes);
    if (rc) return rc;
    if (!params || !x || !cond || !t_idx || !eps) return fail(h, CLD_ERR_ARG, "cld_unet_train_forward: null pointer");
    HIPCK(h, train_forward(params, x, cond, t_idx, eps, tape, B, static_cast<float*>(workspace), static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_unet_backward(cld_handle h, const float* params, const float* x, const float* cond, const int32_t* t_idx, const float* tape,
                      size_t tape_bytes, const float* d_eps, float* d_params, float* dx, float* dcond, int32_t accumulate, int32_t B,
                      void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_train(h, "cld_unet_backward", B, tape, tape_bytes, workspace, workspace_bytes);
    if (rc) return rc;
    (void)cond; (void)t_idx;      // their contribution is on the tape (tc = [time_mlp(t) | cond])
    if (!params || !x || !d_eps) return fail(h, CLD_ERR_ARG, "cld_unet_backward: null pointer");
    if (accumulate != 0 && accumulate != 1) return fail(h, CLD_ERR_ARG, "cld_unet_backward: accumulate must be 0 or 1");
    HIPCK(h, train_backward(params, x, tape, d_eps, d_params, dx, dcond, accumulate, B, static_cast<float*>(workspace),
                            static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

/* ---- LSTM-VAE training (vae_train_kernels.hip) ---- */
int cld_vae_param_count(cld_handle) { return kVaeParams; }

int cld_vae_param_info(cld_handle h, int32_t i, const char** name, size_t* offset, size_t* numel, int32_t* shape, int32_t* ndim) {
    return param_info(h, "cld_vae_param_info", vae_params(), kVaeParams, i, name, offset, numel, shape, ndim);
}

size_t cld_vae_param_floats(cld_handle) { return vae_param_floats(); }

size_t cld_vae_tape_bytes(cld_handle, int32_t part, int32_t B) {
    return (B < 1 || (part != CLD_VAE_ENCODER && part != CLD_VAE_DECODER)) ? 0 : vae_tape_floats(B) * sizeof(float);
}

size_t cld_vae_train_workspace_bytes(cld_handle, int32_t B) { return B < 1 ? 0 : vae_ws_floats(B) * sizeof(float); }

// ws == nullptr: the forward (no workspace)
static int check_vae(cld_handle h, const char* fn, int part, int B, const float* params, const void* tape, size_t tape_bytes, const void* ws,
                     size_t ws_bytes, bool backward) {
    if (int rc = check_f32(h, fn)) return rc;
    if (int rc = check_rows(h, fn, B)) return rc;
    if (!params) return fail(h, CLD_ERR_ARG, std::string(fn) + ": null pointer");
    if (!tape || tape_bytes < cld_vae_tape_bytes(h, part, B)) return fail(h, CLD_ERR_WORKSPACE, std::string(fn) + ": tape too small");
    if (backward && (!ws || ws_bytes < cld_vae_train_workspace_bytes(h, B)))
        return fail(h, CLD_ERR_WORKSPACE, std::string(fn) + ": workspace too small");
    if (misaligned({params, tape, ws}))
        return fail(h, CLD_ERR_ARG, std::string(fn) + ": params, workspace and tape must be 16-byte aligned");
    return CLD_OK;
}

int cld_vae_encode_train(cld_handle h, const float* params, const float* x6, const float* cond, const float* drop_mask, float* mu,
                         float* logvar, float* tape, size_t tape_bytes, int32_t B, void* stream) {
    int rc = check_vae(h, "cld_vae_encode_train", CLD_VAE_ENCODER, B, params, tape, tape_bytes, nullptr, 0, false);
    if (rc) return rc;
    if (!x6 || !cond || !mu || !logvar) return fail(h, CLD_ERR_ARG, "cld_vae_encode_train: null pointer");
    HIPCK(h, vae_train_forward(0, params, x6, cond, drop_mask, mu, logvar, tape, B, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_vae_encode_backward(cld_handle h, const float* params, const float* x6, const float* cond, const float* drop_mask,
                            const float* tape, size_t tape_bytes, const float* d_mu, const float* d_logvar, float* d_params, float* dx6,
                            float* dcond, int32_t accumulate, int32_t B, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_vae(h, "cld_vae_encode_backward", CLD_VAE_ENCODER, B, params, tape, tape_bytes, workspace, workspace_bytes, true);
    if (rc) return rc;
    if (!x6 || !cond) return fail(h, CLD_ERR_ARG, "cld_vae_encode_backward: null pointer");
    if (accumulate != 0 && accumulate != 1) return fail(h, CLD_ERR_ARG, "cld_vae_encode_backward: accumulate must be 0 or 1");
    HIPCK(h, vae_train_backward(0, params, x6, cond, drop_mask, tape, d_mu, d_logvar, d_params, dx6, dcond, accumulate, B,
                                static_cast<float*>(workspace), static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_vae_decode_train(cld_handle h, const float* params, const float* z, const float* cond, const float* drop_mask, float* act,
                         float* tape, size_t tape_bytes, int32_t B, void* stream) {
    int rc = check_vae(h, "cld_vae_decode_train", CLD_VAE_DECODER, B, params, tape, tape_bytes, nullptr, 0, false);
    if (rc) return rc;
    if (!z || !cond || !act) return fail(h, CLD_ERR_ARG, "cld_vae_decode_train: null pointer");
    HIPCK(h, vae_train_forward(1, params, z, cond, drop_mask, act, nullptr, tape, B, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_vae_decode_backward(cld_handle h, const float* params, const float* z, const float* cond, const float* drop_mask,
                            const float* tape, size_t tape_bytes, const float* d_act, float* d_params, float* dz, float* dcond,
                            int32_t accumulate, int32_t B, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_vae(h, "cld_vae_decode_backward", CLD_VAE_DECODER, B, params, tape, tape_bytes, workspace, workspace_bytes, true);
    if (rc) return rc;
    if (!z || !cond) return fail(h, CLD_ERR_ARG, "cld_vae_decode_backward: null pointer");
    if (accumulate != 0 && accumulate != 1) return fail(h, CLD_ERR_ARG, "cld_vae_decode_backward: accumulate must be 0 or 1");
    HIPCK(h, vae_train_backward(1, params, z, cond, drop_mask, tape, d_act, nullptr, d_params, dz, dcond, accumulate, B,
                                static_cast<float*>(workspace), static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

/* ---- reconstruction guidance (include/cld_recon.h; recon_kernels.hip) ---- */
// The step's own buffers behind the sampler workspace: rows Bn = B, or 2 B with CFG ([0, B) conditional, [B, 2 B) unconditional).
struct ReconWs {
    float *xt, *cond2, *eps, *deps, *dx, *x0, *g0, *tape, *tws;
    int32_t* tidx;
};
static size_t recon_al(size_t floats) { return (floats + 63) / 64 * 64; }
static size_t recon_sampler_bytes(cld_handle h, int B, bool cfg) {
    return (cld_workspace_bytes(h, cfg ? 2 * pad16(B) : B) + 255) / 256 * 256;
}
static size_t recon_own_floats(int B, bool cfg) {
    const size_t bn = cfg ? 2 * (size_t)B : (size_t)B;
    return 4 * recon_al(bn * T * D) + recon_al(bn * 256) + recon_al(bn) + 2 * recon_al((size_t)B * T * D) + recon_al(train_tape_floats((int)bn)) +
           recon_al(train_ws_floats((int)bn));
}
static ReconWs recon_carve(cld_handle h, void* ws, int B, bool cfg) {
    const size_t bn = cfg ? 2 * (size_t)B : (size_t)B;
    float* p = reinterpret_cast<float*>(static_cast<char*>(ws) + recon_sampler_bytes(h, B, cfg));
    ReconWs r;
    r.xt = p; p += recon_al(bn * T * D);
    r.eps = p; p += recon_al(bn * T * D);
    r.deps = p; p += recon_al(bn * T * D);
    r.dx = p; p += recon_al(bn * T * D);
    r.cond2 = p; p += recon_al(bn * 256);
    r.tidx = reinterpret_cast<int32_t*>(p); p += recon_al(bn);
    r.x0 = p; p += recon_al((size_t)B * T * D);
    r.g0 = p; p += recon_al((size_t)B * T * D);
    r.tape = p; p += recon_al(train_tape_floats((int)bn));
    r.tws = p;
    return r;
}

size_t cld_recon_workspace_bytes(cld_handle h, int32_t B, int32_t cfg) {
    if (!h || B < 1 || B > (1 << 19)) return 0;
    return recon_sampler_bytes(h, B, cfg != 0) + recon_own_floats(B, cfg != 0) * sizeof(float);
}

int cld_recon_get_posterior(cld_handle h, float* coef1, float* coef2) {
    if (!h) return CLD_ERR_ARG;
    const size_t n = h->post_coef1.size() * sizeof(float);
    if (coef1) std::memcpy(coef1, h->post_coef1.data(), n);
    if (coef2) std::memcpy(coef2, h->post_coef2.data(), n);
    return CLD_OK;
}

int32_t cld_debug_recon_grid_cap(int32_t cap) { return recon_grid_cap(cap); }

// what both calls check before anything is launched; *g2 receives the guidance as run_guidance is to see it: ONE evaluation of the
// gradient, the optimiser fields (which these calls do not read) set to values that make its own update a no-op nobody looks at
static int check_recon(cld_handle h, const char* fn, const cld_guidance* gd, const cld_recon* rc, int B, bool cfg, int iters,
                       const void* ws, size_t ws_bytes, cld_guidance* g2) {
    if (int r = check_f32(h, fn)) return r;
    if (!h->finalized || !h->has_unet) return fail(h, CLD_ERR_STATE, std::string(fn) + ": the handle has no finalized U-Net weights (model.*)");
    if (B < 1 || B > (1 << 19)) return fail(h, CLD_ERR_ARG, std::string(fn) + ": B out of range [1, 2^19]");
    if (!gd || !rc) return fail(h, CLD_ERR_ARG, std::string(fn) + ": null guidance or recon");
    if (!rc->params) return fail(h, CLD_ERR_ARG, std::string(fn) + ": recon->params is NULL (the flat U-Net buffer of cld_unet_param_info)");
    if (gd->grad_steps > 1) return fail(h, CLD_ERR_ARG, std::string(fn) + ": grad_steps > 1 cannot run in this mode (upstream's second backward() goes through a freed graph)");
    if (gd->apply_output) return fail(h, CLD_ERR_ARG, std::string(fn) + ": apply_output is not part of this mode");
    if (gd->no_intermediate) return fail(h, CLD_ERR_ARG, std::string(fn) + ": no_intermediate leaves nothing to guide");
    if (!ws || ws_bytes < cld_recon_workspace_bytes(h, B, cfg)) return fail(h, CLD_ERR_WORKSPACE, std::string(fn) + ": workspace too small (cld_recon_workspace_bytes)");
    if (misaligned({ws, rc->params})) return fail(h, CLD_ERR_ARG, std::string(fn) + ": workspace and params must be 16-byte aligned");
    *g2 = *gd;
    g2->lr = 1.f; g2->perturb_th = -1.f; g2->optimizer = CLD_GUIDE_SGD; g2->grad_steps = 1; g2->final_grad_steps = 0; g2->guide_clean = 0;
    return check_guidance(h, fn, g2, B, iters);
}

// One guided iteration (t = i > 0) on the latent in r.xt (both halves with CFG); leaves x_{i-1} there.
static int recon_iteration(cld_handle h, const Ws& w, const ReconWs& r, bool cfg, int B, int i, const float* z, uint64_t seed,
                           unsigned long long salt, float guidance_w, const cld_guidance* g2, const cld_recon* rc, float* x_next,
                           float* x0_hat, float* grad_xt, float* x0_guided, float* mean, hipStream_t s) {
    const int bn = cfg ? 2 * B : B;
    const size_t half = (size_t)B * T * D;
    const long rows = (long)B * T;
    const float sigma = std::exp(0.5f * h->plvc[i]);
    const float rca = h->sqrt_recip_acp[i], rm1 = h->sqrt_recipm1_acp[i];
    HIPCK(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(r.tidx), i, (size_t)bn, s));
    HIPCK(h, train_forward(rc->params, r.xt, r.cond2, r.tidx, r.eps, r.tape, bn, r.tws, s));
    ReconHeadArgs ha{};
    ha.eps_c = r.eps; ha.eps_u = cfg ? r.eps + half : nullptr; ha.x_t = r.xt; ha.x0_hat = r.x0;
    ha.cfg_w = guidance_w; ha.rc = rca; ha.rm1 = rm1; ha.rows = rows;
    HIPCK(h, launch_recon_head(ha, s));
    // g0 = dL/dx0_hat: the mean-guided step's machinery on x0_hat, asked for its gradient only
    if (int rcg = run_guidance(h, w, g2, B, true, sigma, 0.f, r.x0, r.cond2, nullptr, seed, salt, nullptr, nullptr, nullptr, r.g0, s)) return rcg;
    ReconSeedArgs sa{};
    sa.g0 = r.g0; sa.d_eps_c = r.deps; sa.d_eps_u = cfg ? r.deps + half : nullptr; sa.rows = rows;
    sa.cc = cfg ? -(rm1 * (1.0f + guidance_w)) : -rm1; sa.cu = rm1 * guidance_w;
    HIPCK(h, launch_recon_seed(sa, s));
    HIPCK(h, train_backward(rc->params, r.xt, r.tape, r.deps, nullptr, r.dx, nullptr, 0, bn, r.tws, s));
    ReconUpdateArgs ua{};
    ua.g0 = r.g0; ua.dx_c = r.dx; ua.dx_u = cfg ? r.dx + half : nullptr; ua.x0_hat = r.x0; ua.x_t = r.xt; ua.z = z;
    ua.x_out = r.xt; ua.x_out2 = cfg ? r.xt + half : nullptr; ua.x_next = x_next; ua.grad_xt = grad_xt; ua.x0_guided = x0_guided; ua.mean = mean;
    const float lr_t = rc->lr > 0.f ? rc->lr : sigma;
    ua.rc = rca; ua.slr = rc->descend ? -lr_t : lr_t;
    if (rc->perturb_th < 0.f) ua.th = -1.f;
    else if (rc->perturb_th == 0.f) ua.th = sigma;
    else {      // diffuser.py:888-891, in double and rounded once
        const double sc = 2.0 / (1.0 + std::exp(-10.0 * (double)i / (double)h->cfg.n_timesteps)) - 1.0;
        ua.th = (float)(sc * (4.0 - (double)rc->perturb_th) + (double)rc->perturb_th);
    }
    ua.c1 = h->post_coef1[i]; ua.c2 = h->post_coef2[i]; ua.sigma = sigma; ua.seed = seed; ua.salt = salt; ua.rows = rows;
    HIPCK(h, launch_recon_update(ua, s));
    if (x0_hat) HIPCK(h, hipMemcpyAsync(x0_hat, r.x0, half * sizeof(float), hipMemcpyDeviceToDevice, s));
    return CLD_OK;
}

// the rows the taped passes read besides the latent, and what the unguided t = 0 iteration needs in the sampler workspace
static int recon_prepare(cld_handle h, const Ws& w, const ReconWs& r, bool cfg, int B, const float* x, const float* cond, const float* non_cond,
                         hipStream_t s) {
    const int bp = pad16(B);
    const size_t half = (size_t)B * T * D;
    HIPCK(h, hipMemcpyAsync(r.xt, x, half * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCK(h, hipMemcpyAsync(r.cond2, cond, (size_t)B * 256 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCK(h, launch_cond_bias(cond, h->wc, h->cbias_b, w.cb, B, bp, NCB, s));
    if (cfg) {
        HIPCK(h, hipMemcpyAsync(r.xt + half, x, half * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCK(h, hipMemcpyAsync(r.cond2 + (size_t)B * 256, non_cond, (size_t)B * 256 * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCK(h, launch_cond_bias(non_cond, h->wc, h->cbias_b, w.cb + (size_t)bp * NCB, B, bp, NCB, s));
    }
    return CLD_OK;
}

// t = 0: the sampler's own unguided iteration on the latent in r.xt; leaves x_0 in w.xw and its mean in w.meanb
static int recon_last(cld_handle h, const Ws& w, const ReconWs& r, bool cfg, int B, const float* z, uint64_t seed, unsigned long long salt,
                      const float* cond, float guidance_w, hipStream_t s) {
    const int bp = pad16(B);
    if (int r0 = load_inputs(h, w, B, bp, r.xt, nullptr, nullptr, cfg, s)) return r0;
    return sample_iteration(h, w, cfg, B, bp, 0, z, seed, salt, cond, guidance_w, nullptr, nullptr, nullptr, false, s);
}

int cld_recon_step(cld_handle h, const float* x_t, const float* cond, const float* non_cond, float guidance_w, const cld_guidance* gd,
                   const cld_recon* rc, int32_t t_idx, const float* z, float* x_next, float* x0_hat, float* grad_xt, float* x0_guided,
                   float* mean, float* sigma_host, int32_t B, uint64_t seed, uint64_t salt, void* workspace, size_t workspace_bytes,
                   void* stream) {
    const bool cfg = non_cond != nullptr;
    cld_guidance g2;
    const int iters = salt < 65536 ? (int)salt + 1 : 65536;
    int r0 = check_recon(h, "cld_recon_step", gd, rc, B, cfg, iters, workspace, workspace_bytes, &g2);
    if (r0) return r0;
    if (!x_t || !cond) return fail(h, CLD_ERR_ARG, "cld_recon_step: null pointer");
    if (t_idx < 0 || t_idx >= h->cfg.n_timesteps) return fail(h, CLD_ERR_ARG, "cld_recon_step: timestep out of range");
    if (sigma_host) *sigma_host = std::exp(0.5f * h->plvc[t_idx]);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int bp = pad16(B);
    Ws w = carve(workspace, cfg ? 2 * bp : bp);
    ReconWs r = recon_carve(h, workspace, B, cfg);
    if ((r0 = recon_prepare(h, w, r, cfg, B, x_t, cond, non_cond, s)) != CLD_OK) return r0;
    if (t_idx > 0) return recon_iteration(h, w, r, cfg, B, t_idx, z, seed, salt, guidance_w, &g2, rc, x_next, x0_hat, grad_xt, x0_guided, mean, s);
    if ((r0 = recon_last(h, w, r, cfg, B, z, seed, salt, cond, guidance_w, s)) != CLD_OK) return r0;
    if (x_next) HIPCK(h, launch_unpack(w.xw, x_next, B, s));
    if (mean) HIPCK(h, launch_unpack(w.meanb, mean, B, s));
    return CLD_OK;
}

int cld_sample_recon(cld_handle h, const float* x_T, const float* noise, const float* cond, const float* non_cond, float guidance_w,
                     const cld_guidance* gd, const cld_recon* rc, int32_t steps, float* x0, float* x1, float* logp, int32_t B,
                     uint64_t seed, void* workspace, size_t workspace_bytes, void* stream) {
    const bool cfg = non_cond != nullptr;
    cld_guidance g2;
    int r0 = check_recon(h, "cld_sample_recon", gd, rc, B, cfg, steps > 0 ? steps : 1, workspace, workspace_bytes, &g2);
    if (r0) return r0;
    if (!x_T || !cond) return fail(h, CLD_ERR_ARG, "cld_sample_recon: null pointer");
    if (steps != loop_steps(h))
        return fail(h, CLD_ERR_ARG, "cld_sample_recon: steps must equal len(range(0, n_timesteps, stride)) = " + std::to_string(loop_steps(h)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int bp = pad16(B);
    Ws w = carve(workspace, cfg ? 2 * bp : bp);
    ReconWs r = recon_carve(h, workspace, B, cfg);
    if ((r0 = recon_prepare(h, w, r, cfg, B, x_T, cond, non_cond, s)) != CLD_OK) return r0;
    for (int it = 0; it < steps; ++it) {
        const int i = (steps - 1 - it) * h->stride;
        const float* z = noise ? noise + (size_t)it * B * T * D : nullptr;
        if (i > 0) {
            r0 = recon_iteration(h, w, r, cfg, B, i, z, seed, (unsigned long long)it, guidance_w, &g2, rc, i == 1 ? x1 : nullptr, nullptr, nullptr,
                                 nullptr, nullptr, s);
            if (r0) return r0;
        } else {
            if ((r0 = recon_last(h, w, r, cfg, B, z, seed, (unsigned long long)it, cond, guidance_w, s)) != CLD_OK) return r0;
            if (x0) HIPCK(h, launch_unpack(w.xw, x0, B, s));
            if (logp) HIPCK(h, launch_logprob(w.xw, w.meanb, std::exp(0.5f * h->plvc[0]), logp, B, s));
        }
    }
    return CLD_OK;
}

/* ---- few-step sampling (include/cld_solver.h; solver_kernels.hip) ---- */
namespace {

// what one step applies: the coefficients of cld_solver.h in double, rounded to fp32 once
struct SolverCoef { float a, b, c0, c1, rc, rm1, sigma, sigma_g; int form; bool second; };

int check_solver(cld_handle h, const char* fn, const cld_solver* sv) {
    if (!h) return CLD_ERR_ARG;
    if (!sv) return fail(h, CLD_ERR_ARG, std::string(fn) + ": null solver");
    if (sv->kind != CLD_SOLVER_DDIM && sv->kind != CLD_SOLVER_DPMPP_2M) return fail(h, CLD_ERR_ARG, std::string(fn) + ": unknown solver kind (CLD_SOLVER_DDIM / CLD_SOLVER_DPMPP_2M)");
    if (sv->n_steps < 1) return fail(h, CLD_ERR_ARG, std::string(fn) + ": n_steps < 1 (K >= 1 timesteps)");
    if (!sv->timesteps) return fail(h, CLD_ERR_ARG, std::string(fn) + ": null timesteps");
    for (int k = 0; k < sv->n_steps; ++k) {
        if (sv->timesteps[k] < 0 || sv->timesteps[k] >= h->cfg.n_timesteps)
            return fail(h, CLD_ERR_ARG, std::string(fn) + ": timestep out of range [0, n_timesteps) at index " + std::to_string(k));
        if (k && sv->timesteps[k] >= sv->timesteps[k - 1])
            return fail(h, CLD_ERR_ARG, std::string(fn) + ": timesteps not strictly decreasing at index " + std::to_string(k));
    }
    if (!(sv->eta >= 0.f && sv->eta <= 1.f)) return fail(h, CLD_ERR_ARG, std::string(fn) + ": eta outside [0, 1]");
    if (sv->kind == CLD_SOLVER_DPMPP_2M && sv->eta != 0.f) return fail(h, CLD_ERR_ARG, std::string(fn) + ": DPM-Solver++(2M) is deterministic: eta != 0 is refused");
    return CLD_OK;
}

SolverCoef solver_coef(cld_handle h, const cld_solver* sv, int k) {
    const int K = sv->n_steps;
    const bool last = k == K - 1;
    auto acp = [&](int kk) { return kk >= K ? 1.0 : (double)h->acp[sv->timesteps[kk]]; };
    auto lam = [&](int kk) { const double a = acp(kk); return 0.5 * std::log(a / (1.0 - a)); };     // finite for kk < K
    const double as = acp(k), ap = acp(k + 1);
    SolverCoef c{};
    c.rc = (float)std::sqrt(1.0 / as);
    c.rm1 = (float)std::sqrt(1.0 / as - 1.0);
    const double jump = (1.0 - ap) / (1.0 - as) * (1.0 - as / ap);      // the DDPM posterior variance of the jump s -> p
    c.sigma_g = (float)std::sqrt(std::max(jump, 1e-20));
    c.c0 = 1.f; c.c1 = 0.f;
    if (sv->kind == CLD_SOLVER_DDIM) {
        const double var = (double)sv->eta * (double)sv->eta * jump;
        c.sigma = last ? 0.f : (float)std::sqrt(var);
        c.a = (float)std::sqrt(ap / as);
        c.b = (float)(std::sqrt(std::max(1.0 - ap - var, 0.0)) - std::sqrt(ap * (1.0 - as) / as));
        c.form = SOLVER_FORM_DDIM;
    } else {
        c.sigma = 0.f;
        c.a = (float)std::sqrt((1.0 - ap) / (1.0 - as));
        // -sqrt(acp_p) expm1(-h): the last step has lambda_p = +inf, expm1(-inf) = -1
        c.b = last ? 1.f : (float)(-std::sqrt(ap) * std::expm1(-(lam(k + 1) - lam(k))));
        c.second = k > 0 && !last;
        if (c.second) {
            const double r = (lam(k) - lam(k - 1)) / (lam(k + 1) - lam(k));
            c.c0 = (float)(1.0 + 1.0 / (2.0 * r)); c.c1 = (float)(1.0 / (2.0 * r));
        }
        c.form = SOLVER_FORM_2M;
    }
    if (last) c.form = SOLVER_FORM_FINAL;
    return c;
}

// the scalar arguments of the step kernel: coefficients, CFG weights, the generator's key
SolverStepArgs solver_kernel_args(const SolverCoef& c, float guidance_w, int k, uint64_t seed, int B) {
    SolverStepArgs q{};
    q.w1 = (float)(1.0 + (double)guidance_w); q.nw = -guidance_w; q.rc = c.rc; q.nrm1 = -c.rm1;
    q.a = c.a; q.b = c.b; q.c0 = c.c0; q.nc1 = -c.c1; q.sigma = c.sigma; q.form = c.form;
    q.seed = seed; q.salt = (unsigned long long)k; q.rows = (long)B * T;
    return q;
}

size_t solver_sampler_bytes(cld_handle h, int B, bool cfg) { return (cld_workspace_bytes(h, cfg ? 2 * pad16(B) : B) + 255) / 256 * 256; }

int check_solver_call(cld_handle h, const char* fn, const cld_solver* sv, const cld_guidance* gd, int B, bool cfg, const void* ws, size_t ws_bytes) {
    if (!h) return CLD_ERR_ARG;
    int rc = check_solver(h, fn, sv);
    if (rc) return rc;
    if (B > (1 << 19)) return fail(h, CLD_ERR_ARG, std::string(fn) + ": B out of range [1, 2^19]");
    if ((rc = check_common(h, fn, cfg ? 2 * pad16(B) : B, 0, ws, ws_bytes)) != CLD_OK) return rc;
    if (ws_bytes < cld_solver_workspace_bytes(h, B, cfg)) return fail(h, CLD_ERR_WORKSPACE, std::string(fn) + ": workspace too small (cld_solver_workspace_bytes)");
    if (gd) {
        if (gd->guide_clean != 0) return fail(h, CLD_ERR_ARG, std::string(fn) + ": guide_clean != 0 is not built on the few-step path (mean-form guidance only)");
        if ((rc = check_guidance(h, fn, gd, B, sv->n_steps)) != CLD_OK) return rc;
    }
    return CLD_OK;
}

// Step k on the latent in w.xw (CFG: rows [bp, 2 bp) hold the same latent, w.cb the conditional / unconditional bias rows): U-Net,
// head (noise prediction only, both halves uncombined), the solver kernel, optional guidance step on its deterministic part.
// Leaves x' in w.xw (both halves) and x0_hat in `hist` (when given; a second-order step reads the preceding one from it first).
int solver_iteration(cld_handle h, const Ws& w, const cld_solver* sv, int k, bool cfg, int B, int bp, float* hist, const float* z, uint64_t seed,
                     const float* cond, float guidance_w, const cld_guidance* gd, float* x0_hat, float* mu, float* mu_guided, float* grad,
                     hipStream_t s) {
    const int bpn = cfg ? 2 * bp : bp;
    const size_t half = (size_t)bp * T * D;
    const SolverCoef c = solver_coef(h, sv, k);
    const bool last = k == sv->n_steps - 1;
    const bool guide = gd && (last ? gd->apply_output != 0 : !gd->no_intermediate);
    h->fuse_upd = nullptr;                               // the tail chain leaves the update to the kernel below
    HIPCK(h, run_unet(h, w, w.xw, sv->timesteps[k], bpn, s));
    HeadArgs a{};
    head_source(h, w, a); a.w = h->head_w; a.b = h->head_b; a.x = w.xw; a.eps_out = w.xtmp; a.B = bpn; a.b_pad = bpn;
    HIPCK(h, launch_head(a, s));
    SolverStepArgs q = solver_kernel_args(c, guidance_w, k, seed, B);
    q.x = w.xw; q.eps_c = w.xtmp; q.eps_u = cfg ? w.xtmp + half : nullptr;
    q.x0_prev = c.second ? hist : nullptr; q.z = z; q.hist = hist;
    q.x_out = guide ? nullptr : w.xw; q.x_out2 = (guide || !cfg) ? nullptr : w.xw + half; q.det_out = guide ? w.meanb : nullptr;
    q.x0_out = x0_hat; q.mu_out = mu;
    if (guide) q.sigma = 0.f;                            // the guidance kernel adds sigma_k z behind its step
    HIPCK(h, launch_solver_step(q, s));
    if (guide)
        return run_guidance(h, w, gd, B, !last, c.sigma_g, c.sigma, w.meanb, cond, z, seed, (unsigned long long)k, mu_guided, w.xw,
                            cfg ? w.xw + half : nullptr, grad, s);
    return CLD_OK;
}

}  // namespace

size_t cld_solver_workspace_bytes(cld_handle h, int32_t B, int32_t cfg) {
    if (!h || B < 1 || B > (1 << 19)) return 0;
    return solver_sampler_bytes(h, B, cfg != 0) + (size_t)B * T * D * sizeof(float);
}

int32_t cld_debug_solver_grid_cap(int32_t cap) { return solver_grid_cap(cap); }

int cld_debug_solver_kernel(cld_handle h, const cld_solver* sv, int32_t k, const float* x, const float* eps_c, const float* eps_u, float guidance_w,
                            const float* x0_prev, const float* z, float* x_next, float* x0_hat, float* mu, int32_t B, uint64_t seed, void* stream) {
    int rc = check_solver(h, "cld_debug_solver_kernel", sv);
    if (rc) return rc;
    if (B < 1 || B > (1 << 19)) return fail(h, CLD_ERR_ARG, "cld_debug_solver_kernel: B out of range [1, 2^19]");
    if (k < 0 || k >= sv->n_steps) return fail(h, CLD_ERR_ARG, "cld_debug_solver_kernel: step index out of range [0, n_steps)");
    if (!x || !eps_c) return fail(h, CLD_ERR_ARG, "cld_debug_solver_kernel: null pointer");
    const SolverCoef c = solver_coef(h, sv, k);
    if (c.second && !x0_prev) return fail(h, CLD_ERR_ARG, "cld_debug_solver_kernel: a second-order step (2M, 0 < k < K-1) needs x0_prev");
    if (misaligned({x, eps_c, eps_u, x0_prev, z, x_next, x0_hat, mu})) return fail(h, CLD_ERR_ARG, "cld_debug_solver_kernel: tensors must be 16-byte aligned");
    SolverStepArgs q = solver_kernel_args(c, guidance_w, k, seed, B);
    q.x = x; q.eps_c = eps_c; q.eps_u = eps_u; q.x0_prev = c.second ? x0_prev : nullptr; q.z = z;
    q.x_out = x_next; q.x0_out = x0_hat; q.mu_out = mu;
    HIPCK(h, launch_solver_step(q, static_cast<hipStream_t>(stream)));
    return CLD_OK;
}

int cld_solver_tables(cld_handle h, const cld_solver* sv, float* table) {
    int rc = check_solver(h, "cld_solver_tables", sv);
    if (rc) return rc;
    if (!table) return fail(h, CLD_ERR_ARG, "cld_solver_tables: null pointer");
    for (int k = 0; k < sv->n_steps; ++k) {
        const SolverCoef c = solver_coef(h, sv, k);
        float* t = table + (size_t)k * CLD_SOLVER_TABLE_COLS;
        t[0] = c.a; t[1] = c.b; t[2] = c.c0; t[3] = c.c1; t[4] = c.rc; t[5] = c.rm1; t[6] = c.sigma; t[7] = c.sigma_g;
    }
    return CLD_OK;
}

int cld_solver_step(cld_handle h, const cld_solver* sv, int32_t k, const float* x_t, float* x0_prev, const float* z, const float* cond,
                    const float* non_cond, float guidance_w, const cld_guidance* gd, float* x_next, float* x0_hat, float* mu,
                    float* mu_guided, float* grad, int32_t B, uint64_t seed, void* workspace, size_t workspace_bytes, void* stream) {
    const bool cfg = non_cond != nullptr;
    int rc = check_solver_call(h, "cld_solver_step", sv, gd, B, cfg, workspace, workspace_bytes);
    if (rc) return rc;
    if (!x_t || !cond) return fail(h, CLD_ERR_ARG, "cld_solver_step: null pointer");
    if (k < 0 || k >= sv->n_steps) return fail(h, CLD_ERR_ARG, "cld_solver_step: step index out of range [0, n_steps)");
    if (sv->kind == CLD_SOLVER_DPMPP_2M && k > 0 && k < sv->n_steps - 1 && !x0_prev)
        return fail(h, CLD_ERR_ARG, "cld_solver_step: a second-order step (2M, 0 < k < K-1) needs x0_prev");
    if (misaligned({x_t, x0_prev, z, x_next, x0_hat, mu, mu_guided, grad})) return fail(h, CLD_ERR_ARG, "cld_solver_step: tensors must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int bp = pad16(B);
    Ws w = carve(workspace, cfg ? 2 * bp : bp);
    if ((rc = load_inputs(h, w, B, bp, x_t, cond, non_cond, cfg, s)) != CLD_OK) return rc;
    if ((rc = solver_iteration(h, w, sv, k, cfg, B, bp, x0_prev, z, seed, cond, guidance_w, gd, x0_hat, mu, mu_guided, grad, s)) != CLD_OK) return rc;
    if (x_next) HIPCK(h, launch_unpack(w.xw, x_next, B, s));
    return CLD_OK;
}

int cld_sample_solver(cld_handle h, const cld_solver* sv, const float* x_T, const float* noise, const float* cond, const float* non_cond,
                      float guidance_w, const cld_guidance* gd, float* x0, int32_t B, uint64_t seed, void* workspace, size_t workspace_bytes,
                      void* stream) {
    const bool cfg = non_cond != nullptr;
    int rc = check_solver_call(h, "cld_sample_solver", sv, gd, B, cfg, workspace, workspace_bytes);
    if (rc) return rc;
    if (!x_T || !cond) return fail(h, CLD_ERR_ARG, "cld_sample_solver: null pointer");
    if (misaligned({x_T, noise, x0})) return fail(h, CLD_ERR_ARG, "cld_sample_solver: tensors must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int bp = pad16(B);
    Ws w = carve(workspace, cfg ? 2 * bp : bp);
    float* hist = reinterpret_cast<float*>(static_cast<char*>(workspace) + solver_sampler_bytes(h, B, cfg));
    if ((rc = load_inputs(h, w, B, bp, x_T, cond, non_cond, cfg, s)) != CLD_OK) return rc;
    for (int k = 0; k < sv->n_steps; ++k) {
        rc = solver_iteration(h, w, sv, k, cfg, B, bp, hist, noise ? noise + (size_t)k * B * T * D : nullptr, seed, cond, guidance_w, gd, nullptr,
                              nullptr, nullptr, nullptr, s);
        if (rc) return rc;
    }
    if (x0) HIPCK(h, launch_unpack(w.xw, x0, B, s));
    return CLD_OK;
}

}  // extern "C"
