// Internal interface of the exact-fp32 training paths of the U-Net (train_kernels.hip) and of the LSTM-VAE (vae_train_kernels.hip):
// the flat parameter tables, the tape and workspace sizes, and the forward / backward walks behind cld_unet_train_forward /
// cld_unet_backward / cld_vae_*_train / cld_vae_*_backward (include/cld.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <deque>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

// return the first HIP error of a walk
#define TRY(expr)                                  \
    do {                                           \
        hipError_t e__ = (expr);                   \
        if (e__ != hipSuccess) return e__;         \
    } while (0)

namespace cld {

inline unsigned nblk(long n) { return (unsigned)((n + 255) / 256); }

// the U-Net's 12 residual blocks (temporal.py:16-45 ResidualTemporalMapBlockConcat) in execution order (temporal.py:84-115,148-167)
struct BlockDef { const char* name; int cin, cout, L; };
inline constexpr BlockDef kBlocks[12] = {
    {"model.downs.0.0", 4, 64, 52},     {"model.downs.0.1", 64, 64, 52},    {"model.downs.1.0", 64, 128, 26},
    {"model.downs.1.1", 128, 128, 26},  {"model.downs.2.0", 128, 256, 13},  {"model.downs.2.1", 256, 256, 13},
    {"model.mid_block1", 256, 256, 13}, {"model.mid_block2", 256, 256, 13}, {"model.ups.0.0", 512, 128, 13},
    {"model.ups.0.1", 128, 128, 13},    {"model.ups.1.0", 256, 64, 26},     {"model.ups.1.1", 64, 64, 26},
};

struct TrainParam {
    const char* name;      // reference state_dict key (models/dm/dm_model.py: self.model = TemporalMapUnet(...))
    size_t offset, numel;  // floats into the flat buffer; offsets are multiples of kTrainAlign
    int ndim, shape[3];
};
constexpr int kTrainParams = 148;
constexpr size_t kTrainAlign = 64;   // floats (256 bytes)

// A model's tensors in state_dict order, each at the next aligned offset of one flat buffer.  A model derives from it and calls add()
// for every tensor in its constructor; the one instance lives for the whole process (the entries point into `names`).
struct ParamTable {
    std::vector<TrainParam> p;
    std::deque<std::string> names;      // a deque: add() must not move the earlier names
    std::map<std::string, int> idx;
    size_t floats = 0;
    ParamTable() = default;
    ParamTable(const ParamTable&) = delete;
    void add(const std::string& n, std::initializer_list<int> shape) {
        TrainParam t{};
        size_t numel = 1;
        for (int d : shape) { t.shape[t.ndim++] = d; numel *= d; }
        t.numel = numel;
        t.offset = floats;
        floats += (numel + kTrainAlign - 1) / kTrainAlign * kTrainAlign;
        idx[n] = (int)p.size();
        names.push_back(n);
        t.name = names.back().c_str();
        p.push_back(t);
    }
    size_t off(const std::string& n) const { return p[idx.at(n)].offset; }
};

const TrainParam* train_params();     // kTrainParams entries in state_dict order
size_t train_param_floats();           // length of the flat buffer (aligned offsets: > the 4,349,284 values)
size_t train_tape_floats(int B);
size_t train_ws_floats(int B);

// eps [B,52,4] = U-Net(x [B,52,4], cond [B,256], t [B]) from the raw fp32 weights in `params`; writes the tape.
hipError_t train_forward(const float* params, const float* x, const float* cond, const int32_t* t_idx, float* eps, float* tape,
                         int B, float* ws, hipStream_t s);
// d_params (nullable), dx [B,52,4] (nullable), dcond [B,256] (nullable) from d_eps [B,52,4] and the tape of train_forward.
hipError_t train_backward(const float* params, const float* x, const float* tape, const float* d_eps, float* d_params, float* dx,
                          float* dcond, int accumulate, int B, float* ws, hipStream_t s);

// The weight-gradient GEMM of the U-Net path (launch_wgrad in train_kernels.hip: wgrad_kernel + wreduce_kernel, K split over at
// most 256 row chunks, summed in a fixed order) for a Linear-shaped weight:
//   dw[m om + c] (+)= sum_{b < rows, l < lp} P[(b lp + l) p_ld + m] G[(b lg + l - pd) g_ld + c]   (c < gc; G rows outside [0, lg) read 0)
//   db[m], db2[m] (+)= sum_{b, l} P[(b lp + l) p_ld + m]                                           (each nullable)
// `part` holds train_wgrad_part_floats(M, gc) floats.
size_t train_wgrad_part_floats(int M, int gc);
hipError_t train_wgrad(const float* P, int lp, int p_ld, int M, const float* G, int lg, int g_ld, int gc, int pd, int rows, float* dw,
                       long om, float* db, float* db2, int accumulate, float* part, hipStream_t s);

// ---- LSTM-VAE training (vae_train_kernels.hip) ----
constexpr int kVaeParams = 26;
const TrainParam* vae_params();       // kVaeParams entries in LSTMVAE state_dict order
size_t vae_param_floats();
size_t vae_tape_floats(int B);        // the encoder's and the decoder's tape have the same size
size_t vae_ws_floats(int B);
// part 0 (encoder): x = x6 [B,52,6] -> out = mu, out2 = logvar [B,52,4]; part 1 (decoder): x = z [B,52,4] -> out = act [B,52,2].
// mask: [B,52,64] multiplied into layer 0's output where layer 1 reads it, or null.
hipError_t vae_train_forward(int part, const float* params, const float* x, const float* cond, const float* mask, float* out,
                             float* out2, float* tape, int B, hipStream_t s);
// d_out / d_out2: the cotangents of out / out2 (nullable: zero).  d_params, dx, dcond nullable.
hipError_t vae_train_backward(int part, const float* params, const float* x, const float* cond, const float* mask, const float* tape,
                              const float* d_out, const float* d_out2, float* d_params, float* dx, float* dcond, int accumulate, int B,
                              float* ws, hipStream_t s);

}  // namespace cld
