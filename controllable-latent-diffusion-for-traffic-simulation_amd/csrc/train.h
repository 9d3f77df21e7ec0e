// Internal interface of the exact-fp32 training path of the U-Net (train_kernels.hip): the flat parameter table, the tape and
// workspace sizes, and the forward / backward walks behind cld_unet_train_forward / cld_unet_backward (include/cld.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace cld {

struct TrainParam {
    const char* name;      // reference state_dict key (models/dm/dm_model.py: self.model = TemporalMapUnet(...))
    size_t offset, numel;  // floats into the flat buffer; offsets are multiples of kTrainAlign
    int ndim, shape[3];
};
constexpr int kTrainParams = 148;
constexpr size_t kTrainAlign = 64;   // floats (256 bytes)

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

}  // namespace cld
