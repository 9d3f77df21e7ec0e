// sample_metrics_kernels.h -- launch interface of the open-loop sample metrics (sample_metrics_kernels.hip; include/cld_eval.h is the
// public side).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace cld {

constexpr int kSmCols = 10;                 // cld_eval.h CLD_SM_COLS
constexpr int kSmMaxBlocks = 2048;          // workgroups of one launch; more agents are taken in further grid-stride passes
constexpr int kSmMaxN = 256;                // cld_eval.h CLD_SM_MAX_SAMPLES: one lane per sample
constexpr int kSmMaxNT = 8192;              // cld_eval.h CLD_SM_MAX_POINTS: two fp32 planes of N T values = 64 KB of LDS
constexpr int kSmFoldTile = 256;            // per-agent rows one partial of the batch mean covers
constexpr int kSmMaxB = 1 << 20;

inline size_t sm_fold_tiles(int B) { return ((size_t)B + kSmFoldTile - 1) / kSmFoldTile; }

struct SampleMetricsArgs {
    const float* pred;     // [B, N, T, C]: channels 0 and 1 are read
    const float* gt;       // [B, T, 2]
    const float* avail;    // [B, T]
    double* per_agent;     // [B, kSmCols]
    int* index;            // [B, 4]: best_ade, best_fde, last, nonfinite
    int B, N, T, C;
};
// the per-agent rows and, when `means` is given, their batch means through `ws` (sm_fold_tiles(B) * kSmCols doubles)
hipError_t launch_sample_metrics(const SampleMetricsArgs& a, double* means, double* ws, hipStream_t s);

}  // namespace cld
