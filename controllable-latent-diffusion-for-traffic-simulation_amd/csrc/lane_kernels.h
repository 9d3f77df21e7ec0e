// lane_kernels.h -- launch interface of the lane guidance (lane_kernels.hip; include/cld_lane.h is the public side).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cld {

enum { LANE_FOLLOWING = 0, LANE_CHANGE_LEFT = 1, LANE_FOLLOW_DECAYED = 2 };   // cld_lane.h CLD_LANE_*
constexpr int kLaneMaxPts = 1024;                                            // cld_lane.h CLD_LANE_MAX_PTS

// world-frame polylines -> agent-frame fp32 polylines sorted by (x, original index), NaN rows last
struct LanePrepareArgs {
    const double* world_lines;       // [num_lines, max_pts, 3] (x, y, heading), NaN-padded
    const int* line_frame;           // [num_lines] index into agent_from_world
    const float* agent_from_world;   // [num_frames, 3, 3]
    float* lines;                    // [num_lines, max_pts, 3]
    int num_lines, max_pts, num_frames;
};
hipError_t launch_lane_prepare(const LanePrepareArgs& a, hipStream_t s);

// upstream's lane-projection losses + their gradient w.r.t. the decoded plans (guidance_loss.py:1574-1628, 1795-1841, 1958-2011)
struct LaneArgs {
    const float* traj;               // [rows = A * num_samp, 52, 6] descaled plans, sample-minor
    const float* lines;              // [num_lines, max_pts, 3] prepared polylines
    const int* agent;                // [num_entries] agent (batch) index; an agent's entries are contiguous
    const int* line;                 // [num_entries]
    const int* kind;                 // [num_entries] LANE_*
    const float* decay;              // [num_entries] LANE_FOLLOW_DECAYED only
    const float* scale;              // [num_entries] d total / d value of an (entry, sample)
    float* value;                    // [num_entries, num_samp] or null
    float* proj;                     // [num_entries, num_samp, 52, 3] or null
    float* grad;                     // [rows, 52, 6] or null; the kernel ADDS to it (launch_lane puts grad_in there first)
    int rows, num_entries, num_lines, max_pts, num_samp;
};
// grad = grad_in (or 0) + the term's gradient; grad_in may be grad itself
hipError_t launch_lane(const LaneArgs& a, const float* grad_in, hipStream_t s);

}  // namespace cld
