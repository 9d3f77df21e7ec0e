/* cld_lane.h -- lane guidance of libcld_hip: upstream's lane-projection losses inside the sampler.  A header of its own beside cld.h
 * (whose table of entry points is pinned); everything of cld.h's conventions holds: DEVICE pointers, row-major, an int return
 * (CLD_OK / CLD_ERR_*), the message behind cld_last_error, `stream` a hipStream_t or NULL. */
#ifndef CLD_LANE_H
#define CLD_LANE_H

#include "cld.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Upstream's lane-projection losses (src/tbsim/utils/guidance_loss.py), classes it reaches only through its language-model front
 * end: LaneFollowingLoss (:1574-1628), ChangeToLeftLaneLoss (:1795-1841), FollowLaneLoss (:1958-2011).  All three rest on
 * get_lane_projection (src/tbsim/utils/trajdata_utils.py:573-664) and project_onto (:726-821): per agent a polyline [S,3] of
 * (x, y, heading) in the agent's own frame, transformed in fp64, rounded to fp32, NaN-padded and sorted by x (NaN last); every plan
 * point of every sample is projected onto it and the deviation penalised.  Which lane an agent is on (vec_map.get_current_lane, the
 * successor rule :617-639, get_neighbor_lane) is the caller's business: the library starts from world-frame polylines.
 *
 * Projection of a plan point p = (x, y) onto the polyline of its entry: segments j = 0 .. max_pts - 2 join consecutive rows,
 * d = p1 - p0, u = clip(((p - p0) . d) / |d|^2, 0, 1), proj = p0 + u d, dist = |p - proj|.  A segment with a NaN end, or of zero length
 * (upstream: 0 / 0 -> NaN distance -> +inf; a duplicated point, such as the junction of a lane and its successor), is never chosen.
 * The chosen segment is the lexicographic minimum of (dist, j): ties take the first index.  (Squared distances are compared, in
 * fp32.)  The projection is (proj.x, proj.y, heading of that segment's p0) and is a CONSTANT for the gradient: upstream detaches
 * positions and yaws before projecting.
 *
 * Entry k = (agent[k], line[k], kind[k], decay[k], scale[k]); dev = plan - projection on lines[line[k]], yaw = column 3 of the plan,
 * h the projection's heading.  The step's term e_t and value[k, n]:
 *     CLD_LANE_FOLLOWING        dx^2 + dy^2 + (yaw - h)^2, yaw not wrapped                        mean over t
 *     CLD_LANE_CHANGE_LEFT      sqrt(dx^2 + dy^2) + |yaw - h|  (on the LEFT lane's polyline)       mean over t
 *     CLD_LANE_FOLLOW_DECAYED   min(|dx| + |dy|, 5) decay^t / sum_t decay^t                        mean over t (so / 52 again, as
 *                                                                                                  the decayed pair relations)
 * The term's total is the sum over (k, n) of scale[k] * value[k, n]; LaneFollowingLoss(target_inds) with K targets is K entries of
 * scale weight / (num_samp K), its reported value their mean.  The gradient goes to columns 0, 1 (x, y) and 3 (yaw) of the plans of
 * agent[k]; the decayed form has no yaw term.  The norm's gradient at 0 is 0, abs at 0 gives 0, clip(max = 5) passes the gradient
 * where its argument is <= 5 (torch).
 * An agent may carry several entries (from different configurations): they must be CONTIGUOUS in the entry arrays and are summed
 * in their order.  Rows without an entry: gradient grad_in, bit for bit.  Deterministic: no atomics, the same bits on every run;
 * plain fp32 in both precisions.  Agents A = B / num_samp.
 * Contract on the device-side data (as cld_pair_term): an entry whose agent lies outside [0, A) or whose line lies outside
 * [0, num_lines), or whose polyline has no segment with a finite, non-zero length, is not evaluated -- NaN value, NaN projection,
 * no contribution.  NOT checked: that an agent's entries are contiguous -- an agent in two separate runs stays inside the arrays,
 * but two workgroups then add to one row and the bits of that row are no longer the same on every run.
 * Upstream runs these classes on a single-scene batch only (it indexes the full-batch projection with masked plans, the defect
 * recorded for MapCollisionLoss in cld.h); here agent indices are batch indices and the entries of all scenes go into one launch. */
enum { CLD_LANE_FOLLOWING = 0, CLD_LANE_CHANGE_LEFT = 1, CLD_LANE_FOLLOW_DECAYED = 2 };
#define CLD_LANE_MAX_PTS 1024       /* the bound on max_pts (the polyline is sorted and staged in LDS) */
typedef struct cld_lane_term {
    const float* lines;             /* DEVICE [num_lines, max_pts, 3] agent-frame polylines as cld_lane_prepare writes them */
    const int32_t* agent;           /* DEVICE [num_entries] agent (batch) index; an agent's entries are contiguous          */
    const int32_t* line;            /* DEVICE [num_entries] index into lines                                                */
    const int32_t* kind;            /* DEVICE [num_entries] CLD_LANE_*                                                      */
    const float* decay;             /* DEVICE [num_entries] CLD_LANE_FOLLOW_DECAYED: the decay rate                         */
    const float* scale;             /* DEVICE [num_entries] d total / d value of an (entry, sample)                         */
    int32_t num_entries;
    int32_t num_lines;
    int32_t max_pts;                /* 2 .. CLD_LANE_MAX_PTS */
    int32_t num_samp;
} cld_lane_term;

/* World-frame polylines -> the polylines a cld_lane_term reads.  world_lines [num_lines, max_pts, 3] DOUBLE (x, y, heading),
 * NaN-padded; line_frame [num_lines] picks the row of agent_from_world [num_frames,3,3] (float, as upstream's data_batch holds it).
 * Every point is transformed in fp64 -- x and y through the 3x3 matrix, heading' = atan2 of the rotated (cos h, sin h): this
 * project's definition of trajdata's transform_xyh_np, which is not part of the reference tree -- and rounded once to fp32; the
 * rows are then sorted by (x, original index), rows with a NaN x last (upstream's argsort leaves the order among equal x open;
 * here it is stable, and -0 counts as +0).  A line whose frame index lies outside [0, num_frames) comes out all NaN.
 * max_pts 1 .. CLD_LANE_MAX_PTS, more is CLD_ERR_ARG.  Meant to run once per plan (per get_action), not per denoising step. */
int cld_lane_prepare(cld_handle h, const double* world_lines, const int32_t* line_frame, const float* agent_from_world, float* lines,
                     int32_t num_lines, int32_t max_pts, int32_t num_frames, void* stream);

/* The losses above on given plans: traj [B,52,6] descaled -> value [num_entries, num_samp] (unweighted), proj [num_entries,
 * num_samp, 52, 3] (the projections, for tests) and grad [B,52,6] = grad_in (when given; may be grad itself) + d total / d traj.
 * Any output may be NULL, not all three. */
int cld_lane_loss(cld_handle h, const float* traj, const cld_lane_term* term, const float* grad_in, float* value, float* proj,
                  float* grad, int32_t B, void* stream);

/* Keep a lane term on the handle (the struct is copied by value; NULL clears it).  While one is set, every guided call
 * (cld_sample_guided, cld_sample_step, cld_guidance_step) adds its gradient after the pair term's, on the same decoded iterate; it
 * counts as a loss term of the `cld_guidance` it is used with.  A malformed term is CLD_ERR_ARG, decided before anything is
 * launched.  (A setter and not a pointer in cld_guidance: that struct's layout is frozen.) */
int cld_set_lane_term(cld_handle h, const cld_lane_term* term);

#ifdef __cplusplus
}
#endif

#endif
