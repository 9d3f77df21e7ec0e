// metrics_kernels.hip -- the closed-loop episode metrics on the device: what upstream's OffRoadRate, DiskOffRoadRate, CollisionRate,
// DiskCollisionRate, CriticalFailure and Comfort (src/tbsim/envs/env_metrics.py:147-311, 391-646, 1436-1501) compute on the host from every
// pose of every step, from the world poses cld_world_step leaves in HBM (include/cld.h `cld_scene_metrics_step` for the definitions).
//
// scene_metrics_step_kernel, one launch per environment step: one wave per agent, so every reduction is a wave operation and nothing is
// atomic.  Lanes 0 .. 51 are the 52 disk samples of the off-road test and lane 52 the centroid; each looks its raster pixel up in the map
// with the arithmetic raster_kernel uses for the drivable plane, and two ballots give the two flags.  The wave then strides over its scene
// 64 partners at a time (poses are read through L2: 12 bytes per partner, shared by every wave of the scene): a ballot of the disk test,
// a ballot of the separating-axis test, and the first set bit of the first non-empty ballot is the lowest-index partner.  The type of
// the box collision is clipped against that one partner.  Lane 0 then updates the agent's own accumulator row in place: the same bits on
// every run.  scene_metrics_read_kernel, one workgroup per scene, finalises the rows and sums them in a fixed order (fp64 partials per
// thread, a fixed LDS tree).  Plain fp32 in both library precisions.
#include "cld_kernels.h"
#include "metrics_device.h"

namespace cld {

namespace {
constexpr int kWaves = 4;                 // agents per workgroup of the step kernel
constexpr int kReadThreads = 256;
constexpr int kSceneCols = METRICS_SCENE_COLS, kAgentCols = METRICS_AGENT_COLS;

enum : unsigned int { BIT_ANY = 1u, BIT_FRONT = 2u, BIT_REAR = 4u, BIT_SIDE = 8u, BIT_DISK = 16u, BIT_FAIL_OFF = 32u, BIT_FAIL_COLL = 64u };

// the accumulator row of one agent; all-zero = empty
struct MetricsRow {
    unsigned int seen, valid, off_sum, disk_sum, bits, ring_n;
    float ring[3][3];                     // the last three down-sampled poses (x, y, h), oldest first
    float prev_acc;                       // |acc| of the previous down-sampled step (has_prev)
    unsigned int has_prev;
    unsigned int cnt[4];                  // speed, lon_acc, lat_acc, jerk: terms that were not NaN
    double sum[4];
    unsigned int reserved[2];
};
static_assert(sizeof(MetricsRow) == METRICS_ROW_BYTES, "cld_scene_metrics_state_bytes");

// the length of the segment (x0, y0) -> (x1, y1), of length `len`, inside the box |x| <= b0, |y| <= b1 (Liang-Barsky)
__device__ inline float clipped_length(float x0, float y0, float x1, float y1, float len, float b0, float b1) {
    float t0 = 0.f, t1 = 1.f;
    const float dx = x1 - x0, dy = y1 - y0;
    const float pp[4] = {-dx, dx, -dy, dy}, qq[4] = {x0 + b0, b0 - x0, y0 + b1, b1 - y0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (pp[e] == 0.f) {
            if (qq[e] < 0.f) return 0.f;
            continue;
        }
        const float r = qq[e] / pp[e];
        if (pp[e] < 0.f) {
            if (r > t1) return 0.f;
            t0 = fmaxf(t0, r);
        } else {
            if (r < t0) return 0.f;
            t1 = fminf(t1, r);
        }
    }
    return (t1 - t0) * len;
}

__global__ __launch_bounds__(kWaves * 64) void scene_metrics_step_kernel(const MetricsArgs p) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= p.B_all) return;                                    // (a whole wave; the kernel has no barrier)
    const float xi = p.world[(size_t)i * 3], yi = p.world[(size_t)i * 3 + 1], hi_ = p.world[(size_t)i * 3 + 2];
    const float a0 = 0.5f * p.extent[(size_t)i * 3], a1 = 0.5f * p.extent[(size_t)i * 3 + 1];
    const float ri = 0.5f * fminf(p.extent[(size_t)i * 3], p.extent[(size_t)i * 3 + 1]);
    const bool valid = !(isnan(xi) || isnan(yi));
    const float c = cosf(hi_), s = sinf(hi_);
    const int sc = mdev::scene_of(p.scene_start, p.num_scenes, i);

    // ---- off road: lane 52 the centroid pixel, lanes 0 .. 51 the disk samples (radius index major, as upstream reshapes them)
    unsigned int off = 0u, dsk = 0u;
    if (valid) {
        float fu = p.ox, fv = p.oy;
        if (lane < 52) mdev::disk_sample(p, ri, lane, fu, fv);
        const float x = mdev::raster_value(p, sc, xi, yi, c, s, fu, fv);      // raster_kernel's semantic plane, for this one pixel
        const unsigned long long bad = __ballot(lane <= 52 && x == 0.f);
        off = (unsigned int)((bad >> 52) & 1ull);
        dsk = (bad & ((1ull << 52) - 1ull)) ? 1u : 0u;
    }

    // ---- collisions: the scene, 64 partners at a time
    int partner = -1;
    unsigned int disk_hit = 0u;
    if (valid) {
        const int j0 = max(p.scene_start[sc], 0), j1 = min(p.scene_start[sc + 1], p.B_all);
        for (int base = j0; base < j1; base += 64) {
            const int j = base + lane;
            bool dhit = false, bhit = false;
            if (j < j1 && j != i) {
                const float xj = p.world[(size_t)j * 3], yj = p.world[(size_t)j * 3 + 1], hj = p.world[(size_t)j * 3 + 2];
                const float e0 = p.extent[(size_t)j * 3], e1 = p.extent[(size_t)j * 3 + 1];
                if (!(isnan(xj) || isnan(yj))) {
                    float dist, rsum;
                    mdev::pair_hits(xi, yi, c, s, a0, a1, ri, xj, yj, hj, e0, e1, dist, rsum, bhit);
                    dhit = dist < rsum;
                }
            }
            if (__ballot(dhit)) disk_hit = 1u;
            const unsigned long long bm = __ballot(bhit);
            if (partner < 0 && bm) partner = base + __ffsll((long long)bm) - 1;
        }
    }
    unsigned int code = 0u;                                      // 0 none, 1 FRONT, 2 REAR, 3 SIDE
    if (partner >= 0) {
        const float xj = p.world[(size_t)partner * 3], yj = p.world[(size_t)partner * 3 + 1], hj = p.world[(size_t)partner * 3 + 2];
        const float b0 = 0.5f * p.extent[(size_t)partner * 3], b1 = 0.5f * p.extent[(size_t)partner * 3 + 1];
        const float cj = cosf(hj), sj = sinf(hj);
        float qx[4], qy[4];                                      // i's corners (+,+) (+,-) (-,+) (-,-) in the partner's frame
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float f0 = (k & 2) ? -a0 : a0, f1 = (k & 1) ? -a1 : a1;
            const float wx = (xi - xj) + (f0 * c - f1 * s), wy = (yi - yj) + (f0 * s + f1 * c);
            qx[k] = wx * cj + wy * sj;
            qy[k] = wy * cj - wx * sj;
        }
        const float len[4] = {clipped_length(qx[0], qy[0], qx[1], qy[1], 2.f * a1, b0, b1),       // front: the + e0 / 2 side
                              clipped_length(qx[2], qy[2], qx[3], qy[3], 2.f * a1, b0, b1),       // rear
                              clipped_length(qx[0], qy[0], qx[2], qy[2], 2.f * a0, b0, b1),       // left: the + e1 / 2 side
                              clipped_length(qx[1], qy[1], qx[3], qy[3], 2.f * a0, b0, b1)};      // right
        int best = 0;
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (len[k] > len[best]) best = k;                    // argmax, the first wins
        code = 1u + (unsigned int)min(best, 2);
    }

    if (lane != 0) return;
    if (p.flags) {
        unsigned char* f = p.flags + (size_t)i * 4;
        f[0] = valid ? (unsigned char)off : 255;
        f[1] = valid ? (unsigned char)dsk : 255;
        f[2] = (unsigned char)disk_hit;
        f[3] = (unsigned char)code;
    }
    if (p.partner) p.partner[i] = partner;
    MetricsRow& st = reinterpret_cast<MetricsRow*>(p.state)[i];
    st.seen += 1u;
    unsigned int bits = st.bits;
    if (valid) {
        st.valid += 1u;
        st.off_sum += off;
        st.disk_sum += dsk;
        if (off) bits |= BIT_FAIL_OFF;
    }
    if (code) bits |= BIT_ANY | BIT_FAIL_COLL | (1u << code);    // (1 << code: BIT_FRONT, BIT_REAR, BIT_SIDE)
    if (disk_hit) bits |= BIT_DISK;
    st.bits = bits;
    if (p.step % p.ratio) return;
    // ---- comfort: this pose joins the ring; NaN terms are not counted
#pragma unroll
    for (int k = 0; k < 3; ++k) { st.ring[0][k] = st.ring[1][k]; st.ring[1][k] = st.ring[2][k]; }
    st.ring[2][0] = xi; st.ring[2][1] = yi; st.ring[2][2] = hi_;
    const unsigned int n = st.ring_n + 1u;
    st.ring_n = n;
    if (n < 2u) return;
    const float inv_dt = 1.f / p.dt;
    const float v2x = (st.ring[2][0] - st.ring[1][0]) * inv_dt, v2y = (st.ring[2][1] - st.ring[1][1]) * inv_dt;
    const float speed = sqrtf(v2x * v2x + v2y * v2y);
    if (!isnan(speed)) { st.sum[0] += (double)speed; st.cnt[0] += 1u; }
    if (n < 3u) return;
    const float v1x = (st.ring[1][0] - st.ring[0][0]) * inv_dt, v1y = (st.ring[1][1] - st.ring[0][1]) * inv_dt;
    const float ddx = (v2x - v1x) * inv_dt, ddy = (v2y - v1y) * inv_dt;
    const float acc = sqrtf(ddx * ddx + ddy * ddy);
    const float lon = fabsf(acc * cosf(st.ring[0][2])), lat = fabsf(acc * sinf(st.ring[0][2]));      // the yaw of the first of the three
    if (!isnan(lon)) { st.sum[1] += (double)lon; st.cnt[1] += 1u; }
    if (!isnan(lat)) { st.sum[2] += (double)lat; st.cnt[2] += 1u; }
    if (st.has_prev) {
        const float jerk = fabsf((acc - st.prev_acc) * inv_dt);
        if (!isnan(jerk)) { st.sum[3] += (double)jerk; st.cnt[3] += 1u; }
    }
    st.prev_acc = acc;
    st.has_prev = 1u;
}

__global__ __launch_bounds__(kReadThreads) void scene_metrics_read_kernel(const MetricsArgs p) {
    __shared__ double part[kReadThreads];
    __shared__ unsigned int cnt[kReadThreads];
    const int sc = blockIdx.x, tid = threadIdx.x;
    const int j0 = max(p.scene_start[sc], 0), j1 = max(min(p.scene_start[sc + 1], p.B_all), j0);
    const MetricsRow* rows = reinterpret_cast<const MetricsRow*>(p.state);
    const float nan = __int_as_float(0x7fc00000);
    // per scene: [0] sum of valid, [1] off_sum, [2] disk_sum, [3..7] any / front / rear / side / disk, [8..10] failures, [11..14] comfort
    double acc[15];
    unsigned int have[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 15; ++k) acc[k] = 0.0;
    for (int j = j0 + tid; j < j1; j += kReadThreads) {
        const MetricsRow& st = rows[j];
        float row[kAgentCols];
        row[0] = (float)st.seen; row[1] = (float)st.valid; row[2] = (float)st.off_sum; row[3] = (float)st.disk_sum;
        row[4] = st.bits & BIT_ANY ? 1.f : 0.f; row[5] = st.bits & BIT_FRONT ? 1.f : 0.f; row[6] = st.bits & BIT_REAR ? 1.f : 0.f;
        row[7] = st.bits & BIT_SIDE ? 1.f : 0.f; row[8] = st.bits & BIT_DISK ? 1.f : 0.f;
        row[9] = st.bits & BIT_FAIL_OFF ? 1.f : 0.f; row[10] = st.bits & BIT_FAIL_COLL ? 1.f : 0.f;
        row[11] = st.bits & (BIT_FAIL_OFF | BIT_FAIL_COLL) ? 1.f : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) row[12 + k] = st.cnt[k] ? (float)(st.sum[k] / (double)st.cnt[k]) : nan;
        if (p.per_agent)
#pragma unroll
            for (int k = 0; k < kAgentCols; ++k) p.per_agent[(size_t)j * kAgentCols + k] = row[k];
#pragma unroll
        for (int k = 0; k < 11; ++k) acc[k] += (double)row[1 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (st.cnt[k]) { acc[11 + k] += (double)row[12 + k]; have[k] += 1u; }
    }
    if (!p.per_scene) return;
    double tot[15];
    unsigned int tothave[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < 15; ++k) {                               // a fixed tree per quantity: the same bits on every run
        part[tid] = acc[k];
        if (k >= 11) cnt[tid] = have[k - 11];
        __syncthreads();
        for (int w = kReadThreads >> 1; w > 0; w >>= 1) {
            if (tid < w) {
                part[tid] += part[tid + w];
                if (k >= 11) cnt[tid] += cnt[tid + w];
            }
            __syncthreads();
        }
        tot[k] = part[0];
        if (k >= 11) tothave[k - 11] = cnt[0];
        __syncthreads();
    }
    if (tid != 0) return;
    float* o = p.per_scene + (size_t)sc * kSceneCols;
    const double n = (double)(j1 - j0);
    o[0] = (float)(tot[1] / tot[0]); o[1] = (float)(tot[1] / n);                  // OffRoadRate: rate (0 / 0 = NaN), nframe
    o[2] = (float)(tot[2] / tot[0]); o[3] = (float)(tot[2] / n);                  // DiskOffRoadRate
    o[4] = (float)(tot[4] / n); o[5] = (float)(tot[5] / n); o[6] = (float)(tot[6] / n); o[7] = (float)(tot[3] / n);   // CollisionRate
    o[8] = (float)(tot[7] / n);                                                   // DiskCollisionRate coll_any
    o[9] = (float)(tot[8] / n); o[10] = (float)(tot[9] / n); o[11] = (float)(tot[10] / n);                            // CriticalFailure
    for (int k = 0; k < 4; ++k) o[12 + k] = tothave[k] ? (float)(tot[11 + k] / (double)tothave[k]) : nan;            // Comfort
}
}  // namespace

hipError_t launch_scene_metrics_step(const MetricsArgs& a, hipStream_t s) {
    const unsigned int blocks = ((unsigned int)a.B_all + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(scene_metrics_step_kernel, dim3(blocks), dim3(kWaves * 64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scene_metrics_read(const MetricsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(scene_metrics_read_kernel, dim3((unsigned int)a.num_scenes), dim3(kReadThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace cld
