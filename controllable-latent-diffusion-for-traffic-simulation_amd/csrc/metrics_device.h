// metrics_device.h -- the fp32 flag arithmetic the two scorers share: scene_metrics_step_kernel (metrics_kernels.hip) and
// guide_metrics_step_kernel (guide_metrics_kernels.hip) decide the disk test, the separating-axis test and the off-road pixel lookup with
// these functions, so on the same poses their flags are the same bits (include/cld.h `cld_scene_metrics_step` for the definitions).
// The args structs of both kernels name the raster and map fields alike (maps, scene_map, map_from_world, num_maps, n_sem, layer, map_h,
// map_w, H, W, ppm, ox, oy, fill); the functions are templates over that struct.
#pragma once
#include <hip/hip_runtime.h>

namespace cld {
namespace mdev {

// cos, sin of linspace(0, 2 pi, 13), formed in double (both ends kept, as upstream's batch_detect_off_road_disk does)
static __device__ const float kDiskCos[13] = {(float)1.0, (float)0.8660254037844387, (float)0.5000000000000001, (float)6.123233995736766e-17,
                                              (float)-0.4999999999999998, (float)-0.8660254037844387, (float)-1.0, (float)-0.8660254037844386,
                                              (float)-0.5000000000000004, (float)-1.8369701987210297e-16, (float)0.5000000000000001,
                                              (float)0.8660254037844384, (float)1.0};
static __device__ const float kDiskSin[13] = {(float)0.0, (float)0.49999999999999994, (float)0.8660254037844386, (float)1.0,
                                              (float)0.8660254037844387, (float)0.49999999999999994, (float)1.2246467991473532e-16,
                                              (float)-0.5000000000000001, (float)-0.8660254037844384, (float)-1.0, (float)-0.8660254037844386,
                                              (float)-0.5000000000000004, (float)-2.4492935982947064e-16};

// disk sample `lane` (0 .. 51, radius index major) of an agent of disk radius ri (metres) -> its raster coordinates, clamped to the raster
template <class A>
__device__ __forceinline__ void disk_sample(const A& p, float ri, int lane, float& fu, float& fv) {
    const int k = lane / 13, a = lane - k * 13;
    const float rad = p.ppm * ri * (0.25f * (float)(k + 1));
    fu = fminf(fmaxf(p.ox + rad * kDiskCos[a], 0.f), (float)(p.W - 1));
    fv = fminf(fmaxf(p.oy + rad * kDiskSin[a], 0.f), (float)(p.H - 1));
}

// the value of the raster pixel nearest (fu, fv) (rounded half to even, clamped) of an agent of scene sc standing at (xi, yi) with heading
// (c, s) = (cos h, sin h): raster_kernel's semantic plane for this one pixel; 0.f = not drivable
template <class A>
__device__ __forceinline__ float raster_value(const A& p, int sc, float xi, float yi, float c, float s, float fu, float fv) {
    const int u = (int)fminf(fmaxf(rintf(fu), 0.f), (float)(p.W - 1)), v = (int)fminf(fmaxf(rintf(fv), 0.f), (float)(p.H - 1));
    int m = p.maps ? p.scene_map[sc] : -1;
    if (m >= p.num_maps) m = -1;
    float x = p.fill;
    if (m >= 0) {
        const float* M = p.map_from_world + (size_t)m * 9;
        const float inv_ppm = 1.f / p.ppm;
        const float ay = ((float)v - p.oy) * inv_ppm;
        const float ax = ((float)u - p.ox) * inv_ppm;
        const float wx = xi + (c * ax - s * ay), wy = yi + (s * ax + c * ay);
        const float mx = rintf(M[0] * wx + M[1] * wy + M[2]), my = rintf(M[3] * wx + M[4] * wy + M[5]);
        if (mx >= 0.f && mx < (float)p.map_w && my >= 0.f && my < (float)p.map_h)
            x = p.maps[((size_t)m * p.n_sem + p.layer) * p.map_h * p.map_w + (size_t)my * p.map_w + (size_t)mx];
    }
    return x;
}

// agent i at (xi, yi), heading (c, s), half extents a0, a1, disk radius ri against a VALID partner at (xj, yj, hj) with extents e0, e1:
// dist = the centre distance, rsum = the radius sum (the disk test is dist < rsum), bhit = the separating-axis test on the four edge normals
__device__ __forceinline__ void pair_hits(float xi, float yi, float c, float s, float a0, float a1, float ri, float xj, float yj, float hj,
                                          float e0, float e1, float& dist, float& rsum, bool& bhit) {
    const float dx = xj - xi, dy = yj - yi, b0 = 0.5f * e0, b1 = 0.5f * e1;
    dist = sqrtf(dx * dx + dy * dy);
    rsum = ri + 0.5f * fminf(e0, e1);
    const float cj = cosf(hj), sj = sinf(hj);
    const float cc = fabsf(c * cj + s * sj), cs = fabsf(c * sj - s * cj);      // |u_i . u_j| = |v_i . v_j|, |u_i . v_j| = |v_i . u_j|
    bhit = fabsf(dx * c + dy * s) <= a0 + b0 * cc + b1 * cs && fabsf(dy * c - dx * s) <= a1 + b0 * cs + b1 * cc &&
           fabsf(dx * cj + dy * sj) <= b0 + a0 * cc + a1 * cs && fabsf(dy * cj - dx * sj) <= b1 + a0 * cs + a1 * cc;
}

// scene_start[sc] <= i < scene_start[sc + 1]
__device__ __forceinline__ int scene_of(const int* scene_start, int num_scenes, int i) {
    int sc = 0, hi = num_scenes;
    while (hi - sc > 1) {
        const int mid = (sc + hi) >> 1;
        if (scene_start[mid] <= i) sc = mid; else hi = mid;
    }
    return sc;
}

}  // namespace mdev
}  // namespace cld
