// raster_kernels.hip -- the closed-loop observation raster built on the device from the scene: what upstream's parse_node_centric ->
// rasterize_agents (src/tbsim/utils/trajdata_utils.py:123-156, 381-420) hands the ContextEncoder as data_batch['image'], from the world
// poses cld_world_step leaves in HBM.  image [B, T_hist + n_sem, H, W]:
//   planes 0 .. T_hist-1 (oldest first)  the agents' positions at that history frame: every neighbour paints -1, the ego +1 on top, and flat
//                                         pixels 0 and H W - 1 are 0 afterwards (rasterize_agents :138-151, quirks kept: an unavailable frame
//                                         lands on pixel 0, an out-of-raster neighbour is clamped onto the border)
//   planes T_hist .. T_hist+n_sem-1      the scene's map layers sampled at the nearest map pixel, `no_map_fill` outside the map or without one
// drivable [B, H, W] bytes = (first semantic plane != 0) and raster_from_world [B, 3, 3] come out of the same launch.
//
// The kernel is bound by its stores (6.8 MB per agent at 34 x 224 x 224): one workgroup per (agent, plane) writes its plane once, in
// 16-byte stores that are contiguous over a wave.  A history plane is first painted into two H W-bit masks in LDS (ego, neighbour) with
// LDS atomics -- one lane per agent of the scene, any scene size -- and after one barrier the masks are expanded to floats, so the zeros and
// the painted pixels leave in the same pass and no store to HBM has to be ordered against another.  A semantic plane is four consecutive
// pixels per lane, each a gather from the map.  Planes whose size is no multiple of four pixels (or an unaligned image) take dword stores.
// Plain fp32 in both library precisions; deterministic (the masks are OR-ed, the result does not depend on the order).
#include "cld_kernels.h"

namespace cld {

namespace {
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void raster_kernel(const RasterArgs p) {
    extern __shared__ unsigned int mask[];                       // [2][words]: ego, neighbour
    const int C = p.T + p.n_sem, HW = p.H * p.W;
    const int i = blockIdx.x / C, plane = blockIdx.x - i * C, tid = threadIdx.x;
    const int r = p.row0 + i;
    const float* me = p.hist_world + ((size_t)r * p.T + (p.T - 1)) * 3;
    const float xi = me[0], yi = me[1], c = cosf(me[2]), s = sinf(me[2]);
    int sc = 0, hi = p.num_scenes;                               // scene_start[sc] <= r < scene_start[sc + 1]
    while (hi - sc > 1) {
        const int mid = (sc + hi) >> 1;
        if (p.scene_start[mid] <= r) sc = mid; else hi = mid;
    }
    float* out = p.image + ((size_t)i * C + plane) * HW;
    const int groups = (HW + 3) >> 2;

    if (plane == 0 && tid == 0 && p.raster_from_world) {         // raster_from_agent . agent_from_world
        float* m = p.raster_from_world + (size_t)i * 9;
        m[0] = p.ppm * c;  m[1] = p.ppm * s; m[2] = p.ppm * -(c * xi + s * yi) + p.ox;
        m[3] = -p.ppm * s; m[4] = p.ppm * c; m[5] = p.ppm * (s * xi - c * yi) + p.oy;
        m[6] = 0.f; m[7] = 0.f; m[8] = 1.f;
    }

    if (plane < p.T) {
        const int words = (HW + 31) >> 5;
        unsigned int *ego = mask, *nbr = mask + words;
        for (int w = tid; w < 2 * words; w += kThreads) mask[w] = 0u;
        __syncthreads();
        const int j0 = max(p.scene_start[sc], 0), j1 = min(p.scene_start[sc + 1], p.B_all);
        const float d2max = p.max_dist * p.max_dist;
        for (int j = j0 + tid; j < j1; j += kThreads) {
            // (all four loads are issued before anything is decided: one memory latency per agent, not three)
            const size_t row = (size_t)j * p.T;
            const unsigned char here_now = p.hist_avail[row + p.T - 1], here_then = p.hist_avail[row + plane];
            const float *qn = p.hist_world + (row + p.T - 1) * 3, *q = p.hist_world + (row + plane) * 3;
            const float nx = qn[0] - xi, ny = qn[1] - yi, dx = q[0] - xi, dy = q[1] - yi;
            // a neighbour is present now and within reach now; an unavailable frame would land on flat pixel 0, which is zeroed
            const bool paints = here_then && (j == r || (here_now && !(p.max_dist > 0.f && nx * nx + ny * ny > d2max)));
            if (!paints) continue;
            float rx = (c * dx + s * dy) * p.ppm + p.ox, ry = (c * dy - s * dx) * p.ppm + p.oy;
            rx = fminf(fmaxf(rx, 0.f), (float)(p.W - 1));
            ry = fminf(fmaxf(ry, 0.f), (float)(p.H - 1));
            const int flat = (int)rintf(ry) * p.W + (int)rintf(rx);
            atomicOr((j == r ? ego : nbr) + (flat >> 5), 1u << (flat & 31));
        }
        __syncthreads();
        for (int g = tid; g < groups; g += kThreads) {
            const int p0 = g << 2;
            const unsigned int e = ego[p0 >> 5] >> (p0 & 31), n = nbr[p0 >> 5] >> (p0 & 31);
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = (e >> k) & 1u ? 1.f : ((n >> k) & 1u ? -1.f : 0.f);
                if (p0 + k == 0 || p0 + k == HW - 1) v[k] = 0.f;
            }
            if (p.vec) {
                *reinterpret_cast<float4*>(out + p0) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (p0 + k < HW) out[p0 + k] = v[k];
            }
        }
        return;
    }

    const int layer = plane - p.T;
    int m = p.maps ? p.scene_map[sc] : -1;
    if (m >= p.num_maps) m = -1;
    MapView f{};                                                 // the per-pixel lookup itself: map_pixel_value (cld_kernels.h)
    f.xi = xi; f.yi = yi; f.c = c; f.s = s; f.ox = p.ox; f.oy = p.oy; f.fill = p.fill;
    f.inv_ppm = 1.f / p.ppm;                                     // (metres per pixel: one division per workgroup)
    f.mw = (float)p.map_w; f.mh = (float)p.map_h; f.map_w = p.map_w;
    if (m >= 0) {
        const float* M = p.map_from_world + (size_t)m * 9;
        f.m00 = M[0]; f.m01 = M[1]; f.m02 = M[2]; f.m10 = M[3]; f.m11 = M[4]; f.m12 = M[5];
        f.src = p.maps + ((size_t)m * p.n_sem + layer) * p.map_h * p.map_w;
    }
    unsigned char* drv = (p.drivable && layer == 0) ? p.drivable + (size_t)i * HW : nullptr;
    for (int g = tid; g < groups; g += kThreads) {
        const int p0 = g << 2;
        int v = p0 / p.W, u = p0 - v * p.W;
        float val[4];
        float ay = map_agent_coord(v, f.oy, f.inv_ppm);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            val[k] = map_pixel_value(f, map_agent_coord(u, f.ox, f.inv_ppm), ay);
            if (++u == p.W) { u = 0; ++v; ay = map_agent_coord(v, f.oy, f.inv_ppm); }
        }
        if (p.vec) {
            *reinterpret_cast<float4*>(out + p0) = make_float4(val[0], val[1], val[2], val[3]);
            if (drv)
                *reinterpret_cast<unsigned int*>(drv + p0) = (val[0] != 0.f ? 1u : 0u) | (val[1] != 0.f ? 0x100u : 0u) |
                                                             (val[2] != 0.f ? 0x10000u : 0u) | (val[3] != 0.f ? 0x1000000u : 0u);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p0 + k < HW) {
                    out[p0 + k] = val[k];
                    if (drv) drv[p0 + k] = val[k] != 0.f ? 1 : 0;
                }
        }
    }
}
}  // namespace

size_t raster_lds_bytes(int H, int W) { return (size_t)2 * ((H * W + 31) >> 5) * sizeof(unsigned int); }

hipError_t launch_raster(const RasterArgs& a, hipStream_t s) {
    RasterArgs p = a;
    const int HW = p.H * p.W;
    // 16-byte stores need every plane (and every agent's drivable map) to start on a 16-byte boundary
    p.vec = HW % 4 == 0 && reinterpret_cast<uintptr_t>(p.image) % 16 == 0 &&
            (!p.drivable || reinterpret_cast<uintptr_t>(p.drivable) % 4 == 0);
    const unsigned int blocks = (unsigned int)p.B * (unsigned int)(p.T + p.n_sem);
    hipLaunchKernelGGL(raster_kernel, dim3(blocks), dim3(kThreads), raster_lds_bytes(p.H, p.W), s, p);
    return hipGetLastError();
}

}  // namespace cld
