// occupancy_kernels.hip -- the occupancy coverage and diversity metrics on the device: what upstream's OccupancyGrid / OccupancyCoverage /
// OccupancyDiversity (src/tbsim/envs/env_metrics.py:977-1218) keep in Python dicts on the host, from the world poses cld_world_step leaves
// in HBM (include/cld.h `cld_occupancy_splat` for the definitions).
//
// occupancy_splat_kernel, one launch per environment step: one wave per agent.  The wave finds its scene, rounds its pose to the centre cell
// in fp64 and strides over the (2 N + 1)^2 window cells 64 at a time (the 9 x 9 window of sigma = 4 takes two trips); a lane's cell is
// (c / W, c % W), so neighbouring lanes add to neighbouring 8-byte words of one grid row.  Each lane adds rint(k 2^40) with one 64-bit integer
// atomic: integer adds commute, so the plane holds the same bits on every run and under every order of agents and steps.  Cells outside the
// scene's window are counted per wave (a ballot) and one lane adds the count to dropped[scene].
// occupancy_mark_kernel replays an episode's poses once its failures are known: one wave per (step, agent), agents with ok == 0 leave at
// once, the others store 1 to every window cell inside the scene's window (idempotent byte stores, no atomics).
// occupancy_read_kernel, one workgroup per scene: every cell's lane flag from the map at the cell's world point (map_pixel_value, the function
// the raster and the metrics kernels use, for an agent standing on the point with heading 0), the fixed-point value as fp64, and the three
// counts and the on-road mass as integer sums over a fixed LDS tree.  Integers throughout: nothing here depends on an order.
#include "cld_kernels.h"

namespace cld {

namespace {
constexpr int kWaves = 4;                 // agents per workgroup of the splat and mark kernels
constexpr int kReadThreads = 256;
constexpr double kQ40 = 1099511627776.0;  // 2^40

struct OccWave {                          // what one wave needs of its scene: the window and where its cells start
    int sc, ix0, iy0, nx, ny;
    long long base;
};

__device__ inline OccWave occ_scene(const OccArgs& p, int agent) {
    OccWave w;
    int sc = 0, hi = p.num_scenes;                               // scene_start[sc] <= agent < scene_start[sc + 1]
    while (hi - sc > 1) {
        const int mid = (sc + hi) >> 1;
        if (p.scene_start[mid] <= agent) sc = mid; else hi = mid;
    }
    w.sc = sc;
    w.ix0 = p.window[sc * 4]; w.iy0 = p.window[sc * 4 + 1];
    w.nx = max(p.window[sc * 4 + 2], 0); w.ny = max(p.window[sc * 4 + 3], 0);
    w.base = p.cell_start[sc];
    return w;
}

// the centre cell of a pose: np.round((x - o) / s) in fp64, half to even.  false: the cell index does not fit (every window cell is dropped)
__device__ inline bool occ_centre(const OccArgs& p, float x, float y, long long* cx, long long* cy) {
    const double fx = rint(((double)x - p.o0) / p.s0), fy = rint(((double)y - p.o1) / p.s1);
    if (!(fabs(fx) < 1073741824.0) || !(fabs(fy) < 1073741824.0)) return false;
    *cx = (long long)fx; *cy = (long long)fy;
    return true;
}

// the flat index of cell (gx, gy) in the planes, or -1: outside the scene's window (or outside the planes: a malformed cell_start)
__device__ inline long long occ_flat(const OccArgs& p, const OccWave& w, long long gx, long long gy) {
    const long long ix = gx - w.ix0, iy = gy - w.iy0;
    if (ix < 0 || ix >= w.nx || iy < 0 || iy >= w.ny) return -1;
    const long long f = w.base + ix * w.ny + iy;
    return f >= 0 && f < p.cells ? f : -1;
}

__global__ __launch_bounds__(kWaves * 64) void occupancy_splat_kernel(const OccArgs p) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= p.B_all) return;                                    // (a whole wave; the kernel has no barrier)
    const float x = p.world[(size_t)i * 3], y = p.world[(size_t)i * 3 + 1];
    if (isnan(x) || isnan(y)) return;                            // an absent agent contributes nothing
    const OccWave w = occ_scene(p, i);
    const int W = 2 * p.N + 1, area = W * W;
    long long cx = 0, cy = 0;
    const bool fits = occ_centre(p, x, y, &cx, &cy);
    unsigned int n_drop = 0u;
    for (int c0 = 0; c0 < area; c0 += 64) {                      // a window may hold more than 64 cells
        const int c = c0 + lane;
        bool out = false;
        if (c < area) {
            const long long gx = cx + (c / W - p.N), gy = cy + (c % W - p.N);
            const long long f = fits ? occ_flat(p, w, gx, gy) : -1;
            if (f >= 0) {
                const double dx = (double)x - (p.s0 * (double)gx + p.o0), dy = (double)y - (p.s1 * (double)gy + p.o1);
                const double k = exp(-(dx * dx + dy * dy) / 2.0 / p.sigma);
                atomicAdd(p.grid + f, (unsigned long long)rint(k * kQ40));
            } else {
                out = true;
            }
        }
        n_drop += (unsigned int)__popcll(__ballot(out));
    }
    if (lane == 0 && n_drop) atomicAdd(p.dropped + w.sc, (unsigned long long)n_drop);
}

__global__ __launch_bounds__(kWaves * 64) void occupancy_mark_kernel(const OccArgs p) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);      // row of world [n_steps, B_all, 3]
    if (r >= (long long)p.n_steps * p.B_all) return;
    const int i = (int)(r % p.B_all);
    if (!p.ok[i]) return;
    const float x = p.world[(size_t)r * 3], y = p.world[(size_t)r * 3 + 1];
    if (isnan(x) || isnan(y)) return;
    const OccWave w = occ_scene(p, i);
    long long cx = 0, cy = 0;
    if (!occ_centre(p, x, y, &cx, &cy)) return;
    const int W = 2 * p.N + 1, area = W * W;
    for (int c = lane; c < area; c += 64) {
        const long long f = occ_flat(p, w, cx + (c / W - p.N), cy + (c % W - p.N));
        if (f >= 0) p.success[f] = 1;
    }
}

__global__ __launch_bounds__(kReadThreads) void occupancy_read_kernel(const OccArgs p) {
    __shared__ unsigned long long part[4][kReadThreads];
    const int sc = blockIdx.x, tid = threadIdx.x;
    const int ix0 = p.window[sc * 4], iy0 = p.window[sc * 4 + 1];
    const long long nx = max(p.window[sc * 4 + 2], 0), ny = max(p.window[sc * 4 + 3], 0);
    const long long base = p.cell_start[sc];
    long long n = nx * ny;
    if (base < 0 || base > p.cells) n = 0;                       // (a malformed cell_start reads and writes nothing)
    else if (n > p.cells - base) n = p.cells - base;
    int m = p.maps ? p.scene_map[sc] : -1;
    if (m >= p.num_maps) m = -1;
    MapView f{};
    f.c = 1.f; f.s = 0.f; f.inv_ppm = 1.f; f.ox = 0.f; f.oy = 0.f;
    f.src = nullptr; f.fill = p.fill; f.map_w = p.map_w; f.mw = (float)p.map_w; f.mh = (float)p.map_h;
    if (m >= 0) {
        const float* M = p.map_from_world + (size_t)m * 9;
        f.m00 = M[0]; f.m01 = M[1]; f.m02 = M[2]; f.m10 = M[3]; f.m11 = M[4]; f.m12 = M[5];
        f.src = p.maps + ((size_t)m * p.n_sem + p.layer) * p.map_h * p.map_w;
    }
    unsigned long long cnt[3] = {0ull, 0ull, 0ull}, mass = 0ull;
    for (long long c = tid; c < n; c += kReadThreads) {
        const long long ix = c / ny, iy = c - ix * ny;
        f.xi = (float)(p.s0 * (double)(ix0 + ix) + p.o0);        // the cell's world point: an agent standing on it, heading 0, pixel (ox, oy)
        f.yi = (float)(p.s1 * (double)(iy0 + iy) + p.o1);
        const bool lane = map_pixel_value(f, 0.f, 0.f) != 0.f;
        const unsigned long long v = p.grid_in[base + c];
        if (p.lane) p.lane[base + c] = lane ? 1 : 0;
        if (p.values) p.values[base + c] = (double)v / kQ40;     // exact below 2^53; one rounding above
        const bool over = v > p.thr_q;
        cnt[0] += over ? 1ull : 0ull;
        cnt[1] += over && lane ? 1ull : 0ull;
        cnt[2] += over && lane && p.success_in && p.success_in[base + c] ? 1ull : 0ull;
        mass += lane ? v : 0ull;
    }
    if (!p.counts && !p.mass) return;
    part[0][tid] = cnt[0]; part[1][tid] = cnt[1]; part[2][tid] = cnt[2]; part[3][tid] = mass;
    __syncthreads();
    for (int w = kReadThreads >> 1; w > 0; w >>= 1) {
        if (tid < w)
#pragma unroll
            for (int k = 0; k < 4; ++k) part[k][tid] += part[k][tid + w];
        __syncthreads();
    }
    if (tid != 0) return;
    if (p.counts)
        for (int k = 0; k < 3; ++k) p.counts[(size_t)sc * 3 + k] = (long long)part[k][0];
    if (p.mass) p.mass[sc] = part[3][0];
}
}  // namespace

hipError_t launch_occupancy_splat(const OccArgs& a, hipStream_t s) {
    const unsigned int blocks = ((unsigned int)a.B_all + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(occupancy_splat_kernel, dim3(blocks), dim3(kWaves * 64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_occupancy_mark(const OccArgs& a, hipStream_t s) {
    const long long rows = (long long)a.n_steps * a.B_all;
    hipLaunchKernelGGL(occupancy_mark_kernel, dim3((unsigned int)((rows + kWaves - 1) / kWaves)), dim3(kWaves * 64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_occupancy_read(const OccArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(occupancy_read_kernel, dim3((unsigned int)a.num_scenes), dim3(kReadThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace cld
