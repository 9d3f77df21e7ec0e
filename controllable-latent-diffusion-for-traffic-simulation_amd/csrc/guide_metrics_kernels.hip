// guide_metrics_kernels.hip -- the guidance satisfaction metrics on the device: what upstream's GuidanceMetric classes
// (src/tbsim/utils/guidance_metrics.py) compute on the host, in Python loops over agents, from poses copied off the device every step
// (include/cld.h `cld_guide_metrics_step` for the definitions and the entry table).
//
// Launch shape (the one the feature request suggested, kept): guide_metrics_step_kernel, one launch per environment step over every entry
// of every scene.  Waves 0 .. num_members - 1 are one wave per (entry, member): the flag kinds stride over the member's scene 64 partners
// at a time and resolve them with ballots, exactly as scene_metrics_step_kernel does (the fp32 flag arithmetic is shared: metrics_device.h),
// the map kinds put their 52 disk samples / 4 box corners on lanes, social_group strides over the entry's other members with an fp64 wave
// minimum, the waypoint kinds are one lane's work.  Waves num_members .. num_members + num_entries - 1 are one wave per entry and serve the
// three per-step-mean kinds (target_speed, speed_limit, acc_limit): lanes stride over the members, a fixed xor-shuffle tree reduces them.
// Lane 0 of a wave updates its own row in place: no atomics, the same bytes on every run.  A wave whose kind belongs to the other group
// leaves at once.  guide_metrics_read_kernel, one workgroup per entry, finalises the member rows and takes their mean in the order numpy's
// add.reduce takes it (the pairwise sum: halves down to blocks of at most 128, eight accumulators per block), so a mean of per-member step
// fractions is upstream's np.mean bit for bit.  Distances and sums are fp64 from the fp32 inputs with contraction off.
#include "cld_kernels.h"
#include "metrics_device.h"

namespace cld {

namespace {
constexpr int kWaves = 4;                 // waves per workgroup of the step kernel
constexpr int kReadThreads = 256;
constexpr int kReadLds = 4096;            // member values one workgroup of the read kernel stages in LDS

enum : int { K_TARGET_SPEED = 0, K_SPEED_LIMIT, K_ACC_LIMIT, K_AGENT_COLLISION, K_AGENT_COLLISION_DISK, K_SOCIAL_DIST, K_MAP_COLLISION,
             K_MAP_COLLISION_DISK, K_TARGET_POS, K_GLOBAL_TARGET_POS, K_TARGET_POS_AT_TIME, K_GLOBAL_TARGET_POS_AT_TIME, K_SOCIAL_GROUP,
             K_COUNT };

struct EntryRow {                         // all-zero = empty
    double sum;                           // the per-step means so far (per-step-mean kinds)
    unsigned int steps, reserved[5];
};
struct MemberRow {                        // all-zero = empty
    unsigned int steps, flag_sum, flag_max, have;
    double val;                           // the minimum distance / the distance at the target time (have)
    double sum;                           // the member's terms so far (per-step-mean kinds, social_group)
    double frame[6];                      // agent_from_world of the first scored step, rows 0 and 1 (local waypoint kinds)
};
static_assert(sizeof(EntryRow) == GUIDE_METRICS_ENTRY_BYTES && sizeof(MemberRow) == GUIDE_METRICS_MEMBER_BYTES, "cld_guide_metrics_state_bytes");

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ double dnan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double dinf() { return __longlong_as_double(0x7ff0000000000000ll); }

// the clamped ranges of entry e in the three flat arrays
struct EntryView {
    int kind, scene, m0, m1, x0, x1, q0, q1;
};
__device__ __forceinline__ EntryView entry_view(const GuideMetricsArgs& p, int e) {
    EntryView v;
    v.kind = p.entry_kind[e];
    v.scene = clampi(p.entry_scene[e], 0, p.num_scenes - 1);
    v.m0 = clampi(p.member_start[e], 0, p.num_members);
    v.m1 = clampi(p.member_start[e + 1], v.m0, p.num_members);
    v.x0 = p.excluded ? clampi(p.excl_start[e], 0, p.num_excluded) : 0;
    v.x1 = p.excluded ? clampi(p.excl_start[e + 1], v.x0, p.num_excluded) : 0;
    v.q0 = p.params ? clampi(p.param_start[e], 0, p.num_params) : 0;
    v.q1 = p.params ? clampi(p.param_start[e + 1], v.q0, p.num_params) : 0;
    return v;
}
__device__ __forceinline__ double param(const GuideMetricsArgs& p, const EntryView& v, long long k) {      // NaN past the entry's range
    return (k >= 0 && k < (long long)(v.q1 - v.q0)) ? p.params[v.q0 + k] : dnan();
}
__device__ __forceinline__ bool is_excluded(const GuideMetricsArgs& p, const EntryView& v, int row) {       // the list is sorted ascending
    int lo = v.x0, hi = v.x1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int x = p.excluded[mid];
        if (x == row) return true;
        if (x < row) lo = mid + 1; else hi = mid;
    }
    return false;
}
__device__ __forceinline__ double dist64(double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
    const double dx = ax - bx, dy = ay - by;
    return sqrt(dx * dx + dy * dy);
}

__device__ void entry_wave(const GuideMetricsArgs& p, int e, int lane) {
#pragma clang fp contract(off)
    const EntryView v = entry_view(p, e);
    if (v.kind < K_TARGET_SPEED || v.kind > K_ACC_LIMIT) return;
    MemberRow* mrows = reinterpret_cast<MemberRow*>(static_cast<char*>(p.state) + (size_t)p.num_entries * sizeof(EntryRow));
    const double L = param(p, v, 0);                             // the limit, or the length of a target_speed row
    const long long len = (v.kind == K_TARGET_SPEED && L >= 0.0) ? (long long)fmin(L, 1073741824.0) : 0;
    double sum = 0.0;
    unsigned int cnt = 0u;
    for (int m = v.m0 + lane; m < v.m1; m += 64) {
        const int i = clampi(p.members[m], 0, p.B_all - 1);
        MemberRow& mr = mrows[m];
        double term;
        if (v.kind == K_TARGET_SPEED) {
            term = (long long)p.global_t < len ? fabs((double)p.speed[i] - param(p, v, 1 + (long long)(m - v.m0) * len + p.global_t)) : 0.0;
            if (term == term) { sum += term; cnt += 1u; mr.sum += term; mr.steps += 1u; }      // nanmean
        } else {
            const double x = v.kind == K_SPEED_LIMIT ? (double)p.speed[i] : fabs((double)p.acc[i]);
            const double d = x - L;
            term = d != d ? d : (d < 0.0 ? 0.0 : d);             // np.clip keeps a NaN
            sum += term; cnt += 1u; mr.sum += term; mr.steps += 1u;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {                     // a fixed tree
        sum += __shfl_xor(sum, off);
        cnt += __shfl_xor(cnt, off);
    }
    if (lane != 0) return;
    EntryRow& er = reinterpret_cast<EntryRow*>(p.state)[e];
    er.sum += cnt ? sum / (double)cnt : dnan();
    er.steps += 1u;
}

__device__ void member_wave(const GuideMetricsArgs& p, int m, int lane) {
#pragma clang fp contract(off)
    int e = 0, hi = p.num_entries;                               // member_start[e] <= m < member_start[e + 1]
    while (hi - e > 1) {
        const int mid = (e + hi) >> 1;
        if (p.member_start[mid] <= m) e = mid; else hi = mid;
    }
    const EntryView v = entry_view(p, e);
    if (m < v.m0 || m >= v.m1 || v.kind <= K_ACC_LIMIT || v.kind >= K_COUNT) return;
    const int i = clampi(p.members[m], 0, p.B_all - 1), sc = v.scene;
    const float xi = p.world[(size_t)i * 3], yi = p.world[(size_t)i * 3 + 1], hi_ = p.world[(size_t)i * 3 + 2];
    const bool valid = !(isnan(xi) || isnan(yi));
    MemberRow& mr = reinterpret_cast<MemberRow*>(static_cast<char*>(p.state) + (size_t)p.num_entries * sizeof(EntryRow))[m];

    if (v.kind <= K_SOCIAL_DIST) {
        // ---- the collision kinds: the member's scene, 64 partners at a time
        const bool box = v.kind == K_AGENT_COLLISION;
        const float a0 = 0.5f * p.extent[(size_t)i * 3], a1 = 0.5f * p.extent[(size_t)i * 3 + 1];
        const float ri = 0.5f * fminf(p.extent[(size_t)i * 3], p.extent[(size_t)i * 3 + 1]);
        const float c = cosf(hi_), s = sinf(hi_);
        const bool i_excl = is_excluded(p, v, i);
        const float buffer = v.kind == K_SOCIAL_DIST ? (float)param(p, v, 0) : 0.f;
        int partner = -1;
        unsigned int disk_hit = 0u;
        if (valid && (box || !i_excl)) {
            const int j0 = clampi(p.scene_start[sc], 0, p.B_all), j1 = clampi(p.scene_start[sc + 1], j0, p.B_all);
            for (int base = j0; base < j1; base += 64) {
                const int j = base + lane;
                bool dhit = false, bhit = false;
                if (j < j1 && j != i) {
                    const float xj = p.world[(size_t)j * 3], yj = p.world[(size_t)j * 3 + 1], hj = p.world[(size_t)j * 3 + 2];
                    const float e0 = p.extent[(size_t)j * 3], e1 = p.extent[(size_t)j * 3 + 1];
                    if (!(isnan(xj) || isnan(yj))) {
                        float dist, rsum;
                        mdev::pair_hits(xi, yi, c, s, a0, a1, ri, xj, yj, hj, e0, e1, dist, rsum, bhit);
                        if (!box && !is_excluded(p, v, j)) dhit = v.kind == K_SOCIAL_DIST ? dist < rsum + buffer : dist < rsum;
                    }
                }
                if (__ballot(dhit)) disk_hit = 1u;
                const unsigned long long bm = __ballot(bhit);
                if (partner < 0 && bm) partner = base + __ffsll((long long)bm) - 1;
            }
        }
        unsigned int flag = disk_hit;
        if (box) flag = (partner >= 0 && !(i_excl && is_excluded(p, v, partner))) ? 1u : 0u;
        if (lane != 0) return;
        mr.steps += 1u;
        mr.flag_sum += flag;
        mr.flag_max |= flag;
        return;
    }

    if (v.kind <= K_MAP_COLLISION_DISK) {
        // ---- the map kinds: the 4 box corners (get_box_world_coords' order) or the 52 disk samples on lanes
        unsigned int flag = 0u;
        if (valid) {
            const float e0 = p.extent[(size_t)i * 3], e1 = p.extent[(size_t)i * 3 + 1];
            const float c = cosf(hi_), s = sinf(hi_);
            const int lanes = v.kind == K_MAP_COLLISION ? 4 : 52;
            float fu = p.ox, fv = p.oy;
            if (v.kind == K_MAP_COLLISION) {
                const float h0 = 0.5f * (p.ppm * e0), h1 = 0.5f * (p.ppm * e1);
                const int k = lane & 3;                          // (-,-) (-,+) (+,+) (+,-)
                fu = fminf(fmaxf(p.ox + (k >= 2 ? h0 : -h0), 0.f), (float)(p.W - 1));
                fv = fminf(fmaxf(p.oy + ((k == 1 || k == 2) ? h1 : -h1), 0.f), (float)(p.H - 1));
            } else if (lane < 52) {
                mdev::disk_sample(p, 0.5f * fminf(e0, e1), lane, fu, fv);
            }
            const float x = mdev::raster_value(p, sc, xi, yi, c, s, fu, fv);
            flag = __ballot(lane < lanes && x == 0.f) ? 1u : 0u;
        }
        if (lane != 0) return;
        mr.steps += 1u;
        mr.flag_sum += flag;
        mr.flag_max |= flag;
        return;
    }

    if (v.kind == K_SOCIAL_GROUP) {
        // ---- the minimum over the entry's other members of the pairwise distance; a NaN wins, as np.amin lets it
        double mn = dinf();
        bool anynan = false;
        for (int mm = v.m0 + lane; mm < v.m1; mm += 64) {
            if (mm == m) continue;
            const int j = clampi(p.members[mm], 0, p.B_all - 1);
            const double d = dist64((double)p.world[(size_t)j * 3], (double)p.world[(size_t)j * 3 + 1], (double)xi, (double)yi);
            if (d != d) anynan = true; else mn = fmin(mn, d);
        }
        const bool wave_nan = __ballot(anynan) != 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mn = fmin(mn, __shfl_xor(mn, off));
        if (lane != 0) return;
        mr.sum += wave_nan ? dnan() : fabs(mn - param(p, v, 0));
        mr.steps += 1u;
        return;
    }

    // ---- the waypoint kinds: one lane's work
    if (lane != 0) return;
    const long long n = v.m1 - v.m0, k = m - v.m0;
    const bool local = v.kind == K_TARGET_POS || v.kind == K_TARGET_POS_AT_TIME;
    double px = (double)xi, py = (double)yi;
    if (local) {
        if (mr.steps == 0u) {                                    // agent_from_world of the first scored step
            const double c = cos((double)hi_), s = sin((double)hi_);
            mr.frame[0] = c; mr.frame[1] = s; mr.frame[2] = -(c * px) - (s * py);
            mr.frame[3] = -s; mr.frame[4] = c; mr.frame[5] = (s * px) - (c * py);
        }
        const double lx = (px * mr.frame[0] + py * mr.frame[1]) + mr.frame[2];
        const double ly = (px * mr.frame[3] + py * mr.frame[4]) + mr.frame[5];
        px = lx; py = ly;
    }
    const double d = dist64(px, py, param(p, v, 2 * k), param(p, v, 2 * k + 1));
    if (v.kind <= K_GLOBAL_TARGET_POS) {
        const double cur = mr.have ? mr.val : dinf();
        if (d < cur) { mr.val = d; mr.have = 1u; }               // a NaN never wins
    } else if ((double)p.global_t == param(p, v, 2 * n + k) + 1.0) {
        mr.val = d; mr.have = 1u;
    }
    mr.steps += 1u;
}

__global__ __launch_bounds__(kWaves * 64) void guide_metrics_step_kernel(const GuideMetricsArgs p) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (w >= (long long)p.num_members + p.num_entries) return;   // (a whole wave; the kernel has no barrier)
    if (w < p.num_members) member_wave(p, (int)w, lane);
    else entry_wave(p, (int)(w - p.num_members), lane);
}

// the value of one member (per_member of cld_guide_metrics_read)
__device__ __forceinline__ double member_value(int kind, const MemberRow& mr) {
#pragma clang fp contract(off)
    switch (kind) {
    case K_TARGET_SPEED: case K_SPEED_LIMIT: case K_ACC_LIMIT: case K_SOCIAL_GROUP:
        return mr.steps ? mr.sum / (double)mr.steps : dnan();
    case K_AGENT_COLLISION: case K_AGENT_COLLISION_DISK: case K_SOCIAL_DIST:
        return mr.steps ? (double)mr.flag_max : dnan();
    case K_MAP_COLLISION: case K_MAP_COLLISION_DISK:
        return mr.steps ? (double)mr.flag_sum / (double)mr.steps : dnan();
    case K_TARGET_POS: case K_GLOBAL_TARGET_POS:
        return mr.have ? mr.val : dinf();
    case K_TARGET_POS_AT_TIME: case K_GLOBAL_TARGET_POS_AT_TIME:
        return mr.have ? mr.val : dnan();
    default:
        return dnan();
    }
}

// numpy's pairwise sum of a[0 .. n) (n <= 128 at the leaves): eight accumulators over whole groups of eight, their fixed tree, the rest one by one
template <class G>
__device__ double pairwise_block(const G& get, long long a, long long n) {
#pragma clang fp contract(off)
    if (n < 8) {
        double res = 0.0;
        for (long long i = 0; i < n; ++i) res += get(a + i);
        return res;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = get(a + j);
    long long i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += get(a + i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += get(a + i);
    return res;
}
template <class G>
__device__ double pairwise_sum(const G& get, long long a0, long long n0) {
#pragma clang fp contract(off)
    long long sa[32], sn[32];
    double left[32];
    int stage[32];
    int sp = 0;
    sa[0] = a0; sn[0] = n0; stage[0] = 0;
    double ret = 0.0;
    while (sp >= 0) {
        long long half = sn[sp] / 2;
        half -= half % 8;
        if (stage[sp] == 0) {
            if (sn[sp] <= 128) { ret = pairwise_block(get, sa[sp], sn[sp]); --sp; continue; }
            stage[sp] = 1;
            sa[sp + 1] = sa[sp]; sn[sp + 1] = half; stage[sp + 1] = 0; ++sp;
        } else if (stage[sp] == 1) {
            left[sp] = ret;
            stage[sp] = 2;
            sa[sp + 1] = sa[sp] + half; sn[sp + 1] = sn[sp] - half; stage[sp + 1] = 0; ++sp;
        } else {
            ret = left[sp] + ret;
            --sp;
        }
    }
    return ret;
}
// np.mean of a[0 .. n), n >= 1: add.reduce starts from the identity 0 and adds the pairwise sum of the whole array
template <class G>
__device__ double numpy_mean(const G& get, long long n) {
#pragma clang fp contract(off)
    const double total = 0.0 + pairwise_sum(get, 0, n);
    return total / (double)n;
}

__global__ __launch_bounds__(kReadThreads) void guide_metrics_read_kernel(const GuideMetricsArgs p) {
    __shared__ double vals[kReadLds];
    const int e = blockIdx.x, tid = threadIdx.x;
    const EntryView v = entry_view(p, e);
    const int kind = v.kind, n = v.m1 - v.m0;
    const MemberRow* mrows = reinterpret_cast<const MemberRow*>(static_cast<const char*>(p.state) + (size_t)p.num_entries * sizeof(EntryRow)) + v.m0;
    const bool stage = n <= kReadLds;
    for (int k = tid; k < n; k += kReadThreads) {
        const double x = member_value(kind, mrows[k]);
        if (p.per_member) p.per_member[v.m0 + k] = x;
        if (stage) vals[k] = x;
    }
    if (!p.per_entry) return;
    __syncthreads();
    if (tid != 0) return;
    double out = dnan();
    if (kind >= K_TARGET_SPEED && kind <= K_ACC_LIMIT) {
        const EntryRow& er = reinterpret_cast<const EntryRow*>(p.state)[e];
        if (er.steps) out = er.sum / (double)er.steps;
    } else if (kind > K_ACC_LIMIT && kind < K_COUNT && n > 0) {
        if (stage) out = numpy_mean([&](long long k) { return vals[k]; }, n);
        else out = numpy_mean([&](long long k) { return member_value(kind, mrows[k]); }, n);
    }
    p.per_entry[e] = out;
}
}  // namespace

hipError_t launch_guide_metrics_step(const GuideMetricsArgs& a, hipStream_t s) {
    const long long waves = (long long)a.num_members + a.num_entries;
    hipLaunchKernelGGL(guide_metrics_step_kernel, dim3((unsigned int)((waves + kWaves - 1) / kWaves)), dim3(kWaves * 64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_guide_metrics_read(const GuideMetricsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(guide_metrics_read_kernel, dim3((unsigned int)a.num_entries), dim3(kReadThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace cld
