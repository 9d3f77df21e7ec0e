// recon_kernels.hip -- the three elementwise kernels of a reconstruction-guided step (include/cld_recon.h; upstream p_sample with
// guide_clean == "video_diff", src/tbsim/models/diffuser.py:844-929, perturb_video_diffusion, src/tbsim/utils/guidance_loss.py:2284-2330,
// q_posterior, diffuser.py:911).  They sit between the launches that carry the step's cost -- the taped U-Net forward, the guidance
// machinery, the U-Net's input-gradient backward -- and are memory bound: one row of 4 floats per lane and access (16 bytes), a
// grid-stride loop over the B * 52 rows, no LDS, no atomics, a row's result a function of that row's inputs only.
//
// Rounding.  Every multiply-add below is written as the instruction it is (__fmaf_rn / __fmul_rn / __fadd_rn); nothing is left for the
// compiler to contract.  That matters for: eps (the CFG combine), x0_hat, g_xt, mean and x_next -- each a sum of two products that a
// compiler may fuse either way round, and differently in the four unrolled copies of a row (the trap DESIGN.md 4.12 records).  The
// loop and the single-step call run the same instructions, and so do all rows: bit identity between them rests on that.
#include "cld_kernels.h"
#include "recon_kernels.h"

namespace cld {

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kReconBlock = 256;
constexpr int kReconMaxBlocksDefault = 1024;     // 4 workgroups per CU of the 256: beyond ~5,000 agents a lane walks several rows
int g_recon_max_blocks = kReconMaxBlocksDefault;

inline unsigned recon_grid(long rows) {
    const long need = (rows + kReconBlock - 1) / kReconBlock;
    return (unsigned)(need < g_recon_max_blocks ? (need < 1 ? 1 : need) : g_recon_max_blocks);
}

__global__ __launch_bounds__(kReconBlock) void recon_head_kernel(const ReconHeadArgs a) {
    const long stride = (long)gridDim.x * kReconBlock;
    const float w1 = 1.0f + a.cfg_w, nw = -a.cfg_w, nrm1 = -a.rm1;
    for (long row = (long)blockIdx.x * kReconBlock + threadIdx.x; row < a.rows; row += stride) {
        v4f eps = reinterpret_cast<const v4f*>(a.eps_c)[row];
        if (a.eps_u) {
            const v4f u = reinterpret_cast<const v4f*>(a.eps_u)[row];
#pragma unroll
            for (int d = 0; d < 4; ++d) eps[d] = __fmaf_rn(nw, u[d], __fmul_rn(w1, eps[d]));      // (1 + w) eps_c - w eps_u
        }
        const v4f x = reinterpret_cast<const v4f*>(a.x_t)[row];
        v4f x0;
#pragma unroll
        for (int d = 0; d < 4; ++d) x0[d] = __fmaf_rn(nrm1, eps[d], __fmul_rn(a.rc, x[d]));       // rc x_t - rm1 eps
        reinterpret_cast<v4f*>(a.x0_hat)[row] = x0;
    }
}

__global__ __launch_bounds__(kReconBlock) void recon_seed_kernel(const ReconSeedArgs a) {
    const long stride = (long)gridDim.x * kReconBlock;
    for (long row = (long)blockIdx.x * kReconBlock + threadIdx.x; row < a.rows; row += stride) {
        const v4f g = reinterpret_cast<const v4f*>(a.g0)[row];
        v4f c;
#pragma unroll
        for (int d = 0; d < 4; ++d) c[d] = __fmul_rn(a.cc, g[d]);
        reinterpret_cast<v4f*>(a.d_eps_c)[row] = c;
        if (a.d_eps_u) {
            v4f u;
#pragma unroll
            for (int d = 0; d < 4; ++d) u[d] = __fmul_rn(a.cu, g[d]);
            reinterpret_cast<v4f*>(a.d_eps_u)[row] = u;
        }
    }
}

__global__ __launch_bounds__(kReconBlock) void recon_update_kernel(const ReconUpdateArgs a) {
    const long stride = (long)gridDim.x * kReconBlock;
    for (long row = (long)blockIdx.x * kReconBlock + threadIdx.x; row < a.rows; row += stride) {
        const v4f g0 = reinterpret_cast<const v4f*>(a.g0)[row];
        const v4f dxc = reinterpret_cast<const v4f*>(a.dx_c)[row];
        const v4f x0 = reinterpret_cast<const v4f*>(a.x0_hat)[row];
        const v4f xt = reinterpret_cast<const v4f*>(a.x_t)[row];
        v4f g;
#pragma unroll
        for (int d = 0; d < 4; ++d) g[d] = __fmaf_rn(a.rc, g0[d], dxc[d]);                        // rc g0 + dx_c
        if (a.dx_u) {
            const v4f dxu = reinterpret_cast<const v4f*>(a.dx_u)[row];
#pragma unroll
            for (int d = 0; d < 4; ++d) g[d] = __fadd_rn(g[d], dxu[d]);                           // ... + dx_u
        }
        v4f z = {0.f, 0.f, 0.f, 0.f};
        if (a.sigma != 0.f) z = a.z ? reinterpret_cast<const v4f*>(a.z)[row] : normal4(a.seed, a.salt, (unsigned)row);
        v4f x0g, mean, xn;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            float delta = __fmul_rn(a.slr, g[d]);
            if (a.th >= 0.f) delta = fminf(fmaxf(delta, -a.th), a.th);
            x0g[d] = __fadd_rn(x0[d], delta);
            mean[d] = __fmaf_rn(a.c1, x0g[d], __fmul_rn(a.c2, xt[d]));                            // c1 x0_g + c2 x_t
            xn[d] = __fmaf_rn(a.sigma, z[d], mean[d]);                                            // mean + sigma z
        }
        if (a.grad_xt) reinterpret_cast<v4f*>(a.grad_xt)[row] = g;
        if (a.x0_guided) reinterpret_cast<v4f*>(a.x0_guided)[row] = x0g;
        if (a.mean) reinterpret_cast<v4f*>(a.mean)[row] = mean;
        if (a.x_next) reinterpret_cast<v4f*>(a.x_next)[row] = xn;
        if (a.x_out) reinterpret_cast<v4f*>(a.x_out)[row] = xn;
        if (a.x_out2) reinterpret_cast<v4f*>(a.x_out2)[row] = xn;
    }
}

}  // namespace

int recon_grid_cap(int cap) {
    g_recon_max_blocks = cap < 1 ? kReconMaxBlocksDefault : cap;
    return g_recon_max_blocks;
}

hipError_t launch_recon_head(const ReconHeadArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(recon_head_kernel, dim3(recon_grid(a.rows)), dim3(kReconBlock), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_recon_seed(const ReconSeedArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(recon_seed_kernel, dim3(recon_grid(a.rows)), dim3(kReconBlock), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_recon_update(const ReconUpdateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(recon_update_kernel, dim3(recon_grid(a.rows)), dim3(kReconBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace cld
