// solver_kernels.hip -- the elementwise step of the few-step samplers (include/cld_solver.h): DDIM(eta) and DPM-Solver++(2M) on a
// subset of the training timesteps.  It sits behind the U-Net evaluation and the head's noise prediction and is memory bound: one row
// of 4 floats per lane and access (16 bytes), a grid-stride loop over the B * 52 rows, no LDS, no atomics, a row's result a function
// of that row's inputs only.
//
// Rounding.  Every multiply-add below is written as the instruction it is (__fmaf_rn / __fmul_rn / __fadd_rn), in the order
// solver_kernels.h writes down; nothing is left for the compiler to contract (the trap DESIGN.md 4.12 records).  A row alone and in a
// batch, one pass of the grid and several, the loop and the single-step call therefore run the same instructions.
#include "cld_kernels.h"
#include "solver_kernels.h"

namespace cld {

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kSolverBlock = 256;
constexpr int kSolverMaxBlocksDefault = 1024;    // 4 workgroups per CU of the 256: beyond ~5,000 agents a lane walks several rows
int g_solver_max_blocks = kSolverMaxBlocksDefault;

inline unsigned solver_grid(long rows) {
    const long need = (rows + kSolverBlock - 1) / kSolverBlock;
    return (unsigned)(need < g_solver_max_blocks ? (need < 1 ? 1 : need) : g_solver_max_blocks);
}

__global__ __launch_bounds__(kSolverBlock) void solver_step_kernel(const SolverStepArgs a) {
    const long stride = (long)gridDim.x * kSolverBlock;
    for (long row = (long)blockIdx.x * kSolverBlock + threadIdx.x; row < a.rows; row += stride) {
        v4f eps = reinterpret_cast<const v4f*>(a.eps_c)[row];
        if (a.eps_u) {
            const v4f u = reinterpret_cast<const v4f*>(a.eps_u)[row];
#pragma unroll
            for (int d = 0; d < 4; ++d) eps[d] = __fmaf_rn(a.nw, u[d], __fmul_rn(a.w1, eps[d]));       // (1 + w) eps_c - w eps_u
        }
        const v4f x = reinterpret_cast<const v4f*>(a.x)[row];
        v4f x0, det;
#pragma unroll
        for (int d = 0; d < 4; ++d) x0[d] = __fmaf_rn(a.nrm1, eps[d], __fmul_rn(a.rc, x[d]));          // rc x - rm1 eps
        if (a.form == SOLVER_FORM_DDIM) {
#pragma unroll
            for (int d = 0; d < 4; ++d) det[d] = __fmaf_rn(a.b, eps[d], __fmul_rn(a.a, x[d]));         // A x + B eps
        } else if (a.form == SOLVER_FORM_2M) {
            v4f dd = x0;
            if (a.x0_prev) {
                const v4f p = reinterpret_cast<const v4f*>(a.x0_prev)[row];
#pragma unroll
                for (int d = 0; d < 4; ++d) dd[d] = __fmaf_rn(a.nc1, p[d], __fmul_rn(a.c0, x0[d]));    // (1 + 1/2r) x0 - (1/2r) x0_prev
            }
#pragma unroll
            for (int d = 0; d < 4; ++d) det[d] = __fmaf_rn(a.b, dd[d], __fmul_rn(a.a, x[d]));          // A x + C D
        } else {
            det = x0;
        }
        v4f xn = det;
        if (a.sigma != 0.f) {
            const v4f z = a.z ? reinterpret_cast<const v4f*>(a.z)[row] : normal4(a.seed, a.salt, (unsigned)row);
#pragma unroll
            for (int d = 0; d < 4; ++d) xn[d] = __fmaf_rn(a.sigma, z[d], det[d]);                      // det + sigma z
        }
        if (a.hist) reinterpret_cast<v4f*>(a.hist)[row] = x0;
        if (a.x0_out) reinterpret_cast<v4f*>(a.x0_out)[row] = x0;
        if (a.mu_out) reinterpret_cast<v4f*>(a.mu_out)[row] = det;
        if (a.det_out) reinterpret_cast<v4f*>(a.det_out)[row] = det;
        if (a.x_out) reinterpret_cast<v4f*>(a.x_out)[row] = xn;
        if (a.x_out2) reinterpret_cast<v4f*>(a.x_out2)[row] = xn;
    }
}

}  // namespace

int solver_grid_cap(int cap) {
    g_solver_max_blocks = cap < 1 ? kSolverMaxBlocksDefault : cap;
    return g_solver_max_blocks;
}

hipError_t launch_solver_step(const SolverStepArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(solver_step_kernel, dim3(solver_grid(a.rows)), dim3(kSolverBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace cld
