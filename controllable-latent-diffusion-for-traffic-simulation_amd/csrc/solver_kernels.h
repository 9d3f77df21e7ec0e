// solver_kernels.h -- launch interface of the few-step samplers' step (solver_kernels.hip; include/cld_solver.h is the public side).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cld {

enum { SOLVER_FORM_DDIM = 0, SOLVER_FORM_2M = 1, SOLVER_FORM_FINAL = 2 };

// One step of DDIM(eta) / DPM-Solver++(2M) on rows = B * 52 rows of 4 floats.  The operations, in this order, each one instruction:
//   eps   = eps_u ? fma(-w, eps_u, mul(1 + w, eps_c)) : eps_c                      (1 + w formed once on the host)
//   x0    = fma(-rm1, eps, mul(rc, x))
//   det   = FORM_DDIM:  fma(b, eps, mul(a, x))
//           FORM_2M:    fma(b, D, mul(a, x)),  D = x0_prev ? fma(-c1, x0_prev, mul(c0, x0)) : x0
//           FORM_FINAL: x0
//   x'    = sigma != 0 ? fma(sigma, z, det) : det
struct SolverStepArgs {
    const float* x;          // [rows,4] the working latent; may be x_out (a lane reads its row before it writes it)
    const float* eps_c;      // [rows,4] noise prediction of the conditional half (or of the only pass)
    const float* eps_u;      // [rows,4] unconditional half, or null
    const float* x0_prev;    // [rows,4] the clean prediction of the preceding step (2M, second-order steps), or null
    const float* z;          // [rows,4] N(0,1) draw, or null: the on-device generator keyed by (seed, salt, row); read when sigma != 0
    float* hist;             // [rows,4] receives x0 (the history the next step reads; may be x0_prev), or null
    float* x_out;            // [rows,4] x': the conditional half of the working latent, or null (a guidance step follows)
    float* x_out2;           // ... the unconditional half, or null
    float* det_out;          // [rows,4] the deterministic part (the iterate of a guidance step), or null
    float* x0_out;           // [rows,4] caller's copy of x0, or null
    float* mu_out;           // [rows,4] caller's copy of the deterministic part, or null
    float w1, nw;            // 1 + w, -w
    float rc, nrm1;          // sqrt(1 / acp_s), -sqrt(1 / acp_s - 1)
    float a, b, c0, nc1;     // the step's coefficients (c0, -c1: the history blend of a second-order step)
    float sigma;
    int form;
    unsigned long long seed, salt;
    long rows;
};
hipError_t launch_solver_step(const SolverStepArgs& a, hipStream_t s);

int solver_grid_cap(int cap);    // cld_debug_solver_grid_cap

}  // namespace cld
