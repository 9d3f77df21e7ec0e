// recon_kernels.h -- launch interface of the reconstruction-guidance step (recon_kernels.hip; include/cld_recon.h is the public side).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cld {

// x0_hat = rc x_t - rm1 eps, eps = (1 + w) eps_c - w eps_u when eps_u is given.  rows = B * 52 rows of 4 floats everywhere.
struct ReconHeadArgs {
    const float* eps_c;      // [rows,4] noise prediction of the conditional half (or of the only pass)
    const float* eps_u;      // [rows,4] unconditional half, or null
    const float* x_t;        // [rows,4]
    float* x0_hat;           // [rows,4]
    float cfg_w, rc, rm1;    // guidance weight, sqrt_recip_acp[t], sqrt_recipm1_acp[t]
    long rows;
};
hipError_t launch_recon_head(const ReconHeadArgs& a, hipStream_t s);

// the cotangents of the taped pass: d_eps_c = cc g0, d_eps_u = cu g0
struct ReconSeedArgs {
    const float* g0;         // [rows,4] dL/dx0_hat
    float* d_eps_c;          // [rows,4]
    float* d_eps_u;          // [rows,4] or null
    float cc, cu;            // -rm1 (1 + w), +rm1 w
    long rows;
};
hipError_t launch_recon_seed(const ReconSeedArgs& a, hipStream_t s);

// g_xt = rc g0 + dx_c (+ dx_u); delta = slr g_xt; clip to +-th (th < 0: none); x0_g = x0_hat + delta_c; mean = c1 x0_g + c2 x_t;
// x_next = mean + sigma z
struct ReconUpdateArgs {
    const float* g0;         // [rows,4]
    const float* dx_c;       // [rows,4]
    const float* dx_u;       // [rows,4] or null
    const float* x0_hat;     // [rows,4]
    const float* x_t;        // [rows,4]; may be x_out (a lane reads its row before it writes it)
    const float* z;          // [rows,4] N(0,1) draw, or null: the on-device generator keyed by (seed, salt, row)
    float* x_out;            // [rows,4] x_{t-1}: the conditional half of the working latent, or null
    float* x_out2;           // ... the unconditional half, or null
    float* x_next;           // [rows,4] caller's copy of x_{t-1}, or null
    float* grad_xt;          // [rows,4] or null
    float* x0_guided;        // [rows,4] or null
    float* mean;             // [rows,4] or null
    float rc, slr, th, c1, c2, sigma;
    unsigned long long seed, salt;
    long rows;
};
hipError_t launch_recon_update(const ReconUpdateArgs& a, hipStream_t s);

int recon_grid_cap(int cap);     // cld_debug_recon_grid_cap

}  // namespace cld
