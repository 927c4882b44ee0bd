// pg_specest.h -- spectral estimate of the Krylov matrix Â by Arnoldi (pg_specest.hip): what admits the polynomial right
// preconditioner where Gershgorin refuses it (pg_krylov_opts.precond = PG_PRECOND_POLY_EST).
#pragma once
#include "pg_krylov.h"
#include "pg_spmv.h"

namespace pg {

constexpr int SPECEST_STEPS = 30;             // Arnoldi steps
constexpr double SPECEST_BREAKDOWN = 1e-14;   // h(j+1, j) at or below it: the Krylov space is invariant, the recursion ends
constexpr double SPECEST_BOUND = 0.95;        // decide_poly's bound on the disc radius
constexpr double SPECEST_MARGIN = PG_SPECEST_MARGIN;

// Runs the estimate on A unless A.est.tried; fills A.est (verdict included).  One rank only (checked).  Synchronises the
// stream: it is a set-up step, once per assembled matrix.
void specest_run(CsrMatrix& A, const Numbering& nb, const Slab& slab);

// the conditions every rank count / method must meet before PG_PRECOND_POLY_EST is served (named in the error otherwise)
void specest_require_one_rank();

// ---- the CGS2 kernels of pg_gmres.hip, shared with the estimate (defined there) -------------------------------------------
constexpr int GM_GRP = 8;   // basis vectors handled per launch of the dot / update kernels
// sums of `nslots` partial slots (fixed order: deterministic) into out[0..nslots)
__global__ __launch_bounds__(BLOCK) void k_gm_reduce(int nslots, int grid, const double* __restrict__ partials,
                                                     double* __restrict__ out, const double* __restrict__ sc, int check_done);
// v *= gm[invn_at]
__global__ __launch_bounds__(BLOCK) void k_gm_scale(i64 n, const double* __restrict__ sc, const double* __restrict__ gm,
                                                    int invn_at, double* __restrict__ v);
// partial slots [k0, k0+cnt) = (V_i, w), i = k0 .. k0+cnt-1   (cnt <= GM_GRP)
__global__ __launch_bounds__(BLOCK) void k_gm_dots(i64 n, i64 stride, int k0, int cnt, const double* __restrict__ V,
                                                   const double* __restrict__ w, const double* __restrict__ sc,
                                                   double* __restrict__ partials);
// w -= sum_{i in [k0,k0+cnt)} h_i V_i ;  norm_slot >= 0: partial slot norm_slot = (w,w) after the update
__global__ __launch_bounds__(BLOCK) void k_gm_update(i64 n, i64 stride, int k0, int cnt, const double* __restrict__ V,
                                                     double* __restrict__ w, const double* __restrict__ h,
                                                     const double* __restrict__ sc, int norm_slot,
                                                     double* __restrict__ partials);

}  // namespace pg
