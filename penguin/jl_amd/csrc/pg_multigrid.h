// pg_multigrid.h -- geometric-aggregation multigrid V-cycle, the right preconditioner `precond = PG_PRECOND_MG` of the BiCGStab
// driver (pg_krylov.hip) for steady monophasic diffusion systems with a Dirichlet interface (DESIGN.md "Multigrid").
#pragma once
#include <memory>

#include "pg_system.h"

namespace pg {

constexpr int MG_MAX_LEVELS = 16;
constexpr int MG_COARSEST_ROWS = 200;     // coarsening stops at the first level with at most this many rows (solved exactly)
constexpr int MG_TAIL_DOUBLES = 8000;     // LDS doubles of the fused tail's vectors (64 000 of the 65 536 bytes a workgroup gets)
constexpr int MG_MAX_ROW = 48;            // entries of a coarse row the Galerkin kernels can hold (a (2N+1)-point row per kind pair: <= 14)
constexpr double MG_OMEGA = 0.7;          // damped Jacobi
constexpr double MG_OVER = 1.8;           // over-correction of the coarse-grid correction

// One level.  Level 0 borrows the Krylov matrix Â (unit diagonal: dinv == nullptr); coarser levels own their Galerkin product
// A_{l+1} = P_lᵀ A_l P_l (not equilibrated: the smoother divides by the diagonal).
struct MgLevel {
  i64 n = 0, nnz = 0;
  int K = 2;
  i64 ext[3] = {1, 1, 1};              // padded cell grid of this level (dimension 0 fastest)
  const int* rowptr = nullptr;
  const int* col = nullptr;
  const double* val = nullptr;
  DevBuf<int> o_rowptr, o_col;         // storage of the levels >= 1
  DevBuf<double> o_val, dinv;
  DevBuf<int> key;                     // n: kind * cells + linear cell of every row
  DevBuf<int> agg;                     // n: row of the next level this row belongs to (all but the last level)
  DevBuf<int> child;                   // 8 per row of the NEXT level: its rows of this level by (i&1) + 2 (j&1) + 4 (k&1), -1 padded
  DevBuf<double> pw;                   // n: prolongation weights 1 / ds (level 0 only; plain 0 / 1 elsewhere)
  DevBuf<double> r, xa, xb;            // work vectors of the levels above the tail (level 0: r and xb are the caller's)
};

struct MgHierarchy {
  std::vector<std::unique_ptr<MgLevel>> lev;
  int tail0 = 0;                       // first level of the fused tail (levels [tail0, L) run in one launch by one workgroup)
  DevBuf<double> inv;                  // dense inverse of the last level, row-major
  double setup_ms = 0.0;
  i64 bytes = 0;                       // device memory the hierarchy holds
  const void* matrix = nullptr;        // the CsrMatrix it was built from
};

// the one place the one-rank condition is written (pg_solver.hip mg_conditions, mg_build, krylov_solve)
void mg_require_one_rank();
// Builds the hierarchy of Â (one rank, no ghosts; a positive diagonal is checked): aggregate maps, coarse
// numbering (flag + scan) and the Galerkin products on the device, the dense inverse of the last level on the host.
void mg_build(MgHierarchy& H, const CsrMatrix& A, const Numbering& nb, const Slab& slab);
// out = M⁻¹ in: one V-cycle (2 + 2 damped Jacobi sweeps, over-corrected, exact last level).  in / out: n_vec device vectors,
// in != out; in is not modified.  sc (may be NULL): the Krylov scalar block, whose done flag makes the kernels return at once.
void mg_apply(MgHierarchy& H, const CsrMatrix& A, const Numbering& nb, const Slab& slab, double* in, double* out, const double* sc,
              hipStream_t st);
// (the host side of the set-up -- the dense inverse of the last level and the choice of the tail -- is in pg_host_algos.h)

}  // namespace pg
