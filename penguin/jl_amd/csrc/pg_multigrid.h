// pg_multigrid.h -- geometric-aggregation multigrid V-cycle, the right preconditioner `precond = PG_PRECOND_MG` of the BiCGStab
// driver (pg_krylov.hip) for steady monophasic diffusion systems with a Dirichlet interface (DESIGN.md "Multigrid"), and its
// cell-aggregated sibling `precond = PG_PRECOND_MG_CELL` for Dirichlet, Robin and Neumann interfaces alike (DESIGN.md
// "Cell-aggregated multigrid"): the same cycle on a hierarchy whose first coarsening merges the ω and γ unknowns of a cell.
// `precond = PG_PRECOND_MG_STEP` runs that cell-rule cycle on the systems of the unsteady time loop (DESIGN.md "Multigrid in
// the time loop"): the same set-up and the same kernels on another matrix, one hierarchy per assembled matrix.
#pragma once
#include <memory>

#include "pg_system.h"

namespace pg {

constexpr int MG_MAX_LEVELS = 16;
constexpr int MG_COARSEST_ROWS = 200;     // coarsening stops at the first level with at most this many rows (solved exactly)
constexpr int MG_TAIL_DOUBLES = 8000;     // LDS doubles of the fused tail's vectors (64 000 of the 65 536 bytes a workgroup gets)
constexpr int MG_MAX_ROW = 48;            // entries of a coarse row the Galerkin kernels can hold.  Kind rule: a (2N+1)-point row per
                                          // kind pair, <= 14.  Cell rule: the <= 16 fine rows of a level-1 row (<= 2 (2N+1) entries
                                          // each) reach their own and the face-neighbour cells only, which lie in <= 3^N <= 27 coarse
                                          // cells; Galerkin products of a 3^N-point operator stay 3^N-point.  Longer rows: err = 2
constexpr double MG_OMEGA = 0.7;          // damped Jacobi
constexpr double MG_OVER = 1.8;           // over-correction of the coarse-grid correction

// How level 0 is aggregated.  MG_RULE_KIND (PG_PRECOND_MG): ω and γ unknowns apart, kind-major coarse numbering on every level.
// MG_RULE_CELL (PG_PRECOND_MG_CELL): every unknown of a 2 x 2 (x 2) block of padded cells, ω and γ together, shares ONE coarse
// unknown -- the levels >= 1 have one kind.  With a Robin or Neumann interface the γ rows are equations of their own and a coarse
// space of γ unknowns alone has non-positive Galerkin diagonals; the cell rule serves those systems (and Dirichlet ones too).
enum MgRule { MG_RULE_KIND = 0, MG_RULE_CELL = 1 };
inline bool mg_is_precond(int precond) { return precond == PG_PRECOND_MG || precond == PG_PRECOND_MG_CELL; }
inline MgRule mg_rule_of(int precond) { return precond == PG_PRECOND_MG_CELL ? MG_RULE_CELL : MG_RULE_KIND; }
inline const char* mg_precond_name(MgRule rule) { return rule == MG_RULE_CELL ? "PG_PRECOND_MG_CELL" : "PG_PRECOND_MG"; }
// PG_PRECOND_MG_STEP: the cell rule's V-cycle inside the unsteady time loop (DESIGN.md "Multigrid in the time loop").  A value of
// its own: mg_is_precond stays the test for the two steady values, whose conditions refuse every time step.
inline bool mg_is_step(int precond) { return precond == PG_PRECOND_MG_STEP; }
inline bool mg_any_precond(int precond) { return mg_is_precond(precond) || mg_is_step(precond); }
inline MgRule mg_rule_of_any(int precond) { return mg_is_step(precond) ? MG_RULE_CELL : mg_rule_of(precond); }
inline const char* mg_precond_name_of(int precond) { return mg_is_step(precond) ? "PG_PRECOND_MG_STEP" : mg_precond_name(mg_rule_of(precond)); }

// One level.  Level 0 borrows the Krylov matrix Â (unit diagonal: dinv == nullptr); coarser levels own their Galerkin product
// A_{l+1} = P_lᵀ A_l P_l (not equilibrated: the smoother divides by the diagonal).
struct MgLevel {
  i64 n = 0, nnz = 0;
  int K = 2;                           // kinds the keys of this level tell apart (cell rule: 1 on every level)
  int cw = 8;                          // width of `child`: 8, or 8 K of the system between levels 0 and 1 under the cell rule
  i64 ext[3] = {1, 1, 1};              // padded cell grid of this level (dimension 0 fastest)
  const int* rowptr = nullptr;
  const int* col = nullptr;
  const double* val = nullptr;
  DevBuf<int> o_rowptr, o_col;         // storage of the levels >= 1
  DevBuf<double> o_val, dinv;
  DevBuf<int> key;                     // n: kind * cells + linear cell of every row (cell rule: the linear cell alone)
  DevBuf<int> agg;                     // n: row of the next level this row belongs to (all but the last level)
  DevBuf<int> child;                   // cw per row of the NEXT level: its rows of this level by (i&1) + 2 (j&1) + 4 (k&1) (+ 8 kind
                                       // where the cell rule merges the kinds), -1 padded.  Slots ascending = the order of summation
  DevBuf<double> pw;                   // n: prolongation weights 1 / ds (level 0 only; plain 0 / 1 elsewhere)
  DevBuf<double> r, xa, xb;            // work vectors of the levels above the tail (level 0: r and xb are the caller's)
};

struct MgHierarchy {
  std::vector<std::unique_ptr<MgLevel>> lev;
  MgRule rule = MG_RULE_KIND;          // the rule it was built with
  int tail0 = 0;                       // first level of the fused tail (levels [tail0, L) run in one launch by one workgroup)
  DevBuf<double> inv;                  // dense inverse of the last level, row-major
  double setup_ms = 0.0;
  i64 bytes = 0;                       // device memory the hierarchy holds
  const void* matrix = nullptr;        // the CsrMatrix it was built from
};

// the one place the one-rank condition is written (pg_solver.hip mg_conditions, mg_build, krylov_solve)
void mg_require_one_rank(MgRule rule = MG_RULE_KIND);
void mg_require_one_rank_of(int precond);   // ... with the name of any of the three values in the message
// Builds the hierarchy of Â (one rank, no ghosts; a positive diagonal is checked): aggregate maps, coarse
// numbering (flag + scan) and the Galerkin products on the device, the dense inverse of the last level on the host.
void mg_build(MgHierarchy& H, const CsrMatrix& A, const Numbering& nb, const Slab& slab, MgRule rule = MG_RULE_KIND);
// out = M⁻¹ in: one V-cycle (2 + 2 damped Jacobi sweeps, over-corrected, exact last level).  in / out: n_vec device vectors,
// in != out; in is not modified.  sc (may be NULL): the Krylov scalar block, whose done flag makes the kernels return at once.
void mg_apply(MgHierarchy& H, const CsrMatrix& A, const Numbering& nb, const Slab& slab, double* in, double* out, const double* sc,
              hipStream_t st);
// (the host side of the set-up -- the dense inverse of the last level and the choice of the tail -- is in pg_host_algos.h)

}  // namespace pg
