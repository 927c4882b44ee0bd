// pg_solver.hip -- Solver / DiffusionUnsteadyMono / DiffusionUnsteadyDiph and their time loops
//
//   reference                                                        here
//   DiffusionUnsteadyMono ctor               diffusion.jl:192-210     pg_solver_create_unsteady_mono
//   DiffusionUnsteadyDiph ctor               diffusion.jl:319-332     pg_solver_create_unsteady_diph
//   b_mono_unstead_diff / b_diph_unstead_diff diffusion.jl:243-265,391-420   k_row_static + k_bconst + k_rhs (K8)
//   solve_DiffusionUnsteadyMono!/Diph!       diffusion.jl:268-301,422-454    pg_solver_initial_solve / _step / _run
//   s.x = zeros(n); s.x[cols_idx] = x_reduced solver.jl:186-187       k_scatter_active (K12)
//
// Everything the loop touches stays in HBM in the reduced (active-set) layout; the padded 2M/4M vector is
// only materialised when the host asks for a state.
#include <algorithm>
#include <cmath>
#include <memory>

#include "pg_krylov.h"
#include "pg_reduce.h"
#include "pg_multigrid.h"
#include "pg_program.h"
#include "pg_scan.h"
#include "pg_solver_internal.h"
#include "pg_spmv.h"
#include "pg_specest.h"

using namespace pg;

namespace pg { extern double g_host_wait_us; }

struct pg_solver {
  int nphase = 1;
  pg_capacity* cap[2] = {nullptr, nullptr};
  pg_diffops* ops[2] = {nullptr, nullptr};   // (their convection data, if any, enters the bulk rows)
  Slab slab;
  int K = 2;
  i64 Mloc = 0, M = 0;
  double dt = 0.0, t = 0.0;
  int scheme_ctor = PG_SCHEME_BE;
  // problem description
  pg_bc_desc bc_i{};          // mono interface condition
  pg_jump_desc ic{};          // diph jumps
  int border_kind[6] = {0, 0, 0, 0, 0, 0};
  double border_value[6] = {0, 0, 0, 0, 0, 0};
  double inv_dx = 0.0;
  DevBuf<double> Id[2];       // D(C_ω), optional
  DevBuf<double> f_n[2], f_np1[2];   // source at t and t+Δt (padded local), optional (NULL = 0)
  DevBuf<double> g_n, g_np1;  // mono interface value arrays, optional
  DevBuf<double> g_arr, h_arr;  // diph jump arrays, optional
  // numbering + matrices
  Numbering nb;
  CsrMatrix A_ctor, A_run;
  GammaElim elim_ctor, elim_run;   // the same matrices without the Dirichlet interface unknowns (pg_reduce.hip), on first use
  DiagElim diag_ctor, diag_run;    // ... without any row that is alone on its diagonal, compact vectors (PG_DIAG_ELIM=1)
  bool have_run = false;
  int scheme_run = -1;
  // per-row data
  DevBuf<double> mass, bconst, bcv;
  DevBuf<unsigned char> fixed;
  int bconst_scheme = -1;
  bool bconst_dirty = true;
  long long bconst_version = 0;   // counts the recomputations of bconst
  // time-separable data Σ_k φ_k(x) a_k(t) (pg_solver_set_separable).  A slot keeps the ROW-SPACE response of each of its terms
  // to unit data without the scheme's factor -- V φ on bulk rows, Γ φ on interface rows, the border value on fixed rows, n_own
  // doubles each -- and the table of coefficients on the host.  bconst of a step is td_base + Σ_j c_j mode_j (k_td_combine),
  // td_base being what k_bconst gives with the separable slots empty; the scheme's factor (Δt, Δt/2, 1) rides in c_j, so a
  // change of the scheme rebuilds td_base alone.
  struct TdSlot {
    int K = 0;                     // 0: empty
    i64 nrows = 0;
    DevBuf<double> mode[PG_TD_MAX_TERMS];
    std::vector<double> coef;      // nrows x 2 x K
    // ... or device functions (pg_solver_set_program; K == 0 then): each a program, the compact list of the rows that carry its
    // data -- (row, weight, point) in SoA form, built once by k_td_points_* -- and the two times of every step.  One program in
    // a source or interface slot; in the border slot one for every border cell (key -1) or one per border key.
    struct Prog {
      pg_program prog;
      int key = -1;
      i64 n = 0;                   // listed rows (0: nothing is launched)
      DevBuf<int> row;
      DevBuf<double> w, p[3];
      i64 nrows = 0;
      std::vector<double> times;   // nrows x 2
    };
    std::vector<Prog> progs;
    bool empty() const { return K == 0 && progs.empty(); }
  };
  TdSlot td[4];                    // source of phase 0, source of phase 1, mono interface value, border values
  DevBuf<double> td_base;
  int td_base_scheme = -1;
  i64 td_cursor = 0;               // the row the next step consumes
  i64 td_row = -1;                 // the row of the step under way
  // block rows of the warm loop's right-hand side with everything that does not depend on the state folded into two tables
  // (k_blk_cache / k_rhs_block_c), valid for one (matrix, scheme, bconst)
  DevBuf<double> blk_wz, blk_c0;
  const CsrMatrix* blk_cache_matrix = nullptr;
  int blk_cache_scheme = -1;
  long long blk_cache_version = -1;
  const DiagElim* rc_last = nullptr;   // the compact system the last step ran on, if it took one (pg_solver_row_const_info)
  // vectors
  DevBuf<double> x, b, y;     // n_vec: unscaled state, scaled right-hand side, Â z
  DevBuf<double> z, ysol;     // n_vec: scaled state S⁻¹x (SpMV input), Krylov solution y (x = S y)
  // The loop carries the SCALED state z (the Krylov solution itself); the unscaled x = S z is materialised only when
  // somebody asks for it (state download, saved states, a cold-start step).
  bool x_valid = true;
  const CsrMatrix* z_matrix = nullptr;   // the matrix whose S the current z refers to
  DevBuf<double> T0pad;       // K*Mloc, ctor initial condition
  KrylovWork work;
  // multigrid hierarchy of A_ctor (pg_multigrid.hip), built by the first solve that asks for PG_PRECOND_MG and kept with the
  // system: a steady solver is solved again and again on the same matrix (the stream-function solver of a pg_streamvort)
  MgHierarchy mg;
  // ... and the one of the cell rule (PG_PRECOND_MG_CELL): one hierarchy per rule, neither reuses or disturbs the other's
  MgHierarchy mg_cell;
  // ŷ = Â z of the NEXT step, queued speculatively behind the previous solve's first batch (KrylovCall::after_first_batch):
  // valid when that solve ended inside the batch (nothing moved z afterwards) and the next step runs on the same matrix
  bool spec_y_valid = false, spec_pending = false, hint_more_steps = false;
  const CsrMatrix* spec_matrix = nullptr;
  // the last states z^{n-1}.. and their products ŷ^{n-1}.. = Â z^{n-1}.. (same-size buffers that trade places with z / y):
  // the extrapolated start of a quiet step (GuessArgs).  hist_cnt of them are valid, all for the matrix of hist_de.
  DevBuf<double> zh[8], yh[8], guess_coef, guess_partials;
  DevBuf<unsigned> guess_ticket;
  int guess_buf = 0;                // which of guess_coef's two coefficient blocks stands (GUESS_USED; 1 only where the fit rides
                                    // in the right-hand-side launch: it reads one block and writes the other)
  int hist_cnt = 0, hist_k = 0;     // (hist_k: the ring's depth the count refers to)
  bool plain_guess_on[2] = {false, false};          // the plain warm path's switch and last solve's products, per matrix
  double plain_last_products[2] = {0.0, 0.0};       // (ctor / run; the compact path keeps its own in DiagElim)
  const void* hist_de = nullptr;
  bool initial_done = false;
  std::vector<DevBuf<double>> states;
  i64 steps_done = 0;
  DevBuf<double> red_scratch;  // max-abs partials
  DevBuf<i64> border_cells_lin;  // global linear index of each border cell (mesh order), lazily uploaded
  // moving body (pg_solver_create_moving_mono): one space-time step; Ψn1 = psip.(Vn, Vn_1), Ψn = psim.(Vn, Vn_1)
  bool moving = false;
  DevBuf<double> psi_p[2], psi_m[2];   // per phase
  // moving advection-diffusion (pg_solver_create_moving_advdiff_*): psip_conv.(Vn, Vn_1) / psim_conv.(Vn, Vn_1), per phase
  // (prescribedmotionsolver/advectiondiffusion.jl:35-61); the convection data come from the ConvectionOps in ops[]
  bool advdiff = false;
  bool convection = false;   // an operator handed to the constructor was a ConvectionOps (noted there: the caller owns the operators)
  DevBuf<double> psi_cp[2], psi_cm[2];
  // the Stefan diphasic blocks (pg_solver_create_moving_stefan_diph, liquidmotionsolver/diffusion.jl:445-651)
  bool stefan = false;
  bool solved_once = false;         // built for one solve and replaced (the vorticity solver of a pg_streamvort step)
  pg_solver* init_from = nullptr;   // constructor only: the previous slab's solver whose state is this one's initial state
  // monitors (pg_solver_set_monitors): weighted sums Σ w_i x_i / Σ w_i x_i² of the state after every completed solve.  The
  // weights live in the solver's row numbering, dense (n_own doubles) or as a sorted (row, weight) list, whichever streams
  // fewer bytes per step (mon_choose_storage).  k_monitor writes one partial per block and monitor straight into `series`
  // (rows x G x K); the G partials of a row are added in the order of the blocks when the series is read.
  struct Monitors {
    int K = 0;                     // 0: none installed -- no launch, no allocation
    int kind[PG_MON_MAX] = {};
    bool sparse[PG_MON_MAX] = {};
    i64 stored[PG_MON_MAX] = {};   // doubles of a dense monitor (n_own), entries of a sparse one
    DevBuf<double> w[PG_MON_MAX];  // dense: the weight of every row; sparse: the weight of every entry
    DevBuf<int> row[PG_MON_MAX];   // sparse: the entries' rows, ascending
    int G = 0;                     // blocks of k_monitor: a function of n_own alone
    DevBuf<double> series;         // cap x G x K
    i64 rows = 0, cap = 0;
    std::vector<double> times;     // s->t of every row
  };
  Monitors mon;
  // the two hierarchies of PG_PRECOND_MG_STEP, one per assembled matrix of the time loop: [0] A_ctor, [1] A_run (dropped with
  // it); slots of their own, beside mg / mg_cell above.  (At the end: every field the default loop touches keeps its offset.)
  MgHierarchy mg_step[2];
};

namespace {

using pg::BLOCK;   // 256 (pg_spmv.h)

struct RowSegs {
  int K;
  i64 off_own[MAX_KINDS];
};

__device__ inline int seg_kind(const RowSegs& s, i64 r) {
  int k = 0;
  while (k + 1 < s.K && r >= s.off_own[k + 1]) ++k;
  return k;
}

RowSegs make_segs(const Numbering& nb) {
  RowSegs s;
  s.K = nb.K;
  for (int k = 0; k < MAX_KINDS; ++k) s.off_own[k] = nb.off_own[k];
  return s;
}

struct KeyVals {
  double v[6];
};

// static per-row data: mass (V for bulk rows that are not overwritten), fixed (b = bconst), border constant
__global__ void k_row_static(SysParams P, RowSegs seg, i64 n_own, const int* row_cell, KeyVals kv, double* mass,
                             unsigned char* fixed, double* bcv) {
  const CapView& c = P.cap[0];
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n_own; r += (i64)gridDim.x * blockDim.x) {
    const int k = seg_kind(seg, r);
    const i64 lc = row_cell[r];
    i64 idx[3];
    decode_cell(c.N, c.ext, c.plane, c.s0, lc, idx);
    double m = 0.0, bv = 0.0;
    unsigned char fx = 0;
    if ((k & 1) == 0) {
      const int ph = k >> 1;
      int key = -1;
      const int bk = border_row_kind(P, ph, lc, idx, &key);
      if (bk != PG_BC_NONE) {
        fx = 1;
        bv = (bk == PG_BC_PERIODIC) ? 0.0 : kv.v[key];
      } else {
        m = P.mv_psi_w[0] ? P.mv_v1[ph][lc] : P.mass * P.cap[ph].V[lc];   // moving: b1 = Vn Tω + ...  (diffusion.jl:214,216)
      }
    } else if (P.nphase == 2) {
      fx = 1;   // jump rows: b2 = g, b4 = Γ₂h for both schemes (diffusion.jl:415-416)
    }
    mass[r] = m;
    fixed[r] = fx;
    bcv[r] = bv;
  }
}

struct SrcView {
  const double* f_n[2];
  const double* f_np1[2];
  const double* g_n;     // mono: g(t)      diph: g array
  const double* g_np1;   // mono: g(t+Δt)   diph: h array
  double g_const, h_const;
};

// time-data part of the right-hand side                 diffusion.jl:257-261, 409-416
__global__ void k_bconst(SysParams P, RowSegs seg, i64 n_own, const int* row_cell, SrcView s, int scheme, double dt,
                         const unsigned char* fixed, const double* bcv, double* bconst, int moving) {
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n_own; r += (i64)gridDim.x * blockDim.x) {
    const int k = seg_kind(seg, r);
    const i64 lc = row_cell[r];
    const int ph = k >> 1;
    double v;
    if ((k & 1) == 0) {
      if (fixed[r]) v = bcv[r];
      else {
        const double V = P.cap[ph].V[lc];
        const double f1 = s.f_np1[ph] ? s.f_np1[ph][lc] : 0.0;
        if (scheme == PG_SCHEME_CN) {
          // f(t) not supplied separately (BE constructor, constant-in-time source): f(t) = f(t+Δt)
          const double f0 = s.f_n[ph] ? s.f_n[ph][lc] : f1;
          v = dt / 2 * V * (f0 + f1);
        } else {
          v = dt * V * f1;
        }
      }
    } else if (P.nphase == 1) {
      const double G = P.cap[0].G[lc];
      const double g1 = s.g_np1 ? s.g_np1[lc] : s.g_const;
      if (scheme == PG_SCHEME_CN && !moving) {   // moving: b2 = Γ g under both schemes (diffusion.jl:218)
        const double g0 = s.g_n ? s.g_n[lc] : s.g_const;
        v = dt / 2 * G * (g0 + g1);
      } else {
        v = G * g1;
      }
    } else if (k == 1 || P.mv_stefan) {
      v = s.g_n ? s.g_n[lc] : s.g_const;                          // b2 = gᵧ  (Stefan: b4 = gᵧ too, :646-647)
    } else {
      v = P.cap[1].G[lc] * (s.g_np1 ? s.g_np1[lc] : s.h_const);   // b4 = Γ₂ hᵧ
    }
    bconst[r] = v;
  }
}

// K8, loop form: x is the previous (unscaled) reduced state; yhat = Â (S⁻¹x) (CN only); output is S b
__global__ void k_rhs(i64 n, int scheme, const double* __restrict__ x, const double* __restrict__ yhat,
                      const double* __restrict__ ds, const double* __restrict__ mass, const double* __restrict__ bconst,
                      const unsigned char* __restrict__ fixed, double* __restrict__ b) {
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) {
    double v;
    if (fixed[r]) v = ds[r] * bconst[r];
    else if (scheme == PG_SCHEME_CN) v = ds[r] * (2.0 * (mass[r] * x[r]) + bconst[r]) - yhat[r];
    else v = ds[r] * (mass[r] * x[r] + bconst[r]);
    b[r] = v;
  }
}

// K8 for the rows of cells with a non-trivial preconditioner block (overwrites what k_rhs wrote there):
//   b̂_r = Σ_j (B⁻¹S)[r,j] c_j  -  Σ_j (B⁻¹MB)[r,j] ŷ_j      c = un-preconditioned constant part, ŷ = Â S⁻¹x
// (x = ds ∘ z when ds != NULL: the loop form carries the scaled state)
__global__ void k_rhs_block(i64 nblk, int scheme, const int* __restrict__ blk_rows, const int* __restrict__ blk_idx,
                            const double* __restrict__ blk_coef, const double* __restrict__ blk_cn,
                            const double* __restrict__ x, const double* __restrict__ ds, const double* __restrict__ yhat,
                            const double* __restrict__ mass, const double* __restrict__ bconst,
                            const unsigned char* __restrict__ fixed, double* __restrict__ b) {
  const double fac = scheme == PG_SCHEME_CN ? 2.0 : 1.0;
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < nblk; q += (i64)gridDim.x * blockDim.x) {
    double v = 0.0;
#pragma unroll
    for (int a = 0; a < MAX_KINDS; ++a) {
      const int j = blk_idx[q * MAX_KINDS + a];
      if (j < 0) continue;
      const double xj = ds ? ds[j] * x[j] : x[j];
      const double cj = fixed[j] ? bconst[j] : fac * (mass[j] * xj) + bconst[j];
      v += blk_coef[q * MAX_KINDS + a] * cj;
      if (scheme == PG_SCHEME_CN) v -= blk_cn[q * MAX_KINDS + a] * yhat[j];
    }
    b[blk_rows[q]] = v;
  }
}

// The same rows in the warm loop, state-independent part precomputed:  b̂_r = c0_q + Σ_a (wz_qa z_j - cn_qa ŷ_j)  with
//   wz_qa = (B⁻¹S)[r,j] fac mass_j s_j  (0 for fixed rows),   c0_q = Σ_a (B⁻¹S)[r,j] bconst_j
// -- two gathers per unknown of the cell instead of six (42 -> ~20 us at 512^3)
__global__ void k_blk_cache(i64 nblk, int scheme, const int* __restrict__ blk_idx, const double* __restrict__ blk_coef,
                            const double* __restrict__ ds, const double* __restrict__ mass, const double* __restrict__ bconst,
                            const unsigned char* __restrict__ fixed, double* __restrict__ wz, double* __restrict__ c0) {
  const double fac = scheme == PG_SCHEME_CN ? 2.0 : 1.0;
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < nblk; q += (i64)gridDim.x * blockDim.x) {
    double c = 0.0;
#pragma unroll
    for (int a = 0; a < MAX_KINDS; ++a) {
      const int j = blk_idx[q * MAX_KINDS + a];
      double w = 0.0;
      if (j >= 0) {
        const double cf = blk_coef[q * MAX_KINDS + a];
        c += cf * bconst[j];
        if (!fixed[j]) w = cf * (fac * (mass[j] * ds[j]));
      }
      wz[q * MAX_KINDS + a] = w;
    }
    c0[q] = c;
  }
}

// the tables of the block rows as the warm loop's kernels take them
struct BlkTables {
  const int* idx;        // blk_idx
  const double* wz;      // k_blk_cache
  const double* c0;
  const double* cn;      // blk_cn
  const int* pos;        // row -> block-table index (CsrMatrix::blk_pos): how the fit's blocks of k_rhs_init_c find a sampled block row
};

// block row q of the table: the one expression of k_rhs_block_c and of the fit's blocks of k_rhs_init_c (guess_fit_part)
__device__ inline double rhs_block_row(i64 q, int scheme, const BlkTables& t, const double* z, const double* yhat) {
  int j[MAX_KINDS];
  double zz[MAX_KINDS], yy[MAX_KINDS];
#pragma unroll
  for (int a = 0; a < MAX_KINDS; ++a) j[a] = t.idx[q * MAX_KINDS + a];
#pragma unroll
  for (int a = 0; a < MAX_KINDS; ++a) {   // every gather in flight before the first FMA
    zz[a] = j[a] >= 0 ? z[j[a]] : 0.0;
    yy[a] = (j[a] >= 0 && scheme == PG_SCHEME_CN) ? yhat[j[a]] : 0.0;
  }
  double v = t.c0[q];
#pragma unroll
  for (int a = 0; a < MAX_KINDS; ++a) v += t.wz[q * MAX_KINDS + a] * zz[a] - (scheme == PG_SCHEME_CN ? t.cn[q * MAX_KINDS + a] * yy[a] : 0.0);
  return v;
}

__global__ void k_rhs_block_c(i64 nblk, int scheme, const int* __restrict__ blk_rows, BlkTables t, const double* __restrict__ z,
                              const double* __restrict__ yhat, double* __restrict__ b) {
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < nblk; q += (i64)gridDim.x * blockDim.x)
    b[blk_rows[q]] = rhs_block_row(q, scheme, t, z, yhat);
}

// The same rows of a DIPHASIC system under Crank-Nicolson, matrix-free: b̂_r = Σ_a (B⁻¹S)[r,a] (c_a - M_a (A x)_a), with
// (A x)_a evaluated from the capacities (eval_row, the row the assembler would store, un-preconditioned) and x = S z.
// The subtraction happens in the row's own scale and B⁻¹ is applied once -- the table form (B⁻¹S)c - (B⁻¹MB)ŷ loses
// eps·cond(B) of b̂ there (M = diag(1,0,1,0) inside a cell: the product is no identity), 1e-8 in 3-D cut cells.
// One thread per block row evaluates the (<= 4) rows of its cell: 4x redundant, on a few thousand rows.
__global__ void k_rhs_block_mf(SysParams P, RowSegs seg, i64 Mloc, i64 nblk, const int* __restrict__ blk_rows,
                               const int* __restrict__ blk_idx, const double* __restrict__ blk_coef,
                               const int* __restrict__ row_cell, const int* __restrict__ red, const double* __restrict__ ds,
                               const double* __restrict__ z, const double* __restrict__ mass, const double* __restrict__ bconst,
                               const unsigned char* __restrict__ fixed, double* __restrict__ b) {
  const CapView& c = P.cap[0];
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < nblk; q += (i64)gridDim.x * blockDim.x) {
    const i64 lc = row_cell[blk_rows[q]];
    i64 idx[3];
    decode_cell(c.N, c.ext, c.plane, c.s0, lc, idx);
    double v = 0.0;
    for (int a = 0; a < MAX_KINDS; ++a) {
      const int j = blk_idx[q * MAX_KINDS + a];
      if (j < 0) continue;
      const int k = seg_kind(seg, j);
      double ca;
      if (fixed[j]) {
        ca = bconst[j];                                         // jump rows, border rows: b = data
      } else {
        double ax = 0.0;                                        // (A x)_j, x = S z
        eval_row(P, k, lc, idx, [&](int ck, i64 cl, double val) {
          const int col = red[(i64)ck * Mloc + cl];
          if (val != 0.0 && col >= 0) ax += val * (ds[col] * z[col]);
        });
        ca = 2.0 * (mass[j] * (ds[j] * z[j])) + bconst[j] - ax;  // CN bulk row: (2 V - A) x + data      diffusion.jl:409-412
      }
      v += blk_coef[q * MAX_KINDS + a] * ca;
    }
    b[blk_rows[q]] = v;
  }
}

// The start of a quiet step extrapolated from older states.  The solver keeps the last R states z^{n-1} .. z^{n-R} and their
// products ŷ^{n-o} = Â z^{n-o} (ring buffers; no extra store: the buffers trade places with z / ŷ).  For a choice of
// offsets o_j, d_j = z^{n-o_j} - z^n and q_j = Â d_j = ŷ^{n-o_j} - ŷ^n cost two reads each, and
//   z_g = z^n + Σ c_j d_j   has the residual   r̂ = (b̂ - ŷ^n) - Σ c_j q_j   exactly (linearity; no product).
// Which (at most KH) offsets and which c_j: the weighted least-squares fit of the PREVIOUS step's plain residual on its
// q_j over a sample of the rows (k_guess_fit, which also weighs the products saved against the reads) -- a second pass for
// this step's own fit would cost what the fit saves, and the c_j move slowly from step to step.  Crank-Nicolson's
// alternating component makes the states of the SAME parity (offsets 1, 3, 5, 7) the useful ones, backward Euler the
// nearest ones; the fit finds that out.  Only the start changes: the iteration and its stopping test see r̂ as ever.
struct GuessArgs {
  const double* zr[8];      // z^{n-1} .. z^{n-R}   (the last one is also znew: a lane reads its element before writing it)
  const double* yr[8];      // ŷ^{n-1} ..
  double* znew;             // z^{n+1}'s buffer: z_g for the rows of the loop, the solved value for a row alone on its diagonal
  const double* coef;       // [0..3] c_j, [4] how many, [5..8] their ring indices o_j - 1   (the fit of the step before)
  double* count;            // += the number of older states this launch read (a running total for the bench's byte count)
  int defer;                // (k_rhs_init_c takes it at compile time, its DEFER)  1: z_g is NOT formed here -- the older states are not read for it and znew gets the rows alone on
                            // their diagonal only; the solve's first update of x writes z_g + α M⁻¹p (KrylovCall::xguess) from
                            // the coefficients this launch read: `coef` itself where the fit rides in this launch (it writes the
                            // other one of two coefficient blocks), else the copy of [0..8] this launch leaves at `used`
  double* used;             // NULL: no copy
};
// The solver's coefficient buffer: block 0 at [0..11] ([9..11]: the fit's diagnostics), [13] the running count, [16..] the
// fit's sums of several ranks, [GUESS_USED..]: the copy of [0..8] for the deferred start, or -- where the fit rides in the
// right-hand-side launch -- coefficient block 1, which trades roles with block 0 at every fit (pg_solver::guess_buf)
constexpr int GUESS_USED = 64;

__device__ inline const double* ring_pick(const double* const (&r)[8], int i) {
  const double* p = r[0];
#pragma unroll
  for (int q = 1; q < 8; ++q) p = i == q ? r[q] : p;   // (uniform: scalar selects, no private-memory copy of the argument)
  return p;
}

// The fit behind the extrapolated start (GuessArgs): over every `stride`-th chunk of BLOCK rows (a few hundred blocks share
// them), the normal equations of
//   min || r_u - Σ c_j q_j ||_W ,  r_u = b̂ - ŷ^n (the plain start residual), q_j = ŷ^{n-j-1} - ŷ^n, j < avail <= RM
// (Gram matrix, right-hand side, (r_u,r_u)_W and (r,r)_W of the start actually taken).  The last block then tries every
// subset of at most kmax of the avail older states -- one thread each, a Cholesky factorisation of at most 4 x 4 -- and
// keeps the one whose saving,  gain · log((r_u,r_u) / (left,left)) / rate2  products, exceeds its reads (2 passes per
// state, pass_cost products each) by most: offsets and coefficients for the NEXT step.
constexpr int GUESS_RM = 7;
constexpr int GUESS_NS = GUESS_RM * (GUESS_RM + 1) / 2 + GUESS_RM + 2;
struct GuessFit {
  const double* yr[8];
  double* partials;       // GUESS_NS * grid
  unsigned* ticket;
  double* coef;           // [0..3] c_j, [4] how many, [5..8] ring indices, [9] (r_u,r_u)_W, [10] (r,r)_W, [11] the fit's left-over
  int stride, avail, kmax;
  double rate2, pass_cost, gain;
  double* sums;           // several ranks: where the GUESS_NS local sums go (NULL: one rank, the launch decides itself)
  int nblocks;            // blocks the partial sums are kept for (k_guess_fit: its grid)
};

__device__ inline int guess_tri(int j, int l) { return j * GUESS_RM - j * (j - 1) / 2 + (l - j); }   // l >= j

// the choice among the subsets (k_guess_fit's doc), from the sums s_g (GUESS_NS of them, in LDS), by the whole block
__device__ inline void guess_decide(const double* s_g, const GuessFit& f) {
  constexpr int RM = GUESS_RM, NS = GUESS_NS;
  __shared__ double s_left[128], s_net[128];
  __shared__ double s_c[128][4];
  const double ru = s_g[NS - 2], rw = s_g[NS - 1];
  // one subset of the older states per thread: bit j of the thread number = state j
  if (threadIdx.x < 128) {
    const int mask = threadIdx.x, m = __popc(mask);
    double left = ru, cc[4] = {0.0, 0.0, 0.0, 0.0};
    if (mask != 0 && m <= f.kmax && m <= 4 && (mask >> f.avail) == 0 && ru > 0.0) {
      int idx[4] = {0, 0, 0, 0};
      for (int j = 0, a = 0; j < RM; ++j) if (mask >> j & 1) { if (a < 4) idx[a] = j; ++a; }
      double L[4][4], wv[4];
      bool ok = true;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        wv[a] = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) L[a][e] = 0.0;
      }
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (a >= m || !ok) continue;
        const double g0 = s_g[guess_tri(idx[a], idx[a])];
        double dj = g0;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (e < a) dj -= L[a][e] * L[a][e];
        if (!(g0 > 0.0) || !(dj > 1e-12 * g0)) { ok = false; continue; }   // (collinear with the ones before it)
        const double lj = sqrt(dj);
        L[a][a] = lj;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          if (l <= a || l >= m) continue;
          double v = s_g[guess_tri(idx[a], idx[l])];
#pragma unroll
          for (int e = 0; e < 4; ++e) if (e < a) v -= L[l][e] * L[a][e];
          L[l][a] = v / lj;
        }
        double v = s_g[RM * (RM + 1) / 2 + idx[a]];
#pragma unroll
        for (int e = 0; e < 4; ++e) if (e < a) v -= L[a][e] * wv[e];
        wv[a] = v / lj;
        left -= wv[a] * wv[a];
      }
      if (ok) {
#pragma unroll
        for (int aa = 0; aa < 4; ++aa) {            // Lᵀ c = w
          const int a = 3 - aa;
          if (a >= m) continue;
          double v = wv[a];
#pragma unroll
          for (int e = 0; e < 4; ++e) if (e > a && e < m) v -= L[e][a] * cc[e];
          cc[a] = v / L[a][a];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) ok = ok && isfinite(cc[a]) && fabs(cc[a]) < 256.0;
      }
      if (!ok) { left = ru; cc[0] = cc[1] = cc[2] = cc[3] = 0.0; }
      if (!(left > 1e-30 * ru)) left = 1e-30 * ru;
    }
    s_left[threadIdx.x] = left;
#pragma unroll
    for (int a = 0; a < 4; ++a) s_c[threadIdx.x][a] = cc[a];
    // what the subset nets: the products its fit saves less its reads (a start that the extrapolation made worse: none
    // next time)
    const bool live = ru > 0.0 && f.rate2 > 0.0 && rw <= ru * (1.0 + 1e-12) && left < ru;
    s_net[threadIdx.x] = live ? f.gain * log(ru / left) / f.rate2 - 2.0 * m * f.pass_cost : 0.0;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    // the subset that nets most (ties: the lower number), by the first wave
    int pick = threadIdx.x;
    double best = s_net[pick];
    if (s_net[pick + 64] > best) { best = s_net[pick + 64]; pick += 64; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ob = __shfl_down(best, off, 64);
      const int op = __shfl_down(pick, off, 64);
      if (ob > best || (ob == best && op < pick)) { best = ob; pick = op; }
    }
    if (!(best > 0.0)) pick = 0;
    if (threadIdx.x != 0) return;
    int a = 0;
    for (int j = 0; j < RM; ++j)
      if (pick >> j & 1) { f.coef[a] = s_c[pick][a]; f.coef[5 + a] = (double)j; ++a; }
    f.coef[4] = (double)a;
    for (; a < 4; ++a) { f.coef[a] = 0.0; f.coef[5 + a] = 0.0; }
    f.coef[9] = ru; f.coef[10] = rw; f.coef[11] = pick ? s_left[pick] : ru;
  }
}

// K8 + the BiCGStab start in one pass (loop form, warm start): from the scaled state z and ŷ = Âz
//   b̂ = S(2 mass∘(S z) + bconst) - ŷ  (CN) | S(mass∘(S z) + bconst) (BE) | S bconst (fixed rows) | as written by k_rhs_block
//   r = r̂ = p = b̂ - ŷ,  x = z (in place),  partial sums of (r,r) and (b̂,b̂) in slots 0 / 1   (k_rhs_init_c: r̂ only)
// replaces k_rhs + k_bicg_init: 9.3 instead of 14.1 vector passes, and no separate scaling kernels per step
typedef double rd2_t __attribute__((ext_vector_type(2)));
typedef unsigned char ruc2_t __attribute__((ext_vector_type(2)));

// one element of k_rhs_init
__device__ inline void rhs_init_one(int scheme, double z, double yh, double d, double ms, double bc, bool fx, bool blk, double bold,
                                    double& bi, double& ri) {
  if (blk) bi = bold;
  else if (fx) bi = d * bc;
  else if (scheme == PG_SCHEME_CN) bi = d * (2.0 * (ms * (d * z)) + bc) - yh;
  else bi = d * (ms * (d * z) + bc);
  ri = bi - yh;
}

// TWO elements per lane (16-byte accesses: half the vector-memory instructions of the 11 streams; the two flag bytes of
// a pair come with one 2-byte load each); the odd last element and the ghost tail are handled by the same lanes
// KH > 0: the start extrapolated from older states (GuessArgs; every row takes part: no row is left out on this path), the
// state written out of place
template <int KH>
__global__ __launch_bounds__(BLOCK) void k_rhs_init(i64 n, i64 nvec, int scheme, const double* __restrict__ z,
                                                    const double* __restrict__ yhat, const double* __restrict__ ds,
                                                    const double* __restrict__ mass, const double* __restrict__ bconst,
                                                    const unsigned char* __restrict__ fixed,
                                                    const unsigned char* __restrict__ isblk, double* __restrict__ b,
                                                    double* __restrict__ r, double* __restrict__ rhat,
                                                    double* __restrict__ p, double* __restrict__ partials, GuessArgs g) {
  __shared__ double s_red[BLOCK / 64];
  double acc = 0.0, accb = 0.0, accw = 0.0;   // (r,r), (b,b)_W, (r,r)_W: slots 0, 1, 2 as k_bicg_init (weights ds²)
  double cj[KH > 0 ? KH : 1];
  const double* zo[KH > 0 ? KH : 1];
  const double* yo[KH > 0 ? KH : 1];
  int ku = 0;
  if (KH > 0) {
    ku = min(KH, (int)g.coef[4]);
#pragma unroll
    for (int j = 0; j < KH; ++j) {
      const int sel = j < ku ? (int)g.coef[5 + j] : 0;
      cj[j] = j < ku ? g.coef[j] : 0.0;
      zo[j] = ring_pick(g.zr, sel);
      yo[j] = ring_pick(g.yr, sel);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *g.count += (double)ku;
  }
  const i64 npair = (nvec + 1) / 2;
  for (i64 q = blockIdx.x * (i64)BLOCK + threadIdx.x; q < npair; q += (i64)gridDim.x * BLOCK) {
    const i64 i = 2 * q;
    if (i + 1 < n) {
      // (stream hints: the per-row data is read once per step and b̂ is only kept for inspection -- neither should
      //  displace the SpMV's matrix data from the Infinity Cache)
      const rd2_t yh = __builtin_nontemporal_load(reinterpret_cast<const rd2_t*>(yhat + i));
      const rd2_t d = __builtin_nontemporal_load(reinterpret_cast<const rd2_t*>(ds + i));
      const rd2_t bc = __builtin_nontemporal_load(reinterpret_cast<const rd2_t*>(bconst + i));
      const rd2_t ms = __builtin_nontemporal_load(reinterpret_cast<const rd2_t*>(mass + i));
      const rd2_t zz = *reinterpret_cast<const rd2_t*>(z + i);
      const ruc2_t fx = *reinterpret_cast<const ruc2_t*>(fixed + i);
      const ruc2_t bk = *reinterpret_cast<const ruc2_t*>(isblk + i);
      rd2_t bold;
      bold.x = 0.0; bold.y = 0.0;
      if (bk.x | bk.y) bold = *reinterpret_cast<const rd2_t*>(b + i);
      double b0, r0, b1, r1;
      rhs_init_one(scheme, zz.x, yh.x, d.x, ms.x, bc.x, fx.x != 0, bk.x != 0, bold.x, b0, r0);
      rhs_init_one(scheme, zz.y, yh.y, d.y, ms.y, bc.y, fx.y != 0, bk.y != 0, bold.y, b1, r1);
      if (KH > 0) {
        rd2_t zg = zz;
#pragma unroll
        for (int j = 0; j < KH; ++j) {
          if (j < ku) {
            const rd2_t a = *reinterpret_cast<const rd2_t*>(zo[j] + i);
            const rd2_t y2 = *reinterpret_cast<const rd2_t*>(yo[j] + i);
            r0 -= cj[j] * (y2.x - yh.x); r1 -= cj[j] * (y2.y - yh.y);
            zg.x += cj[j] * (a.x - zz.x); zg.y += cj[j] * (a.y - zz.y);
          }
        }
        *reinterpret_cast<rd2_t*>(g.znew + i) = zg;
      }
      rd2_t bi, ri;
      bi.x = b0; bi.y = b1; ri.x = r0; ri.y = r1;
      __builtin_nontemporal_store(bi, reinterpret_cast<rd2_t*>(b + i));
      *reinterpret_cast<rd2_t*>(r + i) = ri;
      *reinterpret_cast<rd2_t*>(rhat + i) = ri;
      *reinterpret_cast<rd2_t*>(p + i) = ri;
      acc += ri.x * ri.x + ri.y * ri.y;
      accb += (d.x * bi.x) * (d.x * bi.x) + (d.y * bi.y) * (d.y * bi.y);
      accw += (d.x * ri.x) * (d.x * ri.x) + (d.y * ri.y) * (d.y * ri.y);
    } else {
      for (i64 k = i; k < i + 2 && k < nvec; ++k) {
        if (k < n) {
          double bi, ri;
          rhs_init_one(scheme, z[k], yhat[k], ds[k], mass[k], bconst[k], fixed[k] != 0, isblk[k] != 0, isblk[k] ? b[k] : 0.0, bi, ri);
          if (KH > 0) {
            double zg = z[k];
#pragma unroll
            for (int j = 0; j < KH; ++j)
              if (j < ku) { ri -= cj[j] * (yo[j][k] - yhat[k]); zg += cj[j] * (zo[j][k] - z[k]); }
            g.znew[k] = zg;
          }
          b[k] = bi;
          r[k] = ri; rhat[k] = ri; p[k] = ri;
          acc += ri * ri;
          accb += (ds[k] * bi) * (ds[k] * bi);
          accw += (ds[k] * ri) * (ds[k] * ri);
        } else {
          p[k] = 0.0;
        }
      }
    }
  }
  const double t = block_sum(acc, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
  const double tb = block_sum(accb, s_red);
  if (threadIdx.x == 0) partials[gridDim.x + blockIdx.x] = tb;
  const double tw = block_sum(accw, s_red);
  if (threadIdx.x == 0) partials[2 * (size_t)gridDim.x + blockIdx.x] = tw;
}

// the last block of a fit, every block's partial sums standing: the sums in a fixed order -- a wave per sum, a lane per block
// (at most 128 blocks), shuffle tree; every load of a wave in flight before the first is used, the trees level by level --
// and the decision (one rank) or the hand-over to the all-reduce (several)
__device__ inline void guess_fit_last(const GuessFit& f, int G, double* s_g) {
  constexpr int NS = GUESS_NS;
  {
    constexpr int PW = (NS + BLOCK / 64 - 1) / (BLOCK / 64);   // sums per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double a0[PW], a1[PW];
#pragma unroll
    for (int k = 0; k < PW; ++k) {
      const int sl = wave + k * (BLOCK / 64);
      a0[k] = (sl < NS && lane < G) ? pg::load_partial(f.partials + (size_t)sl * G + lane) : 0.0;
      a1[k] = (sl < NS && lane + 64 < G) ? pg::load_partial(f.partials + (size_t)sl * G + lane + 64) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < PW; ++k) a0[k] += a1[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int k = 0; k < PW; ++k) a0[k] += __shfl_down(a0[k], off, 64);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < PW; ++k) {
        const int sl = wave + k * (BLOCK / 64);
        if (sl < NS) s_g[sl] = a0[k];
      }
    }
  }
  __syncthreads();
  if (f.sums) {                     // several ranks: the sums go through an all-reduce, k_guess_decide follows
    if (threadIdx.x < NS) f.sums[threadIdx.x] = s_g[threadIdx.x];
    return;
  }
  guess_decide(s_g, f);
}

// the correction of the start residual by the chosen older products (cj = 0, yv = yh beyond the ones in use)
template <int KH>
__device__ inline double guess_corr(const double* cj, const double* yv, double yh) {
  double corr = 0.0;
#pragma unroll
  for (int j = 0; j < KH; ++j) corr += cj[j] * (yv[j] - yh);
  return corr;
}

// Which instantiations of k_rhs_init_c take the fit inside: KH (the older states the launch is built for) from 2 on, the
// extrapolated state left to the solve's first update of x (DEFER, the default: the launch then reads no older state, and
// its main path has the registers to spare).  Those ask, by their launch bounds, for 5 waves per SIMD -- KH = 4 had 4: the
// fifth is the slot in which the fit's blocks run beside the 4 main blocks per CU, from the launch's start -- and must
// reach them without scratch; every other instantiation is compiled as it was and keeps k_guess_fit as a launch.
// profiles/step_head_resource_usage_{parent,this}.txt have the compiler's report.
constexpr bool rhs_fuses(int KH, bool DEFER) { return KH >= 2 && DEFER; }
// The 37 sums of the fit are shared out among FIT_PARTS blocks per sampled set of chunks, FIT_PER sums each: the
// accumulators of one group and the row in flight fit the registers of the main path (all 37 in one block: 158 VGPRs)
constexpr int FIT_PARTS = 5, FIT_PER = (GUESS_NS + FIT_PARTS - 1) / FIT_PARTS;

// The fit as blocks of the right-hand-side launch itself (k_rhs_init_c: the blocks past its main ones).  bid / G: the
// number of the k_guess_fit block whose chunks this block takes, and their count; part: its group of sums.  What k_guess_fit
// reads from b̂ and r̂ is being written by the main blocks of the same launch, so a fit block evaluates both for its sampled
// rows from the launch's inputs, by the main blocks' own functions (rhs_init_one, guess_corr; a sampled block row by
// rhs_block_row, the function of k_rhs_block_c): the same bits.  Every sum is k_guess_fit's -- a lane adds its chunks in
// their order, then the shuffle tree, the waves, the blocks.  The FIT_PARTS blocks of a bid read the same rows, about 5 MB
// in all at 512^3; what they buy is a chain of dependent memory round trips per block -- 2 to 3 us each beside the main
// blocks' streams -- that is a fraction of the launch: one block taking the groups one after another outlasted the main blocks.
template <int KH, int PART>
__device__ inline void guess_fit_part(i64 n, int scheme, const double* z, const double* yhat, const double* ds, const double* mass,
                                      const double* bconst, const unsigned char* fixed, const unsigned char* isblk, const int* cmap,
                                      const BlkTables& bt, const GuessArgs& g, const GuessFit& f, int bid, int G, const double (&cj)[KH],
                                      const int (&sel)[KH], int ku, int nld, double (*s_w)[GUESS_NS]) {
  constexpr int RM = GUESS_RM, NS = GUESS_NS, PER = FIT_PER, T0 = PART * PER, T1 = T0 + PER < NS ? T0 + PER : NS;
  constexpr bool NEED_RU = T1 > RM * (RM + 1) / 2, NEED_RA = T1 == NS;
  double gs[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) gs[k] = 0.0;
  const i64 nchunk = (n + BLOCK - 1) / BLOCK;
  for (i64 ch = (i64)bid * f.stride; ch < nchunk; ch += (i64)G * f.stride) {
    const i64 i = ch * BLOCK + threadIdx.x;
    if (i >= n) continue;
    // (every stream at once: the rows left out of the loop are read too and dropped below)
    // (a group made of Gram entries alone needs neither residual, NEED_RU, nor the residual taken, NEED_RA)
    const int c = cmap[i];
    const double d = ds[i], y0 = yhat[i];
    double zi = 0.0, ms = 0.0, bc = 0.0;
    bool fx = false, bk = false;
    if (NEED_RU) { zi = z[i]; ms = mass[i]; bc = bconst[i]; fx = fixed[i] != 0; bk = isblk[i] != 0; }
    double yr[RM];
#pragma unroll
    for (int j = 0; j < RM; ++j) yr[j] = j < nld ? g.yr[j][i] : 0.0;      // (g.yr: the pointers of f.yr)
    if (c < 0) continue;
    const double w = d * d;
    double bi, ru = 0.0, ra = 0.0;
    if (NEED_RU) rhs_init_one(scheme, zi, y0, d, ms, bc, fx, bk, bk ? rhs_block_row(bt.pos[i], scheme, bt, z, yhat) : 0.0, bi, ru);
    if (NEED_RA) {
      double yv[KH];
#pragma unroll
      for (int j = 0; j < KH; ++j) {
        double v = yr[0];
#pragma unroll
        for (int q = 1; q < RM; ++q) v = sel[j] == q ? yr[q] : v;
        yv[j] = j < ku ? v : y0;
      }
      ra = ru - guess_corr<KH>(cj, yv, y0);
    }
    double q[RM];
#pragma unroll
    for (int j = 0; j < RM; ++j) q[j] = j < f.avail ? yr[j] - y0 : 0.0;
    int t = 0;                      // (k_guess_fit's sums in its numbering; this block keeps [T0, T1) of them)
#pragma unroll
    for (int j = 0; j < RM; ++j)
#pragma unroll
      for (int l = j; l < RM; ++l, ++t)
        if (t >= T0 && t < T1) gs[t - T0] += w * q[j] * q[l];
#pragma unroll
    for (int j = 0; j < RM; ++j, ++t)
      if (t >= T0 && t < T1) gs[t - T0] += w * q[j] * ru;
    if (t >= T0 && t < T1) gs[t - T0] += w * ru * ru;
    ++t;
    if (t >= T0 && t < T1) gs[t - T0] += w * ra * ra;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < PER; ++k) gs[k] += __shfl_down(gs[k], off, 64);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (T0 + k < T1) s_w[threadIdx.x >> 6][T0 + k] = gs[k];
  }
}

template <int KH>
__device__ inline void guess_fit_rows(i64 n, int scheme, const double* z, const double* yhat, const double* ds, const double* mass,
                                      const double* bconst, const unsigned char* fixed, const unsigned char* isblk, const int* cmap,
                                      const BlkTables& bt, const GuessArgs& g, const GuessFit& f, int bid, int part, int G,
                                      double* s_red) {
  constexpr int NS = GUESS_NS, RM = GUESS_RM;
  __shared__ double s_g[NS];
  __shared__ double s_w[BLOCK / 64][NS];
  // the coefficients the main blocks of this launch take
  double cj[KH];
  int sel[KH];
  const int ku = min(KH, (int)g.coef[4]);
  int nld = f.avail;                // products read per row: the fit's, and the ones the start takes
#pragma unroll
  for (int j = 0; j < KH; ++j) {
    sel[j] = j < ku ? (int)g.coef[5 + j] : 0;
    cj[j] = j < ku ? g.coef[j] : 0.0;
    if (j < ku) nld = max(nld, sel[j] + 1);
  }
  nld = min(nld, RM);
#define PG_FIT_PART(P) guess_fit_part<KH, P>(n, scheme, z, yhat, ds, mass, bconst, fixed, isblk, cmap, bt, g, f, bid, G, cj, sel, ku, nld, s_w)
  static_assert(FIT_PARTS == 5, "guess_fit_rows: one case per group of sums");
  switch (part) {                   // (uniform per block)
    case 0: PG_FIT_PART(0); break;
    case 1: PG_FIT_PART(1); break;
    case 2: PG_FIT_PART(2); break;
    case 3: PG_FIT_PART(3); break;
    default: PG_FIT_PART(4); break;
  }
#undef PG_FIT_PART
  __syncthreads();
  const int t0 = part * FIT_PER;
  if ((int)threadIdx.x >= t0 && (int)threadIdx.x < min(t0 + FIT_PER, NS)) {
    double a = 0.0;
#pragma unroll
    for (int q = 0; q < BLOCK / 64; ++q) a += s_w[q][threadIdx.x];
    pg::store_partial(f.partials + (size_t)threadIdx.x * G + bid, a);
  }
  if (!pg::last_block_arrives(f.ticket, (unsigned)(FIT_PARTS * G), s_red)) return;
  guess_fit_last(f, G, s_g);
}

// k_rhs_init for a COMPACT loop system (pg_reduce.hip, DiagElim): cmap[i] >= 0: the row stays, r = r̂ = p go to that index of
// the compact vectors and count in the start sums; cmap[i] = -1 - e: the row is alone on its diagonal (entry e of gdiag /
// delta): solved on the spot, left out of the sums.  b̂ is written for every row, (b̂,b̂)_W sums over all of them.
// KH > 0: the extrapolated start above (out of place: the state written is g.znew), up to KH older states.
// DEFER: GuessArgs::defer at compile time (the older states' registers are not taken where they are not read).
template <int KH, bool DEFER>
__global__ __launch_bounds__(BLOCK, (rhs_fuses(KH, DEFER) ? 5 : 1)) void k_rhs_init_c(i64 n, int scheme, const double* z,
                                                      const double* __restrict__ yhat, const double* __restrict__ ds,
                                                      const double* __restrict__ mass, const double* __restrict__ bconst,
                                                      const unsigned char* __restrict__ fixed,
                                                      const unsigned char* __restrict__ isblk, const int* __restrict__ cmap,
                                                      double* __restrict__ b, const double* __restrict__ gdiag,
                                                      double* __restrict__ delta, int* __restrict__ flag, int stamp,
                                                      double* __restrict__ rhat, double* __restrict__ partials,
                                                      unsigned* __restrict__ ticket, double* __restrict__ sc, double reltol2,
                                                      double abstol2, int coupled, GuessArgs g, BlkTables bt, GuessFit gf,
                                                      int main_grid, RowConst rc) {
  // (p = r = r̂ are NOT written: the first iteration reads r̂ for them, KrylovCall::p_in_rhat)
  // coupled != 0: diag_fix follows (the data changed): every δ != 0 moves its row, raises the flag and is coupled into the
  // residual of the rows that reference it.  coupled == 0: no coupling launch follows (unchanged data); only a δ beyond the
  // noise threshold raises the flag, and the step is then finished on the full system.  Several ranks with unchanged data
  // take this branch WITHOUT a ticket (their start phase goes through an all-reduce): there a δ within the threshold still
  // moves its row with neither coupling nor S_HELD, and the residual reported can miss the state's by up to ||S Â_RE δ|| --
  // the one-rank remedy below needs the held sum in that all-reduce and is not carried over yet.
  // ticket != NULL: the solver's start phase (scalar reset, start sums, PH_INIT) by the last block of this launch -- the
  // caller knows that nothing will touch the start sums afterwards (diag_fix is not launched).  A row alone on its diagonal
  // whose δ is within the noise threshold then STAYS where it is: moving it would leave the start residual of the rows coupled
  // to it -- formed from ŷ = Âz with the row at its old place -- short of Â_RE δ, and with it every residual the solve reports
  // afterwards.  (With a Dirichlet interface and CN such a row reads x_new = 2 g - x_old: what the first solve left on it, a
  // fraction of its tolerance, changes sign every step and never dies out.)  What the rows that stay lack is their own
  // residual, constant through the solve and on rows of their own: its weighted square goes to S_HELD, the tolerance of the
  // iteration is lowered by it and the residual reported has it added (pg_krylov.hip) -- the solve is accepted on, and
  // reports, the residual of the whole state.  Where that square is half the tolerance's or more the step is finished on the
  // full system, as if a row had moved.
  __shared__ double s_red[BLOCK / 64];
  // main_grid > 0: the blocks past the first main_grid are the fit's (guess_fit_rows); the main blocks stride, count and sum
  // over main_grid, and the fit's blocks draw the fit's ticket and write the fit's partials only
  const unsigned G0 = main_grid > 0 ? (unsigned)main_grid : gridDim.x;
  if (KH > 0 && blockIdx.x >= G0) {      // (uniform per block)
    if constexpr (rhs_fuses(KH, DEFER))
      guess_fit_rows<KH>(n, scheme, z, yhat, ds, mass, bconst, fixed, isblk, cmap, bt, g, gf, (int)((blockIdx.x - G0) % gf.nblocks),
                         (int)((blockIdx.x - G0) / gf.nblocks), gf.nblocks, s_red);
    return;
  }
  double acc = 0.0, accb = 0.0, accw = 0.0, acch = 0.0;
  const bool hold = ticket != nullptr;
  double cj[KH > 0 ? KH : 1];
  const double* zo[KH > 0 ? KH : 1];
  const double* yo[KH > 0 ? KH : 1];
  int ku = 0;
  constexpr bool defer = KH > 0 && DEFER;
  if (KH > 0) {
    ku = min(KH, (int)g.coef[4]);
#pragma unroll
    for (int j = 0; j < KH; ++j) {
      const int sel = j < ku ? (int)g.coef[5 + j] : 0;
      cj[j] = j < ku ? g.coef[j] : 0.0;
      zo[j] = ring_pick(g.zr, sel);
      yo[j] = ring_pick(g.yr, sel);
    }
    if (defer && g.used && blockIdx.x == 0 && threadIdx.x < 9) g.used[threadIdx.x] = g.coef[threadIdx.x];
  }
  int moved = 0;
  double* zw = KH > 0 ? g.znew : const_cast<double*>(z);   // (in place: a lane writes only elements it has read itself)
  // zh / yv: the row's entries of the chosen older states and products
  auto one = [&](i64 i, double zi, double yh, double d, double ms, double bc, bool fx, bool blk, double bold, int c, double& bi,
                 const double* zh, const double* yv) {
    double ri;
    rhs_init_one(scheme, zi, yh, d, ms, bc, fx, blk, bold, bi, ri);
    accb += (d * bi) * (d * bi);
    if (c >= 0) {
      if (KH > 0) {
        double zg = zi;
#pragma unroll
        for (int j = 0; j < KH; ++j) zg += cj[j] * (zh[j] - zi);      // (cj = 0, yv = yh, zh = zi beyond ku)
        ri -= guess_corr<KH>(cj, yv, yh);
        if (!defer) zw[i] = zg;
      }
      rhat[c] = ri;
      acc += ri * ri;
      accw += (d * ri) * (d * ri);
    } else {
      // a row alone on its diagonal: solved here, x += δ = r / a_ii (δ = 0 once the row's datum has stopped changing, up to
      // the rows that stay on a folded start); δ is what the rows coupled to it need (diag_fix), the flag says whether any row moved
      const int e = -1 - c;
      double dl = ri / gdiag[e];
      const bool beyond = fabs(dl) > 1e-12 * fabs(zi);
      if (hold && !beyond) {
        acch += (d * ri) * (d * ri);
        dl = 0.0;
      }
      delta[e] = dl;
      if (KH > 0 || dl != 0.0) zw[i] = zi + dl;
      if (coupled ? dl != 0.0 : beyond) moved = 1;
    }
  };
  // two rows per lane, 16-byte loads of the seven input streams (as k_rhs_init); the compact stores are 8-byte
  const i64 npair = (n + 1) / 2;
  for (i64 q = blockIdx.x * (i64)BLOCK + threadIdx.x; q < npair; q += (i64)G0 * BLOCK) {
    const i64 i = 2 * q;
    double zh0[KH > 0 ? KH : 1], zh1[KH > 0 ? KH : 1], yv0[KH > 0 ? KH : 1], yv1[KH > 0 ? KH : 1];
    if (i + 1 < n) {
      // RowConst (pg_system.h): a group of 16 rows -- 8 lanes -- whose ds, mass (and bconst, where its mark stands) are one value
      // each, no row fixed or a block row, cmap advancing by one from e: those lanes request none of the six lines
      const int e = rc.tab ? rc.tab[i >> RC_SHIFT] : -1;
      const bool bc_one = e >= 0 && rc.bmark && rc.bmark[i >> RC_SHIFT] != 0;
      const rd2_t yh = __builtin_nontemporal_load(reinterpret_cast<const rd2_t*>(yhat + i));
      const rd2_t zz = *reinterpret_cast<const rd2_t*>(z + i);
      rd2_t d, bc, ms;
      ruc2_t fx, bk;
      int c0 = e + (int)(i & (RC_GROUP - 1)), c1 = c0 + 1;
      d.x = rc.d; d.y = rc.d; ms.x = rc.ms; ms.y = rc.ms; bc.x = rc.bc; bc.y = rc.bc;
      fx.x = 0; fx.y = 0; bk.x = 0; bk.y = 0;
      if (e < 0) {
        d = __builtin_nontemporal_load(reinterpret_cast<const rd2_t*>(ds + i));
        ms = __builtin_nontemporal_load(reinterpret_cast<const rd2_t*>(mass + i));
        fx = *reinterpret_cast<const ruc2_t*>(fixed + i);
        bk = *reinterpret_cast<const ruc2_t*>(isblk + i);
        c0 = cmap[i]; c1 = cmap[i + 1];
      }
      if (!bc_one) bc = __builtin_nontemporal_load(reinterpret_cast<const rd2_t*>(bconst + i));
      rd2_t bold;
      bold.x = 0.0; bold.y = 0.0;
      if (bk.x | bk.y) bold = *reinterpret_cast<const rd2_t*>(b + i);
      if (KH > 0) {
#pragma unroll
        for (int j = 0; j < KH; ++j) {
          rd2_t a = zz, y2 = yh;
          if (j < ku && (c0 >= 0 || c1 >= 0)) {     // (rows alone on their diagonal take nothing from the older states)
            if (!defer) a = *reinterpret_cast<const rd2_t*>(zo[j] + i);
            y2 = *reinterpret_cast<const rd2_t*>(yo[j] + i);
          }
          zh0[j] = a.x; zh1[j] = a.y; yv0[j] = y2.x; yv1[j] = y2.y;
        }
      }
      rd2_t bi;
      double b0, b1;
      one(i, zz.x, yh.x, d.x, ms.x, bc.x, fx.x != 0, bk.x != 0, bold.x, c0, b0, zh0, yv0);
      one(i + 1, zz.y, yh.y, d.y, ms.y, bc.y, fx.y != 0, bk.y != 0, bold.y, c1, b1, zh1, yv1);
      bi.x = b0; bi.y = b1;
      __builtin_nontemporal_store(bi, reinterpret_cast<rd2_t*>(b + i));
    } else if (i < n) {
      const double zi = z[i], yh = yhat[i];
      if (KH > 0) {
#pragma unroll
        for (int j = 0; j < KH; ++j) {
          zh0[j] = (j < ku && !defer) ? zo[j][i] : zi;
          yv0[j] = j < ku ? yo[j][i] : yh;
        }
      }
      double b0;
      one(i, zi, yh, ds[i], mass[i], bconst[i], fixed[i] != 0, isblk[i] != 0, isblk[i] ? b[i] : 0.0, cmap[i], b0, zh0, yv0);
      b[i] = b0;
    }
  }
  if (__any(moved) && (threadIdx.x & 63) == 0) atomicMax(flag, stamp);
  const double t = block_sum(acc, s_red);
  const double tb = block_sum(accb, s_red);
  const double tw = block_sum(accw, s_red);
  if (!ticket) {
    if (threadIdx.x == 0) {
      partials[blockIdx.x] = t;
      partials[G0 + blockIdx.x] = tb;
      partials[2 * (size_t)G0 + blockIdx.x] = tw;
      if (KH > 0 && blockIdx.x == 0) *g.count += (double)ku;
    }
    return;
  }
  if (threadIdx.x == 0) {
    pg::store_partial(partials + blockIdx.x, t);
    pg::store_partial(partials + G0 + blockIdx.x, tb);
    pg::store_partial(partials + 2 * (size_t)G0 + blockIdx.x, tw);
  }
  const double th = block_sum(acch, s_red);
  if (threadIdx.x == 0) pg::store_partial(partials + 3 * (size_t)G0 + blockIdx.x, th);
  if (!pg::last_block_arrives(ticket, G0, s_red)) return;
  // (k_start's work, in its order of summation)
  if (threadIdx.x < pg::S_COUNT) sc[threadIdx.x] = threadIdx.x == pg::S_RELTOL2 ? reltol2 : (threadIdx.x == pg::S_ABSTOL2 ? abstol2 : 0.0);
  __syncthreads();
  for (int sl = 0; sl < 4; ++sl) {      // (slot 3: the rows that stayed)
    double a = 0.0;
    for (int i = threadIdx.x; i < (int)G0; i += BLOCK) a += pg::load_partial(partials + (size_t)sl * G0 + i);
    const double sum = block_sum(a, s_red);
    if (threadIdx.x == 0) sc[pg::S_RED0 + sl] = sum;
  }
  if (threadIdx.x == 0) {
    pg::derive(pg::PH_INIT, sc);
    // (every block's atomicMax on the flag was drained before it drew its ticket)
    sc[pg::S_MOVED] = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == stamp ? 1.0 : 0.0;
    const double held = sc[pg::S_RED0 + 3];
    if (held > 0.0) {
      if (2.0 * held >= sc[pg::S_TOL2]) sc[pg::S_MOVED] = 1.0;
      else {
        sc[pg::S_HELD] = held;
        sc[pg::S_TOL2] -= held;
        sc[pg::S_DONE] = sc[pg::S_RR] <= sc[pg::S_TOL2] ? 1.0 : 0.0;
      }
    }
    if (KH > 0) *g.count += (double)ku;
  }
}

__global__ __launch_bounds__(BLOCK) void k_guess_fit(i64 n, const int* __restrict__ cmap, const double* __restrict__ ds,
                                                     const double* __restrict__ b, const double* __restrict__ yn,
                                                     const double* __restrict__ rhat, GuessFit f) {
  constexpr int RM = GUESS_RM, NS = GUESS_NS;
  __shared__ double s_red[BLOCK / 64];
  __shared__ double s_g[NS];
  double gs[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) gs[j] = 0.0;
  const i64 nchunk = (n + BLOCK - 1) / BLOCK;
  for (i64 ch = (i64)blockIdx.x * f.stride; ch < nchunk; ch += (i64)gridDim.x * f.stride) {
    const i64 i = ch * BLOCK + threadIdx.x;
    const int c = i < n ? (cmap ? cmap[i] : (int)i) : -1;   // (no map: every row is in the loop)
    if (c < 0) continue;
    const double d = ds[i], w = d * d, y0 = yn[i], ru = b[i] - y0, ra = rhat[c];
    double q[RM];
#pragma unroll
    for (int j = 0; j < RM; ++j) q[j] = j < f.avail ? f.yr[j][i] - y0 : 0.0;
    int t = 0;
#pragma unroll
    for (int j = 0; j < RM; ++j)
#pragma unroll
      for (int l = j; l < RM; ++l) gs[t++] += w * q[j] * q[l];
#pragma unroll
    for (int j = 0; j < RM; ++j) gs[t++] += w * q[j] * ru;
    gs[t++] += w * ru * ru;
    gs[t] += w * ra * ra;
  }
  {
    __shared__ double s_w[BLOCK / 64][NS];     // all the sums through one barrier
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // (the shuffle tree level by level over all the sums: NS independent shuffles in flight instead of one chain each)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int j = 0; j < NS; ++j) gs[j] += __shfl_down(gs[j], off, 64);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < NS; ++j) s_w[wave][j] = gs[j];
    }
    __syncthreads();
    if (threadIdx.x < NS) {
      double a = 0.0;
#pragma unroll
      for (int q = 0; q < BLOCK / 64; ++q) a += s_w[q][threadIdx.x];
      pg::store_partial(f.partials + (size_t)threadIdx.x * gridDim.x + blockIdx.x, a);
    }
  }
  if (!pg::last_block_arrives(f.ticket, gridDim.x, s_red)) return;
  guess_fit_last(f, (int)gridDim.x, s_g);
}

__global__ __launch_bounds__(BLOCK) void k_guess_decide(GuessFit f) {
  __shared__ double s_g[GUESS_NS];
  if (threadIdx.x < GUESS_NS) s_g[threadIdx.x] = f.sums[threadIdx.x];
  __syncthreads();
  guess_decide(s_g, f);
}

// z refers to S_old: re-express it with S_new (x = S_old z = S_new z')
__global__ void k_rescale_state(i64 n, const double* __restrict__ ds_old, const double* __restrict__ ds_new,
                                double* __restrict__ z) {
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x)
    z[r] = (ds_old[r] * z[r]) / ds_new[r];
}

__global__ void k_scale_state(i64 n, const double* __restrict__ ds, const double* __restrict__ in, double* __restrict__ out,
                              int divide) {
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x)
    out[r] = divide ? in[r] / ds[r] : in[r] * ds[r];
}

// K8, constructor form: T0 and K*T0 live in the padded layout (T0 may be non-zero at eliminated unknowns)
__global__ void k_rhs_first(RowSegs seg, i64 n, i64 Mloc, int scheme, const int* row_cell, const double* T0pad,
                            const double* ypad, const double* mass, const double* bconst,
                            const unsigned char* fixed, double* braw, double* x0, int moving) {
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) {
    const int k = seg_kind(seg, r);
    const i64 q = (i64)k * Mloc + row_cell[r];
    const double T = T0pad[q];
    double v;
    if (fixed[r]) v = bconst[r];
    else if (moving && (k & 1)) v = bconst[r];                                        // b2 = Γ g
    else if (moving && ypad) v = mass[r] * T - ypad[q] + bconst[r];   // CN: (Vn - Id GᵀWꜝGΨn)Tω - ½Id GᵀWꜝH Tγ + ...;
                                                                     // advection-diffusion: - the explicit convection too
    else if (scheme == PG_SCHEME_CN) v = 2.0 * (mass[r] * T) - ypad[q] + bconst[r];
    else v = mass[r] * T + bconst[r];
    braw[r] = v;
    x0[r] = T;
  }
}

// Ψn1 = psip.(Vn, Vn_1), Ψn = psim.(Vn, Vn_1)      prescribedmotionsolver/diffusion.jl:55-98 (the live definitions)
// and, for the advection-diffusion solvers (psicp != nullptr), psip_conv / psim_conv     advectiondiffusion.jl:35-61
__global__ void k_psi(i64 Mloc, int scheme, const double* __restrict__ vn_1 /*lower face*/, const double* __restrict__ vn,
                      double* __restrict__ psip, double* __restrict__ psim, double* __restrict__ psicp,
                      double* __restrict__ psicm) {
  for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < Mloc; i += (i64)gridDim.x * blockDim.x) {
    const bool z1 = vn[i] == 0.0, z2 = vn_1[i] == 0.0;   // args = (Vn, Vn_1)
    double pp, pm;
    if (scheme == PG_SCHEME_CN) {
      pp = (z1 && z2) ? 0.0 : (!z1 && !z2) ? 0.5 : (z1 && !z2) ? 0.5 : 1.0;   // psip_cn
      pm = (z1 && z2) ? 0.0 : (!z1 && !z2) ? 0.5 : (z1 && !z2) ? 0.5 : 0.0;   // psim_cn
    } else {
      pp = (z1 && z2) ? 0.0 : 1.0;                                            // psip_be
      pm = 0.0;                                                               // psim_be
    }
    psip[i] = pp;
    psim[i] = pm;
    if (psicp) {
      psicp[i] = (z1 && !z2) ? 1.0 : 0.0;                                     // psip_conv: 1 only for (Vn = 0, Vn_1 ≠ 0)
      psicm[i] = (!z1 && !z2) || (!z1 && z2) ? 1.0 : 0.0;                     // psim_conv: both live, or (Vn ≠ 0, Vn_1 = 0)
    }
  }
}

// K12: padded[k*Mloc + cell] = x[r]
__global__ void k_scatter_active(RowSegs seg, i64 n, i64 Mloc, const int* row_cell, const double* x, double* padded) {
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) {
    const int k = seg_kind(seg, r);
    padded[(i64)k * Mloc + row_cell[r]] = x[r];
  }
}

__global__ void k_maxabs(i64 n, const double* x, const double* ds /*NULL: x is unscaled*/, double* partials) {
  __shared__ double sh[BLOCK];
  double m = 0.0;
  for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    const double a = fabs(ds ? ds[i] * x[i] : x[i]);
    m = a > m ? a : m;
  }
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] > sh[threadIdx.x + s] ? sh[threadIdx.x] : sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

// The Stefan terms of a solved 1-D space-time slab, per phase    liquidmotionsolver/diffusion.jl:240-255, height_tracking.jl:23-31
//   Σ A_t(t0) ("Hₙ₊₁", Vn_1), Σ A_t(t1) ("Hₙ", Vn), Σᵢ qᵢ, maxᵢ |qᵢ|,   q = Id Hᵀ Wꜝ (G Tω + H Tγ)
// q_i is row i of the monophasic interface rows [HᵀWꜝG, HᵀWꜝH] (eval_row, Iᵦ = 1, Iₐ = 0, no Ψ) applied to the padded state and
// scaled by Id_i.  Fixed-order reduction (no atomics): wave64 shuffles, the block's waves in order, then k_stefan_final over the
// blocks in order -- the same state gives bitwise the same numbers (the Newton loop branches on them).
constexpr int STEFAN_OUT = 8;        // 4 per phase
constexpr int STEFAN_BLOCKS = 64;    // most partial rows (grid depends on Mloc only)
struct StefanArgs {
  SysParams P[2];                    // mono interface-row parameters of each phase's capacity
  const double* v0[2];
  const double* v1[2];
  const double* Id[2];               // D(C_ω), or nullptr (= 1)
  const int* red;                    // K*Mloc: reduced index of (kind, cell), -1 = eliminated (T = 0 there)
  const double* x;                   // reduced state: unscaled x (ds == nullptr) or z with x = S z
  const double* ds;
  const double* Tpad;                // != nullptr: an unsolved slab, T = the padded state it was built from (K*Mloc)
  i64 Mloc;
  int nphase;
};

__global__ __launch_bounds__(BLOCK) void k_stefan_partials(StefanArgs a, double* __restrict__ partials) {
  double acc[STEFAN_OUT];
#pragma unroll
  for (int j = 0; j < STEFAN_OUT; ++j) acc[j] = 0.0;
  const CapView& c = a.P[0].cap[0];
  for (i64 lc = blockIdx.x * (i64)blockDim.x + threadIdx.x; lc < a.Mloc; lc += (i64)gridDim.x * blockDim.x) {
    i64 idx[3];
    decode_cell(c.N, c.ext, c.plane, c.s0, lc, idx);
    for (int ph = 0; ph < a.nphase; ++ph) {
      const int* red = a.red + (i64)(2 * ph) * a.Mloc;
      double row = 0.0;
      eval_row(a.P[ph], 1, lc, idx, [&](int k, i64 col, double v) {
        const i64 q = (i64)k * a.Mloc + col;
        if (a.Tpad) {
          row += v * a.Tpad[(i64)(2 * ph) * a.Mloc + q];
        } else {
          const int r = red[q];
          if (r >= 0) row += v * (a.ds ? a.ds[r] * a.x[r] : a.x[r]);
        }
      });
      const double q = (a.Id[ph] ? a.Id[ph][lc] : 1.0) * row;
      acc[4 * ph + 0] += a.v0[ph][lc];
      acc[4 * ph + 1] += a.v1[ph][lc];
      acc[4 * ph + 2] += q;
      acc[4 * ph + 3] = fmax(acc[4 * ph + 3], fabs(q));
    }
  }
#pragma unroll
  for (int j = 0; j < STEFAN_OUT; ++j)
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_down(acc[j], off, 64);
      acc[j] = (j & 3) == 3 ? fmax(acc[j], o) : acc[j] + o;
    }
  __shared__ double sh[BLOCK / 64][STEFAN_OUT];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0)
#pragma unroll
    for (int j = 0; j < STEFAN_OUT; ++j) sh[wave][j] = acc[j];
  __syncthreads();
  if (threadIdx.x < STEFAN_OUT) {
    const int j = threadIdx.x;
    double v = sh[0][j];
    for (int w = 1; w < BLOCK / 64; ++w) v = (j & 3) == 3 ? fmax(v, sh[w][j]) : v + sh[w][j];
    partials[(i64)blockIdx.x * STEFAN_OUT + j] = v;
  }
}

__global__ void k_stefan_final(const double* __restrict__ partials, int nblk, double* __restrict__ out) {
  if (threadIdx.x < STEFAN_OUT) {
    const int j = threadIdx.x;
    double v = partials[j];
    for (int b = 1; b < nblk; ++b) v = (j & 3) == 3 ? fmax(v, partials[(i64)b * STEFAN_OUT + j]) : v + partials[(i64)b * STEFAN_OUT + j];
    out[j] = v;
  }
}

__global__ void k_set_border_values(i64 nb, const i64* cells_global, const double* values, i64 first_cell, i64 Mloc,
                                    int nbulk, const int* red, i64 n_own, double* bcv) {
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < nb; q += (i64)gridDim.x * blockDim.x) {
    const i64 lc = cells_global[q] - first_cell;
    if (lc < 0 || lc >= Mloc) continue;
    for (int ph = 0; ph < nbulk; ++ph) {
      const int r = red[(i64)(2 * ph) * Mloc + lc];
      if (r >= 0 && r < n_own) bcv[r] = values[q];
    }
  }
}

// ---- time-separable data: mode builders and the per-step combine ----------------------------------------------------------
// the row-space response to unit data φ (a padded field) of a source (which = PG_TD_SOURCE: V φ on the bulk rows of `phase`
// that are not fixed) or of the monophasic interface value (PG_TD_INTERFACE: Γ φ on the interface rows); zero on every other
// row.  k_bconst multiplies the same products by the scheme's factor.
__global__ void k_td_mode(SysParams P, RowSegs seg, i64 n_own, const int* row_cell, int which, int phase,
                          const double* __restrict__ phi, const unsigned char* __restrict__ fixed, double* __restrict__ mode) {
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n_own; r += (i64)gridDim.x * blockDim.x) {
    const int k = seg_kind(seg, r);
    const i64 lc = row_cell[r];
    double v = 0.0;
    if (which == PG_TD_SOURCE) {
      if ((k & 1) == 0 && (k >> 1) == phase && !fixed[r]) v = P.cap[phase].V[lc] * phi[lc];
    } else if ((k & 1) == 1 && P.nphase == 1) {
      v = P.cap[0].G[lc] * phi[lc];
    }
    mode[r] = v;
  }
}

// the fixed rows of the border cells, as k_set_border_values finds them: out[r] = values[q] (values == nullptr: 0)
__global__ void k_td_border_rows(i64 nb, const i64* cells_global, const double* values, i64 first_cell, i64 Mloc, int nbulk,
                                 const int* red, i64 n_own, const unsigned char* fixed, double* out) {
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < nb; q += (i64)gridDim.x * blockDim.x) {
    const i64 lc = cells_global[q] - first_cell;
    if (lc < 0 || lc >= Mloc) continue;
    for (int ph = 0; ph < nbulk; ++ph) {
      const int r = red[(i64)(2 * ph) * Mloc + lc];
      if (r >= 0 && r < n_own && fixed[r]) out[r] = values ? values[q] : 0.0;
    }
  }
}

// ---- device functions: the list of the rows that carry a slot's data (built once per installed program) --------------------
// item i of a source / interface slot is row i; item i of the border slot is (border cell i / nbulk, phase i % nbulk)
struct TdPointsArgs {
  int which, phase, nbulk, N;
  i64 n_items, n_own, first_cell, Mloc;
  const int* row_cell;
  const int* red;
  const unsigned char* fixed;
  const i64* cells_global;         // border: global linear index of each border cell
  const unsigned char* selected;   // border: 1 for the cells of the program's key(s)
  const double* weight;            // V (source) / Γ (interface) by local cell; border: none (1)
  const double* pos[3];            // C_ω / C_γ by local cell (source / interface), the cell centres by border cell (border)
};

// the row of item i, or -1 when the item carries no data of the slot -- the rows and weights of k_td_mode and k_td_border_rows
__device__ inline i64 td_item_row(const TdPointsArgs& a, const RowSegs& seg, i64 i, i64* src) {
  if (a.which == PG_TD_BORDER) {
    const i64 q = i / a.nbulk;
    const int ph = (int)(i % a.nbulk);
    *src = q;
    if (!a.selected[q]) return -1;
    const i64 lc = a.cells_global[q] - a.first_cell;
    if (lc < 0 || lc >= a.Mloc) return -1;
    const int r = a.red[(i64)(2 * ph) * a.Mloc + lc];
    return (r >= 0 && r < a.n_own && a.fixed[r]) ? r : -1;
  }
  const int k = seg_kind(seg, i);
  *src = a.row_cell[i];
  if (a.which == PG_TD_SOURCE) return ((k & 1) == 0 && (k >> 1) == a.phase && !a.fixed[i]) ? i : -1;
  return (k & 1) == 1 ? i : -1;
}

__global__ void k_td_points_flag(TdPointsArgs a, RowSegs seg, unsigned char* __restrict__ flag) {
  for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < a.n_items; i += (i64)gridDim.x * blockDim.x) {
    i64 src;
    flag[i] = td_item_row(a, seg, i, &src) >= 0 ? 1 : 0;
  }
}

// k_td_points: the flagged items in their order, compact: (row, weight, p0, p1, p2), coordinates the problem lacks as 0.0
__global__ void k_td_points(TdPointsArgs a, RowSegs seg, const int* __restrict__ where, i64 n_list, int* __restrict__ row,
                            double* __restrict__ w, double* __restrict__ p0, double* __restrict__ p1, double* __restrict__ p2) {
  for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < a.n_items; i += (i64)gridDim.x * blockDim.x) {
    i64 src;
    const i64 r = td_item_row(a, seg, i, &src);
    if (r < 0) continue;
    const i64 e = where[i];
    if (e < 0 || e >= n_list) continue;        // (cannot happen: the list has the scan's total)
    row[e] = (int)r;
    w[e] = a.weight ? a.weight[src] : 1.0;
    p0[e] = a.pos[0] ? a.pos[0][src] : 0.0;
    p1[e] = a.pos[1] ? a.pos[1][src] : 0.0;
    p2[e] = a.pos[2] ? a.pos[2][src] : 0.0;
  }
}

__global__ void k_td_zero_rows(i64 n, const int* __restrict__ row, double* __restrict__ out) {
  for (i64 e = blockIdx.x * (i64)blockDim.x + threadIdx.x; e < n; e += (i64)gridDim.x * blockDim.x) out[row[e]] = 0.0;
}

struct TdTerms {
  const double* m[PG_TD_MAX_TERMS];
  double c[PG_TD_MAX_TERMS];
};

// out = base + Σ_{j<J} c_j mode_j, the sum taken in the order of j: (J + 2) · 8 · n bytes streamed, 16 bytes per access, the
// coefficients by value in the launch (nothing is read back), no atomics, no LDS -- bitwise reproducible.  base may be out
// itself (the second and later launches of more than PG_TD_MAX_TERMS modes): every element is read and written by one thread.
template <int J>
__global__ __launch_bounds__(256) void k_td_combine(i64 n, const double* base, TdTerms T, double* out) {
  const i64 n2 = n >> 1;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n2; i += stride) {
    rd2_t v = reinterpret_cast<const rd2_t*>(base)[i];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const rd2_t m = __builtin_nontemporal_load(reinterpret_cast<const rd2_t*>(T.m[j]) + i);
      v.x += T.c[j] * m.x;
      v.y += T.c[j] * m.y;
    }
    reinterpret_cast<rd2_t*>(out)[i] = v;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last row
    double v = base[n - 1];
#pragma unroll
    for (int j = 0; j < J; ++j) v += T.c[j] * T.m[j][n - 1];
    out[n - 1] = v;
  }
}

// ---- monitors: weighted sums of the state after every completed solve ------------------------------------------------------
// One launch per solve evaluates all K monitors.  The state is read where it lives -- x, or z with x = S z (ds != nullptr) --
// and never written.  Dense monitors share ONE sweep over the rows: block b owns the rows [b·chunk, (b+1)·chunk) (chunk even, so
// every pair load is 16 bytes wide and aligned), lane l the pairs l, l + 256, ... of that range, one accumulator per monitor in
// registers.  Sparse monitors follow in the same launch as gathers: entry e belongs to thread e mod (G·256).  Every
// accumulator is reduced over its wave by shuffles, the block's four waves are added in order through LDS, and the block's K
// sums go to out[b·K .. b·K + K): no atomics, nothing handed from block to block, an order of summation that depends on
// (n, chunk, G) alone.  Bytes per launch: 16·n (z and ds; 8·n when x is valid) once if any monitor is dense, 8·n per dense
// monitor, 12 bytes and two gathered words per sparse entry, G·K·8 written.
constexpr int MON_ROWS_PER_BLOCK = 2 * BLOCK;   // one pair per lane at the sizes where the launch is all latency
constexpr int MON_MAX_BLOCKS = 1024;            // 4 blocks per CU: 16-byte loads from 256 K lanes keep HBM busy
struct MonArgs {
  const double* w[PG_MON_MAX];
  const int* row[PG_MON_MAX];     // nullptr: a dense monitor
  i64 cnt[PG_MON_MAX];            // entries of a sparse monitor
  int kind[PG_MON_MAX];
  int dense[PG_MON_MAX];          // the dense monitors, in order
  int K;
};

__device__ inline double mon_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

template <int ND>
__global__ __launch_bounds__(BLOCK) void k_monitor(i64 n, i64 chunk, const double* __restrict__ x, const double* __restrict__ ds,
                                                   MonArgs a, double* __restrict__ out) {
  __shared__ double sh[PG_MON_MAX][BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (ND > 0) {
    double acc[ND > 0 ? ND : 1];
#pragma unroll
    for (int j = 0; j < ND; ++j) acc[j] = 0.0;
    const i64 r0 = blockIdx.x * chunk;
    const i64 r1 = r0 + chunk < n ? r0 + chunk : n;
    for (i64 i = r0 + 2 * (i64)threadIdx.x; i + 1 < r1; i += 2 * BLOCK) {
      rd2_t v = *reinterpret_cast<const rd2_t*>(x + i);
      if (ds) {
        const rd2_t d = *reinterpret_cast<const rd2_t*>(ds + i);
        v.x *= d.x;
        v.y *= d.y;
      }
      const rd2_t q = {v.x * v.x, v.y * v.y};
#pragma unroll
      for (int j = 0; j < ND; ++j) {
        const int m = a.dense[j];
        const rd2_t wv = __builtin_nontemporal_load(reinterpret_cast<const rd2_t*>(a.w[m] + i));
        const bool sq = a.kind[m] == PG_MON_SUMSQ;
        acc[j] += wv.x * (sq ? q.x : v.x);
        acc[j] += wv.y * (sq ? q.y : v.y);
      }
    }
    if (((r1 - r0) & 1) && r1 > r0 && threadIdx.x == 0) {   // the odd last row (of the last block: chunk is even)
      const i64 i = r1 - 1;
      const double v = ds ? ds[i] * x[i] : x[i];
#pragma unroll
      for (int j = 0; j < ND; ++j) {
        const int m = a.dense[j];
        acc[j] += a.w[m][i] * (a.kind[m] == PG_MON_SUMSQ ? v * v : v);
      }
    }
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      const double v = mon_wave_sum(acc[j]);
      if (lane == 0) sh[a.dense[j]][wave] = v;
    }
  }
  for (int m = 0; m < a.K; ++m) {
    if (!a.row[m]) continue;
    double acc = 0.0;
    for (i64 e = blockIdx.x * (i64)BLOCK + threadIdx.x; e < a.cnt[m]; e += (i64)gridDim.x * BLOCK) {
      const int r = a.row[m][e];
      const double v = ds ? ds[r] * x[r] : x[r];
      acc += a.w[m][e] * (a.kind[m] == PG_MON_SUMSQ ? v * v : v);
    }
    acc = mon_wave_sum(acc);
    if (lane == 0) sh[m][wave] = acc;
  }
  __syncthreads();
  if ((int)threadIdx.x < a.K) {
    double v = sh[threadIdx.x][0];
#pragma unroll
    for (int wv = 1; wv < BLOCK / 64; ++wv) v += sh[threadIdx.x][wv];
    out[(i64)blockIdx.x * a.K + threadIdx.x] = v;
  }
}

SysParams make_params(const pg_solver* s, int scheme) {
  SysParams P;
  std::memset(&P, 0, sizeof(P));
  P.nphase = s->nphase;
  for (int q = 0; q < s->nphase; ++q) {
    P.cap[q] = cap_view(s->cap[q]);
    P.ct[q] = s->cap[q]->ct.p;
    P.Id[q] = s->Id[q].p;
    if (s->ops[q] && s->ops[q]->has_velocity) {
      for (int d = 0; d < s->cap[q]->N; ++d) P.conv_a[q][d] = s->ops[q]->conv_a[d].p;
      P.conv_k[q] = s->ops[q]->conv_k.p;
    }
  }
  if (s->nphase == 1) { P.cap[1] = P.cap[0]; P.ct[1] = P.ct[0]; P.Id[1] = nullptr; }
  // steady (diffusion.jl:30-43): the unsteady BE blocks with Δt = 1 and without the V term
  const double th = scheme == PG_SCHEME_CN ? s->dt / 2 : s->dt;
  P.theta = th;
  P.gscale = scheme == PG_SCHEME_CN ? s->dt / 2 : 1.0;
  P.mass = scheme == PG_SCHEME_STEADY ? 0.0 : 1.0;
  if (s->nphase == 1) {
    switch (s->bc_i.kind) {     // build_I_bc, solver.jl:203-223
      case PG_BC_DIRICHLET: P.Ia = 1.0; P.Ib = 0.0; break;
      case PG_BC_NEUMANN: P.Ia = 0.0; P.Ib = 1.0; break;
      case PG_BC_ROBIN: P.Ia = s->bc_i.alpha; P.Ib = s->bc_i.beta; break;
      default: P.Ia = 0.0; P.Ib = 0.0; break;
    }
  } else {
    P.a1 = s->ic.alpha1; P.a2 = s->ic.alpha2; P.b1 = s->ic.beta1; P.b2 = s->ic.beta2;
  }
  for (int k = 0; k < 6; ++k) P.border_kind[k] = s->border_kind[k];
  P.inv_dx = s->inv_dx;
  P.border_both_phases = (s->moving && s->nphase == 2) ? 1 : 0;
  if (s->moving) {            // Δt lives inside the space-time capacities
    P.theta = 1.0;
    P.gscale = 1.0;
    P.mass = 1.0;
    for (int q = 0; q < s->nphase; ++q) {
      P.mv_v0[q] = s->cap[q]->Vt[0].p;
      P.mv_v1[q] = s->cap[q]->Vt[1].p;
      P.mv_psi_w[q] = s->psi_p[q].p;
      P.mv_psi_g[q] = s->psi_p[q].p;
    }
    if (s->nphase == 1) { P.mv_v0[1] = P.mv_v0[0]; P.mv_v1[1] = P.mv_v1[0]; P.mv_psi_w[1] = P.mv_psi_w[0]; P.mv_psi_g[1] = P.mv_psi_g[0]; }
    if (s->advdiff) {         // A: - (sum(C) + ½K[1]) Ψ_conv, - ½K[1] Ψ_conv   (advectiondiffusion.jl:123-124, 357-360)
      P.mv_conv_sign = -1.0;
      for (int q = 0; q < 2; ++q) {
        const int src = q < s->nphase ? q : 0;
        P.mv_psi_c[q] = P.mv_psi_k[q] = P.mv_psi_kg[q] = s->psi_cp[src].p;
      }
      P.mv_flux_no_dv = s->nphase == 2 ? 1 : 0;   // :362-365: no -(Vn_1 - Vn) in the flux row
    }
    P.mv_stefan = s->stefan ? 1 : 0;
  }
  return P;
}

// the explicit operator of the moving Crank-Nicolson right-hand side (diffusion.jl:214); advection-diffusion: the explicit
// operator of either scheme, convection included (advectiondiffusion.jl:192-194, 494-498):
//   BE        b1 = Vn Tω + V f - ½K Ψc Tω - ½K Tγ - ΣC Ψc Tω                      Ψc = psim_conv, no diffusion term
//   CN mono   b1 = (Vn - Id GᵀWꜝG Ψn) Tω - ½Id GᵀWꜝH Tγ + .. - ½K Ψn Tω - ½K Tγ - ΣC Tω      Ψn = psim
//   CN diph   b1 = (Vn - Id GᵀWꜝG Ψn) Tω - ½Id GᵀWꜝH Tγ + .. - ΣC Tω - ½K Tω - ½K Tγ    (no Ψ on the γ term either)
SysParams make_params_moving_explicit(const pg_solver* s) {
  SysParams P = make_params(s, PG_SCHEME_CN);
  const bool cn = s->scheme_ctor == PG_SCHEME_CN;
  for (int q = 0; q < 2; ++q) {
    const int src = q < s->nphase ? q : 0;
    P.mv_psi_w[q] = s->psi_m[src].p;
    // mono (:214): the γ term is -½ Id GᵀWꜝH Tγ; diph (:487-488): -Id GᵀWꜝH Ψn Tγ with the same Ψn = psim as the ω term
    P.mv_psi_g[q] = s->nphase == 2 ? s->psi_m[src].p : nullptr;
    if (s->stefan) P.mv_psi_g[q] = nullptr;                      // Stefan CN (:637-638): -½ Id GᵀWꜝH Tγ, no Ψ
    if (s->advdiff) {
      P.mv_psi_g[q] = cn ? nullptr : s->psi_m[src].p;            // CN: the constant ½; BE: psim_be = 0, no diffusion term
      P.mv_psi_c[q] = cn ? nullptr : s->psi_cm[src].p;
      P.mv_psi_k[q] = cn ? (s->nphase == 1 ? s->psi_m[src].p : nullptr) : s->psi_cm[src].p;
      P.mv_psi_kg[q] = nullptr;
    }
  }
  if (s->advdiff) {
    P.mv_conv_sign = 1.0;
    P.mv_flux_no_dv = 0;   // (interface rows are empty in the explicit operator)
  }
  P.mv_gconst = 0.5;
  P.mv_explicit = 1;
  return P;
}

void upload_local(DevBuf<double>& dst, const double* host_global, const Slab& slab) {
  dst.alloc(slab.Mloc());
  dst.upload(host_global + slab.first_cell(), slab.Mloc());
}

SrcView src_view(const pg_solver* s) {
  SrcView v;
  for (int q = 0; q < 2; ++q) { v.f_n[q] = s->f_n[q].p; v.f_np1[q] = s->f_np1[q].p; }
  if (s->nphase == 1) {
    v.g_n = s->g_n.p; v.g_np1 = s->g_np1.p;
    v.g_const = s->bc_i.value; v.h_const = 0.0;
  } else {
    v.g_n = s->g_arr.p; v.g_np1 = s->h_arr.p;
    v.g_const = s->ic.g; v.h_const = s->ic.h;
  }
  return v;
}

bool td_installed(const pg_solver* s) {
  for (const auto& t : s->td)
    if (!t.empty()) return true;
  return false;
}

void td_clear(pg_solver* s, int slot) {
  pg_solver::TdSlot& t = s->td[slot];
  if (t.empty()) return;
  for (auto& m : t.mode) m.release();
  t.progs.clear();
  t.K = 0;
  t.nrows = 0;
  t.coef.clear();
  s->bconst_dirty = true;            // bconst is k_bconst's again (or a td_base with this slot's own data back in it)
  if (!td_installed(s)) {
    s->td_base.release();
    s->td_base_scheme = -1;
    s->td_cursor = 0;
    s->td_row = -1;
  }
}

// global linear index of every border cell in the mesh's order, on the device (uploaded on first use); returns their count
i64 ensure_border_cells(pg_solver* s) {
  pg_mesh* m = s->cap[0]->mesh;
  mesh_build_border(m);
  const i64 nb = (i64)m->border_key.size();
  if (!s->border_cells_lin.p) {
    std::vector<i64> lin(nb);
    for (i64 q = 0; q < nb; ++q) {
      i64 li = 0;
      for (int d = 0; d < m->N; ++d) li += (m->border_idx[q * m->N + d] - 1) * s->slab.stride[d];
      lin[q] = li;
    }
    s->border_cells_lin.alloc(nb);
    s->border_cells_lin.upload(lin.data(), nb);
  }
  return nb;
}

// bconst of the step whose table row is s->td_row: td_base (k_bconst with the separable slots empty, rebuilt when other data or
// the scheme changed) + Σ_j c_j mode_j.  The factor k_bconst would put on the data is put on the coefficient:
//   source      BE: Δt a(t+Δt)        CN: Δt/2 (a(t) + a(t+Δt))          diffusion.jl:257-261
//   interface   BE: a(t+Δt)           CN: Δt/2 (a(t) + a(t+Δt))
//   border      a(t)                                                      (the loop applies the border rows with t, :292)
void td_bconst(pg_solver* s, int scheme) {
  hipStream_t st = ctx().stream;
  const i64 n = s->nb.n_own;
  if (n > 0 && (s->bconst_dirty || s->td_base_scheme != scheme || s->td_base.n != n)) {
    if (s->td_base.n != n) s->td_base.alloc(n);
    SrcView v = src_view(s);
    for (int q = 0; q < 2; ++q)
      if (!s->td[q].empty()) v.f_n[q] = v.f_np1[q] = nullptr;
    if (!s->td[2].empty()) { v.g_n = v.g_np1 = nullptr; v.g_const = 0.0; }
    hipLaunchKernelGGL(k_bconst, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, st, make_params(s, scheme), make_segs(s->nb), n,
                       s->nb.row_cell.p, v, scheme, s->dt, s->fixed.p, s->bcv.p, s->td_base.p, 0);
    PG_HIP(hipGetLastError());
    if (s->td[3].K > 0) {
      const i64 nb = ensure_border_cells(s);
      if (nb > 0)
        hipLaunchKernelGGL(k_td_border_rows, dim3(grid_for(nb, BLOCK)), dim3(BLOCK), 0, st, nb, s->border_cells_lin.p,
                           (const double*)nullptr, s->slab.first_cell(), s->Mloc, s->nphase, s->nb.red.p, n, s->fixed.p,
                           s->td_base.p);
      PG_HIP(hipGetLastError());
    }
    for (const auto& pr : s->td[3].progs) {      // a border program's rows: its value alone, the others keep what bcv holds
      if (pr.n <= 0) continue;
      hipLaunchKernelGGL(k_td_zero_rows, dim3(grid_for(pr.n, BLOCK)), dim3(BLOCK), 0, st, pr.n, pr.row.p, s->td_base.p);
      PG_HIP(hipGetLastError());
    }
  }
  s->td_base_scheme = scheme;
  const bool cn = scheme == PG_SCHEME_CN;
  TdTerms T{};
  int J = 0;
  const double* base = s->td_base.p;
  auto flush = [&]() {
    if (J == 0 || n <= 0) return;
    const int grid = grid_for((n + 1) / 2, BLOCK);
    switch (J) {
#define PG_TD_COMBINE(JV) \
  case JV: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_td_combine<JV>), dim3(grid), dim3(BLOCK), 0, st, n, base, T, s->bconst.p); break;
      PG_TD_COMBINE(1) PG_TD_COMBINE(2) PG_TD_COMBINE(3) PG_TD_COMBINE(4)
      PG_TD_COMBINE(5) PG_TD_COMBINE(6) PG_TD_COMBINE(7) PG_TD_COMBINE(8)
#undef PG_TD_COMBINE
    }
    PG_HIP(hipGetLastError());
    base = s->bconst.p;
    J = 0;
  };
  for (int slot = 0; slot < 4; ++slot) {
    const pg_solver::TdSlot& t = s->td[slot];
    if (t.K == 0) continue;
    PG_REQUIRE(s->td_row >= 0 && s->td_row < t.nrows, "time-separable data: no table row for this right-hand side");
    const double* c0 = t.coef.data() + (size_t)s->td_row * 2 * t.K;
    const double* c1 = c0 + t.K;
    for (int k = 0; k < t.K; ++k) {
      double c;
      if (slot == 3) c = c0[k];
      else if (cn) c = s->dt / 2 * (c0[k] + c1[k]);
      else c = slot == 2 ? c1[k] : s->dt * c1[k];
      T.m[J] = t.mode[k].p;
      T.c[J] = c;
      if (++J == PG_TD_MAX_TERMS) flush();
    }
  }
  flush();
  // device functions: bconst = base (+ separable terms), then every program adds its own rows, slot after slot
  bool any_prog = false;
  for (const auto& t : s->td) any_prog = any_prog || !t.progs.empty();
  if (!any_prog) return;
  if (base != s->bconst.p && n > 0)
    PG_HIP(hipMemcpyAsync(s->bconst.p, s->td_base.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
  for (int slot = 0; slot < 4; ++slot)
    for (const auto& pr : s->td[slot].progs) {
      PG_REQUIRE(s->td_row >= 0 && s->td_row < pr.nrows, "device function: no table row for this right-hand side");
      const double t0 = pr.times[(size_t)2 * s->td_row], t1 = pr.times[(size_t)2 * s->td_row + 1];
      double c0, c1;
      if (slot == 3) { c0 = 0.0; c1 = 1.0; }
      else if (cn) c0 = c1 = s->dt / 2;
      else { c0 = 0.0; c1 = slot == 2 ? 1.0 : s->dt; }
      td_eval_launch(pr.prog, pr.n, pr.row.p, pr.w.p, pr.p[0].p, pr.p[1].p, pr.p[2].p, c0, c1, t0, slot == 3 ? t0 : t1,
                     s->bconst.p, st);
    }
}

void ensure_bconst(pg_solver* s, int scheme) {
  if (td_installed(s)) {               // every step has its own data: combined anew, and counted as changed data
    td_bconst(s, scheme);
    s->bconst_scheme = scheme;
    s->bconst_dirty = false;
    ++s->bconst_version;
    return;
  }
  if (!s->bconst_dirty && s->bconst_scheme == scheme) return;
  hipStream_t st = ctx().stream;
  const i64 n = s->nb.n_own;
  if (n > 0) {
    const SysParams P = make_params(s, scheme);
    hipLaunchKernelGGL(k_bconst, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, st, P, make_segs(s->nb), n, s->nb.row_cell.p,
                       src_view(s), scheme, s->dt, s->fixed.p, s->bcv.p, s->bconst.p, s->moving ? 1 : 0);
    PG_HIP(hipGetLastError());
  }
  s->bconst_scheme = scheme;
  s->bconst_dirty = false;
  ++s->bconst_version;
}

// first right-hand side: b(t = 0) with the constructor scheme (diffusion.jl:202/205, 328); re-run when the host
// supplies per-cell data after construction but before the first solve
void build_first_rhs(pg_solver* s) {
  hipStream_t st = ctx().stream;
  const i64 n = s->nb.n_own;
  const SysParams P = make_params(s, s->scheme_ctor);
  ensure_bconst(s, s->scheme_ctor);
  DevBuf<double> ypad;
  if (s->scheme_ctor == PG_SCHEME_CN || s->advdiff) {
    ypad.alloc((i64)s->K * s->Mloc);
    ypad.zero();
    apply_rows_padded(s->moving ? make_params_moving_explicit(s) : P, s->slab, s->T0pad.p, ypad.p);
  }
  if (n > 0) {
    DevBuf<double> braw(n);
    hipLaunchKernelGGL(k_rhs_first, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, st, make_segs(s->nb), n, s->Mloc,
                       s->scheme_ctor, s->nb.row_cell.p, s->T0pad.p, ypad.p, s->mass.p, s->bconst.p, s->fixed.p, braw.p,
                       s->x.p, s->moving ? 1 : 0);
    PG_HIP(hipGetLastError());
    apply_left(s->A_ctor, braw.p, s->b.p, st);   // b̂ = B⁻¹ S b
    PG_HIP(hipStreamSynchronize(st));
  }
  PG_HIP(hipStreamSynchronize(st));
}

void materialize_x(pg_solver* s);

void setup_common(pg_solver* s, const pg_border_desc* borders, int nborders, const double* T0) {
  hipStream_t st = ctx().stream;
  const Slab& slab = s->slab;
  s->K = s->nphase == 1 ? 2 : 4;
  s->Mloc = slab.Mloc();
  s->M = slab.M;
  for (int i = 0; i < nborders; ++i) {
    const int key = borders[i].key;
    PG_REQUIRE(key >= 0 && key < 6, "border key out of range");
    const int kind = borders[i].kind;
    PG_REQUIRE(kind == PG_BC_DIRICHLET || kind == PG_BC_PERIODIC || kind == PG_BC_NEUMANN || kind == PG_BC_NONE ||
               kind == PG_BC_ROBIN, "border kind not supported");
    // Robin (and Neumann in >1-D) borders are silently ignored by the reference (solver.jl:450-499)
    s->border_kind[key] = (kind == PG_BC_ROBIN) ? PG_BC_NONE : kind;
    s->border_value[key] = borders[i].value;
  }
  if (slab.N == 1) {
    const auto& nd = s->cap[0]->mesh->nodes[0];
    double dx = 1e300;
    for (size_t i = 1; i < nd.size(); ++i) dx = std::min(dx, nd[i] - nd[i - 1]);
    s->inv_dx = 1.0 / dx;   // solver.jl:476
  }
  if (ctx().nranks > 1)
    for (int k = 0; k < 6; ++k)
      PG_REQUIRE(s->border_kind[k] != PG_BC_PERIODIC, "periodic borders are single-rank only");

  // initial condition, padded local layout
  s->T0pad.alloc((i64)s->K * s->Mloc);
  s->T0pad.zero();   // T0 == NULL: zeros(2M) without a host array (multi-GPU sizes)
  if (T0)
    for (int k = 0; k < s->K; ++k) s->T0pad.upload(T0 + (i64)k * s->M + slab.first_cell(), s->Mloc, (i64)k * s->Mloc);
  if (s->init_from) {     // the previous slab's state, device to device (zeros at its eliminated unknowns, solver.jl:186-187)
    pg_solver* p = s->init_from;
    PG_REQUIRE(p->K == s->K && p->Mloc == s->Mloc && p->M == s->M, "previous solver lives on another mesh");
    materialize_x(p);
    if (p->nb.n_own > 0)
      hipLaunchKernelGGL(k_scatter_active, dim3(grid_for(p->nb.n_own, BLOCK)), dim3(BLOCK), 0, st, make_segs(p->nb), p->nb.n_own,
                         p->Mloc, p->nb.row_cell.p, p->x.p, s->T0pad.p);
    PG_HIP(hipGetLastError());
    s->init_from = nullptr;
  }

  // K10 once, K7/K9 for the constructor scheme
  const SysParams P = make_params(s, s->scheme_ctor);
  Laps laps;
  build_numbering(P, slab, s->nb);
  laps.lap("build_numbering");
  assemble_csr_preconditioned(P, slab, s->nb, s->A_ctor);
  laps.lap("assemble_csr_preconditioned");
  s->A_ctor.scheme = s->scheme_ctor;

  const i64 n = s->nb.n_own, nv = s->nb.n_vec();
  const i64 na = n > 0 ? n : 1, nva = nv > 0 ? nv : 1;
  s->mass.alloc(na); s->bconst.alloc(na); s->bcv.alloc(na); s->fixed.alloc(na);
  s->x.alloc(nva); s->b.alloc(nva); s->y.alloc(nva); s->z.alloc(nva); s->ysol.alloc(nva);
  s->x.zero(); s->b.zero(); s->y.zero(); s->z.zero(); s->ysol.zero();
  s->work.init(n, nv);
  s->red_scratch.alloc(2048);
  if (n > 0) {
    KeyVals kv;
    for (int k = 0; k < 6; ++k) kv.v[k] = s->border_value[k];
    hipLaunchKernelGGL(k_row_static, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, st, P, make_segs(s->nb), n, s->nb.row_cell.p,
                       kv, s->mass.p, s->fixed.p, s->bcv.p);
    PG_HIP(hipGetLastError());
  }
  laps.lap("row data, vectors");
  build_first_rhs(s);
  laps.lap("first right-hand side");
  s->t = 0.0;
}

double max_abs(pg_solver* s) {
  hipStream_t st = ctx().stream;
  const i64 n = s->nb.n_own;
  double m = 0.0;
  if (n > 0) {
    const int g = grid_for(n, BLOCK, 2048);
    if (s->x_valid) hipLaunchKernelGGL(k_maxabs, dim3(g), dim3(BLOCK), 0, st, n, s->x.p, (const double*)nullptr, s->red_scratch.p);
    else hipLaunchKernelGGL(k_maxabs, dim3(g), dim3(BLOCK), 0, st, n, s->z.p, s->z_matrix->ds.p, s->red_scratch.p);
    PG_HIP(hipGetLastError());
    std::vector<double> h(g);
    s->red_scratch.download(h.data(), g);
    for (double v : h) m = std::max(m, v);
  }
  if (ctx().nranks > 1 || ctx().comm) {
    DevBuf<double> d(1);
    d.upload(&m, 1);
    comm_allreduce_max_f64(d.p, 1, st);
    d.download(&m, 1);
  }
  return m;
}

void ensure_run_matrix(pg_solver* s, int scheme) {
  if (s->have_run && s->scheme_run == scheme) return;
  if (scheme == s->scheme_ctor && s->A_ctor.n == s->nb.n_own && s->A_ctor.rowptr.p) {
    // same scheme: the loop matrix equals the constructor matrix (border rows are re-applied identically)
    s->scheme_run = scheme;
    s->have_run = true;
    return;
  }
  const SysParams P = make_params(s, scheme);
  s->spec_y_valid = false;          // (a product queued ahead with the matrix that is about to be replaced)
  s->elim_run = GammaElim();        // (belongs to the matrix that is about to be replaced)
  s->diag_run = DiagElim();
  if (s->rc_last == &s->diag_run) s->rc_last = nullptr;
  if (!s->mg_step[1].lev.empty()) s->mg_step[1] = MgHierarchy();
  if (s->blk_cache_matrix == &s->A_run) s->blk_cache_matrix = nullptr;
  assemble_csr_like(P, s->slab, s->nb, s->A_ctor, s->A_run);
  s->A_run.scheme = scheme;
  s->scheme_run = scheme;
  s->have_run = true;
}

const CsrMatrix& run_matrix(const pg_solver* s) {
  return (s->scheme_run == s->scheme_ctor) ? s->A_ctor : s->A_run;
}

void fill_info(pg_solver* s, const SolveStats& st, pg_step_info* info) {
  if (!info) return;
  info->iters = st.iters;
  info->converged = st.converged;
  info->resnorm = st.resnorm;
  info->bnorm = st.bnorm;
  info->extremum = max_abs(s);
  info->time = s->t;
}

// x = S z, on demand
void materialize_x(pg_solver* s) {
  if (s->x_valid) return;
  const i64 n = s->nb.n_own;
  if (n > 0) {
    hipLaunchKernelGGL(k_scale_state, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx().stream, n, s->z_matrix->ds.p, s->z.p,
                       s->x.p, 0);
    PG_HIP(hipGetLastError());
  }
  s->x_valid = true;
}

void keep_state(pg_solver* s) {
  materialize_x(s);
  DevBuf<double> cp(s->nb.n_own > 0 ? s->nb.n_own : 1);
  if (s->nb.n_own > 0)
    PG_HIP(hipMemcpyAsync(cp.p, s->x.p, sizeof(double) * s->nb.n_own, hipMemcpyDeviceToDevice, ctx().stream));
  s->states.emplace_back(std::move(cp));
}

// ---- monitors, host side ---------------------------------------------------------------------------------------------------
// Storage rule.  Per step a dense monitor streams its n_own weights (8·n bytes) and shares one read of the state (z and ds,
// 16·n bytes) with every other dense monitor; a sparse entry costs its row and weight (12 bytes) and two gathered words, each
// counted as a 128-byte line of its own, the unit gfx950's L2 requests from memory (MON_SPARSE_ENTRY_BYTES = 268).  With
// C = {m : 268·nnz_m > 8·n}, the monitors that are cheaper dense once the state is paid for, the cheapest assignment is: all of
// C dense when Σ_C (268·nnz_m − 8·n) > 16·n, else every monitor sparse (a subset of C gains less, a monitor outside C loses).
constexpr i64 MON_SPARSE_ENTRY_BYTES = 12 + 2 * 128;

void mon_choose_storage(i64 n, int K, const i64* nnz, bool* sparse) {
  i64 gain = 0;
  for (int m = 0; m < K; ++m)
    if (MON_SPARSE_ENTRY_BYTES * nnz[m] > 8 * n) gain += MON_SPARSE_ENTRY_BYTES * nnz[m] - 8 * n;
  const bool any_dense = gain > 16 * n;
  for (int m = 0; m < K; ++m) sparse[m] = !(any_dense && MON_SPARSE_ENTRY_BYTES * nnz[m] > 8 * n);
}

void mon_clear(pg_solver* s) {
  pg_solver::Monitors& M = s->mon;
  for (int m = 0; m < PG_MON_MAX; ++m) {
    M.w[m].release();
    M.row[m].release();
    M.kind[m] = 0; M.sparse[m] = false; M.stored[m] = 0;
  }
  M.series.release();
  M.times.clear();
  M.K = 0; M.G = 0; M.rows = 0; M.cap = 0;
}

// one evaluation of every monitor on the current state: G·K partials to `out`
void mon_launch(const pg_solver* s, double* out, hipStream_t st) {
  const pg_solver::Monitors& M = s->mon;
  const i64 n = s->nb.n_own;
  MonArgs a{};
  int nd = 0;
  for (int m = 0; m < M.K; ++m) {
    a.w[m] = M.w[m].p;
    a.row[m] = M.sparse[m] ? M.row[m].p : nullptr;
    a.cnt[m] = M.sparse[m] ? M.stored[m] : 0;
    a.kind[m] = M.kind[m];
    if (!M.sparse[m]) a.dense[nd++] = m;
  }
  a.K = M.K;
  const double* x = s->x_valid ? s->x.p : s->z.p;
  const double* ds = s->x_valid ? nullptr : s->z_matrix->ds.p;
  i64 chunk = (n + M.G - 1) / M.G;
  chunk += chunk & 1;
  switch (nd) {
#define PG_MONITOR(NDV) \
  case NDV: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_monitor<NDV>), dim3(M.G), dim3(BLOCK), 0, st, n, chunk, x, ds, a, out); break;
    PG_MONITOR(0) PG_MONITOR(1) PG_MONITOR(2) PG_MONITOR(3) PG_MONITOR(4)
    PG_MONITOR(5) PG_MONITOR(6) PG_MONITOR(7) PG_MONITOR(8)
#undef PG_MONITOR
  }
  PG_HIP(hipGetLastError());
}

// room for `more` further rows: the buffer grows by doubling (at least), the copy ordered on the same stream.  pg_solver_run
// reserves its whole loop before the first step, so nothing is allocated, freed or copied between its steps.
void mon_reserve(pg_solver* s, i64 more) {
  pg_solver::Monitors& M = s->mon;
  if (M.K == 0 || M.rows + more <= M.cap) return;
  hipStream_t st = ctx().stream;
  const i64 per_row = (i64)M.G * M.K;
  i64 cap = M.cap > 0 ? 2 * M.cap : 64;
  while (cap < M.rows + more) cap *= 2;
  DevBuf<double> grown(cap * per_row);
  if (M.rows > 0)
    PG_HIP(hipMemcpyAsync(grown.p, M.series.p, sizeof(double) * (size_t)(M.rows * per_row), hipMemcpyDeviceToDevice, st));
  M.series = std::move(grown);
  M.cap = cap;
}

// after a completed solve: one row of the series
void mon_record(pg_solver* s) {
  pg_solver::Monitors& M = s->mon;
  if (M.K == 0) return;
  hipStream_t st = ctx().stream;
  const i64 per_row = (i64)M.G * M.K;
  mon_reserve(s, 1);
  mon_launch(s, M.series.p + M.rows * per_row, st);
  M.times.push_back(s->t);
  ++M.rows;
}

pg_krylov_opts default_opts() {
  pg_krylov_opts o;
  o.method = PG_METHOD_BICGSTAB;
  o.reltol = 1e-12;
  o.abstol = 0.0;
  o.maxiter = 0;
  o.check_every = 4;
  o.warm_start = 1;
  o.restart = 0;
  o.precond = 0;
  return o;
}

// opts.precond = PG_PRECOND_MG: the conditions under which the multigrid preconditioner is offered -- anything else is refused
// with the condition that failed, never served by another iteration -- then the hierarchy, on first use, and its hand-over to
// the Krylov driver for the solve that follows.
// PG_PRECOND_MG_CELL (the cell rule) asks the same but for the interface condition: Dirichlet, Robin and Neumann are all served.
void mg_conditions(const pg_solver* s, int method, MgRule rule = MG_RULE_KIND) {
  const std::string who = std::string("multigrid preconditioner (precond = ") + mg_precond_name(rule) + ") refused: ";
  mg_require_one_rank(rule);
  PG_REQUIRE(s->scheme_ctor == PG_SCHEME_STEADY && !s->moving,
             who + (rule == MG_RULE_CELL ? "the system is an unsteady one (steady monophasic diffusion only)"
                                         : "the system is an unsteady one (steady monophasic diffusion and the stream-function solve only)"));
  PG_REQUIRE(s->nphase == 1, who + "the system is diphasic (its jump rows need the cell-block left preconditioner)");
  PG_REQUIRE(!s->advdiff && !(s->ops[0] && s->ops[0]->has_velocity), who + "the operator is a ConvectionOps (DiffusionOps only)");
  PG_REQUIRE(rule == MG_RULE_CELL || s->bc_i.kind == PG_BC_DIRICHLET,
             who + (s->bc_i.kind == PG_BC_ROBIN ? "the interface condition is Robin (Dirichlet only)"
                                                : "the interface condition is Neumann (Dirichlet only)"));
  // (not "no blocked rows": the cut cells of a Dirichlet interface are blocked too -- their γ row is a row of the identity, and
  //  B⁻¹ only takes the same-cell γ entry out of the ω row.  Â keeps its unit diagonal; the hierarchy is built on Â as it is.)
  PG_REQUIRE(method == PG_METHOD_BICGSTAB, who + krylov_method_refusal(method));
}

MgHierarchy& mg_of(pg_solver* s, MgRule rule) { return rule == MG_RULE_CELL ? s->mg_cell : s->mg; }

MgHierarchy& mg_ensure(pg_solver* s, MgRule rule = MG_RULE_KIND) {
  MgHierarchy& H = mg_of(s, rule);
  if (H.matrix != &s->A_ctor || H.lev.empty()) mg_build(H, s->A_ctor, s->nb, s->slab, rule);
  return H;
}

// before every krylov_solve on A_ctor that takes the caller's options: the hierarchy for that solve's KrylovCall (null: none asked for)
MgHierarchy* mg_prepare(pg_solver* s, const pg_krylov_opts& o) {
  if (!mg_is_precond(o.precond)) return nullptr;
  const MgRule rule = mg_rule_of(o.precond);
  mg_conditions(s, o.method, rule);
  return &mg_ensure(s, rule);
}

// opts.precond = PG_PRECOND_MG_STEP: the cell rule's V-cycle inside the unsteady time loop.  Served on the systems of
// DiffusionUnsteadyMono (Dirichlet, Robin or Neumann interface) and DiffusionUnsteadyDiph, BE and CN; refused with the failed
// condition anywhere else.
void mg_step_conditions(const pg_solver* s, int method) {
  const std::string who = "multigrid preconditioner (precond = PG_PRECOND_MG_STEP) refused: ";
  mg_require_one_rank_of(PG_PRECOND_MG_STEP);
  PG_REQUIRE(s->scheme_ctor != PG_SCHEME_STEADY,
             who + "the system is a steady one (the time loop of the unsteady monophasic diffusion solver only; steady solves are "
                   "served by PG_PRECOND_MG and PG_PRECOND_MG_CELL)");
  PG_REQUIRE(!s->moving, who + "a moving-body solver (every space-time slab is a new matrix that is solved once)");
  PG_REQUIRE(!s->solved_once, who + "the vorticity solver of a pg_streamvort step (a new matrix every step, solved once)");
  PG_REQUIRE(!s->advdiff && !s->convection && !(s->ops[0] && s->ops[0]->has_velocity),
             who + "the operator is a ConvectionOps (DiffusionOps only)");
  // (diphasic systems are served: the cell rule merges the four kinds of unknowns of a cell as it merges two -- mg_build)
  PG_REQUIRE(method == PG_METHOD_BICGSTAB, who + krylov_method_refusal(method));
}

// the hierarchy of A (&s->A_ctor or &s->A_run), built on first use and kept for the life of the matrix.  A set-up that fails (a
// coarse diagonal entry that is not positive) is the refusal of this solve: nothing is kept, nothing else runs in its place.
MgHierarchy& mg_step_ensure(pg_solver* s, const CsrMatrix& A) {
  MgHierarchy& H = s->mg_step[&A == &s->A_ctor ? 0 : 1];
  if (H.matrix == &A && !H.lev.empty()) return H;
  try {
    mg_build(H, A, s->nb, s->slab, MG_RULE_CELL);
  } catch (...) {
    H = MgHierarchy();
    throw;
  }
  return H;
}

// opts.precond = PG_PRECOND_POLY_EST: what it is refused on (with the condition that failed, as the multigrid does), then --
// before every krylov_solve on A that takes the caller's options, and only where Gershgorin refuses A -- the spectral estimate of
// A (pg_specest.hip), once per assembled matrix.  Where Gershgorin admits A nothing runs: the solve is the precond = 0 solve.
void specest_conditions(const pg_solver* s, int method) {
  const std::string who = "estimated polynomial preconditioner (precond = PG_PRECOND_POLY_EST) refused: ";
  specest_require_one_rank();
  PG_REQUIRE(!s->moving, who + "a moving-body solver (every space-time slab is a new matrix that is solved once)");
  PG_REQUIRE(!s->advdiff && !s->convection, who + "the operator is a ConvectionOps (DiffusionOps only)");
  PG_REQUIRE(method == PG_METHOD_BICGSTAB, who + krylov_method_refusal(method));
}

void specest_prepare(pg_solver* s, const CsrMatrix& A, const pg_krylov_opts& o) {
  if (o.precond != PG_PRECOND_POLY_EST) return;
  specest_conditions(s, o.method);
  if (A.poly_ok || A.est.tried || A.poly_gave_up) return;   // (stagnated: it runs plain, as with precond = 0 -- no second chance)
  specest_run(const_cast<CsrMatrix&>(A), s->nb, s->slab);
}

// One solve of the constructor's system Â z = b̂ (A_ctor, s->b) and the state it leaves, for do_initial, solver_solve_again and
// solver_first_solve_from_state.  from_state: start from a state and one product with it (the caller knows which methods that
// serves), else from zero.  first: the solver's first solve -- the start state is s->x, scaled here (later solves start from the
// z they left), and the time loop's bookkeeping begins.  mg: the hierarchy for a multigrid precond (mg_prepare), or null.
void solve_ctor_system(pg_solver* s, const pg_krylov_opts& o, SolveStats& st, bool from_state, bool first, MgHierarchy* mg) {
  const i64 n = s->nb.n_own;
  KrylovCall call;
  call.mg = mg;
  if (from_state) {
    hipStream_t stream = ctx().stream;
    if (first) hipLaunchKernelGGL(k_scale_state, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, stream, n, s->A_ctor.ds.p, s->x.p, s->z.p, 1);
    spmv_halo(s->A_ctor, s->nb, s->slab, s->z.p, s->y.p, stream);
    PG_HIP(hipGetLastError());
    call.x0 = s->z.p; call.Ax0 = s->y.p;
  }
  krylov_solve(s->A_ctor, s->nb, s->slab, s->b.p, s->ysol.p, s->work, o, st, call);
  std::swap(s->z.p, s->ysol.p);   // the scaled solution becomes the state (same-size buffers trade roles)
  s->z_matrix = &s->A_ctor;
  s->x_valid = false;
  if (!first) return;
  s->initial_done = true;
  s->diag_ctor.snapped_version = s->diag_run.snapped_version = -1;   // z was replaced behind the compact path's back
  s->hist_cnt = 0;
  s->spec_y_valid = false;
}

void do_initial(pg_solver* s, const pg_krylov_opts* opts, SolveStats& st) {
  const pg_krylov_opts o = opts ? *opts : default_opts();
  MgHierarchy* mg = mg_prepare(s, o);
  if (mg_is_step(o.precond)) {
    mg_step_conditions(s, o.method);
    mg = &mg_step_ensure(s, s->A_ctor);
  }
  specest_prepare(s, s->A_ctor, o);
  // solve_system!(s) with the constructor's A and b (diffusion.jl:275).  A slab of the moving solver starts from the previous
  // state on this slab's active set (s->x, written by k_rhs_first; fresh cells start from the 0 their eliminated unknown held)
  // -- a time step, as pg_solver_step's warm start
  const bool from_state = s->moving && o.warm_start != 0 && o.method == PG_METHOD_BICGSTAB && s->nb.n_own > 0;
  solve_ctor_system(s, o, st, from_state, true, mg);
}

// ---- host side of the extrapolated start (GuessArgs), shared by the compact and the plain warm path ---------------------
// Worth its launch?  The fit costs about 20 us per step whatever the size, a product max(5 us, its bytes at 5 TB/s): the
// mechanism is switched on (for good, on this system) once a solve has used so many products that a few of them saved pay
// for it -- 512^3: from 7 products (the loop needs 26), 64^3 ... 2048^2: from 18 (launch-bound: the 26 products of the 3-D CN
// loops qualify, +15 ... +50 %) -- and not on systems of a few thousand rows, where every launch is latency and the fit's
// is one more (80^2, 1815 rows: 19 -> 11 products per step and still 6400 instead of 7800 steps/s).
void guess_policy(bool& on, double last_products, double bytes_per_product) {
  const Config& cfg = config();
  if (on || cfg.guess_n <= 0 || last_products <= 0.0) return;
  const double t_prod_us = std::max(5.0, bytes_per_product / 5.0e6);
  if (cfg.guess_always || (bytes_per_product >= 256.0 * 1024.0 && last_products >= 6.0 + 3.0 * (20.0 / t_prod_us))) on = true;
}

struct GuessPlan {
  int KH = 0, R = 0, hist_had = 0;
  bool refit = true;      // false: this step keeps the coefficients it has (see guess_prepare)
  GuessArgs ga{};
  bool fit_due() const { return KH > 0 && hist_had > 0 && refit; }
};

inline double* guess_block(pg_solver* s) { return s->guess_coef.p + (s->guess_buf ? GUESS_USED : 0); }

// before the step's first kernel: the ring buffers and the kernel's arguments; the count of valid older states is taken
// and reset (guess_commit restores it once the step has gone its way to the end)
// two_blocks: the caller's fit rides in its right-hand-side launch and alternates between the two coefficient blocks; every
// other caller reads and rewrites block 0 (a solver that changes from the one to the other starts its history afresh)
GuessPlan guess_prepare(pg_solver* s, const void* owner, bool allowed, double last_products, hipStream_t stream,
                        bool two_blocks = false) {
  const Config& cfg = config();
  GuessPlan gp;
  // a loop that is down to the smallest polynomial (or meets the tolerance at the start) has nothing left to save: the fit
  // then runs every eighth step only -- its launch is a third of such a step on small systems
  gp.refit = last_products > 4.0 || s->steps_done % 8 == 0;
  gp.KH = allowed ? cfg.guess_n : 0;                           // older states read at most
  gp.R = gp.KH > 0 ? cfg.guess_depth : 0;                      // older states kept
  gp.hist_had = (s->hist_de == owner && s->hist_k == gp.R) ? s->hist_cnt : 0;
  s->hist_cnt = 0;
  if (gp.KH == 0) return gp;
  if (!two_blocks && s->guess_buf != 0) gp.hist_had = 0;
  const int R = gp.R;
  const i64 nva = s->z.n;
  if (s->guess_coef.n == 0) { s->guess_coef.alloc(GUESS_USED + 16); s->guess_coef.zero(); s->guess_ticket.alloc(1); s->guess_ticket.zero(); }
  for (int j = 0; j <= R; ++j) {      // (one more product buffer than states: the one retired a step ago takes the next
    if (j < R && s->zh[j].n != nva) { s->zh[j].alloc(nva); s->zh[j].zero(); }   //  product while the fit still reads the others)
    if (s->yh[j].n != nva) { s->yh[j].alloc(nva); s->yh[j].zero(); }
  }
  if (gp.hist_had == 0) {
    PG_HIP(hipMemsetAsync(s->guess_coef.p, 0, 12 * sizeof(double), stream));   // (the counters stay)
    PG_HIP(hipMemsetAsync(s->guess_coef.p + GUESS_USED, 0, 12 * sizeof(double), stream));
    s->guess_buf = 0;
  }
  for (int j = 0; j < 8; ++j) { gp.ga.zr[j] = s->zh[std::min(j, R - 1)].p; gp.ga.yr[j] = s->yh[std::min(j, R - 1)].p; }
  gp.ga.znew = s->zh[R - 1].p;
  gp.ga.coef = guess_block(s);
  gp.ga.count = s->guess_coef.p + 13;
  gp.ga.used = nullptr;
  return gp;
}

// after the step's first kernel: the fit for the next step (k_guess_fit; cmap == NULL: every row is in the loop), then the
// buffers trade places
// the fit's arguments and its number of blocks (gp.fit_due() holds); the coefficients go to the block that stands
GuessFit guess_fit_args(pg_solver* s, const GuessPlan& gp, i64 n, bool single, const KrylovWork& w, int& gfit) {
  const Config& cfg = config();
  const int R = gp.R;
  GuessFit gf{};
  for (int j = 0; j < 8; ++j) gf.yr[j] = s->yh[std::min(j, R - 1)].p;
  const i64 nchunk = (n + BLOCK - 1) / BLOCK;
  gf.stride = (int)std::max<i64>(1, std::min<i64>(cfg.guess_monitor, nchunk / 128));   // (small systems: every chunk)
  gfit = std::max((int)std::min<i64>(128, (nchunk + gf.stride - 1) / gf.stride), 1);
  if (s->guess_partials.n != (i64)GUESS_NS * gfit) s->guess_partials.alloc((i64)GUESS_NS * gfit);
  gf.partials = s->guess_partials.p;
  gf.ticket = s->guess_ticket.p;
  gf.coef = guess_block(s);
  gf.avail = std::min(gp.hist_had, GUESS_RM);
  gf.kmax = gp.KH;
  gf.rate2 = w.last_rate2;
  gf.pass_cost = cfg.guess_pass_cost;
  gf.gain = cfg.guess_gain;
  gf.sums = single ? nullptr : s->guess_coef.p + 16;
  gf.nblocks = gfit;
  return gf;
}

// fit_done: the fit has run inside the step's first kernel (step_compact)
void guess_after_rhs(pg_solver* s, const GuessPlan& gp, i64 n, const int* cmap, const double* ds, const double* rhat, bool single,
                     KrylovWork& w, hipStream_t stream, bool fit_done = false) {
  if (gp.KH == 0) return;
  const int R = gp.R;
  if (gp.fit_due() && !fit_done) {
    int gfit = 0;
    const GuessFit gf = guess_fit_args(s, gp, n, single, w, gfit);
    hipLaunchKernelGGL(k_guess_fit, dim3(gfit), dim3(BLOCK), 0, stream, n, cmap, ds, (const double*)s->b.p,
                       (const double*)s->y.p, rhat, gf);
    if (!single) {
      comm_allreduce_sum_f64(gf.sums, GUESS_NS, stream);
      hipLaunchKernelGGL(k_guess_decide, dim3(1), dim3(BLOCK), 0, stream, gf);
    }
    PG_HIP(hipGetLastError());
  }
  // the buffers trade places (stream order keeps the kernels above ahead of whatever writes them next): the state written
  // becomes z, z and ŷ become the newest kept pair, the product buffer retired a step ago is the next product's output
  double* znew = s->zh[R - 1].p;
  double* yspare = s->yh[R].p;
  double* yretire = s->yh[R - 1].p;
  for (int j = R - 1; j > 0; --j) { s->zh[j].p = s->zh[j - 1].p; s->yh[j].p = s->yh[j - 1].p; }
  s->zh[0].p = s->z.p; s->z.p = znew;
  s->yh[0].p = s->y.p; s->y.p = yspare;
  s->yh[R].p = yretire;
}

// the step has gone its way to the end: one more older state stands
void guess_commit(pg_solver* s, const GuessPlan& gp, const void* owner) {
  if (gp.KH == 0) return;
  if (config().debug) {
    double hc[16];
    s->guess_coef.download(hc, 16, s->guess_buf ? GUESS_USED : 0);
    fprintf(stderr, "[pg_solver] extrapolated start: %d older states kept; sampled (r,r)_W plain %.3e, taken %.3e; next step: %d states",
            gp.hist_had, hc[9], hc[10], (int)hc[4]);
    for (int j = 0; j < (int)hc[4]; ++j) fprintf(stderr, " z(n-%d)*%.4f", (int)hc[5 + j] + 1, hc[j]);
    fprintf(stderr, ", fit leaves %.3e\n", hc[11]);
  }
  s->hist_cnt = std::min(gp.hist_had + 1, gp.R);
  s->hist_k = gp.R;
  s->hist_de = owner;
}

// the block rows of a diphasic CN right-hand side, matrix-free from the scaled state z (see k_rhs_block_mf)
void launch_rhs_block_mf(pg_solver* s, int scheme, const CsrMatrix& A, hipStream_t stream) {
  hipLaunchKernelGGL(k_rhs_block_mf, dim3(grid_for(A.n_blk, BLOCK)), dim3(BLOCK), 0, stream, make_params(s, scheme), make_segs(s->nb),
                     s->Mloc, A.n_blk, A.blk_rows.p, A.blk_idx.p, A.blk_coef.p, s->nb.row_cell.p, s->nb.red.p, A.ds.p,
                     (const double*)s->z.p, s->mass.p, s->bconst.p, s->fixed.p, s->b.p);
}

// The block rows of the warm loop's right-hand side.  rhs_block_cached: they come from the tables of k_blk_cache, which are
// brought up to date here (false: there are none, or the diphasic CN form evaluates them matrix-free); launch_rhs_block: the
// launch that writes them to b̂, whichever form it is.
bool rhs_block_cached(pg_solver* s, int scheme, const CsrMatrix& A) {
  hipStream_t stream = ctx().stream;
  const bool blk_mf = s->nphase == 2 && scheme == PG_SCHEME_CN;   // (see k_rhs_block_mf)
  if (A.n_blk <= 0 || blk_mf) return false;
  if (s->blk_cache_matrix != &A || s->blk_cache_scheme != scheme || s->blk_cache_version != s->bconst_version) {
    if (s->blk_wz.n != A.n_blk * MAX_KINDS) s->blk_wz.alloc(A.n_blk * MAX_KINDS);   // (time-dependent data: rebuilt every step)
    if (s->blk_c0.n != A.n_blk) s->blk_c0.alloc(A.n_blk);
    hipLaunchKernelGGL(k_blk_cache, dim3(grid_for(A.n_blk, BLOCK)), dim3(BLOCK), 0, stream, A.n_blk, scheme, A.blk_idx.p,
                       A.blk_coef.p, A.ds.p, s->mass.p, s->bconst.p, s->fixed.p, s->blk_wz.p, s->blk_c0.p);
    s->blk_cache_matrix = &A; s->blk_cache_scheme = scheme; s->blk_cache_version = s->bconst_version;
  }
  return true;
}

void launch_rhs_block(pg_solver* s, int scheme, const CsrMatrix& A, hipStream_t stream) {
  if (A.n_blk <= 0) return;
  if (rhs_block_cached(s, scheme, A))
    hipLaunchKernelGGL(k_rhs_block_c, dim3(grid_for(A.n_blk, BLOCK)), dim3(BLOCK), 0, stream, A.n_blk, scheme, A.blk_rows.p,
                       BlkTables{A.blk_idx.p, s->blk_wz.p, s->blk_c0.p, A.blk_cn.p, nullptr}, (const double*)s->z.p,
                       (const double*)s->y.p, s->b.p);
  else launch_rhs_block_mf(s, scheme, A, stream);
}

// The compact warm step: the right-hand-side kernel solves the rows alone on their diagonal, BiCGStab with the polynomial runs on
// the compact image DE.A of A (pg_reduce.hip, DiagElim).  used_de tells do_step's QuietGuard that this path's bookkeeping stands.
void step_compact(pg_solver* s, int scheme, const pg_krylov_opts& o, const CsrMatrix& A, DiagElim& DE, const DiagElim*& used_de,
                  SolveStats& st) {
  hipStream_t stream = ctx().stream;
  const i64 n = s->nb.n_own;
  KrylovWork& w = s->work;
  // r = r̂ = p of the remaining rows go straight to the compact vectors; the other rows are solved in the same pass
  const int stamp = (int)((s->steps_done % 2000000000) + 1);   // marks E.flag when a diagonal row moved in THIS step
  // quiet: the previous step ran this path with the same constant data, so every diagonal row already holds its solution
  // and none can move (beyond rounding) -- the coupling / renorm launches are not queued and the solver's start phase is
  // folded into the right-hand-side kernel (3 launches less)
  // Several ranks: the host-side knowledge "same constant data as the step before" is the same on every rank, so the
  // coupling / renorm launches (and the exchange of the deltas they need there) are skipped collectively; only the folded
  // start is a one-rank thing (the scalar phase of several ranks goes through an all-reduce).
  const bool single = ctx().nranks == 1 && !ctx().comm;
  const bool same_data = DE.snapped_version == s->bconst_version;
  const bool quiet = same_data && single;
  // extrapolated start (GuessArgs): steps with unchanged data only -- the rows alone on their diagonal rest, so the
  // differences of the kept states are differences of the loop's rows alone and the products ŷ^{n-o} combine linearly.
  // Several ranks: "unchanged data" is the same verdict everywhere, the fit's sums go through an all-reduce and every rank
  // takes the same decision.
  guess_policy(DE.guess_on, DE.last_products, DE.bytes_per_rank);
  const Config& cfg = config();
  // PG_STEP_FUSE, one rank: the fit for the next step rides in the right-hand-side launch -- blocks of the same launch, past its
  // w.grid main ones, writing the coefficient block this launch does not read.  Not where the block rows are evaluated
  // matrix-free (k_rhs_block_mf): the fit's blocks evaluate the block rows they sample from the tables of k_blk_cache (do_step
  // has brought them up to date), and read no b̂.
  const bool fuse_mode = cfg.step_fuse && single && !(A.n_blk > 0 && s->nphase == 2 && scheme == PG_SCHEME_CN);
  GuessPlan gp = guess_prepare(s, &DE, same_data && DE.guess_on, DE.last_products, stream, fuse_mode);
  const int KH = gp.KH;
  // the extrapolated state itself is formed by the solve's first update of x (KrylovCall::xguess): the older states are
  // then read there through the compact system's index map, once, and this kernel neither reads them nor writes the state
  // (not after a solve that met the tolerance at its start: the next one probably will too, no update of x runs then, and
  //  writing the state from the first s kernel's early exit costs more than writing it here -- 64^3 BE near steady state)
  const bool defer = KH > 0 && cfg.guess_defer && DE.last_products > 0.0;
  gp.ga.defer = defer ? 1 : 0;
  const bool fit_rides = fuse_mode && rhs_fuses(KH, defer);      // (whenever a fit is due)
  const bool fit_fused = fit_rides && gp.fit_due();
  const BlkTables bt{A.blk_idx.p, s->blk_wz.p, s->blk_c0.p, A.blk_cn.p, A.n_blk > 0 ? A.blk_pos.p : nullptr};
  int gfit = 0;
  GuessFit gf{};
  if (fit_fused) {
    gf = guess_fit_args(s, gp, n, true, w, gfit);
    s->guess_buf ^= 1;
    gf.coef = guess_block(s);
  }
  // (the fit rides: nothing rewrites the block this launch reads before the step is over -- the first update of x reads it there too)
  gp.ga.used = (defer && !fit_rides) ? s->guess_coef.p + GUESS_USED : nullptr;
  const GuessArgs& ga = gp.ga;
  const double* zprev = s->z.p;      // z^n (the buffers trade places below)
  // the rows whose constants are one value (PG_ROW_CONST; pg_reduce.h): mass and fixed are written once, by setup_common, so
  // the tables stand as long as DE does; bconst's mark is looked up for this step's version
  if (!DE.rc_tried) build_row_const(A, s->mass.p, s->fixed.p, DE);
  const RowConst rc_full = row_const_bconst(DE, s->bconst.p, s->bconst_version);
#define PG_RHS_INIT_C(KHV, DF)                                                                                                    \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rhs_init_c<KHV, DF>), dim3(w.grid + gfit * FIT_PARTS), dim3(BLOCK), 0, stream, n, scheme, s->z.p, s->y.p, A.ds.p, \
                     s->mass.p, s->bconst.p, s->fixed.p, A.isblk.p, DE.cmap.p, s->b.p, (const double*)DE.gdiag.p, DE.delta.p,     \
                     DE.flag.p, stamp, w.rhat.p, w.partials.p, quiet ? w.ticket.p : nullptr, w.sc.p, o.reltol * o.reltol,          \
                     o.abstol * o.abstol, same_data ? 0 : 1, ga, bt, gf, w.grid, rc_full)
  switch (KH) {
    case 1: if (defer) PG_RHS_INIT_C(1, true); else PG_RHS_INIT_C(1, false); break;
    case 2: if (defer) PG_RHS_INIT_C(2, true); else PG_RHS_INIT_C(2, false); break;
    case 3: if (defer) PG_RHS_INIT_C(3, true); else PG_RHS_INIT_C(3, false); break;
    case 4: if (defer) PG_RHS_INIT_C(4, true); else PG_RHS_INIT_C(4, false); break;
    default: PG_RHS_INIT_C(0, false); break;
  }
#undef PG_RHS_INIT_C
  PG_HIP(hipGetLastError());
  guess_after_rhs(s, gp, n, (const int*)DE.cmap.p, (const double*)A.ds.p, (const double*)w.rhat.p, single, w, stream, fit_fused);
  if (!same_data) diag_fix(DE, s->nb, s->slab, stamp, !single, w.rhat.p, w.partials.p, w.grid, stream);
  KrylovCall call;
  call.preinit = call.p_in_rhat = true;
  call.start_folded = quiet;
  call.scatter = DE.rlist.p;
  call.row_const = DE.rc_view_loop();
  s->rc_last = &DE;
  // several ranks, unchanged data: nobody looks at the rows alone on their diagonal (no diag_fix), so the flag k_rhs_init_c
  // raised goes through the start phase's all-reduce and comes back as S_MOVED, the same on every rank
  if (same_data && !single) { call.moved_flag = DE.flag.p; call.moved_stamp = stamp; }
  DE.snapped_version = s->bconst_version;
  used_de = &DE;
  s->spec_pending = false;
  if (quiet && s->hint_more_steps && config().speculate_product)
    call.after_first_batch = [s, &A, stream]() {     // the next step's ŷ = Â z, behind this solve's (expected) last update of z
      spmv_halo(A, s->nb, s->slab, s->z.p, s->y.p, stream);
      s->spec_pending = true;
      s->spec_matrix = &A;
    };
  if (defer) {
    call.xguess.zbase = zprev;
    for (int j = 0; j < 8; ++j) call.xguess.zr[j] = ga.zr[j];
    call.xguess.coef = ga.used ? ga.used : ga.coef;
  }
  krylov_solve(DE.A, DE.nb, s->slab, nullptr, s->z.p, w, o, st, call);
  // the speculative product stands when the solve ended inside its first batch (nothing has touched z since)
  s->spec_y_valid = s->spec_pending && st.polls == 1 && st.converged && st.poly_degree >= 0;
  s->spec_pending = false;
  const bool solved = st.poly_degree >= 0;   // -1: the polynomial stagnated on the compact system -> the full system below
  DE.last_products = (double)st.products;

  // A step with unchanged data rests on "no row alone on its diagonal moves while the data are unchanged"; k_rhs_init_c
  // checks it anyway and the start phase reports it (S_MOVED): the residual the iteration started from then lacked the
  // coupling term, and the step is finished on the full system from the state reached.  Several ranks read the verdict
  // out of the start phase's all-reduce: a row that moved on one rank sends all of them this way, or none.
  const bool moved_unseen = solved && same_data && w.h_sc[S_MOVED] != 0.0;
  if (!solved || moved_unseen) {
    s->spec_y_valid = false;
    // z has moved (the rows left out hold their solution, the x-space iteration has updated the rest): the right-hand
    // side b̂ of this step -- written for every row by k_rhs_init_c -- stands, the iteration continues on the full
    // system from the state reached, r = b̂ - Âz
    if (!solved) {
      DE.active = false;
      // the compact matrix is made of the full one's rows: the verdict on the polynomial holds for both, and the solve
      // below goes plain at once instead of stagnating a second time
      poly_record_stagnation(A);
    }
    used_de = nullptr;
    const SolveStats first = st;
    st = SolveStats();
    spmv_halo(A, s->nb, s->slab, s->z.p, s->y.p, stream);
    KrylovCall full;
    full.x0 = s->z.p; full.Ax0 = s->y.p;
    krylov_solve(A, s->nb, s->slab, s->b.p, s->ysol.p, w, o, st, full);
    std::swap(s->z.p, s->ysol.p);
    st.iters += first.iters;
    st.products += first.products;
  }
  else guess_commit(s, gp, &DE);
  s->x_valid = false;
}

// The plain warm step: the iteration starts from the previous state on the full system, or on Â_ωω where the γ elimination runs.
void step_warm(pg_solver* s, int scheme, const pg_krylov_opts& o, const CsrMatrix& A, bool mgs, SolveStats& st) {
  hipStream_t stream = ctx().stream;
  const i64 n = s->nb.n_own;
  KrylovWork& w = s->work;
  // Dirichlet interface: the γ rows are rows of the identity -- solved here, the iteration runs on Â_ωω (pg_reduce.hip)
  GammaElim& E = (&A == &s->A_ctor) ? s->elim_ctor : s->elim_run;
  if (!mgs && !E.tried) build_gamma_elim(A, s->nb, E);
  const bool e_active = !mgs && E.active;
  // The plain warm path (no row left out: diphasic systems, interfaces with Robin / Neumann conditions and no border rows)
  // takes the extrapolated start as well, on one rank: the kept products are products of whole states whatever the data do,
  // so steps with changing data qualify too.
  const bool single = ctx().nranks == 1 && !ctx().comm;
  const int which = (&A == &s->A_ctor) ? 0 : 1;
  if (single && !e_active) guess_policy(s->plain_guess_on[which], s->plain_last_products[which], (double)A.spmv_bytes);
  const GuessPlan gp = guess_prepare(s, &A, single && !e_active && s->plain_guess_on[which], s->plain_last_products[which], stream);
#define PG_RHS_INIT(KHV)                                                                                                          \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rhs_init<KHV>), dim3(w.grid), dim3(BLOCK), 0, stream, n, s->nb.n_vec(), scheme, s->z.p,     \
                     s->y.p, A.ds.p, s->mass.p, s->bconst.p, s->fixed.p, A.isblk.p, s->b.p, w.r.p, w.rhat.p, w.p.p, w.partials.p, \
                     gp.ga)
  switch (gp.KH) {
    case 1: PG_RHS_INIT(1); break;
    case 2: PG_RHS_INIT(2); break;
    case 3: PG_RHS_INIT(3); break;
    case 4: PG_RHS_INIT(4); break;
    default: PG_RHS_INIT(0); break;
  }
#undef PG_RHS_INIT
  PG_HIP(hipGetLastError());
  guess_after_rhs(s, gp, n, nullptr, (const double*)A.ds.p, (const double*)w.rhat.p, true, w, stream);
  KrylovCall call;
  call.preinit = true;
  if (e_active) {
    gamma_fix(E, s->z.p, w.r.p, w.rhat.p, w.p.p, w.partials.p, w.grid, stream);
    // the sub-matrix carries Gershgorin's verdict on Â but no spectral estimate: PG_PRECOND_POLY_EST is precond = 0 here (the
    // polynomial where Gershgorin admits, the plain loop where it refuses -- DESIGN.md section 16)
    pg_krylov_opts oe = o;
    if (oe.precond == PG_PRECOND_POLY_EST) oe.precond = 0;
    krylov_solve(E.A, E.nb, s->slab, s->b.p, s->z.p, w, oe, st, call);
  } else {
    // y0 = z (in place), r0 = b̂ - ŷ: same solution as a zero start, fewer iterations
    if (mgs) call.mg = &mg_step_ensure(s, A);
    krylov_solve(A, s->nb, s->slab, s->b.p, s->z.p, w, o, st, call);
    s->plain_last_products[which] = (double)st.products;
    guess_commit(s, gp, &A);
  }
  s->x_valid = false;
}

// The cold step (and IDR(s)'s warm one): the right-hand side from the unscaled state, the solve from zero or from x0 / Ax0.
void step_cold(pg_solver* s, int scheme, const pg_krylov_opts& o, const CsrMatrix& A, bool mgs, SolveStats& st) {
  hipStream_t stream = ctx().stream;
  const i64 n = s->nb.n_own;
  // cold start / CG: the reference's zero initial guess, on the unscaled state
  s->hist_cnt = 0;
  materialize_x(s);
  // IDR(s) starts from the previous state here too (krylov_solve's x0 / Ax0): the scaled state and one product, which CN takes anyway
  const bool idr_warm = o.warm_start != 0 && o.method == PG_METHOD_IDRS && n > 0;
  if (n > 0) {
    if (scheme == PG_SCHEME_CN || idr_warm) {
      hipLaunchKernelGGL(k_scale_state, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, stream, n, A.ds.p, s->x.p, s->z.p, 1);
      spmv_halo(A, s->nb, s->slab, s->z.p, s->y.p, stream);
    }
    hipLaunchKernelGGL(k_rhs, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, stream, n, scheme, s->x.p, s->y.p, A.ds.p, s->mass.p,
                       s->bconst.p, s->fixed.p, s->b.p);
    if (A.n_blk > 0 && s->nphase == 2 && scheme == PG_SCHEME_CN)
      launch_rhs_block_mf(s, scheme, A, stream);
    else if (A.n_blk > 0)
      hipLaunchKernelGGL(k_rhs_block, dim3(grid_for(A.n_blk, BLOCK)), dim3(BLOCK), 0, stream, A.n_blk, scheme, A.blk_rows.p,
                         A.blk_idx.p, A.blk_coef.p, A.blk_cn.p, s->x.p, (const double*)nullptr, s->y.p, s->mass.p,
                         s->bconst.p, s->fixed.p, s->b.p);
    PG_HIP(hipGetLastError());
  }
  KrylovCall call;
  if (mgs) call.mg = &mg_step_ensure(s, A);
  if (idr_warm) { call.x0 = s->z.p; call.Ax0 = s->y.p; }
  krylov_solve(A, s->nb, s->slab, s->b.p, s->ysol.p, s->work, o, st, call);
  std::swap(s->z.p, s->ysol.p);
  s->z_matrix = &A;
  s->x_valid = false;
}

void do_step(pg_solver* s, int scheme, const pg_krylov_opts* opts, SolveStats& st) {
  PG_REQUIRE(s->scheme_ctor != PG_SCHEME_STEADY, "a steady solver has no time loop");
  PG_REQUIRE(!s->moving, "a moving-body solver is one space-time step: create the next one from the next time slab");
  PG_REQUIRE(s->initial_done, "Solver is not initialized. Call pg_solver_initial_solve first.");
  const pg_krylov_opts o = opts ? *opts : default_opts();
  if (mg_is_precond(o.precond)) mg_conditions(s, o.method, mg_rule_of(o.precond));   // (refuses: a time step is an unsteady system)
  // PG_PRECOND_MG_STEP: its conditions and the hierarchy of this step's matrix before the step consumes anything (time, a row of
  // the coefficient table) -- a refusal, the set-up's included, leaves the solver where it was
  const bool mgs = mg_is_step(o.precond);
  if (mgs) {
    mg_step_conditions(s, o.method);
    ensure_run_matrix(s, scheme);
    mg_step_ensure(s, run_matrix(s));
  }
  // time-separable data: this step's row of the coefficient table -- never an older one
  for (const auto& t : s->td) {
    PG_REQUIRE(t.K == 0 || s->td_cursor < t.nrows,
               "time-separable data: this step is past the last row of the coefficient table (" + std::to_string(t.nrows) +
               " rows, all consumed); install a longer table with pg_solver_set_separable");
    for (const auto& pr : t.progs)
      PG_REQUIRE(s->td_cursor < pr.nrows,
                 "device function: this step is past the last row of the table of times (" + std::to_string(pr.nrows) +
                 " rows, all consumed); install a longer table with pg_solver_set_program");
  }
  if (td_installed(s)) s->td_row = s->td_cursor++;
  hipStream_t stream = ctx().stream;
  ensure_run_matrix(s, scheme);
  const CsrMatrix& A = run_matrix(s);
  specest_prepare(s, A, o);
  const i64 n = s->nb.n_own;
  const bool warm = o.warm_start != 0 && o.method == PG_METHOD_BICGSTAB && n > 0;
  const DiagElim* used_de = nullptr;   // the compact path taken in this step (its "quiet" bookkeeping stays valid)
  struct QuietGuard {                  // any other path moves z behind the compact path's back
    pg_solver* s; const DiagElim*& used;
    ~QuietGuard() {
      if (used != &s->diag_ctor) s->diag_ctor.snapped_version = -1;
      if (used != &s->diag_run) s->diag_run.snapped_version = -1;
    }
  } quiet_guard{s, used_de};
  s->t += s->dt;                     // diffusion.jl:287
  s->rc_last = nullptr;
  ensure_bconst(s, scheme);
  if (warm) {
    // loop form on the scaled state: z is the previous Krylov solution itself
    if (s->z_matrix != &A) {         // the matrix (hence S) changed since z was computed: BE ctor system -> CN run system
      hipLaunchKernelGGL(k_rescale_state, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, stream, n, s->z_matrix->ds.p, A.ds.p, s->z.p);
      s->z_matrix = &A;
    }
    // ŷ = Â z = B⁻¹S A x: CN right-hand side and warm-start residual -- unless the previous step has queued it already
    const bool have_y = s->spec_y_valid && s->spec_matrix == &A;
    s->spec_y_valid = false;
    if (!have_y) spmv_halo(A, s->nb, s->slab, s->z.p, s->y.p, stream);
    launch_rhs_block(s, scheme, A, stream);
    // rows alone on their diagonal (interface AND border identity rows) left out, compact vectors (pg_reduce.hip, DiagElim)
    DiagElim& DE = (&A == &s->A_ctor) ? s->diag_ctor : s->diag_run;
    // (PG_PRECOND_MG_STEP iterates on the full system: neither the compact system nor the γ elimination starts)
    if (!mgs && !DE.tried) build_diag_elim(A, s->nb, s->slab, DE);
    if (!mgs && DE.active && krylov_uses_polynomial(DE.A, o)) step_compact(s, scheme, o, A, DE, used_de, st);
    else step_warm(s, scheme, o, A, mgs, st);
  } else step_cold(s, scheme, o, A, mgs, st);
  s->steps_done += 1;
}

}  // namespace

extern "C" {

// What a solver constructor is asked to build.  Every pg_solver_create_* below fills one of these, and create_solver is the
// one place that checks it, fills the pg_solver and assembles.
struct SolverSpec {
  const char* entry;                          // the entry point that was called (error texts)
  int nphase = 1;
  pg_capacity* cap[2] = {nullptr, nullptr};   // per phase
  pg_diffops* ops[2] = {nullptr, nullptr};
  const double* D[2] = {nullptr, nullptr};
  const double* f_n[2] = {nullptr, nullptr};
  const double* f_np1[2] = {nullptr, nullptr};
  const pg_bc_desc* bc_interface = nullptr;   // one phase
  const pg_jump_desc* ic = nullptr;           // two phases
  const pg_border_desc* borders = nullptr;
  int32_t nborders = 0;
  double dt = 1.0;
  const double* T0 = nullptr;                 // the initial state on the host (NULL = zeros) ...
  pg_solver* previous = nullptr;              // ... and / or a solved solver whose state is taken on the device
  int32_t scheme = PG_SCHEME_BE;              // the caller's BE / CN; not read when ...
  bool steady = false;                        // ... the steady blocks are asked for
  bool moving = false, advdiff = false, stefan = false;
  // one phase, set by a composite handle that keeps its data on the device (pg_streamvort.hip): D, sources and interface values
  // as Mloc doubles each in the local layout, copied device to device; they take the place of the host arrays above
  const pg::SolverDeviceData* dev = nullptr;
  bool solved_once = false;                   // the system is solved once and replaced (as a slab of the moving solvers)
  pg_solver** out = nullptr;
};

static int32_t create_solver(const SolverSpec& d) {
  PG_API_BEGIN
  require_init();
  const std::string who = std::string(d.entry) + ": ";
  const bool mono = d.nphase == 1;
  // one solver per time slab: the stream-ordered allocator, freed blocks are reused without synchronisation (pg_common.h)
  std::unique_ptr<AsyncAllocScope> pool(d.moving ? new AsyncAllocScope() : nullptr);
  PG_REQUIRE(d.steady || d.scheme == PG_SCHEME_BE || d.scheme == PG_SCHEME_CN, who + "scheme must be BE or CN");
  PG_REQUIRE(d.out && (mono ? d.bc_interface != nullptr : d.ic != nullptr), who + "NULL argument");
  for (int q = 0; q < d.nphase; ++q) {
    PG_REQUIRE(d.cap[q] && d.ops[q], who + "NULL argument");
    PG_REQUIRE(d.ops[q]->cap == d.cap[q], who + "operators were built from a different capacity");
  }
  if (!mono) {
    PG_REQUIRE(d.cap[0]->mesh == d.cap[1]->mesh, "Phase capacities must share the same mesh.");
    PG_REQUIRE(d.cap[0]->slab.p0 == d.cap[1]->slab.p0 && d.cap[0]->slab.p1 == d.cap[1]->slab.p1,
               who + "phase capacities must share the slab partition");
  }
  if (d.moving) {
    for (int q = 0; q < d.nphase; ++q) {
      PG_REQUIRE(d.cap[q]->spacetime, who + "every phase needs a space-time capacity (pg_capacity_create_spacetime)");
      if (d.advdiff)
        PG_REQUIRE(d.ops[q]->st_velocity, who + "the moving advection-diffusion solver needs the ConvectionOps of its "
                   "space-time capacity (pg_diffops_set_velocity_spacetime)");
      else
        PG_REQUIRE(!d.ops[q]->has_velocity, who + "the moving diffusion solver takes no convection operators");
    }
    PG_REQUIRE(ctx().nranks == 1 && !ctx().comm, who + "space-time steps are single-rank");
    PG_REQUIRE(!d.previous || d.previous->initial_done, who + "the previous slab has not been solved");
  } else {
    PG_REQUIRE(d.dt > 0.0, who + "dt must be positive");
    if (d.previous) {           // a time step built as a new solver: the state of the step before, handed over on the device
      PG_REQUIRE(!d.steady, who + "a steady solver has no previous state");
      PG_REQUIRE(ctx().nranks == 1 && !ctx().comm, who + "a state is handed from solver to solver on one rank only");
      PG_REQUIRE(d.previous->initial_done, who + "the previous solver has not been solved");
    }
  }
  auto* s = new pg_solver();
  std::unique_ptr<pg_solver> guard(s);
  s->nphase = d.nphase;
  s->slab = d.cap[0]->slab;
  s->dt = d.moving ? 1.0 : d.dt;            // moving: Δt is inside the space-time capacities
  s->moving = d.moving;
  s->advdiff = d.advdiff;
  s->stefan = d.stefan;
  s->scheme_ctor = d.steady ? PG_SCHEME_STEADY : d.scheme;
  const i64 Ml = s->slab.Mloc();
  for (int q = 0; q < d.nphase; ++q) {
    s->cap[q] = d.cap[q];
    s->ops[q] = d.ops[q];
    s->convection = s->convection || (d.ops[q] && d.ops[q]->has_velocity);
    if (d.moving) {
      s->psi_p[q].alloc(Ml);
      s->psi_m[q].alloc(Ml);
      if (d.advdiff) {
        s->psi_cp[q].alloc(Ml);
        s->psi_cm[q].alloc(Ml);
      }
      hipLaunchKernelGGL(k_psi, dim3(grid_for(Ml, BLOCK)), dim3(BLOCK), 0, ctx().stream, Ml, (int)d.scheme, d.cap[q]->Vt[0].p,
                         d.cap[q]->Vt[1].p, s->psi_p[q].p, s->psi_m[q].p, s->psi_cp[q].p, s->psi_cm[q].p);
      PG_HIP(hipGetLastError());
    }
    if (d.D[q]) upload_local(s->Id[q], d.D[q], s->slab);
    if (d.f_np1[q]) upload_local(s->f_np1[q], d.f_np1[q], s->slab);
    if (d.f_n[q]) upload_local(s->f_n[q], d.f_n[q], s->slab);
  }
  if (d.dev) {
    PG_REQUIRE(mono, who + "device-resident data: one phase only");
    auto take = [&](DevBuf<double>& dst, const double* src) {
      if (!src) return;
      dst.alloc(Ml);
      PG_HIP(hipMemcpyAsync(dst.p, src, sizeof(double) * (size_t)Ml, hipMemcpyDeviceToDevice, ctx().stream));
    };
    take(s->Id[0], d.dev->D);
    take(s->f_n[0], d.dev->f_n);
    take(s->f_np1[0], d.dev->f_np1);
  }
  // the descriptor is copied, its arrays go to the device: their host memory dies with the call
  if (mono) {
    s->bc_i = *d.bc_interface;
    if (d.bc_interface->value_array) {
      upload_local(s->g_np1, d.bc_interface->value_array, s->slab);
      upload_local(s->g_n, d.bc_interface->value_array, s->slab);
    }
    s->bc_i.value_array = nullptr;
    if (d.dev && d.dev->g_np1) {
      s->g_np1.alloc(Ml);
      s->g_n.alloc(Ml);
      PG_HIP(hipMemcpyAsync(s->g_np1.p, d.dev->g_np1, sizeof(double) * (size_t)Ml, hipMemcpyDeviceToDevice, ctx().stream));
      PG_HIP(hipMemcpyAsync(s->g_n.p, d.dev->g_n ? d.dev->g_n : d.dev->g_np1, sizeof(double) * (size_t)Ml, hipMemcpyDeviceToDevice,
                            ctx().stream));
    }
  } else {
    s->ic = *d.ic;
    if (d.ic->g_array) upload_local(s->g_arr, d.ic->g_array, s->slab);
    if (d.ic->h_array) upload_local(s->h_arr, d.ic->h_array, s->slab);
    s->ic.g_array = s->ic.h_array = nullptr;
  }
  s->init_from = d.previous;                // consumed by setup_common after T0: its active unknowns overwrite T0's
  s->A_ctor.want_units = !d.moving && !d.solved_once;
  s->solved_once = d.solved_once;
  setup_common(s, d.borders, d.nborders, d.T0);
  *d.out = guard.release();
  PG_API_END
}

static SolverSpec spec_mono(const char* entry, pg_capacity* c, pg_diffops* o, const pg_bc_desc* bc_interface,
                            const pg_border_desc* borders, int32_t nborders, const double* Dcoef, const double* f_n,
                            const double* f_np1, pg_solver** out) {
  SolverSpec d;
  d.entry = entry;
  d.cap[0] = c; d.ops[0] = o; d.D[0] = Dcoef; d.f_n[0] = f_n; d.f_np1[0] = f_np1;
  d.bc_interface = bc_interface;
  d.borders = borders; d.nborders = nborders;
  d.out = out;
  return d;
}

static SolverSpec spec_diph(const char* entry, pg_capacity* c1, pg_diffops* o1, pg_capacity* c2, pg_diffops* o2,
                            const pg_jump_desc* ic, const pg_border_desc* borders, int32_t nborders, const double* D1,
                            const double* D2, const double* f1_n, const double* f1_np1, const double* f2_n,
                            const double* f2_np1, pg_solver** out) {
  SolverSpec d;
  d.entry = entry;
  d.nphase = 2;
  d.cap[0] = c1; d.ops[0] = o1; d.D[0] = D1; d.f_n[0] = f1_n; d.f_np1[0] = f1_np1;
  d.cap[1] = c2; d.ops[1] = o2; d.D[1] = D2; d.f_n[1] = f2_n; d.f_np1[1] = f2_np1;
  d.ic = ic;
  d.borders = borders; d.nborders = nborders;
  d.out = out;
  return d;
}

int32_t pg_solver_create_unsteady_mono(pg_capacity* c, pg_diffops* o, const pg_bc_desc* bc_interface,
                                       const pg_border_desc* borders, int32_t nborders, const double* Dcoef,
                                       const double* source, double dt, const double* T0, int32_t scheme,
                                       pg_solver** out) {
  SolverSpec d = spec_mono("pg_solver_create_unsteady_mono", c, o, bc_interface, borders, nborders, Dcoef, nullptr, source, out);
  d.dt = dt; d.T0 = T0; d.scheme = scheme;
  return create_solver(d);
}

int32_t pg_solver_create_steady_mono(pg_capacity* c, pg_diffops* o, const pg_bc_desc* bc_interface,
                                     const pg_border_desc* borders, int32_t nborders, const double* Dcoef,
                                     const double* source, pg_solver** out) {
  SolverSpec d = spec_mono("pg_solver_create_steady_mono", c, o, bc_interface, borders, nborders, Dcoef, nullptr, source, out);
  d.steady = true;
  return create_solver(d);
}

int32_t pg_solver_create_moving_mono(pg_capacity* c, pg_diffops* o, const pg_bc_desc* bc_interface,
                                     const pg_border_desc* borders, int32_t nborders, const double* Dcoef,
                                     const double* source_n, const double* source_np1, const double* T_prev,
                                     pg_solver* previous, int32_t scheme, pg_solver** out) {
  SolverSpec d = spec_mono("pg_solver_create_moving_mono", c, o, bc_interface, borders, nborders, Dcoef, source_n, source_np1, out);
  d.moving = true;
  d.T0 = T_prev; d.previous = previous; d.scheme = scheme;
  return create_solver(d);
}

// MovingAdvDiffusionUnsteadyMono + A_/b_mono_unstead_advdiff_moving of one slab   prescribedmotionsolver/advectiondiffusion.jl:15-33,
// 64-199: the moving blocks with the convection of the space-time ConvectionOps o (pg_diffops_set_velocity_spacetime)
int32_t pg_solver_create_moving_advdiff_mono(pg_capacity* c, pg_diffops* o, const pg_bc_desc* bc_interface,
                                             const pg_border_desc* borders, int32_t nborders, const double* Dcoef,
                                             const double* source_n, const double* source_np1, const double* T_prev,
                                             pg_solver* previous, int32_t scheme, pg_solver** out) {
  SolverSpec d = spec_mono("pg_solver_create_moving_advdiff_mono", c, o, bc_interface, borders, nborders, Dcoef, source_n,
                           source_np1, out);
  d.moving = d.advdiff = true;
  d.T0 = T_prev; d.previous = previous; d.scheme = scheme;
  return create_solver(d);
}

int32_t pg_solver_create_unsteady_diph(pg_capacity* c1, pg_diffops* o1, pg_capacity* c2, pg_diffops* o2,
                                       const pg_jump_desc* ic, const pg_border_desc* borders, int32_t nborders,
                                       const double* D1, const double* D2, const double* f1, const double* f2, double dt,
                                       const double* T0, int32_t scheme, pg_solver** out) {
  SolverSpec d = spec_diph("pg_solver_create_unsteady_diph", c1, o1, c2, o2, ic, borders, nborders, D1, D2, nullptr, f1, nullptr,
                           f2, out);
  d.dt = dt; d.T0 = T0; d.scheme = scheme;
  return create_solver(d);
}

int32_t pg_solver_create_steady_diph(pg_capacity* c1, pg_diffops* o1, pg_capacity* c2, pg_diffops* o2,
                                     const pg_jump_desc* ic, const pg_border_desc* borders, int32_t nborders,
                                     const double* D1, const double* D2, const double* f1, const double* f2,
                                     pg_solver** out) {
  SolverSpec d = spec_diph("pg_solver_create_steady_diph", c1, o1, c2, o2, ic, borders, nborders, D1, D2, nullptr, f1, nullptr, f2,
                           out);
  d.steady = true;
  return create_solver(d);
}

// MovingDiffusionUnsteadyDiph + A_/b_diph_unstead_diff_moving of one slab      prescribedmotionsolver/diffusion.jl:272-498
int32_t pg_solver_create_moving_diph(pg_capacity* c1, pg_diffops* o1, pg_capacity* c2, pg_diffops* o2, const pg_jump_desc* ic,
                                     const pg_border_desc* borders, int32_t nborders, const double* D1, const double* D2,
                                     const double* f1_n, const double* f1_np1, const double* f2_n, const double* f2_np1,
                                     const double* T_prev, pg_solver* previous, int32_t scheme, pg_solver** out) {
  SolverSpec d = spec_diph("pg_solver_create_moving_diph", c1, o1, c2, o2, ic, borders, nborders, D1, D2, f1_n, f1_np1, f2_n,
                           f2_np1, out);
  d.moving = true;
  d.T0 = T_prev; d.previous = previous; d.scheme = scheme;
  return create_solver(d);
}

// MovingAdvDiffusionUnsteadyDiph + A_/b_diph_unstead_advdiff_moving of one slab   prescribedmotionsolver/advectiondiffusion.jl:246-507
int32_t pg_solver_create_moving_advdiff_diph(pg_capacity* c1, pg_diffops* o1, pg_capacity* c2, pg_diffops* o2,
                                             const pg_jump_desc* ic, const pg_border_desc* borders, int32_t nborders,
                                             const double* D1, const double* D2, const double* f1_n, const double* f1_np1,
                                             const double* f2_n, const double* f2_np1, const double* T_prev,
                                             pg_solver* previous, int32_t scheme, pg_solver** out) {
  SolverSpec d = spec_diph("pg_solver_create_moving_advdiff_diph", c1, o1, c2, o2, ic, borders, nborders, D1, D2, f1_n, f1_np1,
                           f2_n, f2_np1, out);
  d.moving = d.advdiff = true;
  d.T0 = T_prev; d.previous = previous; d.scheme = scheme;
  return create_solver(d);
}

// MovingLiquidDiffusionUnsteadyDiph + A_/b_diph_unstead_diff_moving_stef of one slab   liquidmotionsolver/diffusion.jl:445-673:
// the moving diphasic blocks with row block 4 = [0 0 0 Iα₂], b₂ = b₄ = gᵧ and, under CN, -½ Id GᵀWꜝH Tγ without Ψ in b₁ / b₃
int32_t pg_solver_create_moving_stefan_diph(pg_capacity* c1, pg_diffops* o1, pg_capacity* c2, pg_diffops* o2,
                                            const pg_jump_desc* ic, const pg_border_desc* borders, int32_t nborders,
                                            const double* D1, const double* D2, const double* f1_n, const double* f1_np1,
                                            const double* f2_n, const double* f2_np1, const double* T_prev,
                                            pg_solver* previous, int32_t scheme, pg_solver** out) {
  SolverSpec d = spec_diph("pg_solver_create_moving_stefan_diph", c1, o1, c2, o2, ic, borders, nborders, D1, D2, f1_n, f1_np1,
                           f2_n, f2_np1, out);
  d.moving = d.stefan = true;
  d.T0 = T_prev; d.previous = previous; d.scheme = scheme;
  return create_solver(d);
}

int32_t pg_solver_destroy(pg_solver* s) {
  PG_API_BEGIN
  delete s;
  PG_API_END
}

int32_t pg_solver_set_source(pg_solver* s, int32_t phase, const double* f_n, const double* f_np1) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && phase >= 0 && phase < s->nphase, "pg_solver_set_source: bad arguments");
  td_clear(s, phase);
  if (f_n) upload_local(s->f_n[phase], f_n, s->slab);
  if (f_np1) upload_local(s->f_np1[phase], f_np1, s->slab);
  s->bconst_dirty = true;
  if (!s->initial_done) build_first_rhs(s);
  PG_API_END
}

int32_t pg_solver_set_interface_value(pg_solver* s, const double* g_n, const double* g_np1) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && s->nphase == 1, "pg_solver_set_interface_value: monophasic solver expected");
  td_clear(s, 2);
  if (g_n) upload_local(s->g_n, g_n, s->slab);
  if (g_np1) upload_local(s->g_np1, g_np1, s->slab);
  s->bconst_dirty = true;
  if (!s->initial_done) build_first_rhs(s);
  PG_API_END
}

int32_t pg_solver_set_border_values(pg_solver* s, const double* values) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && values, "pg_solver_set_border_values: NULL argument");
  td_clear(s, 3);
  const i64 nb = ensure_border_cells(s);
  DevBuf<double> dv(nb);
  dv.upload(values, nb);
  hipLaunchKernelGGL(k_set_border_values, dim3(grid_for(nb, BLOCK)), dim3(BLOCK), 0, ctx().stream, nb, s->border_cells_lin.p,
                     dv.p, s->slab.first_cell(), s->Mloc, s->nphase, s->nb.red.p, s->nb.n_own, s->bcv.p);
  PG_HIP(hipGetLastError());
  PG_HIP(hipStreamSynchronize(ctx().stream));
  s->bconst_dirty = true;
  if (!s->initial_done) build_first_rhs(s);
  PG_API_END
}

static int td_slot_of(const pg_solver* s, int32_t which, int32_t phase, const char* entry) {
  const std::string who = std::string(entry) + ": ";
  PG_REQUIRE(s, who + "NULL solver");
  PG_REQUIRE(which == PG_TD_SOURCE || which == PG_TD_INTERFACE || which == PG_TD_BORDER,
             who + "which must be PG_TD_SOURCE, PG_TD_INTERFACE or PG_TD_BORDER");
  if (which == PG_TD_SOURCE) {
    PG_REQUIRE(phase >= 0 && phase < s->nphase, who + "a source belongs to phase 0 (or 1 of a diphasic solver)");
    return phase;
  }
  PG_REQUIRE(phase == 0, who + "phase must be 0 for PG_TD_INTERFACE and PG_TD_BORDER");
  return which == PG_TD_INTERFACE ? 2 : 3;
}

int32_t pg_solver_set_separable(pg_solver* s, int32_t which, int32_t phase, int32_t K, const double* modes, int64_t nrows,
                                const double* coef) {
  PG_API_BEGIN
  require_init();
  const std::string who = "pg_solver_set_separable refused: ";
  const int slot = td_slot_of(s, which, phase, "pg_solver_set_separable");
  PG_REQUIRE(K >= 1, who + "K must be at least 1");
  PG_REQUIRE(K <= PG_TD_MAX_TERMS, who + "more than " + std::to_string((int)PG_TD_MAX_TERMS) + " terms (K = " +
             std::to_string(K) + ")");
  PG_REQUIRE(modes && coef && nrows >= 1, who + "modes, coef and at least one table row are needed");
  PG_REQUIRE(s->scheme_ctor != PG_SCHEME_STEADY, who + "a steady solver has no time loop");
  PG_REQUIRE(!s->moving && !s->stefan, who + "moving-body and Stefan solvers are one space-time step each");
  PG_REQUIRE(!(which == PG_TD_INTERFACE && s->nphase == 2),
             who + "PG_TD_INTERFACE on a diphasic solver (its jump rows carry no time)");
  PG_REQUIRE(ctx().nranks == 1 && !ctx().comm, who + "it runs on one rank only (virtual ranks included)");
  PG_REQUIRE(s->initial_done, who + "install after pg_solver_initial_solve (the constructor's system takes its data from the host)");
  hipStream_t st = ctx().stream;
  const i64 n = s->nb.n_own;
  pg_solver::TdSlot& t = s->td[slot];
  td_clear(s, slot);
  const i64 nb = which == PG_TD_BORDER ? ensure_border_cells(s) : 0;
  DevBuf<double> field;                        // one spatial part at a time: the padded field does not stay
  if (which == PG_TD_BORDER) field.alloc(nb > 0 ? nb : 1);
  for (int k = 0; k < K; ++k) {
    t.mode[k].alloc(n > 0 ? n : 1);
    t.mode[k].zero();
    if (n <= 0) continue;
    if (which == PG_TD_BORDER) {
      if (nb <= 0) continue;
      field.upload(modes + (i64)k * nb, nb);
      hipLaunchKernelGGL(k_td_border_rows, dim3(grid_for(nb, BLOCK)), dim3(BLOCK), 0, st, nb, s->border_cells_lin.p,
                         (const double*)field.p, s->slab.first_cell(), s->Mloc, s->nphase, s->nb.red.p, n, s->fixed.p,
                         t.mode[k].p);
    } else {
      upload_local(field, modes + (i64)k * s->M, s->slab);
      hipLaunchKernelGGL(k_td_mode, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, st, make_params(s, s->scheme_ctor), make_segs(s->nb),
                         n, s->nb.row_cell.p, (int)which, (int)phase, (const double*)field.p, s->fixed.p, t.mode[k].p);
    }
    PG_HIP(hipGetLastError());
    PG_HIP(hipStreamSynchronize(st));          // (field is overwritten by the next term)
  }
  t.coef.assign(coef, coef + (size_t)nrows * 2 * K);
  t.nrows = nrows;
  t.K = K;
  s->td_cursor = 0;
  s->td_row = -1;
  s->bconst_dirty = true;                      // td_base: k_bconst without this slot's own data
  PG_API_END
}

// a program into slot `slot` (border: for the cells of `key`, -1 every one): refusals, the list of its rows, the table
static void td_install_program(pg_solver* s, const std::string& who, int which, int phase, int slot, int key,
                               const pg_program* prog, int64_t nrows, const double* times) {
  std::string why;
  PG_REQUIRE(pgprog::program_validate(prog, &why), who + "invalid program: " + why);
  PG_REQUIRE(times && nrows >= 1, who + "times and at least one table row are needed");
  PG_REQUIRE(s->scheme_ctor != PG_SCHEME_STEADY, who + "a steady solver has no time loop");
  PG_REQUIRE(!s->moving && !s->stefan, who + "moving-body and Stefan solvers are one space-time step each");
  PG_REQUIRE(!(which == PG_TD_INTERFACE && s->nphase == 2),
             who + "PG_TD_INTERFACE on a diphasic solver (its jump rows carry no time)");
  PG_REQUIRE(ctx().nranks == 1 && !ctx().comm, who + "it runs on one rank only (virtual ranks included)");
  PG_REQUIRE(s->initial_done, who + "install after pg_solver_initial_solve (the constructor's system takes its data from the host)");
  const pg_capacity* cap = s->cap[which == PG_TD_SOURCE ? phase : 0];
  PG_REQUIRE(which != PG_TD_INTERFACE || cap->has_cg, who + "the capacity was built without C_gamma (PG_FLAG_NO_CENTROIDS)");
  const i64 n = s->nb.n_own;
  const i64 nb = which == PG_TD_BORDER ? ensure_border_cells(s) : 0;
  const i64 n_items = which == PG_TD_BORDER ? nb * s->nphase : n;
  PG_REQUIRE(n_items < ((i64)1 << 31), who + "more rows than the list's 32-bit positions hold");
  hipStream_t st = ctx().stream;                                        // (every refusal is above: what was installed stays until here)
  pg_solver::TdSlot& t = s->td[slot];
  if (t.K > 0 || which != PG_TD_BORDER || key < 0) td_clear(s, slot);   // separable terms, or the slot's one program, go
  for (size_t j = 0; j < t.progs.size(); ++j)                            // (border: the program of the same key, or of every key)
    if (t.progs[j].key == key || t.progs[j].key < 0) { t.progs.erase(t.progs.begin() + j); --j; }
  pg_solver::TdSlot::Prog pr;
  pr.prog = *prog;
  pr.key = key;
  const pg_mesh* m = s->cap[0]->mesh;
  const int N = m->N;
  const SysParams P = make_params(s, s->scheme_ctor);
  TdPointsArgs a{};
  a.which = which; a.phase = phase; a.nbulk = s->nphase; a.N = N;
  a.n_own = n; a.first_cell = s->slab.first_cell(); a.Mloc = s->Mloc;
  a.row_cell = s->nb.row_cell.p; a.red = s->nb.red.p; a.fixed = s->fixed.p;
  DevBuf<unsigned char> selected;
  DevBuf<double> centres;
  if (which == PG_TD_BORDER) {
    a.n_items = n_items;
    if (nb > 0) {
      std::vector<unsigned char> sel(nb);
      std::vector<double> pos((size_t)N * nb);
      for (i64 q = 0; q < nb; ++q) {
        sel[q] = key < 0 || m->border_key[q] == key;
        for (int d = 0; d < N; ++d) pos[(size_t)d * nb + q] = m->border_pos[q * N + d];
      }
      selected.alloc(nb); selected.upload(sel.data(), nb);
      centres.alloc((i64)N * nb); centres.upload(pos.data(), (i64)N * nb);
      for (int d = 0; d < N; ++d) a.pos[d] = centres.p + (i64)d * nb;
    }
    a.cells_global = s->border_cells_lin.p;
    a.selected = selected.p;
  } else {
    a.n_items = n_items;
    a.weight = which == PG_TD_SOURCE ? P.cap[phase].V : P.cap[0].G;
    for (int d = 0; d < N; ++d) a.pos[d] = which == PG_TD_SOURCE ? cap->Cw[d].p : cap->Cg[d].p;
  }
  if (a.n_items > 0) {
    DevBuf<unsigned char> flag(a.n_items);
    DevBuf<int> where(a.n_items), total(1);
    const RowSegs seg = make_segs(s->nb);
    hipLaunchKernelGGL(k_td_points_flag, dim3(grid_for(a.n_items, BLOCK)), dim3(BLOCK), 0, st, a, seg, flag.p);
    PG_HIP(hipGetLastError());
    scan_exclusive<unsigned char>(flag.p, where.p, a.n_items, total.p, st);
    int cnt = 0;
    total.download(&cnt, 1);
    pr.n = cnt;
    if (cnt > 0) {
      pr.row.alloc(cnt); pr.w.alloc(cnt);
      for (auto& p : pr.p) p.alloc(cnt);
      hipLaunchKernelGGL(k_td_points, dim3(grid_for(a.n_items, BLOCK)), dim3(BLOCK), 0, st, a, seg, (const int*)where.p, (i64)cnt,
                         pr.row.p, pr.w.p, pr.p[0].p, pr.p[1].p, pr.p[2].p);
      PG_HIP(hipGetLastError());
    }
    PG_HIP(hipStreamSynchronize(st));          // (flag, where, selected and centres go with this scope)
  }
  pr.times.assign(times, times + (size_t)nrows * 2);
  pr.nrows = nrows;
  t.progs.push_back(std::move(pr));
  s->td_cursor = 0;
  s->td_row = -1;
  s->bconst_dirty = true;                      // td_base: k_bconst without this slot's own data
}

int32_t pg_solver_set_program(pg_solver* s, int32_t which, int32_t phase, const pg_program* prog, int64_t nrows,
                              const double* times) {
  PG_API_BEGIN
  require_init();
  const int slot = td_slot_of(s, which, phase, "pg_solver_set_program");
  td_install_program(s, "pg_solver_set_program refused: ", which, phase, slot, -1, prog, nrows, times);
  PG_API_END
}

int32_t pg_solver_set_border_program(pg_solver* s, int32_t key, const pg_program* prog, int64_t nrows, const double* times) {
  PG_API_BEGIN
  require_init();
  const std::string who = "pg_solver_set_border_program refused: ";
  PG_REQUIRE(s, who + "NULL solver");
  PG_REQUIRE(key >= 0 && key < 6, who + "key must be one of PG_KEY_*");
  td_install_program(s, who, PG_TD_BORDER, 0, 3, key, prog, nrows, times);
  PG_API_END
}

int32_t pg_solver_program_info(const pg_solver* s, int32_t* programs, int64_t* entries, int64_t* nrows, int64_t* cursor) {
  PG_API_BEGIN
  PG_REQUIRE(s, "pg_solver_program_info: NULL solver");
  i64 rows = 0;
  auto take = [&](i64 r) { rows = rows == 0 ? r : std::min(rows, r); };
  for (int q = 0; q < 4; ++q) {
    i64 e = 0;
    if (s->td[q].K > 0) take(s->td[q].nrows);
    for (const auto& pr : s->td[q].progs) { e += pr.n; take(pr.nrows); }
    if (programs) programs[q] = (int32_t)s->td[q].progs.size();
    if (entries) entries[q] = e;
  }
  if (nrows) *nrows = rows;
  if (cursor) *cursor = s->td_cursor;
  PG_API_END
}

// measurement (scripts/bench_device_function.py): the evaluation of every installed program at the last step's times launched
// `repeats` times between two events.  It adds to a scratch vector, not to bconst: the solver's data stay what they were.
int32_t pg_debug_td_eval_ms(pg_solver* s, int32_t scheme, int32_t repeats, double* ms_per_eval, int64_t* entries,
                            int64_t* instructions) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && ms_per_eval && repeats >= 1, "pg_debug_td_eval_ms: bad arguments");
  PG_REQUIRE(scheme == PG_SCHEME_BE || scheme == PG_SCHEME_CN, "scheme must be BE or CN");
  PG_REQUIRE(s->td_row >= 0, "pg_debug_td_eval_ms: no step has consumed a row of the table yet");
  hipStream_t st = ctx().stream;
  const bool cn = scheme == PG_SCHEME_CN;
  DevBuf<double> sink(s->nb.n_own > 0 ? s->nb.n_own : 1);
  sink.zero();
  i64 ne = 0, ni = 0;
  auto once = [&](bool count) {
    for (int slot = 0; slot < 4; ++slot)
      for (const auto& pr : s->td[slot].progs) {
        PG_REQUIRE(s->td_row < pr.nrows, "pg_debug_td_eval_ms: no table row");
        const double t0 = pr.times[(size_t)2 * s->td_row], t1 = pr.times[(size_t)2 * s->td_row + 1];
        const double c0 = (slot != 3 && cn) ? s->dt / 2 : 0.0, c1 = slot == 3 ? 1.0 : cn ? s->dt / 2 : slot == 2 ? 1.0 : s->dt;
        td_eval_launch(pr.prog, pr.n, pr.row.p, pr.w.p, pr.p[0].p, pr.p[1].p, pr.p[2].p, c0, c1, t0, slot == 3 ? t0 : t1, sink.p, st);
        if (count) { ne += pr.n; ni += pr.n * pr.prog.n_ops * (c0 != 0.0 ? 2 : 1); }
      }
  };
  once(true);
  PG_REQUIRE(ne > 0, "pg_debug_td_eval_ms: no program with listed rows is installed");
  EventPair ev;
  PG_HIP(hipEventRecord(ev.e0, st));
  for (int r = 0; r < repeats; ++r) once(false);
  PG_HIP(hipEventRecord(ev.e1, st));
  PG_HIP(hipEventSynchronize(ev.e1));
  float ms = 0.f;
  PG_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *ms_per_eval = (double)ms / repeats;
  if (entries) *entries = ne;
  if (instructions) *instructions = ni;
  PG_API_END
}

int32_t pg_solver_clear_separable(pg_solver* s, int32_t which, int32_t phase) {
  PG_API_BEGIN
  require_init();
  td_clear(s, td_slot_of(s, which, phase, "pg_solver_clear_separable"));
  PG_API_END
}

int32_t pg_solver_time_data_info(const pg_solver* s, int32_t* terms, int64_t* nrows, int64_t* cursor) {
  PG_API_BEGIN
  PG_REQUIRE(s, "pg_solver_time_data_info: NULL solver");
  i64 rows = 0;
  for (int q = 0; q < 4; ++q) {
    if (terms) terms[q] = s->td[q].K;
    if (s->td[q].K > 0) rows = rows == 0 ? s->td[q].nrows : std::min(rows, s->td[q].nrows);
  }
  if (nrows) *nrows = rows;
  if (cursor) *cursor = s->td_cursor;
  PG_API_END
}

// measurement (scripts/bench_time_separable.py): the combine of the last step's table row launched `repeats` times between two
// events -- the same launches ensure_bconst queues, writing the same bconst again
int32_t pg_debug_td_combine_ms(pg_solver* s, int32_t scheme, int32_t repeats, double* ms_per_combine, int32_t* modes,
                               int64_t* bytes) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && ms_per_combine && repeats >= 1, "pg_debug_td_combine_ms: bad arguments");
  PG_REQUIRE(scheme == PG_SCHEME_BE || scheme == PG_SCHEME_CN, "scheme must be BE or CN");
  PG_REQUIRE(td_installed(s) && s->td_row >= 0, "pg_debug_td_combine_ms: no step has consumed a row of separable data yet");
  hipStream_t st = ctx().stream;
  int J = 0;
  for (const auto& t : s->td) J += t.K;
  td_bconst(s, scheme);                        // (td_base of this scheme, outside the timed region)
  s->bconst_scheme = scheme;
  s->bconst_dirty = false;
  ++s->bconst_version;
  EventPair ev;
  PG_HIP(hipEventRecord(ev.e0, st));
  for (int r = 0; r < repeats; ++r) td_bconst(s, scheme);
  PG_HIP(hipEventRecord(ev.e1, st));
  PG_HIP(hipEventSynchronize(ev.e1));
  float ms = 0.f;
  PG_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *ms_per_combine = (double)ms / repeats;
  if (modes) *modes = J;
  if (bytes) *bytes = (int64_t)(J + 2) * 8 * s->nb.n_own;
  PG_API_END
}

int32_t pg_solver_set_monitors(pg_solver* s, int32_t K, const int32_t* kinds, const double* weights, int64_t len) {
  PG_API_BEGIN
  require_init();
  const std::string who = "pg_solver_set_monitors refused: ";
  PG_REQUIRE(s, who + "NULL solver");
  PG_REQUIRE(K >= 1, who + "K must be at least 1");
  PG_REQUIRE(K <= PG_MON_MAX, who + "more than " + std::to_string((int)PG_MON_MAX) + " monitors (K = " + std::to_string(K) + ")");
  PG_REQUIRE(kinds && weights, who + "kinds and weights are needed");
  for (int m = 0; m < K; ++m)
    PG_REQUIRE(kinds[m] == PG_MON_SUM || kinds[m] == PG_MON_SUMSQ,
               who + "unknown kind " + std::to_string(kinds[m]) + " (PG_MON_SUM or PG_MON_SUMSQ)");
  PG_REQUIRE(len == (i64)s->K * s->M, who + "len must be 2M (mono) or 4M (diph), the length of pg_solver_get_state's vector");
  PG_REQUIRE(s->scheme_ctor != PG_SCHEME_STEADY, who + "a steady solver has no time loop");
  PG_REQUIRE(!s->moving && !s->stefan, who + "moving-body and Stefan solvers are one space-time step each");
  PG_REQUIRE(!s->solved_once, who + "the solvers of a stream-function - vorticity step are replaced every step");
  PG_REQUIRE(ctx().nranks == 1 && !ctx().comm && s->Mloc == s->M, who + "it runs on one rank only (virtual ranks included)");
  mon_clear(s);
  const i64 n = s->nb.n_own;
  // the weights in the solver's row numbering: row r is unknown (kind of r, cell of r) of the full vector, as k_scatter_active
  // places it -- unknowns that are no row (eliminated: the state is 0 there) drop out
  std::vector<int> row_cell((size_t)std::max<i64>(n, 1));
  if (n > 0) s->nb.row_cell.download(row_cell.data(), n);
  std::vector<std::vector<double>> wr((size_t)K, std::vector<double>((size_t)std::max<i64>(n, 1), 0.0));
  i64 nnz[PG_MON_MAX] = {};
  for (int m = 0; m < K; ++m) {
    const double* w = weights + (i64)m * len;
    for (int k = 0; k < s->nb.K; ++k) {
      const i64 r_end = k + 1 < s->nb.K ? s->nb.off_own[k + 1] : n;
      for (i64 r = s->nb.off_own[k]; r < r_end; ++r) {
        const double v = w[(i64)k * s->M + row_cell[(size_t)r]];
        wr[(size_t)m][(size_t)r] = v;
        if (v != 0.0) ++nnz[m];
      }
    }
  }
  pg_solver::Monitors& M = s->mon;
  mon_choose_storage(n, K, nnz, M.sparse);
  for (int m = 0; m < K; ++m) {
    M.kind[m] = kinds[m];
    if (!M.sparse[m]) {
      M.w[m].alloc(std::max<i64>(n, 1));
      M.w[m].upload(wr[(size_t)m].data(), n);
      M.stored[m] = n;
      continue;
    }
    std::vector<int> rows;
    std::vector<double> vals;
    for (i64 r = 0; r < n; ++r)
      if (wr[(size_t)m][(size_t)r] != 0.0) { rows.push_back((int)r); vals.push_back(wr[(size_t)m][(size_t)r]); }
    M.row[m].alloc(std::max<i64>((i64)rows.size(), 1));
    M.w[m].alloc(std::max<i64>((i64)rows.size(), 1));
    M.row[m].upload(rows.data(), (i64)rows.size());
    M.w[m].upload(vals.data(), (i64)vals.size());
    M.stored[m] = (i64)rows.size();
  }
  M.G = (int)std::min<i64>(MON_MAX_BLOCKS, std::max<i64>(1, (n + MON_ROWS_PER_BLOCK - 1) / MON_ROWS_PER_BLOCK));
  M.K = K;
  PG_API_END
}

int32_t pg_solver_clear_monitors(pg_solver* s) {
  PG_API_BEGIN
  PG_REQUIRE(s, "pg_solver_clear_monitors: NULL solver");
  mon_clear(s);
  PG_API_END
}

int32_t pg_solver_monitor_info(const pg_solver* s, int32_t* K, int64_t* rows, int32_t* sparse, int64_t* stored) {
  PG_API_BEGIN
  PG_REQUIRE(s, "pg_solver_monitor_info: NULL solver");
  if (K) *K = s->mon.K;
  if (rows) *rows = s->mon.rows;
  for (int m = 0; m < PG_MON_MAX; ++m) {
    if (sparse) sparse[m] = m < s->mon.K && s->mon.sparse[m] ? 1 : 0;
    if (stored) stored[m] = m < s->mon.K ? s->mon.stored[m] : 0;
  }
  PG_API_END
}

int32_t pg_solver_get_monitor_series(const pg_solver* s, int64_t row0, int64_t nrows, double* values, double* times) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && values, "pg_solver_get_monitor_series: NULL argument");
  const pg_solver::Monitors& M = s->mon;
  PG_REQUIRE(M.K > 0, "pg_solver_get_monitor_series: no monitors are installed");
  PG_REQUIRE(row0 >= 0 && nrows >= 0 && row0 <= M.rows && nrows <= M.rows - row0,
             "pg_solver_get_monitor_series: rows " + std::to_string((long long)row0) + " .. " +
             std::to_string((long long)(row0 + nrows)) + " asked for, the series has " + std::to_string((long long)M.rows));
  const i64 per_row = (i64)M.G * M.K;
  std::vector<double> part((size_t)std::max<i64>(nrows * per_row, 1));
  M.series.download(part.data(), nrows * per_row, row0 * per_row);
  for (i64 q = 0; q < nrows; ++q)
    for (int m = 0; m < M.K; ++m) {
      double v = 0.0;                              // the blocks' partials in the order of the blocks
      for (int g = 0; g < M.G; ++g) v += part[(size_t)((q * M.G + g) * M.K + m)];
      values[q * M.K + m] = v;
    }
  if (times)
    for (i64 q = 0; q < nrows; ++q) times[q] = M.times[(size_t)(row0 + q)];
  PG_API_END
}

int32_t pg_solver_drop_states(pg_solver* s) {
  PG_API_BEGIN
  PG_REQUIRE(s, "pg_solver_drop_states: NULL solver");
  s->states.clear();
  PG_API_END
}

// measurement (scripts/bench_monitors.py): the evaluation of the installed monitors on the current state launched `repeats`
// times between two events, into a scratch buffer -- the series does not grow
int32_t pg_debug_monitor_ms(pg_solver* s, int32_t repeats, double* ms_per_eval, int64_t* bytes) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && ms_per_eval && repeats >= 1, "pg_debug_monitor_ms: bad arguments");
  const pg_solver::Monitors& M = s->mon;
  PG_REQUIRE(M.K > 0 && s->initial_done, "pg_debug_monitor_ms: monitors and a solved state are needed");
  hipStream_t st = ctx().stream;
  DevBuf<double> out((i64)M.G * M.K);
  mon_launch(s, out.p, st);                    // (outside the timed region)
  EventPair ev;
  PG_HIP(hipEventRecord(ev.e0, st));
  for (int r = 0; r < repeats; ++r) mon_launch(s, out.p, st);
  PG_HIP(hipEventRecord(ev.e1, st));
  PG_HIP(hipEventSynchronize(ev.e1));
  float ms = 0.f;
  PG_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *ms_per_eval = (double)ms / repeats;
  if (bytes) {
    const i64 n = s->nb.n_own;
    i64 b = (i64)M.G * M.K * 8;
    bool any_dense = false;
    for (int m = 0; m < M.K; ++m) {
      if (M.sparse[m]) b += MON_SPARSE_ENTRY_BYTES * M.stored[m];
      else { b += 8 * n; any_dense = true; }
    }
    if (any_dense) b += (s->x_valid ? 8 : 16) * n;
    *bytes = b;
  }
  PG_API_END
}

// test support: the installed monitors evaluated once on the current state -- x when a state download has made it valid, else z
// and its scaling -- K values, the blocks' partials added as pg_solver_get_monitor_series adds them; the series is not touched
int32_t pg_debug_monitor_eval(pg_solver* s, double* values, int32_t* x_form) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && values, "pg_debug_monitor_eval: NULL argument");
  const pg_solver::Monitors& M = s->mon;
  PG_REQUIRE(M.K > 0 && s->initial_done, "pg_debug_monitor_eval: monitors and a solved state are needed");
  DevBuf<double> out((i64)M.G * M.K);
  mon_launch(s, out.p, ctx().stream);
  std::vector<double> part((size_t)M.G * M.K);
  out.download(part.data(), (i64)M.G * M.K);
  for (int m = 0; m < M.K; ++m) {
    double v = 0.0;
    for (int g = 0; g < M.G; ++g) v += part[(size_t)g * M.K + m];
    values[m] = v;
  }
  if (x_form) *x_form = s->x_valid ? 1 : 0;
  PG_API_END
}

int32_t pg_solver_initial_solve(pg_solver* s, const pg_krylov_opts* opts, pg_step_info* info) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s, "Solver is not initialized. Call a solver constructor first.");
  SolveStats st;
  std::unique_ptr<AsyncAllocScope> pool(s->moving ? new AsyncAllocScope() : nullptr);   // (work vectors allocated on first use)
  do_initial(s, opts, st);
  mon_record(s);
  fill_info(s, st, info);
  PG_API_END
}

int32_t pg_solver_step(pg_solver* s, int32_t scheme, const pg_krylov_opts* opts, pg_step_info* info) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s, "Solver is not initialized. Call a solver constructor first.");
  PG_REQUIRE(scheme == PG_SCHEME_BE || scheme == PG_SCHEME_CN, "scheme must be BE or CN");
  SolveStats st;
  do_step(s, scheme, opts, st);
  mon_record(s);
  fill_info(s, st, info);
  PG_API_END
}

int32_t pg_solver_run(pg_solver* s, double Tend, int32_t scheme, const pg_krylov_opts* opts, int32_t do_initial_flag,
                      int64_t max_steps, int32_t save_every, pg_run_info* info) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s, "Solver is not initialized. Call a solver constructor first.");
  PG_REQUIRE(scheme == PG_SCHEME_BE || scheme == PG_SCHEME_CN, "scheme must be BE or CN");
  hipStream_t stream = ctx().stream;
  EventPair ev;                     // destroyed on every exit path (do_step may throw)
  const auto t_run0 = std::chrono::steady_clock::now();
  const double wait0 = pg::g_host_wait_us;
  PG_HIP(hipEventRecord(ev.e0, stream));
  double used0 = 0.0;               // older states read by the extrapolated starts so far (device counter, GuessArgs)
  if (s->guess_coef.n >= 16) s->guess_coef.download(&used0, 1, 13);
  SolveStats tot;
  i64 steps = 0, iters = 0, unconverged = 0;
  double worst = 0.0;
  auto account = [&](const SolveStats& st) {
    iters += st.iters; tot.spmv_ms += st.spmv_ms; tot.spmv_launches += st.spmv_launches;
    tot.spmv_lean_ms += st.spmv_lean_ms; tot.spmv_lean_launches += st.spmv_lean_launches;
    tot.poly_degree = st.poly_degree;
    tot.poly_xspace = st.poly_xspace;
    tot.half_exit += st.half_exit;
    tot.products += st.products;
    tot.f32_launches += st.f32_launches; tot.f32_ms += st.f32_ms; tot.f32_timed += st.f32_timed;
    tot.f32_chains += st.f32_chains; tot.f32_tail_sum += st.f32_tail_sum;
    if (!st.converged) ++unconverged;
    if (st.bnorm > 0.0) worst = std::max(worst, st.resnorm / st.bnorm);
  };
  if (s->mon.K > 0) {               // the rows this call will record, counted on the loop's own clock (an open-ended run: a
    const i64 limit = 1 << 16;      // first 65 536, the doubling takes care of the rest)
    i64 rows = do_initial_flag ? 1 : 0, n = 0;
    for (double t = s->t; t < Tend && (max_steps < 0 || n < max_steps) && n < limit; t += s->dt) ++n;
    mon_reserve(s, rows + n);
  }
  if (do_initial_flag) {
    SolveStats st;
    do_initial(s, opts, st);
    mon_record(s);
    account(st);
    if (save_every > 0) keep_state(s);
  }
  while (s->t < Tend) {             // diffusion.jl:286
    if (max_steps >= 0 && steps >= max_steps) break;
    SolveStats st;
    s->hint_more_steps = (s->t + s->dt < Tend) && (max_steps < 0 || steps + 1 < max_steps);   // (another step follows this one)
    struct HintReset { pg_solver* s; ~HintReset() { s->hint_more_steps = false; } } hint_reset{s};
    do_step(s, scheme, opts, st);
    mon_record(s);
    account(st);
    ++steps;
    if (save_every > 0 && steps % save_every == 0) keep_state(s);
  }
  PG_HIP(hipEventRecord(ev.e1, stream));
  PG_HIP(hipEventSynchronize(ev.e1));
  float ms = 0.f;
  PG_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  if (config().debug && steps > 0) {
    const double wall_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_run0).count();
    fprintf(stderr, "[pg_solver_run] %lld steps: wall %.1f us per step, of which the host waited %.1f us for the device (the rest: queueing "
            "launches and bookkeeping); device time by events %.1f us per step\n", (long long)steps, wall_us / steps,
            (pg::g_host_wait_us - wait0) / steps, ms * 1e3 / steps);
  }
  if (info) {
    info->steps = steps;
    info->total_iters = iters;
    info->t_final = s->t;
    info->extremum = max_abs(s);
    info->solve_ms = ms;
    info->spmv_ms_total = tot.spmv_ms;
    info->spmv_launches = tot.spmv_launches;
    info->unconverged_steps = unconverged;
    info->worst_relres = worst;
    info->spmv_lean_ms_total = tot.spmv_lean_ms;
    info->spmv_lean_launches = tot.spmv_lean_launches;
    info->poly_degree = tot.poly_degree;
    info->poly_xspace = tot.poly_xspace;
    info->half_exits = tot.half_exit;
    info->products = tot.products;
    info->poly_f32_launches = tot.f32_launches;
    info->poly_f32_ms_total = tot.f32_ms;
    info->poly_f32_timed = tot.f32_timed;
    info->poly_f32_chains = tot.f32_chains;
    info->poly_f32_tail_sum = tot.f32_tail_sum;
    info->guess_states_read = 0;
    if (s->guess_coef.n >= 16) {
      double hc[16];
      s->guess_coef.download(hc, 16);
      info->guess_states_read = (int64_t)(hc[13] - used0);
    }
  }
  PG_API_END
}

int32_t pg_solver_num_states(const pg_solver* s, int64_t* out) {
  PG_API_BEGIN
  PG_REQUIRE(s && out, "pg_solver_num_states: NULL argument");
  *out = (int64_t)s->states.size();
  PG_API_END
}

int32_t pg_solver_get_state(const pg_solver* s, int64_t state_index, double* x, int64_t len) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && x, "pg_solver_get_state: NULL argument");
  PG_REQUIRE(len == (i64)s->K * s->M, "pg_solver_get_state: len must be 2M (mono) or 4M (diph)");
  if (state_index < 0) materialize_x(const_cast<pg_solver*>(s));
  const double* src = s->x.p;
  if (state_index >= 0) {
    PG_REQUIRE(state_index < (i64)s->states.size(), "pg_solver_get_state: state index out of range");
    src = s->states[state_index].p;
  }
  hipStream_t st = ctx().stream;
  DevBuf<double> pad((i64)s->K * s->Mloc);
  pad.zero();                                            // s.x = zeros(n)          solver.jl:186
  if (s->nb.n_own > 0) {
    hipLaunchKernelGGL(k_scatter_active, dim3(grid_for(s->nb.n_own, BLOCK)), dim3(BLOCK), 0, st, make_segs(s->nb),
                       s->nb.n_own, s->Mloc, s->nb.row_cell.p, src, pad.p);   // s.x[cols_idx] = x_reduced   :187
    PG_HIP(hipGetLastError());
  }
  // only the owned planes are authoritative on this rank
  const i64 own_lo = (s->slab.p0 - s->slab.s0) * s->slab.plane, own_n = (s->slab.p1 - s->slab.p0) * s->slab.plane;
  for (int k = 0; k < s->K; ++k)
    pad.download(x + (i64)k * s->M + s->slab.p0 * s->slab.plane, own_n, (i64)k * s->Mloc + own_lo);
  PG_API_END
}

int32_t pg_solver_system_info(const pg_solver* s, int32_t which, pg_system_info* out) {
  PG_API_BEGIN
  PG_REQUIRE(s && out, "pg_solver_system_info: NULL argument");
  const CsrMatrix& Af = ((which & 1) == 0 || !s->have_run) ? s->A_ctor : run_matrix(s);
  // which & 4: the matrix the warm time loop iterates on -- Â without the Dirichlet interface unknowns when that reduction
  // is active for this system (pg_reduce.hip), else Â itself; n_own / n_omega / n_gamma always describe the full system
  const GammaElim& E = (&Af == &s->A_ctor) ? s->elim_ctor : s->elim_run;
  const DiagElim& DE = (&Af == &s->A_ctor) ? s->diag_ctor : s->diag_run;
  const CsrMatrix& A = ((which & 4) && DE.active) ? DE.A : (((which & 4) && E.active) ? E.A : Af);
  out->n_own = s->nb.n_own;
  out->nnz = (which & 6) ? A.nnz : A.nnz_raw;
  out->n_ghost = s->nb.n_ghost;
  i64 nw = 0, ng = 0;
  for (int k = 0; k < s->K; ++k) ((k & 1) ? ng : nw) += s->nb.cnt_own[k];
  out->n_omega = nw;
  out->n_gamma = ng;
  out->M_global = s->M;
  out->spmv_bytes = A.spmv_bytes;
  out->spmv_slices = A.nslices;
  out->rows_uniform = A.rows_u;
  out->rows_pattern = A.rows_p + A.rows_e;
  out->rows_edge = A.rows_e;
  out->rows_irregular = A.rows_g;
  out->neumann_ok = A.poly_ok ? 1 : 0;
  out->gershgorin = A.gersh;
  out->spmv_units = A.nunits;
  out->rows_marched = A.rows_m;
  out->rows_matrix = A.n;
  out->n_ghost_loop = ((which & 4) && DE.active) ? DE.nb.n_ghost : s->nb.n_ghost;
  out->loop_is_compact = DE.active ? 1 : 0;
  PG_API_END
}

static const CsrMatrix& debug_matrix(const pg_solver* s, int32_t which, i64* nv);

int32_t pg_solver_get_system_csr(const pg_solver* s, int32_t which, int64_t* rowptr, int64_t* col, double* val, double* b,
                                 int64_t* idx) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s, "pg_solver_get_system_csr: NULL argument");
  const bool precond = (which & 2) != 0;   // 2/3: the preconditioned system (Â, b̂) exactly as the Krylov solver sees it
  const int sel = which & 1;
  if (sel == 1) PG_REQUIRE(s->have_run, "run matrix not assembled yet");
  if (which & 4) {
    // 6/7: the matrix the warm loop iterates on, in its own numbering (pg_solver_system_info(6/7), pg_debug_spmv_sizes)
    PG_REQUIRE(precond, "pg_solver_get_system_csr: which = 6 / 7 (the loop's matrix is a preconditioned one)");
    PG_REQUIRE(!b && !idx, "pg_solver_get_system_csr: b and idx belong to the full system: NULL for which = 6 / 7");
    i64 nv = 0;
    const CsrMatrix& L = debug_matrix(s, which, &nv);
    if (rowptr) {
      std::vector<int> h(L.n + 1, 0);
      if (L.n > 0) L.rowptr.download(h.data(), L.n + 1);
      for (i64 i = 0; i <= L.n; ++i) rowptr[i] = h[i];
    }
    if (col && L.nnz > 0) {
      std::vector<int> h(L.nnz);
      L.col.download(h.data(), L.nnz);
      for (i64 i = 0; i < L.nnz; ++i) col[i] = h[i];
    }
    if (val && L.nnz > 0) L.val.download(val, L.nnz);
    return 0;
  }
  const CsrMatrix& Ah = sel == 0 ? s->A_ctor : run_matrix(s);
  const i64 n = s->nb.n_own;
  // 0/1: the reference's reduced system A x = b: the matrix is re-assembled without scaling (export is a test /
  // debugging path), b is recovered from b̂ = B⁻¹ S b
  CsrMatrix raw;
  if (!precond && (rowptr || col || val))
    assemble_csr(make_params(s, sel == 0 ? s->scheme_ctor : s->scheme_run), s->slab, s->nb, raw, false);
  const CsrMatrix& A = precond ? Ah : raw;
  if (rowptr) {
    std::vector<int> h(n + 1);
    A.rowptr.download(h.data(), n + 1);
    for (i64 i = 0; i <= n; ++i) rowptr[i] = h[i];
  }
  if (col && A.nnz > 0) {
    std::vector<int> h(A.nnz);
    A.col.download(h.data(), A.nnz);
    for (i64 i = 0; i < A.nnz; ++i) col[i] = h[i];
  }
  if (val && A.nnz > 0) A.val.download(val, A.nnz);
  if (b && n > 0) {
    s->b.download(b, n);
    if (!precond) {
      std::vector<double> hb(b, b + n), hds(n);
      Ah.ds.download(hds.data(), n);
      for (i64 r = 0; r < n; ++r) b[r] = hb[r] / hds[r];
      if (Ah.n_blk > 0) {
        const i64 nq = Ah.n_blk;
        std::vector<int> rows(nq), bi(nq * MAX_KINDS);
        std::vector<double> fw(nq * MAX_KINDS);
        Ah.blk_rows.download(rows.data(), nq);
        Ah.blk_idx.download(bi.data(), nq * MAX_KINDS);
        Ah.blk_fw.download(fw.data(), nq * MAX_KINDS);
        for (i64 q = 0; q < nq; ++q) {
          double v = 0.0;
          for (int a = 0; a < MAX_KINDS; ++a)
            if (bi[q * MAX_KINDS + a] >= 0) v += fw[q * MAX_KINDS + a] * hb[bi[q * MAX_KINDS + a]];
          b[rows[q]] = v / hds[rows[q]];
        }
      }
    }
  }
  if (idx && n > 0) {
    std::vector<int> h(n);
    s->nb.row_cell.download(h.data(), n);
    for (i64 r = 0; r < n; ++r) {
      const int k = s->nb.kind_of_row(r);
      idx[r] = (i64)k * s->M + s->slab.first_cell() + h[r];
    }
  }
  PG_API_END
}

// Hₙ₊₁, Hₙ, Σq, max|q| of each phase of a 1-D space-time slab (k_stefan_partials); out: 4 * nphase doubles.  T is the
// slab's solution once it is solved, the state it was built from before
int32_t pg_solver_stefan_terms(const pg_solver* s, double* out) {
  PG_API_BEGIN
  PG_REQUIRE(s && out, "pg_solver_stefan_terms: NULL argument");
  PG_REQUIRE(s->moving && !s->advdiff && s->cap[0]->spacetime && (s->nphase == 1 || s->cap[1]->spacetime),
             "pg_solver_stefan_terms needs a moving diffusion solver on space-time capacities");
  PG_REQUIRE(ctx().nranks == 1 && !ctx().comm, "pg_solver_stefan_terms: space-time steps are single-rank");
  PG_REQUIRE(s->slab.N == 1, "pg_solver_stefan_terms: 1-D liquid motion only (N = 1)");
  hipStream_t st = ctx().stream;
  StefanArgs a;
  std::memset(&a, 0, sizeof(a));
  for (int q = 0; q < s->nphase; ++q) {
    SysParams& P = a.P[q];
    P.nphase = 1;
    P.cap[0] = P.cap[1] = cap_view(s->cap[q]);
    P.ct[0] = P.ct[1] = s->cap[q]->ct.p;
    P.Ib = 1.0;
    P.gscale = 1.0;
    a.v0[q] = s->cap[q]->Vt[0].p;
    a.v1[q] = s->cap[q]->Vt[1].p;
    a.Id[q] = s->Id[q].p;
  }
  a.red = s->nb.red.p;
  if (s->initial_done) {
    a.x = s->x_valid ? s->x.p : s->z.p;
    a.ds = s->x_valid ? nullptr : s->z_matrix->ds.p;
  } else {
    a.Tpad = s->T0pad.p;   // not solved yet: the state the slab was built from (T_prev or the previous solver's)
  }
  a.Mloc = s->Mloc;
  a.nphase = s->nphase;
  const int g = grid_for(s->Mloc, BLOCK, STEFAN_BLOCKS);
  double* partials = s->red_scratch.p;                    // (2048 doubles: g * 8 partials, then the 8 results)
  double* res = s->red_scratch.p + STEFAN_BLOCKS * STEFAN_OUT;
  hipLaunchKernelGGL(k_stefan_partials, dim3(g), dim3(BLOCK), 0, st, a, partials);
  hipLaunchKernelGGL(k_stefan_final, dim3(1), dim3(64), 0, st, (const double*)partials, g, res);
  PG_HIP(hipGetLastError());
  s->red_scratch.download(out, 4 * s->nphase, STEFAN_BLOCKS * STEFAN_OUT);
  PG_API_END
}

static void fill_mg_info(const MgHierarchy& H, pg_mg_info* out) {
  out->levels = (int32_t)H.lev.size();
  out->tail_level = H.tail0;
  for (size_t l = 0; l < H.lev.size() && l < PG_MG_MAX_LEVELS; ++l) {
    out->rows[l] = H.lev[l]->n;
    out->nnz[l] = H.lev[l]->nnz;
  }
  out->setup_ms = H.setup_ms;
  out->bytes = H.bytes;
}

// one level of a hierarchy to the host (two-call size pattern: NULL arrays are skipped)
static void download_mg_level(const MgLevel& v, int64_t* n, int64_t* nnz, int64_t* rowptr, int64_t* col, double* val) {
  if (n) *n = v.n;
  if (nnz) *nnz = v.nnz;
  hipStream_t st = ctx().stream;
  if (rowptr) {
    std::vector<int> h(v.n + 1);
    PG_HIP(hipMemcpyAsync(h.data(), v.rowptr, sizeof(int) * (size_t)(v.n + 1), hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));
    for (i64 i = 0; i <= v.n; ++i) rowptr[i] = h[i];
  }
  if (col && v.nnz > 0) {
    std::vector<int> h(v.nnz);
    PG_HIP(hipMemcpyAsync(h.data(), v.col, sizeof(int) * (size_t)v.nnz, hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));
    for (i64 i = 0; i < v.nnz; ++i) col[i] = h[i];
  }
  if (val && v.nnz > 0) {
    PG_HIP(hipMemcpyAsync(val, v.val, sizeof(double) * (size_t)v.nnz, hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));
  }
}

static MgRule debug_mg_rule(int32_t precond) {
  PG_REQUIRE(mg_is_precond(precond), "multigrid diagnostics: precond must be PG_PRECOND_MG or PG_PRECOND_MG_CELL");
  return mg_rule_of(precond);
}

int32_t pg_solver_mg_info(const pg_solver* s, pg_mg_info* out) { return pg_solver_mg_info_for(s, PG_PRECOND_MG, out); }

int32_t pg_solver_mg_info_for(const pg_solver* s, int32_t precond, pg_mg_info* out) {
  PG_API_BEGIN
  PG_REQUIRE(s && out, "pg_solver_mg_info: NULL argument");
  std::memset(out, 0, sizeof(*out));
  const MgHierarchy& H = debug_mg_rule(precond) == MG_RULE_CELL ? s->mg_cell : s->mg;
  if (H.matrix != &s->A_ctor) return 0;
  fill_mg_info(H, out);
  PG_API_END
}

// the matrix `which` names (0 constructor, 1 run system) and, unless bit 2 says "report only", its spectral estimate
static CsrMatrix& specest_matrix(pg_solver* s, int32_t which, const char* entry) {
  require_init();
  PG_REQUIRE(s, std::string(entry) + ": NULL solver");
  PG_REQUIRE((which & ~5) == 0, std::string(entry) + ": which = 0 (constructor system) or 1 (run system), + 4: report only");
  PG_REQUIRE((which & 1) == 0 || s->have_run, std::string(entry) + ": the solver has no run system yet (take a step first)");
  CsrMatrix& A = const_cast<CsrMatrix&>((which & 1) == 0 ? s->A_ctor : run_matrix(s));
  if ((which & 4) == 0) {
    specest_conditions(s, PG_METHOD_BICGSTAB);
    specest_run(A, s->nb, s->slab);
  }
  return A;
}

int32_t pg_solver_spectral_estimate(pg_solver* s, int32_t which, pg_specest_info* out) {
  PG_API_BEGIN
  PG_REQUIRE(out, "pg_solver_spectral_estimate: NULL argument");
  std::memset(out, 0, sizeof(*out));
  const CsrMatrix& A = specest_matrix(s, which, "pg_solver_spectral_estimate");
  out->margin = SPECEST_MARGIN;
  out->gershgorin = A.gersh;
  out->gershgorin_admits = A.poly_ok ? 1 : 0;
  if (!A.est.tried) return 0;
  out->steps = A.est.steps;
  out->admitted = A.est.admitted ? 1 : 0;
  out->g_ritz = A.est.g_ritz;
  out->g_used = A.est.g_used;
  out->ritz_re_min = A.est.re_min;
  out->ritz_re_max = A.est.re_max;
  out->ritz_im_max = A.est.im_max;
  out->estimate_ms = A.est.ms;
  PG_API_END
}

int32_t pg_debug_specest_hessenberg(pg_solver* s, int32_t which, int32_t* steps, double* H) {
  PG_API_BEGIN
  const CsrMatrix& A = specest_matrix(s, which, "pg_debug_specest_hessenberg");
  if (steps) *steps = A.est.tried ? A.est.steps : 0;
  if (H && A.est.tried && A.est.steps > 0) std::memcpy(H, A.est.H.data(), sizeof(double) * (size_t)(A.est.steps + 1) * A.est.steps);
  PG_API_END
}

static MgHierarchy& debug_mg(pg_solver* s, int32_t precond) {
  require_init();
  PG_REQUIRE(s, "multigrid diagnostics: NULL solver");
  const MgRule rule = debug_mg_rule(precond);
  mg_conditions(s, PG_METHOD_BICGSTAB, rule);
  return mg_ensure(s, rule);
}

int32_t pg_debug_mg_aggregates(pg_solver* s, int32_t level, int64_t* n, int32_t* agg) {
  return pg_debug_mg_aggregates_for(s, PG_PRECOND_MG, level, n, agg);
}
int32_t pg_debug_mg_level_csr(pg_solver* s, int32_t level, int64_t* n, int64_t* nnz, int64_t* rowptr, int64_t* col, double* val) {
  return pg_debug_mg_level_csr_for(s, PG_PRECOND_MG, level, n, nnz, rowptr, col, val);
}
int32_t pg_debug_mg_apply(pg_solver* s, const double* r, double* z) { return pg_debug_mg_apply_for(s, PG_PRECOND_MG, r, z); }

int32_t pg_debug_mg_aggregates_for(pg_solver* s, int32_t precond, int32_t level, int64_t* n, int32_t* agg) {
  PG_API_BEGIN
  MgHierarchy& H = debug_mg(s, precond);
  PG_REQUIRE(level >= 0 && level + 1 < (int)H.lev.size(), "pg_debug_mg_aggregates: level has no aggregates (0 <= level < levels - 1)");
  const MgLevel& v = *H.lev[level];
  if (n) *n = v.n;
  if (agg) v.agg.download(agg, v.n);
  PG_API_END
}

int32_t pg_debug_mg_level_csr_for(pg_solver* s, int32_t precond, int32_t level, int64_t* n, int64_t* nnz, int64_t* rowptr, int64_t* col,
                                  double* val) {
  PG_API_BEGIN
  MgHierarchy& H = debug_mg(s, precond);
  PG_REQUIRE(level >= 0 && level < (int)H.lev.size(), "pg_debug_mg_level_csr: no such level");
  download_mg_level(*H.lev[level], n, nnz, rowptr, col, val);
  PG_API_END
}

int32_t pg_debug_mg_apply_for(pg_solver* s, int32_t precond, const double* r, double* z) {
  PG_API_BEGIN
  MgHierarchy& H = debug_mg(s, precond);
  PG_REQUIRE(r && z, "pg_debug_mg_apply: NULL argument");
  const i64 n = s->nb.n_own, nv = s->nb.n_vec();
  DevBuf<double> din(nv), dout(nv);
  din.zero();
  dout.zero();
  din.upload(r, n);
  mg_apply(H, s->A_ctor, s->nb, s->slab, din.p, dout.p, nullptr, ctx().stream);
  dout.download(z, n);
  PG_API_END
}

// ---- PG_PRECOND_MG_STEP: the same report and diagnostics per assembled matrix (which = 0 constructor system, 1 run system)
int32_t pg_solver_mg_step_info(const pg_solver* s, int32_t which, pg_mg_info* out) {
  PG_API_BEGIN
  PG_REQUIRE(s && out, "pg_solver_mg_step_info: NULL argument");
  PG_REQUIRE(which == 0 || which == 1, "pg_solver_mg_step_info: which = 0 (constructor system) or 1 (run system)");
  std::memset(out, 0, sizeof(*out));
  const MgHierarchy& H = s->mg_step[which];
  if (H.lev.empty() || H.matrix != (which == 0 ? &s->A_ctor : &s->A_run)) return 0;
  fill_mg_info(H, out);
  PG_API_END
}

// the matrix `which` names and its PG_PRECOND_MG_STEP hierarchy, built if need be
static MgHierarchy& debug_mg_step(pg_solver* s, int32_t which, const CsrMatrix** A) {
  require_init();
  PG_REQUIRE(s, "multigrid diagnostics: NULL solver");
  PG_REQUIRE(which == 0 || which == 1, "multigrid diagnostics: which = 0 (constructor system) or 1 (run system)");
  mg_step_conditions(s, PG_METHOD_BICGSTAB);
  PG_REQUIRE(which == 0 || (s->have_run && &run_matrix(s) == &s->A_run),
             "multigrid diagnostics: the solver has no run system of its own (take a step in the other scheme first)");
  *A = which == 0 ? &s->A_ctor : &s->A_run;
  return mg_step_ensure(s, **A);
}

int32_t pg_debug_mg_step_aggregates(pg_solver* s, int32_t which, int32_t level, int64_t* n, int32_t* agg) {
  PG_API_BEGIN
  const CsrMatrix* A = nullptr;
  MgHierarchy& H = debug_mg_step(s, which, &A);
  PG_REQUIRE(level >= 0 && level + 1 < (int)H.lev.size(), "pg_debug_mg_step_aggregates: level has no aggregates (0 <= level < levels - 1)");
  const MgLevel& v = *H.lev[level];
  if (n) *n = v.n;
  if (agg) v.agg.download(agg, v.n);
  PG_API_END
}

int32_t pg_debug_mg_step_level_csr(pg_solver* s, int32_t which, int32_t level, int64_t* n, int64_t* nnz, int64_t* rowptr, int64_t* col,
                                   double* val) {
  PG_API_BEGIN
  const CsrMatrix* A = nullptr;
  MgHierarchy& H = debug_mg_step(s, which, &A);
  PG_REQUIRE(level >= 0 && level < (int)H.lev.size(), "pg_debug_mg_step_level_csr: no such level");
  download_mg_level(*H.lev[level], n, nnz, rowptr, col, val);
  PG_API_END
}

int32_t pg_debug_mg_step_apply(pg_solver* s, int32_t which, const double* r, double* z) {
  PG_API_BEGIN
  const CsrMatrix* A = nullptr;
  MgHierarchy& H = debug_mg_step(s, which, &A);
  PG_REQUIRE(r && z, "pg_debug_mg_step_apply: NULL argument");
  const i64 n = s->nb.n_own, nv = s->nb.n_vec();
  DevBuf<double> din(nv), dout(nv);
  din.zero();
  dout.zero();
  din.upload(r, n);
  mg_apply(H, *A, s->nb, s->slab, din.p, dout.p, nullptr, ctx().stream);
  dout.download(z, n);
  PG_API_END
}

int32_t pg_solver_get_row_scaling(const pg_solver* s, int32_t which, double* ds) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && ds, "pg_solver_get_row_scaling: NULL argument");
  if ((which & 1) == 1) PG_REQUIRE(s->have_run, "run matrix not assembled yet");
  const CsrMatrix& A = (which & 1) == 0 ? s->A_ctor : run_matrix(s);
  if (s->nb.n_own > 0) A.ds.download(ds, s->nb.n_own);
  PG_API_END
}

// max |y_a - y_b| between two SpMV kernel variants applied to the same deterministic test vector
__global__ void k_test_vector(i64 n, double* x) {
  for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    unsigned long long h = (unsigned long long)i * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
    h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    x[i] = (double)(h >> 11) * (1.0 / 9007199254740992.0) - 0.5;
  }
}

// the matrix pg_solver_system_info(which) describes (bit 0: run matrix, bit 2: the matrix the warm loop iterates on) and the
// length of the vectors it works on
static const CsrMatrix& debug_matrix(const pg_solver* s, int32_t which, i64* nv) {
  if (which & 1) PG_REQUIRE(s->have_run, "run matrix not assembled yet");
  const CsrMatrix& Af = (which & 1) == 0 ? s->A_ctor : run_matrix(s);
  const GammaElim& E = (&Af == &s->A_ctor) ? s->elim_ctor : s->elim_run;
  const DiagElim& DE = (&Af == &s->A_ctor) ? s->diag_ctor : s->diag_run;
  if ((which & 4) && DE.active) { *nv = DE.nb.n_vec(); return DE.A; }
  if ((which & 4) && E.active) { *nv = E.nb.n_vec(); return E.A; }
  *nv = s->nb.n_vec();
  return Af;
}

int32_t pg_debug_spmv_compare(pg_solver* s, int32_t which, int32_t variant_a, int32_t variant_b, double* max_abs_diff,
                              double* max_abs) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && max_abs_diff && max_abs, "pg_debug_spmv_compare: NULL argument");
  i64 nv = 0;
  const CsrMatrix& A = debug_matrix(s, which, &nv);
  hipStream_t st = ctx().stream;
  const i64 n = A.n;
  nv = std::max(nv, n);
  *max_abs_diff = 0.0;
  *max_abs = 0.0;
  if (n > 0) {
    DevBuf<double> xv(nv), ya(n), yb(n);
    hipLaunchKernelGGL(k_test_vector, dim3(grid_for(nv, BLOCK)), dim3(BLOCK), 0, st, nv, xv.p);
    launch_spmv_variant(variant_a, A, xv.p, ya.p, st);
    launch_spmv_variant(variant_b, A, xv.p, yb.p, st);
    PG_HIP(hipGetLastError());
    std::vector<double> ha(n), hb(n);
    ya.download(ha.data(), n);
    yb.download(hb.data(), n);
    for (i64 i = 0; i < n; ++i) {
      *max_abs_diff = std::max(*max_abs_diff, std::fabs(ha[i] - hb[i]));
      *max_abs = std::max(*max_abs, std::fabs(ha[i]));
    }
  }
  PG_API_END
}

int32_t pg_debug_spmv_mode_compare(pg_solver* s, int32_t which, int32_t mode, double* max_abs_diff, double* max_abs,
                                   double* max_dot_rel) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && max_abs_diff && max_abs && max_dot_rel, "pg_debug_spmv_mode_compare: NULL argument");
  PG_REQUIRE(mode == 0 || mode == 1 || mode == 3 || mode == 8, "pg_debug_spmv_mode_compare: launch modes 0, 1, 3 and 8");
  i64 nv = 0;
  const CsrMatrix& A = debug_matrix(s, which, &nv);
  spmv_mode_compare(A, std::max(nv, A.n), mode, max_abs_diff, max_abs, max_dot_rel);
  PG_API_END
}

int32_t pg_debug_spmv_sizes(pg_solver* s, int32_t which, int64_t* n, int64_t* n_vec, int64_t* nnz, int32_t* grid) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s, "pg_debug_spmv_sizes: NULL argument");
  i64 nv = 0;
  const CsrMatrix& A = debug_matrix(s, which, &nv);
  if (n) *n = A.n;
  if (n_vec) *n_vec = std::max(nv, A.n);
  if (nnz) *nnz = A.nnz;
  if (grid) *grid = spmv_default_grid(A.n);
  PG_API_END
}

int32_t pg_debug_spmv_apply(pg_solver* s, int32_t which, int32_t variant, int32_t mode, const double* x, const double* aux,
                            const double* dotx, const double* base, double pc0, double pc1, double pc2, int32_t fold,
                            int32_t done, int32_t repeat, double* y, double* partials, double* slot_sums, double* folded,
                            int64_t* ticket) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && x && y && slot_sums && folded && ticket, "pg_debug_spmv_apply: NULL argument");
  PG_REQUIRE(ctx().nranks == 1 && !ctx().comm, "pg_debug_spmv_apply: one rank (the split launch of a slab is not covered)");
  PG_REQUIRE(variant == 70 || variant == 38 || variant == 2 || variant == 1, "pg_debug_spmv_apply: variants 70, 38, 2 and 1");
  PG_REQUIRE(mode == 0 || mode == 1 || mode == 2 || mode == 3 || mode == 8, "pg_debug_spmv_apply: launch modes 0, 1, 2, 3 and 8");
  PG_REQUIRE(repeat == 1 || repeat == 2, "pg_debug_spmv_apply: repeat is 1 or 2");
  PG_REQUIRE(fold == 0 || fold == 1, "pg_debug_spmv_apply: fold is 0 or 1");
  const bool slices = (variant & 64) != 0;
  PG_REQUIRE(slices || (mode != 8 && !dotx && !fold),
             "pg_debug_spmv_apply: mode 8, a separate dot operand and the folded scalar phase exist in the slice kernel (variant 70) only");
  PG_REQUIRE(!fold || (mode >= 1 && mode <= 3), "pg_debug_spmv_apply: only the modes with dots (1, 2, 3) fold a scalar phase");
  PG_REQUIRE((mode == 1 || mode == 3) == (aux != nullptr), "pg_debug_spmv_apply: aux goes with modes 1 and 3, and only with them");
  PG_REQUIRE(!dotx || mode == 2 || mode == 3, "pg_debug_spmv_apply: dotx goes with modes 2 and 3");
  PG_REQUIRE(!base || mode == 8, "pg_debug_spmv_apply: base goes with mode 8");
  i64 nv = 0;
  const CsrMatrix& A = debug_matrix(s, which, &nv);
  const i64 n = A.n;
  PG_REQUIRE(n > 0, "pg_debug_spmv_apply: the matrix has no rows");
  PG_REQUIRE(!slices || A.srec.p, "pg_debug_spmv_apply: the matrix has no slice image");
  nv = std::max(nv, n);
  hipStream_t st = ctx().stream;
  const int grid = spmv_default_grid(n);
  constexpr i64 GUARD = 64;
  double sentinel;
  const unsigned long long sbits = PG_DEBUG_SPMV_SENTINEL;
  std::memcpy(&sentinel, &sbits, sizeof(double));
  // operands as long as the driver's vectors (n_vec), zeros behind row n
  DevBuf<double> dx(nv), daux(nv), ddot(nv), dbase(nv), dy(n + GUARD), dpart(5 * (i64)grid), dsc(S_COUNT);
  DevBuf<unsigned> dticket(1);
  daux.zero(); ddot.zero(); dbase.zero(); dsc.zero(); dticket.zero();
  dx.upload(x, nv);
  if (aux) daux.upload(aux, n);
  if (dotx) ddot.upload(dotx, n);
  if (base) dbase.upload(base, n);
  {
    std::vector<double> fill((size_t)std::max<i64>(n + GUARD, 5 * (i64)grid), sentinel);
    dy.upload(fill.data(), n + GUARD);
    if (fold && mode == 3) std::fill(fill.begin() + 2 * (size_t)grid, fill.begin() + 4 * (size_t)grid, 0.0);   // slots of another kernel
    dpart.upload(fill.data(), 5 * (i64)grid);
    std::vector<double> hsc(S_COUNT, 0.0);
    for (int k = 0; k < 5; ++k) hsc[S_RED0 + k] = sentinel;
    hsc[S_DONE] = (double)done;
    dsc.upload(hsc.data(), S_COUNT);
  }
  FinArgs f{fold ? dticket.p : nullptr, fold ? dsc.p : nullptr, PH_NONE, fold ? (mode == 1 ? 1 : (mode == 2 ? 2 : 5)) : 0, 0,
            dotx ? ddot.p : nullptr};
  if (mode == 8) { f.pc0 = pc0; f.pc1 = pc1; f.pc2 = pc2; f.base = base ? dbase.p : dx.p; }
  const bool with_fin = mode == 8 || fold || dotx;
  for (int r = 0; r < repeat; ++r) {
    const bool folded_here = launch_spmv_as(variant, mode, A, dx.p, dy.p, aux ? daux.p : nullptr, mode >= 1 && mode <= 3 ? dpart.p : nullptr,
                                            dsc.p, grid, st, with_fin ? &f : nullptr);
    PG_REQUIRE(folded_here == (fold != 0), "pg_debug_spmv_apply: the launch did not report the scalar phase as asked");
  }
  PG_HIP(hipGetLastError());
  dy.download(y, n + GUARD);
  std::vector<double> hp(5 * (size_t)grid), hsc(S_COUNT);
  dpart.download(hp.data(), 5 * (i64)grid);
  dsc.download(hsc.data(), S_COUNT);
  if (partials) std::memcpy(partials, hp.data(), sizeof(double) * hp.size());
  for (int k = 0; k < 5; ++k) {
    double a = 0.0;
    for (int i = 0; i < grid; ++i) a += hp[(size_t)k * grid + i];
    slot_sums[k] = a;
    folded[k] = hsc[S_RED0 + k];
  }
  unsigned ht = 0;
  dticket.download(&ht, 1);
  *ticket = (int64_t)ht;
  PG_API_END
}

int32_t pg_debug_spmv_apply_typed(pg_solver* s, int32_t which, int32_t kind, const void* x, const void* base, double pc0, double pc1,
                                  double pc2, double sigma, int32_t done, double* y64, float* y32, float* p32) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && x, "pg_debug_spmv_apply_typed: NULL argument");
  PG_REQUIRE(ctx().nranks == 1 && !ctx().comm, "pg_debug_spmv_apply_typed: one rank");
  PG_REQUIRE(kind == TYPED_FIRST || kind == TYPED_MIDDLE || kind == TYPED_HANDOVER, "pg_debug_spmv_apply_typed: kinds 1 (first), 2 (middle), 3 (hand-over)");
  PG_REQUIRE((kind == TYPED_FIRST) == (base == nullptr), "pg_debug_spmv_apply_typed: the first launch's base is its x; the others take one");
  PG_REQUIRE((kind == TYPED_FIRST) == (p32 != nullptr), "pg_debug_spmv_apply_typed: p32 is the first launch's output, and only its");
  PG_REQUIRE(kind == TYPED_HANDOVER ? (y64 && !y32) : (y32 && !y64), "pg_debug_spmv_apply_typed: y32 for kinds 1 and 2, y64 for kind 3");
  PG_REQUIRE(spmv_supports_typed_chain(), "pg_debug_spmv_apply_typed: the typed launches exist in the slice kernel with the stream hint only");
  i64 nv = 0;
  const CsrMatrix& A = debug_matrix(s, which, &nv);
  const i64 n = A.n;
  PG_REQUIRE(n > 0 && A.srec.p, "pg_debug_spmv_apply_typed: the matrix has no rows or no slice image");
  nv = std::max(nv, n);
  hipStream_t st = ctx().stream;
  const int grid = spmv_default_grid(n);
  constexpr i64 GUARD = 64;
  double sentinel;
  const unsigned long long sbits = PG_DEBUG_SPMV_SENTINEL;
  std::memcpy(&sentinel, &sbits, sizeof(double));
  float sentinel32;
  const unsigned sbits32 = PG_DEBUG_SPMV_SENTINEL_F32;
  std::memcpy(&sentinel32, &sbits32, sizeof(float));
  // operands as long as the driver's vectors (n_vec), zeros behind row n of base; outputs with 64 guard words behind row n
  DevBuf<double> dx64(nv), db64(nv), dy64(n + GUARD), dsc(S_COUNT);
  DevBuf<float> dx32(nv), db32(nv), dy32(n + GUARD), dp32(n + GUARD);
  db64.zero(); db32.zero();
  if (kind == TYPED_FIRST) dx64.upload(static_cast<const double*>(x), nv);
  else dx32.upload(static_cast<const float*>(x), nv);
  if (kind == TYPED_MIDDLE) db32.upload(static_cast<const float*>(base), n);
  if (kind == TYPED_HANDOVER) db64.upload(static_cast<const double*>(base), n);
  {
    std::vector<double> f64((size_t)(n + GUARD), sentinel);
    std::vector<float> f32((size_t)(n + GUARD), sentinel32);
    dy64.upload(f64.data(), n + GUARD);
    dy32.upload(f32.data(), n + GUARD);
    dp32.upload(f32.data(), n + GUARD);
    std::vector<double> hsc(S_COUNT, 0.0);
    hsc[S_DONE] = (double)done;
    dsc.upload(hsc.data(), S_COUNT);
  }
  FinArgs f{nullptr, nullptr, PH_NONE, 0, 0, nullptr};
  f.pc0 = pc0; f.pc1 = pc1; f.pc2 = pc2;
  if (kind == TYPED_FIRST) {
    f.base = dx64.p; f.p32 = dp32.p; f.psig = sigma;
    launch_spmv_typed(kind, A, dx64.p, dy32.p, dsc.p, grid, st, f);
  } else if (kind == TYPED_MIDDLE) {
    f.base = reinterpret_cast<const double*>(db32.p);
    launch_spmv_typed(kind, A, dx32.p, dy32.p, dsc.p, grid, st, f);
  } else {
    f.base = db64.p;
    launch_spmv_typed(kind, A, dx32.p, dy64.p, dsc.p, grid, st, f);
  }
  PG_HIP(hipGetLastError());
  if (y64) dy64.download(y64, n + GUARD);
  if (y32) dy32.download(y32, n + GUARD);
  if (p32) dp32.download(p32, n + GUARD);
  PG_API_END
}

__global__ void k_scale_rows(i64 n_e, const int* __restrict__ elist, double factor, double* __restrict__ z) {
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < n_e; q += (i64)gridDim.x * blockDim.x) z[elist[q]] *= factor;
}

int32_t pg_debug_scale_diagonal_rows(pg_solver* s, double factor) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && s->have_run, "pg_debug_scale_diagonal_rows: no run matrix yet");
  const CsrMatrix& A = run_matrix(s);
  DiagElim& DE = (&A == &s->A_ctor) ? s->diag_ctor : s->diag_run;
  PG_REQUIRE(DE.active && DE.n_e > 0, "pg_debug_scale_diagonal_rows: the loop of this solver is not the compact one");
  hipLaunchKernelGGL(k_scale_rows, dim3(grid_for(DE.n_e, BLOCK)), dim3(BLOCK), 0, ctx().stream, DE.n_e, (const int*)DE.elist.p, factor,
                     s->z.p);
  PG_HIP(hipGetLastError());
  PG_HIP(hipStreamSynchronize(ctx().stream));
  s->x_valid = false;
  s->spec_y_valid = false;
  PG_API_END
}

int32_t pg_solver_guess_info(pg_solver* s, int32_t* kept, int32_t* nstates, int32_t* offsets, double* coef, double* rr_plain,
                             double* rr_taken) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && kept && nstates && offsets && coef && rr_plain && rr_taken, "pg_solver_guess_info: NULL argument");
  *kept = s->hist_cnt;
  *nstates = 0;
  *rr_plain = *rr_taken = 0.0;
  for (int j = 0; j < 4; ++j) { offsets[j] = 0; coef[j] = 0.0; }
  if (s->guess_coef.n >= 16 && s->hist_cnt > 0) {
    double hc[16];
    s->guess_coef.download(hc, 16, s->guess_buf ? GUESS_USED : 0);
    *nstates = (int32_t)hc[4];
    for (int j = 0; j < *nstates && j < 4; ++j) { offsets[j] = (int32_t)hc[5 + j] + 1; coef[j] = hc[j]; }
    *rr_plain = hc[9];
    *rr_taken = hc[10];
  }
  PG_API_END
}

int32_t pg_solver_row_const_info(pg_solver* s, int64_t* out) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && out, "pg_solver_row_const_info: NULL argument");
  for (int k = 0; k < 4; ++k) out[k] = 0;
  if (const DiagElim* E = s->rc_last) {
    out[0] = E->rc_groups[0]; out[1] = E->rc_const[0];
    out[2] = E->rc_groups[1]; out[3] = E->rc_const[1];
  }
  PG_API_END
}

int32_t pg_debug_row_const_bconst(pg_solver* s, int64_t* out) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && out, "pg_debug_row_const_bconst: NULL argument");
  for (int k = 0; k < 4; ++k) out[k] = 0;
  if (const DiagElim* E = s->rc_last) {
    out[0] = E->rc_bmark_version >= 0 && E->rc_bmark_version == s->bconst_version ? 1 : 0;
    out[1] = out[0] ? E->rc_bmark_const : 0;
    out[2] = E->rc_bmark_builds;
    out[3] = out[0] ? E->rc_bmark_uses : 0;
  }
  PG_API_END
}

int32_t pg_solver_time_spmv(pg_solver* s, int32_t which, int32_t reps, double* avg_ms) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(s && avg_ms && reps > 0, "pg_solver_time_spmv: bad arguments");
  // bits 4-6: mode of the launch (0 plain, 1, 2, 3 fused dots); bit 11: the Horner step of the preconditioned loop
  // (mode 8: out = pc2 base + pc0 x + pc1 A x, three vector streams)
  const int sel = which & 1, mode = (which & 2048) ? 8 : ((which >> 4) & 7);
  PG_REQUIRE(mode <= 3 || mode == 8, "pg_solver_time_spmv: unknown launch mode");
  if (sel == 1) PG_REQUIRE(s->have_run, "run matrix not assembled yet");
  const CsrMatrix& Afull = sel == 0 ? s->A_ctor : run_matrix(s);
  // bit 9: the matrix the warm loop iterates on (without the Dirichlet interface rows, pg_reduce.hip), built here if need be
  GammaElim& E = (&Afull == &s->A_ctor) ? s->elim_ctor : s->elim_run;
  if ((which & 512) && !E.tried) build_gamma_elim(Afull, s->nb, E);
  // bit 12: the compact loop matrix (every row alone on its diagonal left out, DiagElim): what the benchmark's loop streams
  DiagElim& DE = (&Afull == &s->A_ctor) ? s->diag_ctor : s->diag_run;
  if ((which & 4096) && !DE.tried) build_diag_elim(Afull, s->nb, s->slab, DE);
  const CsrMatrix& A = ((which & 4096) && DE.active) ? DE.A : (((which & 512) && E.active) ? E.A : Afull);
  // bit 10: chained launches, each reading what the one before wrote (two vectors in turn): the access pattern of a chain
  // of lean launches in the loop
  const bool chained = (which & 1024) != 0;
  hipStream_t st = ctx().stream;
  EventPair ev;
  KrylovWork& w = s->work;
  // bit 8: "cold" launches -- every launch gets another input / output / dot-operand vector out of a ring of 7 (1.7 GB at
  // 512^3: nothing of the previous launch's vectors survives in the 256 MB Infinity Cache), which is how the launches of
  // the Krylov loop see memory; without it the same x and y stay cache resident from launch to launch
  const bool cold = (which & 256) != 0;
  constexpr int RING = 7;
  std::vector<DevBuf<double>> ring;
  const i64 nv = s->nb.n_vec();
  if (cold) {
    ring.resize(RING);
    for (auto& b : ring) {
      b.alloc(nv > 0 ? nv : 1);
      if (nv > 0) PG_HIP(hipMemcpyAsync(b.p, s->z.p, sizeof(double) * (size_t)nv, hipMemcpyDeviceToDevice, st));
    }
  }
  int it = 0;
  auto one = [&]() {
    const double* xin = cold ? ring[it % RING].p : (chained && (it & 1) ? s->y.p : s->z.p);
    double* yout = cold ? ring[(it + 3) % RING].p : (chained && (it & 1) ? s->z.p : s->y.p);
    const double* ax = cold ? ring[(it + 5) % RING].p : w.rhat.p;
    ++it;
    if (mode == 0) spmv(A, xin, yout, st);
    else if (mode == 8) {
      FinArgs f{nullptr, nullptr, PH_NONE, 0, 0, nullptr};
      f.pc0 = 1.0; f.pc1 = -0.5; f.pc2 = 0.5; f.base = s->b.p;   // (the chain's input: one fixed vector, re-read by every launch)
      launch_spmv(8, A, xin, yout, nullptr, nullptr, nullptr, w.grid, st, &f);
    }
    else launch_spmv(mode, A, xin, yout, ax, w.partials.p, nullptr, w.grid, st);
  };
  for (int i = 0; i < 3; ++i) one();
  PG_HIP(hipEventRecord(ev.e0, st));
  for (int i = 0; i < reps; ++i) one();
  PG_HIP(hipEventRecord(ev.e1, st));
  PG_HIP(hipEventSynchronize(ev.e1));
  PG_HIP(hipGetLastError());
  float ms = 0.f;
  PG_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *avg_ms = ms / reps;
  PG_API_END
}

}  // extern "C"

// ---- what a composite handle needs of a solver (pg_solver_internal.h) ----------------------------------------------------
namespace pg {

int32_t solver_create_unsteady_mono_dev(pg_capacity* c, pg_diffops* o, const pg_bc_desc* bc_interface, const pg_border_desc* borders,
                                        int32_t nborders, const SolverDeviceData& dev, double dt, const double* T0,
                                        pg_solver* previous, int32_t scheme, pg_solver** out) {
  SolverSpec d = spec_mono("pg_streamvort_step", c, o, bc_interface, borders, nborders, nullptr, nullptr, nullptr, out);
  d.dt = dt; d.T0 = T0; d.previous = previous; d.scheme = scheme;
  d.dev = &dev;
  d.solved_once = true;
  return create_solver(d);
}

i64 solver_mloc(const pg_solver* s) { return s->Mloc; }

double* solver_source_dev(pg_solver* s) {
  if (s->f_np1[0].n != s->Mloc) { s->f_np1[0].alloc(s->Mloc); s->f_np1[0].zero(); }
  return s->f_np1[0].p;
}

void solver_data_changed(pg_solver* s) { s->bconst_dirty = true; }

// A steady system solved again with a new right-hand side: the matrix, its numbering and its preconditioner stand; b = the
// time-data part alone (no mass term: b₁ = V f, b₂ = Γ g, border rows their values -- diffusion.jl:45-58); BiCGStab starts
// from the previous solution unless the caller asks for a cold start.  The first call is the initial solve.
void solver_solve_again(pg_solver* s, const pg_krylov_opts* opts, SolveStats& st) {
  PG_REQUIRE(s->scheme_ctor == PG_SCHEME_STEADY && !s->moving, "solve again: a steady solver is expected");
  if (!s->initial_done) {
    build_first_rhs(s);
    do_initial(s, opts, st);
    return;
  }
  const pg_krylov_opts o = opts ? *opts : default_opts();
  MgHierarchy* const mg = mg_prepare(s, o);
  if (mg_is_step(o.precond)) mg_step_conditions(s, o.method);   // (refuses: a steady system)
  specest_prepare(s, s->A_ctor, o);
  const i64 n = s->nb.n_own;
  ensure_bconst(s, PG_SCHEME_STEADY);
  if (n > 0) apply_left(s->A_ctor, s->bconst.p, s->b.p, ctx().stream);      // b̂ = B⁻¹ S b
  // z: the previous solution, scaled by this matrix's S
  const bool from_state = o.warm_start != 0 && (o.method == PG_METHOD_BICGSTAB || o.method == PG_METHOD_IDRS) && n > 0;
  solve_ctor_system(s, o, st, from_state, false, mg);
}

// One step of iterative refinement: r̂ = b̂ - Â z from a product (every row to the accuracy of its OWN entries), Â d = r̂ from zero
// to REFINE_RELTOL of ||r̂||, z += d.  A stopping test on ||r|| / ||b|| bounds the error by cond(Â) times the tolerance only.  The
// vorticity system of a step can be close to singular: the bulk row of a solid cell that nothing but the convection stencil of
// its cut neighbours reaches has a diagonal that is the residue of a cancellation (1e-20 next to off-diagonals of 1e-6 where
// the flow is mirror symmetric about the cell) -- a constraint between the neighbours, its unknown their multiplier,
// cond(Â) = 5e5.  A direct solve, which is what the reference runs, resolves it; the Krylov solve stopped at 1e-13 leaves 1e-8
// ... 1e-6 in that unknown.  The residual of such a row is far below ||b|| but well above the rounding of its own entries, and the
// correction is solved relative to it: the error bound falls by REFINE_RELTOL.  About half the products of the solve again.
constexpr double REFINE_RELTOL = 1e-6;

__global__ void k_refine_residual(i64 n, i64 nvec, const double* __restrict__ b, const double* __restrict__ y, double* __restrict__ r) {
  for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < nvec; i += (i64)gridDim.x * blockDim.x) r[i] = i < n ? b[i] - y[i] : 0.0;
}

__global__ void k_refine_add(i64 n, const double* __restrict__ d, double* __restrict__ z) {
  for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) z[i] += d[i];
}

static void refine_once(pg_solver* s, const pg_krylov_opts& o, SolveStats& st) {
  const i64 n = s->nb.n_own, nv = s->nb.n_vec();
  if (n <= 0) return;
  hipStream_t stream = ctx().stream;
  const CsrMatrix& A = s->A_ctor;
  spmv_halo(A, s->nb, s->slab, s->z.p, s->y.p, stream);
  DevBuf<double> r(nv);
  hipLaunchKernelGGL(k_refine_residual, dim3(grid_for(nv, BLOCK)), dim3(BLOCK), 0, stream, n, nv, (const double*)s->b.p,
                     (const double*)s->y.p, r.p);
  PG_HIP(hipGetLastError());
  pg_krylov_opts oc = o;
  oc.reltol = REFINE_RELTOL;
  oc.abstol = 0.0;
  SolveStats more;
  krylov_solve(A, s->nb, s->slab, r.p, s->ysol.p, s->work, oc, more);
  hipLaunchKernelGGL(k_refine_add, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, stream, n, (const double*)s->ysol.p, s->z.p);
  PG_HIP(hipGetLastError());
  st.iters += more.iters;
  st.products += more.products + 1;
  s->x_valid = false;
}

// The first (and only) solve of a time step that was built as a new solver: as do_initial, but BiCGStab starts from the state
// the solver was built from (s->x on this system's active set, written by k_rhs_first) instead of zero -- what do_initial
// does for a slab of the moving solvers.  One step of iterative refinement follows (refine_once).
void solver_first_solve_from_state(pg_solver* s, const pg_krylov_opts* opts, SolveStats& st) {
  const pg_krylov_opts o = opts ? *opts : default_opts();
  if (mg_is_precond(o.precond)) mg_conditions(s, o.method, mg_rule_of(o.precond));   // (a solver built for one time step: refused)
  if (mg_is_step(o.precond)) mg_step_conditions(s, o.method);                        // (likewise)
  specest_prepare(s, s->A_ctor, o);
  const i64 n = s->nb.n_own;
  if (!(o.warm_start != 0 && o.method == PG_METHOD_BICGSTAB && n > 0) || s->initial_done) {
    do_initial(s, opts, st);
    refine_once(s, o, st);
    return;
  }
  solve_ctor_system(s, o, st, true, true, nullptr);
  refine_once(s, o, st);
}

// padded = zeros(K * Mloc); padded[active] = x     (solver.jl:186-187), device to device
void solver_state_padded(pg_solver* s, double* padded) {
  hipStream_t st = ctx().stream;
  materialize_x(s);
  PG_HIP(hipMemsetAsync(padded, 0, sizeof(double) * (size_t)((i64)s->K * s->Mloc), st));
  if (s->nb.n_own > 0) {
    hipLaunchKernelGGL(k_scatter_active, dim3(grid_for(s->nb.n_own, BLOCK)), dim3(BLOCK), 0, st, make_segs(s->nb), s->nb.n_own,
                       s->Mloc, s->nb.row_cell.p, s->x.p, padded);
    PG_HIP(hipGetLastError());
  }
}

void solver_step_info(pg_solver* s, const SolveStats& st, double time, pg_step_info* info) {
  if (!info) return;
  fill_info(s, st, info);
  info->time = time;
}

}  // namespace pg
