// pg_krylov.h -- K11: Krylov solve of the reduced system on one slab (BiCGStab / CG / GMRES / BiCGStab(l) / IDR(s)).
#pragma once
#include <functional>

#include "pg_system.h"

namespace pg {

struct MgHierarchy;   // pg_multigrid.h

struct XGuess {
  const double* zbase = nullptr;
  const double* zr[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const double* coef = nullptr;
};

struct KrylovWork {
  i64 n = 0, nvec = 0;
  DevBuf<double> r, rhat, p, v, t;      // n_vec each (p and r -- which holds s between the two SpMVs -- carry ghosts)
  DevBuf<double> partials;              // per-block partial sums, 5 slots x grid
  DevBuf<double> sc;                    // device scalars (see pg_krylov.hip)
  double* h_sc = nullptr;               // pinned host mirror of sc
  int grid = 1;
  DevBuf<unsigned> ticket;              // arrival counter of the in-launch scalar phases (pg_spmv.h)
  double last_rate2 = 0.0;              // what one product took off log (r,r)_W in the previous polynomial solve (0: unknown)
  int last_iters = 0;                   // iterations of the previous solve (sizes the first launch batch)
  // degree of the preconditioner polynomial chosen from the previous solve on the same matrix (auto mode, pg_krylov.hip):
  // adapt_m products per application, adapt_h applications expected
  const void* adapt_matrix = nullptr;
  int adapt_m = 0, adapt_h = 0;
  const void* need_matrix = nullptr;    // the last estimates of the products a solve on that matrix needs (newest first)
  double need_hist[3] = {0.0, 0.0, 0.0};
  const void* fail_matrix = nullptr;    // x-space, one application per solve: the last degree that fell short (with the
  int fail_deg = 0, good_deg = 0;       // log of start residual / tolerance it fell short at) and the last that sufficed
  double fail_L = 0.0;
  int fail_wait = 0, fail_backoff = 1;  // solves left before that degree may be tried again; doubles when it falls short again
  // polynomial right preconditioner (pg_krylov.hip), n_vec each, on first use: ya = M⁻¹p, yb = M⁻¹s of the running
  // iteration (the updates of x read them) and the two work vectors the Horner chain alternates between
  DevBuf<double> ya, yb, wa, wb;
  // mixed-precision chain (pg_krylov.hip): the two fp32 work vectors the early Horner steps alternate between and p32 =
  // (float)(σ in), n_vec each, on first use; and what the previous solve on mix_matrix left for the next one: the power-of-two
  // scale σ of the fp32 vectors (from its start norm), the reduction an application has to deliver (mix_need: sets the length
  // of the fp64 tail) and the solves left in which the tail is two launches longer (after a solve whose mixed application
  // missed the half-step test)
  DevBuf<float> fa, fb, p32;
  const void* mix_matrix = nullptr;
  double mix_sigma = 0.0, mix_need = 0.0;
  int mix_wait = 0;
  // GMRES(m) only, allocated on first use (pg_gmres.hip): m+1 basis vectors, H / rotations / g, per-block partial sums
  DevBuf<double> gm_basis, gm, gm_partials;
  int gm_m = -1;
  // BiCGStab(l) only, allocated on first use (pg_bicgstabl.hip): R[0..l], U[0..l] and r̃ in one block (bl_stride apart), the
  // method's device scalars (with the Gram matrix and γ), per-block partial sums of the Gram / update kernels
  DevBuf<double> bl_vecs, bl, bl_partials;
  int bl_l = -1;
  i64 bl_stride = 0;
  // IDR(s) only, allocated on first use (pg_idrs.hip): G[0..s), U[0..s), r and t in one block (id_stride apart), the method's
  // device scalars (M, f, c, α, β, ω), per-block partial sums of its kernels
  DevBuf<double> id_vecs, id, id_partials;
  int id_s = -1;
  i64 id_stride = 0;
  // the event recorded behind the first poll's copy of the scalars when the call carries KrylovCall::after_first_batch
  hipEvent_t ev_poll = nullptr;
  void init(i64 n_own, i64 n_vec);
  ~KrylovWork();
};

// What ONE krylov_solve is asked to do, beyond the system, the options and the workspace: a value the caller builds next to the
// solve that uses it.  krylov_solve reads it and never writes it; nothing of it outlives the solve.  Everything below `preinit`
// belongs to a prepared start of the BiCGStab loop and is refused, not dropped, on any other solve.
struct KrylovCall {
  // x0 == nullptr: zero initial guess; else start from x0 with Ax0 = A*x0 given (BiCGStab and IDR(s) only).  x0 may be x itself
  // (the iteration continues from the iterate x holds).
  const double* x0 = nullptr;
  const double* Ax0 = nullptr;
  // (BiCGStab only) the caller has already written x, w.r = w.rhat = w.p = r0 and the partial sums of (r0,r0) / (b,b) in slots
  // 0 / 1 of w.partials with a w.grid-block launch (pg_solver.hip fuses that with the right-hand side).
  bool preinit = false;
  // a prepared start that wrote r̂ only: p = r = r̂ at the start, so the first iteration reads r̂ wherever it needs p or r
  // (k_bicg_s writes r = s, k_bicg_xrp writes p, as always) and the start kernel writes two vectors less.
  bool p_in_rhat = false;
  // the caller's start kernel has already reset the scalars, summed the start sums and derived PH_INIT (k_rhs_init_c with a
  // ticket): krylov_solve launches no start kernel.
  bool start_folded = false;
  // the system is a compact image of the caller's (pg_reduce.hip, DiagElim) and x is the caller's FULL vector -- the updates
  // x += α M⁻¹p, x += ω M⁻¹s land at x[scatter[i]].  Needs the polynomial path.
  const int* scatter = nullptr;
  // with scatter: the table of the compact system's rows whose ds is one value and whose scatter indices are consecutive
  // (pg_system.h, RowConst; tab == nullptr: none) -- k_bicg_s_x then loads neither on those rows (k_bicg_xrp streams: it measured slower with the table).
  RowConst row_const;
  // with opts.precond = PG_PRECOND_MG and its kin: the multigrid hierarchy of THIS matrix (the caller has checked that the
  // system admits it, pg_solver.hip mg_prepare); refused without such a precond.
  MgHierarchy* mg = nullptr;
  // a compact solve whose start was extrapolated from older states (pg_solver.hip, GuessArgs) and whose caller left the
  // extrapolated state unformed: the FIRST update of x then writes  x[map] = z_g[map] + α M⁻¹p,  z_g = zbase + Σ c_j (zr[o_j] -
  // zbase)  (coef: [0..3] c_j, [4] how many, [5..8] which of zr), instead of adding to x.
  XGuess xguess;
  // a prepared start on SEVERAL ranks that has not looked at the rows alone on their diagonal (a compact step with unchanged
  // data, pg_solver.hip): *moved_flag == moved_stamp says that one of them moved on this rank all the same.  The verdict rides
  // as a fourth slot in the start phase's all-reduce and every rank finds the same S_MOVED in the scalars of the solve.
  const int* moved_flag = nullptr;
  int moved_stamp = 0;
  // work to queue right AFTER the first batch of iterations and the copy of the scalars, BEFORE the host waits for that copy
  // -- the next time step's first product, speculatively: the device then has something to run while the host wakes up, reads
  // the scalars and queues the next step (the wait is on an event recorded behind the copy, not on the stream).  Called at
  // most once per solve.
  std::function<void()> after_first_batch;
};

struct SolveStats {
  int iters = 0;
  int converged = 0;
  double resnorm = 0.0, bnorm = 0.0;
  // profiling: HIP-event time of the sampled SpMV launches, by kind -- launches that carry fused dots (and their operand
  // vectors) and lean ones (plain products and the factors of the preconditioner polynomial: x, y and the matrix only)
  double spmv_ms = 0.0, spmv_lean_ms = 0.0;
  i64 spmv_launches = 0, spmv_lean_launches = 0;
  int poly_degree = 0;      // products with Â per application of the preconditioned operator (0: plain iteration)
  int half_exit = 0;        // 1: the solve ended at the half step of its last iteration (counted as an iteration)
  int poly_xspace = 0;      // 1: the polynomial preconditioner ran (kept for the ABI field pg_run_info.poly_xspace)
  i64 products = 0;         // products with Â inside the solve (the caller's start product not counted)
  int polls = 0;            // host waits of the solve (1: it ended inside the first batch of queued launches)
  // mixed-precision chain: launches that read or write an fp32 vector (first, middle, hand-over), their sampled HIP-event time
  // and count (a bracket of their own: spmv_lean_* keeps the fp64 Horner launches only), chains that ran mixed and the sum of
  // their fp64 tails' lengths j
  i64 f32_launches = 0, f32_timed = 0, f32_chains = 0, f32_tail_sum = 0;
  double f32_ms = 0.0;
};

// halo exchange of the ghost segments of `vec` (no-op on one rank)
void halo_exchange(const Numbering& nb, const Slab& slab, double* vec, hipStream_t st);
// the same exchange, split: halo_begin forks it off `st` onto the communication stream (everything enqueued on `st` so
// far is waited for there), halo_end makes `st` wait for its completion; work enqueued on `st` in between overlaps it.
// (Virtual ranks exchange synchronously inside halo_begin.)
void halo_begin(const Numbering& nb, const Slab& slab, double* vec, hipStream_t st);
void halo_end(hipStream_t st);
// y[0..n) = A * x   (x must hold valid ghosts)
void spmv(const CsrMatrix& A, const double* x, double* y, hipStream_t st);
// halo exchange of x (when the matrix needs one) overlapped with y[0..n) = A * x
void spmv_halo(const CsrMatrix& A, const Numbering& nb, const Slab& slab, double* x, double* y, hipStream_t st);
// x (n_vec, overwritten) = A^{-1} b, started and instructed as `call` says (the default: from zero, nothing prepared).  A call
// that the method of opts cannot honour is refused.  w is workspace and what one solve leaves for the next, never an input.
void krylov_solve(const CsrMatrix& A, const Numbering& nb, const Slab& slab, const double* b, double* x,
                  KrylovWork& w, const pg_krylov_opts& opts, SolveStats& stats, const KrylovCall& call = {});

// will krylov_solve(A, ..., opts) run BiCGStab right-preconditioned with the polynomial?  (Only that loop can solve a
// compact system: it updates x through KrylovCall::scatter.)
bool krylov_uses_polynomial(const CsrMatrix& A, const pg_krylov_opts& opts);

// iterations after which a polynomial-preconditioned solve that has not converged is given up as stagnated; 0: the built-in
// rule 40 + 400 / m.  Process-global, set by tests only (pg_debug_set_poly_give_up).
extern int g_poly_give_up;

// restarted GMRES (pg_gmres.hip): zero initial guess, x (n_vec, overwritten) = A^{-1} b
void gmres_solve(const CsrMatrix& A, const Numbering& nb, const Slab& slab, const double* b, double* x, KrylovWork& w,
                 const pg_krylov_opts& opts, SolveStats& stats);

// BiCGStab(l), l = opts.restart (<= 0: 2, > 8 refused) (pg_bicgstabl.hip): zero initial guess, x (n_vec, overwritten) = A^{-1} b;
// one rank; stats.iters counts BiCG sub-steps (two products each), stats.products = 2 iters + true-residual confirmations
void bicgstabl_solve(const CsrMatrix& A, const Numbering& nb, const Slab& slab, const double* b, double* x, KrylovWork& w,
                     const pg_krylov_opts& opts, SolveStats& stats);
// IDR(s), s = opts.restart (<= 0: 8, > 8 refused) (pg_idrs.hip): x (n_vec, overwritten) = A^{-1} b from zero or from x0 with
// Ax0 = A*x0 given (x0 may be x); one rank; stats.iters counts updates of x (one product each: the unit maxiter caps),
// stats.products = iters + restarts + true-residual confirmations (+ 1 from an x0: the caller's product with it)
void idrs_solve(const CsrMatrix& A, const Numbering& nb, const Slab& slab, const double* b, double* x, KrylovWork& w,
                const pg_krylov_opts& opts, SolveStats& stats, const double* x0 = nullptr, const double* Ax0 = nullptr);
// "the method is CG (BiCGStab only)" and its kin: the refusal texts of what serves BiCGStab alone
const char* krylov_method_refusal(int method);

}  // namespace pg
