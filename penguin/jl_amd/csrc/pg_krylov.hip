// pg_krylov.hip -- K11 of SURVEY.md section 2.3: the Krylov inner loop of solve_system! (src/solver.jl:158-188)
//
//   reference (IterativeSolvers 0.9.4, single thread)          here
//   CSC mul!                                                   pg_spmv.hip (stencil slices; dots fused into the launch)
//   dot / axpy! / norm (OpenBLAS BLAS-1)                       two fused vector kernels per BiCGStab iteration
//   method(A_reduced, b_reduced; kwargs...)                    device-resident BiCGStab / CG: all scalars stay on the
//                                                              GPU; the host polls a done flag between batches of
//                                                              queued iterations (no per-iteration sync)
//
// One BiCGStab iteration = 4 launches on one rank:
//   SpMV (v = Â p, (r̂,v); its last block evaluates: previous iteration's (r,r) -> convergence / restart, then α)
//   k_bicg_s   (s = r - αv over r; (r̂,s), (s,s))
//   SpMV (t = Â s, (t,s), (t,t), (r̂,t); last block: ω, ρ' = (r̂,s) - ω(r̂,t), β / restart decision)
//   k_bicg_xrp (x += αp + ωs; r = s - ωt; p = r + β(p - ωv); (r,r))
// With several ranks the SpMV's last block leaves the local sums, an RCCL all-reduce and k_derive follow.
//
// Polynomial right preconditioner (default where admissible, CsrMatrix::poly_ok; opts.precond = -1 or PG_POLY=0 turns it
// off).  The equilibrated systems of the time loop have their spectrum inside [1 - g, 1 + g], g = the Gershgorin radius
// pg_precond.hip computes (0.72 for the benchmark's Crank-Nicolson matrix).  With λ_1..λ_m the Chebyshev nodes of that
// interval, R(Â) = Π_k (I - Â/λ_k) is the degree-m residual polynomial of smallest maximum on it (0.29, 0.11, 0.043,
// 0.016 for m = 2, 3, 4, 5 at g = 0.72), M⁻¹ = q(Â) = Â⁻¹(I - R(Â)) a polynomial approximation of Â⁻¹, and BiCGStab runs on
// C = Â M⁻¹ = I - R(Â), whose spectrum lies within that maximum of 1: iterations fall like 1/m while the number of
// products with Â stays about the same.  Every application of C computes M⁻¹in = q(Â) in by Horner's rule -- m - 1 LEAN
// launches (mode 8: no dots, no BLAS-1 pass; roots taken alternately from both ends of the interval so that no partial
// product grows) -- and closes with the plain product Â(M⁻¹in) and its dots (modes 1 / 3).  The iteration updates x
// itself with the two preconditioned vectors (x += α M⁻¹p in k_bicg_s_x, which replaces k_bicg_s; x += ω M⁻¹s in
// k_bicg_xrp): x and r move by the SAME computed vectors, so r stays the residual of x whatever rounding does inside the
// chain, and the stopping test is unchanged.  The vector passes, the reductions and, with several ranks, the all-reduces
// of a time step fall with the iteration count.
// opts.precond = PG_PRECOND_POLY_EST (opt-in): the same branch on matrices Gershgorin refuses, with g = the radius of the
// spectral estimate (pg_specest.hip, CsrMatrix::est -- a flag of its own: poly_ok stays false, so neither the diagonal-row
// elimination nor the compact loop system starts); exactly precond = 0 where Gershgorin admits.
//
// Multigrid right preconditioner (opts.precond = PG_PRECOND_MG or PG_PRECOND_MG_CELL, never automatic): the same x-space loop with M⁻¹ = one V-cycle
// of pg_multigrid.hip where the Horner chain stands -- ya = M⁻¹p, yb = M⁻¹s, then the plain product with its dots.  It is a
// branch of its own: no degree, no adaptation, no give-up rule; the half-step test runs in every iteration (an application
// costs five to six products' worth of bytes).  SolveStats::products counts the products with Â of the outer loop, i.e. the
// applications.
#include "pg_host_algos.h"
#include "pg_krylov.h"
#include "pg_multigrid.h"
#include "pg_spmv.h"
#include "pg_specest.h"

using namespace pg;

namespace pg { extern double g_host_wait_us; }

namespace {


// ---- fused vector kernels ---------------------------------------------------------------------------
// x0 == nullptr: zero initial guess (IterativeSolvers' default).  Otherwise x = x0 and r = b - Ax0 (warm start with
// the previous time level; Ax0 is the SpMV the CN right-hand side needs anyway).  partials: slot 0 = r.r, slot 1 =
// (b,b)_W, slot 2 = (r,r)_W with the weights ds² of the convergence test (pg_spmv.h; ds == nullptr: unweighted)
// (x0 may be x itself: the fallback from a stagnated polynomial continues from the iterate reached)
__global__ __launch_bounds__(BLOCK) void k_bicg_init(i64 n, i64 nvec, const double* __restrict__ b,
                                                     const double* x0, const double* __restrict__ Ax0,
                                                     double* x, double* __restrict__ r,
                                                     double* __restrict__ rhat, double* __restrict__ p,
                                                     double* __restrict__ v, double* __restrict__ partials,
                                                     const double* __restrict__ ds) {
  __shared__ double s_red[BLOCK / 64];
  double acc = 0.0, accb = 0.0, accw = 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < nvec; i += (i64)gridDim.x * BLOCK) {
    if (i < n) {
      const double bi = b[i];
      const double ri = x0 ? bi - Ax0[i] : bi;
      const double d = ds ? ds[i] : 1.0;
      x[i] = x0 ? x0[i] : 0.0;
      r[i] = ri; rhat[i] = ri; p[i] = ri; v[i] = 0.0;   // p₀ = r₀ (β = 0)
      acc += ri * ri;
      accb += (d * bi) * (d * bi);
      accw += (d * ri) * (d * ri);
    } else {
      x[i] = 0.0; p[i] = 0.0;
    }
  }
  const double t = block_sum(acc, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
  const double tb = block_sum(accb, s_red);
  if (threadIdx.x == 0) partials[gridDim.x + blockIdx.x] = tb;
  const double tw = block_sum(accw, s_red);
  if (threadIdx.x == 0) partials[2 * (size_t)gridDim.x + blockIdx.x] = tw;
}

// s = r - αv written over r (r is not needed again: r_new = s - ωt); partials slots 2, 3 = (r̂,s), (s,s): they are
// summed together with the dots of the SpMV that follows (one scalar kernel instead of two)
// Stream hints on the vectors that are dead after this kernel (v here; x, t, v in k_bicg_xrp, v and M⁻¹p in k_bicg_s_x),
// so that they do not push the SpMV's matrix data (records, packed irregular rows: ~90 MB) out of the 256 MB Infinity
// Cache between launches.
// slot 4 = (s,s)_W, the weighted norm of the half-step convergence test (PH_BICG_S; the second product overwrites the slot
// afterwards)
__global__ __launch_bounds__(BLOCK) void k_bicg_s(i64 n, double* __restrict__ sc, const double* __restrict__ v,
                                                  const double* __restrict__ rhat, double* __restrict__ r,
                                                  double* __restrict__ partials, const double* __restrict__ ds,
                                                  unsigned* __restrict__ ticket, int r_in_rhat) {
  __shared__ double s_red[BLOCK / 64];
  if (sc[S_DONE] != 0.0) return;
  const double alpha = sc[S_ALPHA];
  const bool rrhat = r_in_rhat != 0 && sc[S_ITERS] == 0.0;   // first iteration of a start that left r = r̂ unwritten
  double a0 = 0.0, a1 = 0.0, aw = 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    const double rh = rhat[i];
    const double si = (rrhat ? rh : r[i]) - alpha * __builtin_nontemporal_load(v + i);
    r[i] = si;
    a0 += rh * si;
    a1 += si * si;
    const double ws = ds[i] * si;
    aw += ws * ws;
  }
  const double t0 = block_sum(a0, s_red);
  if (threadIdx.x == 0) partials[2 * (size_t)gridDim.x + blockIdx.x] = t0;
  const double t1 = block_sum(a1, s_red);
  if (threadIdx.x == 0) partials[3 * (size_t)gridDim.x + blockIdx.x] = t1;
  const double tw = block_sum(aw, s_red);
  if (!ticket) {
    if (threadIdx.x == 0) partials[4 * (size_t)gridDim.x + blockIdx.x] = tw;
    return;
  }
  // the half-step test (PH_BICG_S) inside this launch: the last block to arrive sums slot 4 in k_finalize's order and
  // derives (one rank: no all-reduce in between) -- a scalar kernel and its gap less per half step
  double* slot4 = partials + 4 * (size_t)gridDim.x;
  if (threadIdx.x == 0) store_partial(slot4 + blockIdx.x, tw);
  if (!last_block_arrives(ticket, gridDim.x, s_red)) return;
  double a = 0.0;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += BLOCK) a += load_partial(slot4 + i);
  const double t = block_sum(a, s_red);
  if (threadIdx.x == 0) {
    sc[S_RED0 + 4] = t;
    derive(PH_BICG_S, sc);
  }
}

// k_bicg_s and the x update of the first half in ONE pass (the preconditioned loop): s = r - αv over r with its dots and the
// half-step test, and x += α M⁻¹p through the index map of a compact system.  BiCGStab adds α M⁻¹p to x in every iteration
// whether or not it ends at the half step (x_{i+1} = x_i + α p̂ + ω ŝ, and nothing reads x in between), so the update does
// not wait for the verdict of the test, and k_bicg_xrp adds ω ŝ only.  Two rows per lane (16-byte accesses).
__global__ __launch_bounds__(BLOCK) void k_bicg_s_x(i64 n, double* __restrict__ sc, const double* __restrict__ v,
                                                    const double* __restrict__ rhat, double* __restrict__ r,
                                                    double* __restrict__ partials, const double* __restrict__ ds,
                                                    unsigned* __restrict__ ticket, int r_in_rhat, const double* __restrict__ phat,
                                                    double* x, const int* __restrict__ map, XGuess xg, int first_launch,
                                                    RowConst rc) {
  __shared__ double s_red[BLOCK / 64];
  const bool done = sc[S_DONE] != 0.0;
  if (done && !(xg.zbase != nullptr && first_launch != 0)) return;
  const double alpha = sc[S_ALPHA];
  const bool rrhat = r_in_rhat != 0 && sc[S_ITERS] == 0.0;   // first iteration of a start that left r = r̂ unwritten
  const double* __restrict__ rsrc = rrhat ? rhat : r;
  // first update of an extrapolated start whose state was left unformed (XGuess): x is written, not added to
  const bool fresh = xg.zbase != nullptr && rrhat && map != nullptr;
  int ku = 0;
  double cj[4] = {0.0, 0.0, 0.0, 0.0};
  const double* zo[4] = {xg.zbase, xg.zbase, xg.zbase, xg.zbase};
  if (fresh) {
    ku = min(4, (int)xg.coef[4]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < ku) {
        const int sel = (int)xg.coef[5 + j];
        cj[j] = xg.coef[j];
        const double* p = xg.zr[0];
#pragma unroll
        for (int q = 1; q < 8; ++q) p = sel == q ? xg.zr[q] : p;
        zo[j] = p;
      }
    }
  }
  auto base_of = [&](int j) {
    const double b = xg.zbase[j];
    double g = b;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < ku) g += cj[q] * (zo[q][j] - b);
    return g;
  };
  if (done) {
    // the start met the tolerance: no update will run, and this -- the first s kernel queued for the solve, ahead of whatever
    // the caller queues behind the first batch -- is where the extrapolated state of the loop's rows gets written
    if (fresh)
      for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) { const int j = map[i]; x[j] = base_of(j); }
    return;
  }
  double a0 = 0.0, a1 = 0.0, aw = 0.0;
  typedef double dd2 __attribute__((ext_vector_type(2)));
  const i64 npair = n / 2;
  for (i64 q = blockIdx.x * (i64)BLOCK + threadIdx.x; q < npair; q += (i64)gridDim.x * BLOCK) {
    const i64 i = 2 * q;
    const dd2 rh = *reinterpret_cast<const dd2*>(rhat + i);
    const dd2 rr = rrhat ? rh : *reinterpret_cast<const dd2*>(rsrc + i);
    const dd2 vv = __builtin_nontemporal_load(reinterpret_cast<const dd2*>(v + i));
    // (RowConst: a group of 16 rows -- 8 lanes -- whose ds is rc.d and whose map advances by one loads neither; e: map of its first row)
    const int e = rc.tab ? rc.tab[i >> RC_SHIFT] : -1;
    dd2 dw;
    dw.x = rc.d; dw.y = rc.d;
    if (e < 0) dw = *reinterpret_cast<const dd2*>(ds + i);
    const dd2 ph = __builtin_nontemporal_load(reinterpret_cast<const dd2*>(phat + i));
    dd2 si;
    si.x = rr.x - alpha * vv.x;
    si.y = rr.y - alpha * vv.y;
    *reinterpret_cast<dd2*>(r + i) = si;
    if (map) {
      int j0 = e + (int)(i & (RC_GROUP - 1)), j1 = j0 + 1;
      if (e < 0) { j0 = map[i]; j1 = map[i + 1]; }
      if (fresh) {
        const double g0 = base_of(j0), g1 = base_of(j1);
        x[j0] = g0 + alpha * ph.x;
        x[j1] = g1 + alpha * ph.y;
      } else {
        x[j0] += alpha * ph.x;
        x[j1] += alpha * ph.y;
      }
    } else {
      dd2 xx = *reinterpret_cast<dd2*>(x + i);
      xx.x += alpha * ph.x;
      xx.y += alpha * ph.y;
      *reinterpret_cast<dd2*>(x + i) = xx;
    }
    a0 += rh.x * si.x + rh.y * si.y;
    a1 += si.x * si.x + si.y * si.y;
    const double w0 = dw.x * si.x, w1 = dw.y * si.y;
    aw += w0 * w0 + w1 * w1;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last row
    const i64 i = n - 1;
    const double rh = rhat[i], si = rsrc[i] - alpha * v[i];
    r[i] = si;
    if (fresh) x[map[i]] = base_of(map[i]) + alpha * phat[i];
    else x[map ? map[i] : i] += alpha * phat[i];
    a0 += rh * si;
    a1 += si * si;
    aw += (ds[i] * si) * (ds[i] * si);
  }
  const double t0 = block_sum(a0, s_red);
  if (threadIdx.x == 0) partials[2 * (size_t)gridDim.x + blockIdx.x] = t0;
  const double t1 = block_sum(a1, s_red);
  if (threadIdx.x == 0) partials[3 * (size_t)gridDim.x + blockIdx.x] = t1;
  const double tw = block_sum(aw, s_red);
  if (!ticket) {
    if (threadIdx.x == 0) partials[4 * (size_t)gridDim.x + blockIdx.x] = tw;
    return;
  }
  double* slot4 = partials + 4 * (size_t)gridDim.x;
  if (threadIdx.x == 0) store_partial(slot4 + blockIdx.x, tw);
  if (!last_block_arrives(ticket, gridDim.x, s_red)) return;
  double a = 0.0;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += BLOCK) a += load_partial(slot4 + i);
  const double t = block_sum(a, s_red);
  if (threadIdx.x == 0) {
    sc[S_RED0 + 4] = t;
    derive(PH_BICG_S, sc);
  }
}

// x += αp + ωs;  r = s - ωt;  p = r + β(p - ωv)  (restart: p = r̂ = r);  partial slot 1 = (r,r)_W (convergence, weights
// ds²: pg_spmv.h), slot 2 = (r,r) (restart bookkeeping).
// β is known before r exists because ρ_new = (r̂,r) = (r̂,s) - ω(r̂,t) comes out of the dots of k_bicg_s and of the
// second SpMV: the classical p-update kernel (4 vector passes) and one scalar kernel per iteration disappear.
// shat != nullptr: the preconditioned loop -- x += ω M⁻¹s (α M⁻¹p went in with k_bicg_s_x), through the index map of a
// compact system
__global__ __launch_bounds__(BLOCK) void k_bicg_xrp(i64 n, double* sc, const double* __restrict__ t,
                                                    const double* __restrict__ v, double* __restrict__ x,
                                                    double* __restrict__ r, double* __restrict__ p,
                                                    double* __restrict__ rhat, double* __restrict__ partials,
                                                    const double* __restrict__ ds, int p_in_rhat,
                                                    const double* __restrict__ shat, const int* __restrict__ map) {
  __shared__ double s_red[BLOCK / 64];
  if (sc[S_DONE] != 0.0) return;
  const double alpha = sc[S_ALPHA], omega = sc[S_OMEGA], beta = sc[S_BETA];
  const bool restart = sc[S_RESTART] != 0.0;
  const bool prhat = p_in_rhat != 0 && sc[S_ITERS] == 0.0;   // first iteration of a start that left p = r̂ unwritten
  double a0 = 0.0, aw = 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    const double si = r[i], pi = prhat ? rhat[i] : p[i];
    if (shat) {
      // (`0.0 +` keeps ω M⁻¹s rounded on its own before the add, as this update has always been computed: one fma with x
      // would round differently)
      x[map ? map[i] : i] += 0.0 + omega * __builtin_nontemporal_load(shat + i);
    } else {
      const double xi = __builtin_nontemporal_load(x + i) + alpha * pi + omega * si;
      __builtin_nontemporal_store(xi, x + i);
    }
    const double ri = si - omega * __builtin_nontemporal_load(t + i);
    r[i] = ri;
    if (restart) {
      p[i] = ri;
      rhat[i] = ri;
    } else {
      p[i] = ri + beta * (pi - omega * __builtin_nontemporal_load(v + i));
    }
    a0 += ri * ri;
    const double wr = ds[i] * ri;
    aw += wr * wr;
  }
  // slots 1, 2: summed together with the next SpMV's (r̂,v) in slot 0 (or alone, before a host poll)
  const double tw = block_sum(aw, s_red);
  if (threadIdx.x == 0) partials[(size_t)gridDim.x + blockIdx.x] = tw;
  const double t0 = block_sum(a0, s_red);
  if (threadIdx.x == 0) partials[2 * (size_t)gridDim.x + blockIdx.x] = t0;
  if (blockIdx.x == 0 && threadIdx.x == 0) sc[S_PENDING3] = 1.0;   // (only the scalar kernels read it)
}

__global__ __launch_bounds__(BLOCK) void k_cg_init(i64 n, i64 nvec, const double* __restrict__ b, double* __restrict__ x,
                                                   double* __restrict__ r, double* __restrict__ p,
                                                   double* __restrict__ partials, const double* __restrict__ ds) {
  __shared__ double s_red[BLOCK / 64];
  double acc = 0.0, accw = 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < nvec; i += (i64)gridDim.x * BLOCK) {
    if (i < n) {
      const double bi = b[i];
      x[i] = 0.0; r[i] = bi; p[i] = bi;
      acc += bi * bi;
      accw += (ds[i] * bi) * (ds[i] * bi);
    } else {
      x[i] = 0.0; p[i] = 0.0;
    }
  }
  const double t = block_sum(acc, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
  const double tw = block_sum(accw, s_red);
  if (threadIdx.x == 0) partials[gridDim.x + blockIdx.x] = tw;
}

__global__ __launch_bounds__(BLOCK) void k_cg_xr(i64 n, const double* __restrict__ sc, const double* __restrict__ p,
                                                 const double* __restrict__ q, double* __restrict__ x,
                                                 double* __restrict__ r, double* __restrict__ partials,
                                                 const double* __restrict__ ds) {
  __shared__ double s_red[BLOCK / 64];
  if (sc[S_DONE] != 0.0) return;
  const double alpha = sc[S_ALPHA];
  double a0 = 0.0, aw = 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    x[i] += alpha * p[i];
    const double ri = r[i] - alpha * q[i];
    r[i] = ri;
    a0 += ri * ri;
    aw += (ds[i] * ri) * (ds[i] * ri);
  }
  const double t0 = block_sum(a0, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t0;
  const double tw = block_sum(aw, s_red);
  if (threadIdx.x == 0) partials[gridDim.x + blockIdx.x] = tw;
}

__global__ __launch_bounds__(BLOCK) void k_cg_p(i64 n, const double* __restrict__ sc, const double* __restrict__ r,
                                                double* __restrict__ p) {
  if (sc[S_DONE] != 0.0) return;
  const double beta = sc[S_BETA];
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) p[i] = r[i] + beta * p[i];
}

// ---- scalar phase: sum block partials (deterministic order), then derive the iteration scalars (pg_spmv.h) ----
__global__ __launch_bounds__(BLOCK) void k_finalize(int phase, int slot0, int nslots, int grid,
                                                    const double* __restrict__ partials, double* __restrict__ sc,
                                                    int do_derive, int check_done) {
  __shared__ double s_red[BLOCK / 64];
  if (check_done && sc[S_DONE] != 0.0) return;
  for (int s = slot0; s < slot0 + nslots; ++s) {
    double a = 0.0;
    for (int i = threadIdx.x; i < grid; i += BLOCK) a += partials[(size_t)s * grid + i];
    const double t = block_sum(a, s_red);
    if (threadIdx.x == 0) sc[S_RED0 + s] = t;
  }
  if (do_derive && threadIdx.x == 0) derive(phase, sc);
}

// fresh scalar block of a solve: everything zero but the squared tolerances
__global__ void k_sc_reset(double* sc, double reltol2, double abstol2) {
  const int i = threadIdx.x;
  if (i < S_COUNT) sc[i] = i == S_RELTOL2 ? reltol2 : (i == S_ABSTOL2 ? abstol2 : 0.0);
}

// k_sc_reset + the start phase's k_finalize in one launch (one rank, BiCGStab with a prepared start: nothing reads the
// scalars in between)
__global__ __launch_bounds__(BLOCK) void k_start(int phase, int nslots, int grid, const double* __restrict__ partials,
                                                 double* __restrict__ sc, double reltol2, double abstol2) {
  __shared__ double s_red[BLOCK / 64];
  if (threadIdx.x < S_COUNT) sc[threadIdx.x] = threadIdx.x == S_RELTOL2 ? reltol2 : (threadIdx.x == S_ABSTOL2 ? abstol2 : 0.0);
  __syncthreads();
  for (int s = 0; s < nslots; ++s) {
    double a = 0.0;
    for (int i = threadIdx.x; i < grid; i += BLOCK) a += partials[(size_t)s * grid + i];
    const double t = block_sum(a, s_red);
    if (threadIdx.x == 0) sc[S_RED0 + s] = t;
  }
  if (threadIdx.x == 0) derive(phase, sc);
}

__global__ void k_derive(int phase, double* sc, int check_done) {
  if (check_done && sc[S_DONE] != 0.0) return;
  derive(phase, sc);
}

// The start phase of a prepared start on several ranks that carries KrylovCall::moved_flag: k_finalize's sums of the three
// start slots, and S_RED3 = 1 when a row alone on its diagonal moved on this rank (0 otherwise) ...
__global__ __launch_bounds__(BLOCK) void k_start_sums_moved(int grid, const double* __restrict__ partials, double* __restrict__ sc,
                                                            const int* __restrict__ flag, int stamp) {
  __shared__ double s_red[BLOCK / 64];
  for (int s = 0; s < 3; ++s) {
    double a = 0.0;
    for (int i = threadIdx.x; i < grid; i += BLOCK) a += partials[(size_t)s * grid + i];
    const double t = block_sum(a, s_red);
    if (threadIdx.x == 0) sc[S_RED0 + s] = t;
  }
  if (threadIdx.x == 0) sc[S_RED0 + 3] = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == stamp ? 1.0 : 0.0;
}

// ... and, behind the all-reduce of the four: PH_INIT and the verdict every rank shares (how many ranks saw one move)
__global__ void k_derive_start_moved(double* sc) {
  derive(PH_INIT, sc);
  sc[S_MOVED] = sc[S_RED0 + 3] != 0.0 ? 1.0 : 0.0;
}

// after a launch whose last block already summed (and, on one rank, derived) the phase: only what is left to do
void finalize_folded(int phase, int nslots, KrylovWork& w, hipStream_t st) {
  Context& cx = ctx();
  if (cx.nranks == 1 && !cx.comm) return;
  comm_allreduce_sum_f64(w.sc.p + S_RED0, nslots, st);
  hipLaunchKernelGGL(k_derive, dim3(1), dim3(1), 0, st, phase, w.sc.p, 1);
}

void finalize(int phase, int nslots, KrylovWork& w, hipStream_t st, bool check_done, int slot0 = 0) {
  Context& cx = ctx();
  if (cx.nranks == 1 && !cx.comm) {
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, st, phase, slot0, nslots, w.grid, w.partials.p, w.sc.p, 1,
                       check_done ? 1 : 0);
  } else {
    // local sums -> RCCL all-reduce of <= 5 doubles over xGMI -> identical scalars on every rank
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, st, phase, slot0, nslots, w.grid, w.partials.p, w.sc.p, 0,
                       check_done ? 1 : 0);
    comm_allreduce_sum_f64(w.sc.p + S_RED0 + slot0, nslots, st);
    hipLaunchKernelGGL(k_derive, dim3(1), dim3(1), 0, st, phase, w.sc.p, check_done ? 1 : 0);
  }
}

struct SpmvTimer {
  bool on;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pairs;
  std::vector<int> iter_of;   // Krylov iteration each launch belongs to
  std::vector<char> lean_of;  // 1: lean launch (no dots), 0: launch with fused dots
  std::vector<char> second_of;   // 1: launch of the second half of its iteration (skipped when the half step was accepted)
  std::vector<int> count_of;     // launches between the two events (a chain of lean launches is bracketed as a whole)
  std::vector<char> f32_of;      // 1: the fp32 launches of a mixed chain (counters of their own: spmv_lean_* stays the fp64 Horner step)
  int cur = 0, cur_count = 1;
  bool cur_lean = false, cur_second = false, cur_f32 = false;
  bool armed = false;
  explicit SpmvTimer(bool on_) : on(on_) {}
  // events are recycled through a per-thread pool: nothing is created or destroyed inside the time loop after the
  // first profiled solve
  static std::vector<hipEvent_t>& pool() {
    static thread_local std::vector<hipEvent_t> p;
    return p;
  }
  static hipEvent_t take() {
    auto& p = pool();
    if (!p.empty()) {
      hipEvent_t e = p.back();
      p.pop_back();
      return e;
    }
    hipEvent_t e;
    PG_HIP(hipEventCreate(&e));
    return e;
  }
  void begin(hipStream_t st, int iteration, bool lean = false, bool second = false, int count = 1, bool f32 = false) {
    cur = iteration;
    cur_lean = lean;
    cur_second = second;
    cur_count = count;
    cur_f32 = f32;
    // every `sample`-th bracket is timed (PG_PROFILE_SAMPLE, default 3 -- coprime with the 4 brackets of an iteration: the
    // chain of lean launches and the closing launch of each half, so all four are sampled in turn).  A pair of event
    // records costs the stream ~10 µs (the kernel behind a record starts late): a lean chain is bracketed as a WHOLE so
    // that this cost is spread over its m - 1 launches; rocprofv3's per-kernel durations (profiles/) are the cross-check
    const int sample = config().profile_sample;
    // (the fp32 bracket of a mixed chain draws from a counter of its own: the turn of the other brackets is what it was)
    static thread_local unsigned long long counter = 0, counter_f32 = 0;
    armed = on && ((f32 ? counter_f32++ : counter++) % sample == 0);
    if (!armed) return;
    e0 = take();
    e1 = take();
    PG_HIP(hipEventRecord(e0, st));
  }
  void end(hipStream_t st) {
    if (!armed) return;
    PG_HIP(hipEventRecord(e1, st));
    pairs.emplace_back(e0, e1);
    iter_of.push_back(cur);
    lean_of.push_back(cur_lean ? 1 : 0);
    second_of.push_back(cur_second ? 1 : 0);
    count_of.push_back(cur_count);
    f32_of.push_back(cur_f32 ? 1 : 0);
  }
  // launches queued after convergence return at their first instruction (done flag): they are not SpMVs and are
  // left out of the launch count and of the average
  void collect(SolveStats& s, int iters_done, bool half_exit) {
    for (size_t q = 0; q < pairs.size(); ++q) {
      auto& pr = pairs[q];
      float ms = 0.f;
      (void)hipEventSynchronize(pr.second);
      const bool ran = iter_of[q] < iters_done && !(half_exit && iter_of[q] == iters_done - 1 && second_of[q]);
      if (ran && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
        if (f32_of[q]) { s.f32_ms += ms; s.f32_timed += count_of[q]; }
        else if (lean_of[q]) { s.spmv_lean_ms += ms; s.spmv_lean_launches += count_of[q]; }
        else { s.spmv_ms += ms; s.spmv_launches += 1; }
      }
      pool().push_back(pr.first);
      pool().push_back(pr.second);
    }
    pairs.clear();
    iter_of.clear();
    lean_of.clear();
    second_of.clear();
    count_of.clear();
    f32_of.clear();
  }
};

}  // namespace

namespace pg {

double g_host_wait_us = 0.0;
int g_poly_give_up = 0;

void KrylovWork::init(i64 n_own, i64 n_vec) {
  n = n_own;
  nvec = n_vec;
  const i64 a = n_vec > 0 ? n_vec : 1;
  r.alloc(a); rhat.alloc(a); p.alloc(a); v.alloc(a); t.alloc(a);
  grid = spmv_default_grid(n_own);
  partials.alloc(5 * (i64)grid);
  sc.alloc(S_COUNT);
  sc.zero();
  ticket.alloc(1);
  ticket.zero();
  if (!h_sc) PG_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_sc), sizeof(double) * S_COUNT));
}

KrylovWork::~KrylovWork() {
  if (h_sc) (void)hipHostFree(h_sc);
  if (ev_poll) (void)hipEventDestroy(ev_poll);
}

void spmv_halo(const CsrMatrix& A, const Numbering& nb, const Slab& slab, double* x, double* y, hipStream_t st) {
  spmv_with_halo(0, A, nb, slab, x, y, nullptr, nullptr, nullptr, spmv_default_grid(A.n), st);
  PG_HIP(hipGetLastError());
}

void spmv(const CsrMatrix& A, const double* x, double* y, hipStream_t st) {
  if (A.n == 0) return;
  launch_spmv(0, A, x, y, nullptr, nullptr, nullptr, spmv_default_grid(A.n), st);
  PG_HIP(hipGetLastError());
}

const char* krylov_method_refusal(int method) {
  return method == PG_METHOD_CG ? "the method is CG (BiCGStab only)"
         : method == PG_METHOD_BICGSTABL ? "the method is BiCGStab(l) (BiCGStab only)"
         : method == PG_METHOD_IDRS ? "the method is IDR(s) (BiCGStab only)" : "the method is GMRES (BiCGStab only)";
}

bool krylov_uses_polynomial(const CsrMatrix& A, const pg_krylov_opts& opts) {
  const bool poly_env = config().poly;
  const int degree_env = config().poly_degree;
  // (PG_PRECOND_POLY_EST on a matrix Gershgorin admits is precond = 0; one it refuses never comes here as a compact system)
  const int precond = opts.precond == PG_PRECOND_POLY_EST ? 0 : opts.precond;
  if (!(poly_env && precond >= 0 && opts.method == PG_METHOD_BICGSTAB && A.poly_ok && spmv_supports_preconditioner_product() && A.n > 0))
    return false;
  return (precond > 0 ? precond : degree_env) >= 2;
}

constexpr int MAX_POLY_DEGREE = 40;   // products per application of the polynomial preconditioner

namespace {

// Degree for the next solve on this matrix (auto mode: the loop's warm solves, whose start residual and tolerance move slowly
// from step to step).  This solve applied P = (2 iters - half) m products and took (r,r)_W from rr0 to rr; at that rate the
// tolerance needed  P log(tol²/rr0) / log(rr/rr0)  of them: take the (applications h, degree m) with h m >= need that is
// cheapest.  The polynomial need not be exact (x and r move by the SAME computed M⁻¹p, so r stays the residual of x whatever
// rounding does inside the Horner chain): the cheapest is ONE application of degree ~26 that ends at the half-step test --
// a Chebyshev step with BiCGStab's α, its residual test and, if the estimate was short, its continuation (444 -> 546 steps/s
// at 512^3 against 3 x 9).  No safety margin: a miss costs one more application once, and the next estimate is made from
// that solve.
// what an all-fp32 (middle) Horner launch costs, in fp64 Horner launches: 47.7 against 54.7 us per launch at 512^3 in the kernel
// trace (profiles/f32_chain_kernel_stats_*.csv) -- the launch moves 0.61 of the bytes but is not bound by them.  The first launch
// (two fp32 vectors out) and the hand-over (fp64 base in, fp64 out) are no cheaper than an fp64 launch and get no discount.
constexpr double F32_LAUNCH_WEIGHT = 0.87;

// mixed_g > 0: the next solve's first application may run the mixed chain on a spectrum of radius mixed_g (its fp32 launches
// are cheaper); the reduction that application must deliver, and with it the length of the fp64 tail, goes with (h, m)
void choose_next_degree(const CsrMatrix& A, const SolveStats& stats, int m, bool adaptive, KrylovWork& w, double mixed_g) {
  const Config& cfg = config();
  const bool keep_degree = adaptive && stats.converged && stats.iters == 0 && w.adapt_m >= 2;   // met the tolerance at the start:
  w.adapt_matrix = nullptr;                                                                      // the smallest polynomial next time
  if (keep_degree) { w.adapt_matrix = &A; w.adapt_m = cfg.poly_mindeg; w.adapt_h = 1; }
  if (!(adaptive && stats.converged && stats.iters > 0)) return;
  const double rr0 = w.h_sc[S_RR0], rr = w.h_sc[S_HALF] != 0.0 ? w.h_sc[S_RED4] : w.h_sc[S_RR], tol2 = w.h_sc[S_TOL2];
  const double P = (2.0 * stats.iters - stats.half_exit) * m;
  if (!(rr0 > tol2 && rr > 0.0 && rr < rr0 && tol2 > 0.0)) return;
  w.last_rate2 = std::log(rr0 / rr) / P;
  const double margin = cfg.poly_margin;
  // a third of a product of slack -- with ONE application per solve a miss costs a whole second one, and the estimate moves
  // by a few tenths from step to step (200 steps at 512^3: 7 % of the solves missed without it, 548 steps/s; 1.75 % with 0.3:
  // 575; none with 0.6: 600 -- but 27 instead of 26 products in the bench's first 20 steps)
  const double slack_env = cfg.poly_slack;
  const double slack = slack_env >= 0.0 ? slack_env : 0.3;
  const double need_now = std::min(P, P * std::log(tol2 / rr0) / std::log(rr / rr0)) * margin + slack;
  // the largest of the last three estimates on this matrix: the estimate wobbles by a few tenths of a product from step
  // to step, and with one application per solve falling short by a tenth costs a whole second application
  const int hist_n = cfg.poly_hist;
  if (w.need_matrix != &A) { w.need_matrix = &A; w.need_hist[0] = w.need_hist[1] = w.need_hist[2] = 0.0; }
  w.need_hist[2] = w.need_hist[1]; w.need_hist[1] = w.need_hist[0]; w.need_hist[0] = need_now;
  double need = need_now;
  // The estimates of a run move along a trend (the start residual falls from step to step -- by a third of a product per
  // step while the extrapolated start of pg_solver.hip settles in) with a wobble of a few tenths on top.  Trend: half the
  // change over the last two steps; the older estimates are carried along it before the largest is taken (the wobble
  // guard), and the next solve gets the value the trend predicts for it.  (Without the trend the guard alone kept the
  // degree 0.6 + a step's change above what was needed all the way down: one product per step in the bench window.)
  double trend = 0.0;
  if (cfg.poly_trend && hist_n >= 3 && w.need_hist[2] > 0.0) trend = std::max(-0.5, std::min(0.2, 0.5 * (need_now - w.need_hist[2])));
  for (int q = 1; q < hist_n; ++q)
    if (w.need_hist[q] > 0.0) need = std::max(need, std::min(w.need_hist[q] + q * trend, need_now + 0.6));   // (wobble, not trend)
  need += trend;
  double best = 1e300;
  for (int h = 1; h <= 16; ++h) {
    // (a need below the smallest polynomial -- an extrapolated start close to the tolerance, a field close to steady -- takes
    //  the smallest one; it used to find no admissible degree, which sent the next solve back to the first-solve default
    //  and its extra polls: 64^3 near steady state 240 us per step with 3 products, 150 with 16)
    const int mm = std::max(cfg.poly_mindeg, (int)std::ceil(need / h));
    const int maxdeg = cfg.poly_maxdeg > 0 ? std::min(MAX_POLY_DEGREE, std::max(4, cfg.poly_maxdeg)) : 32;
    if (mm > maxdeg) continue;
    // an application: a chain of one lean launch + mm - 2 Horner launches (1.18 lean launches each), the closing launch and
    // the vector kernel ≈ 3.6
    double cost = h * (1.0 + 1.18 * (mm - 2) + 3.6);
    if (mixed_g > 0.0) {
      const int jt = pghost::mixed_chain_tail(std::pow(std::sqrt(tol2 / rr0), 1.0 / h), mixed_g, mm);
      if (jt >= 0) cost -= (1.0 - F32_LAUNCH_WEIGHT) * 1.18 * (mm - jt - 2);   // the middle launches: mm - 1 - jt fp32 stores less the first
    }
    if (cost < best) { best = cost; w.adapt_m = mm; w.adapt_h = h; }
  }
  if (best < 1e300) w.adapt_matrix = &A;
  // One application per solve: what a degree achieves is not monotone in the degree -- the residual polynomial at the few
  // eigenvalues that carry an extrapolated start's residual goes like |cos(m θ)| on top of the Chebyshev bound, so the
  // estimate made at a lucky degree can undershoot by a product (512^3, step 96: 12, 11, 10 all reached the same residual,
  // 9 fell short; the loop then cycled 11, 11, 10, 9+9).  A degree that fell short is therefore not tried again for a while
  // -- twice what the miss cost, in steps (a miss costs about m + 3 products, a degree less saves one per step), doubled
  // each time the same degree falls short again -- unless the problem has become easier by a product's worth per degree
  // first; and the solve after a miss goes back to the degree that last sufficed.
  if (stats.iters == 1) {
    const double Lnow = std::log(rr0 / tol2);
    if (w.fail_matrix != &A) { w.fail_matrix = &A; w.fail_deg = 0; w.good_deg = 0; w.fail_wait = 0; w.fail_backoff = 1; }
    if (w.fail_wait > 0) --w.fail_wait;
    if (stats.half_exit) w.good_deg = m;
    else {
      w.fail_backoff = (m == w.fail_deg) ? std::min(w.fail_backoff * 2, 64) : 1;
      w.fail_deg = m; w.fail_L = Lnow;
      w.fail_wait = 2 * w.fail_backoff * (m + 3);
    }
    if (best < 1e300 && w.adapt_h == 1) {
      if (!stats.half_exit && w.good_deg > m) w.adapt_m = std::max(m + 1, std::min(w.adapt_m, w.good_deg));
      const double per_product = std::max(1.0, w.last_rate2);
      if (w.fail_deg > 0 && w.fail_wait > 0 && w.adapt_m <= w.fail_deg &&
          Lnow > w.fail_L - per_product * (w.fail_deg - w.adapt_m + 1))
        w.adapt_m = w.fail_deg + 1;
    }
  }
  if (cfg.debug) fprintf(stderr, "[pg_krylov] degree %d used %g products, needed %.1f -> next: %d applications of degree %d\n", m, P, need, w.adapt_h, w.adapt_m);
}

}  // namespace

void krylov_solve(const CsrMatrix& A, const Numbering& nb, const Slab& slab, const double* b, double* x, KrylovWork& w,
                  const pg_krylov_opts& opts, SolveStats& stats, const KrylovCall& call) {
  const double *const x0 = call.x0, *const Ax0 = call.Ax0;
  const bool preinit = call.preinit;
  Context& cx = ctx();
  hipStream_t st = cx.stream;
  const i64 n = A.n, nvec = nb.n_vec();
  PG_REQUIRE(w.n >= n && w.nvec >= nvec, "krylov workspace too small");   // (a reduced system works on prefixes, pg_reduce.hip)
  PG_REQUIRE(opts.method == PG_METHOD_BICGSTAB || opts.method == PG_METHOD_CG || opts.method == PG_METHOD_GMRES ||
                 opts.method == PG_METHOD_BICGSTABL || opts.method == PG_METHOD_IDRS,
             "unknown Krylov method");
  // PG_PRECOND_POLY_EST: precond = 0 wherever Gershgorin admits the matrix; where it refuses, the verdict of the spectral
  // estimate the caller has run on this matrix (CsrMatrix::est, pg_specest.hip) -- a flag of its own, poly_ok stays false
  const bool est_opt = opts.precond == PG_PRECOND_POLY_EST;
  if (est_opt) {
    PG_REQUIRE(opts.method == PG_METHOD_BICGSTAB,
               std::string("estimated polynomial preconditioner (precond = PG_PRECOND_POLY_EST) refused: ") +
                   krylov_method_refusal(opts.method));
    specest_require_one_rank();
    // the contract: whoever passes the option has run the estimate on THIS matrix (pg_solver.hip specest_prepare) -- a
    // matrix nobody looked at would otherwise run plain without a word.  (A matrix the polynomial stagnated on has its verdict:
    // it runs plain, here as the plain finish of that very solve and in every later one.)
    PG_REQUIRE(A.poly_ok || A.est.tried || A.poly_gave_up, "estimated polynomial preconditioner (precond = PG_PRECOND_POLY_EST): no spectral estimate "
               "has run on this matrix (specest_run before krylov_solve)");
  }
  const int precond = est_opt ? 0 : opts.precond;
  // the one place that decides what a method accepts of a call: what it cannot honour is refused, never dropped
  PG_REQUIRE((preinit && opts.method == PG_METHOD_BICGSTAB) ||
                 !(call.p_in_rhat || call.start_folded || call.xguess.zbase || call.scatter || call.moved_flag || call.after_first_batch),
             "krylov_solve: p_in_rhat, start_folded, xguess, scatter, moved_flag and after_first_batch belong to a prepared start "
             "(preinit) of the BiCGStab loop");
  PG_REQUIRE(!call.mg || mg_any_precond(opts.precond), "krylov_solve: a multigrid hierarchy was handed over without a multigrid precond");
  if (opts.method == PG_METHOD_GMRES) {
    PG_REQUIRE(!mg_is_step(opts.precond), std::string("multigrid preconditioner (precond = PG_PRECOND_MG_STEP) refused: ") +
                                              krylov_method_refusal(opts.method));
    PG_REQUIRE(!preinit && !x0, "GMRES starts from zero (IterativeSolvers' default)");
    gmres_solve(A, nb, slab, b, x, w, opts, stats);
    return;
  }
  if (opts.method == PG_METHOD_BICGSTABL) {
    // opt-in, plain: every preconditioner of the BiCGStab loop is refused with it rather than dropped without a word
    PG_REQUIRE(!preinit && !x0, "BiCGStab(l) starts from zero (IterativeSolvers' default)");
    PG_REQUIRE(!mg_any_precond(opts.precond), std::string("multigrid preconditioner (precond = ") + mg_precond_name_of(opts.precond) +
                                                  ") refused: " + krylov_method_refusal(opts.method));
    PG_REQUIRE(opts.precond <= 0, "polynomial preconditioner (precond = " + std::to_string(opts.precond) + ") refused: " +
                                      krylov_method_refusal(opts.method) + "; precond = 0 or -1 runs BiCGStab(l) plain");
    bicgstabl_solve(A, nb, slab, b, x, w, opts, stats);
    return;
  }
  if (opts.method == PG_METHOD_IDRS) {
    // opt-in, plain, as BiCGStab(l); it honours x0 / Ax0 (no prepared start: that is the BiCGStab loop's own)
    PG_REQUIRE(!preinit, "IDR(s) refused: a prepared start (preinit) is the BiCGStab loop's alone; pass x0 and Ax0");
    PG_REQUIRE(!mg_any_precond(opts.precond), std::string("multigrid preconditioner (precond = ") + mg_precond_name_of(opts.precond) +
                                                  ") refused: " + krylov_method_refusal(opts.method));
    PG_REQUIRE(opts.precond <= 0, "polynomial preconditioner (precond = " + std::to_string(opts.precond) + ") refused: " +
                                      krylov_method_refusal(opts.method) + "; precond = 0 or -1 runs IDR(s) plain");
    idrs_solve(A, nb, slab, b, x, w, opts, stats, x0, Ax0);
    return;
  }
  const int G = w.grid;
  const int check_every = opts.check_every > 0 ? opts.check_every : 4;
  int maxiter = opts.maxiter;
  if (maxiter <= 0) {
    // IterativeSolvers default: size of the system (global)
    maxiter = 100000;
  }
  // tolerances -> device scalars (a one-thread kernel: a host-to-device copy out of pageable memory stalls the stream)
  const bool p_in_rhat = call.p_in_rhat, start_folded = call.start_folded;
  const XGuess& xg = call.xguess;      // (first update of x out of place: see KrylovCall::xguess)
  const int* const scatter = call.scatter;
  PG_REQUIRE(scatter || !call.row_const.tab, "krylov_solve: row_const describes scatter and is refused without it");
  const RowConst rc = call.row_const;
  const bool fused_start = !start_folded && preinit && opts.method == PG_METHOD_BICGSTAB && cx.nranks == 1 && !cx.comm;   // k_start below
  if (!fused_start && !start_folded)
    hipLaunchKernelGGL(k_sc_reset, dim3(1), dim3(S_COUNT), 0, st, w.sc.p, opts.reltol * opts.reltol, opts.abstol * opts.abstol);
  SpmvTimer timer(cx.profiling);

  const bool cg = opts.method == PG_METHOD_CG;
  const Config& cfg = config();
  const bool poly_env = cfg.poly;
  const int degree_env = cfg.poly_degree;
  // polynomial right preconditioner: BiCGStab on the slice kernel, where Gershgorin bounds the spectrum inside
  // |λ - 1| < 0.95; m products with Â per application of C = I - R(Â)  (m < 2: the plain iteration)
  int m = 0;
  const bool by_estimate = est_opt && !A.poly_ok && !A.poly_gave_up && A.est.tried && A.est.admitted;   // (Gershgorin admits: no estimate is looked at)
  if (poly_env && precond >= 0 && !cg && (A.poly_ok || by_estimate) && spmv_supports_preconditioner_product() && n > 0)
    m = std::min(precond > 0 ? precond : degree_env, MAX_POLY_DEGREE);
  // auto mode: the degree that fits the number of products the previous solve on this matrix would have needed (below)
  const bool adapt_env = cfg.poly_adapt;
  const bool adaptive = adapt_env && m >= 2 && precond == 0 && preinit;
  int expect_halves = 0;
  if (adaptive && w.adapt_matrix == &A && w.adapt_m >= 2) { m = w.adapt_m; expect_halves = w.adapt_h; }
  if (m < 2) m = 0;
  const bool poly = m > 0;
  MgHierarchy* const mgh = call.mg;
  const bool mg = mg_any_precond(opts.precond);   // (PG_PRECOND_MG_STEP: the same loop from the time loop's prepared start)
  if (mg) {
    PG_REQUIRE(!cg, "multigrid preconditioner refused: the method must be BiCGStab");
    PG_REQUIRE(spmv_supports_preconditioner_product(), "multigrid preconditioner refused: the x-space loop needs the slice kernel (PG_SPMV_VARIANT)");
    mg_require_one_rank_of(opts.precond);
    PG_REQUIRE(mgh && !scatter && !xg.zbase && n > 0,
               mg_is_step(opts.precond)
                   ? "multigrid preconditioner refused: this solve has no hierarchy (the full systems of the unsteady monophasic "
                     "diffusion time loop only)"
                   : "multigrid preconditioner refused: this solve has no hierarchy (steady monophasic "
                     "diffusion systems and the stream-function solve only)");
    PG_REQUIRE(mgh->rule == mg_rule_of_any(opts.precond) && mgh->matrix == &A,
               std::string("multigrid preconditioner: the hierarchy handed over was not built for precond = ") +
                   mg_precond_name_of(opts.precond));
  }
  const bool pre = poly || mg;   // right-preconditioned: x moves by α M⁻¹p (k_bicg_s_x) and ω M⁻¹s (k_bicg_xrp)
  stats.poly_degree = m;
  stats.poly_xspace = poly ? 1 : 0;
  PG_REQUIRE(!scatter || (poly && preinit), "a compact system needs the polynomial path and a prepared start");
  double tau[MAX_POLY_DEGREE];
  if (poly) {
    // 1 / Chebyshev nodes of [1 - g, 1 + g], the largest and the smallest remaining root in turn
    const double g = std::min(std::max(by_estimate ? A.est.g_used : A.gersh, 0.05), 0.95);
    double lam[MAX_POLY_DEGREE];
    for (int k = 0; k < m; ++k) lam[k] = 1.0 + g * std::cos(M_PI * (2.0 * k + 1.0) / (2.0 * m));   // descending
    for (int k = 0, lo = 0, hi = m - 1; k < m; ++k) tau[k] = 1.0 / ((k & 1) ? lam[hi--] : lam[lo++]);
  }
  if (pre && w.ya.n < nvec) {
    w.ya.alloc(nvec); w.wa.alloc(nvec); w.wb.alloc(nvec); w.yb.alloc(nvec);
    w.ya.zero(); w.wa.zero(); w.wb.zero(); w.yb.zero();
  }
  // Mixed-precision chain.  The chain is only a preconditioner (x and r move by the same computed vectors), so
  // its early intermediates need not be stored with 53 bits: the first application of a solve stores the results of its first
  // n32 launches as fp32 (scaled by the power of two σ: the chain is linear) and hands over to the j fp64 launches of the tail,
  // which damp that rounding below what the solve needs (pghost::mixed_chain_schedule / mixed_chain_tail).  It runs where the
  // loop system references no ghost column on ONE rank (the root order has to be the same wherever a halo couples the ranks,
  // and the halo exchange is fp64), with σ and the needed reduction left by the previous solve on this matrix -- scalars every
  // rank holds identically; a solve without them (the first on a matrix) runs all fp64, and so does every application after
  // the first of a solve: the continuation of a solve that missed its half-step test is exact, and the next 2 (m + 3) solves
  // -- the horizon of the degree's backoff -- run a tail two launches longer.
  pghost::MixedChain mc;
  bool mixed = false;
  double mix_sigma = 1.0;
  double mtau[MAX_POLY_DEGREE];     // 1 / root, in the mixed chain's order of application
  if (poly && cfg.poly_f32 && cx.nranks == 1 && !cx.comm && !A.halo_needed && spmv_supports_typed_chain() && w.mix_matrix == &A &&
      w.mix_sigma > 0.0) {
    const double g = std::min(std::max(by_estimate ? A.est.g_used : A.gersh, 0.05), 0.95);
    int j = cfg.poly_f32_tail >= 0 ? cfg.poly_f32_tail : pghost::mixed_chain_tail(w.mix_need, g, m);
    if (j >= 0 && w.mix_wait > 0 && cfg.poly_f32_tail < 0) j += 2;   // (a forced tail stays what was asked for)
    if (w.mix_wait > 0) --w.mix_wait;
    if (j >= 0 && pghost::mixed_chain_schedule(m, g, j, mc)) {
      mixed = true;
      mix_sigma = w.mix_sigma;
      for (int i = 0; i < m; ++i) mtau[i] = 1.0 / pghost::mixed_root(m, g, mc.order[i]);
      if (w.fa.n < nvec) {
        w.fa.alloc(nvec); w.fb.alloc(nvec); w.p32.alloc(nvec);
        w.fa.zero(); w.fb.zero(); w.p32.zero();
      }
    }
  }
  bool mixed_ran = false;
  // convergence is also tested after the first half of an iteration when a half costs several products (the test itself
  // costs two small launches)
  const bool half_test = m >= 3 || mg;
  PG_REQUIRE(!xg.zbase || (poly && p_in_rhat && scatter), "an unformed extrapolated state needs the polynomial loop on a compact system");
  PG_REQUIRE(!preinit || !cg, "preinit is a BiCGStab path");
  if (!cg) {
    if (!preinit)
      hipLaunchKernelGGL(k_bicg_init, dim3(G), dim3(BLOCK), 0, st, n, nvec, b, x0, Ax0, x, w.r.p, w.rhat.p, w.p.p, w.v.p,
                       w.partials.p, (const double*)A.ds.p);
    static_assert(S_COUNT <= BLOCK, "k_start resets the scalar block with one thread per scalar");
    if (start_folded) {
    } else if (fused_start)
      hipLaunchKernelGGL(k_start, dim3(1), dim3(BLOCK), 0, st, (int)PH_INIT, 3, w.grid, (const double*)w.partials.p, w.sc.p,
                         opts.reltol * opts.reltol, opts.abstol * opts.abstol);
    else if (call.moved_flag && !(cx.nranks == 1 && !cx.comm)) {
      // finalize(PH_INIT) with one more slot in the same all-reduce: did a row alone on its diagonal move on ANY rank?
      hipLaunchKernelGGL(k_start_sums_moved, dim3(1), dim3(BLOCK), 0, st, w.grid, (const double*)w.partials.p, w.sc.p, call.moved_flag,
                         call.moved_stamp);
      comm_allreduce_sum_f64(w.sc.p + S_RED0, 4, st);
      hipLaunchKernelGGL(k_derive_start_moved, dim3(1), dim3(1), 0, st, w.sc.p);
    } else
      finalize(PH_INIT, 3, w, st, false);
  } else {
    hipLaunchKernelGGL(k_cg_init, dim3(G), dim3(BLOCK), 0, st, n, nvec, b, x, w.r.p, w.p.p, w.partials.p, (const double*)A.ds.p);
    finalize(PH_CG_INIT, 2, w, st, false);
  }
  PG_HIP(hipGetLastError());

  // Iterations are queued in batches and the done flag is polled in between.  Consecutive time steps need almost
  // the same number of iterations, so the first batch runs up to one short of the previous solve's count and the
  // next few polls come after every iteration: no iterations are queued past convergence (each would still cost
  // its launch overheads), at the price of two or three extra stream syncs per solve.
  // With the half-step test a batch is counted in HALVES and may end in the middle of an iteration: when the previous
  // solve ended at a half step (the usual case: 3 applications of the polynomial), the second half of the last iteration
  // is not queued at all -- its 1 + m launches would each find the done flag and return, at ~5 us apiece.
  int launched = 0, polls = 0;          // launched: iterations whose first half is queued
  bool mid = false;                     // ... and the second half of the last one is not
  bool done = false, poly_failed = false;
  const int poly_give_up = g_poly_give_up > 0 ? g_poly_give_up : 40 + 400 / std::max(m, 1);   // iterations; an admitted system needs 2 .. 10
  const int derive_here = (cx.nranks == 1 && !cx.comm) ? 1 : 0;
  // out = C in = Â q(Â) in with the dots of the phase (mode 1: (r̂,out); 3: (out,in), (out,out), (r̂,out)); q(Â) in stays in
  // ya (first half) / yb (second half) for the update of x.  The plain iteration applies Â itself.
  auto apply = [&](double* in, double* out, int phase, int nslots, int itn) {
    const bool second = phase == PH_BICG_2;
    double* src = in;
    if (poly) {
      // hat = q(Â) in:  u_(m-1) = τ_(m-1) in,  u_k = τ_k in + (I - τ_k Â) u_(k+1),  hat = u_0   (mode 8: pc2 base + pc0 x + pc1 Â x;
      // the first launch has x = base = in)
      double* hat = second ? w.yb.p : w.ya.p;
      if (mixed && itn == 0 && !second) {
        // the mixed chain: launch i applies the root mtau[i + 1] (the first launch carries mtau[0] as its leading coefficient);
        // fp32 vectors hold σ u -- σ and 1/σ ride in the coefficients of the first and the hand-over launch, exactly
        const int n32 = mc.n32, nf32 = n32 + 1, nf64 = m - 1 - nf32;
        const void* src32 = nullptr;
        timer.begin(st, itn, true, second, nf32, true);
        for (int i = 0; i <= n32; ++i) {
          const double tk = mtau[i + 1];
          FinArgs f{nullptr, nullptr, PH_NONE, 0, 0, nullptr};
          if (i == 0) {
            float* dst = w.fa.p;
            f.pc0 = mix_sigma * mtau[0]; f.pc1 = -mix_sigma * (mtau[0] * tk); f.pc2 = mix_sigma * tk;
            f.base = in; f.p32 = w.p32.p; f.psig = mix_sigma;
            launch_spmv_typed(TYPED_FIRST, A, in, dst, w.sc.p, G, st, f);
            src32 = dst;
          } else if (i < n32) {
            float* dst = (i & 1) ? w.fb.p : w.fa.p;
            f.pc0 = 1.0; f.pc1 = -tk; f.pc2 = tk;
            f.base = reinterpret_cast<const double*>(w.p32.p);
            launch_spmv_typed(TYPED_MIDDLE, A, src32, dst, w.sc.p, G, st, f);
            src32 = dst;
          } else {
            double* dst = i == m - 2 ? hat : ((i & 1) ? w.wb.p : w.wa.p);
            const double inv = 1.0 / mix_sigma;
            f.pc0 = inv; f.pc1 = -inv * tk; f.pc2 = tk;
            f.base = in;
            launch_spmv_typed(TYPED_HANDOVER, A, src32, dst, w.sc.p, G, st, f);
            src = dst;
          }
        }
        timer.end(st);
        if (nf64 > 0) {
          timer.begin(st, itn, true, second, nf64);
          for (int i = n32 + 1; i <= m - 2; ++i) {
            double* dst = i == m - 2 ? hat : ((i & 1) ? w.wb.p : w.wa.p);
            FinArgs f{nullptr, nullptr, PH_NONE, 0, 0, nullptr};
            f.pc0 = 1.0; f.pc1 = -mtau[i + 1]; f.pc2 = mtau[i + 1]; f.base = in;
            launch_spmv(8, A, src, dst, nullptr, nullptr, w.sc.p, G, st, &f);
            src = dst;
          }
          timer.end(st);
        }
        mixed_ran = true;
        stats.f32_launches += nf32;
        stats.f32_chains += 1;
        stats.f32_tail_sum += mc.j;
      } else {
      timer.begin(st, itn, true, second, m - 1);
      for (int k = m - 2; k >= 0; --k) {
        double* dst = k == 0 ? hat : ((k & 1) ? w.wb.p : w.wa.p);
        FinArgs f{nullptr, nullptr, PH_NONE, 0, 0, nullptr};
        const double lead = k == m - 2 ? tau[m - 1] : 1.0;
        f.pc0 = lead; f.pc1 = -lead * tau[k]; f.pc2 = tau[k]; f.base = in;
        spmv_with_halo(8, A, nb, slab, src, dst, nullptr, nullptr, w.sc.p, G, st, &f);
        src = dst;
      }
      timer.end(st);
      }
    } else if (mg) {
      double* hat = second ? w.yb.p : w.ya.p;
      timer.begin(st, itn, true, second, 1);              // (profiling: a V-cycle is bracketed as a whole and counted as ONE lean launch)
      mg_apply(*mgh, A, nb, slab, in, hat, w.sc.p, st);   // hat = M⁻¹ in: one V-cycle
      timer.end(st);
      src = hat;
    }
    // the scalar phase that follows is evaluated by the last block of the launch (stencil-slice kernel); with
    // several ranks the halo exchange of the input overlaps the rows that need no ghost value (spmv_with_halo).
    // Mode 3 after the chain: `in` (= s) is the operand of the (out, .) dot, not the launch's x
    FinArgs f{w.ticket.p, w.sc.p, phase, nslots, derive_here, pre ? in : nullptr};
    timer.begin(st, itn, false, second);
    const bool folded = spmv_with_halo(phase == PH_BICG_1 ? 1 : 3, A, nb, slab, src, out, w.rhat.p, w.partials.p, w.sc.p, G, st, &f);
    timer.end(st);
    if (folded) finalize_folded(phase, nslots, w, st); else finalize(phase, nslots, w, st, true);
  };
  // test: make the half-step test in this iteration.  (Not before the half step the previous solve ended at: a solve that
  // could have stopped one application earlier stops at the end of that iteration instead, which happens about never.)
  auto first_half = [&](int itn, bool test) {
    double* pvec = (p_in_rhat && itn == 0) ? w.rhat.p : w.p.p;
    apply(pvec, w.v.p, PH_BICG_1, 3, itn);     // v = C p, (r̂,v); previous iteration's (r,r): convergence / restart; then α
    unsigned* tk = (test && derive_here) ? w.ticket.p : nullptr;   // the half-step test inside the s kernel
    // s, its dots, the half-step test -- and with the polynomial x += α M⁻¹p -- in one pass; without the test in this
    // iteration the sums of slot 4 are simply not looked at
    if (pre)
      hipLaunchKernelGGL(k_bicg_s_x, dim3(G), dim3(BLOCK), 0, st, n, w.sc.p, w.v.p, w.rhat.p, w.r.p, w.partials.p, (const double*)A.ds.p, tk,
                         p_in_rhat ? 1 : 0, (const double*)w.ya.p, x, scatter, xg, itn == 0 ? 1 : 0, rc);
    else
      hipLaunchKernelGGL(k_bicg_s, dim3(G), dim3(BLOCK), 0, st, n, w.sc.p, w.v.p, w.rhat.p, w.r.p, w.partials.p, (const double*)A.ds.p, tk,
                         p_in_rhat ? 1 : 0);
    if (test && !tk) finalize(PH_BICG_S, 1, w, st, true, 4);
  };
  auto second_half = [&](int itn) {
    apply(w.r.p, w.t.p, PH_BICG_2, 5, itn);     // t = C s (r holds s), (t,s), (t,t), (r̂,t); then ω, ρ, β / restart
    hipLaunchKernelGGL(k_bicg_xrp, dim3(G), dim3(BLOCK), 0, st, n, w.sc.p, w.t.p, w.v.p, x, w.r.p, w.p.p, w.rhat.p, w.partials.p,
                       (const double*)A.ds.p, p_in_rhat ? 1 : 0, pre ? (const double*)w.yb.p : nullptr, scatter);
  };
  while (!done) {
    int want = check_every;
    if (w.last_iters > 1) want = polls == 0 ? w.last_iters - 1 : (polls <= 4 ? 1 : check_every);
    if (expect_halves > 0) want = polls == 0 ? (expect_halves + 1) / 2 : (polls <= 4 ? 1 : check_every);   // the predicted count at once
    const int batch = std::max(1, std::min(want, maxiter - launched));
    int halves = 2 * batch;
    if (half_test && expect_halves > 0 && polls == 0) halves = std::max(1, std::min(expect_halves, 2 * (maxiter - launched)));
    ++polls;
    if (!cg) {
      const bool predicted = half_test && expect_halves > 0 && polls == 1;
      for (int h = 0; h < halves; ++h) {
        if (!mid) {
          if (launched >= maxiter) break;
          first_half(launched, half_test && (!predicted || h + 2 >= halves));
          ++launched;
          mid = true;
        } else {
          second_half(launched - 1);
          mid = false;
        }
      }
    } else {
      for (int it = 0; it < batch; ++it) {
        timer.begin(st, launched + it);
        spmv_with_halo(2, A, nb, slab, w.p.p, w.v.p, nullptr, w.partials.p, w.sc.p, G, st);   // v = A p ; (v.p), (v.v)
        timer.end(st);
        finalize(PH_CG_1, 1, w, st, true);
        hipLaunchKernelGGL(k_cg_xr, dim3(G), dim3(BLOCK), 0, st, n, w.sc.p, w.p.p, w.v.p, x, w.r.p, w.partials.p, (const double*)A.ds.p);
        finalize(PH_CG_2, 2, w, st, true);
        hipLaunchKernelGGL(k_cg_p, dim3(G), dim3(BLOCK), 0, st, n, w.sc.p, w.r.p, w.p.p);
      }
      launched += batch;
    }
    if (!cg && !mid) finalize(PH_BICG_3, 2, w, st, true, 1);   // the last iteration's (r,r), not yet folded into a next one
    PG_HIP(hipGetLastError());
    PG_HIP(hipMemcpyAsync(w.h_sc, w.sc.p, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost, st));
    const auto t_wait0 = std::chrono::steady_clock::now();
    struct WaitClock {   // PG_DEBUG: where the host's time goes (pg_solver_run prints the totals)
      std::chrono::steady_clock::time_point t0;
      ~WaitClock() { g_host_wait_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
    } wait_clock{t_wait0};
    if (call.after_first_batch && polls == 1) {
      // the caller's speculative work goes behind the copy; the host waits for the COPY only
      if (!w.ev_poll) PG_HIP(hipEventCreateWithFlags(&w.ev_poll, hipEventDisableTiming));
      PG_HIP(hipEventRecord(w.ev_poll, st));
      call.after_first_batch();
      PG_HIP(hipEventSynchronize(w.ev_poll));
    } else {
      PG_HIP(hipStreamSynchronize(st));   // (spinning on hipStreamQuery instead: no measurable difference)
    }
    if (w.h_sc[S_DONE] != 0.0 || (launched >= maxiter && !mid)) done = true;
    // safety net of the polynomial preconditioner: its roots assume a (nearly) real spectrum inside the Gershgorin
    // interval; a matrix that defeats that assumption shows as stagnation, and the solve falls back to the plain iteration
    // from the iterate reached (the matrix keeps the verdict)
    if (!done && poly && launched >= poly_give_up) { poly_failed = true; done = true; }
  }
  if (poly_failed) {                        // x is the iterate reached
    poly_record_stagnation(A);
    timer.collect(stats, launched, false);
    if (scatter) {                          // (the caller solves again on its full system, which has a right-hand side vector)
      stats.iters = launched;
      stats.converged = 0;
      stats.poly_degree = -1;
      return;
    }
    if (cfg.debug) fprintf(stderr, "[pg_krylov] polynomial preconditioner (m = %d) stagnated after %d iterations: plain iteration\n", m, launched);
    spmv_with_halo(0, A, nb, slab, x, w.t.p, nullptr, nullptr, nullptr, G, st);   // Â x of the iterate reached
    SolveStats rest;
    KrylovCall finish;      // (a fresh call: nothing of the prepared start carries over)
    finish.x0 = x; finish.Ax0 = w.t.p;
    krylov_solve(A, nb, slab, b, x, w, opts, rest, finish);
    stats = rest;
    stats.iters += launched;
    return;
  }
  if (cfg.debug)
    fprintf(stderr, "[pg_krylov] done=%g iters=%g rr0=%g rr=%g tol2=%g rho=%g rho_old=%g alpha=%g omega=%g beta=%g red0=%g red1=%g\n",
            w.h_sc[S_DONE], w.h_sc[S_ITERS], w.h_sc[S_RR0], w.h_sc[S_RR], w.h_sc[S_TOL2], w.h_sc[S_RHO], w.h_sc[S_RHO_OLD], w.h_sc[S_ALPHA],
            w.h_sc[S_OMEGA], w.h_sc[S_BETA], w.h_sc[S_RED0], w.h_sc[S_RED1]);
  stats.iters = (int)w.h_sc[S_ITERS];
  stats.polls = polls;
  w.last_iters = stats.iters;
  stats.converged = w.h_sc[S_DONE] == 1.0 ? 1 : 0;
  stats.half_exit = w.h_sc[S_HALF] != 0.0 ? 1 : 0;
  // the weighted norms of the convergence test (S_HELD: the rows a folded start left where they were, pg_solver.hip)
  stats.resnorm = std::sqrt((cg ? w.h_sc[S_RRW] : w.h_sc[S_RR]) + w.h_sc[S_HELD]);
  stats.bnorm = std::sqrt(w.h_sc[S_BB]);
  timer.collect(stats, stats.iters, w.h_sc[S_HALF] != 0.0);
  stats.products = (i64)(2 * stats.iters - stats.half_exit) * (m >= 2 ? m : 1);
  if (!cg && stats.converged && stats.products > 0) {   // (what a product took off log (r,r)_W: the extrapolated start's cost model)
    const double rr0 = w.h_sc[S_RR0], rr = w.h_sc[S_HALF] != 0.0 ? w.h_sc[S_RED4] : w.h_sc[S_RR];
    if (rr0 > 0.0 && rr > 0.0 && rr < rr0) w.last_rate2 = std::log(rr0 / rr) / (double)stats.products;
  }
  // what the next solve's mixed chain goes by (scalars of this solve: identical on every rank, the same from run to run)
  const bool mix_env = poly && cfg.poly_f32 && cx.nranks == 1 && !cx.comm && !A.halo_needed && spmv_supports_typed_chain();
  choose_next_degree(A, stats, m, adaptive, w,
                     mix_env && cfg.poly_f32_tail < 0 ? std::min(std::max(by_estimate ? A.est.g_used : A.gersh, 0.05), 0.95) : 0.0);
  if (stats.iters == 0) stats.f32_launches = stats.f32_chains = stats.f32_tail_sum = 0;   // (the chain returned at the done flag)
  if (mixed_ran && expect_halves == 1 && !(stats.iters == 1 && stats.half_exit)) w.mix_wait = 2 * (m + 3);
  w.mix_matrix = nullptr;
  if (mix_env && stats.converged) {
    const double rr0 = w.h_sc[S_RR0], tol2 = w.h_sc[S_TOL2];
    if (rr0 > 0.0 && rr0 < 1e300 && tol2 > 0.0) {
      int e = 0;
      (void)std::frexp(std::sqrt(rr0 / (double)n), &e);   // σ: the power of two that brings the start residual's rms near 1
      const int h = (adaptive && w.adapt_matrix == &A && w.adapt_h >= 1) ? w.adapt_h : std::max(1, 2 * stats.iters - stats.half_exit);
      if (e > -100 && e < 100) {
        w.mix_matrix = &A;
        w.mix_sigma = std::ldexp(1.0, -e);
        w.mix_need = std::pow(std::sqrt(std::min(1.0, tol2 / rr0)), 1.0 / h);
      }
    }
  }
}

}  // namespace pg
