// pg_idrs.hip -- IDR(s) on the device (IDR(s) with biorthogonalisation: van Gijzen & Sonneveld, ACM TOMS 38 (2011), Alg. 1):
// `method = IterativeSolvers.idrs` with the keyword s, s = 1 .. 8.  PG_METHOD_IDRS; s travels in pg_krylov_opts.restart (<= 0: 8,
// IterativeSolvers' default).
//
// The residuals are built in nested Sonneveld spaces with s shadow vectors: with s = 4 .. 8 the method behaves close to GMRES per
// product on strongly nonsymmetric spectra (ConvectionOps systems) at a fixed, short recurrence.  tests/idrs_reference.py restates
// the iteration in numpy, operation for operation; DESIGN.md "IDR(s)" has the byte count and what was measured.  One cycle is
// s + 1 products (G[0..s), U[0..s), r, t are the work vectors; M (s x s, lower triangular), f, c, α, β, ω the device scalars):
//
//   per k = 0 .. s-1
//   scalars A     (the stopping test of the update before);  c = solution of  M[k:, k:] c = f[k:]
//   k_idr_dir     U[k] = ω (r - Σ_{i>=k} c_i G[i]) + Σ_{i>=k} c_i U[i]     one pass; the first cycle after a (re)start: U[k] = ω r
//   SpMV mode 0   G[k] = Â U[k]
//   k_idr_pg      h_i = (p_i, G[k]), i = 0 .. s-1, and (G[k], G[k]): one pass over G[k], the shadow vectors made in registers
//   scalars B     α = solution of  M[:k, :k] α = h[:k];  M[i, k] = h_i - Σ_{j<k} M[i, j] α_j (i >= k);  β = f_k / M[k, k];
//                 f_i -= β M[i, k] (i > k) -- the biorthogonalisation from scalars: (p_i, G[j]) = M[i, j] is known, no second pass
//   k_idr_upd     G[k] -= Σ_{i<k} α_i G[i],  U[k] -= Σ_{i<k} α_i U[i],  r -= β G[k],  x += β U[k],  (r, r)_W of the new r
//   per cycle
//   scalars D     (the stopping test of the update before)
//   SpMV mode 0   t = Â r
//   k_idr_tdots   (t, r), (t, t), (r, r)
//   scalars E     ω = (t, r) / (t, t), enlarged by κ / ρ when ρ = |(t, r)| / (|t| |r|) < κ = 0.7
//   k_idr_omega   x += ω r,  r -= ω t,  (r, r)_W  and the next cycle's f = Pᵀ r in the same pass
//
// The shadow vectors are never stored: p_k[i] = pghost::idr_shadow(i, k), a pure integer function of the row number, exact in
// fp64 and bit-identical in numpy.  P is not orthogonalised (as in IterativeSolvers).
//
// It iterates on the same Â = B⁻¹SAS as the other methods and stops on the same quantity as BiCGStab: (r,r)_W <= max(reltol²
// (b,b)_W, abstol²), W = S².  It starts from zero or from the caller's x0 with Â x0 given (krylov_solve's contract; x0 may be x):
// one argument of the start kernel, not a second code path.  All scalars stay on the device, the small triangular solves
// included (pg_host_algos.h idr_lower_solve, one thread); every reduction is per-block partial sums and a second stage in a
// fixed order (no atomics): a solve is bitwise reproducible.  Every kernel returns at once when S_DONE is set; the host polls the
// flag every check_every cycles.
//
// Robustness.  M[k,k] not finite or negligible against |p_k| |G[k]| (the rounding of its own dot product), a c that is not
// finite, (t,t) = 0, (t,r) = 0 or a residual that is not finite: S_DONE = 6, the host forms the TRUE residual b̂ - Âx (one
// product) and the iteration restarts from it -- M = I, ω = 1, G and U forgotten -- at most MAX_RESTARTS times.  When the
// recurrence residual meets the test (S_DONE = 4) the true residual is formed the same way and decides: met -> converged, with
// the true norm reported; not met -> the iteration continues from it as after a restart, at most three times, then the solve
// is reported unconverged (S_DONE = 5).  A true residual that is not finite ends the solve unconverged with x = 0 (S_DONE = 2):
// never NaN.
//
// Counting: iters = updates of x, one product each -- the unit maxiter caps, exactly: no update starts at iters >= maxiter
// (S_DONE = 7; maxiter <= 0: 200 000).  products = iters + restarts + confirmations, plus 1 when started from an x0 (the
// caller's product Â x0).
#include <cstdint>

#include "pg_krylov.h"
#include "pg_spmv.h"
#include "pg_host_algos.h"

using namespace pg;

namespace {

constexpr int MAXS = pghost::IDR_MAX_S;
constexpr int MAX_CONTINUES = 3;
constexpr int MAX_RESTARTS = 16;
constexpr int NSLOTS = 2 * MAXS + 2;   // the start kernel's sums: (r,r)_W, (b,b)_W, f[0..s), (p_k,p_k)[0..s)

// device scalars of the method (KrylovWork::id); the stopping scalars live in KrylovWork::sc
enum { I_OMEGA = 0, I_BETA, I_CONT /* continuations from a true residual */, I_RESTARTS, I_F, I_C = I_F + MAXS, I_ALPHA = I_C + MAXS,
       I_PP = I_ALPHA + MAXS /* (p_k, p_k) */, I_M = I_PP + MAXS /* MAXS x MAXS, row major */, I_COUNT = I_M + MAXS * MAXS };
enum { P_START = 0, P_TRUE, P_A, P_B, P_D, P_E };
enum { AFTER_NOTHING = 0, AFTER_UPD = 1, AFTER_OMEGA = 2 };   // which update's sums a scalar phase finds in the partial slots
// S_DONE: 0 running, 1 converged (true residual), 2 not finite, 4 the recurrence residual met the test: the host queues the
// confirmation, 5 given up (the true residual failed after MAX_CONTINUES continuations, or MAX_RESTARTS restarts), 6 breakdown:
// the host queues the restart from the true residual, 7 maxiter

__device__ inline bool fin(double v) { return pghost::bl_finite(v); }

// 16-byte accesses: a thread works on the rows 2p, 2p + 1.  Every vector starts 16-byte aligned (checked by idrs_solve; the work
// vectors are an even stride apart); the last row of an odd n is read and written alone, its partner counts as zero.
__device__ inline double2 ld2(const double* p, i64 i, bool both) {
  if (both) return *reinterpret_cast<const double2*>(p + i);
  double2 v;
  v.x = p[i];
  v.y = 0.0;
  return v;
}
__device__ inline void st2(double* p, i64 i, double2 v, bool both) {
  if (both) *reinterpret_cast<double2*>(p + i) = v;
  else p[i] = v.x;
}
#define PG_IDR_PAIRS(n)                                                                                                  \
  for (i64 i = 2 * (blockIdx.x * (i64)BLOCK + threadIdx.x); i < (n); i += 2 * (i64)gridDim.x * BLOCK)

__global__ void k_idr_reset(double* __restrict__ sc, double* __restrict__ id, double reltol2, double abstol2) {
  for (int i = threadIdx.x; i < S_COUNT; i += blockDim.x) sc[i] = i == S_RELTOL2 ? reltol2 : (i == S_ABSTOL2 ? abstol2 : 0.0);
  for (int i = threadIdx.x; i < I_COUNT; i += blockDim.x) id[i] = 0.0;
}

// the start and the true residual: r = b - Ax (Ax == nullptr: r = b);  partial slots 0 / 1 = (r,r)_W, (b,b)_W,  2 .. 2+S = f = Pᵀ r,
// 2+S .. 2+2S = (p_k, p_k)
template <int S>
__global__ __launch_bounds__(BLOCK) void k_idr_resid(i64 n, const double* __restrict__ b, const double* __restrict__ Ax,
                                                     double* __restrict__ r, const double* __restrict__ ds,
                                                     double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  double accw = 0.0, accb = 0.0, f[S], pp[S];
#pragma unroll
  for (int k = 0; k < S; ++k) f[k] = pp[k] = 0.0;
  PG_IDR_PAIRS(n) {
    const bool both = i + 1 < n;
    const double2 bi = ld2(b, i, both), di = ld2(ds, i, both);
    double2 ri = bi;
    if (Ax) {
      const double2 a = ld2(Ax, i, both);
      ri.x = bi.x - a.x; ri.y = bi.y - a.y;
    }
    st2(r, i, ri, both);
    accw += (di.x * ri.x) * (di.x * ri.x) + (di.y * ri.y) * (di.y * ri.y);
    accb += (di.x * bi.x) * (di.x * bi.x) + (di.y * bi.y) * (di.y * bi.y);
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const double p0 = pghost::idr_shadow((uint64_t)i, k), p1 = both ? pghost::idr_shadow((uint64_t)i + 1, k) : 0.0;
      f[k] += p0 * ri.x + p1 * ri.y;
      pp[k] += p0 * p0 + p1 * p1;
    }
  }
  const size_t G = gridDim.x;
  double t = block_sum(accw, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
  t = block_sum(accb, s_red);
  if (threadIdx.x == 0) partials[G + blockIdx.x] = t;
#pragma unroll
  for (int k = 0; k < S; ++k) {
    t = block_sum(f[k], s_red);
    if (threadIdx.x == 0) partials[(2 + k) * G + blockIdx.x] = t;
    t = block_sum(pp[k], s_red);
    if (threadIdx.x == 0) partials[(2 + S + k) * G + blockIdx.x] = t;
  }
}

// U[k] = ω (r - Σ c_{k+q} G[k+q]) + Σ c_{k+q} U[k+q], q = 0 .. NL-1  (Gk, Uk: G[k], U[k]; ck: c + k).  NL = 0: the first cycle after
// a (re)start, where G and U count as zero whatever they hold: U[k] = ω r
template <int NL>
__global__ __launch_bounds__(BLOCK) void k_idr_dir(i64 n, i64 stride, const double* __restrict__ Gk, double* __restrict__ Uk,
                                                   const double* __restrict__ r, const double* __restrict__ id, int k,
                                                   const double* __restrict__ sc) {
  if (sc[S_DONE] != 0.0) return;
  const double omega = id[I_OMEGA];
  double c[NL > 0 ? NL : 1];
#pragma unroll
  for (int q = 0; q < NL; ++q) c[q] = id[I_C + k + q];
  PG_IDR_PAIRS(n) {
    const bool both = i + 1 < n;
    double2 v = ld2(r, i, both);
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const double2 g = ld2(Gk + (size_t)q * stride, i, both);
      v.x -= c[q] * g.x; v.y -= c[q] * g.y;
    }
    double2 u;
    u.x = omega * v.x; u.y = omega * v.y;
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const double2 w = ld2(Uk + (size_t)q * stride, i, both);
      u.x += c[q] * w.x; u.y += c[q] * w.y;
    }
    st2(Uk, i, u, both);
  }
}

// h_i = (p_i, G[k]), i = 0 .. S-1, in partial slots 0 .. S-1 and (G[k], G[k]) in slot S: one pass over G[k]
template <int S>
__global__ __launch_bounds__(BLOCK) void k_idr_pg(i64 n, const double* __restrict__ Gk, const double* __restrict__ sc,
                                                  double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  if (sc[S_DONE] != 0.0) return;
  double h[S], gg = 0.0;
#pragma unroll
  for (int q = 0; q < S; ++q) h[q] = 0.0;
  PG_IDR_PAIRS(n) {
    const bool both = i + 1 < n;
    const double2 g = ld2(Gk, i, both);
    gg += g.x * g.x + g.y * g.y;
#pragma unroll
    for (int q = 0; q < S; ++q)   // (g.y = 0 beyond n: the shadow value there is finite and drops out)
      h[q] += pghost::idr_shadow((uint64_t)i, q) * g.x + pghost::idr_shadow((uint64_t)i + 1, q) * g.y;
  }
  const size_t G = gridDim.x;
#pragma unroll
  for (int q = 0; q < S; ++q) {
    const double t = block_sum(h[q], s_red);
    if (threadIdx.x == 0) partials[q * G + blockIdx.x] = t;
  }
  const double t = block_sum(gg, s_red);
  if (threadIdx.x == 0) partials[S * G + blockIdx.x] = t;
}

// G[k] -= Σ_{q<K} α_q G[q],  U[k] -= Σ_{q<K} α_q U[q],  r -= β G[k],  x += β U[k];  partial slot 0 = (r,r)_W of the new r.  K = k.
template <int K>
__global__ __launch_bounds__(BLOCK) void k_idr_upd(i64 n, i64 stride, double* __restrict__ G, double* __restrict__ U,
                                                   double* __restrict__ r, double* __restrict__ x, const double* __restrict__ ds,
                                                   const double* __restrict__ id, const double* __restrict__ sc,
                                                   double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  if (sc[S_DONE] != 0.0) return;
  const double beta = id[I_BETA];
  double a[K > 0 ? K : 1];
#pragma unroll
  for (int q = 0; q < K; ++q) a[q] = id[I_ALPHA + q];
  double* Gk = G + (size_t)K * stride;
  double* Uk = U + (size_t)K * stride;
  double accw = 0.0;
  PG_IDR_PAIRS(n) {
    const bool both = i + 1 < n;
    double2 g = ld2(Gk, i, both), u = ld2(Uk, i, both);
#pragma unroll
    for (int q = 0; q < K; ++q) {
      const double2 gq = ld2(G + (size_t)q * stride, i, both), uq = ld2(U + (size_t)q * stride, i, both);
      g.x -= a[q] * gq.x; g.y -= a[q] * gq.y;
      u.x -= a[q] * uq.x; u.y -= a[q] * uq.y;
    }
    if (K > 0) { st2(Gk, i, g, both); st2(Uk, i, u, both); }
    double2 ri = ld2(r, i, both), xi = ld2(x, i, both);
    const double2 di = ld2(ds, i, both);
    ri.x -= beta * g.x; ri.y -= beta * g.y;
    xi.x += beta * u.x; xi.y += beta * u.y;
    st2(r, i, ri, both);
    st2(x, i, xi, both);
    accw += (di.x * ri.x) * (di.x * ri.x) + (di.y * ri.y) * (di.y * ri.y);
  }
  const double t = block_sum(accw, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// partial slots 0 / 1 / 2 = (t, r), (t, t), (r, r)
__global__ __launch_bounds__(BLOCK) void k_idr_tdots(i64 n, const double* __restrict__ t, const double* __restrict__ r,
                                                     const double* __restrict__ sc, double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  if (sc[S_DONE] != 0.0) return;
  double tr = 0.0, tt = 0.0, rr = 0.0;
  PG_IDR_PAIRS(n) {
    const bool both = i + 1 < n;
    const double2 ti = ld2(t, i, both), ri = ld2(r, i, both);
    tr += ti.x * ri.x + ti.y * ri.y;
    tt += ti.x * ti.x + ti.y * ti.y;
    rr += ri.x * ri.x + ri.y * ri.y;
  }
  const size_t G = gridDim.x;
  double v = block_sum(tr, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = v;
  v = block_sum(tt, s_red);
  if (threadIdx.x == 0) partials[G + blockIdx.x] = v;
  v = block_sum(rr, s_red);
  if (threadIdx.x == 0) partials[2 * G + blockIdx.x] = v;
}

// x += ω r,  r -= ω t;  partial slot 0 = (r,r)_W of the new r, slots 1 .. S = the next cycle's f = Pᵀ r
template <int S>
__global__ __launch_bounds__(BLOCK) void k_idr_omega(i64 n, const double* __restrict__ t, double* __restrict__ r,
                                                     double* __restrict__ x, const double* __restrict__ ds,
                                                     const double* __restrict__ id, const double* __restrict__ sc,
                                                     double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  if (sc[S_DONE] != 0.0) return;
  const double omega = id[I_OMEGA];
  double accw = 0.0, f[S];
#pragma unroll
  for (int q = 0; q < S; ++q) f[q] = 0.0;
  PG_IDR_PAIRS(n) {
    const bool both = i + 1 < n;
    const double2 ti = ld2(t, i, both), di = ld2(ds, i, both);
    double2 ri = ld2(r, i, both), xi = ld2(x, i, both);
    xi.x += omega * ri.x; xi.y += omega * ri.y;
    ri.x -= omega * ti.x; ri.y -= omega * ti.y;
    st2(x, i, xi, both);
    st2(r, i, ri, both);
    accw += (di.x * ri.x) * (di.x * ri.x) + (di.y * ri.y) * (di.y * ri.y);
#pragma unroll
    for (int q = 0; q < S; ++q)
      f[q] += pghost::idr_shadow((uint64_t)i, q) * ri.x + pghost::idr_shadow((uint64_t)i + 1, q) * ri.y;
  }
  const size_t G = gridDim.x;
  double v = block_sum(accw, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = v;
#pragma unroll
  for (int q = 0; q < S; ++q) {
    v = block_sum(f[q], s_red);
    if (threadIdx.x == 0) partials[(1 + q) * G + blockIdx.x] = v;
  }
}

// the iteration forgets G, U and M: what a start, a restart and a continuation share
__device__ inline void idr_fresh(int s, const double* sums_f, double* id) {
  for (int i = 0; i < MAXS; ++i)
    for (int j = 0; j < MAXS; ++j) id[I_M + i * MAXS + j] = i == j ? 1.0 : 0.0;
  for (int i = 0; i < MAXS; ++i) id[I_F + i] = i < s ? sums_f[i] : 0.0;
  id[I_OMEGA] = 1.0;
}

// an update of x has run and left (r,r)_W: count it and test.  True: the iteration goes on.
__device__ inline bool idr_after_update(double rrw, double* sc) {
  sc[S_ITERS] += 1.0;
  sc[S_RR] = rrw;
  if (!fin(rrw)) sc[S_DONE] = 6.0;
  else if (rrw <= sc[S_TOL2]) sc[S_DONE] = 4.0;
  return sc[S_DONE] == 0.0;
}

// the scalar phases: sums of the partial slots the phase reads (fixed order), then one thread derives
__global__ __launch_bounds__(BLOCK) void k_idr_scalar(int phase, int k, int after, int s, int grid, int maxiter,
                                                      const double* __restrict__ partials, double* __restrict__ sc,
                                                      double* __restrict__ id) {
  __shared__ double s_red[BLOCK / 64];
  __shared__ double s_sum[NSLOTS];
  if (phase != P_START && phase != P_TRUE && sc[S_DONE] != 0.0) return;
  int nslots = 0;
  switch (phase) {
    case P_START: case P_TRUE: nslots = 2 + 2 * s; break;
    case P_A: case P_D: nslots = after == AFTER_UPD ? 1 : (after == AFTER_OMEGA ? 1 + s : 0); break;
    case P_B: nslots = s + 1; break;
    case P_E: nslots = 3; break;
  }
  for (int q = 0; q < nslots; ++q) {
    double a = 0.0;
    for (int i = threadIdx.x; i < grid; i += BLOCK) a += partials[(size_t)q * grid + i];
    const double t = block_sum(a, s_red);
    if (threadIdx.x == 0) s_sum[q] = t;
  }
  if (threadIdx.x != 0) return;
  double* M = id + I_M;
  double* f = id + I_F;
  switch (phase) {
    case P_START: {
      const double rrw = s_sum[0], bbw = s_sum[1];
      sc[S_BB] = bbw; sc[S_RR] = rrw; sc[S_RR0] = rrw; sc[S_ITERS] = 0.0;
      const double t2 = sc[S_RELTOL2] * bbw;
      sc[S_TOL2] = t2 > sc[S_ABSTOL2] ? t2 : sc[S_ABSTOL2];
      idr_fresh(s, s_sum + 2, id);
      for (int i = 0; i < s; ++i) id[I_PP + i] = s_sum[2 + s + i];
      // (the start residual is a true residual: nothing to confirm.  b = 0 from zero: x = 0 is exact)
      sc[S_DONE] = (!fin(rrw) || !fin(bbw)) ? 2.0 : (rrw <= sc[S_TOL2] ? 1.0 : 0.0);
      break;
    }
    case P_TRUE: {
      // the TRUE residual of the state the recurrence accepted (S_DONE = 4) or broke down at (6)
      const double rrw = s_sum[0];
      const bool confirm = sc[S_DONE] == 4.0;
      if (confirm) sc[S_RED0] = sc[S_RR];   // (diagnostics: the recurrence value that asked)
      sc[S_RR] = rrw;
      if (!fin(rrw)) sc[S_DONE] = 2.0;
      else if (rrw <= sc[S_TOL2]) sc[S_DONE] = 1.0;
      else if (confirm ? id[I_CONT] >= (double)MAX_CONTINUES : id[I_RESTARTS] >= (double)MAX_RESTARTS) sc[S_DONE] = 5.0;
      else {
        id[confirm ? I_CONT : I_RESTARTS] += 1.0;
        idr_fresh(s, s_sum + 2, id);
        sc[S_DONE] = 0.0;
      }
      break;
    }
    case P_A: case P_D: {
      if (after == AFTER_UPD && !idr_after_update(s_sum[0], sc)) break;
      if (after == AFTER_OMEGA) {
        for (int i = 0; i < s; ++i) f[i] = s_sum[1 + i];
        if (!idr_after_update(s_sum[0], sc)) break;
      }
      if ((int)sc[S_ITERS] >= maxiter) { sc[S_DONE] = 7.0; break; }
      if (phase == P_A && !pghost::idr_lower_solve(M, s, k, s, f, id + I_C)) sc[S_DONE] = 6.0;
      break;
    }
    case P_B: {
      const double* h = s_sum;
      const double gg = s_sum[s];
      double* alpha = id + I_ALPHA;
      const bool ok = pghost::idr_lower_solve(M, s, 0, k, h, alpha);
      for (int i = k; i < s; ++i) {
        double v = h[i];
        for (int j = 0; j < k; ++j) v -= M[i * MAXS + j] * alpha[j];
        M[i * MAXS + k] = v;
      }
      const double mkk = M[k * MAXS + k];
      const double scale = sqrt(id[I_PP + k] * gg);
      if (!ok || !fin(mkk) || !fin(gg) || !(fabs(mkk) > pghost::IDR_PIV_TOL * scale)) { sc[S_DONE] = 6.0; break; }
      const double beta = f[k] / mkk;
      if (!fin(beta)) { sc[S_DONE] = 6.0; break; }
      for (int i = k + 1; i < s; ++i) f[i] -= beta * M[i * MAXS + k];
      f[k] = 0.0;
      id[I_BETA] = beta;
      break;
    }
    case P_E: {
      const double tr = s_sum[0], tt = s_sum[1], rr = s_sum[2];
      if (tt == 0.0 || tr == 0.0 || !fin(tt) || !fin(tr) || !fin(rr)) { sc[S_DONE] = 6.0; break; }
      const double rho = fabs(tr) / sqrt(tt * rr);
      if (!(rho > 0.0)) { sc[S_DONE] = 6.0; break; }   // (t,r) negligible against |t| |r|, or |t|² |r|² beyond the range
      double omega = tr / tt;
      if (rho < pghost::IDR_KAPPA) omega *= pghost::IDR_KAPPA / rho;
      if (!fin(omega) || omega == 0.0) { sc[S_DONE] = 6.0; break; }
      id[I_OMEGA] = omega;
      break;
    }
  }
}

struct IdrArgs {
  int G;
  hipStream_t st;
  i64 n, stride;
  double *Gv, *Uv, *r, *t, *x, *id, *sc, *part;
  const double* ds;
};

template <int S>
void launch_resid(const IdrArgs& a, const double* b, const double* Ax) {
  hipLaunchKernelGGL(k_idr_resid<S>, dim3(a.G), dim3(BLOCK), 0, a.st, a.n, b, Ax, a.r, a.ds, a.part);
}
template <int S>
void launch_pg(const IdrArgs& a, int k) {
  hipLaunchKernelGGL(k_idr_pg<S>, dim3(a.G), dim3(BLOCK), 0, a.st, a.n, (const double*)(a.Gv + (size_t)k * a.stride), (const double*)a.sc,
                     a.part);
}
template <int S>
void launch_omega(const IdrArgs& a) {
  hipLaunchKernelGGL(k_idr_omega<S>, dim3(a.G), dim3(BLOCK), 0, a.st, a.n, (const double*)a.t, a.r, a.x, a.ds, (const double*)a.id,
                     (const double*)a.sc, a.part);
}
template <int NL>
void launch_dir(const IdrArgs& a, int k) {
  hipLaunchKernelGGL(k_idr_dir<NL>, dim3(a.G), dim3(BLOCK), 0, a.st, a.n, a.stride, (const double*)(a.Gv + (size_t)k * a.stride),
                     a.Uv + (size_t)k * a.stride, (const double*)a.r, (const double*)a.id, k, (const double*)a.sc);
}
template <int K>
void launch_upd(const IdrArgs& a) {
  hipLaunchKernelGGL(k_idr_upd<K>, dim3(a.G), dim3(BLOCK), 0, a.st, a.n, a.stride, a.Gv, a.Uv, a.r, a.x, a.ds, (const double*)a.id,
                     (const double*)a.sc, a.part);
}

// the template argument from a run-time count 1 .. 8 (F<1> .. F<8>) or 0 .. 8
#define PG_IDR_SWITCH8(v, CALL)                                                                                          \
  switch (v) {                                                                                                           \
    case 1: CALL(1); break;                                                                                              \
    case 2: CALL(2); break;                                                                                              \
    case 3: CALL(3); break;                                                                                              \
    case 4: CALL(4); break;                                                                                              \
    case 5: CALL(5); break;                                                                                              \
    case 6: CALL(6); break;                                                                                              \
    case 7: CALL(7); break;                                                                                              \
    default: CALL(8); break;                                                                                             \
  }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

namespace pg {

void idrs_solve(const CsrMatrix& A, const Numbering& nb, const Slab& slab, const double* b, double* x, KrylovWork& w,
                const pg_krylov_opts& opts, SolveStats& stats, const double* x0, const double* Ax0) {
  Context& cx = ctx();
  hipStream_t st = cx.stream;
  const i64 n = A.n, nvec = nb.n_vec();
  PG_REQUIRE(w.n >= n && w.nvec >= nvec, "krylov workspace too small");
  const int s = opts.restart > 0 ? opts.restart : 8;
  PG_REQUIRE(s <= MAXS, "IDR(s) refused: s = " + std::to_string(s) + " is more than 8 (pg_krylov_opts.restart carries s)");
  PG_REQUIRE(cx.nranks == 1 && !cx.comm, "IDR(s) refused: the solve runs on several ranks (one rank only)");
  PG_REQUIRE(!x0 || Ax0, "IDR(s): a start from x0 needs the product with x0");
  const int G = w.grid;
  const int maxiter = opts.maxiter > 0 ? opts.maxiter : 200000;
  const int check_every = opts.check_every > 0 ? opts.check_every : 4;
  const i64 stride = ((nvec > 0 ? nvec : 1) + 1) & ~(i64)1;       // even: every work vector starts 16-byte aligned
  if (w.id_s != s || w.id_stride != stride) {
    w.id_vecs.alloc((2 * (i64)s + 2) * stride);
    w.id_vecs.zero();                                             // ghost segments start defined and stay zero
    w.id.alloc(I_COUNT);
    w.id_partials.alloc((i64)NSLOTS * G);
    w.id_s = s;
    w.id_stride = stride;
  }
  IdrArgs a;
  a.G = G; a.st = st; a.n = n; a.stride = stride;
  a.Gv = w.id_vecs.p;
  a.Uv = a.Gv + (size_t)s * stride;
  a.r = a.Uv + (size_t)s * stride;
  a.t = a.r + stride;
  a.x = x; a.id = w.id.p; a.sc = w.sc.p; a.part = w.id_partials.p; a.ds = A.ds.p;
  PG_REQUIRE(aligned16(b) && aligned16(x) && aligned16(a.ds) && aligned16(a.Gv) && (!Ax0 || aligned16(Ax0)),
             "IDR(s): a vector is not 16-byte aligned");

  auto scalar = [&](int phase, int k, int after) {
    hipLaunchKernelGGL(k_idr_scalar, dim3(1), dim3(BLOCK), 0, st, phase, k, after, s, G, maxiter, (const double*)a.part, a.sc, a.id);
  };
  auto resid = [&](const double* Ax) {
#define PG_CALL(V) launch_resid<V>(a, b, Ax)
    PG_IDR_SWITCH8(s, PG_CALL)
#undef PG_CALL
  };
  // one cycle: s + 1 products.  fresh: the first cycle after a (re)start -- G and U count as zero
  auto cycle = [&](bool fresh, bool first) {
    for (int k = 0; k < s; ++k) {
      scalar(P_A, k, k > 0 ? AFTER_UPD : (first ? AFTER_NOTHING : AFTER_OMEGA));
      if (fresh) launch_dir<0>(a, k);
      else {
#define PG_CALL(V) launch_dir<V>(a, k)
        PG_IDR_SWITCH8(s - k, PG_CALL)
#undef PG_CALL
      }
      double* Uk = a.Uv + (size_t)k * stride;
      spmv_with_halo(0, A, nb, slab, Uk, a.Gv + (size_t)k * stride, nullptr, nullptr, a.sc, G, st);
#define PG_CALL(V) launch_pg<V>(a, k)
      PG_IDR_SWITCH8(s, PG_CALL)
#undef PG_CALL
      scalar(P_B, k, AFTER_NOTHING);
      if (k == 0) launch_upd<0>(a);
      else {
#define PG_CALL(V) launch_upd<V>(a)
        PG_IDR_SWITCH8(k, PG_CALL)
#undef PG_CALL
      }
    }
    scalar(P_D, 0, AFTER_UPD);
    spmv_with_halo(0, A, nb, slab, a.r, a.t, nullptr, nullptr, a.sc, G, st);
    hipLaunchKernelGGL(k_idr_tdots, dim3(G), dim3(BLOCK), 0, st, n, (const double*)a.t, (const double*)a.r, (const double*)a.sc,
                       a.part);
    scalar(P_E, 0, AFTER_NOTHING);
#define PG_CALL(V) launch_omega<V>(a)
    PG_IDR_SWITCH8(s, PG_CALL)
#undef PG_CALL
  };
  auto poll = [&]() {
    PG_HIP(hipGetLastError());
    PG_HIP(hipMemcpyAsync(w.h_sc, w.sc.p, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));
  };

  hipLaunchKernelGGL(k_idr_reset, dim3(1), dim3(BLOCK), 0, st, a.sc, a.id, opts.reltol * opts.reltol, opts.abstol * opts.abstol);
  if (!x0) PG_HIP(hipMemsetAsync(x, 0, sizeof(double) * (size_t)nvec, st));
  else if (x0 != x) PG_HIP(hipMemcpyAsync(x, x0, sizeof(double) * (size_t)nvec, hipMemcpyDeviceToDevice, st));
  resid(Ax0);
  scalar(P_START, 0, AFTER_NOTHING);
  int polls = 0, confirmations = 0, restarts = 0;
  bool fresh = true, first = true;
  while (true) {
    for (int it = 0; it < check_every; ++it) {
      cycle(fresh, first);
      fresh = first = false;
    }
    // (the last ω step's sums are looked at by the next cycle's first scalar phase: close the batch with one)
    scalar(P_D, 0, AFTER_OMEGA);
    first = true;   // the next batch's first phase finds those sums consumed
    ++polls;
    poll();
    if (w.h_sc[S_DONE] == 4.0 || w.h_sc[S_DONE] == 6.0) {
      // the recurrence residual met the test, or the recurrence broke down: the true residual of x decides, and the iteration
      // continues from it (k_idr_scalar P_TRUE)
      (w.h_sc[S_DONE] == 4.0 ? confirmations : restarts) += 1;
      spmv_with_halo(0, A, nb, slab, x, w.t.p, nullptr, nullptr, nullptr, G, st);
      resid(w.t.p);
      scalar(P_TRUE, 0, AFTER_NOTHING);
      poll();
      fresh = true;
    }
    if (w.h_sc[S_DONE] != 0.0) break;
  }
  const double flag = w.h_sc[S_DONE];
  stats.iters = (int)w.h_sc[S_ITERS];
  stats.polls = polls;
  stats.converged = flag == 1.0 ? 1 : 0;
  stats.resnorm = std::sqrt(w.h_sc[S_RR]);
  stats.bnorm = std::sqrt(w.h_sc[S_BB]);
  stats.products = (i64)stats.iters + restarts + confirmations + (x0 ? 1 : 0);   // (+ the caller's product with x0)
  if (flag == 2.0) {
    // a state that is not finite is not handed back
    PG_HIP(hipMemsetAsync(x, 0, sizeof(double) * (size_t)nvec, st));
    stats.resnorm = stats.bnorm;
  }
  if (config().debug)
    fprintf(stderr, "[pg_idrs] s=%d done=%g iters=%d confirmations=%d restarts=%d rr=%g tol2=%g\n", s, flag, stats.iters,
            confirmations, restarts, w.h_sc[S_RR], w.h_sc[S_TOL2]);
}

}  // namespace pg
