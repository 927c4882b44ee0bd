// pg_bicgstabl.hip -- BiCGStab(l) on the device (Sleijpen & Fokkema 1993): `method = IterativeSolvers.bicgstabl` with the
// keyword l, l = 1 .. 8.  PG_METHOD_BICGSTABL; l travels in pg_krylov_opts.restart (<= 0: 2).
//
// One outer iteration is l BiCG sub-steps (two products each) and one minimal-residual step over the power basis
// R[0..l] = r, Âr, .., Â^l r of the residual -- a residual polynomial of degree l per 2l products where BiCGStab multiplies l
// polynomials of degree 1: the difference shows on spectra with large imaginary parts (ConvectionOps systems), where the
// degree-1 steps have ω ≈ 0.  tests/bicgstabl_reference.py restates the iteration in numpy; DESIGN.md "BiCGStab(l)" has the
// byte count and the deviations.  Per sub-step j (U[0..l], R[0..l], r̃ are the work vectors):
//
//   scalars A     β = α ρ1 / ρ0                                            (j = 0: ρ0 = -ω ρ0 first; restart: r̃ := R[0], β = 0)
//   k_bl_dir      U[i] = R[i] - β U[i],  i = 0 .. j                         one launch, every vector read and written once
//   SpMV mode 1   U[j+1] = Â U[j],  σ = (U[j+1], r̃) fused
//   scalars B     α = ρ1 / σ
//   k_bl_upd      x += α U[0],  R[i] -= α U[i+1] (i = 0 .. j),  (R[0], R[0])_W in the same pass
//   scalars C     iters += 1, the stopping test
//   SpMV mode 1   R[j+1] = Â R[j],  the next ρ1 = (R[j+1], r̃) fused       (the last sub-step: mode 0, no dot)
// and per outer iteration
//   k_bl_gram     the (l+1)(l+2)/2 entries of the Gram matrix of R[0..l], every vector read once
//   scalars GRAM  the l x l system by Cholesky with diagonal pivoting (pg_host_algos.h bicgstabl_small_solve): γ
//   k_bl_apply    x += Σ γ_i R[i-1],  R[0] -= Σ γ_i R[i],  U[0] -= Σ γ_i U[i];  (r,r), (r,r)_W and (r, r̃) of the new r
//   scalars D     ω = γ_l, the stopping test, the restart rule of the plain loop
//
// It iterates on the same left-preconditioned, equilibrated system Â = B⁻¹SAS as the other methods, from a zero initial
// guess (as GMRES here and IterativeSolvers do), and stops on the same quantity as BiCGStab: (r,r)_W <= max(reltol² (b,b)_W,
// abstol²), W = S², the residual in the units of x (pg_spmv.h).  All scalars stay on the device; every reduction is per-block
// partial sums and a second stage in a fixed order (no atomics): a solve is bitwise reproducible.  The host polls the done
// flag every check_every outer iterations.
//
// Robustness.  ρ or σ vanishing (or not finite) inside a sweep: the rest of the sweep runs with α = β = 0, which keeps R[0..l]
// the power basis of R[0] -- the minimal-residual step is then one GMRES(l)-like step -- and the next sweep restarts with
// r̃ := r.  A shrunk small system (a pivot that is not safely positive), ω = 0 and the collapse of (r̃, r) by the plain loop's
// rule restart as well.  When the recurrence residual meets the test the TRUE residual b̂ - Âx is formed (one more product)
// and decides: met -> converged, with the true norm reported; not met -> the iteration continues from it (R[0] := true
// residual, restart), at most three times, then the solve is reported unconverged (S_DONE = 5).  A residual that is not
// finite ends the solve unconverged with x = 0 (S_DONE = 2): never NaN.
//
// Counting: iters = BiCG sub-steps (two products each, the unit maxiter caps for BiCGStab: l = 1 is directly comparable);
// products = 2 iters + confirmations.  No sweep starts at iters >= maxiter.
#include "pg_krylov.h"
#include "pg_spmv.h"
#include "pg_host_algos.h"

using namespace pg;

namespace {

constexpr int MAXL = pghost::BL_MAX_L;
constexpr int LD = pghost::BL_LD;
constexpr int NGRAM = (MAXL + 1) * (MAXL + 2) / 2;   // 45
constexpr int MAX_CONTINUES = 3;

// device scalars of the method (KrylovWork::bl); the stopping scalars live in KrylovWork::sc
enum { B_RHO0 = 0, B_RHO1, B_ALPHA, B_OMEGA, B_BETA, B_RHAT2, B_RR, B_PEND /* restart at the next sweep */,
       B_NOW /* the running sweep restarted: k_bl_dir copies R[0] into r̃ */, B_FORCE /* breakdown in this sweep */,
       B_CONT /* continuations from a true residual */, B_RESTARTS, B_K /* size of the small system solved */,
       B_GAMMA /* MAXL + 1 */, B_G = B_GAMMA + MAXL + 1 /* LD x LD */, B_COUNT = B_G + LD * LD };
enum { P_INIT = 0, P_A, P_B, P_C, P_GRAM, P_D, P_CONFIRM };
// S_DONE: 0 running, 1 converged (true residual), 2 not finite / Âr = 0, 4 the recurrence residual met the test: the host
// queues the confirmation, 5 the true residual failed after MAX_CONTINUES continuations

__device__ inline bool fin(double v) { return pghost::bl_finite(v); }

__global__ void k_bl_reset(double* __restrict__ sc, double* __restrict__ bl, double reltol2, double abstol2) {
  for (int i = threadIdx.x; i < S_COUNT; i += blockDim.x) sc[i] = i == S_RELTOL2 ? reltol2 : (i == S_ABSTOL2 ? abstol2 : 0.0);
  for (int i = threadIdx.x; i < B_COUNT; i += blockDim.x) bl[i] = 0.0;
}

// r = b - Ax (Ax == nullptr: r = b and x = 0), ghosts zeroed; partial slot 0 = (r,r), slot 1 = (r,r)_W
__global__ __launch_bounds__(BLOCK) void k_bl_resid(i64 n, i64 nvec, const double* __restrict__ b, const double* __restrict__ Ax,
                                                    double* __restrict__ r, double* __restrict__ x_zero,
                                                    const double* __restrict__ ds, double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  double acc = 0.0, accw = 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < nvec; i += (i64)gridDim.x * BLOCK) {
    double ri = 0.0;
    if (i < n) {
      ri = Ax ? b[i] - Ax[i] : b[i];
      acc += ri * ri;
      accw += (ds[i] * ri) * (ds[i] * ri);
    }
    r[i] = ri;
    if (x_zero) x_zero[i] = 0.0;
  }
  const double t = block_sum(acc, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
  const double tw = block_sum(accw, s_red);
  if (threadIdx.x == 0) partials[gridDim.x + blockIdx.x] = tw;
}

// U[i] = R[i] - β U[i], i = 0 .. j  (β == 0: U[i] = R[i], whatever U held); the first sub-step of a restarted sweep: r̃ = R[0]
__global__ __launch_bounds__(BLOCK) void k_bl_dir(i64 n, i64 stride, int j, double* __restrict__ U, const double* __restrict__ R,
                                                  double* __restrict__ rt, const double* __restrict__ bl,
                                                  const double* __restrict__ sc) {
  if (sc[S_DONE] != 0.0) return;
  const double beta = bl[B_BETA];
  const bool copy_rt = j == 0 && bl[B_NOW] != 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    for (int q = 0; q <= j; ++q) {
      const size_t at = (size_t)q * stride + i;
      const double rq = R[at];
      U[at] = beta == 0.0 ? rq : rq - beta * U[at];
      if (q == 0 && copy_rt) rt[i] = rq;
    }
  }
}

// x += α U[0],  R[i] -= α U[i+1], i = 0 .. j;  partial slot 0 = (R[0], R[0])_W after the update  (α == 0: the sums only)
__global__ __launch_bounds__(BLOCK) void k_bl_upd(i64 n, i64 stride, int j, const double* __restrict__ U, double* __restrict__ R,
                                                  double* __restrict__ x, const double* __restrict__ ds,
                                                  const double* __restrict__ bl, const double* __restrict__ sc,
                                                  double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  if (sc[S_DONE] != 0.0) return;
  const double alpha = bl[B_ALPHA];
  double accw = 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    double r0 = R[i];
    if (alpha != 0.0) {
      x[i] += alpha * U[i];
      r0 -= alpha * U[(size_t)stride + i];
      R[i] = r0;
      for (int q = 1; q <= j; ++q) R[(size_t)q * stride + i] -= alpha * U[(size_t)(q + 1) * stride + i];
    }
    accw += (ds[i] * r0) * (ds[i] * r0);
  }
  const double tw = block_sum(accw, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = tw;
}

// Gram matrix of R[0..l]: slot of (a, b), a <= b, is a (2 LP1 - a + 1) / 2 + (b - a); every vector read once
template <int LP1>
__global__ __launch_bounds__(BLOCK) void k_bl_gram(i64 n, i64 stride, const double* __restrict__ R, const double* __restrict__ sc,
                                                   double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  if (sc[S_DONE] != 0.0) return;
  constexpr int NS = LP1 * (LP1 + 1) / 2;
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    double v[LP1];
#pragma unroll
    for (int q = 0; q < LP1; ++q) v[q] = R[(size_t)q * stride + i];
    int s = 0;
#pragma unroll
    for (int a = 0; a < LP1; ++a)
#pragma unroll
      for (int b = a; b < LP1; ++b) acc[s++] += v[a] * v[b];
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const double t = block_sum(acc[s], s_red);
    if (threadIdx.x == 0) partials[(size_t)s * gridDim.x + blockIdx.x] = t;
  }
}

// x += Σ γ_i R[i-1],  R[0] -= Σ γ_i R[i],  U[0] -= Σ γ_i U[i]  (i = 1 .. l);  partial slots 0 / 1 / 2 = (r,r), (r,r)_W, (r, r̃)
template <int LP1>
__global__ __launch_bounds__(BLOCK) void k_bl_apply(i64 n, i64 stride, double* __restrict__ R, double* __restrict__ U,
                                                    double* __restrict__ x, const double* __restrict__ rt,
                                                    const double* __restrict__ ds, const double* __restrict__ bl,
                                                    const double* __restrict__ sc, double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  if (sc[S_DONE] != 0.0) return;
  double g[LP1];
#pragma unroll
  for (int q = 0; q < LP1; ++q) g[q] = bl[B_GAMMA + q];
  double acc = 0.0, accw = 0.0, accr = 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    double rprev = R[i], r0 = rprev, u0 = U[i], xi = x[i];
#pragma unroll
    for (int q = 1; q < LP1; ++q) {   // (a shrunk system: γ_q = 0 beyond it, times vectors that are finite)
      const double rq = R[(size_t)q * stride + i];
      xi += g[q] * rprev;
      r0 -= g[q] * rq;
      u0 -= g[q] * U[(size_t)q * stride + i];
      rprev = rq;
    }
    x[i] = xi;
    R[i] = r0;
    U[i] = u0;
    acc += r0 * r0;
    accw += (ds[i] * r0) * (ds[i] * r0);
    accr += r0 * rt[i];
  }
  const double t = block_sum(acc, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
  const double tw = block_sum(accw, s_red);
  if (threadIdx.x == 0) partials[gridDim.x + blockIdx.x] = tw;
  const double tr = block_sum(accr, s_red);
  if (threadIdx.x == 0) partials[2 * (size_t)gridDim.x + blockIdx.x] = tr;
}

// the scalar phases: sums of the partial slots the phase reads (fixed order), then one thread derives
__global__ __launch_bounds__(BLOCK) void k_bl_scalar(int phase, int j, int l, int grid, const double* __restrict__ partials,
                                                     double* __restrict__ sc, double* __restrict__ bl) {
  __shared__ double s_red[BLOCK / 64];
  __shared__ double s_sum[NGRAM];
  if (phase == P_CONFIRM ? sc[S_DONE] != 4.0 : (phase != P_INIT && sc[S_DONE] != 0.0)) return;
  int nslots = 0;
  switch (phase) {
    case P_INIT: case P_CONFIRM: nslots = 2; break;
    case P_A: nslots = j > 0 ? 1 : 0; break;
    case P_B: case P_C: nslots = 1; break;
    case P_GRAM: nslots = (l + 1) * (l + 2) / 2; break;
    case P_D: nslots = 3; break;
  }
  for (int s = 0; s < nslots; ++s) {
    double a = 0.0;
    for (int i = threadIdx.x; i < grid; i += BLOCK) a += partials[(size_t)s * grid + i];
    const double t = block_sum(a, s_red);
    if (threadIdx.x == 0) s_sum[s] = t;
  }
  if (threadIdx.x != 0) return;
  switch (phase) {
    case P_INIT: {
      const double rr = s_sum[0], bbw = s_sum[1];
      sc[S_BB] = bbw; sc[S_RR] = bbw; sc[S_RR0] = bbw; sc[S_ITERS] = 0.0;
      const double t2 = sc[S_RELTOL2] * bbw;
      sc[S_TOL2] = t2 > sc[S_ABSTOL2] ? t2 : sc[S_ABSTOL2];
      bl[B_RHO0] = 1.0; bl[B_ALPHA] = 0.0; bl[B_OMEGA] = 1.0; bl[B_RHO1] = rr; bl[B_RHAT2] = rr; bl[B_RR] = rr;
      bl[B_PEND] = 1.0;
      sc[S_DONE] = !fin(bbw) ? 2.0 : (bbw <= sc[S_TOL2] ? 1.0 : 0.0);   // (b = 0: x = 0 is exact, nothing to confirm)
      break;
    }
    case P_A: {
      double rho0 = bl[B_RHO0], rho1, beta;
      bool force = bl[B_FORCE] != 0.0;
      if (j == 0) {
        rho0 = -bl[B_OMEGA] * rho0;
        rho1 = bl[B_RHO1];
        force = false;
        const bool restart = bl[B_PEND] != 0.0 || rho0 == 0.0 || rho1 == 0.0 || !fin(rho0) || !fin(rho1);
        if (restart) {
          rho1 = bl[B_RR];
          bl[B_RHAT2] = rho1;
          beta = 0.0;
          bl[B_PEND] = 0.0;
          bl[B_NOW] = 1.0;
          bl[B_RESTARTS] += 1.0;
        } else {
          beta = bl[B_ALPHA] * (rho1 / rho0);
          bl[B_NOW] = 0.0;
        }
      } else {
        rho1 = s_sum[0];
        if (force || rho0 == 0.0 || rho1 == 0.0 || !fin(rho1)) { force = true; beta = 0.0; }
        else beta = bl[B_ALPHA] * (rho1 / rho0);
      }
      if (!fin(beta)) { force = true; beta = 0.0; }
      bl[B_FORCE] = force ? 1.0 : 0.0;
      bl[B_BETA] = beta;
      bl[B_RHO1] = rho1;
      bl[B_RHO0] = rho1;
      break;
    }
    case P_B: {
      const double sigma = s_sum[0];
      double alpha = 0.0;
      bool force = bl[B_FORCE] != 0.0;
      if (force || sigma == 0.0 || !fin(sigma)) force = true;
      else {
        alpha = bl[B_RHO0] / sigma;
        if (!fin(alpha)) { force = true; alpha = 0.0; }
      }
      bl[B_FORCE] = force ? 1.0 : 0.0;
      bl[B_ALPHA] = alpha;
      break;
    }
    case P_C: {
      const double rrw = s_sum[0];
      sc[S_ITERS] += 1.0;
      sc[S_RR] = rrw;
      if (!fin(rrw)) sc[S_DONE] = 2.0;
      else if (rrw <= sc[S_TOL2]) sc[S_DONE] = 4.0;
      break;
    }
    case P_GRAM: {
      double* G = bl + B_G;
      int s = 0;
      for (int a = 0; a <= l; ++a)
        for (int b = a; b <= l; ++b) { G[a * LD + b] = s_sum[s]; G[b * LD + a] = s_sum[s]; ++s; }
      const int k = pghost::bicgstabl_small_solve(G, l, bl + B_GAMMA);
      bl[B_K] = (double)k;
      if (k == 0) sc[S_DONE] = 2.0;
      break;
    }
    case P_D: {
      const double rr = s_sum[0], rrw = s_sum[1], rho1 = s_sum[2];
      const double omega = bl[B_GAMMA + l];
      bl[B_RR] = rr; bl[B_RHO1] = rho1; bl[B_OMEGA] = omega;
      sc[S_RR] = rrw;
      if (!fin(rrw)) sc[S_DONE] = 2.0;
      else if (rrw <= sc[S_TOL2]) sc[S_DONE] = 4.0;
      else if (bl[B_FORCE] != 0.0 || (int)bl[B_K] < l || omega == 0.0 || rho1 * rho1 < 1e-20 * bl[B_RHAT2] * rr) bl[B_PEND] = 1.0;
      break;
    }
    case P_CONFIRM: {
      // the TRUE residual of the state the recurrence accepted
      const double rr = s_sum[0], rrw = s_sum[1];
      sc[S_RED0] = sc[S_RR];   // (diagnostics: the recurrence value that asked)
      sc[S_RR] = rrw;
      if (rrw <= sc[S_TOL2]) sc[S_DONE] = 1.0;
      else if (bl[B_CONT] >= (double)MAX_CONTINUES) sc[S_DONE] = 5.0;
      else { bl[B_CONT] += 1.0; bl[B_RR] = rr; bl[B_PEND] = 1.0; sc[S_DONE] = 0.0; }
      break;
    }
  }
}

template <int LP1>
void launch_gram_apply(bool gram, int G, hipStream_t st, i64 n, i64 stride, double* R, double* U, double* x, const double* rt,
                       const double* ds, const double* bl, const double* sc, double* part) {
  if (gram) hipLaunchKernelGGL(k_bl_gram<LP1>, dim3(G), dim3(BLOCK), 0, st, n, stride, (const double*)R, sc, part);
  else hipLaunchKernelGGL(k_bl_apply<LP1>, dim3(G), dim3(BLOCK), 0, st, n, stride, R, U, x, rt, ds, bl, sc, part);
}

}  // namespace

namespace pg {

void bicgstabl_solve(const CsrMatrix& A, const Numbering& nb, const Slab& slab, const double* b, double* x, KrylovWork& w,
                     const pg_krylov_opts& opts, SolveStats& stats) {
  Context& cx = ctx();
  hipStream_t st = cx.stream;
  const i64 n = A.n, nvec = nb.n_vec();
  PG_REQUIRE(w.n >= n && w.nvec >= nvec, "krylov workspace too small");
  const int l = opts.restart > 0 ? opts.restart : 2;
  PG_REQUIRE(l <= MAXL, "BiCGStab(l) refused: l = " + std::to_string(l) + " is more than 8 (pg_krylov_opts.restart carries l)");
  PG_REQUIRE(cx.nranks == 1 && !cx.comm, "BiCGStab(l) refused: the solve runs on several ranks (one rank only)");
  const int G = w.grid;
  const int maxiter = opts.maxiter > 0 ? opts.maxiter : 100000;
  const int check_every = opts.check_every > 0 ? opts.check_every : 4;
  const i64 stride = ((nvec > 0 ? nvec : 1) + 1) & ~(i64)1;       // even: every work vector starts 16-byte aligned
  if (w.bl_l != l || w.bl_stride != stride) {
    w.bl_vecs.alloc((2 * (i64)(l + 1) + 1) * stride);
    w.bl_vecs.zero();                                             // ghost segments and not-yet-written powers start defined
    w.bl.alloc(B_COUNT);
    w.bl_partials.alloc((i64)NGRAM * G);
    w.bl_l = l;
    w.bl_stride = stride;
  }
  double* R = w.bl_vecs.p;
  double* U = R + (size_t)(l + 1) * stride;
  double* rt = U + (size_t)(l + 1) * stride;
  double* bl = w.bl.p;
  double* part = w.bl_partials.p;
  const double* ds = A.ds.p;

  auto scalar = [&](int phase, int j, const double* partials) {
    hipLaunchKernelGGL(k_bl_scalar, dim3(1), dim3(BLOCK), 0, st, phase, j, l, G, partials, w.sc.p, bl);
  };
  auto gram_apply = [&](bool gram) {
    switch (l) {
      case 1: launch_gram_apply<2>(gram, G, st, n, stride, R, U, x, rt, ds, bl, w.sc.p, part); break;
      case 2: launch_gram_apply<3>(gram, G, st, n, stride, R, U, x, rt, ds, bl, w.sc.p, part); break;
      case 3: launch_gram_apply<4>(gram, G, st, n, stride, R, U, x, rt, ds, bl, w.sc.p, part); break;
      case 4: launch_gram_apply<5>(gram, G, st, n, stride, R, U, x, rt, ds, bl, w.sc.p, part); break;
      case 5: launch_gram_apply<6>(gram, G, st, n, stride, R, U, x, rt, ds, bl, w.sc.p, part); break;
      case 6: launch_gram_apply<7>(gram, G, st, n, stride, R, U, x, rt, ds, bl, w.sc.p, part); break;
      case 7: launch_gram_apply<8>(gram, G, st, n, stride, R, U, x, rt, ds, bl, w.sc.p, part); break;
      default: launch_gram_apply<9>(gram, G, st, n, stride, R, U, x, rt, ds, bl, w.sc.p, part); break;
    }
  };
  auto sweep = [&]() {
    for (int j = 0; j < l; ++j) {
      double* Uj = U + (size_t)j * stride;
      double* Rj = R + (size_t)j * stride;
      scalar(P_A, j, w.partials.p);
      hipLaunchKernelGGL(k_bl_dir, dim3(G), dim3(BLOCK), 0, st, n, stride, j, U, (const double*)R, rt, (const double*)bl,
                         (const double*)w.sc.p);
      spmv_with_halo(1, A, nb, slab, Uj, Uj + stride, rt, w.partials.p, w.sc.p, G, st);
      scalar(P_B, j, w.partials.p);
      hipLaunchKernelGGL(k_bl_upd, dim3(G), dim3(BLOCK), 0, st, n, stride, j, (const double*)U, R, x, ds, (const double*)bl,
                         (const double*)w.sc.p, part);
      scalar(P_C, j, part);
      if (j + 1 < l) spmv_with_halo(1, A, nb, slab, Rj, Rj + stride, rt, w.partials.p, w.sc.p, G, st);
      else spmv_with_halo(0, A, nb, slab, Rj, Rj + stride, nullptr, nullptr, w.sc.p, G, st);
    }
    gram_apply(true);
    scalar(P_GRAM, 0, part);
    gram_apply(false);
    scalar(P_D, 0, part);
  };

  hipLaunchKernelGGL(k_bl_reset, dim3(1), dim3(BLOCK), 0, st, w.sc.p, bl, opts.reltol * opts.reltol, opts.abstol * opts.abstol);
  hipLaunchKernelGGL(k_bl_resid, dim3(G), dim3(BLOCK), 0, st, n, nvec, b, (const double*)nullptr, R, x, ds, part);
  scalar(P_INIT, 0, part);
  int launched = 0, polls = 0, confirmations = 0;
  bool done = false;
  while (!done) {
    for (int it = 0; it < check_every && launched < maxiter; ++it) {
      sweep();
      launched += l;
    }
    ++polls;
    PG_HIP(hipGetLastError());
    PG_HIP(hipMemcpyAsync(w.h_sc, w.sc.p, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));
    if (w.h_sc[S_DONE] == 4.0) {
      // the recurrence residual met the test: the true residual of x decides (k_bl_scalar P_CONFIRM)
      spmv_with_halo(0, A, nb, slab, x, w.t.p, nullptr, nullptr, nullptr, G, st);
      hipLaunchKernelGGL(k_bl_resid, dim3(G), dim3(BLOCK), 0, st, n, nvec, b, (const double*)w.t.p, R, (double*)nullptr, ds, part);
      scalar(P_CONFIRM, 0, part);
      ++confirmations;
      PG_HIP(hipGetLastError());
      PG_HIP(hipMemcpyAsync(w.h_sc, w.sc.p, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost, st));
      PG_HIP(hipStreamSynchronize(st));
      launched = (int)w.h_sc[S_ITERS];   // (what was queued behind the accepted sub-step returned at the done flag)
    }
    if (w.h_sc[S_DONE] != 0.0 || launched >= maxiter) done = true;
  }
  const double flag = w.h_sc[S_DONE];
  stats.iters = (int)w.h_sc[S_ITERS];
  stats.polls = polls;
  stats.converged = flag == 1.0 ? 1 : 0;
  stats.resnorm = std::sqrt(w.h_sc[S_RR]);
  stats.bnorm = std::sqrt(w.h_sc[S_BB]);
  stats.products = 2 * (i64)stats.iters + confirmations;
  if (flag == 2.0) {
    // a residual that is not finite (or Âr = 0): the state is not handed back
    PG_HIP(hipMemsetAsync(x, 0, sizeof(double) * (size_t)nvec, st));
    stats.resnorm = stats.bnorm;
  }
  if (config().debug)
    fprintf(stderr, "[pg_bicgstabl] l=%d done=%g iters=%d confirmations=%d rr=%g tol2=%g\n", l, flag, stats.iters, confirmations,
            w.h_sc[S_RR], w.h_sc[S_TOL2]);
}

}  // namespace pg
