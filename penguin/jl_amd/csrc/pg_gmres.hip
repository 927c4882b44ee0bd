// pg_gmres.hip -- restarted GMRES(m) on the device: `method = IterativeSolvers.gmres`, the DEFAULT of the reference's
// solve_system! (src/solver.jl:158-188; 18 call sites in its examples / tests use it, e.g. test/solver_test.jl:71).
//
//   reference (IterativeSolvers 0.9.4 gmres!, one thread)            here
//   Arnoldi with modified Gram-Schmidt: j dot/axpy pairs per step     classical Gram-Schmidt applied twice (CGS2): the j
//                                                                     dots of a pass are ONE kernel per group of 8 basis
//                                                                     vectors (2 reductions per step instead of j; with
//                                                                     several ranks 3 all-reduces per step instead of j+1)
//   Givens rotations / least squares on the host                      one-thread kernels on device scalars: H, cs, sn, g
//                                                                     never leave the GPU; the host polls the done flag
//                                                                     once per restart cycle
//   restart = 20, zero initial guess, ||r|| <= max(reltol ||r0||, abstol) on the Givens residual estimate    same INSIDE a
//                                                                     cycle; a solve is ACCEPTED on the true residual in the
//                                                                     units of x (below)
//
// Stopping test.  The Givens estimate is the norm of the PRECONDITIONED residual r̂ = B⁻¹S(b - Ax), which weighs a row by
// |a_ii|^-1/2: 1 for the decoupled border rows but 800 for the bulk rows at 512^3, so ||r̂|| <= reltol ||b̂|| left T at 2e-9 of
// the converged field there (pg_spmv.h, the same finding as for BiCGStab).  The estimate therefore only ENDS A CYCLE; at
// every restart the true residual is recomputed anyway (b̂ - Âx, IterativeSolvers does the same) and the solve is accepted
// on  ||S r̂|| <= max(reltol ||S b̂||, abstol) -- the residual of the row-scaled system, whose entries are errors of x.  When
// the estimate was met but the weighted test is not, the next cycle runs with the inner tolerance lowered by the factor
// the weighted norm still has to fall (x 1/4).  S_BB / S_RR report the weighted norms, as BiCGStab and CG do.
//
// It iterates on the same preconditioned system  Â = B⁻¹SAS  as BiCGStab / CG (pg_precond.hip), so the residual it
// minimises is the preconditioned one.  Not on the benchmark path (BiCGStab needs 18 vector passes per two SpMVs, GMRES
// ~4j + 6 per SpMV); it is here so that `method = gmres` means GMRES.
#include "pg_host_algos.h"
#include "pg_krylov.h"
#include "pg_spmv.h"
#include "pg_specest.h"

using namespace pg;

namespace {

constexpr int GRP = GM_GRP;   // basis vectors handled per launch of the dot / update kernels

// device scalar block of GMRES (KrylovWork::gm): the layout and the three one-thread steps are pg_host_algos.h's -- the code the
// CPU suite runs under sanitizers (tests/gmres_host.cpp)
using pghost::GmLayout;

// the steps' scalars in the S_* block: S_RHAT2 holds the weighted tolerance here, S_RRW (b,b), S_FORCE the not-finite mark
constexpr pghost::GmSlots gm_slots() {
  return pghost::GmSlots{S_BB, S_RR, S_RRW, S_ITERS, S_RELTOL2, S_ABSTOL2, S_TOL2, S_RHAT2, S_DONE, S_FORCE};
}

// v = b - Ax (Ax == nullptr: v = b), ghosts zeroed; partial slot 0 = (v,v), slot 1 = (v,v)_W (weights ds^2)
__global__ __launch_bounds__(BLOCK) void k_gm_resid(i64 n, i64 nvec, const double* __restrict__ b, const double* __restrict__ Ax,
                                                    double* __restrict__ v, double* __restrict__ x_zero,
                                                    const double* __restrict__ ds, double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  double acc = 0.0, accw = 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < nvec; i += (i64)gridDim.x * BLOCK) {
    double vi = 0.0;
    if (i < n) {
      vi = Ax ? b[i] - Ax[i] : b[i];
      accw += (ds[i] * vi) * (ds[i] * vi);
    }
    v[i] = vi;
    if (x_zero) x_zero[i] = 0.0;
    acc += vi * vi;
  }
  const double t = block_sum(acc, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
  const double tw = block_sum(accw, s_red);
  if (threadIdx.x == 0) partials[gridDim.x + blockIdx.x] = tw;
}

}  // namespace

// ---- shared with the spectral estimate (pg_specest.hip), declared in pg_specest.h ----
namespace pg {

// sums of `nslots` partial slots (fixed order: deterministic) into out[0..nslots)
__global__ __launch_bounds__(BLOCK) void k_gm_reduce(int nslots, int grid, const double* __restrict__ partials,
                                                     double* __restrict__ out, const double* __restrict__ sc, int check_done) {
  __shared__ double s_red[BLOCK / 64];
  if (check_done && sc[S_DONE] != 0.0) return;
  for (int s = 0; s < nslots; ++s) {
    double a = 0.0;
    for (int i = threadIdx.x; i < grid; i += BLOCK) a += partials[(size_t)s * grid + i];
    const double t = block_sum(a, s_red);
    if (threadIdx.x == 0) out[s] = t;
  }
}

}  // namespace pg

namespace {

// start of a restart cycle (and verdict on the one before): pghost::gm_begin
__global__ void k_gm_begin(GmLayout L, double* __restrict__ gm, double* __restrict__ sc, int first) {
  pghost::gm_begin(L, gm_slots(), gm, sc, first);
}

}  // namespace

// ---- shared with the spectral estimate (pg_specest.hip), declared in pg_specest.h ----
namespace pg {

__global__ __launch_bounds__(BLOCK) void k_gm_scale(i64 n, const double* __restrict__ sc, const double* __restrict__ gm,
                                                    int invn_at, double* __restrict__ v) {
  if (sc[S_DONE] != 0.0) return;
  const double f = gm[invn_at];
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) v[i] *= f;
}

// partial slots [k0, k0+cnt) = (V_i, w), i = k0 .. k0+cnt-1   (cnt <= GRP)
__global__ __launch_bounds__(BLOCK) void k_gm_dots(i64 n, i64 stride, int k0, int cnt, const double* __restrict__ V,
                                                   const double* __restrict__ w, const double* __restrict__ sc,
                                                   double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  if (sc[S_DONE] != 0.0) return;
  double acc[GRP];
#pragma unroll
  for (int q = 0; q < GRP; ++q) acc[q] = 0.0;
  const double* __restrict__ V0 = V + (size_t)k0 * stride;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    const double wi = w[i];
#pragma unroll
    for (int q = 0; q < GRP; ++q)
      if (q < cnt) acc[q] += V0[(size_t)q * stride + i] * wi;
  }
#pragma unroll
  for (int q = 0; q < GRP; ++q) {
    if (q < cnt) {   // block-uniform
      const double t = block_sum(acc[q], s_red);
      if (threadIdx.x == 0) partials[(size_t)(k0 + q) * gridDim.x + blockIdx.x] = t;
    }
  }
}

// w -= sum_{i in [k0,k0+cnt)} h_i V_i ;  norm_slot >= 0: partial slot norm_slot = (w,w) after the update
__global__ __launch_bounds__(BLOCK) void k_gm_update(i64 n, i64 stride, int k0, int cnt, const double* __restrict__ V,
                                                     double* __restrict__ w, const double* __restrict__ h,
                                                     const double* __restrict__ sc, int norm_slot,
                                                     double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  if (sc[S_DONE] != 0.0) return;
  double hc[GRP];
#pragma unroll
  for (int q = 0; q < GRP; ++q) hc[q] = q < cnt ? h[k0 + q] : 0.0;
  const double* __restrict__ V0 = V + (size_t)k0 * stride;
  double acc = 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    double wi = w[i];
#pragma unroll
    for (int q = 0; q < GRP; ++q)
      if (q < cnt) wi -= hc[q] * V0[(size_t)q * stride + i];
    w[i] = wi;
    acc += wi * wi;
  }
  if (norm_slot >= 0) {
    const double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[(size_t)norm_slot * gridDim.x + blockIdx.x] = t;
  }
}

}  // namespace pg

namespace {

// column j of the Hessenberg matrix: pghost::gm_hess
__global__ void k_gm_hess(GmLayout L, int j, double* __restrict__ gm, double* __restrict__ sc) {
  pghost::gm_hess(L, gm_slots(), j, gm, sc);
}

// y = H(0:J,0:J)^-1 g(0:J): pghost::gm_solve_y
__global__ void k_gm_solve_y(GmLayout L, double* __restrict__ gm) { pghost::gm_solve_y(L, gm); }

// x += sum_{i<J} y_i V_i
__global__ __launch_bounds__(BLOCK) void k_gm_xupdate(i64 n, i64 stride, GmLayout L, const double* __restrict__ gm,
                                                      const double* __restrict__ V, double* __restrict__ x) {
  const int J = (int)gm[L.J()];
  if (J <= 0) return;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    double xi = x[i];
    for (int k = 0; k < J; ++k) xi += gm[L.y(k)] * V[(size_t)k * stride + i];
    x[i] = xi;
  }
}

}  // namespace

namespace pg {

void gmres_solve(const CsrMatrix& A, const Numbering& nb, const Slab& slab, const double* b, double* x, KrylovWork& w,
                 const pg_krylov_opts& opts, SolveStats& stats) {
  Context& cx = ctx();
  hipStream_t st = cx.stream;
  const i64 n = A.n, nvec = nb.n_vec();
  PG_REQUIRE(w.n == n && w.nvec == nvec, "krylov workspace size mismatch");
  const int G = w.grid;
  int m = opts.restart > 0 ? opts.restart : 20;                 // IterativeSolvers: restart = min(20, size(A, 2))
  m = std::min(m, 200);
  const bool multi = cx.nranks > 1 || cx.comm;
  if (!multi && n > 0) m = (int)std::min<i64>(m, n);
  const int maxiter = opts.maxiter > 0 ? opts.maxiter : 100000;
  const GmLayout L{m};
  const i64 stride = nvec > 0 ? nvec : 1;
  if (w.gm_m != m) {
    w.gm_basis.alloc((i64)(m + 1) * stride);
    w.gm_basis.zero();                                          // ghost segments of every basis vector start defined
    w.gm.alloc(L.size());
    w.gm_partials.alloc((i64)(m + 2) * G);
    w.gm_m = m;
  }
  w.gm.zero();
  double* V = w.gm_basis.p;
  double* gm = w.gm.p;
  double* part = w.gm_partials.p;

  double hs[S_COUNT];
  std::memset(hs, 0, sizeof(hs));
  hs[S_RELTOL2] = opts.reltol * opts.reltol;
  hs[S_ABSTOL2] = opts.abstol * opts.abstol;
  PG_HIP(hipMemcpyAsync(w.sc.p, hs, sizeof(hs), hipMemcpyHostToDevice, st));

  auto reduce = [&](int nslots, double* out, bool check_done) {
    hipLaunchKernelGGL(k_gm_reduce, dim3(1), dim3(BLOCK), 0, st, nslots, G, part, out, w.sc.p, check_done ? 1 : 0);
    if (multi) comm_allreduce_sum_f64(out, nslots, st);   // identical sums, hence identical control flow, on every rank
  };

  int iters = 0;   // Arnoldi steps that ran (S_ITERS): the unit maxiter caps -- a cycle the estimate ends early is charged what it ran
  bool done = false;
  // r = b - Â x  ->  v_0 = r / ||r||, with the verdict on x (k_gm_begin): at the start, and after every cycle
  auto restart = [&](bool first) {
    if (first) {
      hipLaunchKernelGGL(k_gm_resid, dim3(G), dim3(BLOCK), 0, st, n, nvec, b, (const double*)nullptr, V, x, (const double*)A.ds.p, part);
    } else {
      spmv_halo(A, nb, slab, x, w.t.p, st);
      hipLaunchKernelGGL(k_gm_resid, dim3(G), dim3(BLOCK), 0, st, n, nvec, b, (const double*)w.t.p, V, (double*)nullptr,
                         (const double*)A.ds.p, part);
    }
    reduce(2, gm + L.h2(0), false);
    hipLaunchKernelGGL(k_gm_begin, dim3(1), dim3(1), 0, st, L, gm, w.sc.p, first ? 1 : 0);
    hipLaunchKernelGGL(k_gm_scale, dim3(G), dim3(BLOCK), 0, st, n, w.sc.p, gm, L.invn(), V);
  };
  restart(true);
  while (!done) {
    const int steps = std::max(0, std::min(m, maxiter - iters));
    for (int j = 0; j < steps; ++j) {
      double* vj = V + (size_t)j * stride;
      double* wv = V + (size_t)(j + 1) * stride;
      spmv_with_halo(0, A, nb, slab, vj, wv, nullptr, nullptr, w.sc.p, spmv_default_grid(n), st);
      const int k = j + 1;
      for (int pass = 0; pass < 2; ++pass) {
        double* h = gm + (pass == 0 ? L.h1(0) : L.h2(0));
        for (int k0 = 0; k0 < k; k0 += GRP)
          hipLaunchKernelGGL(k_gm_dots, dim3(G), dim3(BLOCK), 0, st, n, stride, k0, std::min(GRP, k - k0), (const double*)V,
                             (const double*)wv, (const double*)w.sc.p, part);
        reduce(k, h, true);
        for (int k0 = 0; k0 < k; k0 += GRP) {
          const bool last = pass == 1 && k0 + GRP >= k;
          hipLaunchKernelGGL(k_gm_update, dim3(G), dim3(BLOCK), 0, st, n, stride, k0, std::min(GRP, k - k0), (const double*)V, wv,
                             (const double*)h, (const double*)w.sc.p, last ? 0 : -1, part);
        }
      }
      reduce(1, gm + L.h2(k), true);   // ||w||^2 after both passes
      hipLaunchKernelGGL(k_gm_hess, dim3(1), dim3(1), 0, st, L, j, gm, w.sc.p);
      hipLaunchKernelGGL(k_gm_scale, dim3(G), dim3(BLOCK), 0, st, n, w.sc.p, gm, L.invn(), wv);
    }
    // end of the cycle (or convergence inside it): x += V y
    hipLaunchKernelGGL(k_gm_solve_y, dim3(1), dim3(1), 0, st, L, gm);
    hipLaunchKernelGGL(k_gm_xupdate, dim3(G), dim3(BLOCK), 0, st, n, stride, L, (const double*)gm, (const double*)V, x);
    restart(false);    // true residual of the new x: accepted (S_DONE = 1) or the next cycle is ready
    PG_HIP(hipGetLastError());
    PG_HIP(hipMemcpyAsync(w.h_sc, w.sc.p, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));
    iters = (int)w.h_sc[S_ITERS];
    if (w.h_sc[S_DONE] == 1.0 || w.h_sc[S_DONE] == 2.0 || iters >= maxiter || steps == 0) done = true;
  }
  stats.iters = (int)w.h_sc[S_ITERS];
  stats.converged = w.h_sc[S_DONE] == 1.0 ? 1 : 0;
  stats.resnorm = std::sqrt(w.h_sc[S_RR]);
  stats.bnorm = std::sqrt(w.h_sc[S_BB]);
  if (w.h_sc[S_FORCE] != 0.0) {
    // a norm that is not finite (gm_begin / gm_hess stopped the solve): the state is not handed back, as in BiCGStab(l)
    PG_HIP(hipMemsetAsync(x, 0, sizeof(double) * (size_t)nvec, st));
    stats.resnorm = stats.bnorm;
  }
}

}  // namespace pg
