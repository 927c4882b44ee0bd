// pg_specest.hip -- spectral estimate of the Krylov matrix Â = B⁻¹SAS: 30 steps of Arnoldi on the device, the Ritz values on
// the host.  It serves pg_krylov_opts.precond = PG_PRECOND_POLY_EST: the Chebyshev polynomial right
// preconditioner of pg_krylov.hip needs a disc |λ - 1| <= g that holds the spectrum; Gershgorin (decide_poly) gives radii of
// 10 .. 4000 on diphasic systems and on Robin / Neumann interfaces whose true spectra lie inside (0, 2).
//
//   start     v0[i] = cos(1 + c i), c = 12.9898 * 0.7548776662, over the owned rows, normalised.  (The right-hand side is a poor
//             start: some are zero.)  The argument is formed with two roundings -- no fused multiply-add -- so that a host
//             restatement forms the same one: at i = 1e6 a different rounding of the argument moves the cosine by 1e-10.
//   Arnoldi   w = Â v_j through the library's product; classical Gram-Schmidt applied twice with all projections of a pass in
//             one reduction: h1 = V_jᵀw, w -= V_j h1, h2 = V_jᵀw, w -= V_j h2 (+ the partial sums of ||w||²), h = h1 + h2.
//             The dot / update / reduce / scale kernels are GMRES' (pg_gmres.hip: groups of 8 basis vectors per launch, per-block
//             partial sums, one block that adds them in index order): no atomics, two runs give the same bits.
//   breakdown h(j+1, j) <= 1e-14 sets the done flag of the scalar block: every later kernel of the queue returns at once
//             (the products still run; they write vectors nobody reads) and the Ritz values of the j + 1 steps taken stand.
//   host      only the scalar block comes back: the Hessenberg matrix and the count of steps.  Eigenvalues by
//             pghost::hessenberg_eigenvalues;  g_ritz = max |θ - 1|,  g_used = g_ritz + margin,  admitted: g_used < 0.95.
//
// The basis (31 vectors) lives for the estimate only.
#include <chrono>

#include "pg_host_algos.h"
#include "pg_specest.h"

using namespace pg;

namespace {

// device scalars of one estimate, behind the S_COUNT scalars the shared kernels read their done flag from
struct SeLayout {
  int m;
  __host__ __device__ int H(int i, int j) const { return S_COUNT + (m + 1) * j + i; }   // (m+1) x m, column major
  __host__ __device__ int h1(int i) const { return S_COUNT + (m + 1) * m + i; }         // m + 2: first-pass coefficients
  __host__ __device__ int h2(int i) const { return h1(m + 2) + i; }                     // m + 2: second pass, then ||w||²
  __host__ __device__ int invn() const { return h2(m + 2); }                            // 1 / norm of the vector to scale
  __host__ __device__ int steps() const { return invn() + 1; }
  __host__ __device__ int size() const { return steps() + 1; }
};

// v = the start vector (ghosts zero); partial slot 0 = (v, v)
__global__ __launch_bounds__(BLOCK) void k_se_start(i64 n, i64 nvec, double* __restrict__ v, double* __restrict__ partials) {
  __shared__ double s_red[BLOCK / 64];
  constexpr double c = 12.9898 * 0.7548776662;
  double acc = 0.0;
  for (i64 i = blockIdx.x * (i64)BLOCK + threadIdx.x; i < nvec; i += (i64)gridDim.x * BLOCK) {
    const double vi = i < n ? cos(__dadd_rn(1.0, __dmul_rn(c, (double)i))) : 0.0;
    v[i] = vi;
    acc += vi * vi;
  }
  const double t = block_sum(acc, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ void k_se_first(SeLayout L, double* __restrict__ d) {
  const double nn = d[L.h2(0)];
  d[L.invn()] = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;
  d[L.steps()] = 0.0;
}

// column j of the Hessenberg matrix: h = h1 + h2 (CGS2), h(j+1, j) = ||w||; breakdown ends the recursion
__global__ void k_se_hess(SeLayout L, int j, double* __restrict__ d) {
  if (d[S_DONE] != 0.0) return;
  for (int i = 0; i <= j; ++i) d[L.H(i, j)] = d[L.h1(i)] + d[L.h2(i)];
  const double nn = d[L.h2(j + 1)];
  const double hn = sqrt(nn > 0.0 ? nn : 0.0);
  d[L.H(j + 1, j)] = hn;
  d[L.steps()] = (double)(j + 1);
  if (hn <= SPECEST_BREAKDOWN) {
    d[L.invn()] = 0.0;
    d[S_DONE] = 1.0;
  } else {
    d[L.invn()] = 1.0 / hn;
  }
}

}  // namespace

namespace pg {

void specest_require_one_rank() {
  Context& cx = ctx();
  PG_REQUIRE(cx.nranks == 1 && !cx.comm && !cx.local,
             "estimated polynomial preconditioner (precond = PG_PRECOND_POLY_EST) refused: it runs on one rank only (virtual ranks included)");
}

void specest_run(CsrMatrix& A, const Numbering& nb, const Slab& slab) {
  if (A.est.tried) return;
  specest_require_one_rank();
  SpecEst e;
  e.tried = true;
  const i64 n = A.n, nvec = nb.n_vec();
  if (n <= 0 || !spmv_supports_preconditioner_product()) {   // (no polynomial loop to admit anything to)
    A.est = e;
    return;
  }
  PG_REQUIRE(n == nb.n_own && nvec >= n, "spectral estimate: the matrix and its numbering disagree");
  hipStream_t st = ctx().stream;
  PG_HIP(hipStreamSynchronize(st));
  const auto t0 = std::chrono::steady_clock::now();
  const int m = (int)std::min<i64>(SPECEST_STEPS, n);
  const SeLayout L{m};
  const int G = grid_for(n, BLOCK, 1024);
  DevBuf<double> basis((i64)(m + 1) * nvec), d(L.size()), part((i64)(m + 2) * G);
  basis.zero();
  d.zero();
  double* V = basis.p;
  const double* sc = d.p;   // the scalar block of the shared kernels: only its done flag is used
  auto reduce = [&](int nslots, double* out) {
    hipLaunchKernelGGL(k_gm_reduce, dim3(1), dim3(BLOCK), 0, st, nslots, G, (const double*)part.p, out, sc, 1);
  };
  hipLaunchKernelGGL(k_se_start, dim3(G), dim3(BLOCK), 0, st, n, nvec, V, part.p);
  reduce(1, d.p + L.h2(0));
  hipLaunchKernelGGL(k_se_first, dim3(1), dim3(1), 0, st, L, d.p);
  hipLaunchKernelGGL(k_gm_scale, dim3(G), dim3(BLOCK), 0, st, n, sc, (const double*)d.p, L.invn(), V);
  for (int j = 0; j < m; ++j) {
    double* vj = V + (size_t)j * nvec;
    double* wv = V + (size_t)(j + 1) * nvec;
    spmv_halo(A, nb, slab, vj, wv, st);
    const int k = j + 1;
    for (int pass = 0; pass < 2; ++pass) {
      double* h = d.p + (pass == 0 ? L.h1(0) : L.h2(0));
      for (int k0 = 0; k0 < k; k0 += GM_GRP)
        hipLaunchKernelGGL(k_gm_dots, dim3(G), dim3(BLOCK), 0, st, n, nvec, k0, std::min(GM_GRP, k - k0), (const double*)V,
                           (const double*)wv, sc, part.p);
      reduce(k, h);
      for (int k0 = 0; k0 < k; k0 += GM_GRP) {
        const bool last = pass == 1 && k0 + GM_GRP >= k;
        hipLaunchKernelGGL(k_gm_update, dim3(G), dim3(BLOCK), 0, st, n, nvec, k0, std::min(GM_GRP, k - k0), (const double*)V, wv,
                           (const double*)h, sc, last ? 0 : -1, part.p);
      }
    }
    reduce(1, d.p + L.h2(k));   // ||w||² after both passes
    hipLaunchKernelGGL(k_se_hess, dim3(1), dim3(1), 0, st, L, j, d.p);
    hipLaunchKernelGGL(k_gm_scale, dim3(G), dim3(BLOCK), 0, st, n, sc, (const double*)d.p, L.invn(), wv);
  }
  PG_HIP(hipGetLastError());
  std::vector<double> hd((size_t)L.size());
  d.download(hd.data(), L.size());   // (synchronises)
  const int k = std::max(0, std::min(m, (int)hd[L.steps()]));
  e.steps = k;
  e.H.assign((size_t)(k + 1) * std::max(k, 1), 0.0);
  for (int j = 0; j < k; ++j)
    for (int i = 0; i <= std::min(j + 1, k); ++i) e.H[(size_t)j * (k + 1) + i] = hd[L.H(i, j)];
  if (k > 0) {
    std::vector<double> wr(k), wi(k);
    PG_REQUIRE(pghost::hessenberg_eigenvalues(k, e.H.data(), k + 1, wr.data(), wi.data()),
               "spectral estimate: the QR iteration on the Hessenberg matrix did not converge");
    e.re_min = e.re_max = wr[0];
    for (int i = 0; i < k; ++i) {
      PG_REQUIRE(std::isfinite(wr[i]) && std::isfinite(wi[i]), "spectral estimate: a Ritz value is not finite");
      e.g_ritz = std::max(e.g_ritz, std::hypot(wr[i] - 1.0, wi[i]));
      e.re_min = std::min(e.re_min, wr[i]);
      e.re_max = std::max(e.re_max, wr[i]);
      e.im_max = std::max(e.im_max, std::fabs(wi[i]));
    }
    e.g_used = e.g_ritz + SPECEST_MARGIN;
    e.admitted = e.g_used < SPECEST_BOUND;
  }
  e.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (config().debug)
    fprintf(stderr, "[pg_specest] %d Arnoldi steps on %lld rows: Ritz values in [%.4f, %.4f], |Im| <= %.2e, g_ritz %.4f + margin %.4f = %.4f "
            "(Gershgorin %.2f) => polynomial preconditioner %s; %.2f ms\n", k, (long long)n, e.re_min, e.re_max, e.im_max, e.g_ritz,
            SPECEST_MARGIN, e.g_used, A.gersh, e.admitted ? "admitted" : "not admitted", e.ms);
  A.est = std::move(e);
}

}  // namespace pg
