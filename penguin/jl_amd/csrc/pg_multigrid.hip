// pg_multigrid.hip -- geometric-aggregation multigrid V-cycle: the right preconditioner M⁻¹ of the BiCGStab driver for the
// systems without a mass term (steady diffusion, the Poisson solve of StreamVorticity), whose plain iteration count grows with
// the side of the grid and which Gershgorin keeps away from the Chebyshev polynomial (DESIGN.md "Multigrid").
//
//   level 0        Â = B⁻¹ S A S, the matrix the Krylov loop iterates on (unit diagonal), borrowed.  Under a Dirichlet interface
//                  B⁻¹ only removes the same-cell γ entry of the ω rows of cut cells (their γ rows are rows of the identity)
//   aggregates     unknown of kind k in padded cell (i, j, k3) -> (k, i >> 1, j >> 1, k3 >> 1); coarse unknowns numbered kind-major,
//                  then by coarse cell, dimension 0 fastest (flag + scan, the layout of Numbering).  Cell rule (MG_RULE_CELL,
//                  PG_PRECOND_MG_CELL): level 0 -> 1 drops the kind -- every unknown of the 2 x 2 (x 2) cells shares one coarse
//                  unknown, <= 8 K children in slot parity + 8 kind; the levels below have one kind and coarsen as above
//   transfers      P̂_0 has 1 / s_i at fine unknown i (piecewise constant in the unknowns of A: P̂ᵀ S A S P̂ = Pᵀ A P); 0 / 1 below
//   operators      Galerkin, A_(l+1) = P_lᵀ A_l P_l, one thread per coarse row gathering its <= 8 (cell rule, level 1: 8 K) fine rows
//   smoother       damped Jacobi, ω = 0.7, 2 + 2 sweeps (the first from zero: a pointwise scale)
//   correction     x += 1.8 P e_c, fused with the prolongation; the residual is fused with the restriction, written as a gather
//                  over coarse rows: no atomics anywhere, an application is bitwise reproducible.  (Level 0 above the tail:
//                  the marching-unit SpMV forms the residual and the gather restricts that vector -- measured)
//   last level     <= 200 rows, dense inverse from the host (pg_host_algos.h), one matrix-vector product
//   fused tail     the levels [tail0, L) run in ONE launch by ONE workgroup with their vectors in LDS (k_mg_tail): they are
//                  latency-bound -- a few hundred rows and seven launches each otherwise
#include "pg_multigrid.h"

#include "pg_host_algos.h"
#include "pg_scan.h"
#include "pg_spmv.h"

using namespace pg;

namespace {

constexpr int MG_BLOCK = 256;
constexpr int MG_TAIL_BLOCK = 1024;

struct MgSegs {
  int K;
  i64 off_own[MAX_KINDS];
};

struct MgGrid {
  i64 ext0, ext1, cext0, cext1;   // padded extents of the fine and of the coarse cell grid (dimensions 0, 1)
  i64 M, Mc;                      // cells of the two grids
};

// ---- set-up ---------------------------------------------------------------------------------------------------------
// slot0 == nullptr: the kind rule, key = kind * M + cell.  Otherwise the cell rule: the kind-free key, and the kind's offset
// 8 * kind into the child table of the coarse unknown the cell's unknowns share (k_mg_agg adds the parity of the cell).
__global__ void k_mg_key0(i64 n, MgSegs seg, const int* __restrict__ row_cell, i64 M, const double* __restrict__ ds, int* __restrict__ key,
                          double* __restrict__ pw, unsigned char* __restrict__ slot0) {
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) {
    int k = 0;
    while (k + 1 < seg.K && r >= seg.off_own[k + 1]) ++k;
    if (slot0) {
      key[r] = row_cell[r];
      slot0[r] = (unsigned char)(8 * k);
    } else {
      key[r] = (int)((i64)k * M + row_cell[r]);
    }
    pw[r] = 1.0 / ds[r];
  }
}

// *err = 1 where a row of Â has no positive diagonal entry (the flag is read and checked after every pass: one cause at a time)
__global__ void k_mg_check_diag(i64 n, const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                                int* __restrict__ err) {
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) {
    double d = 0.0;
    for (int e = rowptr[r]; e < rowptr[r + 1]; ++e)
      if (col[e] == r) d += val[e];
    if (!(d > 0.0)) *err = 1;   // (every writer stores the same value)
  }
}

__device__ inline i64 mg_coarse_key(const MgGrid& g, int key, int* slot) {
  const i64 kind = key / g.M, cell = key % g.M;
  const i64 i = cell % g.ext0, j = (cell / g.ext0) % g.ext1, k = cell / (g.ext0 * g.ext1);
  *slot = (int)((i & 1) | ((j & 1) << 1) | ((k & 1) << 2));
  return kind * g.Mc + (i >> 1) + (j >> 1) * g.cext0 + (k >> 1) * g.cext0 * g.cext1;
}

__global__ void k_mg_flag(i64 n, MgGrid g, const int* __restrict__ key, unsigned char* __restrict__ flag) {
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) {
    int slot;
    flag[mg_coarse_key(g, key[r], &slot)] = 1;   // (every writer stores the same value)
  }
}

// idx: exclusive scan of the flags = the coarse numbering.  The <= cw fine rows of a coarse row have distinct slots (slot0, cell
// rule between levels 0 and 1: the offset of the row's kind; nullptr elsewhere, cw = 8).
__global__ void k_mg_agg(i64 n, MgGrid g, const int* __restrict__ key, const int* __restrict__ idx, const unsigned char* __restrict__ slot0,
                         int cw, int* __restrict__ agg, int* __restrict__ child, int* __restrict__ keyc) {
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) {
    int slot;
    const i64 ck = mg_coarse_key(g, key[r], &slot);
    if (slot0) slot += slot0[r];
    const int a = idx[ck];
    agg[r] = a;
    child[(i64)a * cw + slot] = (int)r;
    keyc[a] = (int)ck;   // (the same value from every child)
  }
}

// Row c of Pᵀ A P, one thread per coarse row: the entries of its fine rows, in slot and CSR order, merged into a list kept
// sorted by coarse column.  FILL = false counts the row (cnt[c]); FILL = true writes it at crowptr[c] and 1 / its diagonal.
// *err = 2: a row longer than MG_MAX_ROW (count pass); = 4: a coarse diagonal that is not positive (fill pass).
template <bool FILL>
__global__ void k_mg_galerkin(i64 nc, const int* __restrict__ child, int cw, const int* __restrict__ rowptr, const int* __restrict__ col,
                              const double* __restrict__ val, const int* __restrict__ agg, const double* __restrict__ pw,
                              int* __restrict__ cnt, const int* __restrict__ crowptr, int* __restrict__ ccol, double* __restrict__ cval,
                              double* __restrict__ dinv, int* __restrict__ err) {
  for (i64 c = blockIdx.x * (i64)blockDim.x + threadIdx.x; c < nc; c += (i64)gridDim.x * blockDim.x) {
    int cols[MG_MAX_ROW];
    double vals[FILL ? MG_MAX_ROW : 1];
    int m = 0;
    bool over = false;
    for (int s = 0; s < cw; ++s) {
      const int i = child[c * cw + s];
      if (i < 0) continue;
      const double wi = pw ? pw[i] : 1.0;
      for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) {
        const int j = col[e];
        const int cj = agg[j];
        int pos = 0;
        while (pos < m && cols[pos] < cj) ++pos;
        if (pos == m || cols[pos] != cj) {
          if (m >= MG_MAX_ROW) { over = true; continue; }
          for (int q = m; q > pos; --q) {
            cols[q] = cols[q - 1];
            if (FILL) vals[q] = vals[q - 1];
          }
          cols[pos] = cj;
          if (FILL) vals[pos] = 0.0;
          ++m;
        }
        if (FILL) vals[pos] += (wi * val[e]) * (pw ? pw[j] : 1.0);
      }
    }
    if (over) *err = 2;
    if (!FILL) {
      cnt[c] = m;
    } else {
      const int base = crowptr[c];
      double d = 0.0;
      for (int q = 0; q < m; ++q) {
        ccol[base + q] = cols[q];
        cval[base + q] = vals[q];
        if (cols[q] == c) d = vals[q];
      }
      if (!(d > 0.0)) *err = 4;
      dinv[c] = 1.0 / d;
    }
  }
}

// ---- one application ------------------------------------------------------------------------------------------------
__device__ inline double mg_row_dot(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val, int i,
                                    const double* x) {
  double s = 0.0;
  for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) s += val[e] * x[col[e]];
  return s;
}

// the four pointwise formulas of the cycle, shared by the per-level kernels and the fused tail
__device__ inline double mg_scale(const double* dinv, const double* r, int i) { return MG_OMEGA * (dinv ? dinv[i] : 1.0) * r[i]; }
__device__ inline double mg_jacobi(const int* rowptr, const int* col, const double* val, const double* dinv, const double* r,
                                   const double* x, int i) {
  return x[i] + MG_OMEGA * (dinv ? dinv[i] : 1.0) * (r[i] - mg_row_dot(rowptr, col, val, i, x));
}
__device__ inline double mg_restrict(const int* child, int cw, const int* rowptr, const int* col, const double* val, const double* pw,
                                     const double* r, const double* x, int c) {
  double acc = 0.0;
  for (int s = 0; s < cw; ++s) {
    const int i = child[(i64)c * cw + s];
    if (i >= 0) acc += (pw ? pw[i] : 1.0) * (r[i] - mg_row_dot(rowptr, col, val, i, x));
  }
  return acc;
}
__device__ inline double mg_prolong(const int* agg, const double* pw, const double* ec, double xi, int i) {
  return xi + MG_OVER * ((pw ? pw[i] : 1.0) * ec[agg[i]]);
}

__global__ __launch_bounds__(MG_BLOCK) void k_mg_scale(i64 n, const double* __restrict__ dinv, const double* __restrict__ r,
                                                       double* __restrict__ x, const double* __restrict__ sc) {
  if (sc && sc[S_DONE] != 0.0) return;
  for (i64 i = blockIdx.x * (i64)MG_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * MG_BLOCK) x[i] = mg_scale(dinv, r, (int)i);
}

__global__ __launch_bounds__(MG_BLOCK) void k_mg_jacobi(i64 n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        const double* __restrict__ val, const double* __restrict__ dinv,
                                                        const double* __restrict__ r, const double* __restrict__ xin,
                                                        double* __restrict__ xout, const double* __restrict__ sc) {
  if (sc && sc[S_DONE] != 0.0) return;
  for (i64 i = blockIdx.x * (i64)MG_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * MG_BLOCK)
    xout[i] = mg_jacobi(rowptr, col, val, dinv, r, xin, (int)i);
}

// r_c = Pᵀ (r - A x): the residual fused with the restriction, a gather over coarse rows
__global__ __launch_bounds__(MG_BLOCK) void k_mg_restrict(i64 nc, const int* __restrict__ child, int cw, const int* __restrict__ rowptr,
                                                          const int* __restrict__ col, const double* __restrict__ val,
                                                          const double* __restrict__ pw, const double* __restrict__ r,
                                                          const double* __restrict__ x, double* __restrict__ rc,
                                                          const double* __restrict__ sc) {
  if (sc && sc[S_DONE] != 0.0) return;
  for (i64 c = blockIdx.x * (i64)MG_BLOCK + threadIdx.x; c < nc; c += (i64)gridDim.x * MG_BLOCK)
    rc[c] = mg_restrict(child, cw, rowptr, col, val, pw, r, x, (int)c);
}

// r_c = Pᵀ res with the residual already formed (level 0, where the marching-unit SpMV forms it: see mg_apply)
__global__ __launch_bounds__(MG_BLOCK) void k_mg_restrict_vec(i64 nc, const int* __restrict__ child, int cw, const double* __restrict__ pw,
                                                              const double* __restrict__ res, double* __restrict__ rc,
                                                              const double* __restrict__ sc) {
  if (sc && sc[S_DONE] != 0.0) return;
  for (i64 c = blockIdx.x * (i64)MG_BLOCK + threadIdx.x; c < nc; c += (i64)gridDim.x * MG_BLOCK) {
    double acc = 0.0;
    for (int s = 0; s < cw; ++s) {
      const int i = child[c * cw + s];
      if (i >= 0) acc += (pw ? pw[i] : 1.0) * res[i];
    }
    rc[c] = acc;
  }
}

// x += 1.8 P e_c: the prolongation fused with the correction
__global__ __launch_bounds__(MG_BLOCK) void k_mg_prolong(i64 n, const int* __restrict__ agg, const double* __restrict__ pw,
                                                         const double* __restrict__ ec, double* __restrict__ x,
                                                         const double* __restrict__ sc) {
  if (sc && sc[S_DONE] != 0.0) return;
  for (i64 i = blockIdx.x * (i64)MG_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * MG_BLOCK) x[i] = mg_prolong(agg, pw, ec, x[i], (int)i);
}

// ---- the fused tail ---------------------------------------------------------------------------------------------------
// Levels [tail0, L) in one launch by one workgroup.  LDS: r, xa, xb of every level but the last (off, off + n, off + 2n) and
// r, x of the last; the matrices are read from memory (they sit in L2 after the first application).  Every phase is a loop
// over the rows of one level strided by the workgroup, closed by a barrier.
struct MgTailLevel {
  int n, off;
  const int* rowptr;
  const int* col;
  const double* val;
  const double* dinv;
  const double* pw;
  const int* agg;
  const int* child;   // cw per row of the next level
  int cw;
};
struct MgTailArgs {
  int nl;
  MgTailLevel L[MG_MAX_LEVELS];
  const double* invT;   // inverse of the last level, column-major: thread i reads invT[j n + i] (coalesced)
};

__global__ __launch_bounds__(MG_TAIL_BLOCK) void k_mg_tail(MgTailArgs a, const double* __restrict__ rin, double* __restrict__ xout,
                                                          const double* __restrict__ sc) {
  extern __shared__ double sm[];
  if (sc && sc[S_DONE] != 0.0) return;   // (the same verdict in every thread: no barrier is skipped by some)
  const int tid = threadIdx.x, nt = blockDim.x;
  const int last = a.nl - 1;
  for (int i = tid; i < a.L[0].n; i += nt) sm[a.L[0].off + i] = rin[i];
  __syncthreads();
  for (int l = 0; l < last; ++l) {
    const MgTailLevel& v = a.L[l];
    double* r = sm + v.off;
    double* xa = r + v.n;
    double* xb = xa + v.n;
    for (int i = tid; i < v.n; i += nt) xa[i] = mg_scale(v.dinv, r, i);
    __syncthreads();
    for (int i = tid; i < v.n; i += nt) xb[i] = mg_jacobi(v.rowptr, v.col, v.val, v.dinv, r, xa, i);
    __syncthreads();
    const MgTailLevel& c = a.L[l + 1];
    double* rc = sm + c.off;
    for (int q = tid; q < c.n; q += nt) rc[q] = mg_restrict(v.child, v.cw, v.rowptr, v.col, v.val, v.pw, r, xb, q);
    __syncthreads();
  }
  {
    const MgTailLevel& v = a.L[last];
    const double* r = sm + v.off;
    double* x = sm + v.off + v.n;
    for (int i = tid; i < v.n; i += nt) {
      double s = 0.0;
      for (int j = 0; j < v.n; ++j) s += a.invT[(size_t)j * v.n + i] * r[j];
      x[i] = s;
    }
    __syncthreads();
  }
  for (int l = last - 1; l >= 0; --l) {
    const MgTailLevel& v = a.L[l];
    const MgTailLevel& c = a.L[l + 1];
    const double* r = sm + v.off;
    double* xa = sm + v.off + v.n;
    double* xb = xa + v.n;
    const double* ec = sm + c.off + (l + 1 == last ? c.n : 2 * c.n);
    for (int i = tid; i < v.n; i += nt) xb[i] = mg_prolong(v.agg, v.pw, ec, xb[i], i);
    __syncthreads();
    for (int i = tid; i < v.n; i += nt) xa[i] = mg_jacobi(v.rowptr, v.col, v.val, v.dinv, r, xb, i);
    __syncthreads();
    for (int i = tid; i < v.n; i += nt) xb[i] = mg_jacobi(v.rowptr, v.col, v.val, v.dinv, r, xa, i);
    __syncthreads();
  }
  const double* sol = sm + a.L[0].off + (last == 0 ? a.L[0].n : 2 * a.L[0].n);
  for (int i = tid; i < a.L[0].n; i += nt) xout[i] = sol[i];
}

int mg_grid(i64 n) { return grid_for(n, MG_BLOCK); }

void check_err(const DevBuf<int>& err, const char* where) {
  int h = 0;
  err.download(&h, 1);
  PG_REQUIRE(h != 1, "multigrid preconditioner refused: a row of the system has no positive diagonal entry");
  PG_REQUIRE(h != 2, std::string("multigrid set-up: a coarse row has more than ") + std::to_string(MG_MAX_ROW) + " entries (" + where + ")");
  PG_REQUIRE(h != 4, std::string("multigrid set-up: a coarse diagonal entry is not positive (") + where + ")");
}

}  // namespace

namespace pg {

void mg_require_one_rank(MgRule rule) {
  Context& cx = ctx();
  PG_REQUIRE(cx.nranks == 1 && !cx.comm && !cx.local, std::string("multigrid preconditioner (precond = ") + mg_precond_name(rule) +
                                                          ") refused: it runs on one rank only (virtual ranks included)");
}

void mg_require_one_rank_of(int precond) {
  Context& cx = ctx();
  PG_REQUIRE(cx.nranks == 1 && !cx.comm && !cx.local, std::string("multigrid preconditioner (precond = ") + mg_precond_name_of(precond) +
                                                          ") refused: it runs on one rank only (virtual ranks included)");
}

void mg_build(MgHierarchy& H, const CsrMatrix& A, const Numbering& nb, const Slab& slab, MgRule rule) {
  Context& cx = ctx();
  hipStream_t st = cx.stream;
  mg_require_one_rank(rule);
  PG_REQUIRE(nb.n_ghost == 0 && slab.s0 == 0 && slab.Mloc() == slab.M, "multigrid set-up: the numbering of one rank (no ghosts, every plane) is expected");
  // (the cell rule merges whatever kinds a cell has: the child table between levels 0 and 1 is 8 K wide, K = 4 on a diphasic
  //  system -- slot = cell parity + 8 kind -- and every kernel reads the width from the level.  The callers decide which systems
  //  come here: pg_solver.hip mg_conditions keeps diphasic systems away from PG_PRECOND_MG and PG_PRECOND_MG_CELL.)
  PG_REQUIRE(nb.K == 2 || (rule == MG_RULE_CELL && nb.K == 4),
             "multigrid preconditioner refused: a monophasic system (two kinds of unknowns) is expected");
  static_assert(8 * MAX_KINDS <= 255, "k_mg_key0 keeps 8 * kind in a byte");
  PG_REQUIRE(A.n > 0 && A.n == nb.n_own, "multigrid preconditioner refused: empty system");
  PG_REQUIRE((i64)nb.K * slab.M < (i64)2000000000, "multigrid preconditioner: grid too large for 32-bit cell keys");
  PG_HIP(hipStreamSynchronize(st));
  const auto t0 = std::chrono::steady_clock::now();
  H.lev.clear();
  H.bytes = 0;
  H.rule = rule;
  H.matrix = nullptr;
  const bool cells = rule == MG_RULE_CELL;
  DevBuf<int> err(1);
  err.zero();
  DevBuf<unsigned char> slot0;   // cell rule: 8 * kind of every row of level 0 (set-up only)

  {
    std::unique_ptr<MgLevel> l0(new MgLevel());
    l0->n = A.n; l0->nnz = A.nnz;
    l0->K = cells ? 1 : nb.K;
    l0->cw = cells ? 8 * nb.K : 8;
    if (cells) slot0.alloc(A.n);
    for (int d = 0; d < 3; ++d) l0->ext[d] = slab.ext[d];
    l0->rowptr = A.rowptr.p; l0->col = A.col.p; l0->val = A.val.p;
    l0->key.alloc(A.n);
    l0->pw.alloc(A.n);
    MgSegs seg;
    seg.K = nb.K;
    for (int k = 0; k < MAX_KINDS; ++k) seg.off_own[k] = nb.off_own[k];
    hipLaunchKernelGGL(k_mg_key0, dim3(mg_grid(A.n)), dim3(MG_BLOCK), 0, st, A.n, seg, (const int*)nb.row_cell.p, slab.M,
                       (const double*)A.ds.p, l0->key.p, l0->pw.p, cells ? slot0.p : (unsigned char*)nullptr);
    hipLaunchKernelGGL(k_mg_check_diag, dim3(mg_grid(A.n)), dim3(MG_BLOCK), 0, st, A.n, l0->rowptr, l0->col, l0->val, err.p);
    PG_HIP(hipGetLastError());
    check_err(err, "level 0");
    H.bytes += A.n * (i64)(sizeof(int) + sizeof(double));
    H.lev.push_back(std::move(l0));
  }

  while (H.lev.back()->n > MG_COARSEST_ROWS && (int)H.lev.size() < MG_MAX_LEVELS) {
    MgLevel& f = *H.lev.back();
    std::unique_ptr<MgLevel> c(new MgLevel());
    c->K = f.K;
    for (int d = 0; d < 3; ++d) c->ext[d] = (f.ext[d] + 1) >> 1;
    MgGrid g;
    g.ext0 = f.ext[0]; g.ext1 = f.ext[1]; g.cext0 = c->ext[0]; g.cext1 = c->ext[1];
    g.M = f.ext[0] * f.ext[1] * f.ext[2];
    g.Mc = c->ext[0] * c->ext[1] * c->ext[2];
    const i64 nkeys = (i64)f.K * g.Mc;
    DevBuf<unsigned char> flag(nkeys);
    DevBuf<int> idx(nkeys), total(1);
    flag.zero();
    hipLaunchKernelGGL(k_mg_flag, dim3(mg_grid(f.n)), dim3(MG_BLOCK), 0, st, f.n, g, (const int*)f.key.p, flag.p);
    PG_HIP(hipGetLastError());
    scan_exclusive<unsigned char>(flag.p, idx.p, nkeys, total.p, st);
    int nc = 0;
    total.download(&nc, 1);
    PG_REQUIRE(nc > 0 && nc < f.n, "multigrid set-up: the aggregation does not coarsen");
    c->n = nc;
    const bool first = H.lev.size() == 1;
    const int cw = f.cw;
    f.agg.alloc(f.n);
    f.child.alloc((i64)nc * cw);
    c->key.alloc(nc);
    PG_HIP(hipMemsetAsync(f.child.p, 0xFF, sizeof(int) * (size_t)nc * cw, st));
    hipLaunchKernelGGL(k_mg_agg, dim3(mg_grid(f.n)), dim3(MG_BLOCK), 0, st, f.n, g, (const int*)f.key.p, (const int*)idx.p,
                       (const unsigned char*)(cells && first ? slot0.p : nullptr), cw, f.agg.p, f.child.p, c->key.p);
    PG_HIP(hipGetLastError());
    // Galerkin product: count, scan, fill
    DevBuf<int> cnt(nc);
    c->o_rowptr.alloc(nc + 1);
    c->dinv.alloc(nc);
    const double* pw = f.pw.n > 0 ? f.pw.p : nullptr;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mg_galerkin<false>), dim3(mg_grid(nc)), dim3(MG_BLOCK), 0, st, (i64)nc, (const int*)f.child.p,
                       cw, f.rowptr, f.col, f.val, (const int*)f.agg.p, pw, cnt.p, (const int*)nullptr, (int*)nullptr, (double*)nullptr,
                       (double*)nullptr, err.p);
    PG_HIP(hipGetLastError());
    scan_exclusive<int>(cnt.p, c->o_rowptr.p, nc, c->o_rowptr.p + nc, st);
    int nnz = 0;
    c->o_rowptr.download(&nnz, 1, nc);
    const std::string where = "level " + std::to_string(H.lev.size());
    check_err(err, (where + ", row count").c_str());
    PG_REQUIRE(nnz > 0, "multigrid set-up: empty coarse matrix");
    c->nnz = nnz;
    c->o_col.alloc(nnz);
    c->o_val.alloc(nnz);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mg_galerkin<true>), dim3(mg_grid(nc)), dim3(MG_BLOCK), 0, st, (i64)nc, (const int*)f.child.p,
                       cw, f.rowptr, f.col, f.val, (const int*)f.agg.p, pw, (int*)nullptr, (const int*)c->o_rowptr.p, c->o_col.p, c->o_val.p,
                       c->dinv.p, err.p);
    PG_HIP(hipGetLastError());
    check_err(err, where.c_str());
    c->rowptr = c->o_rowptr.p; c->col = c->o_col.p; c->val = c->o_val.p;
    H.bytes += f.n * (i64)sizeof(int) + (i64)nc * (cw * sizeof(int) + sizeof(int) + sizeof(int) + sizeof(double)) +
               (i64)nnz * (sizeof(int) + sizeof(double));
    H.lev.push_back(std::move(c));
  }
  const int L = (int)H.lev.size();
  PG_REQUIRE(H.lev.back()->n <= MG_COARSEST_ROWS, "multigrid set-up: too many levels");

  {  // the last level, inverted on the host
    MgLevel& c = *H.lev.back();
    const int n = (int)c.n;
    std::vector<int> rp(n + 1), cc(c.nnz);
    std::vector<double> vv(c.nnz), dense((size_t)n * n, 0.0), inv((size_t)n * n), invT((size_t)n * n);
    PG_HIP(hipMemcpyAsync(rp.data(), c.rowptr, sizeof(int) * (size_t)(n + 1), hipMemcpyDeviceToHost, st));
    PG_HIP(hipMemcpyAsync(cc.data(), c.col, sizeof(int) * (size_t)c.nnz, hipMemcpyDeviceToHost, st));
    PG_HIP(hipMemcpyAsync(vv.data(), c.val, sizeof(double) * (size_t)c.nnz, hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i)
      for (int e = rp[i]; e < rp[i + 1]; ++e) {
        PG_REQUIRE(cc[e] >= 0 && cc[e] < n, "multigrid set-up: column out of range on the last level");
        dense[(size_t)i * n + cc[e]] += vv[e];
      }
    PG_REQUIRE(pghost::mg_dense_inverse(n, dense.data(), inv.data()), "multigrid preconditioner refused: the coarsest system is singular");
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) invT[(size_t)j * n + i] = inv[(size_t)i * n + j];
    H.inv.alloc((i64)n * n);
    H.inv.upload(invT.data(), (i64)n * n);
    H.bytes += (i64)n * n * (i64)sizeof(double);
  }

  {  // the tail, and the work vectors of the levels above it
    i64 rows[MG_MAX_LEVELS];
    for (int l = 0; l < L; ++l) rows[l] = H.lev[l]->n;
    H.tail0 = pghost::mg_plan_tail(rows, L, config().mg_tail_rows, MG_TAIL_DOUBLES);
    for (int l = 0; l <= H.tail0 && l < L; ++l) {
      MgLevel& v = *H.lev[l];
      if (l < H.tail0) { v.xa.alloc(v.n); H.bytes += v.n * (i64)sizeof(double); }
      if (l > 0) { v.r.alloc(v.n); v.xb.alloc(v.n); H.bytes += 2 * v.n * (i64)sizeof(double); }
    }
  }
  PG_HIP(hipStreamSynchronize(st));
  H.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  H.matrix = &A;
}

void mg_apply(MgHierarchy& H, const CsrMatrix& A, const Numbering& nb, const Slab& slab, double* in, double* out, const double* sc,
              hipStream_t st) {
  const int L = (int)H.lev.size(), t = H.tail0;
  PG_REQUIRE(L > 0 && H.matrix == &A, "multigrid: the hierarchy belongs to another matrix");
  auto R = [&](int l) { return l == 0 ? in : H.lev[l]->r.p; };
  auto XB = [&](int l) { return l == 0 ? out : H.lev[l]->xb.p; };
  const bool march = spmv_supports_preconditioner_product();
  const int G0 = spmv_default_grid(A.n);
  // x_out = x_in + ω D⁻¹ (r - A x_in); on level 0 (unit diagonal) this is the SpMV's Horner step, y = ω r + x - ω Â x
  auto jacobi = [&](int l, double* r, double* xin, double* xout) {
    const MgLevel& v = *H.lev[l];
    if (l == 0 && march) {
      FinArgs f{nullptr, nullptr, PH_NONE, 0, 0, nullptr};
      f.pc0 = 1.0; f.pc1 = -MG_OMEGA; f.pc2 = MG_OMEGA; f.base = r;
      spmv_with_halo(8, A, nb, slab, xin, xout, nullptr, nullptr, sc, G0, st, &f);
    } else {
      hipLaunchKernelGGL(k_mg_jacobi, dim3(mg_grid(v.n)), dim3(MG_BLOCK), 0, st, v.n, v.rowptr, v.col, v.val,
                         (const double*)(v.dinv.n > 0 ? v.dinv.p : nullptr), (const double*)r, (const double*)xin, xout, sc);
    }
  };
  for (int l = 0; l < t; ++l) {
    MgLevel& v = *H.lev[l];
    const MgLevel& c = *H.lev[l + 1];
    const double* dinv = v.dinv.n > 0 ? v.dinv.p : nullptr;
    if (l == 0 && march) {
      // Level 0 through the marching-unit SpMV (mode 8, y = pc2 base + pc0 x + pc1 Â x), three passes over Â instead of a
      // scale, a sweep and a thread-per-coarse-row CSR walk (measured at 1024², profiles/: 5.5 + 9.1 + 57.5 us before):
      //   both pre-sweeps in one launch, x = base = r:   x2 = ω r + (ω r - ω² Â r)
      //   the residual, base = r:                        res = r - Â x2     (into xa, which is free until the post-sweeps)
      //   the restriction of that vector, a gather over coarse rows
      FinArgs f{nullptr, nullptr, PH_NONE, 0, 0, nullptr};
      f.pc0 = MG_OMEGA; f.pc1 = -MG_OMEGA * MG_OMEGA; f.pc2 = MG_OMEGA; f.base = in;
      spmv_with_halo(8, A, nb, slab, in, out, nullptr, nullptr, sc, G0, st, &f);
      FinArgs g{nullptr, nullptr, PH_NONE, 0, 0, nullptr};
      g.pc0 = 0.0; g.pc1 = -1.0; g.pc2 = 1.0; g.base = in;
      spmv_with_halo(8, A, nb, slab, out, v.xa.p, nullptr, nullptr, sc, G0, st, &g);
      hipLaunchKernelGGL(k_mg_restrict_vec, dim3(mg_grid(c.n)), dim3(MG_BLOCK), 0, st, c.n, (const int*)v.child.p, v.cw,
                         (const double*)(v.pw.n > 0 ? v.pw.p : nullptr), (const double*)v.xa.p, R(1), sc);
      continue;
    }
    hipLaunchKernelGGL(k_mg_scale, dim3(mg_grid(v.n)), dim3(MG_BLOCK), 0, st, v.n, dinv, (const double*)R(l), v.xa.p, sc);
    jacobi(l, R(l), v.xa.p, XB(l));
    hipLaunchKernelGGL(k_mg_restrict, dim3(mg_grid(c.n)), dim3(MG_BLOCK), 0, st, c.n, (const int*)v.child.p, v.cw, v.rowptr, v.col, v.val,
                       (const double*)(v.pw.n > 0 ? v.pw.p : nullptr), (const double*)R(l), (const double*)XB(l), R(l + 1), sc);
  }
  {
    MgTailArgs a;
    std::memset(&a, 0, sizeof(a));
    a.nl = L - t;
    int off = 0;
    for (int l = t; l < L; ++l) {
      const MgLevel& v = *H.lev[l];
      MgTailLevel& q = a.L[l - t];
      q.n = (int)v.n; q.off = off;
      q.rowptr = v.rowptr; q.col = v.col; q.val = v.val;
      q.dinv = v.dinv.n > 0 ? v.dinv.p : nullptr;
      q.pw = v.pw.n > 0 ? v.pw.p : nullptr;
      q.agg = v.agg.p; q.child = v.child.p; q.cw = v.cw;
      off += (l == L - 1 ? 2 : 3) * (int)v.n;
    }
    a.invT = H.inv.p;
    PG_REQUIRE(off <= MG_TAIL_DOUBLES, "multigrid: the fused tail does not fit the LDS");
    hipLaunchKernelGGL(k_mg_tail, dim3(1), dim3(MG_TAIL_BLOCK), sizeof(double) * (size_t)off, st, a, (const double*)R(t), XB(t), sc);
  }
  for (int l = t - 1; l >= 0; --l) {
    MgLevel& v = *H.lev[l];
    hipLaunchKernelGGL(k_mg_prolong, dim3(mg_grid(v.n)), dim3(MG_BLOCK), 0, st, v.n, (const int*)v.agg.p,
                       (const double*)(v.pw.n > 0 ? v.pw.p : nullptr), (const double*)XB(l + 1), XB(l), sc);
    jacobi(l, R(l), XB(l), v.xa.p);
    jacobi(l, R(l), v.xa.p, XB(l));
  }
  PG_HIP(hipGetLastError());
}

}  // namespace pg
