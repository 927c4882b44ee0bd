// pg_spmv.hip -- the dominant kernel of the path: y = A x for the reduced cut-cell system
// (fp64 values, int32 column indices; rows in box order, 1 / 2N+1 / up to 2(2N+1) entries).
// Replaces the single-threaded CSC mul! inside IterativeSolvers (src/solver.jl:178-181).  Roofline: HBM.
//
// Three kernels, in the order they were written (PG_SPMV_VARIANT; profiles/r01_spmv_sweeps.txt, r01_spmv_slices.txt):
//
//   1    k_spmv      plain CSR, a block of 256 rows staged through LDS, two block barriers per chunk (2.0 TB/s).
//
//   2|38 k_spmv_cw   plain CSR (12 nnz + 20 n bytes), the best a CSR stream can do here: 61 % of 8 TB/s back-to-back.
//        The rows are cut once per matrix into CHUNKS of <= 64 consecutive rows and <= 508 entries (chunk_desc, the
//        row-block idea of CSR-Adaptive).  One WAVE owns one chunk per iteration: it streams the chunk's contiguous
//        val/col range with coalesced 16-byte loads into its PRIVATE slice of LDS -- no block barrier anywhere -- and
//        lane l walks row l out of LDS: column indices, all x gathers issued together, FMAs.  Everything inside an
//        iteration is branch-free with a FIXED number of vector-memory operations (clamped indices + selects):
//        hipcc puts every predicated load in its own basic block behind `s_waitcnt vmcnt(0)`, and only when every
//        path issues the same number of loads can it emit counted waits.  The chunk descriptor (a scalar load the
//        stream addresses depend on) is fetched two chunks ahead.  +4 = non-temporal hint on the matrix stream.
//
//   70   k_spmv_s    stencil slices (default): see "stencil slices" below.  0.25 GB instead of 0.99 GB at 512^3.
//
// The dots that follow an SpMV in BiCGStab / CG are fused into the epilogue (one partial per block, summed in a fixed
// order: deterministic); the slice kernel's last-arriving block can also evaluate the scalar phase (pg_spmv.h).  The slice
// kernel has one more epilogue, y = pc2 base + pc0 x + pc1 A x: a Horner step of the polynomial preconditioner of
// pg_krylov.hip (launch mode 8).
#include <algorithm>
#include <cstdlib>
#include <thread>
#include <type_traits>
#include <vector>

#include "pg_host_algos.h"
#include "pg_krylov.h"
#include "pg_spmv.h"

namespace pg {
namespace {

// ---- variant 1 ---------------------------------------------------------------------------------------
constexpr int SPMV_ROWS = 256;          // rows per block iteration
constexpr int SPMV_LDS_ENTRIES = 3584;  // 256 rows x 14 entries (max row: 2*(2N+1) in 3-D)

template <int MODE>
__global__ __launch_bounds__(BLOCK) void k_spmv(i64 n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                const double* __restrict__ val, const double* __restrict__ x,
                                                double* __restrict__ y, const double* __restrict__ aux,
                                                double* __restrict__ partials, const double* __restrict__ sc) {
  __shared__ double s_val[SPMV_LDS_ENTRIES];
  __shared__ int s_col[SPMV_LDS_ENTRIES];
  __shared__ double s_red[BLOCK / 64];
  if (sc && sc[S_DONE] != 0.0) return;
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  const i64 nchunks = (n + SPMV_ROWS - 1) / SPMV_ROWS;
  for (i64 chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const i64 r0 = chunk * SPMV_ROWS;
    const i64 r1 = r0 + SPMV_ROWS < n ? r0 + SPMV_ROWS : n;
    const int base = rowptr[r0];
    const int cnt = rowptr[r1] - base;
    const i64 r = r0 + threadIdx.x;
    int a = 0, b = 0;
    if (r < r1) {
      a = rowptr[r] - base;
      b = rowptr[r + 1] - base;
    }
    double sum = 0.0;
    if (cnt <= SPMV_LDS_ENTRIES) {
      for (int k = threadIdx.x; k < cnt; k += BLOCK) {
        s_val[k] = val[base + k];
        s_col[k] = col[base + k];
      }
      __syncthreads();
      for (int k = a; k < b; ++k) sum += s_val[k] * x[s_col[k]];
      __syncthreads();
    } else {
      for (int k = a; k < b; ++k) sum += val[base + k] * x[col[base + k]];
    }
    if (r < r1) {
      y[r] = sum;
      if (MODE == 1) acc0 += aux[r] * sum;
      if (MODE >= 2) {
        acc0 += sum * x[r];
        acc1 += sum * sum;
      }
      if (MODE == 3) acc2 += aux[r] * sum;
    }
  }
  if (MODE >= 1) {
    const double t0 = block_sum(acc0, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t0;
  }
  if (MODE >= 2) {
    const double t1 = block_sum(acc1, s_red);
    if (threadIdx.x == 0) partials[gridDim.x + blockIdx.x] = t1;
  }
  if (MODE == 3) {
    const double t2 = block_sum(acc2, s_red);
    if (threadIdx.x == 0) partials[4 * (size_t)gridDim.x + blockIdx.x] = t2;
  }
}

// ---- chunked wave kernel ---------------------------------------------------------------------------------------
constexpr int WUNR = 8;                          // gathers issued together per row (bulk rows: 2N+1 <= 7)
constexpr int GUNR = 4;                          // slice kernel, irregular rows: LDS (value, x) pairs read per round

template <bool NT, class T>
__device__ inline T stream_load(const T* p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}

struct Desc {          // wave-uniform (SGPRs): rows [r0,r1), entries [base,end)
  int r0, base, r1, end;
};

__device__ inline Desc load_desc(const int* __restrict__ cd, i64 ch) {
  // 4 consecutive ints at a wave-uniform address: one s_load_dwordx4 (lgkmcnt, independent of vmcnt)
  const int* p = cd + 2 * ch;
  Desc d;
  d.r0 = p[0]; d.base = p[1]; d.r1 = p[2]; d.end = p[3];
  return d;
}

// ---- chunked CSR kernel, 16-byte stream loads ---------------------------------------------------------------------
// values are read as aligned pairs of doubles starting at base & ~1, columns as aligned quads of ints starting at
// base & ~3 (1 KiB per wave instruction, the widest coalesced access; 6 instead of 16 stream instructions per
// chunk); the LDS image keeps the same shift.  Chunks hold <= 508 entries so the shifted image fits 512 slots;
// CsrMatrix pads val/col by 8 entries so the widened reads stay inside the allocation.
typedef double d2_t __attribute__((ext_vector_type(2)));
typedef int i4_t __attribute__((ext_vector_type(4)));
constexpr int XV_IT = 4, XC_IT = 2;

struct StreamW {
  int ra, rb;
  d2_t v[XV_IT];
  i4_t c[XC_IT];
};

template <bool NT>
__device__ __forceinline__ void stream_issue_w(StreamW& q, const Desc& d, const int* __restrict__ rowptr,
                                      const int* __restrict__ col, const double* __restrict__ val, int lane) {
  const int r = d.r0 + lane;
  q.ra = stream_load<NT>(rowptr + (r < d.r1 ? r : d.r1));
  q.rb = stream_load<NT>(rowptr + (r + 1 < d.r1 ? r + 1 : d.r1));
  const int basev = d.base & ~1, basec = d.base & ~3;
  const int endm1 = d.end > d.base ? d.end - 1 : d.base;
  const int lastp = (endm1 - basev) >> 1, lastq = (endm1 - basec) >> 2;
  const d2_t* vp = reinterpret_cast<const d2_t*>(val + basev);
  const i4_t* cp = reinterpret_cast<const i4_t*>(col + basec);
#pragma unroll
  for (int j = 0; j < XV_IT; ++j) {
    const int k = lane + 64 * j;
    q.v[j] = stream_load<NT>(vp + (k < lastp ? k : lastp));
  }
#pragma unroll
  for (int j = 0; j < XC_IT; ++j) {
    const int k = lane + 64 * j;
    q.c[j] = stream_load<NT>(cp + (k < lastq ? k : lastq));
  }
}

template <int MODE, bool NT>
__global__ __launch_bounds__(BLOCK) void k_spmv_cw(i64 n, i64 nchunks, const int* __restrict__ chunk_desc,
                                                   const int* __restrict__ rowptr, const int* __restrict__ col,
                                                   const double* __restrict__ val, const double* __restrict__ x,
                                                   double* __restrict__ y, const double* __restrict__ aux,
                                                   double* __restrict__ partials, const double* __restrict__ sc) {
  __shared__ __attribute__((aligned(16))) double s_val[BLOCK / 64][512];
  __shared__ __attribute__((aligned(16))) int s_col[BLOCK / 64][512];
  __shared__ double s_red[BLOCK / 64];
  if (sc && sc[S_DONE] != 0.0) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* __restrict__ sv = s_val[wave];
  int* __restrict__ scl = s_col[wave];
  d2_t* sv2 = reinterpret_cast<d2_t*>(sv);
  i4_t* sc4 = reinterpret_cast<i4_t*>(scl);
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  const i64 first = (i64)blockIdx.x * (BLOCK / 64) + wave, wstride = (i64)gridDim.x * (BLOCK / 64);
  const i64 lastc = nchunks - 1;
  StreamW q;
  Desc dcur, dnext;
  if (first < nchunks) {
    dcur = load_desc(chunk_desc, first);
    dnext = load_desc(chunk_desc, first + wstride < nchunks ? first + wstride : lastc);
  }
  for (i64 chunk = first; chunk < nchunks; chunk += wstride) {
    stream_issue_w<NT>(q, dcur, rowptr, col, val, lane);
    const int r = dcur.r0 + lane;
    const bool live = r < dcur.r1;
    const int basev = dcur.base & ~1, basec = dcur.base & ~3;
    const int av = q.ra - basev, ac = q.ra - basec, len = q.rb - q.ra;
#pragma unroll
    for (int j = 0; j < XV_IT; ++j) sv2[lane + 64 * j] = q.v[j];
#pragma unroll
    for (int j = 0; j < XC_IT; ++j) sc4[lane + 64 * j] = q.c[j];
    __builtin_amdgcn_wave_barrier();
    double xv[WUNR], vv[WUNR];
    const int c0 = dcur.base - basec;           // first real column slot of the chunk: always valid
#pragma unroll
    for (int j = 0; j < WUNR; ++j) {
      const bool ok = j < len;
      xv[j] = x[scl[ok ? ac + j : c0]];
      vv[j] = ok ? sv[av + j] : 0.0;
    }
    const i64 c2 = chunk + 2 * wstride;
    const Desc dnext2 = load_desc(chunk_desc, c2 < nchunks ? c2 : lastc);
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < WUNR; ++j) sum += vv[j] * xv[j];
    if (__builtin_expect(len > WUNR, 0))
      for (int k = WUNR; k < len; ++k) sum += sv[av + k] * x[scl[ac + k]];
    __builtin_amdgcn_wave_barrier();
    if (live) {
      y[r] = sum;
      if (MODE == 1) acc0 += aux[r] * sum;
      if (MODE >= 2) {
        acc0 += sum * x[r];
        acc1 += sum * sum;
      }
      if (MODE == 3) acc2 += aux[r] * sum;
    }
    dcur = dnext;
    dnext = dnext2;
  }
  if (MODE >= 1) {
    const double t0 = block_sum(acc0, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t0;
  }
  if (MODE >= 2) {
    const double t1 = block_sum(acc1, s_red);
    if (threadIdx.x == 0) partials[gridDim.x + blockIdx.x] = t1;
  }
  if (MODE == 3) {
    const double t2 = block_sum(acc2, s_red);
    if (threadIdx.x == 0) partials[4 * (size_t)gridDim.x + blockIdx.x] = t2;
  }
}

// ---- stencil slices (default) ----------------------------------------------------------------------------------
// The assembler knows what a generic CSR kernel cannot: away from the interface every row of a line carries the
// SAME stencil -- identical (col - row) offsets, and on a uniform mesh bitwise identical (equilibrated) values.
// build_spmv_chunks() detects that once per matrix (k_row_same) and re-slices the rows:
//   U slice   <= 254 consecutive rows, identical offsets and values: the slice is ONE 128-byte record (descriptor,
//             offsets, values); lane l computes rows r0+2l, r0+2l+1 from coalesced 16-byte x loads.  Nothing else
//             of the matrix is streamed.
//   P slice   identical offsets, per-row values: values re-laid slot-major (pval[j*rows + l]) so the 8 B/entry
//             stream is coalesced without LDS; the 4 B/entry column stream disappears.
//   G chunk   the remaining irregular rows (cut cells, their neighbours, line ends, rows with > 8 entries), packed 64
//             at a time into a compact CSR of their own and processed like k_spmv_cw (LDS-staged stream + gathers).
// The products are accumulated in the CSR entry order in all three paths, so y is bitwise what the CSR kernels give.
//
// What bounds the U path (SQ counters + ablations, profiles/r01_spmv_slices.txt): the kernel ran at the same speed with
// every x load forced to hit one L1 line, with the record loads forced to one line, at 4, 5, 6 or 8 waves per SIMD,
// and with 8- or 16-byte accesses: ~22 cycles per vector-memory INSTRUCTION per CU whatever its width -- the
// address unit, not HBM, L2 or latency.  Hence: two rows per lane (16-byte accesses), no padded slots (the slot
// count is a template parameter: 1 border identity rows, 3 / 5 / 7 the 1-D / 2-D / 3-D stencils), and one record
// load per slice instead of descriptor + offsets + values.
//
// Slices are sorted by first row; with `xcd` each XCD (blocks are dispatched round-robin over the 8 XCDs) sweeps one
// contiguous eighth of them, so the +-line / +-plane x neighbours are found in that XCD's own L2.
enum { SL_U = 0, SL_P = 1, SL_G = 2 };
constexpr int SL_MAXROWS_U = 254, SL_MAXROWS_P = 128, SL_MAXCNT = 8, SL_REC = 32;   // record: 32 dwords

struct SDesc {
  int r0, meta, base, aux;
};

// wave-uniform values out of a vector register (the result lives in SGPRs)
__device__ inline int rlane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

typedef double d2u_t __attribute__((ext_vector_type(2), aligned(8)));   // 16-byte access, 8-byte aligned

template <bool NT>
__device__ inline d2_t load_pair(const double* p) {
  const d2u_t* q = reinterpret_cast<const d2u_t*>(p);
  d2u_t v = NT ? __builtin_nontemporal_load(q) : *q;
  d2_t r;
  r.x = v.x; r.y = v.y;
  return r;
}

// ---- element type per vector stream (mode 8 of the mixed-precision chain, launch_spmv_typed) ---------------------------
// VecTypes names the element types of x (TX), of the operand B = base (TB) and of y (TY) in memory; P32: the launch also
// writes p32 = (float)(psig B) for the rows it computes -- the chain's first launch, whose B IS x (same vector): the row's
// own x serves as B and no B stream is loaded at all.  A float stream is converted at the load and at the store (round to
// nearest); the arithmetic in between is the fp64 kernel's.  The all-double instantiation is the kernel as it was: its helpers
// below are the very loads and stores it used.
template <class TX_, class TB_, class TY_, bool P32_>
struct VecTypes {
  using TX = TX_;
  using TB = TB_;
  using TY = TY_;
  static constexpr bool P32 = P32_;
};
using VecF64 = VecTypes<double, double, double, false>;

typedef float f2u_t __attribute__((ext_vector_type(2), aligned(4)));   // 8-byte access, 4-byte aligned

template <bool NT>
__device__ inline d2_t load_pair_t(const double* p) { return load_pair<NT>(p); }
template <bool NT>
__device__ inline d2_t load_pair_t(const float* p) {
  const f2u_t* q = reinterpret_cast<const f2u_t*>(p);
  f2u_t v = NT ? __builtin_nontemporal_load(q) : *q;
  d2_t r;
  r.x = (double)v.x; r.y = (double)v.y;
  return r;
}
// a pair as it sits in registers between its load and its use: fp32 streams stay two dwords until the arithmetic widens them
typedef float f2_t __attribute__((ext_vector_type(2)));
template <class T> struct PairOf { typedef d2_t type; };
template <> struct PairOf<float> { typedef f2_t type; };
template <bool NT>
__device__ inline d2_t load_raw(const double* p) { return load_pair<NT>(p); }
template <bool NT>
__device__ inline f2_t load_raw(const float* p) {
  const f2u_t* q = reinterpret_cast<const f2u_t*>(p);
  f2u_t v = NT ? __builtin_nontemporal_load(q) : *q;
  f2_t r;
  r.x = v.x; r.y = v.y;
  return r;
}
__device__ inline d2_t widen(const d2_t& v) { return v; }
__device__ inline d2_t widen(const f2_t& v) {
  d2_t r;
  r.x = (double)v.x; r.y = (double)v.y;
  return r;
}
// a pair of rows of y (or of p32): stream hint unless `plain`
__device__ inline void store_pair_t(double* p, double a, double b, bool plain) {
  d2u_t out;
  out.x = a; out.y = b;
  if (!plain) __builtin_nontemporal_store(out, reinterpret_cast<d2u_t*>(p));
  else *reinterpret_cast<d2u_t*>(p) = out;
}
// (an fp32 store saturates at the largest finite float: a start residual that outgrew the scale σ taken from the previous solve
//  then costs this application its accuracy, not the solve its finiteness -- x and r still move by the same computed vectors,
//  and every later application of the solve is fp64)
__device__ inline float narrow(double a) {
  const float f = (float)a;
  return __builtin_fminf(__builtin_fmaxf(f, -3.402823466e+38f), 3.402823466e+38f);
}
__device__ inline void store_pair_t(float* p, double a, double b, bool plain) {
  f2u_t out;
  out.x = narrow(a); out.y = narrow(b);
  if (!plain) __builtin_nontemporal_store(out, reinterpret_cast<f2u_t*>(p));
  else *reinterpret_cast<f2u_t*>(p) = out;
}
__device__ inline void store_one_t(double* p, double a) { *p = a; }
__device__ inline void store_one_t(float* p, double a) { *p = narrow(a); }

// Launch modes of the slice kernel (MODE): what the epilogue does with s = (A x)_row.  A, B = operand vectors read at the
// row (pa, pb below); own = x_row.
//   0  y = s
//   1  y = s;                         acc0 += A y                                   A = aux
//   2  y = s;                         acc0 += A y, acc1 += y y                      A = dotx (or x)
//   3  y = s;                         acc0 += A y, acc1 += y y, acc2 += B y         A = dotx (or x), B = aux
//   8  y = pc2 B + (pc0 own + pc1 s)                                                B = base
// 8 is a step of the Horner chain that applies the polynomial preconditioner M⁻¹ = q(Â) (pg_krylov.hip); 1 / 3 close an
// application of the operator with its dots.
template <int MODE>
struct ModeInfo {
  static constexpr bool OWN = MODE == 8;
  static constexpr bool HAS_A = MODE == 1 || MODE == 2 || MODE == 3;
  static constexpr bool HAS_B = MODE == 3 || MODE == 8;
  static constexpr bool DOT0 = MODE == 1 || MODE == 2 || MODE == 3;
  static constexpr bool DOT1 = MODE == 2 || MODE == 3;
  static constexpr bool DOT2 = MODE == 3;
};

// y of one row from its product s; b = the operand B at the row.  The ONE expression every path of the kernel uses.
template <int MODE>
__device__ __forceinline__ double mode_out(double s, double own, double b, double pc0, double pc1, double pc2) {
  // (spelled out: which product of `pc2 b + (pc0 own + pc1 s)` is rounded before the fused adds is otherwise the compiler's
  // choice, path by path; this is the form it has been emitting -- pc1 s rounded, two fused multiply-adds)
  if (MODE == 8) return __builtin_fma(pc2, b, __builtin_fma(pc0, own, pc1 * s));
  return s;
}

// rows of one U (PSL = false) or P (PSL = true) slice with CNT stencil slots; rec = the slice's record (lane & 31).
// NB batches of 128 rows: every load of the slice is issued before the first FMA (one exposed latency per slice).
template <int CNT, int NB, bool PSL, int MODE, bool NT, class VT>
__device__ __forceinline__ void slice_rows(const SDesc& d, int nrows, int rec, const double* __restrict__ pval,
                                  const typename VT::TX* __restrict__ x, typename VT::TY* __restrict__ y, const double* __restrict__ pa,
                                  const typename VT::TB* __restrict__ pb, int lane, double& acc0, double& acc1, double& acc2, int dbg,
                                  double pc0, double pc1, double pc2, float* __restrict__ p32, double psig) {
  using MI = ModeInfo<MODE>;
  int o[CNT];
#pragma unroll
  for (int j = 0; j < CNT; ++j) o[j] = (dbg & 4) ? 0 : rlane(rec, 4 + j);
  int l0[NB];
  bool live0[NB], live1[NB];
  typename PairOf<typename VT::TX>::type xv[NB][CNT];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int l = 128 * b + 2 * lane;
    live0[b] = l < nrows;
    live1[b] = l + 1 < nrows;
    l0[b] = live0[b] ? l : 0;
#pragma unroll
    for (int j = 0; j < CNT; ++j) xv[b][j] = load_raw<false>(x + d.r0 + l0[b] + o[j]);
  }
  d2_t sum[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) { sum[b].x = 0.0; sum[b].y = 0.0; }
  if (!PSL) {
#pragma unroll
    for (int j = 0; j < CNT; ++j) {
      const double c = __hiloint2double(rlane(rec, 13 + 2 * j), rlane(rec, 12 + 2 * j));
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const d2_t xw = widen(xv[b][j]);
        sum[b].x += c * xw.x;
        sum[b].y += c * xw.y;
      }
    }
  } else {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const double* __restrict__ pv = pval + d.base + l0[b];
      d2_t vv[CNT];
#pragma unroll
      for (int j = 0; j < CNT; ++j) vv[j] = load_pair<NT>(pv + j * nrows);
#pragma unroll
      for (int j = 0; j < CNT; ++j) {
        const d2_t xw = widen(xv[b][j]);
        sum[b].x += vv[j].x * xw.x;
        sum[b].y += vv[j].y * xw.y;
      }
    }
  }
  d2_t own[NB], ax[NB], ax2[NB];   // the row's own x, operands A and B (ModeInfo)
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    own[b].x = own[b].y = ax[b].x = ax[b].y = ax2[b].x = ax2[b].y = 0.0;
    if (MI::OWN) own[b] = load_pair_t<false>(x + d.r0 + l0[b]);
    if (MI::HAS_A) ax[b] = load_pair<false>(pa + d.r0 + l0[b]);
    if (MI::HAS_B && !VT::P32) ax2[b] = load_pair_t<false>(pb + d.r0 + l0[b]);
    if (VT::P32) ax2[b] = own[b];
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    sum[b].x = mode_out<MODE>(sum[b].x, own[b].x, ax2[b].x, pc0, pc1, pc2);
    sum[b].y = mode_out<MODE>(sum[b].y, own[b].y, ax2[b].y, pc0, pc1, pc2);
    const bool st = !(dbg & 8) || sum[b].x == 1.2345e-300;
    typename VT::TY* yp = y + d.r0 + l0[b];
    if (VT::P32) {   // p32 = (float)(psig base) for the rows computed here
      float* pp = p32 + d.r0 + l0[b];
      if (live1[b]) store_pair_t(pp, psig * ax2[b].x, psig * ax2[b].y, false);
      else if (live0[b]) store_one_t(pp, psig * ax2[b].x);
    }
    if (live1[b]) {
      if (st) store_pair_t(yp, sum[b].x, sum[b].y, (dbg & 2048) != 0);
      if (MI::DOT0) acc0 += ax[b].x * sum[b].x + ax[b].y * sum[b].y;
      if (MI::DOT1) acc1 += sum[b].x * sum[b].x + sum[b].y * sum[b].y;
      if (MI::DOT2) acc2 += ax2[b].x * sum[b].x + ax2[b].y * sum[b].y;
    } else if (live0[b]) {
      if (st) store_one_t(yp, sum[b].x);
      if (MI::DOT0) acc0 += ax[b].x * sum[b].x;
      if (MI::DOT1) acc1 += sum[b].x * sum[b].x;
      if (MI::DOT2) acc2 += ax2[b].x * sum[b].x;
    }
  }
}

template <int CNT, bool PSL, int MODE, bool NT, class VT>
__device__ __forceinline__ void slice_nb(const SDesc& d, int nrows, int rec, const double* __restrict__ pval,
                                const typename VT::TX* __restrict__ x, typename VT::TY* __restrict__ y, const double* __restrict__ pa,
                                const typename VT::TB* __restrict__ pb, int lane, double& acc0, double& acc1, double& acc2, int dbg,
                                double pc0, double pc1, double pc2, float* __restrict__ p32, double psig) {
  if (!PSL && nrows > 128) slice_rows<CNT, 2, PSL, MODE, NT, VT>(d, nrows, rec, pval, x, y, pa, pb, lane, acc0, acc1, acc2, dbg, pc0, pc1, pc2, p32, psig);
  else slice_rows<CNT, 1, PSL, MODE, NT, VT>(d, nrows, rec, pval, x, y, pa, pb, lane, acc0, acc1, acc2, dbg, pc0, pc1, pc2, p32, psig);
}

template <bool PSL, int MODE, bool NT, class VT>
__device__ __forceinline__ void slice_dispatch(int cnt, const SDesc& d, int nrows, int rec, const double* __restrict__ pval,
                                      const typename VT::TX* __restrict__ x, typename VT::TY* __restrict__ y,
                                      const double* __restrict__ pa, const typename VT::TB* __restrict__ pb, int lane, double& acc0,
                                      double& acc1, double& acc2, int dbg, double pc0, double pc1, double pc2,
                                      float* __restrict__ p32, double psig) {
  switch (cnt) {   // wave-uniform
    case 1: slice_nb<1, PSL, MODE, NT, VT>(d, nrows, rec, pval, x, y, pa, pb, lane, acc0, acc1, acc2, dbg, pc0, pc1, pc2, p32, psig); break;
    case 3: slice_nb<3, PSL, MODE, NT, VT>(d, nrows, rec, pval, x, y, pa, pb, lane, acc0, acc1, acc2, dbg, pc0, pc1, pc2, p32, psig); break;
    case 5: slice_nb<5, PSL, MODE, NT, VT>(d, nrows, rec, pval, x, y, pa, pb, lane, acc0, acc1, acc2, dbg, pc0, pc1, pc2, p32, psig); break;
    case 7: slice_nb<7, PSL, MODE, NT, VT>(d, nrows, rec, pval, x, y, pa, pb, lane, acc0, acc1, acc2, dbg, pc0, pc1, pc2, p32, psig); break;
    case 2: slice_nb<2, PSL, MODE, NT, VT>(d, nrows, rec, pval, x, y, pa, pb, lane, acc0, acc1, acc2, dbg, pc0, pc1, pc2, p32, psig); break;
    case 4: slice_nb<4, PSL, MODE, NT, VT>(d, nrows, rec, pval, x, y, pa, pb, lane, acc0, acc1, acc2, dbg, pc0, pc1, pc2, p32, psig); break;
    case 6: slice_nb<6, PSL, MODE, NT, VT>(d, nrows, rec, pval, x, y, pa, pb, lane, acc0, acc1, acc2, dbg, pc0, pc1, pc2, p32, psig); break;
    default: slice_nb<8, PSL, MODE, NT, VT>(d, nrows, rec, pval, x, y, pa, pb, lane, acc0, acc1, acc2, dbg, pc0, pc1, pc2, p32, psig); break;
  }
}


// ---- marching units (M): the uniform interior of a 2-D / 3-D stencil ----------------------------------------------
// What bounds the U path is bytes through the L1 / texture-address path: 7 loads of x per row (80 B per row with the dot
// operands and the store) while only 8 B per row have to come from memory.  A U run of a 3-D problem is a piece of a grid
// line, and the +-1 taps of a row are its neighbours in the SAME load, the +-plane taps the rows of the next / previous
// line of the chain of runs that face each other across the slowest stencil direction (col - row offsets o[0] / o[cnt-1]
// lead from a row to the row of the same lateral position one plane down / up).  So one wave MARCHES along such a chain:
// it keeps the lines of planes k-1, k, k+1 in registers, lane l holding elements 2l, 2l+1 of a window of 128 consecutive
// elements; per plane it loads ONE new line of the chain plus the two lateral neighbour lines (3-D only), computes the
// 126 rows 1..126 of the window -- row 2l+1 from (2l, 2l+1, 2l+2), row 2l+2 from (2l+1, 2l+2, 2l+3), the elements of lane
// l+1 arriving by a lane shift -- and stores them: 3 loads of x per 126 rows instead of 7 per 128 (1 instead of 5 in
// 2-D), 24 instead of 56 bytes of x through L1 per row.  The products are accumulated in the rows' entry order as
// everywhere else: y is bitwise the CSR kernels' y.
//
// One 256-byte record per UNIT (<= MARCH_K consecutive planes of one chain x one window), read with one vector load:
//   dword 0            K | cnt << 8 | active lanes << 16   (planes in the unit, MARCH_K or MARCH_KS: shorter units are closed by empty
//                                               planes; 7 = 3-D stencil, 5 = 2-D stencil)
//   dword 1            first computed row (sort key only)
//   dwords 2..15       the cnt values of the rows (all rows of a unit share them bitwise), in the entry order of the
//                      assembled rows: +1, -1, [+lateral, -lateral,] +plane, -plane, diagonal (eval_row, pg_stencil.h)
//   dword 16, 17       row index held by lane 0 (.x) in the line below the first / above the last plane of the unit
//   dwords 18 + 4i..   plane i: row index held by lane 0 (.x); offset to the lower / upper lateral neighbour line
//                      (col - row; 3-D only); lo | hi << 8 = window-relative range [lo, hi) of the rows computed here
//   dword 34, 35       edge rows of the unit: the first one's number in the stream of edge rows, their count (<= 64)
//   dwords 36 + i      plane i: edge rows below lo | above hi << 8 | number of the plane's first edge row in the unit << 16
// build_march_units() forms chains and units on the host from the same row flags the slices are cut from.
//
// EDGE ROWS.  The irregular rows at the two ends of a plane's marched range -- the cells where a chord of the fluid meets the
// body, and their neighbours -- are irregular in their VALUES only: their (col - row) offsets are those of the marched rows
// next to them on the line, a neighbour that does not exist is a missing entry.  The planner (pg_host_algos.h) hands up to 8 of
// them per end (64 per unit) to the unit: the lane that computes a window position holds the row's seven x operands already,
// so all such a row needs from memory is its values -- 7 slots per row in the slot order of the marched rows, +0.0 where the
// row has no entry (an eighth slot pads the row to 64 bytes), unit by unit and in PAIRS of slots inside a unit: slots 2p, 2p+1
// of the unit's e-th edge row at e_val[8 first + 2 (p count + e)].  Lane e of the wave loads the pairs of row e with the
// unit's other loads -- straight into the wave's slice of LDS (global_load_lds_dwordx4: the values never occupy a VGPR while
// they are in flight, which is when the unit's registers are scarce) -- and the lane that owns the row reads them from there
// and takes them as the row's coefficients: the products are accumulated in slot order, a +0.0 x term leaves a partial sum as
// it is, so y is bitwise the CSR kernels' y.  No column index, row pointer or row id is read for these rows, no x element is
// gathered.
#ifndef PG_MARCH_K
#define PG_MARCH_K 4
#endif
#ifndef PG_MARCH_SPLIT
#define PG_MARCH_SPLIT 1
#endif
constexpr int MARCH_K = PG_MARCH_K, MARCH_KS = 2, MARCH_REC = 64, MARCH_W = 126;   // planes per unit: full / short units
constexpr int MARCH_EDGE = pghost::EDGE_REC, MARCH_ESLOTS = pghost::EDGE_SLOTS;   // edge rows: record dwords 34.., slots per row
static_assert(MARCH_K > MARCH_KS && 18 + 4 * MARCH_K <= MARCH_EDGE && MARCH_EDGE + 2 + MARCH_K <= MARCH_REC, "unit record layout");

__device__ inline double lane_up(double v) {   // the value lane l + 1 holds (lane 63: unspecified)
  return __shfl_down(v, 1, 64);
}

template <class TX, class TB>
struct MarchSide {   // per-plane operands besides the chain's own lines: lateral neighbour lines, dot operands
  typename PairOf<TX>::type ym, yp;
  d2_t ax;
  typename PairOf<TB>::type ax2;
};

// rows 2l+1, 2l+2 of one plane from the lines in registers; returns lane l+1's xc.x (the next plane's xm_n)
template <int CNT, int MODE, bool EDGE, class VT>
__device__ __forceinline__ double march_plane(const double (&c)[CNT], int rng, int l2, typename VT::TY* __restrict__ yrow,
                                              const typename PairOf<typename VT::TX>::type& xm_, double xm_n,
                                              const typename PairOf<typename VT::TX>::type& xc_,
                                              const typename PairOf<typename VT::TX>::type& xp_,
                                              const MarchSide<typename VT::TX, typename VT::TB>& sd_, double pc0,
                                              double pc1, double pc2, double& acc0, double& acc1, double& acc2, int dbg,
                                              int einfo, int e_first, const d2_t* el, const d2_t* cl, float* __restrict__ prow,
                                              double psig) {
  using MI = ModeInfo<MODE>;
  constexpr bool Y = CNT == 7;
  const d2_t xm = widen(xm_), xc = widen(xc_), xp = widen(xp_);
  struct { d2_t ym, yp, ax, ax2; } sd;
  sd.ym = widen(sd_.ym); sd.yp = widen(sd_.yp); sd.ax = sd_.ax; sd.ax2 = widen(sd_.ax2);
  const double xc_nx = lane_up(xc.x), xc_ny = lane_up(xc.y), xp_n = lane_up(xp.x);
  // entry order of the assembled rows (eval_row, pg_stencil.h): +1, -1, [+lateral, -lateral,] +plane, -plane, diagonal
  double a1[CNT], a2[CNT];   // the x operands of rows 2l+1, 2l+2 by slot
  {
    int j = 0;
    a1[j] = xc_nx; a2[j] = xc_ny; ++j;
    a1[j] = xc.x;  a2[j] = xc.y;  ++j;
    if (Y) {
      a1[j] = sd.yp.x; a2[j] = sd.yp.y; ++j;
      a1[j] = sd.ym.x; a2[j] = sd.ym.y; ++j;
    }
    a1[j] = xp.y;  a2[j] = xp_n;  ++j;
    a1[j] = xm.y;  a2[j] = xm_n;  ++j;
    a1[j] = xc.y;  a2[j] = xc_nx;
  }
  double s1 = 0.0, s2 = 0.0;
  int lo = rng & 255, hi = rng >> 8;
  if (EDGE) {   // edge rows below lo / above hi (einfo; none: no lane takes part): the row's own values out of LDS, not the unit's
    const int nlo = einfo & 255, nhi = (einfo >> 8) & 255, e0 = (einfo >> 16) - e_first;
    const int elo = lo - nlo, ehi = hi + nhi, p1 = l2 + 1, p2 = l2 + 2;
    const bool g1 = p1 >= elo && p1 < ehi && !(p1 >= lo && p1 < hi), g2 = p2 >= elo && p2 < ehi && !(p2 >= lo && p2 < hi);
    // every lane reads its coefficients from LDS: an edge row's own, or the unit's shared ones (cl) -- a select between a
    // loaded value and a wave-uniform one would need the latter in VGPRs, 14 of them for the whole unit
    const d2_t* q1 = g1 ? el + (e0 + (p1 - elo) - (p1 >= hi ? hi - lo : 0)) : cl;
    const d2_t* q2 = g2 ? el + (e0 + (p2 - elo) - (p2 >= hi ? hi - lo : 0)) : cl;
#pragma unroll
    for (int jp = 0; jp < (CNT + 1) / 2; ++jp) {
      const d2_t w1 = q1[64 * jp], w2 = q2[64 * jp];
      s1 += w1.x * a1[2 * jp];
      s2 += w2.x * a2[2 * jp];
      if (2 * jp + 1 < CNT) {
        s1 += w1.y * a1[2 * jp + 1];
        s2 += w2.y * a2[2 * jp + 1];
      }
    }
    lo = elo;
    hi = ehi;
  } else {
#pragma unroll
    for (int j = 0; j < CNT; ++j) { s1 += c[j] * a1[j]; s2 += c[j] * a2[j]; }
  }
  // (the row's own x: elements 2l+1, 2l+2 of the centre line)
  const double b1 = VT::P32 ? xc.y : sd.ax2.x, b2 = VT::P32 ? xc_nx : sd.ax2.y;   // (P32: B is x)
  s1 = mode_out<MODE>(s1, xc.y, b1, pc0, pc1, pc2);
  s2 = mode_out<MODE>(s2, xc_nx, b2, pc0, pc1, pc2);
  const bool nost = (dbg & 32) && s1 != 1.2345e-300;   // diagnostics: no stores
  const bool allst = (dbg & 512) != 0;                  // diagnostics: every lane stores its pair (whole windows)
  const bool v1 = ((l2 + 1 >= lo && l2 + 1 < hi) || allst) && !nost, v2 = ((l2 + 2 >= lo && l2 + 2 < hi) || allst) && !nost;
  if (VT::P32) {   // p32 = (float)(psig base) for the rows computed here
    if (v1 && v2) store_pair_t(prow, psig * b1, psig * b2, false);
    else if (v1) store_one_t(prow, psig * b1);
    else if (v2) store_one_t(prow + 1, psig * b2);
  }
  if (v1 && v2) {
    // y leaves with the stream hint: fewer dirty lines for the end-of-kernel write-back, which sits between every two
    // dependent launches of the loop (55.3 -> 52.6 µs per back-to-back launch at 512^3 on one box, within the noise on another; system-scope write-through
    // stores, `sc0 sc1`, double the launch; dbg bit 2048: plain stores)
    store_pair_t(yrow, s1, s2, (dbg & 2048) != 0);
  } else if (v1) {
    store_one_t(yrow, s1);
  } else if (v2) {
    store_one_t(yrow + 1, s2);
  }
  if (MI::DOT0) {
    const double w1 = v1 ? s1 : 0.0, w2 = v2 ? s2 : 0.0;
    acc0 += (v1 ? sd.ax.x : 0.0) * w1 + (v2 ? sd.ax.y : 0.0) * w2;
    if (MI::DOT1) acc1 += w1 * w1 + w2 * w2;
    if (MI::DOT2) acc2 += (v1 ? sd.ax2.x : 0.0) * w1 + (v2 ? sd.ax2.y : 0.0) * w2;
  }
  return xc_nx;
}

// One unit of exactly KK planes (the builder closes shorter ones with empty planes), fully unrolled: EVERY load of the
// unit -- KK + 2 lines of the chain, 2 KK lateral lines, the dot operands -- is independent of the arithmetic, so the
// compiler issues them up front (as far as registers allow) and the wave pays ONE memory round trip per unit.  A loop
// over the planes with prefetch registers did not get there: the registers carried around the back edge are copied,
// and a copy waits for the load that fills it (2.2 us per plane, measured).
// (Q0, KTOT: planes [Q0, Q0 + KK) of a unit of KTOT planes -- the launches with fused dots take a full unit in two halves,
// see march_dispatch)
// EDGE: the unit has edge rows.  The two forms are two straight-line bodies: a branch per plane inside one body pins every
// load of the unit above the first branch and costs ~25 spilled VGPRs (the compiler's report).
template <int CNT, int MODE, bool EDGE, class VT, int KK, int Q0 = 0, int KTOT = KK>
__device__ __forceinline__ void march_unit(int rec, int lane, const typename VT::TX* __restrict__ x, typename VT::TY* __restrict__ y,
                                  const double* __restrict__ pa, const typename VT::TB* __restrict__ pb, double pc0, double pc1,
                                  double pc2, double& acc0, double& acc1, double& acc2, int dbg,
                                  const double* __restrict__ e_val, double* sv, double* sx, float* __restrict__ p32, double psig) {
  using MI = ModeInfo<MODE>;
  constexpr bool Y = CNT == 7;
  const int amask = (dbg & 128) ? ~1 : ~0;          // diagnostics: every access 16-byte aligned (wrong results)
  const int one = (dbg & 128) ? 0 : 1;
  const bool nolat = (dbg & 64) != 0;               // diagnostics: no lateral lines
  double c[CNT];
#pragma unroll
  for (int j = 0; j < CNT; ++j) c[j] = __hiloint2double(rlane(rec, 3 + 2 * j), rlane(rec, 2 + 2 * j));
  const int l2 = 2 * lane;
  int rb[KK];
  typedef typename PairOf<typename VT::TX>::type xpair_t;
  typedef typename PairOf<typename VT::TB>::type bpair_t;
  xpair_t ln[KK + 2];       // lines -1 .. KK of the chain
  MarchSide<typename VT::TX, typename VT::TB> sd[KK];
  // lanes beyond the widest plane of the unit load nothing (a window at the end of a chord is mostly empty: what a load
  // costs the CU's memory pipe goes with its active lanes); they run the arithmetic on zeros and store nothing
  const bool act = lane < (rlane(rec, 0) >> 16);
  d2_t zero;
  zero.x = zero.y = 0.0;
  xpair_t xzero;
  xzero.x = xzero.y = 0;
  bpair_t bzero;
  bzero.x = bzero.y = 0;
#pragma unroll
  for (int q = 0; q < KK + 2; ++q) ln[q] = xzero;
#pragma unroll
  for (int q = 0; q < KK; ++q) {
    rb[q] = rlane(rec, 18 + 4 * (Q0 + q)) & amask;
    sd[q].ym = sd[q].yp = xzero;
    sd[q].ax = zero;
    sd[q].ax2 = bzero;
  }
  if (act) {
    ln[0] = load_raw<false>(x + (rlane(rec, Q0 == 0 ? 16 : 18 + 4 * (Q0 - 1)) & amask) + l2);
#pragma unroll
    for (int q = 0; q < KK; ++q) ln[q + 1] = load_raw<false>(x + rb[q] + l2);
    ln[KK + 1] = load_raw<false>(x + (rlane(rec, Q0 + KK == KTOT ? 17 : 18 + 4 * (Q0 + KK)) & amask) + l2);
#pragma unroll
    for (int q = 0; q < KK; ++q) {
      if (Y && !nolat) {
        sd[q].ym = load_raw<false>(x + rb[q] + (rlane(rec, 19 + 4 * (Q0 + q)) & amask) + l2 + one);
        sd[q].yp = load_raw<false>(x + rb[q] + (rlane(rec, 20 + 4 * (Q0 + q)) & amask) + l2 + one);
      }
      if (MI::HAS_A) sd[q].ax = load_pair<false>(pa + rb[q] + l2 + one);
      if (MI::HAS_B && !VT::P32) sd[q].ax2 = load_raw<false>(pb + rb[q] + l2 + one);   // (no stream hint: the chain's input is re-read by every launch of the chain and stays in the Infinity Cache -- with the hint a Horner step took 65.7 instead of 53.8 us)
    }
  }
  // the values of the edge rows of these planes, a row per lane, issued with the lines: pair p of lane e's row lands at
  // sv[2 (64 p + e)] (a wave instruction writes lane x 16 bytes from its LDS base on)
  const int e_first = rlane(rec, MARCH_EDGE + 2 + Q0) >> 16;
  const int e_cnt = (Q0 + KK == KTOT ? rlane(rec, MARCH_EDGE + 1) : rlane(rec, MARCH_EDGE + 2 + Q0 + KK) >> 16) - e_first;
  // (the lane number as the edge rows' addresses see it is made opaque: hoisted out of the kernel's loops as loop invariants,
  // those addresses would occupy VGPRs through the slices' code as well, which has none to spare)
  int elane = lane;
  if (EDGE) asm volatile("" : "+v"(elane));
  if (EDGE && e_cnt > 0) {
    const int e_all = rlane(rec, MARCH_EDGE + 1);
    const double* ep = e_val + (i64)MARCH_ESLOTS * rlane(rec, MARCH_EDGE) + 2 * (e_first + elane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the previous unit's reads of these LDS slots have returned)
    if (elane < e_cnt) {
#pragma unroll
      for (int jp = 0; jp < (CNT + 1) / 2; ++jp)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ep + 2 * jp * e_all),
                                         (__attribute__((address_space(3))) void*)(sv + 128 * jp), 16, 0, 0);
    }
    // the LDS writes of these loads count on vmcnt like the loads around them; everything the unit loads is needed now anyway
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  if (EDGE) {
    // the unit's shared coefficients in the same layout (pair p at sx[128 p]): record dwords 2..15, lane l holds dword l
    const int k = elane - 2;
    if (k >= 0 && k < 2 * CNT) reinterpret_cast<int*>(sx)[256 * (k >> 2) + (k & 3)] = rec;
  }
  const d2_t* el = reinterpret_cast<const d2_t*>(sv);
  const d2_t* cl = reinterpret_cast<const d2_t*>(sx);
  double xm_n = lane_up((double)ln[0].x);
#pragma unroll
  for (int q = 0; q < KK; ++q)
    xm_n = march_plane<CNT, MODE, EDGE, VT>(c, rlane(rec, 21 + 4 * (Q0 + q)), l2, y + rb[q] + l2 + one, ln[q], xm_n, ln[q + 1], ln[q + 2], sd[q], pc0,
                                  pc1, pc2, acc0, acc1, acc2, dbg, rlane(rec, MARCH_EDGE + 2 + Q0 + q), e_first, el, cl,
                                  VT::P32 ? p32 + rb[q] + l2 + one : nullptr, psig);
}

template <int CNT, int MODE, bool EDGE, class VT>
__device__ __forceinline__ void march_dispatch(int rec, int lane, const typename VT::TX* __restrict__ x, typename VT::TY* __restrict__ y,
                                      const double* __restrict__ pa, const typename VT::TB* __restrict__ pb, double pc0, double pc1,
                                      double pc2, double& acc0, double& acc1, double& acc2, int dbg,
                                      const double* __restrict__ e_val, double* sv, double* sx, float* __restrict__ p32, double psig) {
  // The launch with three fused dots and two more operand vectors per plane (mode 3) does not fit a unit of MARCH_K planes into
  // the 128 VGPRs of four waves per SIMD: it takes it in two halves -- two more line loads per unit, which hit L1.  (Mode 1, one
  // operand vector, fits a whole unit: 127 VGPRs, no scratch.)
  constexpr bool SPLIT = MODE == 3 && MARCH_K == 2 * MARCH_KS && PG_MARCH_SPLIT;
  if ((rlane(rec, 0) & 255) == MARCH_K) {
    if (SPLIT) {
      march_unit<CNT, MODE, EDGE, VT, MARCH_KS, 0, MARCH_K>(rec, lane, x, y, pa, pb, pc0, pc1, pc2, acc0, acc1, acc2, dbg, e_val, sv, sx, p32, psig);
      march_unit<CNT, MODE, EDGE, VT, MARCH_KS, MARCH_KS, MARCH_K>(rec, lane, x, y, pa, pb, pc0, pc1, pc2, acc0, acc1, acc2, dbg, e_val, sv, sx, p32, psig);
    } else {
      march_unit<CNT, MODE, EDGE, VT, MARCH_K>(rec, lane, x, y, pa, pb, pc0, pc1, pc2, acc0, acc1, acc2, dbg, e_val, sv, sx, p32, psig);
    }
  } else {
    march_unit<CNT, MODE, EDGE, VT, MARCH_KS>(rec, lane, x, y, pa, pb, pc0, pc1, pc2, acc0, acc1, acc2, dbg, e_val, sv, sx, p32, psig);
  }
}

// DIAG: the diagnostic build of the kernel (ablations for profiles/: PG_SPMV_XCD bits 8.. skip parts of the work or force
// access patterns and give WRONG products).  The shipped instantiation has DIAG = false: `dbg` is the constant 0 there and
// none of the switches exists in its code.
template <int MODE, bool NT, bool DIAG, class VT = VecF64>
__global__ __launch_bounds__(BLOCK, 4) void k_spmv_s(i64 nslices, const int* __restrict__ srec,
                                                  const double* __restrict__ pval, const int* __restrict__ g_rowid,
                                                  const int* __restrict__ g_rowptr, const int* __restrict__ g_col,
                                                  const double* __restrict__ g_val, const typename VT::TX* __restrict__ x,
                                                  typename VT::TY* __restrict__ y, const double* __restrict__ aux,
                                                  double* __restrict__ partials, const double* __restrict__ sc, int xcd,
                                                  FinArgs fin, int pstride, int accum, const int* __restrict__ mrec,
                                                  i64 nunits, const int* __restrict__ tiles, int tpx,
                                                  const double* __restrict__ e_val) {
  __shared__ __attribute__((aligned(16))) double s_val[BLOCK / 64][512];
  __shared__ __attribute__((aligned(16))) double s_x[BLOCK / 64][512];   // G chunks: x[col] of every entry of the chunk
  __shared__ double s_red[BLOCK / 64];
  if (sc && sc[S_DONE] != 0.0) return;
  using MI = ModeInfo<MODE>;
  constexpr bool DOTS = MI::DOT0;
  static_assert(MODE == 8 || std::is_same<VT, VecF64>::value, "element types per stream exist for mode 8 only");
  // operand of the (y, .) dot of modes 2 / 3 (their x is double)
  const double* __restrict__ dx = fin.dotx ? fin.dotx : reinterpret_cast<const double*>(x);
  // operand vectors A and B of the epilogue (ModeInfo)
  const double* __restrict__ pa = MODE == 1 ? aux : ((MODE == 2 || MODE == 3) ? dx : nullptr);
  const typename VT::TB* __restrict__ pb = reinterpret_cast<const typename VT::TB*>(MODE == 3 ? aux : (MODE == 8 ? fin.base : nullptr));
  float* __restrict__ p32 = VT::P32 ? fin.p32 : nullptr;
  const double psig = fin.psig;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* __restrict__ sv = s_val[wave];
  double* __restrict__ sx = s_x[wave];
  d2_t* sv2 = reinterpret_cast<d2_t*>(sv);
  d2_t* sx2 = reinterpret_cast<d2_t*>(sx);
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  // diagnostics (PG_SPMV_XCD bits 8..; results are wrong with any of them): 1 skip G chunks, 2 skip U/P slices,
  // 4 every x load hits one line, 8 no y stores in U/P slices, 16 skip the marching units, 32 no y stores in the units,
  // 64 no lateral lines in the units, 128 every access of the units 16-byte aligned, 256 non-temporal y stores in the
  // units, 512 the units store whole windows, 2048 plain y stores in the units, 4096 slices before units (the latency-bound
  // irregular chunks then run alone at the start instead of under the streaming units of slower waves: 52 vs 45.6 us)
  const int dbg = DIAG ? (xcd >> 8) : 0;
  xcd &= 255;
  // ---- marching units first (the bulk of the rows), then the slices.  (Alternating units and slices in every wave, so
  // that the latency-bound irregular chunks of some waves overlap the streaming of others, measured no faster, and one
  // merged loop costs registers: the live ranges of both bodies add up -- 144 VGPRs, a wave per SIMD less.)
  xcd &= 1;
  // Work of this wave: every (BLOCK / 64 x blocks)-th unit and slice of its XCD's eighth of both lists (XCD-aware: the
  // blocks of an XCD share one L2) -- in TILES when the image has a tile table (build_tiles): tile t of XCD q = units
  // [tb[2t], tb[2t+2]) and the slices [tb[2t+1], tb[2t+3]) that lie next to them in the grid, units first.  The irregular
  // rows of a tile then gather x from lines the tile's units have just pulled into this XCD's L2; with all units before
  // all slices those lines crossed the fabric twice (PMC, 512^3: 28 MB of 234 per launch).  The round robin over the
  // waves runs on across the tiles (a tile holds about one unit per wave).
  const bool xsplit = xcd && gridDim.x >= 8;
  const int xid = xsplit ? (blockIdx.x & 7) : 0;
  const int woff = xsplit ? (int)(blockIdx.x >> 3) * (BLOCK / 64) + wave : (int)blockIdx.x * (BLOCK / 64) + wave;
  const int wstr = xsplit ? (int)(((i64)gridDim.x + 7 - xid) >> 3) * (BLOCK / 64) : (int)gridDim.x * (BLOCK / 64);
  const int* __restrict__ tb = tiles ? tiles + 2 * (tpx + 1) * xid : nullptr;
  const int ntile = tiles ? tpx : 1;
  const int l31 = lane & 31;
  for (int tile = 0; tile < ntile; ++tile) {
  i64 ulo, uhi, slo, shi, ubase, sbase;
  if (tiles) {
    ubase = tb[0]; sbase = tb[1];
    ulo = tb[2 * tile]; slo = tb[2 * tile + 1]; uhi = tb[2 * tile + 2]; shi = tb[2 * tile + 3];
  } else if (xsplit) {
    ubase = ulo = nunits * xid / 8; uhi = nunits * (xid + 1) / 8;
    sbase = slo = nslices * xid / 8; shi = nslices * (xid + 1) / 8;
  } else {
    ubase = ulo = 0; uhi = nunits;
    sbase = slo = 0; shi = nslices;
  }
  // (two bodies in program order, not a loop over two phases: hoisted out of such a loop, the first record addresses of the
  // slices were held -- spilled -- across the units)
  auto run_units = [&]() __attribute__((always_inline)) {
  if (nunits > 0) {
    int d = (woff - (int)(ulo - ubase)) % wstr;
    d = d < 0 ? d + wstr : d;
    i64 ucur = ulo + d;
    const i64 ustride = wstr;
    // (record addresses as base + 32-bit offset: one VGPR instead of a 64-bit address pair held across the unit's body)
    int urec = ucur < uhi ? mrec[(unsigned)(MARCH_REC * (int)ucur + lane)] : 0;
    for (; ucur < uhi; ucur += ustride) {
      const i64 un = ucur + ustride;
      const int urec_n = mrec[(unsigned)(MARCH_REC * (int)(un < uhi ? un : ucur) + lane)];   // the next unit's record is in flight meanwhile
      if (!(dbg & 16)) {
        const bool edge = rlane(urec, MARCH_EDGE + 1) > 0;
        if (((rlane(urec, 0) >> 8) & 255) == 7) {
          if (edge) march_dispatch<7, MODE, true, VT>(urec, lane, x, y, pa, pb, fin.pc0, fin.pc1, fin.pc2, acc0, acc1, acc2, dbg, e_val, sv, sx, p32, psig);
          else march_dispatch<7, MODE, false, VT>(urec, lane, x, y, pa, pb, fin.pc0, fin.pc1, fin.pc2, acc0, acc1, acc2, dbg, e_val, sv, sx, p32, psig);
        } else {
          if (edge) march_dispatch<5, MODE, true, VT>(urec, lane, x, y, pa, pb, fin.pc0, fin.pc1, fin.pc2, acc0, acc1, acc2, dbg, e_val, sv, sx, p32, psig);
          else march_dispatch<5, MODE, false, VT>(urec, lane, x, y, pa, pb, fin.pc0, fin.pc1, fin.pc2, acc0, acc1, acc2, dbg, e_val, sv, sx, p32, psig);
        }
      }
      urec = urec_n;
    }
  }
  };
  auto run_slices = [&]() __attribute__((always_inline)) {
  int ds_ = (woff - (int)(slo - sbase)) % wstr;
  ds_ = ds_ < 0 ? ds_ + wstr : ds_;
  const i64 first = slo + ds_, wstride = wstr, hi = shi;
  const i64 lastc = hi - 1;
  // the record of a slice is fetched with ONE vector load TWO slices ahead (lane l reads dword l & 31) and its
  // wave-uniform fields are broadcast with v_readlane
  int rec = first < hi ? srec[(unsigned)(SL_REC * (int)first + l31)] : 0;
  int rec_n = srec[(unsigned)(SL_REC * (int)(first + wstride < hi ? first + wstride : (first < hi ? lastc : 0)) + l31)];
  for (i64 chunk = first; chunk < hi; chunk += wstride) {
    const i64 cnn = chunk + 2 * wstride;
    const int rec_nn = srec[(unsigned)(SL_REC * (int)(cnn < hi ? cnn : lastc) + l31)];
    SDesc d;
    d.r0 = rlane(rec, 0); d.meta = rlane(rec, 1); d.base = rlane(rec, 2); d.aux = rlane(rec, 3);
    const int nrows = d.meta & 255, type = (d.meta >> 8) & 3, cnt = d.meta >> 16;
    const bool skip = ((dbg & 1) && type == SL_G) || ((dbg & 2) && type != SL_G);
    if (skip) {
    } else if (type == SL_U) {
      slice_dispatch<false, MODE, NT, VT>(cnt, d, nrows, rec, pval, x, y, pa, pb, lane, acc0, acc1, acc2, dbg, fin.pc0, fin.pc1, fin.pc2, p32, psig);
    } else if (type == SL_P) {
      slice_dispatch<true, MODE, NT, VT>(cnt, d, nrows, rec, pval, x, y, pa, pb, lane, acc0, acc1, acc2, dbg, fin.pc0, fin.pc1, fin.pc2, p32, psig);
    } else {
      // packed irregular rows: same data flow as k_spmv_cw on the compact CSR, plus the row-id indirection
      Desc dd;
      dd.r0 = d.r0; dd.base = d.base; dd.r1 = d.r0 + nrows; dd.end = d.aux;
      StreamW q;
      stream_issue_w<NT>(q, dd, g_rowptr, g_col, g_val, lane);
      const bool live = lane < nrows;
      const int rid = g_rowid[d.r0 + (live ? lane : 0)];
      const int basev = dd.base & ~1, basec = dd.base & ~3;
      const int av = q.ra - basev, ac = q.ra - basec, len = q.rb - q.ra;
#pragma unroll
      for (int j = 0; j < XV_IT; ++j) sv2[lane + 64 * j] = q.v[j];
      // the dot operands of the row ride with the gathers (issued before the LDS phase, not after it)
      const double opa = MI::HAS_A ? pa[rid] : 0.0, opb_ = (MI::HAS_B && !VT::P32) ? (double)pb[rid] : 0.0;
      const double xown = MI::OWN ? (double)x[rid] : 0.0;
      const double opb = VT::P32 ? xown : opb_;
      // ENTRY-parallel x gathers: lane l holds the columns of entries 4l..4l+3 (and 256 + 4l..), so neighbouring lanes
      // gather for the same or the next row and one gather instruction touches ~20 cache lines -- a row per lane (the CSR
      // kernel's way) touches 64, and the vector-memory unit serves a line per cycle.  The x values go to LDS next to the
      // matrix values; the row sums then read LDS only, in CSR entry order (bitwise the CSR kernels' result).
      double xg[XC_IT][4];
#pragma unroll
      for (int j = 0; j < XC_IT; ++j) {
        xg[j][0] = (double)x[q.c[j].x]; xg[j][1] = (double)x[q.c[j].y]; xg[j][2] = (double)x[q.c[j].z]; xg[j][3] = (double)x[q.c[j].w];
      }
#pragma unroll
      for (int j = 0; j < XC_IT; ++j) {
        d2_t lo2, hi2;
        lo2.x = xg[j][0]; lo2.y = xg[j][1]; hi2.x = xg[j][2]; hi2.y = xg[j][3];
        sx2[2 * (lane + 64 * j)] = lo2;
        sx2[2 * (lane + 64 * j) + 1] = hi2;
      }
      __builtin_amdgcn_wave_barrier();
      double sum = 0.0;
      int maxlen = len;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const int other = __shfl_xor(maxlen, off, 64);
        maxlen = other > maxlen ? other : maxlen;
      }
      maxlen = __builtin_amdgcn_readfirstlane(maxlen);
      for (int j0 = 0; j0 < maxlen; j0 += GUNR) {   // LDS reads of a round issued together
        double vv[GUNR], xv[GUNR];
#pragma unroll
        for (int j = 0; j < GUNR; ++j) {
          const int k = j0 + j < len ? j0 + j : 0;
          vv[j] = sv[av + k];
          xv[j] = sx[ac + k];
        }
#pragma unroll
        for (int j = 0; j < GUNR; ++j)
          if (j0 + j < len) sum += vv[j] * xv[j];
      }
      __builtin_amdgcn_wave_barrier();
      if (live) {
        sum = mode_out<MODE>(sum, xown, opb, fin.pc0, fin.pc1, fin.pc2);
        store_one_t(y + rid, sum);
        if (VT::P32) store_one_t(p32 + rid, psig * opb);
        if (MI::DOT0) acc0 += opa * sum;
        if (MI::DOT1) acc1 += sum * sum;
        if (MI::DOT2) acc2 += opb * sum;
      }
    }
    rec = rec_n;
    rec_n = rec_nn;
  }
  };
  if (DIAG && (dbg & 4096)) { run_slices(); run_units(); }   // (diagnostics, bit 4096: slices before units)
  else { run_units(); run_slices(); }
  }   // tiles
  // (write-through stores: the last block of this launch may read them, see fold_scalar_phase)
  // pstride = blocks per partial slot (the grid the Krylov workspace was sized for; >= gridDim.x).  accum: this launch
  // covers the rows left out by an earlier launch of the same product (spmv_with_halo: the rows that had to wait for
  // the halo) and adds its sums to that launch's -- which has completed: same stream.
  if (DOTS) {
    const double t0 = block_sum(acc0, s_red);
    if (threadIdx.x == 0) put_partial(partials + blockIdx.x, t0, accum);
  }
  if (MI::DOT1) {
    const double t1 = block_sum(acc1, s_red);
    if (threadIdx.x == 0) put_partial(partials + pstride + blockIdx.x, t1, accum);
  }
  if (MI::DOT2) {
    const double t2 = block_sum(acc2, s_red);
    if (threadIdx.x == 0) put_partial(partials + 4 * (size_t)pstride + blockIdx.x, t2, accum);
  }
  if (DOTS) fold_scalar_phase(fin, partials, s_red, pstride);
}

// flags[r]: bit 0 = row r has the count and (col - row) offsets of row r-1, bit 1 = and bitwise the same values,
// bit 2 = row r references a ghost column (col >= n: its product needs the halo exchange of x to have landed)
__global__ void k_row_same(i64 n, const int* __restrict__ rowptr, const int* __restrict__ col,
                           const double* __restrict__ val, unsigned char* __restrict__ flags) {
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) {
    unsigned char f = 0;
    bool ghost = false;
    for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) ghost = ghost || col[k] >= n;
    if (r > 0) {
      const int a = rowptr[r], b = rowptr[r + 1], pa = rowptr[r - 1];
      if (b - a == a - pa) {
        bool same = true, vsame = true;
        for (int k = 0; k < b - a; ++k) {
          same = same && (col[a + k] - 1 == col[pa + k]);
          vsame = vsame && (__double_as_longlong(val[a + k]) == __double_as_longlong(val[pa + k]));
        }
        f = same ? (vsame ? 3 : 1) : 0;
      }
    }
    flags[r] = f | (ghost ? 4 : 0);
  }
}

// P slices: pval[base + j*rows + l] = val[rowptr[r0+l] + j]
__global__ void k_pval_fill(i64 nslices, const int* __restrict__ srec, const int* __restrict__ rowptr,
                            const double* __restrict__ val, double* __restrict__ pval) {
  for (i64 sidx = blockIdx.x; sidx < nslices; sidx += gridDim.x) {
    const int r0 = srec[SL_REC * sidx], meta = srec[SL_REC * sidx + 1], base = srec[SL_REC * sidx + 2];
    if (((meta >> 8) & 3) != SL_P) continue;
    const int nrows = meta & 255, cnt = meta >> 16;
    for (int q = threadIdx.x; q < nrows * cnt; q += blockDim.x) {
      const int l = q / cnt, j = q % cnt;
      pval[(i64)base + (i64)j * nrows + l] = val[rowptr[r0 + l] + j];
    }
  }
}

// packed CSR of the irregular rows
__global__ void k_gpack(i64 ng, const int* __restrict__ g_rowid, const int* __restrict__ g_rowptr,
                        const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                        int* __restrict__ g_col, double* __restrict__ g_val) {
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < ng; q += (i64)gridDim.x * blockDim.x) {
    const int r = g_rowid[q], a = rowptr[r], len = rowptr[r + 1] - a, ga = g_rowptr[q];
    for (int k = 0; k < len; ++k) {
      g_col[ga + k] = col[a + k];
      if (g_val) g_val[ga + k] = val[a + k];   // (nullptr: the columns alone)
    }
  }
}

// offsets (dwords 4..11) and values (dwords 12..27) of every U / P record, from the slice's first row
__global__ void k_fill_records(i64 nslices, int* __restrict__ srec, const int* __restrict__ rowptr,
                               const int* __restrict__ col, const double* __restrict__ val) {
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < nslices; q += (i64)gridDim.x * blockDim.x) {
    int* rec = srec + SL_REC * q;
    const int type = (rec[1] >> 8) & 3;
    if (type == SL_G) continue;
    const int r = rec[0], a = rowptr[r], len = rowptr[r + 1] - a;
    for (int k = 0; k < SL_MAXCNT; ++k) {
      rec[4 + k] = col[a + (k < len ? k : 0)] - r;
      const double v = (k < len && type == SL_U) ? val[a + k] : 0.0;
      rec[12 + 2 * k] = __double2loint(v);
      rec[13 + 2 * k] = __double2hiint(v);
    }
  }
}

int variant() {
  // default 70 = stencil slices + non-temporal streams; 38 = the chunked CSR kernel + non-temporal streams; 1 = first kernel
  return config().spmv_variant;
}

int xcd_map() {
  return config().spmv_xcd;
}

}  // namespace
void ensure_csr_chunks(const CsrMatrix& A);
namespace {

#define PG_LAUNCH_C_ARGS(KERNEL, X, Y, AUX, PART)                                                               \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL), dim3(grid), dim3(BLOCK), 0, st, A.n, A.nchunks, A.chunk_desc.p, \
                     A.rowptr.p, A.col.p, A.val.p, X, Y, AUX, PART, (const double*)nullptr)
#define PG_LAUNCH_C(KERNEL)                                                                                    \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL), dim3(grid), dim3(BLOCK), 0, st, A.n, A.nchunks, A.chunk_desc.p, \
                     A.rowptr.p, A.col.p, A.val.p, x, y, aux, partials, sc)

// slices [s0, s0 + ns) of the slice image (the whole image: 0, A.nslices); `grid` blocks, partial slots `pstride` apart
template <int MODE>
bool launch_slices(int v, const CsrMatrix& A, i64 s0, i64 ns, const double* x, double* y, const double* aux, double* partials,
                   const double* sc, int grid, int pstride, int accum, hipStream_t st, const FinArgs* fin, bool units = true) {
  FinArgs fa{nullptr, nullptr, PH_NONE, 0, 0, nullptr};
  if (fin && MODE >= 1) fa = *fin;
  const int* rec = A.srec.p + SL_REC * s0;
  const i64 nu = units ? A.nunits : 0;   // the marching units ride with the launch that covers the interior slices
  const bool tiled = units && A.tiles_per_xcd > 0 && s0 == 0 && ns == A.tile_ns && (xcd_map() & 1) && grid >= 8;
  const int* tiles = tiled ? (const int*)A.tiles.p : nullptr;
  const int tpx = tiled ? A.tiles_per_xcd : 0;
  if (xcd_map() >= 256)   // diagnostic switches set: the diagnostic build (wrong products; ablation runs only)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_spmv_s<MODE, true, true>), dim3(grid), dim3(BLOCK), 0, st, ns, rec, A.pval.p,
                       A.g_rowid.p, A.g_rowptr.p, A.g_col.p, A.g_val.p, x, y, aux, partials, sc, xcd_map(), fa, pstride, accum,
                       (const int*)A.mrec.p, nu, tiles, tpx, (const double*)A.e_val.p);
  else if (v & 4)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_spmv_s<MODE, true, false>), dim3(grid), dim3(BLOCK), 0, st, ns, rec, A.pval.p,
                       A.g_rowid.p, A.g_rowptr.p, A.g_col.p, A.g_val.p, x, y, aux, partials, sc, xcd_map(), fa, pstride, accum,
                       (const int*)A.mrec.p, nu, tiles, tpx, (const double*)A.e_val.p);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_spmv_s<MODE, false, false>), dim3(grid), dim3(BLOCK), 0, st, ns, rec, A.pval.p,
                       A.g_rowid.p, A.g_rowptr.p, A.g_col.p, A.g_val.p, x, y, aux, partials, sc, xcd_map(), fa, pstride, accum,
                       (const int*)A.mrec.p, nu, tiles, tpx, (const double*)A.e_val.p);
  return fa.ticket != nullptr;
}

template <int MODE>
bool launch_mode(int v, const CsrMatrix& A, const double* x, double* y, const double* aux, double* partials,
                 const double* sc, int grid, hipStream_t st, const FinArgs* fin) {
  if (v & 64) return launch_slices<MODE>(v, A, 0, A.nslices, x, y, aux, partials, sc, grid, grid, 0, st, fin);
  PG_REQUIRE(MODE != 8 && !(fin && fin->dotx), "the preconditioner products and separate dot operands need the slice kernel");
  if (v != 1) ensure_csr_chunks(A);
  if (v == 1) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_spmv<MODE>), dim3(grid), dim3(BLOCK), 0, st, A.n, A.rowptr.p, A.col.p, A.val.p, x, y,
                       aux, partials, sc);
    return false;
  }
  // every other variant: the chunked CSR kernel (bit 2), with (bit 4) or without the non-temporal stream hint
  if (v & 4) PG_LAUNCH_C((k_spmv_cw<MODE, true>));
  else PG_LAUNCH_C((k_spmv_cw<MODE, false>));
  return false;
}

// the whole image as a Horner step with the element types VT (the shipped build of the kernel: stream hint, no diagnostics)
template <class VT>
void launch_typed(const CsrMatrix& A, const void* x, void* y, const double* sc, int grid, hipStream_t st, const FinArgs& fin) {
  const bool tiled = A.tiles_per_xcd > 0 && A.nslices == A.tile_ns && (xcd_map() & 1) && grid >= 8;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_spmv_s<8, true, false, VT>), dim3(grid), dim3(BLOCK), 0, st, A.nslices, (const int*)A.srec.p,
                     (const double*)A.pval.p, (const int*)A.g_rowid.p, (const int*)A.g_rowptr.p, (const int*)A.g_col.p,
                     (const double*)A.g_val.p, static_cast<const typename VT::TX*>(x), static_cast<typename VT::TY*>(y),
                     (const double*)nullptr, (double*)nullptr, sc, xcd_map(), fin, grid, 0, (const int*)A.mrec.p, A.nunits,
                     tiled ? (const int*)A.tiles.p : (const int*)nullptr, tiled ? A.tiles_per_xcd : 0, (const double*)A.e_val.p);
}

}  // namespace

bool spmv_supports_typed_chain() { return (variant() & 64) != 0 && (variant() & 4) != 0 && xcd_map() < 256; }

void launch_spmv_typed(int kind, const CsrMatrix& A, const void* x, void* y, const double* sc, int grid, hipStream_t st,
                       const FinArgs& fin) {
  if (A.n == 0) return;
  PG_REQUIRE(spmv_supports_typed_chain() && A.srec.p, "typed Horner launches need the slice kernel with the stream hint (PG_SPMV_VARIANT 70)");
  PG_REQUIRE(!fin.ticket && fin.base, "typed Horner launch: a base operand and no scalar phase");
  if (kind == TYPED_FIRST) {
    PG_REQUIRE(fin.p32 && x == (const void*)fin.base, "typed Horner launch (first): x = base and a p32 output");
    launch_typed<VecTypes<double, double, float, true>>(A, x, y, sc, grid, st, fin);
  } else if (kind == TYPED_MIDDLE) {
    launch_typed<VecTypes<float, float, float, false>>(A, x, y, sc, grid, st, fin);
  } else {
    PG_REQUIRE(kind == TYPED_HANDOVER, "unknown typed Horner launch");
    launch_typed<VecTypes<float, double, double, false>>(A, x, y, sc, grid, st, fin);
  }
}


namespace {

struct Slice {
  int r0, meta, base, aux;
  int key;   // first matrix row (sort key)
  int bnd;   // 1: some row references a ghost column (the slice waits for the halo exchange)
  i64 okey = 0;   // place in the order of the work items (march_order of the first row's cell, then the row)
};

using pghost::MRun;   // rows [r0, r0 + len) with one stencil (offsets and values), cnt = 5 / 7 entries

constexpr int RUN_INFO = 25;   // dwords per run: 8 offsets, 8 values (lo, hi), grid cell of the first row (-1: unknown)

// col - row offsets and values of the first row of every run
__global__ void k_run_info(i64 nruns, const int* __restrict__ run_r0, const int* __restrict__ rowptr,
                           const int* __restrict__ col, const double* __restrict__ val, const int* __restrict__ cell,
                           const int* __restrict__ map, int* __restrict__ out) {
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < nruns; q += (i64)gridDim.x * blockDim.x) {
    const int r = run_r0[q], a = rowptr[r], len = rowptr[r + 1] - a;
    out[RUN_INFO * q + 24] = cell ? cell[map ? map[r] : r] : -1;
    for (int k = 0; k < 8; ++k) {
      out[RUN_INFO * q + k] = k < len ? col[a + k] - r : 0;
      const double v = k < len ? val[a + k] : 0.0;
      out[RUN_INFO * q + 8 + 2 * k] = __double2loint(v);
      out[RUN_INFO * q + 9 + 2 * k] = __double2hiint(v);
    }
  }
}

// values (dwords 2..15) of every unit record from its first computed row (dword 1)
__global__ void k_fill_units(i64 nunits, int* __restrict__ mrec, const int* __restrict__ rowptr,
                             const double* __restrict__ val) {
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < nunits; q += (i64)gridDim.x * blockDim.x) {
    int* rec = mrec + MARCH_REC * q;
    const int cnt = (rec[0] >> 8) & 255, a = rowptr[rec[1]];
    for (int k = 0; k < cnt; ++k) {
      rec[2 + 2 * k] = __double2loint(val[a + k]);
      rec[3 + 2 * k] = __double2hiint(val[a + k]);
    }
  }
}

// value stream of the edge rows (pghost::EdgePlan::meta: row, slot 0, distance between pairs of slots, slot per entry): +0.0
// where the row has no entry
__global__ void k_fill_edges(i64 ne, const int* __restrict__ meta, const int* __restrict__ rowptr, const double* __restrict__ val,
                             double* __restrict__ e_val) {
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < ne; q += (i64)gridDim.x * blockDim.x) {
    const int r = meta[4 * q], dst = meta[4 * q + 1], dist = meta[4 * q + 2], sm = meta[4 * q + 3];
    const int a = rowptr[r], len = sm >> 24;
    for (int j = 0; j < MARCH_ESLOTS; ++j) e_val[dst + (i64)(j >> 1) * dist + (j & 1)] = 0.0;
    for (int k = 0; k < len; ++k) {
      const int j = (sm >> (3 * k)) & 7;
      e_val[dst + (i64)(j >> 1) * dist + (j & 1)] = val[a + k];
    }
  }
}

// do the edge rows of T's image have T's columns in A as well?
__global__ void k_edges_invalid(i64 ne, const int* __restrict__ meta, const int* __restrict__ rowptr_t, const int* __restrict__ col_t,
                                const int* __restrict__ rowptr, const int* __restrict__ col, unsigned long long* __restrict__ out) {
  unsigned long long c = 0;
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < ne; q += (i64)gridDim.x * blockDim.x) {
    const int r = meta[4 * q], a = rowptr[r], at = rowptr_t[r], len = rowptr[r + 1] - a;
    bool same = len == rowptr_t[r + 1] - at && len == (meta[4 * q + 3] >> 24);
    for (int k = 0; same && k < len; ++k) same = col[a + k] == col_t[at + k];
    c += same ? 0 : 1;
  }
  if (c) atomicAdd(out, c);
}

// do the rows of every unit still share one stencil?  (rows after the first of a plane repeat their predecessor --
// row flags -- and the first row of every plane carries the values of the unit's first row)
__global__ void k_units_invalid(i64 nunits, const int* __restrict__ mrec, const int* __restrict__ rowptr,
                                const double* __restrict__ val, const unsigned char* __restrict__ flags,
                                unsigned long long* __restrict__ out) {
  unsigned long long c = 0;
  for (i64 q = blockIdx.x; q < nunits; q += gridDim.x) {
    const int* rec = mrec + MARCH_REC * q;
    const int K = rec[0] & 255, cnt = (rec[0] >> 8) & 255, a0 = rowptr[rec[1]];
    for (int i = 0; i < K; ++i) {
      const int rb = rec[18 + 4 * i], lo = rec[21 + 4 * i] & 255, hi = rec[21 + 4 * i] >> 8;
      for (int l = lo + threadIdx.x; l < hi; l += blockDim.x) {
        const int r = rb + l;
        if (l > lo) {
          c += (flags[r] & 3) != 3 ? 1 : 0;
        } else {
          const int a = rowptr[r];
          bool same = rowptr[r + 1] - a == cnt;
          for (int k = 0; same && k < cnt; ++k)
            same = __double_as_longlong(val[a + k]) == __double_as_longlong(val[a0 + k]);
          c += same ? 0 : 1;
        }
      }
    }
  }
  if (c) atomicAdd(out, c);
}

__global__ void k_row_cells(i64 nrows, const int* __restrict__ rows, const int* __restrict__ cell, const int* __restrict__ map,
                            int* __restrict__ out) {
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < nrows; q += (i64)gridDim.x * blockDim.x) {
    const int r = rows[q];
    out[q] = cell[map ? map[r] : r];
  }
}

int march_strip() {
  return config().spmv_strip;
}
bool has_geo(const CsrMatrix& A) { return A.geo_cell && A.geo_ext0 > 0 && A.geo_lines > 0 && march_strip() > 0; }

// march_order of the given rows (0 for all without grid geometry)
std::vector<i64> row_orders(const CsrMatrix& A, const std::vector<int>& rows) {
  std::vector<i64> ord(rows.size(), 0);
  if (!has_geo(A) || rows.empty()) return ord;
  const i64 nr = (i64)rows.size();
  DevBuf<int> d_rows(nr), d_cells(nr);
  d_rows.upload(rows.data(), nr);
  hipLaunchKernelGGL(k_row_cells, dim3(grid_for(nr, 256)), dim3(256), 0, ctx().stream, nr, d_rows.p, A.geo_cell, A.geo_map, d_cells.p);
  PG_HIP(hipGetLastError());
  std::vector<int> cells(rows.size());
  d_cells.download(cells.data(), nr);
  for (i64 q = 0; q < nr; ++q) ord[q] = pghost::march_order(cells[q], A.geo_ext0, A.geo_lines, march_strip());
  return ord;
}

void emit_u_rows(std::vector<Slice>& up, i64 a, i64 b, int cnt) {
  for (i64 r = a; r < b; r += SL_MAXROWS_U) {
    const int rows = (int)std::min<i64>(SL_MAXROWS_U, b - r);
    up.push_back(Slice{(int)r, rows | (SL_U << 8) | (cnt << 16), 0, 0, (int)r, 0});
  }
}

// Chains of runs -> unit records: the planning itself is plain host code (pg_host_algos.h: also compiled, with
// AddressSanitizer / UBSan, into the CPU test-suite); here: the run descriptors come from the device and the result goes
// back.  Rows that cannot march are appended to `up` as U slices.
void build_march_units(CsrMatrix& A, const std::vector<MRun>& runs, std::vector<int>& mrec, std::vector<Slice>& up,
                       std::vector<i64>& ukeys, pghost::EdgePlan* edges) {
  A.rows_m = 0;
  const i64 nr = (i64)runs.size();
  if (nr == 0) return;
  hipStream_t st = ctx().stream;
  std::vector<int> info((size_t)RUN_INFO * nr);
  {
    std::vector<int> r0s(nr);
    for (i64 i = 0; i < nr; ++i) r0s[i] = runs[i].r0;
    DevBuf<int> d_r0(nr), d_info(RUN_INFO * nr);
    d_r0.upload(r0s.data(), nr);
    hipLaunchKernelGGL(k_run_info, dim3(grid_for(nr, 256)), dim3(256), 0, st, nr, d_r0.p, A.rowptr.p, A.col.p, A.val.p,
                       A.geo_cell, A.geo_map, d_info.p);
    PG_HIP(hipGetLastError());
    d_info.download(info.data(), RUN_INFO * nr);
  }
  const int kmax = config().spmv_march_k > 0 ? std::max(1, std::min(MARCH_K, config().spmv_march_k)) : MARCH_K;
  pghost::MarchGeometry geo{MARCH_K, MARCH_KS, MARCH_REC, MARCH_W, RUN_INFO, kmax, A.geo_ext0, A.geo_lines, march_strip(),
                            has_geo(A) ? config().unit_order : 0};
  std::vector<pghost::RowRange> fallback;
  i64 rows_m = 0;
  pghost::plan_march_units(A.n, runs, info, geo, mrec, fallback, rows_m, &ukeys, edges);
  A.rows_m = rows_m;
  for (const auto& f : fallback) emit_u_rows(up, f.a, f.b, f.cnt);
}

// stencil-slice image of A (see "stencil slices" above); rp = host copy of A.rowptr
void build_slices(CsrMatrix& A, const int* rp) {
  hipStream_t st = ctx().stream;
  Laps laps;
  const i64 n = A.n;
  const int minrun = config().spmv_minrun;
  unsigned char* fl = static_cast<unsigned char*>(pinned_scratch(1, (size_t)n));
  A.rowflags.alloc(n);
  hipLaunchKernelGGL(k_row_same, dim3(grid_for(n, 256, 256 * 16)), dim3(256), 0, st, n, A.rowptr.p, A.col.p, A.val.p,
                     A.rowflags.p);
  PG_HIP(hipGetLastError());
  A.rowflags.download(fl, n);
  laps.lap("    slices: row flags");
  // run classification over [lo, hi) (lo, hi on pattern-run boundaries): independent per range, so the 10^7-row
  // sweep is split over a few host threads and the pieces are concatenated in row order
  struct Part {
    std::vector<Slice> up;      // U and P slices
    std::vector<int> grows;     // irregular rows, ascending
    std::vector<MRun> runs;     // U runs of 2-D / 3-D stencil rows: candidates for marching units
    i64 rows_u = 0, rows_p = 0, nnz_p = 0;
  };
  const bool march_env = config().spmv_march;
  const bool march_on = march_env && A.want_units;
  auto classify = [&](i64 lo, i64 hi, Part& out) {
    auto emit = [&](int type, i64 a, i64 b, int cnt) {
      if (march_on && type == SL_U && (cnt == 5 || cnt == 7)) {
        // a piece of a grid line with one stencil: kept whole, turned into marching units (or U slices) below
        bool ghost = false;
        for (i64 q = a; q < b; ++q) ghost = ghost || ((fl[q] >> 2) & 1);
        if (!ghost) {
          out.runs.push_back(MRun{(int)a, (int)(b - a), cnt});
          out.rows_u += b - a;
          return;
        }
      }
      const i64 maxrows = type == SL_U ? SL_MAXROWS_U : SL_MAXROWS_P;
      for (i64 r = a; r < b; r += maxrows) {
        const int rows = (int)std::min<i64>(maxrows, b - r);
        int bnd = 0;
        for (i64 q = r; q < r + rows; ++q) bnd |= (fl[q] >> 2) & 1;
        out.up.push_back(Slice{(int)r, rows | (type << 8) | (cnt << 16), 0, 0, (int)r, bnd});
      }
      (type == SL_U ? out.rows_u : out.rows_p) += b - a;
      if (type == SL_P) out.nnz_p += (b - a) * cnt;
    };
    auto irregular = [&](i64 a, i64 b) {
      for (i64 r = a; r < b; ++r) out.grows.push_back((int)r);
    };
    i64 i = lo;
    while (i < hi) {
      i64 j = i + 1;
      while (j < n && (fl[j] & 1)) ++j;                 // pattern run [i, j)
      const int cnt = rp[i + 1] - rp[i];
      if (j - i >= minrun && cnt >= 1 && cnt <= SL_MAXCNT) {   // rows with more entries than a record holds stay irregular
        i64 pstart = i, k = i;
        auto flush_p = [&](i64 a, i64 b) {
          if (b - a >= minrun) emit(SL_P, a, b, cnt);
          else irregular(a, b);
        };
        while (k < j) {
          i64 m = k + 1;
          while (m < j && (fl[m] & 2)) ++m;             // value run [k, m)
          if (m - k >= minrun) {
            flush_p(pstart, k);
            emit(SL_U, k, m, cnt);
            pstart = m;
          }
          k = m;
        }
        flush_p(pstart, j);
      } else {
        irregular(i, j);
      }
      i = j;
    }
  };
  const int nthreads = n > (i64)1 << 20 ? (int)std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency())) : 1;
  std::vector<i64> cut(nthreads + 1, n);
  cut[0] = 0;
  for (int t = 1; t < nthreads; ++t) {
    i64 c = n * t / nthreads;
    while (c < n && (fl[c] & 1)) ++c;   // move to the start of a pattern run
    cut[t] = std::max(c, cut[t - 1]);
  }
  std::vector<Part> parts(nthreads);
  if (nthreads == 1) {
    classify(0, n, parts[0]);
  } else {
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t) th.emplace_back([&, t] { classify(cut[t], cut[t + 1], parts[t]); });
    for (auto& x : th) x.join();
  }
  std::vector<Slice> up;
  std::vector<int> grows;
  std::vector<MRun> runs;
  A.rows_u = A.rows_p = A.rows_g = A.nnz_p = A.nnz_g = 0;
  {
    size_t nu = 0, ngr = 0, nr = 0;
    for (auto& pt : parts) { nu += pt.up.size(); ngr += pt.grows.size(); nr += pt.runs.size(); }
    up.reserve(nu);
    grows.reserve(ngr);
    runs.reserve(nr);
    for (auto& pt : parts) {
      up.insert(up.end(), pt.up.begin(), pt.up.end());
      grows.insert(grows.end(), pt.grows.begin(), pt.grows.end());
      runs.insert(runs.end(), pt.runs.begin(), pt.runs.end());
      A.rows_u += pt.rows_u; A.rows_p += pt.rows_p; A.nnz_p += pt.nnz_p;
    }
  }
  laps.lap("    slices: host classification");
  // marching units out of the stencil runs; what cannot march comes back as U slices
  std::vector<int> mrec;
  std::vector<i64> ukeys;
  // the irregular rows are the candidates for edge rows: their columns, as a compact CSR (the rows arrive in ascending order)
  pghost::EdgePlan edges;
  std::vector<int> c_ptr, c_col;
  if (!runs.empty() && !grows.empty() && config().spmv_edges) {
    const i64 nc = (i64)grows.size();
    c_ptr.assign(nc + 1, 0);
    for (i64 q = 0; q < nc; ++q) c_ptr[q + 1] = c_ptr[q] + (rp[grows[q] + 1] - rp[grows[q]]);
    c_col.resize((size_t)c_ptr[nc] + 1);
    DevBuf<int> d_rows(nc), d_ptr(nc + 1), d_col(c_ptr[nc] + 8);
    d_rows.upload(grows.data(), nc);
    d_ptr.upload(c_ptr.data(), nc + 1);
    hipLaunchKernelGGL(k_gpack, dim3(grid_for(nc, 256)), dim3(256), 0, st, nc, d_rows.p, d_ptr.p, A.rowptr.p, A.col.p, A.val.p,
                       d_col.p, (double*)nullptr);
    PG_HIP(hipGetLastError());
    if (c_ptr[nc] > 0) d_col.download(c_col.data(), c_ptr[nc]);
    edges.cand = pghost::EdgeCands{grows.data(), nc, c_ptr.data(), c_col.data()};
  }
  build_march_units(A, runs, mrec, up, ukeys, &edges);
  A.rows_e = edges.rows_e;
  A.e_slots = edges.slots_read;
  A.e_meta.alloc(std::max<i64>((i64)edges.meta.size(), 1));
  A.e_val.alloc((i64)MARCH_ESLOTS * A.rows_e + 8);
  A.e_val.zero();
  if (A.rows_e > 0) {
    A.e_meta.upload(edges.meta.data(), (i64)edges.meta.size());
    hipLaunchKernelGGL(k_fill_edges, dim3(grid_for(A.rows_e, 256)), dim3(256), 0, st, A.rows_e, (const int*)A.e_meta.p, A.rowptr.p,
                       A.val.p, A.e_val.p);
    PG_HIP(hipGetLastError());
    // they leave the irregular rows
    std::vector<int> er((size_t)A.rows_e);
    for (i64 q = 0; q < A.rows_e; ++q) er[q] = edges.meta[4 * q];
    std::sort(er.begin(), er.end());
    size_t w = 0;
    for (size_t q = 0; q < grows.size(); ++q)
      if (!std::binary_search(er.begin(), er.end(), grows[q])) grows[w++] = grows[q];
    grows.resize(w);
  }
  A.nunits = (i64)mrec.size() / MARCH_REC;
  A.mrec.alloc(std::max<i64>((i64)mrec.size(), 1));
  if (!mrec.empty()) A.mrec.upload(mrec.data(), (i64)mrec.size());
  laps.lap("    slices: marching units");
  // P value bases
  {
    i64 pbase = 0;
    for (auto& sl : up) {
      if (((sl.meta >> 8) & 3) != SL_P) continue;
      const int rows = sl.meta & 255, cnt = sl.meta >> 16;
      PG_REQUIRE(pbase + (i64)rows * cnt < (i64)2147483647, "P-slice value array exceeds int32 indexing");
      sl.base = (int)pbase;
      pbase += (i64)rows * cnt;
    }
  }
  A.pval.alloc(A.nnz_p + 8);
  // packed CSR of the irregular rows + its chunks: the rows that reference a ghost column go last, so that no chunk
  // mixes rows that can be multiplied before the halo has landed with rows that cannot
  // ... in the order of the work items (strip of lines, plane, row: the chunks of a tile gather x where the tile's units
  // have just read it) -- a counting sort, the rows arrive in ascending order
  std::vector<i64> g_ord = row_orders(A, grows);
  if (has_geo(A) && !grows.empty()) {
    std::vector<i64> uniq(g_ord);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    std::vector<i64> start(uniq.size() + 1, 0);
    std::vector<int> bucket(grows.size());
    for (size_t q = 0; q < grows.size(); ++q) {
      bucket[q] = (int)(std::lower_bound(uniq.begin(), uniq.end(), g_ord[q]) - uniq.begin());
      ++start[bucket[q] + 1];
    }
    for (size_t b = 0; b < uniq.size(); ++b) start[b + 1] += start[b];
    std::vector<int> sorted(grows.size());
    std::vector<i64> sorted_ord(grows.size());
    for (size_t q = 0; q < grows.size(); ++q) {
      const i64 pos = start[bucket[q]]++;
      sorted[pos] = grows[q];
      sorted_ord[pos] = g_ord[q];
    }
    grows.swap(sorted);
    g_ord.swap(sorted_ord);
  }
  {   // (the order keys travel with the rows through the partition)
    std::vector<std::pair<int, i64>> both(grows.size());
    for (size_t q = 0; q < grows.size(); ++q) both[q] = {grows[q], g_ord[q]};
    std::stable_partition(both.begin(), both.end(), [&](const std::pair<int, i64>& e) { return (fl[e.first] & 4) == 0; });
    for (size_t q = 0; q < grows.size(); ++q) { grows[q] = both[q].first; g_ord[q] = both[q].second; }
  }
  const i64 ng = (i64)grows.size();
  i64 ng_int = 0;
  while (ng_int < ng && (fl[grows[ng_int]] & 4) == 0) ++ng_int;
  A.rows_g = ng;
  std::vector<int> grp(ng + 1, 0);
  for (i64 q = 0; q < ng; ++q) grp[q + 1] = grp[q] + (rp[grows[q] + 1] - rp[grows[q]]);
  A.nnz_g = grp[ng];
  A.g_rowid.alloc(ng > 0 ? ng : 1);
  A.g_rowptr.alloc(ng + 1);
  A.g_col.alloc(A.nnz_g + 8);
  A.g_val.alloc(A.nnz_g + 8);
  A.g_col.zero();
  A.g_val.zero();
  A.g_rowptr.upload(grp.data(), ng + 1);
  {
    std::vector<int> firsts(up.size());
    for (size_t q = 0; q < up.size(); ++q) firsts[q] = up[q].key;
    const std::vector<i64> ord = row_orders(A, firsts);
    for (size_t q = 0; q < up.size(); ++q) up[q].okey = ord[q] * ((i64)1 << 32) + up[q].key;
  }
  std::vector<Slice> all(up);
  if (ng > 0) {
    A.g_rowid.upload(grows.data(), ng);
    hipLaunchKernelGGL(k_gpack, dim3(grid_for(ng, 256)), dim3(256), 0, st, ng, A.g_rowid.p, A.g_rowptr.p, A.rowptr.p, A.col.p,
                       A.val.p, A.g_col.p, A.g_val.p);
    PG_HIP(hipGetLastError());
    i64 q = 0;
    while (q < ng) {
      i64 e = q + 1;
      PG_REQUIRE(grp[e] - grp[q] <= SPMV_CHUNK_ENTRIES, "CSR row longer than an SpMV chunk");
      const i64 stop = q < ng_int ? ng_int : ng;   // chunks end at the interior / boundary seam
      while (e < stop && e - q < 64 && grp[e + 1] - grp[q] <= SPMV_CHUNK_ENTRIES) ++e;
      all.push_back(Slice{(int)q, (int)(e - q) | (SL_G << 8), grp[q], grp[e], grows[q], q >= ng_int ? 1 : 0,
                          g_ord[q] * ((i64)1 << 32) + grows[q]});
      q = e;
    }
  }
  // by first row within each group; the slices that wait for the halo form the tail [nslices_int, nslices)
  std::stable_sort(all.begin(), all.end(), [](const Slice& a, const Slice& b) { return a.bnd != b.bnd ? a.bnd < b.bnd : a.okey < b.okey; });
  A.nslices = (i64)all.size();
  A.nslices_int = 0;
  while (A.nslices_int < A.nslices && !all[A.nslices_int].bnd) ++A.nslices_int;
  // tiles (PG_SPMV_TILE_UNITS = units per tile, e.g. 512 = one per resident wave of an XCD; default off): measured at
  // 512^3, tiles of 512 units take 5 MB off the 159 MB a lean launch reads but cost 6 us of its 45 -- a wave then has one
  // unit and about one slice per tile and nothing to prefetch the next record behind
  {
    const int tile_units = config().spmv_tile_units;
    const i64 T = tile_units > 0 ? std::min<i64>(256, (A.nunits / 8 + tile_units / 2) / tile_units) : 0;
    A.tiles_per_xcd = 0;
    A.tile_ns = 0;
    A.tiles.release();
    if (T >= 2 && A.nslices_int > 0 && (i64)ukeys.size() == A.nunits) {
      std::vector<i64> skeys((size_t)A.nslices_int);
      for (i64 q = 0; q < A.nslices_int; ++q) skeys[q] = all[q].okey;
      std::vector<int> tab;
      pghost::plan_tiles(ukeys, skeys, (int)T, tab);
      A.tiles.alloc((i64)tab.size());
      A.tiles.upload(tab.data(), (i64)tab.size());
      A.tiles_per_xcd = (int)T;
      A.tile_ns = A.nslices_int;
    }
  }
  std::vector<int> sd(SL_REC * (A.nslices + 1), 0);
  for (i64 q = 0; q < A.nslices; ++q) {
    int* rec = sd.data() + SL_REC * q;
    rec[0] = all[q].r0; rec[1] = all[q].meta; rec[2] = all[q].base; rec[3] = all[q].aux;
  }
  A.srec.alloc((i64)sd.size());
  A.srec.upload(sd.data(), (i64)sd.size());
  if (A.nslices > 0) {
    hipLaunchKernelGGL(k_fill_records, dim3(grid_for(A.nslices, 256)), dim3(256), 0, st, A.nslices, A.srec.p, A.rowptr.p, A.col.p,
                       A.val.p);
    PG_HIP(hipGetLastError());
  }
  if (A.nnz_p > 0) {
    hipLaunchKernelGGL(k_pval_fill, dim3((unsigned)std::min<i64>(A.nslices, 65535)), dim3(256), 0, st, A.nslices, A.srec.p,
                       A.rowptr.p, A.val.p, A.pval.p);
    PG_HIP(hipGetLastError());
  }
  PG_HIP(hipStreamSynchronize(st));
  laps.lap("    slices: packing + records");
  A.spmv_bytes = 4 * SL_REC * A.nslices + 4 * MARCH_REC * A.nunits + 8 * A.nnz_p + 12 * A.nnz_g + 8 * ng + 8 * A.e_slots + 16 * n;
  if (config().debug)
    fprintf(stderr, "[pg_spmv] slices %lld (%lld wait for the halo), marching units %lld (%lld rows, %lld edge rows): rows U %lld P %lld G %lld of %lld; nnz P %lld G %lld of %lld; bytes/launch %lld (CSR %lld)\n",
            (long long)A.nslices, (long long)(A.nslices - A.nslices_int), (long long)A.nunits, (long long)A.rows_m, (long long)A.rows_e, (long long)A.rows_u, (long long)A.rows_p, (long long)A.rows_g,
            (long long)n, (long long)A.nnz_p, (long long)A.nnz_g, (long long)A.nnz, (long long)A.spmv_bytes,
            (long long)(12 * A.nnz + 20 * n));
}

}  // namespace

// rows -> chunks of <= 64 rows and <= SPMV_CHUNK_ENTRIES entries for the plain-CSR kernels (greedy, host side).  Only
// the CSR variants need it: built on first use.
void ensure_csr_chunks(const CsrMatrix& Ac) {
  CsrMatrix& A = const_cast<CsrMatrix&>(Ac);
  if (A.chunk_desc.p || A.n == 0) return;
  std::vector<int> rp(A.n + 1);
  A.rowptr.download(rp.data(), A.n + 1);
  std::vector<int> cd;   // {first row, first entry} per chunk, closed by {n, nnz}; padded for the 4-int descriptor read
  cd.reserve(2 * (A.n / 60 + 16));
  i64 r = 0;
  while (r < A.n) {
    i64 e = r + 1;   // a chunk holds at least one row (rows never exceed the slice: <= 4(2N+1) entries)
    PG_REQUIRE(rp[e] - rp[r] <= SPMV_CHUNK_ENTRIES, "CSR row longer than an SpMV chunk");
    while (e < A.n && e - r < 64 && rp[e + 1] - rp[r] <= SPMV_CHUNK_ENTRIES) ++e;
    cd.push_back((int)r);
    cd.push_back(rp[r]);
    r = e;
  }
  A.nchunks = (i64)cd.size() / 2;
  cd.push_back((int)A.n);
  cd.push_back(rp[A.n]);
  cd.push_back((int)A.n);   // pad
  cd.push_back(rp[A.n]);
  A.chunk_desc.alloc((i64)cd.size());
  A.chunk_desc.upload(cd.data(), (i64)cd.size());
}

// SpMV image of a freshly assembled matrix (once per matrix)
void build_spmv_chunks(CsrMatrix& A) {
  Laps laps;
  int* rp = static_cast<int*>(pinned_scratch(0, sizeof(int) * (size_t)(A.n + 1)));
  A.rowptr.download(rp, A.n + 1);
  laps.lap("    chunks: rowptr download");
  A.chunk_desc.release();
  A.nchunks = 0;
  build_slices(A, rp);
}

// do the new row flags still support every slice?  (U: rows 2.. repeat offsets and values; P: offsets.)  More repetition
// than before is fine -- it is just not exploited; rows outside the slices (G) need nothing.
__global__ void k_slices_invalid(i64 nslices, const int* __restrict__ srec, const unsigned char* __restrict__ flags,
                                 unsigned long long* __restrict__ out) {
  unsigned long long c = 0;
  for (i64 q = blockIdx.x; q < nslices; q += gridDim.x) {
    const int r0 = srec[SL_REC * q], meta = srec[SL_REC * q + 1];
    const int nrows = meta & 255, type = (meta >> 8) & 3;
    const unsigned char need = type == SL_U ? 3 : 1;
    for (int l = 1 + threadIdx.x; l < nrows; l += blockDim.x) c += (flags[r0 + l] & need) != need ? 1 : 0;
  }
  if (c) atomicAdd(out, c);
}

template <class T>
static void clone_buf(DevBuf<T>& dst, const DevBuf<T>& src, hipStream_t st) {
  dst.alloc(src.n > 0 ? src.n : 1);
  if (src.n > 0) PG_HIP(hipMemcpyAsync(dst.p, src.p, sizeof(T) * (size_t)src.n, hipMemcpyDeviceToDevice, st));
}

bool build_slices_like(const CsrMatrix& T, CsrMatrix& A) {
  hipStream_t st = ctx().stream;
  const i64 n = A.n;
  if (!T.rowflags.p || T.n != n || !T.srec.p) return false;
  A.rowflags.alloc(n);
  DevBuf<unsigned long long> diff(1);
  diff.zero();
  hipLaunchKernelGGL(k_row_same, dim3(grid_for(n, 256, 256 * 16)), dim3(256), 0, st, n, A.rowptr.p, A.col.p, A.val.p,
                     A.rowflags.p);
  if (T.nslices > 0)
    hipLaunchKernelGGL(k_slices_invalid, dim3((unsigned)std::min<i64>(T.nslices, 16384)), dim3(64), 0, st, T.nslices, T.srec.p,
                       A.rowflags.p, diff.p);
  if (T.nunits > 0)
    hipLaunchKernelGGL(k_units_invalid, dim3((unsigned)std::min<i64>(T.nunits, 16384)), dim3(64), 0, st, T.nunits, T.mrec.p,
                       A.rowptr.p, A.val.p, A.rowflags.p, diff.p);
  if (T.rows_e > 0)
    hipLaunchKernelGGL(k_edges_invalid, dim3(grid_for(T.rows_e, 256)), dim3(256), 0, st, T.rows_e, (const int*)T.e_meta.p,
                       (const int*)T.rowptr.p, (const int*)T.col.p, (const int*)A.rowptr.p, (const int*)A.col.p, diff.p);
  PG_HIP(hipGetLastError());
  unsigned long long h = 0;
  diff.download(&h, 1);
  if (h != 0) return false;
  // every slice still holds: copy the structure, refill the values
  A.chunk_desc.release();
  A.nchunks = 0;
  A.nslices = T.nslices;
  A.nslices_int = T.nslices_int;
  A.rows_u = T.rows_u; A.rows_p = T.rows_p; A.rows_g = T.rows_g; A.nnz_p = T.nnz_p; A.nnz_g = T.nnz_g;
  A.spmv_bytes = T.spmv_bytes;
  A.nunits = T.nunits; A.rows_m = T.rows_m;
  A.tiles_per_xcd = T.tiles_per_xcd; A.tile_ns = T.tile_ns;
  if (T.tiles_per_xcd > 0) clone_buf(A.tiles, T.tiles, st);
  else A.tiles.release();
  clone_buf(A.mrec, T.mrec, st);
  if (A.nunits > 0)
    hipLaunchKernelGGL(k_fill_units, dim3(grid_for(A.nunits, 256)), dim3(256), 0, st, A.nunits, A.mrec.p, A.rowptr.p, A.val.p);
  A.rows_e = T.rows_e; A.e_slots = T.e_slots;
  clone_buf(A.e_meta, T.e_meta, st);
  A.e_val.alloc((i64)MARCH_ESLOTS * A.rows_e + 8);
  A.e_val.zero();
  if (A.rows_e > 0)
    hipLaunchKernelGGL(k_fill_edges, dim3(grid_for(A.rows_e, 256)), dim3(256), 0, st, A.rows_e, (const int*)A.e_meta.p, A.rowptr.p,
                       A.val.p, A.e_val.p);
  clone_buf(A.srec, T.srec, st);
  clone_buf(A.g_rowid, T.g_rowid, st);
  clone_buf(A.g_rowptr, T.g_rowptr, st);
  A.pval.alloc(A.nnz_p + 8);
  A.g_col.alloc(A.nnz_g + 8);
  A.g_val.alloc(A.nnz_g + 8);
  A.g_col.zero();
  A.g_val.zero();
  if (A.nslices > 0)
    hipLaunchKernelGGL(k_fill_records, dim3(grid_for(A.nslices, 256)), dim3(256), 0, st, A.nslices, A.srec.p, A.rowptr.p, A.col.p,
                       A.val.p);
  if (A.nnz_p > 0)
    hipLaunchKernelGGL(k_pval_fill, dim3((unsigned)std::min<i64>(A.nslices, 65535)), dim3(256), 0, st, A.nslices, A.srec.p,
                       A.rowptr.p, A.val.p, A.pval.p);
  if (A.rows_g > 0)
    hipLaunchKernelGGL(k_gpack, dim3(grid_for(A.rows_g, 256)), dim3(256), 0, st, A.rows_g, A.g_rowid.p, A.g_rowptr.p, A.rowptr.p,
                       A.col.p, A.val.p, A.g_col.p, A.g_val.p);
  PG_HIP(hipGetLastError());
  PG_HIP(hipStreamSynchronize(st));
  return true;
}

bool spmv_supports_preconditioner_product() { return (variant() & 64) != 0; }

int spmv_default_grid(i64 n) {
  // resident blocks per CU: the slice kernel holds ~100 VGPRs (4 waves / SIMD), the CSR kernels 24.6 KB of LDS (6 blocks)
  const int per_cu = config().spmv_blocks_per_cu > 0 ? config().spmv_blocks_per_cu : ((variant() & 64) ? 4 : 6);
  static int cus = 0;
  if (cus == 0) {
    hipDeviceProp_t prop;
    cus = 256;
    if (hipGetDeviceProperties(&prop, ctx().device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
  }
  return grid_for(n, BLOCK, cus * per_cu);
}

// the launch of mode `mode` with kernel variant v: the one body of launch_spmv and launch_spmv_as
static inline __attribute__((always_inline)) bool launch_by_mode(int v, int mode, const CsrMatrix& A, const double* x, double* y,
                                                                 const double* aux, double* partials, const double* sc, int grid,
                                                                 hipStream_t st, const FinArgs* fin) {
  if (mode == 0) return launch_mode<0>(v, A, x, y, aux, partials, sc, grid, st, fin);
  if (mode == 1) return launch_mode<1>(v, A, x, y, aux, partials, sc, grid, st, fin);
  if (mode == 2) return launch_mode<2>(v, A, x, y, aux, partials, sc, grid, st, fin);
  if (mode == 8) return launch_mode<8>(v, A, x, y, aux, partials, sc, grid, st, fin);
  PG_REQUIRE(mode == 3, "unknown SpMV launch mode");
  return launch_mode<3>(v, A, x, y, aux, partials, sc, grid, st, fin);
}

bool launch_spmv(int mode, const CsrMatrix& A, const double* x, double* y, const double* aux, double* partials,
                 const double* sc, int grid, hipStream_t st, const FinArgs* fin) {
  if (A.n == 0) return false;
  return launch_by_mode(variant(), mode, A, x, y, aux, partials, sc, grid, st, fin);
}

bool launch_spmv_as(int v, int mode, const CsrMatrix& A, const double* x, double* y, const double* aux, double* partials,
                    const double* sc, int grid, hipStream_t st, const FinArgs* fin) {
  if (A.n == 0) return false;
  return launch_by_mode(v, mode, A, x, y, aux, partials, sc, grid, st, fin);
}

bool spmv_with_halo(int mode, const CsrMatrix& A, const Numbering& nb, const Slab& slab, double* x, double* y, const double* aux,
                    double* partials, const double* sc, int grid, hipStream_t st, const FinArgs* fin) {
  if (A.n == 0 || !A.halo_needed) {
    // (a rank without rows still takes part in the exchange: its neighbours receive from it)
    if (A.halo_needed) halo_exchange(nb, slab, x, st);
    return launch_spmv(mode, A, x, y, aux, partials, sc, grid, st, fin);
  }
  const int v = variant();
  const bool overlap = config().halo_overlap;
  const i64 ni = A.nslices_int, nbnd = A.nslices - A.nslices_int;
  if (!(v & 64) || !overlap || (ni == 0 && A.nunits == 0) || nbnd == 0) {
    halo_exchange(nb, slab, x, st);
    return launch_spmv(mode, A, x, y, aux, partials, sc, grid, st, fin);
  }
  // blocks of the second launch: one wave per slice, never more blocks than partial-sum entries per slot
  const int grid2 = (int)std::max<i64>(1, std::min<i64>(grid, (nbnd + BLOCK / 64 - 1) / (BLOCK / 64)));
  halo_begin(nb, slab, x, st);                      // x's owned part is final on `st`; ghosts arrive on the comm stream
  bool folded;
  FinArgs fin_nofold{nullptr, nullptr, PH_NONE, 0, 0, fin ? fin->dotx : nullptr};   // first launch: dot operand, no scalar phase
  if (fin) { fin_nofold.pc0 = fin->pc0; fin_nofold.pc1 = fin->pc1; fin_nofold.pc2 = fin->pc2; fin_nofold.base = fin->base; }
#define PG_SPLIT(MODE_)                                                                                              \
  launch_slices<MODE_>(v, A, 0, ni, x, y, aux, partials, sc, grid, grid, 0, st, fin ? &fin_nofold : nullptr);      \
  halo_end(st);                                                                                                      \
  folded = launch_slices<MODE_>(v, A, ni, nbnd, x, y, aux, partials, sc, grid2, grid, 1, st, fin, false)
  if (mode == 0) { PG_SPLIT(0); }
  else if (mode == 1) { PG_SPLIT(1); }
  else if (mode == 2) { PG_SPLIT(2); }
  else if (mode == 8) { PG_SPLIT(8); }
  else { PG_REQUIRE(mode == 3, "unknown SpMV launch mode"); PG_SPLIT(3); }
#undef PG_SPLIT
  return folded;
}

namespace {

__global__ void k_hash_vector(i64 n, unsigned long long seed, double* x) {
  for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    unsigned long long h = ((unsigned long long)i + seed) * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
    h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    x[i] = (double)(h >> 11) * (1.0 / 9007199254740992.0) - 0.5;
  }
}

// the epilogue of launch mode MODE on a plain product s (in y): the expression the slice kernel uses
template <int MODE>
__global__ void k_mode_epilogue(i64 n, double* __restrict__ y, const double* __restrict__ x, const double* __restrict__ b, double pc0,
                                double pc1, double pc2) {
  for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x)
    y[i] = mode_out<MODE>(y[i], x[i], b[i], pc0, pc1, pc2);
}

template <int MODE>
void mode_compare(const CsrMatrix& A, i64 nv, double* max_abs_diff, double* max_abs, double* max_dot_rel) {
  hipStream_t st = ctx().stream;
  const i64 n = A.n;
  const int grid = spmv_default_grid(n);
  DevBuf<double> x(nv), aux(nv), base(nv), ya(n), yb(n), pa(5 * (i64)grid), pb(5 * (i64)grid);
  hipLaunchKernelGGL(k_hash_vector, dim3(grid_for(nv, BLOCK)), dim3(BLOCK), 0, st, nv, 0ull, x.p);
  hipLaunchKernelGGL(k_hash_vector, dim3(grid_for(nv, BLOCK)), dim3(BLOCK), 0, st, nv, 0x5851F42D4C957F2Dull, aux.p);
  hipLaunchKernelGGL(k_hash_vector, dim3(grid_for(nv, BLOCK)), dim3(BLOCK), 0, st, nv, 0x14057B7EF767814Full, base.p);
  pa.zero();
  pb.zero();
  FinArgs fin{nullptr, nullptr, PH_NONE, 0, 0, nullptr};
  fin.pc0 = 0.75; fin.pc1 = -0.4375; fin.pc2 = 1.25;
  fin.base = base.p;
  launch_slices<MODE>(70, A, 0, A.nslices, x.p, ya.p, aux.p, pa.p, nullptr, grid, grid, 0, st, MODE == 8 ? &fin : nullptr);
  ensure_csr_chunks(A);
  if (MODE == 8) {
    PG_LAUNCH_C_ARGS((k_spmv_cw<0, true>), x.p, yb.p, aux.p, pb.p);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mode_epilogue<MODE>), dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, st, n, yb.p,
                       (const double*)x.p, (const double*)base.p, fin.pc0, fin.pc1, fin.pc2);
  } else {
    PG_LAUNCH_C_ARGS((k_spmv_cw<(MODE == 8 ? 0 : MODE), true>), x.p, yb.p, aux.p, pb.p);
  }
  PG_HIP(hipGetLastError());
  std::vector<double> ha(n), hb(n), qa(5 * (size_t)grid), qb(5 * (size_t)grid);
  ya.download(ha.data(), n);
  yb.download(hb.data(), n);
  pa.download(qa.data(), 5 * (i64)grid);
  pb.download(qb.data(), 5 * (i64)grid);
  *max_abs_diff = *max_abs = *max_dot_rel = 0.0;
  for (i64 i = 0; i < n; ++i) {
    *max_abs_diff = std::max(*max_abs_diff, std::fabs(ha[i] - hb[i]));
    *max_abs = std::max(*max_abs, std::fabs(ha[i]));
  }
  // dot slots of the launch modes (pg_spmv.h): 0 always, 1 and 4 with mode 3
  const int slots[3] = {0, 1, 4};
  const int nslot = MODE == 1 ? 1 : (MODE == 3 ? 3 : 0);
  for (int k = 0; k < nslot; ++k) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < grid; ++i) { a += qa[(size_t)slots[k] * grid + i]; b += qb[(size_t)slots[k] * grid + i]; }
    *max_dot_rel = std::max(*max_dot_rel, std::fabs(a - b) / std::max(std::fabs(b), 1e-300));
  }
}

}  // namespace

void spmv_mode_compare(const CsrMatrix& A, i64 nv, int mode, double* max_abs_diff, double* max_abs, double* max_dot_rel) {
  *max_abs_diff = *max_abs = *max_dot_rel = 0.0;
  if (A.n == 0) return;
  PG_REQUIRE(A.srec.p, "spmv_mode_compare: the matrix has no slice image");
  if (mode == 0) mode_compare<0>(A, nv, max_abs_diff, max_abs, max_dot_rel);
  else if (mode == 1) mode_compare<1>(A, nv, max_abs_diff, max_abs, max_dot_rel);
  else if (mode == 3) mode_compare<3>(A, nv, max_abs_diff, max_abs, max_dot_rel);
  else mode_compare<8>(A, nv, max_abs_diff, max_abs, max_dot_rel);
}

void launch_spmv_variant(int v, const CsrMatrix& A, const double* x, double* y, hipStream_t st) {
  if (A.n == 0) return;
  launch_mode<0>(v, A, x, y, nullptr, nullptr, nullptr, spmv_default_grid(A.n), st, nullptr);
}

}  // namespace pg
