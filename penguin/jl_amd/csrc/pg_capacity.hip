// pg_capacity.hip -- K1-K5 of SURVEY.md section 2.3: per-cell cut-cell capacities on the GPU.
//
//   reference                                             here
//   CartesianGeometry.integrate(Tuple{0},...)  capacity.jl:90-92   k_classify + k_cut_cells  (V, C_w, Gamma, type)
//   computeInterfaceCentroids                  capacity.jl:137-197 k_cut_cells               (C_gamma)
//   integrate(Tuple{1},...)                    capacity.jl:103     k_sections                (A_d)
//   integrate(Tuple{1},...,bary)               capacity.jl:105     k_sections                (B_d)
//   integrate(Tuple{0},...,bary)               capacity.jl:104     k_stagger + k_stagger_cut (W_d)
//
// Layout: one thread per padded cell, dim-0 fastest => every store is a coalesced 8-byte-per-lane
// stream.  Cells whose geometry needs quadrature (cut cells, ~n^(N-1) of n^N) are appended to a
// compacted work list and processed by a dense second kernel so that no wave idles on a lone cut
// cell.  Compiled with -ffp-contract=off: classification must match the oracle bit for bit.
#include "pg_capacity.h"
#include "pg_geom_program.h"
#include "pg_geom_program3.h"
#include "pg_geom_polygon.h"
#include "pg_scan.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>
#include <type_traits>

using namespace pg;
using namespace pggeom;

__constant__ GLTable c_gl;
// the programs of the traced level set under construction: phi, d phi / dx, d phi / dy, d phi / dt (moving bodies), d phi / dz
// (3-D bodies).  (Not in the unnamed namespace: a variable with internal linkage that no device code writes is folded to its
// zero initialiser.)
__constant__ pg_program c_prog[5];

namespace {

struct GeoView {
  int N;
  i64 ext[3], n[3], stride[3];
  i64 plane, s0, s1;
  const double* nodes[3];
  double h[3];     // mesh spacing L_d / n_d, the number Mesh() builds the nodes from (src/mesh.jl:49-50)
};

// Measures of FULL cells / faces / staggered volumes come from the mesh spacing h, not from differences of node
// coordinates: x0 + (j+½)h carries rounding noise, so nodes[i+1] - nodes[i] varies in the last bits from cell to cell
// unless h is a binary fraction.  With h every full cell of a uniform mesh has bitwise the same capacities, hence the
// same matrix rows, and the SpMV's uniform slices work on ANY mesh Mesh() can build (768^3 over [0,4]^3: h = 1/192).
// The difference to the node-difference value is ~1e-16 relative -- the noise level of the reference's own VOFI sums.
__device__ inline double full_measure(const GeoView& g, int skip) {
  double p = 0.0;
  bool first = true;
  for (int d = 0; d < g.N; ++d) {
    if (d == skip) continue;
    p = first ? g.h[d] : p * g.h[d];
    first = false;
  }
  return first ? 1.0 : p;
}

__device__ inline bool is_real_cell(const GeoView& g, const i64* idx) {
  for (int d = 0; d < g.N; ++d)
    if (idx[d] >= g.n[d]) return false;
  return true;
}

__device__ inline void cell_box(const GeoView& g, const i64* idx, double* lo, double* hi) {
  for (int d = 0; d < g.N; ++d) {
    lo[d] = g.nodes[d][idx[d]];
    hi[d] = g.nodes[d][idx[d] + 1];
  }
}

// The kernels below reach the body through pick_ball, box_measure and section_measure only, and are templates over the kernel
// argument the body travels in: BallArg for the closed-form kinds (a BallSet by value, the code the project always had) and
// ProgArg for a traced level set (pg_geom_program.h), PolyArg for a marker polygon (pg_geom_polygon.h).  LISTS_TOUCHING: a cell
// that is not CUT may still own a piece of the front (an edge along its lower or left face); only PolyArg has such cells, and
// for the other kinds the constant folds the branches away: they compile to the code they always compiled to.
struct BallArg : BallSet {
  static constexpr int MAX_BLOCK = 1024;        // (HIP's default: the closed-form instantiations compile as they always did)
  static constexpr bool LISTS_TOUCHING = false;
};
__device__ __forceinline__ const BallSet& kernel_body(const BallArg& a) { return a; }

// A traced level set.  The programs live in __constant__ memory (c_prog, 1824 bytes for phi and three derivatives), written
// before the launches of one capacity.  The evaluator is one function per kernel, called and not inlined (pg_geom_program.h
// says why); the program index is a literal at every call, so it is read into a scalar register and the instruction fetches
// are scalar loads.  The operand stack of lane l is column l of stack[PG_PROG_MAX_STACK][256] in LDS, as in k_td_eval
// (pg_program.hip): consecutive lanes hit consecutive banks, no lane reads another's column, so there is no barrier.
constexpr int PROG_BLOCK = 256;

struct ProgArg {
  static constexpr int MAX_BLOCK = PROG_BLOCK;
  static constexpr bool LISTS_TOUCHING = false;
  int N;
  double sgn;
};

struct ProgStack {
  double* col;
  __device__ double get(int d) const { return col[d * PROG_BLOCK]; }
  __device__ void set(int d, double x) { col[d * PROG_BLOCK] = x; }
};

__device__ __noinline__ __attribute__((flatten)) double prog_value(int which, double* col, double x, double y, double t) {
  ProgStack S{col};
  return pgprog::prog_eval(c_prog[__builtin_amdgcn_readfirstlane(which)], x, y, 0.0, t, S);
}

struct DevEval {
  double* col;
  __device__ double value(int which, double x, double y, double t) const { return prog_value(which, col, x, y, t); }
};

__device__ __forceinline__ ProgBody<DevEval> kernel_body(const ProgArg& a) {
  __shared__ double stack[PG_PROG_MAX_STACK * PROG_BLOCK];
  return ProgBody<DevEval>{a.N, 0, a.sgn, DevEval{stack + threadIdx.x}};
}

// A traced level set in 3-D (pg_geom_program3.h): the same table, slot 4 holding d phi / dz, an evaluator of its own that passes
// z on, and the same LDS columns.  One WAVE shares a cut box (lane l: outer node l & 15, inner nodes l >> 4, (l >> 4) + 4, ...);
// the faces the cell types do not finish go to a work list, 16 lanes per item (SECTION_LIST).
struct Prog3Arg {
  static constexpr int MAX_BLOCK = PROG_BLOCK;
  static constexpr bool LISTS_TOUCHING = false;
  double sgn;
};

// (flatten, here and on prog_value: prog_eval is part of each evaluator whatever the number of its callers -- left to the
// inliner, a second caller put it out of line and gave every ProgArg kernel a call level and 56 bytes of scratch)
__device__ __noinline__ __attribute__((flatten)) double prog_value3(int which, double* col, double x, double y, double z, double t) {
  ProgStack S{col};
  return pgprog::prog_eval(c_prog[__builtin_amdgcn_readfirstlane(which)], x, y, z, t, S);
}

struct DevEval3 {
  double* col;
  __device__ double value(int which, double x, double y, double z) const { return prog_value3(which, col, x, y, z, 0.0); }
};

__device__ __forceinline__ Prog3Body<DevEval3> kernel_body(const Prog3Arg& a) {
  __shared__ double stack[PG_PROG_MAX_STACK * PROG_BLOCK];
  return Prog3Body<DevEval3>{3, 0, a.sgn, DevEval3{stack + threadIdx.x}};
}

// A marker polygon: the body is the struct itself (markers, mesh nodes and the edge lookup, all in device memory).
struct PolyArg : PolyBody {
  static constexpr int MAX_BLOCK = 256;
  static constexpr bool LISTS_TOUCHING = true;
};
__device__ __forceinline__ const PolyBody& kernel_body(const PolyArg& a) { return a; }

// ---- the edge lookup of a polygon (pg_geom_polygon.h): count, scan (pg_scan.h), fill, order.  One thread per edge walks its
// bins (poly_edge_bins: at most 2 (n0 + n1) + 3 n0 + n1 visits, whatever the markers are; an edge outside the mesh visits none);
// the integer atomics fix only WHERE in its bin an edge lands, and k_poly_order then puts every bin in ascending edge order,
// so the lists, and every sum taken along them, are the same in every run.
// (templates over PolyBody and MovingPoly: a moving polygon lists its swept edges, pg_geom_polygon.h)
template <class P>
__global__ void k_poly_count(P b, int* __restrict__ count) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= b.M) return;
  poly_edge_bins(b, k, [&](int bin) { atomicAdd(&count[bin], 1); });
}
template <class P>
__global__ void k_poly_fill(P b, const int* __restrict__ ptr, int* __restrict__ cursor, int* __restrict__ tmp_edge,
                            int* __restrict__ tmp_bin) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= b.M) return;
  poly_edge_bins(b, k, [&](int bin) {
    const int pos = ptr[bin] + atomicAdd(&cursor[bin], 1);
    tmp_edge[pos] = k;
    tmp_bin[pos] = bin;
  });
}
// entry e of bin b goes to the place its rank among the bin's edge ids gives it (an edge is in a bin once: the ranks differ)
__global__ void k_poly_order(const int* __restrict__ ptr, const int* __restrict__ tmp_edge, const int* __restrict__ tmp_bin, int total,
                             int* __restrict__ idx) {
  for (i64 e = blockIdx.x * (i64)blockDim.x + threadIdx.x; e < total; e += (i64)gridDim.x * blockDim.x) {
    const int bin = tmp_bin[e], id = tmp_edge[e];
    int rank = 0;
    for (int q = ptr[bin]; q < ptr[bin + 1]; ++q) rank += tmp_edge[q] < id ? 1 : 0;
    idx[ptr[bin] + rank] = id;
  }
}

// K1 (cheap part): classify every stored cell; full/empty cells are finished here.
template <class BodyArg>
__global__ __launch_bounds__(BodyArg::MAX_BLOCK) void k_classify(GeoView g, BodyArg ba, i64 Mloc, double* V, double* G, double* ct,
                                                                 double* Cw0, double* Cw1, double* Cw2, double* Cg0, double* Cg1,
                                                                 double* Cg2, int* cut_list, int* cut_count) {
  const auto& bs = kernel_body(ba);
  double* Cw[3] = {Cw0, Cw1, Cw2};
  double* Cg[3] = {Cg0, Cg1, Cg2};
  for (i64 lc = blockIdx.x * (i64)blockDim.x + threadIdx.x; lc < Mloc; lc += (i64)gridDim.x * blockDim.x) {
    i64 idx[3];
    decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
    double v = 0.0, t = 0.0;
    double cw[3] = {0.0, 0.0, 0.0};
    if (is_real_cell(g, idx)) {
      double lo[3], hi[3];
      cell_box(g, idx, lo, hi);
      int type;
      bool listed;
      if constexpr (BodyArg::LISTS_TOUCHING) listed = pick_ball(bs, lo, hi, type) != 0 || type == PG_CUT;
      else {
        pick_ball(bs, lo, hi, type);
        listed = type == PG_CUT;
      }
      if (type != PG_CUT && bs.complement) type = 1 - type;
      for (int d = 0; d < g.N; ++d) cw[d] = 0.5 * (lo[d] + hi[d]);
      if (type == PG_FULL) v = full_measure(g, -1);
      if (listed) {
        const int slot = atomicAdd(cut_count, 1);
        cut_list[slot] = (int)lc;
      }
      t = (double)type;
    }
    V[lc] = v;
    G[lc] = 0.0;
    ct[lc] = t;
    for (int d = 0; d < g.N; ++d) {
      Cw[d][lc] = cw[d];
      if (Cg[d]) Cg[d][lc] = 0.0;
    }
  }
}

// The cut-cell quadrature is ~10^5 flops of branchy fp64 per box and there are only O(n^(N-1)) boxes: one thread per box
// leaves ~3 waves per SIMD walking long serial chains (20 + 43 ms at 512^3).  CUT_LANES lanes share a box instead: each
// takes one Gauss-Legendre node of every z piece and the partial moments are summed with shuffles.
constexpr int CUT_LANES = 16;   // = NGL
// BODY_PLANE has no quadrature to share (closed form): by default it keeps the convention of the other closed-form kind --
// lane 0 of the group returns the whole result -- and so the launch shape every body uses.  -DPG_PLANE_CUT_LANES=1 launches
// its two work lists with one lane per item instead; which is faster at 256^3 is not measured yet
#ifndef PG_PLANE_CUT_LANES
#define PG_PLANE_CUT_LANES CUT_LANES
#endif

template <int LANES>
struct LaneGroup {
  __device__ void operator()(pggeom::Mom& m) const {
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) {
      m.vol += __shfl_xor(m.vol, off, LANES);
      m.gamma += __shfl_xor(m.gamma, off, LANES);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        m.m[d] += __shfl_xor(m.m[d], off, LANES);
        m.gm[d] += __shfl_xor(m.gm[d], off, LANES);
      }
    }
  }
};

// K1/K5 (expensive part): LANES lanes per cut cell of the compacted list.
template <int LANES, class BodyArg>
__global__ __launch_bounds__(BodyArg::MAX_BLOCK) void k_cut_cells(GeoView g, BodyArg ba, const int* cut_list, int ncut, double* V,
                                                                  double* G, double* Cw0, double* Cw1, double* Cw2, double* Cg0,
                                                                  double* Cg1, double* Cg2) {
  const auto& bs = kernel_body(ba);
  double* Cw[3] = {Cw0, Cw1, Cw2};
  double* Cg[3] = {Cg0, Cg1, Cg2};
  const i64 gt = blockIdx.x * (i64)blockDim.x + threadIdx.x;
  const int ql = (int)(gt % LANES);
  i64 k = gt / LANES;
  const bool live = k < ncut;
  if (!live) k = ncut - 1;          // whole groups stay in the shuffles
  const i64 lc = cut_list[k];
  i64 idx[3];
  decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
  double lo[3], hi[3];
  cell_box(g, idx, lo, hi);
  const BoxMeasure m = box_measure(bs, lo, hi, true, c_gl, ql, LANES, LaneGroup<LANES>());
  if (!live || ql != 0) return;
  if constexpr (BodyArg::LISTS_TOUCHING) {
    if (m.type != PG_CUT) {           // listed for the piece of the front it owns: its type, volume and centroid stand
      G[lc] = m.gamma;
      for (int d = 0; d < g.N; ++d)
        if (Cg[d]) Cg[d][lc] = m.cg[d];
      return;
    }
  }
  V[lc] = m.vol;
  G[lc] = m.gamma;
  for (int d = 0; d < g.N; ++d) {
    Cw[d][lc] = m.cen[d];
    if (Cg[d]) Cg[d][lc] = m.cg[d];
  }
}

// K2 + K4: A_d (face x_d = nodes_d[i_d], i_d <= n_d, other dims real) and B_d (section through C_w[d]).
// A face or a centroid section of cell i lies inside the closed cell: if the cell is FULL (EMPTY) the section is FULL
// (EMPTY) by the same monotone far / near tests that classified the cell, with the same value prod_ext(...) (0) the
// geometric path returns -- so only cut cells (and the padding faces next to them) evaluate geometry: 17 -> 3 ms at 512^3.
template <class BodyArg>
__global__ __launch_bounds__(BodyArg::MAX_BLOCK) void k_sections(GeoView g, BodyArg ba, i64 Mloc, const double* ct, const double* Cw0,
                                                                 const double* Cw1, const double* Cw2, double* A0, double* A1,
                                                                 double* A2, double* B0, double* B1, double* B2) {
  const auto& bs = kernel_body(ba);
  const double* Cw[3] = {Cw0, Cw1, Cw2};
  double* A[3] = {A0, A1, A2};
  double* B[3] = {B0, B1, B2};
  for (i64 lc = blockIdx.x * (i64)blockDim.x + threadIdx.x; lc < Mloc; lc += (i64)gridDim.x * blockDim.x) {
    i64 idx[3];
    decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
    const bool real = is_real_cell(g, idx);
    for (int d = 0; d < g.N; ++d) {
      // A_d: other dims must be real; the section box uses the cell extents of the other dims
      bool others_real = true;
      for (int k = 0; k < g.N; ++k)
        if (k != d && idx[k] >= g.n[k]) others_real = false;
      double a = 0.0, b = 0.0;
      if (others_real) {
        double lo[3], hi[3];
        for (int k = 0; k < g.N; ++k) {
          const i64 ik = idx[k] < g.n[k] ? idx[k] : g.n[k] - 1;
          lo[k] = g.nodes[k][ik];
          hi[k] = g.nodes[k][ik + 1];
        }
        // type of the real cell that contains the face: cell i, or cell i - e_d for the padding face i_d = n_d
        double t = (double)PG_CUT;
        if (real) t = ct[lc];
        else if (idx[d] >= g.n[d] && lc - g.stride[d] >= 0) t = ct[lc - g.stride[d]];
        // the faces / sections of a full (empty) cell are full (empty) -- except in 1-D, where a face is a POINT and a
        // point exactly on the interface counts as fluid (f <= 0) whichever cell owns it: always evaluated there
        if (g.N > 1 && t == (double)PG_FULL) {
          a = full_measure(g, d);
          b = real ? a : 0.0;
        } else if (g.N > 1 && t == (double)PG_EMPTY) {
          a = 0.0;
          b = 0.0;
        } else {
          a = section_measure(bs, d, g.nodes[d][idx[d]], lo, hi, full_measure(g, d));
          if (real) b = section_measure(bs, d, Cw[d][lc], lo, hi, full_measure(g, d));
        }
      }
      A[d][lc] = a;
      B[d][lc] = b;
    }
  }
}

// K2 + K4 of a 3-D traced level set.  A section there is a 2-D quadrature: k_sections_list finishes the faces of FULL and EMPTY
// cells as k_sections does and lists the others as (cell, 2 d + (0: A, 1: B)); k_sections_cut measures every item with a group of
// SEC_LANES lanes that share the Gauss-Legendre nodes of the 2-D rule.
constexpr int SEC_LANES = 16;   // = NGL

__global__ void k_sections_list(GeoView g, i64 Mloc, const double* ct, double* A0, double* A1, double* A2, double* B0, double* B1,
                                double* B2, int* list, int* count, int cap) {
  double* A[3] = {A0, A1, A2};
  double* B[3] = {B0, B1, B2};
  for (i64 lc = blockIdx.x * (i64)blockDim.x + threadIdx.x; lc < Mloc; lc += (i64)gridDim.x * blockDim.x) {
    i64 idx[3];
    decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
    const bool real = is_real_cell(g, idx);
    for (int d = 0; d < g.N; ++d) {
      bool others_real = true;
      for (int k = 0; k < g.N; ++k)
        if (k != d && idx[k] >= g.n[k]) others_real = false;
      double a = 0.0, b = 0.0;
      if (others_real) {
        double t = (double)PG_CUT;
        if (real) t = ct[lc];
        else if (idx[d] >= g.n[d] && lc - g.stride[d] >= 0) t = ct[lc - g.stride[d]];
        if (t == (double)PG_FULL) {
          a = full_measure(g, d);
          b = real ? a : 0.0;
        } else if (t != (double)PG_EMPTY) {
          const int want = real ? 2 : 1;
          const int slot = atomicAdd(count, want);
          for (int q = 0; q < want; ++q)
            if (slot + q < cap) { list[2 * (slot + q)] = (int)lc; list[2 * (slot + q) + 1] = 2 * d + q; }
        }
      }
      A[d][lc] = a;
      B[d][lc] = b;
    }
  }
}

template <class BodyArg>
__global__ __launch_bounds__(BodyArg::MAX_BLOCK) void k_sections_cut(GeoView g, BodyArg ba, const int* __restrict__ list, int nlist,
                                                                     const double* Cw0, const double* Cw1, const double* Cw2,
                                                                     double* A0, double* A1, double* A2, double* B0, double* B1,
                                                                     double* B2) {
  const auto& bs = kernel_body(ba);
  const i64 gt = blockIdx.x * (i64)blockDim.x + threadIdx.x;
  const int ql = (int)(gt % SEC_LANES);
  i64 k = gt / SEC_LANES;
  const bool live = k < nlist;
  if (!live) k = nlist - 1;         // whole groups stay in the shuffles
  const i64 lc = list[2 * k];
  const int d = list[2 * k + 1] >> 1, which = list[2 * k + 1] & 1;
  i64 idx[3];
  decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
  double lo[3], hi[3];
  for (int q = 0; q < 3; ++q) {
    const i64 iq = idx[q] < g.n[q] ? idx[q] : g.n[q] - 1;
    lo[q] = g.nodes[q][iq];
    hi[q] = g.nodes[q][iq + 1];
  }
  // (d picks by selects, never by an index into a private array)
  const double* cw = d == 0 ? Cw0 : d == 1 ? Cw1 : Cw2;
  double* dst = which ? (d == 0 ? B0 : d == 1 ? B1 : B2) : (d == 0 ? A0 : d == 1 ? A1 : A2);
  const double s = which ? cw[lc] : g.nodes[d][d == 0 ? idx[0] : d == 1 ? idx[1] : idx[2]];
  const double m = section_measure(bs, d, s, lo, hi, full_measure(g, d), c_gl, ql, SEC_LANES, LaneGroup<SEC_LANES>());
  if (live && ql == 0) dst[lc] = m;
}

// K3 (cheap part): W_d between the centroids of i-e_d and i; cut boxes go to the work list.
template <class BodyArg>
__global__ __launch_bounds__(BodyArg::MAX_BLOCK) void k_stagger(GeoView g, BodyArg ba, i64 Mloc, const double* ct, const double* Cw0,
                                                                const double* Cw1, const double* Cw2, double* W0, double* W1,
                                                                double* W2, int* wlist, int* wcount, int wcap) {
  const auto& bs = kernel_body(ba);
  const double* Cw[3] = {Cw0, Cw1, Cw2};
  double* W[3] = {W0, W1, W2};
  for (i64 lc = blockIdx.x * (i64)blockDim.x + threadIdx.x; lc < Mloc; lc += (i64)gridDim.x * blockDim.x) {
    i64 idx[3];
    decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
    for (int d = 0; d < g.N; ++d) {
      double w = 0.0;
      bool others_real = true;
      for (int k = 0; k < g.N; ++k)
        if (k != d && idx[k] >= g.n[k]) others_real = false;
      // prev = max(i-1, first), next = min(i, last real)      capacity.jl:401-402
      const i64 ip = idx[d] - 1 < 0 ? 0 : idx[d] - 1;
      const i64 in = idx[d] < g.n[d] - 1 ? idx[d] : g.n[d] - 1;
      const i64 lp = lc + (ip - idx[d]) * g.stride[d];
      const i64 ln = lc + (in - idx[d]) * g.stride[d];
      // the neighbour in the slowest dim may lie outside the stored planes: leave 0 (never read)
      const bool have = lp >= 0 && ln >= 0 && lp < Mloc && ln < Mloc;
      if (others_real && have && ip != in) {
        const double tp = ct[lp], tn = ct[ln];
        if (!(tp == 0.0 && tn == 0.0)) {   // capacity.jl:420-427
          double lo[3], hi[3];
          for (int k = 0; k < g.N; ++k) {
            if (k == d) continue;
            lo[k] = g.nodes[k][idx[k]];
            hi[k] = g.nodes[k][idx[k] + 1];
          }
          lo[d] = Cw[d][lp];
          hi[d] = Cw[d][ln];
          int type;
          pick_ball(bs, lo, hi, type);
          if (type != PG_CUT && bs.complement) type = 1 - type;
          bool degenerate = false;
          for (int k = 0; k < g.N; ++k)
            if (!(hi[k] - lo[k] > 0.0)) degenerate = true;
          if (!degenerate) {
            // between the centres of two full cells: exactly one cell volume
            if (type == PG_FULL) w = (tp == 1.0 && tn == 1.0) ? full_measure(g, -1) : prod_ext(lo, hi, g.N, -1);
            else if (type == PG_CUT) {
              const int slot = atomicAdd(wcount, 1);
              if (slot < wcap) {
                wlist[2 * slot] = (int)lc;
                wlist[2 * slot + 1] = d;
              }
            }
          }
        }
      }
      W[d][lc] = w;
    }
  }
}

template <int LANES, class BodyArg>
__global__ __launch_bounds__(BodyArg::MAX_BLOCK) void k_stagger_cut(GeoView g, BodyArg ba, const int* wlist, int nw, const double* Cw0,
                                                                    const double* Cw1, const double* Cw2, double* W0, double* W1,
                                                                    double* W2) {
  const auto& bs = kernel_body(ba);
  const double* Cw[3] = {Cw0, Cw1, Cw2};
  double* W[3] = {W0, W1, W2};
  const i64 gt = blockIdx.x * (i64)blockDim.x + threadIdx.x;
  const int ql = (int)(gt % LANES);
  i64 k = gt / LANES;
  const bool live = k < nw;
  if (!live) k = nw - 1;
  const i64 lc = wlist[2 * k];
  const int d = wlist[2 * k + 1];
  i64 idx[3];
  decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
  const i64 ip = idx[d] - 1 < 0 ? 0 : idx[d] - 1;
  const i64 in = idx[d] < g.n[d] - 1 ? idx[d] : g.n[d] - 1;
  const i64 lp = lc + (ip - idx[d]) * g.stride[d];
  const i64 ln = lc + (in - idx[d]) * g.stride[d];
  double lo[3], hi[3];
  if constexpr (std::is_same<BodyArg, Prog3Arg>::value) {
    // the same box, every entry written at a literal index: lo and hi stay in registers (the other kinds keep their code)
    const double cp = Cw[d][lp], cn = Cw[d][ln];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const i64 iq = q == d ? 0 : idx[q];        // (along d the nodes are not read: always an index inside the array)
      lo[q] = q == d ? cp : g.nodes[q][iq];
      hi[q] = q == d ? cn : g.nodes[q][iq + 1];
    }
  } else {
    for (int q = 0; q < g.N; ++q) {
      if (q == d) continue;
      lo[q] = g.nodes[q][idx[q]];
      hi[q] = g.nodes[q][idx[q] + 1];
    }
    lo[d] = Cw[d][lp];
    hi[d] = Cw[d][ln];
  }
  const double w = box_measure(bs, lo, hi, false, c_gl, ql, LANES, LaneGroup<LANES>()).vol;
  if (live && ql == 0) W[d][lc] = w;
}

// per-plane count of non-empty cells (slab balancing weights)
__global__ void k_plane_weights(GeoView g, BallSet bs, i64 plane_lo, i64 plane_hi, unsigned long long* weight) {
  const i64 total = (plane_hi - plane_lo) * g.plane;
  for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < total; q += (i64)gridDim.x * blockDim.x) {
    const i64 p = q / g.plane + plane_lo;
    i64 rem = q % g.plane;
    i64 idx[3] = {0, 0, 0};
    for (int d = 0; d < g.N - 1; ++d) { idx[d] = rem % g.ext[d]; rem /= g.ext[d]; }
    idx[g.N - 1] = p;
    if (!is_real_cell(g, idx)) continue;
    double lo[3], hi[3];
    cell_box(g, idx, lo, hi);
    int type;
    pick_ball(bs, lo, hi, type);
    if (type != PG_CUT && bs.complement) type = 1 - type;
    if (type != PG_EMPTY) atomicAdd(&weight[p], type == PG_CUT ? 2ull : 1ull);
    else {
      // an empty cell on a lateral face of the box still becomes a row when a border condition is set there (identity
      // row of BC_border_mono!): 1.05 M of the 10.3 M rows of the 512^3 benchmark problem, spread over ALL planes --
      // left out, the slabs outside the body end up 20 % larger than the others when one body is cut into 8 slabs
      bool lateral = false;
      for (int d = 0; d < g.N - 1; ++d) lateral = lateral || idx[d] == 0 || idx[d] == g.n[d] - 1;
      if (lateral) atomicAdd(&weight[p], 1ull);
    }
  }
}

// ---- space-time capacities of one time slab [t0, t1] ------------------------------------------------------------
// Capacity(body, SpaceTimeMesh(mesh, [t, t+Δt])) of the reference (prescribedmotionsolver/diffusion.jl:251-252) hands the
// (N+1)-D cell  (space cell) x [t0, t1]  to libvofi.  Here the body is a ball / half space whose parameters move in
// time, and every first-layer capacity is the time integral of the corresponding spatial measure (exact in space, as
// the static kernels; composite Gauss-Legendre in time, nodes supplied by the host which evaluates the motion there):
//   V = ∫V(τ)dτ   C_ω = ∫∫(x, τ) / V   A_d = ∫A_d(τ)dτ   B_d = ∫|{x_d = C_ω,d} ∩ fluid(τ)|dτ   W_d = ∫|box(C_ω) ∩ fluid(τ)|dτ
//   Γ = ∫Γ(τ) sqrt(1 + v_n²) dτ  (v_n: normal speed of the interface at the spatial interface centroid)
//   A_(N+1) at the two time faces = V(t0), V(t1)   ("Vn_1", "Vn" of diffusion.jl:113-114)
struct MotionNode {
  double tau, w, c[3], r, dc[3], dr;   // half space: c[0] = position, dc[0] = its speed
};
struct MotionView {
  int kind, complement, axis, nq;
  double sgn, t0, t1;
  const MotionNode* q;
  MotionNode end[2];
  // the body at mid time and how far any of the bodies the rule sees (nodes and both faces) is from it: |c - c_mid| + |r - r_mid|
  // at most `reach` -- a cell FULL for the mid body shrunk by `reach` (EMPTY for it grown by `reach`) is so at every node
  MotionNode mid;
  double reach;
  // the body at node k (k < nq) and at the two time faces (nq, nq + 1), built by the host: every lane of a wave reads the
  // same one (scalar loads) -- a BallSet per lane would live in scratch
  const BallSet* bodies;
};

// The k_st_* kernels that look at the body are templates over how "the body at node k / at a time face" is obtained, as the
// static kernels are templates over BallArg / ProgArg: StBall reads the BallSet table the host built (the code the project
// always had), StProg evaluates the traced level set phi(x, t) at tau[k], t0, t1 (ProgBody with its time set).  Slot k of
// st_body: k < nq the time node k, nq the face t0, nq + 1 the face t1.  (k_st_sections and k_st_stagger, the cheap passes that
// only read the cell types, never touch the body and serve both.)
struct StBall {
  static constexpr int MAX_BLOCK = 1024;        // (HIP's default: the closed-form instantiations compile as they always did)
  static constexpr bool LISTS_TOUCHING = false;
};
struct StBallBase {};
__device__ __forceinline__ StBallBase st_base(const StBall&) { return StBallBase(); }

struct StProg : ProgArg {};
__device__ __forceinline__ ProgBody<DevEval> st_base(const StProg& a) { return kernel_body(a); }

__device__ __forceinline__ const BallSet& st_body(const StBallBase&, const MotionView& mv, int k) { return mv.bodies[k]; }
__device__ __forceinline__ ProgBody<DevEval> st_body(ProgBody<DevEval> b, const MotionView& mv, int k) {
  b.t = k < mv.nq ? mv.q[k].tau : k == mv.nq ? mv.t0 : mv.t1;
  return b;
}

// A moving marker polygon (MovingPoly of pg_geom_polygon.h: the markers at t0 and t1 and the lookup of the swept edges, all in
// device memory).  The polygon at slot k is a view that interpolates a vertex when it is read: nothing is stored per node.  The
// host puts s_k = (tau_k - t0) / (t1 - t0) into MotionNode::c[0]; the faces are taken by slot, never by s.
struct StPoly : MovingPoly {
  static constexpr int MAX_BLOCK = 256;
  static constexpr bool LISTS_TOUCHING = true;  // a cell that is never CUT may own a piece of the front (an edge along its face)
};
__device__ __forceinline__ const MovingPoly& st_base(const StPoly& a) { return a; }
__device__ __forceinline__ MovingPoly st_body(MovingPoly b, const MotionView& mv, int k) {
  b.face = k < mv.nq ? 0 : k == mv.nq ? 1 : 2;
  b.s = k < mv.nq ? mv.q[k].c[0] : 0.0;
  return b;
}

// the cheap test of a cell: 1 inside every body the rule sees, -1 outside every one, 0 near
__device__ inline int st_far(const StBallBase&, const GeoView& g, const MotionView& mv, const double* lo, const double* hi) {
  int far = 0;
  if (mv.kind == BODY_HALFSPACE) {
    const double pl = mv.mid.c[0] - mv.reach, ph = mv.mid.c[0] + mv.reach;
    if (hi[mv.axis] <= pl) far = mv.sgn > 0.0 ? 1 : -1;
    else if (lo[mv.axis] >= ph) far = mv.sgn > 0.0 ? -1 : 1;
  } else {
    if (mv.mid.r - mv.reach > 0.0 && ball_box_type(mv.mid.c, mv.mid.r - mv.reach, lo, hi, g.N) == PG_FULL) far = 1;
    else if (ball_box_type(mv.mid.c, mv.mid.r + mv.reach, lo, hi, g.N) == PG_EMPTY) far = -1;
  }
  return far;
}
// a traced level set has no `reach`: the sample lattice at t0, mid time and t1 with a margin from d phi / dt (prog_st_far)
__device__ inline int st_far(const ProgBody<DevEval>& b, const GeoView&, const MotionView& mv, const double* lo, const double* hi) {
  return prog_st_far(b, lo, hi, mv.t0, mv.t1);
}

// a polygon: no swept edge in the cell's list -- no edge comes into the closed cell at any time of the slab, so the cell is
// what its centre is at t0 (parity, from its row's bucket)
__device__ inline int st_far(const MovingPoly& b, const GeoView&, const MotionView&, const double* lo, const double* hi) {
  const double cx = 0.5 * (lo[0] + hi[0]), cy = 0.5 * (lo[1] + hi[1]);
  const int bin = poly_cell_bin(b, poly_locate(b, 0, cx), poly_locate(b, 1, cy));
  if (b.ptr[bin + 1] > b.ptr[bin]) return 0;
  MovingPoly f = b;
  f.face = 1;
  return poly_fluid_at(f, cx, cy) ? 1 : -1;
}

// the spatial volume at a time face.  Program bodies: a face that is FULL gets the measure the full cells get (from h, see
// full_measure), so that V(t1) of one slab and V(t0) of the next are the same bits whichever of the two slabs cuts the cell;
// the closed-form kinds keep the box's own product of node differences, as they always had
__device__ __forceinline__ double st_face_volume(const StBallBase&, const GeoView&, const BoxMeasure& m) { return m.vol; }
__device__ __forceinline__ double st_face_volume(const ProgBody<DevEval>&, const GeoView& g, const BoxMeasure& m) {
  return m.type == PG_FULL ? full_measure(g, -1) : m.vol;
}

__device__ __forceinline__ double st_face_volume(const MovingPoly&, const GeoView& g, const BoxMeasure& m) {
  return m.type == PG_FULL ? full_measure(g, -1) : m.vol;     // (as the program bodies: Vn and the next slab's Vn_1 are the same bits)
}

// the normal speed of the interface at the spatial interface centroid cg of time node q
__device__ inline double st_normal_speed(const BallSet&, const MotionView& mv, const MotionNode& q, const double* cg, int N) {
  double vn;
  if (mv.kind == BODY_HALFSPACE) vn = q.dc[0];
  else {
    double nn = 0.0, dot = 0.0;
    for (int d = 0; d < N; ++d) {
      const double e = cg[d] - q.c[d];
      nn += e * e;
      dot += e * q.dc[d];
    }
    vn = q.dr + (nn > 0.0 ? dot / sqrt(nn) : 0.0);
  }
  return vn;
}
// - d_t phi / |grad phi| at (cg, tau) -- the body carries tau
__device__ inline double st_normal_speed(const ProgBody<DevEval>& b, const MotionView&, const MotionNode&, const double* cg, int N) {
  return b.normal_speed(cg[0], N > 1 ? cg[1] : 0.0);
}

// a polygon takes one speed per PIECE of the front, inside box_measure: its gamma already carries sqrt(1 + v_n^2)
__device__ __forceinline__ double st_normal_speed(const MovingPoly&, const MotionView&, const MotionNode&, const double*, int) {
  return 0.0;
}

// Work is split as in the static kernels: a cheap pass over all cells finishes the ones that need no quadrature and
// lists the others; a second kernel gives every listed item one WAVE whose lanes take the time nodes (a box / section
// measure is a few thousand fp64 instructions with square roots and arc tangents: 64 of them in one lane, for the few
// cells near the interface, left the whole grid waiting -- 6.4 ms per slab at 1024², 0.3 ms this way).
__device__ inline double wave_add(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

struct StOut {
  double *V, *G, *ct, *Cw[3], *Cg[3], *Vt0, *Vt1, *Ctw, *Ctg;
};

__device__ inline void st_store_plain(const GeoView& g, const MotionView& mv, const StOut& o, i64 lc, const double* lo, const double* hi,
                                      bool real, bool fluid) {
  double cw[3] = {0.0, 0.0, 0.0};
  double v = 0.0, v01 = 0.0, t = 0.0, tw = 0.0;
  if (real) {
    for (int d = 0; d < g.N; ++d) cw[d] = 0.5 * (lo[d] + hi[d]);
    tw = 0.5 * (mv.t0 + mv.t1);
    if (fluid) { v = full_measure(g, -1) * (mv.t1 - mv.t0); v01 = full_measure(g, -1); t = (double)PG_FULL; }
  }
  o.V[lc] = v; o.G[lc] = 0.0; o.ct[lc] = t; o.Vt0[lc] = v01; o.Vt1[lc] = v01; o.Ctw[lc] = tw; o.Ctg[lc] = 0.0;
  for (int d = 0; d < g.N; ++d) {
    o.Cw[d][lc] = cw[d];
    if (o.Cg[d]) o.Cg[d][lc] = 0.0;
  }
}

// pass 1 of V, C_ω, Γ, C_γ, type, V(t0), V(t1): cells far from the interface during the whole slab are finished here
template <class St>
__global__ __launch_bounds__(St::MAX_BLOCK) void k_st_classify(GeoView g, MotionView mv, St sa, i64 Mloc, StOut o, int* list,
                                                               int* count) {
  const auto base = st_base(sa);
  for (i64 lc = blockIdx.x * (i64)blockDim.x + threadIdx.x; lc < Mloc; lc += (i64)gridDim.x * blockDim.x) {
    i64 idx[3];
    decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    const bool real = is_real_cell(g, idx);
    int far = -1;   // 1: inside every body the rule sees, -1: outside every one, 0: near
    if (real) {
      cell_box(g, idx, lo, hi);
      far = st_far(base, g, mv, lo, hi);
    }
    if (far != 0) st_store_plain(g, mv, o, lc, lo, hi, real, (far == 1) != (mv.complement != 0));
    else list[atomicAdd(count, 1)] = (int)lc;
  }
}

// pass 2: one wave per listed cell, lanes over the time nodes (+ lanes 0 / 1: the two time faces)
template <class St>
__global__ __launch_bounds__(St::MAX_BLOCK) void k_st_cells(GeoView g, MotionView mv, St sa, const int* __restrict__ list, int nlist,
                                                            StOut o) {
  const auto base = st_base(sa);
  const int lane = threadIdx.x & 63;
  const i64 item = (blockIdx.x * (i64)blockDim.x + threadIdx.x) >> 6;
  if (item >= nlist) return;
  const i64 lc = list[item];
  i64 idx[3];
  decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
  double lo[3], hi[3];
  cell_box(g, idx, lo, hi);
  double v = 0.0, gam = 0.0, momt = 0.0, gmt = 0.0, vend = 0.0;
  double mom[3] = {0.0, 0.0, 0.0}, gm[3] = {0.0, 0.0, 0.0};
  bool full = true, empty = true;
  if (lane < 2) {
    const auto& face = st_body(base, mv, mv.nq + lane);
    const BoxMeasure m = box_measure(face, lo, hi, false, c_gl);
    vend = st_face_volume(base, g, m);
    full = m.type == PG_FULL;
    empty = m.type == PG_EMPTY;
  }
  for (int k = lane; k < mv.nq; k += 64) {
    const MotionNode q = mv.q[k];
    const auto& body = st_body(base, mv, k);
    const BoxMeasure m = box_measure(body, lo, hi, true, c_gl);
    full = full && m.type == PG_FULL;
    empty = empty && m.type == PG_EMPTY;
    const double wv = q.w * m.vol;
    v += wv;
    momt += wv * q.tau;
    for (int d = 0; d < g.N; ++d) mom[d] += wv * m.cen[d];
    if (m.gamma > 0.0) {
      const double vn = st_normal_speed(body, mv, q, m.cg, g.N);
      const double ws = q.w * m.gamma * sqrt(1.0 + vn * vn);
      gam += ws;
      gmt += ws * q.tau;
      for (int d = 0; d < g.N; ++d) gm[d] += ws * m.cg[d];
    }
  }
  const bool all_full = __all(full), all_empty = __all(empty);
  v = wave_add(v); gam = wave_add(gam); momt = wave_add(momt); gmt = wave_add(gmt);
  for (int d = 0; d < g.N; ++d) { mom[d] = wave_add(mom[d]); gm[d] = wave_add(gm[d]); }
  const double v0 = __shfl(vend, 0, 64), v1 = __shfl(vend, 1, 64);
  if (lane != 0) return;
  if (all_full || all_empty) {
    st_store_plain(g, mv, o, lc, lo, hi, true, all_full);
    if constexpr (St::LISTS_TOUCHING) {
      if (gam > 0.0) {                  // never CUT, but it owns a piece of the front: its type, volume and centroid stand
        o.G[lc] = gam;
        o.Ctg[lc] = gmt / gam;
        for (int d = 0; d < g.N; ++d)
          if (o.Cg[d]) o.Cg[d][lc] = gm[d] / gam;
      }
    }
    return;
  }
  double cw[3], cg[3] = {0.0, 0.0, 0.0}, tw = 0.5 * (mv.t0 + mv.t1), tg = 0.0;
  for (int d = 0; d < g.N; ++d) cw[d] = 0.5 * (lo[d] + hi[d]);
  if (v > 0.0) {
    for (int d = 0; d < g.N; ++d) cw[d] = mom[d] / v;
    tw = momt / v;
  }
  if (gam > 0.0) {
    for (int d = 0; d < g.N; ++d) cg[d] = gm[d] / gam;
    tg = gmt / gam;
  }
  o.V[lc] = v; o.G[lc] = gam; o.ct[lc] = (double)PG_CUT; o.Vt0[lc] = v0; o.Vt1[lc] = v1; o.Ctw[lc] = tw; o.Ctg[lc] = tg;
  for (int d = 0; d < g.N; ++d) {
    o.Cw[d][lc] = cw[d];
    if (o.Cg[d]) o.Cg[d][lc] = cg[d];
  }
}

// A_d, B_d: the conventions of k_sections, integrated over the slab.  Pass 1 writes the faces that need no quadrature and
// lists (cell, d) for the others; pass 2: one wave per item.
__global__ void k_st_sections(GeoView g, MotionView mv, i64 Mloc, const double* ct, double* A0, double* A1, double* A2, double* B0,
                              double* B1, double* B2, int* list, int* count, int cap) {
  double* A[3] = {A0, A1, A2};
  double* B[3] = {B0, B1, B2};
  const double dt = mv.t1 - mv.t0;
  for (i64 lc = blockIdx.x * (i64)blockDim.x + threadIdx.x; lc < Mloc; lc += (i64)gridDim.x * blockDim.x) {
    i64 idx[3];
    decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
    const bool real = is_real_cell(g, idx);
    for (int d = 0; d < g.N; ++d) {
      bool others_real = true;
      for (int k = 0; k < g.N; ++k)
        if (k != d && idx[k] >= g.n[k]) others_real = false;
      double a = 0.0, b = 0.0;
      if (others_real) {
        double t = (double)PG_CUT;
        if (real) t = ct[lc];
        else if (idx[d] >= g.n[d] && lc - g.stride[d] >= 0) t = ct[lc - g.stride[d]];
        if (g.N > 1 && t == (double)PG_FULL) {
          a = full_measure(g, d) * dt;
          b = real ? a : 0.0;
        } else if (!(g.N > 1 && t == (double)PG_EMPTY)) {
          const int slot = atomicAdd(count, 1);
          if (slot < cap) { list[2 * slot] = (int)lc; list[2 * slot + 1] = d; }
        }
      }
      A[d][lc] = a;
      B[d][lc] = b;
    }
  }
}

template <class St>
__global__ __launch_bounds__(St::MAX_BLOCK) void k_st_sections_cut(GeoView g, MotionView mv, St src, const int* __restrict__ list,
                                                                   int nlist, const double* Cw0, const double* Cw1, const double* Cw2,
                                                                   double* A0, double* A1, double* A2, double* B0, double* B1,
                                                                   double* B2) {
  const auto base = st_base(src);
  const double* Cw[3] = {Cw0, Cw1, Cw2};
  double* A[3] = {A0, A1, A2};
  double* B[3] = {B0, B1, B2};
  const int lane = threadIdx.x & 63;
  const i64 item = (blockIdx.x * (i64)blockDim.x + threadIdx.x) >> 6;
  if (item >= nlist) return;
  const i64 lc = list[2 * item];
  const int d = list[2 * item + 1];
  i64 idx[3];
  decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
  const bool real = is_real_cell(g, idx);
  double lo[3], hi[3];
  for (int k = 0; k < g.N; ++k) {
    const i64 ik = idx[k] < g.n[k] ? idx[k] : g.n[k] - 1;
    lo[k] = g.nodes[k][ik];
    hi[k] = g.nodes[k][ik + 1];
  }
  double a = 0.0, b = 0.0;
  const double fm = full_measure(g, d);
  bool a_full = true, b_full = real;
  for (int k = lane; k < mv.nq; k += 64) {
    const double wq = mv.q[k].w;
    const auto& body = st_body(base, mv, k);
    const double sa = section_measure(body, d, g.nodes[d][idx[d]], lo, hi, fm);
    a += wq * sa;
    a_full = a_full && sa == fm;
    if (real) {
      const double sb = section_measure(body, d, Cw[d][lc], lo, hi, fm);
      b += wq * sb;
      b_full = b_full && sb == fm;
    }
  }
  a = wave_add(a);
  b = wave_add(b);
  // a section that is full at every time node gets the measure the full cells get, full x Δt, and not the quadrature sum
  // Σ w_k full, which differs from it in the last bits: A_d - B_d between such a face and a full neighbour is then an EXACT
  // zero (as in the static kernels) instead of 1e-17 -- a residue that switches the γ unknowns of full cells on with
  // 1e-34 diagonals and makes their cell blocks singular (the moving two-phase systems met it)
  if (__all(a_full)) a = fm * (mv.t1 - mv.t0);
  if (__all(b_full)) b = fm * (mv.t1 - mv.t0);
  if (lane == 0) { A[d][lc] = a; B[d][lc] = b; }
}

// W_d: the conventions of k_stagger, integrated over the slab; same two passes
__global__ void k_st_stagger(GeoView g, MotionView mv, i64 Mloc, const double* ct, const double* Cw0, const double* Cw1,
                             const double* Cw2, double* W0, double* W1, double* W2, int* list, int* count, int cap) {
  const double* Cw[3] = {Cw0, Cw1, Cw2};
  double* W[3] = {W0, W1, W2};
  const double dt = mv.t1 - mv.t0;
  for (i64 lc = blockIdx.x * (i64)blockDim.x + threadIdx.x; lc < Mloc; lc += (i64)gridDim.x * blockDim.x) {
    i64 idx[3];
    decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
    for (int d = 0; d < g.N; ++d) {
      double w = 0.0;
      bool others_real = true;
      for (int k = 0; k < g.N; ++k)
        if (k != d && idx[k] >= g.n[k]) others_real = false;
      const i64 ip = idx[d] - 1 < 0 ? 0 : idx[d] - 1;
      const i64 in = idx[d] < g.n[d] - 1 ? idx[d] : g.n[d] - 1;
      const i64 lp = lc + (ip - idx[d]) * g.stride[d];
      const i64 ln = lc + (in - idx[d]) * g.stride[d];
      const bool have = lp >= 0 && ln >= 0 && lp < Mloc && ln < Mloc;
      if (others_real && have && ip != in) {
        const double tp = ct[lp], tn = ct[ln];
        if (!(tp == 0.0 && tn == 0.0)) {
          bool degenerate = !(Cw[d][ln] - Cw[d][lp] > 0.0);
          for (int k = 0; k < g.N; ++k)
            if (k != d && !(g.nodes[k][idx[k] + 1] - g.nodes[k][idx[k]] > 0.0)) degenerate = true;
          if (!degenerate) {
            if (tp == 1.0 && tn == 1.0) w = full_measure(g, -1) * dt;
            else {
              const int slot = atomicAdd(count, 1);
              if (slot < cap) { list[2 * slot] = (int)lc; list[2 * slot + 1] = d; }
            }
          }
        }
      }
      W[d][lc] = w;
    }
  }
}

template <class St>
__global__ __launch_bounds__(St::MAX_BLOCK) void k_st_stagger_cut(GeoView g, MotionView mv, St sa, const int* __restrict__ list,
                                                                  int nlist, const double* Cw0, const double* Cw1, const double* Cw2,
                                                                  double* W0, double* W1, double* W2) {
  const auto base = st_base(sa);
  const double* Cw[3] = {Cw0, Cw1, Cw2};
  double* W[3] = {W0, W1, W2};
  const int lane = threadIdx.x & 63;
  const i64 item = (blockIdx.x * (i64)blockDim.x + threadIdx.x) >> 6;
  if (item >= nlist) return;
  const i64 lc = list[2 * item];
  const int d = list[2 * item + 1];
  i64 idx[3];
  decode_cell(g.N, g.ext, g.plane, g.s0, lc, idx);
  const i64 ip = idx[d] - 1 < 0 ? 0 : idx[d] - 1;
  const i64 in = idx[d] < g.n[d] - 1 ? idx[d] : g.n[d] - 1;
  const i64 lp = lc + (ip - idx[d]) * g.stride[d];
  const i64 ln = lc + (in - idx[d]) * g.stride[d];
  double lo[3], hi[3];
  for (int k = 0; k < g.N; ++k) {
    if (k == d) continue;
    lo[k] = g.nodes[k][idx[k]];
    hi[k] = g.nodes[k][idx[k] + 1];
  }
  lo[d] = Cw[d][lp];
  hi[d] = Cw[d][ln];
  double w = 0.0;
  for (int k = lane; k < mv.nq; k += 64) {
    const auto& body = st_body(base, mv, k);
    w += mv.q[k].w * box_measure(body, lo, hi, false, c_gl).vol;
  }
  w = wave_add(w);
  if (lane == 0) W[d][lc] = w;
}

GeoView geo_view(pg_mesh* m, const Slab& s) {
  GeoView g;
  g.N = s.N;
  for (int d = 0; d < 3; ++d) {
    g.ext[d] = s.ext[d];
    g.n[d] = s.n[d];
    g.stride[d] = s.stride[d];
    g.nodes[d] = nullptr;
  }
  g.plane = s.plane;
  g.s0 = s.s0;
  g.s1 = s.s1;
  for (int d = 0; d < s.N; ++d) {
    if (!m->d_nodes[d].p) {
      m->d_nodes[d].alloc(m->n[d] + 1);
      m->d_nodes[d].upload(m->nodes[d].data(), m->n[d] + 1);
    }
    g.nodes[d] = m->d_nodes[d].p;
  }
  for (int d = 0; d < 3; ++d) g.h[d] = d < s.N ? m->L[d] / (double)m->n[d] : 1.0;
  return g;
}

void alloc_fields(pg_capacity* c) {
  const i64 Ml = c->slab.Mloc();
  PG_REQUIRE(Ml < (i64)2147483647, "capacity: local slab exceeds 2^31 cells");
  c->V.alloc(Ml); c->G.alloc(Ml); c->ct.alloc(Ml);
  for (int d = 0; d < c->N; ++d) {
    c->A[d].alloc(Ml); c->B[d].alloc(Ml); c->W[d].alloc(Ml); c->Cw[d].alloc(Ml);
    if (c->has_cg) c->Cg[d].alloc(Ml);
  }
}

bool g_gl_uploaded = false;
void ensure_gl() {
  if (g_gl_uploaded) return;
  GLTable t;
  gl_init(t);
  PG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_gl), &t, sizeof(t)));
  g_gl_uploaded = true;
}

// The edge lookup of `body` (PolyBody: the edges; MovingPoly: the swept edges) on the device: count, scan, fill, order.  The
// lists stay alive in `t`; ms: the time of the four steps.
struct PolyBins {
  DevBuf<int> ptr, idx;
  double ms = 0.0;
};
template <class P>
void build_poly_bins(const P& body, pg_mesh* m, const char* who, hipStream_t st, PolyBins& t) {
  const i64 nbins = m->n[0] + m->n[1] + m->n[0] * m->n[1], M = body.M;
  DevBuf<int> count(nbins + 1), cursor(nbins), d_total(1);
  t.ptr.alloc(nbins + 1);
  count.zero();
  cursor.zero();
  EventPair bin_ev;
  PG_HIP(hipEventRecord(bin_ev.e0, st));
  const dim3 per_edge((unsigned)((M + 255) / 256));
  hipLaunchKernelGGL(k_poly_count<P>, per_edge, dim3(256), 0, st, body, count.p);
  PG_HIP(hipGetLastError());
  scan_exclusive<int>(count.p, t.ptr.p, nbins + 1, d_total.p, st);          // ptr[nbins] = the total
  int total = 0;
  d_total.download(&total, 1);
  PG_REQUIRE(total >= 0, std::string(who) + ": the edge lookup exceeds 2^31 entries");
  DevBuf<int> tmp_edge(total > 0 ? total : 1), tmp_bin(total > 0 ? total : 1);
  t.idx.alloc(total > 0 ? total : 1);
  t.idx.zero();
  if (total > 0) {                               // (a polygon wholly outside the mesh: no list, nothing to launch)
    hipLaunchKernelGGL(k_poly_fill<P>, per_edge, dim3(256), 0, st, body, t.ptr.p, cursor.p, tmp_edge.p, tmp_bin.p);
    PG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_poly_order, dim3(grid_for(total, 256, 256 * 16)), dim3(256), 0, st, t.ptr.p, tmp_edge.p, tmp_bin.p, total,
                       t.idx.p);
    PG_HIP(hipGetLastError());
  }
  PG_HIP(hipEventRecord(bin_ev.e1, st));
  PG_HIP(hipEventSynchronize(bin_ev.e1));        // (tmp_edge / tmp_bin are freed on return)
  float ms = 0.f;
  PG_HIP(hipEventElapsedTime(&ms, bin_ev.e0, bin_ev.e1));
  t.ms = ms;
}

// K1 .. K5 on the stored slab of c for the body in `ba`; LANES lanes share a cut box.  An empty work list launches nothing.
template <int LANES, class BodyArg>
void run_static_kernels(pg_capacity* c, pg_mesh* m, const BodyArg& ba, hipStream_t st) {
  const int N = c->N;
  alloc_fields(c);
  const Slab& s = c->slab;
  const i64 Ml = s.Mloc();
  GeoView g = geo_view(m, s);
  DevBuf<int> cut_list(Ml), counters(2);
  DevBuf<int> wlist;
  counters.zero();
  EventPair ev, part[5];                        // the whole sequence, and each kernel alone (pg_capacity_kernel_ms_parts)
  bool ran[5] = {true, false, true, true, false};
  PG_HIP(hipEventRecord(ev.e0, st));
  const int gr = grid_for(Ml, 256, 256 * 16);
  PG_HIP(hipEventRecord(part[0].e0, st));
  hipLaunchKernelGGL(k_classify<BodyArg>, dim3(gr), dim3(256), 0, st, g, ba, Ml, c->V.p, c->G.p, c->ct.p, c->Cw[0].p,
                     c->Cw[1].p, c->Cw[2].p, c->Cg[0].p, c->Cg[1].p, c->Cg[2].p, cut_list.p, counters.p);
  PG_HIP(hipGetLastError());
  PG_HIP(hipEventRecord(part[0].e1, st));
  int hc[2];
  counters.download(hc, 2);
  const int ncut = hc[0];
  c->n_cut_local = ncut;
  if (ncut > 0) {
    ran[1] = true;
    PG_HIP(hipEventRecord(part[1].e0, st));
    hipLaunchKernelGGL((k_cut_cells<LANES, BodyArg>), dim3((unsigned)(((i64)ncut * LANES + 255) / 256)), dim3(256), 0, st, g, ba,
                       cut_list.p, ncut, c->V.p, c->G.p, c->Cw[0].p, c->Cw[1].p, c->Cw[2].p, c->Cg[0].p, c->Cg[1].p, c->Cg[2].p);
    PG_HIP(hipGetLastError());
    PG_HIP(hipEventRecord(part[1].e1, st));
  }
  PG_HIP(hipEventRecord(part[2].e0, st));
  if constexpr (std::is_same<BodyArg, Prog3Arg>::value) {
    // at most 6 sections per cut cell and 3 padding faces next to one
    const i64 scap = std::min<i64>((i64)2 * N * Ml, (i64)9 * (i64)ncut + 1024);
    DevBuf<int> slist(2 * scap), scount(1);
    scount.zero();
    hipLaunchKernelGGL(k_sections_list, dim3(gr), dim3(256), 0, st, g, Ml, c->ct.p, c->A[0].p, c->A[1].p, c->A[2].p, c->B[0].p,
                       c->B[1].p, c->B[2].p, slist.p, scount.p, (int)scap);
    PG_HIP(hipGetLastError());
    int ns = 0;
    scount.download(&ns, 1);
    PG_REQUIRE(ns <= scap, "internal: section work list overflow");
    if (ns > 0) {
      hipLaunchKernelGGL(k_sections_cut<BodyArg>, dim3((unsigned)(((i64)ns * SEC_LANES + 255) / 256)), dim3(256), 0, st, g, ba, slist.p,
                         ns, c->Cw[0].p, c->Cw[1].p, c->Cw[2].p, c->A[0].p, c->A[1].p, c->A[2].p, c->B[0].p, c->B[1].p, c->B[2].p);
      PG_HIP(hipGetLastError());
    }
    PG_HIP(hipEventRecord(part[2].e1, st));
    PG_HIP(hipEventSynchronize(part[2].e1));    // (the list is freed at the end of this block)
  } else {
    hipLaunchKernelGGL(k_sections<BodyArg>, dim3(gr), dim3(256), 0, st, g, ba, Ml, c->ct.p, c->Cw[0].p, c->Cw[1].p, c->Cw[2].p,
                       c->A[0].p, c->A[1].p, c->A[2].p, c->B[0].p, c->B[1].p, c->B[2].p);
    PG_HIP(hipGetLastError());
    PG_HIP(hipEventRecord(part[2].e1, st));
  }
  // W work list: at most N entries per cut-adjacent cell; bound by 2*N*ncut + slack
  const i64 wcap = std::min<i64>((i64)N * Ml, (i64)4 * N * (i64)ncut + 1024);
  wlist.alloc(2 * wcap);
  PG_HIP(hipEventRecord(part[3].e0, st));
  hipLaunchKernelGGL(k_stagger<BodyArg>, dim3(gr), dim3(256), 0, st, g, ba, Ml, c->ct.p, c->Cw[0].p, c->Cw[1].p, c->Cw[2].p,
                     c->W[0].p, c->W[1].p, c->W[2].p, wlist.p, counters.p + 1, (int)wcap);
  PG_HIP(hipGetLastError());
  PG_HIP(hipEventRecord(part[3].e1, st));
  counters.download(hc, 2);
  const int nw = hc[1];
  PG_REQUIRE(nw <= wcap, "internal: staggered-volume work list overflow");
  if (nw > 0) {
    ran[4] = true;
    PG_HIP(hipEventRecord(part[4].e0, st));
    hipLaunchKernelGGL((k_stagger_cut<LANES, BodyArg>), dim3((unsigned)(((i64)nw * LANES + 255) / 256)), dim3(256), 0, st, g, ba,
                       wlist.p, nw, c->Cw[0].p, c->Cw[1].p, c->Cw[2].p, c->W[0].p, c->W[1].p, c->W[2].p);
    PG_HIP(hipGetLastError());
    PG_HIP(hipEventRecord(part[4].e1, st));
  }
  PG_HIP(hipEventRecord(ev.e1, st));
  PG_HIP(hipEventSynchronize(ev.e1));
  float ms = 0.f;
  PG_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  c->kernel_ms = ms;
  for (int k = 0; k < 5; ++k) {
    c->kernel_ms_parts[k] = 0.0;
    if (!ran[k]) continue;                      // an empty work list: nothing was launched
    PG_HIP(hipEventElapsedTime(&ms, part[k].e0, part[k].e1));
    c->kernel_ms_parts[k] = ms;
  }
}

// The six space-time kernels on the whole mesh for the body `sa` reaches (mv: the time rule on the device, and for StBall the
// bodies).  parts (may be NULL): the time of each kernel alone, 0 for one an empty list did not launch.
template <class St>
void run_spacetime_kernels(pg_capacity* c, pg_mesh* m, const MotionView& mv, const St& sa, hipStream_t st, double* parts) {
  const int N = c->N;
  alloc_fields(c);
  const i64 Ml = c->slab.Mloc();
  c->Vt[0].alloc(Ml); c->Vt[1].alloc(Ml); c->Ctw.alloc(Ml); c->Ctg.alloc(Ml);
  GeoView g = geo_view(m, c->slab);
  EventPair ev;
  std::unique_ptr<EventPair[]> part(parts ? new EventPair[6] : nullptr);
  bool ran[6] = {true, false, true, false, true, false};
  auto t_begin = [&](int k) { if (parts) PG_HIP(hipEventRecord(part[k].e0, st)); };
  auto t_end = [&](int k) { if (parts) PG_HIP(hipEventRecord(part[k].e1, st)); };
  PG_HIP(hipEventRecord(ev.e0, st));
  const int gr = grid_for(Ml, 256, 256 * 16);
  StOut so;
  so.V = c->V.p; so.G = c->G.p; so.ct = c->ct.p; so.Vt0 = c->Vt[0].p; so.Vt1 = c->Vt[1].p; so.Ctw = c->Ctw.p; so.Ctg = c->Ctg.p;
  for (int d = 0; d < 3; ++d) { so.Cw[d] = c->Cw[d].p; so.Cg[d] = c->Cg[d].p; }
  DevBuf<int> near_list(Ml), counters(3);
  counters.zero();
  t_begin(0);
  hipLaunchKernelGGL(k_st_classify<St>, dim3(gr), dim3(256), 0, st, g, mv, sa, Ml, so, near_list.p, counters.p);
  PG_HIP(hipGetLastError());
  t_end(0);
  int hc[3];
  counters.download(hc, 3);
  const int nnear = hc[0];
  c->n_cut_local = nnear;
  auto waves = [](i64 items) { return dim3((unsigned)((items * 64 + 255) / 256)); };
  if (nnear > 0) {
    ran[1] = true;
    t_begin(1);
    hipLaunchKernelGGL(k_st_cells<St>, waves(nnear), dim3(256), 0, st, g, mv, sa, near_list.p, nnear, so);
    PG_HIP(hipGetLastError());
    t_end(1);
  }
  // at most N faces / staggered volumes per near cell and per neighbour of one (1-D: every face is evaluated)
  const i64 cap = std::min<i64>((i64)N * Ml, (N == 1 ? (i64)Ml : (i64)6 * N * (i64)nnear) + 1024);
  DevBuf<int> list2(2 * cap);
  t_begin(2);
  hipLaunchKernelGGL(k_st_sections, dim3(gr), dim3(256), 0, st, g, mv, Ml, c->ct.p, c->A[0].p, c->A[1].p, c->A[2].p, c->B[0].p,
                     c->B[1].p, c->B[2].p, list2.p, counters.p + 1, (int)cap);
  PG_HIP(hipGetLastError());
  t_end(2);
  counters.download(hc, 3);
  PG_REQUIRE(hc[1] <= cap, "internal: space-time section work list overflow");
  if (hc[1] > 0) {
    ran[3] = true;
    t_begin(3);
    hipLaunchKernelGGL(k_st_sections_cut<St>, waves(hc[1]), dim3(256), 0, st, g, mv, sa, list2.p, hc[1], c->Cw[0].p, c->Cw[1].p,
                       c->Cw[2].p, c->A[0].p, c->A[1].p, c->A[2].p, c->B[0].p, c->B[1].p, c->B[2].p);
    PG_HIP(hipGetLastError());
    t_end(3);
  }
  t_begin(4);
  hipLaunchKernelGGL(k_st_stagger, dim3(gr), dim3(256), 0, st, g, mv, Ml, c->ct.p, c->Cw[0].p, c->Cw[1].p, c->Cw[2].p, c->W[0].p,
                     c->W[1].p, c->W[2].p, list2.p, counters.p + 2, (int)cap);
  PG_HIP(hipGetLastError());
  t_end(4);
  counters.download(hc, 3);
  PG_REQUIRE(hc[2] <= cap, "internal: space-time staggered-volume work list overflow");
  if (hc[2] > 0) {
    ran[5] = true;
    t_begin(5);
    hipLaunchKernelGGL(k_st_stagger_cut<St>, waves(hc[2]), dim3(256), 0, st, g, mv, sa, list2.p, hc[2], c->Cw[0].p, c->Cw[1].p,
                       c->Cw[2].p, c->W[0].p, c->W[1].p, c->W[2].p);
    PG_HIP(hipGetLastError());
    t_end(5);
  }
  PG_HIP(hipEventRecord(ev.e1, st));
  PG_HIP(hipEventSynchronize(ev.e1));
  float ms = 0.f;
  PG_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  c->kernel_ms = ms;
  for (int k = 0; parts && k < 6; ++k) {
    parts[k] = 0.0;
    if (!ran[k]) continue;
    PG_HIP(hipEventElapsedTime(&ms, part[k].e0, part[k].e1));
    parts[k] = ms;
  }
}

// c_prog is one table per process: two host threads building program capacities at once take turns
std::mutex g_prog_mutex;
// measurement only (pg_debug_spacetime_kernel_timing): each of the six kernels of a program or polygon body between its own events
bool g_st_timing = false;

}  // namespace

namespace pg {
CapView cap_view(const pg_capacity* c) {
  CapView v;
  v.N = c->N;
  for (int d = 0; d < 3; ++d) {
    v.ext[d] = c->slab.ext[d];
    v.n[d] = c->slab.n[d];
    v.stride[d] = c->slab.stride[d];
    v.A[d] = c->A[d].p;
    v.B[d] = c->B[d].p;
    v.W[d] = c->W[d].p;
  }
  v.plane = c->slab.plane;
  v.s0 = c->slab.s0;
  v.s1 = c->slab.s1;
  v.nplanes = c->slab.nplanes;
  v.V = c->V.p;
  v.G = c->G.p;
  return v;
}
}  // namespace pg

extern "C" {

int32_t pg_capacity_create_levelset(pg_mesh* m, int32_t body_kind, const double* params, int32_t nparams,
                                    int32_t flags, pg_capacity** out) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(m && params && out, "pg_capacity_create_levelset: NULL argument");
  Context& cx = ctx();
  const int N = m->N;
  BallSet bs;
  std::memset(&bs, 0, sizeof(bs));
  bs.N = N;
  bs.complement = (flags & PG_FLAG_COMPLEMENT) ? 1 : 0;
  for (int d = 0; d < 3; ++d) bs.ax[d] = 1.0;
  if (body_kind == PG_BODY_BALL) {
    PG_REQUIRE(nparams == N + 1, "PG_BODY_BALL expects params = {c_1..c_N, r}");
    bs.nballs = 1;
    for (int d = 0; d < N; ++d) bs.c[0][d] = params[d];
    bs.r = params[N];
  } else if (body_kind == PG_BODY_MULTIBALL) {
    PG_REQUIRE(nparams >= 2, "PG_BODY_MULTIBALL expects params = {r, nballs, centres...}");
    bs.r = params[0];
    bs.nballs = (int)params[1];
    PG_REQUIRE(bs.nballs >= 1 && bs.nballs <= MAX_BALLS, "PG_BODY_MULTIBALL: 1..16 balls");
    PG_REQUIRE(nparams == 2 + bs.nballs * N, "PG_BODY_MULTIBALL: wrong parameter count");
    PG_REQUIRE(!bs.complement, "PG_BODY_MULTIBALL: complement not supported");
    for (int s = 0; s < bs.nballs; ++s)
      for (int d = 0; d < N; ++d) bs.c[s][d] = params[2 + s * N + d];
  } else if (body_kind == PG_BODY_HALFSPACE) {
    PG_REQUIRE(nparams == 3, "PG_BODY_HALFSPACE expects params = {axis (0-based), position, sign}");
    bs.kind = BODY_HALFSPACE;
    bs.axis = (int)params[0];
    bs.pos = params[1];
    bs.sgn = params[2] < 0.0 ? -1.0 : 1.0;
    bs.nballs = 1;
    bs.r = 1.0;
    PG_REQUIRE(bs.axis >= 0 && bs.axis < N && (double)bs.axis == params[0], "PG_BODY_HALFSPACE: axis must be 0 .. N-1");
  } else if (body_kind == PG_BODY_ELLIPSOID) {
    PG_REQUIRE(nparams == 2 * N, "PG_BODY_ELLIPSOID expects params = {c_1..c_N, a_1..a_N}");
    bs.nballs = 1;
    bs.r = 1.0;
    for (int d = 0; d < N; ++d) {
      bs.c[0][d] = params[d];
      bs.ax[d] = params[N + d];
      PG_REQUIRE(bs.ax[d] > 0.0, "PG_BODY_ELLIPSOID: semi-axes must be positive");
    }
    if (N == 1) bs.r = bs.ax[0];                 // an interval: the 1-D ball
    else bs.kind = BODY_ELLIPSOID;
  } else if (body_kind == PG_BODY_PLANE) {
    PG_REQUIRE(nparams == N + 1, "PG_BODY_PLANE expects params = {n_1..n_N, offset}");
    bs.kind = BODY_PLANE;
    bs.nballs = 1;
    bs.r = 1.0;
    double nn = 0.0;
    for (int d = 0; d < N; ++d) {
      PG_REQUIRE(std::isfinite(params[d]), "PG_BODY_PLANE: the normal must be finite");
      bs.c[0][d] = params[d];                    // as passed: the classification never normalises
      nn = std::max(nn, std::fabs(params[d]));
    }
    PG_REQUIRE(nn > 0.0, "PG_BODY_PLANE: the normal must not be zero");
    PG_REQUIRE(std::isfinite(params[N]), "PG_BODY_PLANE: the offset must be finite");
    bs.pos = params[N];
  } else {
    throw Error("pg_capacity_create_levelset: unknown body kind (arbitrary bodies: use pg_capacity_create_from_arrays)");
  }
  PG_REQUIRE(bs.r > 0.0, "ball radius must be positive");

  auto* c = new pg_capacity();
  std::unique_ptr<pg_capacity> guard(c);
  c->mesh = m;
  c->N = N;
  c->from_body = true;
  c->has_cg = !(flags & PG_FLAG_NO_CENTROIDS);
  c->body = bs;
  c->slab = m->base_slab();
  ensure_gl();
  hipStream_t st = cx.stream;

  // ---- slab partition balanced by non-empty cells per plane ----------------
  if (cx.nranks > 1 || cx.comm) {
    const Slab& s = c->slab;
    PG_REQUIRE(s.nplanes >= cx.nranks, "fewer planes than ranks");
    GeoView g = geo_view(m, s);
    DevBuf<unsigned long long> w(s.nplanes);
    w.zero();
    const i64 lo = s.nplanes * cx.rank / cx.nranks, hi = s.nplanes * (cx.rank + 1) / cx.nranks;
    if (hi > lo)
      hipLaunchKernelGGL(k_plane_weights, dim3(grid_for((hi - lo) * s.plane, 256)), dim3(256), 0, st, g, bs, lo, hi, w.p);
    PG_HIP(hipGetLastError());
    comm_allreduce_sum_u64(w.p, s.nplanes, st);
    std::vector<unsigned long long> hw(s.nplanes);
    w.download(hw.data(), s.nplanes);
    std::vector<i64> wt(hw.begin(), hw.end()), bounds(cx.nranks + 1);
    PG_REQUIRE(pg_partition_planes(wt.data(), s.nplanes, cx.nranks, bounds.data()) == 0, "partition failed");
    c->slab.set_own(bounds[cx.rank], bounds[cx.rank + 1]);
  }

  BallArg ba;
  static_cast<BallSet&>(ba) = bs;
  if (bs.kind == BODY_PLANE) run_static_kernels<PG_PLANE_CUT_LANES>(c, m, ba, st);
  else run_static_kernels<CUT_LANES>(c, m, ba, st);
  *out = guard.release();
  PG_API_END
}

int32_t pg_capacity_create_program(pg_mesh* m, const pg_program* phi, const pg_program* grad, int32_t flags, pg_capacity** out) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(m && phi && out, "pg_capacity_create_program: NULL argument");
  Context& cx = ctx();
  PG_REQUIRE(cx.nranks == 1 && !cx.comm, "pg_capacity_create_program: single rank only (program bodies on slabs are not supported yet)");
  const int N = m->N;
  {
    i64 n[3];
    const double* nodes[3];
    for (int d = 0; d < N; ++d) { n[d] = m->n[d]; nodes[d] = m->nodes[d].data(); }
    std::string why;
    PG_REQUIRE(program_body_check(N, n, nodes, phi, grad, &why),
               "pg_capacity_create_program refused: " + why + (N == 3 && grad ? ": pg_capacity_create_program3 takes a 3-D mesh" : ""));
  }
  auto* c = new pg_capacity();
  std::unique_ptr<pg_capacity> guard(c);
  c->mesh = m;
  c->N = N;
  c->from_body = true;
  c->has_cg = !(flags & PG_FLAG_NO_CENTROIDS);
  std::memset(&c->body, 0, sizeof(c->body));     // (not a BallSet: nothing reads it)
  c->slab = m->base_slab();
  ensure_gl();
  pg_program progs[3];
  std::memset(progs, 0, sizeof(progs));
  progs[0] = *phi;
  for (int d = 0; d < N; ++d) progs[1 + d] = grad[d];
  std::lock_guard<std::mutex> table(g_prog_mutex);   // held until the last kernel of this capacity has run
  PG_HIP(hipStreamSynchronize(cx.stream));       // (no earlier launch may still read the table)
  PG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_prog), progs, sizeof(progs)));
  ProgArg pa;
  pa.N = N;
  pa.sgn = (flags & PG_FLAG_COMPLEMENT) ? -1.0 : 1.0;
  run_static_kernels<CUT_LANES>(c, m, pa, cx.stream);
  *out = guard.release();
  PG_API_END
}

int32_t pg_capacity_create_program3(pg_mesh* m, const pg_program* phi, const pg_program* grad, int32_t flags, pg_capacity** out) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(m && out, "pg_capacity_create_program3: NULL argument");
  *out = nullptr;                                // (a missing program is named by program3_body_check below)
  Context& cx = ctx();
  {
    i64 n[3] = {1, 1, 1};
    const double* nodes[3] = {nullptr, nullptr, nullptr};
    for (int d = 0; d < m->N; ++d) { n[d] = m->n[d]; nodes[d] = m->nodes[d].data(); }
    std::string why;
    PG_REQUIRE(program3_body_check(m->N, n, nodes, phi, grad, cx.nranks == 1 && !cx.comm, &why),
               "pg_capacity_create_program3 refused: " + why);
  }
  auto* c = new pg_capacity();
  std::unique_ptr<pg_capacity> guard(c);
  c->mesh = m;
  c->N = 3;
  c->from_body = true;
  c->has_cg = !(flags & PG_FLAG_NO_CENTROIDS);
  std::memset(&c->body, 0, sizeof(c->body));     // (not a BallSet: nothing reads it)
  c->slab = m->base_slab();
  ensure_gl();
  pg_program progs[5];
  std::memset(progs, 0, sizeof(progs));
  progs[0] = *phi;
  progs[P3_DX] = grad[0];
  progs[P3_DY] = grad[1];
  progs[P3_DZ] = grad[2];
  std::lock_guard<std::mutex> table(g_prog_mutex);   // held until the last kernel of this capacity has run
  PG_HIP(hipStreamSynchronize(cx.stream));       // (no earlier launch may still read the table)
  PG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_prog), progs, sizeof(progs)));
  Prog3Arg pa;
  pa.sgn = (flags & PG_FLAG_COMPLEMENT) ? -1.0 : 1.0;
  run_static_kernels<64>(c, m, pa, cx.stream);   // one wave per cut box
  *out = guard.release();
  PG_API_END
}

int32_t pg_capacity_create_polygon(pg_mesh* m, const double* xy, int64_t M, int32_t flags, pg_capacity** out) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(m && out, "pg_capacity_create_polygon: NULL argument");
  *out = nullptr;
  Context& cx = ctx();
  PG_REQUIRE(m->N == 2, "pg_capacity_create_polygon: a marker polygon is a 2-D body, the mesh is " + std::to_string(m->N) + "-D");
  PG_REQUIRE(cx.nranks == 1 && !cx.comm, "pg_capacity_create_polygon: single rank only (polygon bodies on slabs are not supported yet)");
  M = polygon_open_count(xy, M);
  {
    std::string why;
    PG_REQUIRE(polygon_body_check(xy, M, &why), "pg_capacity_create_polygon refused: " + why);
  }
  PG_REQUIRE(m->n[0] < (i64)1 << 30 && m->n[1] < (i64)1 << 30 && m->n[0] + m->n[1] + m->n[0] * m->n[1] < (i64)2147483647 - 1,
             "pg_capacity_create_polygon: the edge lookup exceeds 2^31 bins");
  const std::vector<double> ccw = polygon_normalise(xy, M);
  auto* c = new pg_capacity();
  std::unique_ptr<pg_capacity> guard(c);
  c->mesh = m;
  c->N = 2;
  c->from_body = true;
  c->has_cg = !(flags & PG_FLAG_NO_CENTROIDS);
  std::memset(&c->body, 0, sizeof(c->body));     // (not a BallSet: nothing reads it)
  c->slab = m->base_slab();
  ensure_gl();
  hipStream_t st = cx.stream;
  const GeoView g = geo_view(m, c->slab);
  DevBuf<double> dxy(2 * M);
  dxy.upload(ccw.data(), 2 * M);
  PolyArg pa;
  pa.N = 2;
  pa.complement = 0;
  pa.flip = (flags & PG_FLAG_COMPLEMENT) ? 1 : 0;
  pa.M = (int)M;
  pa.xy = dxy.p;
  for (int d = 0; d < 2; ++d) { pa.n[d] = (int)m->n[d]; pa.nodes[d] = g.nodes[d]; }
  pa.ptr = nullptr;
  pa.idx = nullptr;
  PolyBins bins;                                 // the edge lookup: count, scan, fill, order
  build_poly_bins(static_cast<const PolyBody&>(pa), m, "pg_capacity_create_polygon", st, bins);
  pa.ptr = bins.ptr.p;
  pa.idx = bins.idx.p;
  run_static_kernels<CUT_LANES>(c, m, pa, st);   // (waits for its last kernel: the lists above outlive every launch)
  c->poly_bin_ms = bins.ms;
  *out = guard.release();
  PG_API_END
}

int32_t pg_capacity_polygon_ms_parts(const pg_capacity* c, double* ms) {
  PG_API_BEGIN
  PG_REQUIRE(c && ms, "pg_capacity_polygon_ms_parts: NULL argument");
  for (int k = 0; k < 5; ++k) ms[k] = c->kernel_ms_parts[k];
  ms[5] = c->poly_bin_ms;
  PG_API_END
}

int32_t pg_capacity_create_from_arrays(pg_mesh* m, const double* V, const double* const* A, const double* const* B,
                                       const double* const* W, const double* Gamma, const double* const* C_omega,
                                       const double* const* C_gamma, const double* cell_types, pg_capacity** out) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(m && V && A && B && W && Gamma && C_omega && cell_types && out, "pg_capacity_create_from_arrays: NULL argument");
  PG_REQUIRE(ctx().nranks == 1, "pg_capacity_create_from_arrays: single rank only");
  auto* c = new pg_capacity();
  std::unique_ptr<pg_capacity> guard(c);
  c->mesh = m;
  c->N = m->N;
  c->from_body = false;
  c->has_cg = C_gamma != nullptr;
  c->slab = m->base_slab();
  alloc_fields(c);
  const i64 M = c->slab.M;
  c->V.upload(V, M);
  c->G.upload(Gamma, M);
  c->ct.upload(cell_types, M);
  for (int d = 0; d < c->N; ++d) {
    c->A[d].upload(A[d], M);
    c->B[d].upload(B[d], M);
    c->W[d].upload(W[d], M);
    c->Cw[d].upload(C_omega[d], M);
    if (c->has_cg) c->Cg[d].upload(C_gamma[d], M);
  }
  *out = guard.release();
  PG_API_END
}

int32_t pg_capacity_create_spacetime(pg_mesh* m, const pg_motion_desc* mo, pg_capacity** out) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(m && mo && out && mo->nodes, "pg_capacity_create_spacetime: NULL argument");
  AsyncAllocScope pool;   // one capacity per time slab: the stream-ordered allocator (pg_common.h)
  PG_REQUIRE(ctx().nranks == 1 && !ctx().comm, "pg_capacity_create_spacetime: single rank only");
  const int N = m->N;
  PG_REQUIRE(N == 1 || N == 2, "space-time capacities: 1-D+t and 2-D+t (the reference's 3-D+t blocks drop the z direction)");
  PG_REQUIRE(mo->body_kind == PG_BODY_BALL || mo->body_kind == PG_BODY_HALFSPACE, "moving body: PG_BODY_BALL or PG_BODY_HALFSPACE");
  PG_REQUIRE(mo->nq >= 1 && mo->nq <= 4096, "pg_capacity_create_spacetime: 1 .. 4096 time nodes");
  PG_REQUIRE(mo->t1 > mo->t0, "pg_capacity_create_spacetime: empty time slab");
  MotionView mv;
  std::memset(&mv, 0, sizeof(mv));
  mv.kind = mo->body_kind == PG_BODY_HALFSPACE ? BODY_HALFSPACE : BODY_BALLS;
  mv.complement = (mo->flags & PG_FLAG_COMPLEMENT) ? 1 : 0;
  mv.axis = mo->axis;
  mv.sgn = mo->sign < 0.0 ? -1.0 : 1.0;
  mv.nq = mo->nq;
  mv.t0 = mo->t0;
  mv.t1 = mo->t1;
  if (mv.kind == BODY_HALFSPACE) PG_REQUIRE(mv.axis >= 0 && mv.axis < N, "moving half space: axis must be 0 .. N-1");
  std::vector<MotionNode> hq(mo->nq);
  double wsum = 0.0;
  for (int k = 0; k < mo->nq; ++k) {
    const double* r = mo->nodes + (size_t)k * 10;
    MotionNode& q = hq[k];
    q.tau = r[0]; q.w = r[1];
    for (int d = 0; d < 3; ++d) { q.c[d] = r[2 + d]; q.dc[d] = r[6 + d]; }
    q.r = r[5]; q.dr = r[9];
    PG_REQUIRE(q.tau > mo->t0 && q.tau < mo->t1, "time nodes must lie inside (t0, t1)");
    if (mv.kind == BODY_BALLS) PG_REQUIRE(q.r > 0.0, "ball radius must be positive");
    wsum += q.w;
  }
  PG_REQUIRE(fabs(wsum - (mo->t1 - mo->t0)) <= 1e-12 * (mo->t1 - mo->t0), "time weights must add up to t1 - t0");
  for (int e = 0; e < 2; ++e) {
    const double* b = e == 0 ? mo->body0 : mo->body1;
    std::memset(&mv.end[e], 0, sizeof(MotionNode));
    mv.end[e].tau = e == 0 ? mo->t0 : mo->t1;
    for (int d = 0; d < 3; ++d) mv.end[e].c[d] = b[d];
    mv.end[e].r = b[3];
    if (mv.kind == BODY_BALLS) PG_REQUIRE(b[3] > 0.0, "ball radius must be positive");
  }
  DevBuf<MotionNode> dq(mo->nq);
  dq.upload(hq.data(), mo->nq);
  mv.q = dq.p;
  {
    const double tm = 0.5 * (mo->t0 + mo->t1);
    int km = 0;
    for (int k = 1; k < mo->nq; ++k)
      if (fabs(hq[k].tau - tm) < fabs(hq[km].tau - tm)) km = k;
    mv.mid = hq[km];
    double reach = 0.0;
    auto dist = [&](const MotionNode& q) {
      double dc = 0.0;
      if (mv.kind == BODY_HALFSPACE) return fabs(q.c[0] - mv.mid.c[0]);
      for (int d = 0; d < N; ++d) dc += (q.c[d] - mv.mid.c[d]) * (q.c[d] - mv.mid.c[d]);
      return std::sqrt(dc) + fabs(q.r - mv.mid.r);
    };
    for (int k = 0; k < mo->nq; ++k) reach = std::max(reach, dist(hq[k]));
    reach = std::max(reach, std::max(dist(mv.end[0]), dist(mv.end[1])));
    mv.reach = reach * (1.0 + 1e-12) + 1e-300;
  }
  std::vector<BallSet> hb(mo->nq + 2);
  for (int k = 0; k < mo->nq + 2; ++k) {
    const MotionNode& q = k < mo->nq ? hq[k] : mv.end[k - mo->nq];
    BallSet& b = hb[k];
    std::memset(&b, 0, sizeof(b));
    b.N = N; b.nballs = 1; b.complement = mv.complement; b.kind = mv.kind; b.axis = mv.axis; b.sgn = mv.sgn;
    b.r = mv.kind == BODY_HALFSPACE ? 1.0 : q.r;
    b.pos = mv.kind == BODY_HALFSPACE ? q.c[0] : 0.0;
    for (int d = 0; d < 3; ++d) { b.c[0][d] = mv.kind == BODY_HALFSPACE ? 0.0 : q.c[d]; b.ax[d] = 1.0; }
  }
  DevBuf<BallSet> dbodies(mo->nq + 2);
  dbodies.upload(hb.data(), mo->nq + 2);
  mv.bodies = dbodies.p;

  auto* c = new pg_capacity();
  std::unique_ptr<pg_capacity> guard(c);
  c->mesh = m;
  c->N = N;
  c->from_body = false;        // (the stored body is not the geometry: nothing may re-evaluate it)
  c->has_cg = !(mo->flags & PG_FLAG_NO_CENTROIDS);
  c->spacetime = true;
  c->t0 = mo->t0;
  c->t1 = mo->t1;
  c->slab = m->base_slab();
  ensure_gl();
  run_spacetime_kernels(c, m, mv, StBall(), ctx().stream, nullptr);
  *out = guard.release();
  PG_API_END
}

int32_t pg_capacity_create_spacetime_program(pg_mesh* m, const pg_program* phi, const pg_program* grad, const pg_program* dphidt,
                                             int32_t flags, double t0, double t1, int32_t nq, const double* tau_w,
                                             pg_capacity** out) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(m && out, "pg_capacity_create_spacetime_program: NULL argument");
  *out = nullptr;                                // (a missing program or rule is named by spacetime_program_check below)
  PG_REQUIRE(ctx().nranks == 1 && !ctx().comm,
             "pg_capacity_create_spacetime_program: single rank only (program bodies on slabs are not supported yet)");
  const int N = m->N;
  {
    i64 n[3];
    const double* nodes[3];
    for (int d = 0; d < N; ++d) { n[d] = m->n[d]; nodes[d] = m->nodes[d].data(); }
    std::string why;
    PG_REQUIRE(spacetime_program_check(N, n, nodes, phi, grad, dphidt, t0, t1, nq, tau_w, &why),
               N == 1 || N == 2 ? "pg_capacity_create_spacetime_program refused: " + why : why);
  }
  AsyncAllocScope pool;   // one capacity per time slab: the stream-ordered allocator (pg_common.h)
  MotionView mv;
  std::memset(&mv, 0, sizeof(mv));
  mv.kind = BODY_BALLS;          // (not read: the body is the program)
  mv.sgn = 1.0;
  mv.nq = nq;
  mv.t0 = t0;
  mv.t1 = t1;
  std::vector<MotionNode> hq(nq);
  for (int k = 0; k < nq; ++k) {
    std::memset(&hq[k], 0, sizeof(MotionNode));
    hq[k].tau = tau_w[2 * k];
    hq[k].w = tau_w[2 * k + 1];
  }
  DevBuf<MotionNode> dq(nq);
  dq.upload(hq.data(), nq);
  mv.q = dq.p;

  auto* c = new pg_capacity();
  std::unique_ptr<pg_capacity> guard(c);
  c->mesh = m;
  c->N = N;
  c->from_body = false;
  c->has_cg = !(flags & PG_FLAG_NO_CENTROIDS);
  std::memset(&c->body, 0, sizeof(c->body));     // (not a BallSet: nothing reads it)
  c->spacetime = true;
  c->t0 = t0;
  c->t1 = t1;
  c->slab = m->base_slab();
  ensure_gl();
  pg_program progs[4];
  std::memset(progs, 0, sizeof(progs));
  progs[0] = *phi;
  for (int d = 0; d < N; ++d) progs[1 + d] = grad[d];
  progs[3] = *dphidt;
  std::lock_guard<std::mutex> table(g_prog_mutex);   // held until the last kernel of this capacity has run
  PG_HIP(hipStreamSynchronize(ctx().stream));    // (no earlier launch may still read the table)
  PG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_prog), progs, sizeof(progs)));
  StProg sp;
  sp.N = N;
  sp.sgn = (flags & PG_FLAG_COMPLEMENT) ? -1.0 : 1.0;
  run_spacetime_kernels(c, m, mv, sp, ctx().stream, g_st_timing ? c->st_ms_parts : nullptr);
  *out = guard.release();
  PG_API_END
}

// compute_spacetime_capacities(mesh, front_n, front_np1, dt) -- src/front_tracking.jl:1472
int32_t pg_capacity_create_spacetime_polygon(pg_mesh* m, const double* xy0, const double* xy1, int64_t M, int32_t flags, double t0,
                                             double t1, int32_t nq, const double* tau_w, pg_capacity** out) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(m, "pg_capacity_create_spacetime_polygon: NULL mesh");
  PG_REQUIRE(out, "pg_capacity_create_spacetime_polygon: NULL output pointer");
  *out = nullptr;                                // (missing markers or a missing rule are named by spacetime_polygon_check below)
  PG_REQUIRE(ctx().nranks == 1 && !ctx().comm,
             "pg_capacity_create_spacetime_polygon: single rank only (polygon bodies on slabs are not supported yet)");
  M = moving_polygon_open_count(xy0, xy1, M);
  {
    std::string why;
    PG_REQUIRE(spacetime_polygon_check(m->N, xy0, xy1, M, t0, t1, nq, tau_w, &why), "pg_capacity_create_spacetime_polygon refused: " + why);
  }
  PG_REQUIRE(m->n[0] < (i64)1 << 30 && m->n[1] < (i64)1 << 30 && m->n[0] + m->n[1] + m->n[0] * m->n[1] < (i64)2147483647 - 1,
             "pg_capacity_create_spacetime_polygon: the edge lookup exceeds 2^31 bins");
  const std::vector<double> ccw0 = polygon_normalise_as(xy0, xy0, M), ccw1 = polygon_normalise_as(xy1, xy0, M);
  AsyncAllocScope pool;   // one capacity per time slab: the stream-ordered allocator (pg_common.h)
  hipStream_t st = ctx().stream;
  MotionView mv;
  std::memset(&mv, 0, sizeof(mv));
  mv.kind = BODY_BALLS;          // (not read: the body is the polygon; the phase lives in its flip)
  mv.sgn = 1.0;
  mv.nq = nq;
  mv.t0 = t0;
  mv.t1 = t1;
  std::vector<MotionNode> hq(nq);
  for (int k = 0; k < nq; ++k) {
    std::memset(&hq[k], 0, sizeof(MotionNode));
    hq[k].tau = tau_w[2 * k];
    hq[k].w = tau_w[2 * k + 1];
    hq[k].c[0] = (hq[k].tau - t0) / (t1 - t0);   // s_k of the interpolating view
  }
  DevBuf<MotionNode> dq(nq);
  dq.upload(hq.data(), nq);
  mv.q = dq.p;

  auto* c = new pg_capacity();
  std::unique_ptr<pg_capacity> guard(c);
  c->mesh = m;
  c->N = 2;
  c->from_body = false;
  c->has_cg = !(flags & PG_FLAG_NO_CENTROIDS);
  std::memset(&c->body, 0, sizeof(c->body));     // (not a BallSet: nothing reads it)
  c->spacetime = true;
  c->t0 = t0;
  c->t1 = t1;
  c->slab = m->base_slab();
  ensure_gl();
  const GeoView g = geo_view(m, c->slab);
  DevBuf<double> dxy0(2 * M), dxy1(2 * M);
  dxy0.upload(ccw0.data(), 2 * M);
  dxy1.upload(ccw1.data(), 2 * M);
  StPoly sp;
  sp.N = 2;
  sp.complement = 0;
  sp.flip = (flags & PG_FLAG_COMPLEMENT) ? 1 : 0;
  sp.M = (int)M;
  sp.xy = dxy0.p;
  sp.xy1 = dxy1.p;
  for (int d = 0; d < 2; ++d) { sp.n[d] = (int)m->n[d]; sp.nodes[d] = g.nodes[d]; }
  sp.ptr = nullptr;
  sp.idx = nullptr;
  sp.s = 0.0;
  sp.dt = t1 - t0;
  sp.face = 1;
  PolyBins bins;                                 // of the swept edges: one table for every node and both faces
  build_poly_bins(static_cast<const MovingPoly&>(sp), m, "pg_capacity_create_spacetime_polygon", st, bins);
  sp.ptr = bins.ptr.p;
  sp.idx = bins.idx.p;
  run_spacetime_kernels(c, m, mv, sp, st, g_st_timing ? c->st_ms_parts : nullptr);   // (waits for its last kernel)
  c->poly_bin_ms = bins.ms;
  *out = guard.release();
  PG_API_END
}

int32_t pg_debug_spacetime_kernel_timing(int32_t on) {
  PG_API_BEGIN
  g_st_timing = on != 0;
  PG_API_END
}

int32_t pg_debug_capacity_spacetime_ms_parts(const pg_capacity* c, double* ms, int64_t* n_listed) {
  PG_API_BEGIN
  PG_REQUIRE(c && ms && n_listed, "pg_debug_capacity_spacetime_ms_parts: NULL argument");
  PG_REQUIRE(c->spacetime, "pg_debug_capacity_spacetime_ms_parts: not a space-time capacity");
  for (int k = 0; k < 6; ++k) ms[k] = c->st_ms_parts[k];
  *n_listed = c->n_cut_local;
  PG_API_END
}

int32_t pg_capacity_set_spacetime(pg_capacity* c, double t0, double t1, const double* V_t0, const double* V_t1,
                                  const double* Ct_omega, const double* Ct_gamma) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(c && V_t0 && V_t1, "pg_capacity_set_spacetime: NULL argument");
  PG_REQUIRE(!c->from_body && ctx().nranks == 1, "pg_capacity_set_spacetime: for capacities built from arrays, single rank");
  const i64 M = c->slab.M;
  c->Vt[0].alloc(M); c->Vt[1].alloc(M); c->Ctw.alloc(M); c->Ctg.alloc(M);
  c->Vt[0].upload(V_t0, M);
  c->Vt[1].upload(V_t1, M);
  c->Ctw.zero(); c->Ctg.zero();
  if (Ct_omega) c->Ctw.upload(Ct_omega, M);
  if (Ct_gamma) c->Ctg.upload(Ct_gamma, M);
  c->spacetime = true;
  c->t0 = t0; c->t1 = t1;
  PG_API_END
}

int32_t pg_capacity_destroy(pg_capacity* c) {
  PG_API_BEGIN
  delete c;
  PG_API_END
}

int32_t pg_capacity_get(const pg_capacity* c, int32_t field, int32_t d, double* out, int64_t len) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(c && out, "pg_capacity_get: NULL argument");
  PG_REQUIRE(len == c->slab.M, "pg_capacity_get: len must be prod(n_d+1)");
  const DevBuf<double>* src = nullptr;
  switch (field) {
    case PG_CAP_V: src = &c->V; break;
    case PG_CAP_GAMMA: src = &c->G; break;
    case PG_CAP_CELL_TYPES: src = &c->ct; break;
    case PG_CAP_A: case PG_CAP_B: case PG_CAP_W: case PG_CAP_C_OMEGA: case PG_CAP_C_GAMMA:
      PG_REQUIRE(d >= 0 && d < c->N, "pg_capacity_get: bad dimension");
      src = field == PG_CAP_A ? &c->A[d] : field == PG_CAP_B ? &c->B[d] : field == PG_CAP_W ? &c->W[d]
          : field == PG_CAP_C_OMEGA ? &c->Cw[d] : &c->Cg[d];
      break;
    case PG_CAP_ST_V0: case PG_CAP_ST_V1: case PG_CAP_ST_CT_OMEGA: case PG_CAP_ST_CT_GAMMA:
      PG_REQUIRE(c->spacetime, "pg_capacity_get: not a space-time capacity");
      src = field == PG_CAP_ST_V0 ? &c->Vt[0] : field == PG_CAP_ST_V1 ? &c->Vt[1] : field == PG_CAP_ST_CT_OMEGA ? &c->Ctw : &c->Ctg;
      break;
    default: throw Error("pg_capacity_get: unknown field");
  }
  PG_REQUIRE(src->p != nullptr, "pg_capacity_get: field not available (centroids disabled?)");
  src->download(out + c->slab.first_cell(), c->slab.Mloc());
  PG_API_END
}

int32_t pg_capacity_kernel_ms(const pg_capacity* c, double* ms) {
  PG_API_BEGIN
  PG_REQUIRE(c && ms, "pg_capacity_kernel_ms: NULL argument");
  *ms = c->kernel_ms;
  PG_API_END
}

int32_t pg_capacity_kernel_ms_parts(const pg_capacity* c, double* ms) {
  PG_API_BEGIN
  PG_REQUIRE(c && ms, "pg_capacity_kernel_ms_parts: NULL argument");
  for (int k = 0; k < 5; ++k) ms[k] = c->kernel_ms_parts[k];
  PG_API_END
}

int32_t pg_diffops_create(pg_capacity* c, pg_diffops** out) {
  PG_API_BEGIN
  PG_REQUIRE(c && out, "pg_diffops_create: NULL argument");
  auto* o = new pg_diffops();
  o->cap = c;
  *out = o;
  PG_API_END
}

int32_t pg_diffops_destroy(pg_diffops* o) {
  PG_API_BEGIN
  delete o;
  PG_API_END
}

}  // extern "C"
