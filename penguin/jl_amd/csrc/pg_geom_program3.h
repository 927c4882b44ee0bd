// pg_geom_program3.h -- cut-cell geometry of a TRACED level set in 3-D: pick_ball, box_measure and section_measure, the three
// primitives the capacity kernels reach a body through, for a body given as a pg_program phi(x, y, z) and the three programs of
// its partial derivatives.  Capacity(body::Function, mesh) of the reference (src/capacity.jl:51-123) in 3-D.  Fluid is where
// phi <= 0.  Usable from HIP kernels and from a host (g++) build, like pg_geom_program.h, whose conventions it keeps unchanged
// (9 samples per segment, Illinois regula falsi to <= 2 ulp, pieces by the sign at their midpoint, 16 Gauss-Legendre nodes per
// piece, NaN counts as solid, touching is EMPTY); compile with -ffp-contract=off.
//
//   box type    the 9 samples of each of the 12 edges, the 6 face centres and the cell centre, left as soon as both signs have
//               been seen.  FULL if all are <= 0, else EMPTY if all are >= 0, else CUT
//   box         the axes are ordered by |d phi / d x_d| at the box centre (ties: the later axis): heights run along the
//               largest, v; the inner integration along the middle one, u; the outer along the smallest, w.  Outer breakpoints
//               are the box ends and the roots of phi along the 4 edges parallel to w, streamed in ascending order (the four
//               edges of one sample interval are merged in registers); every outer piece has 16 nodes in w, and at each the
//               2-D rule of pg_geom_program.h runs in the plane w = const: breakpoints in u are the box ends and the roots of
//               phi on the two lines v = lo_v, v = hi_v, 16 nodes per piece, one pass along v at each.  A root strictly inside
//               adds w_u w_w |grad phi| / |d_v phi| to the interface measure.  Moments about the box's lower corner
//   section     {x_d = s} /\ box is the 2-D box rule of pg_geom_program.h on a view of the body with x_d fixed (SliceEval)
//
// Limit: a cell in which the trace of the interface on a face v = const turns back in w, or d_v phi vanishes (the cells around
// the six "poles" of a closed body), has a square-root singularity inside an outer piece and is integrated across it, as the 2-D
// kind integrates across a kink (DESIGN.md section 27 has the measured error).
// Nothing is indexed in private memory: axes are picked with selects, roots and breakpoints are consumed as they are found.
#pragma once
#include "pg_geom_program.h"

#if defined(__HIPCC__)
#define PG_HD_FLAT __host__ __device__ __forceinline__
#else
#define PG_HD_FLAT inline
#endif

namespace pggeom {

// Eval: value(which, x, y, z) runs program `which` at a point: 0 phi, 1 d/dx, 2 d/dy, 4 d/dz (3 is d/dt of the moving 2-D
// bodies; the table keeps its slot).  `which` is a literal at every call, as in ProgBody.
constexpr int P3_DX = 1, P3_DY = 2, P3_DZ = 4;

template <class Eval>
struct Prog3Body {
  int N;                        // always 3
  int complement;               // always 0: the sign lives in sgn
  double sgn;                   // -1: PG_FLAG_COMPLEMENT
  Eval ev;
  PG_HD double f(double x, double y, double z) const {
    const double v = sgn * ev.value(0, x, y, z);
    return v == v ? v : 1.0;
  }
  PG_HD void grad(double x, double y, double z, double g[3]) const {
    g[0] = sgn * ev.value(P3_DX, x, y, z);
    g[1] = sgn * ev.value(P3_DY, x, y, z);
    g[2] = sgn * ev.value(P3_DZ, x, y, z);
  }
};

struct HostEval3 {
  const pg_program* phi;
  const pg_program* grad;       // 3 programs
  pgprog::HostStack* S;
  double value(int which, double x, double y, double z) const {
    return pgprog::prog_eval(which == 0 ? *phi : grad[which == P3_DZ ? 2 : which - 1], x, y, z, 0.0, *S);
  }
};

// The body with x_d = s, as the evaluator of a 2-D ProgBody: (a, b) are the two other coordinates in ascending order.  The
// derivative programs are reached through branches with a literal index each, so lanes of one wave may hold different d.
template <class Eval>
struct SliceEval {
  Eval ev;
  int d;
  double s;
  PG_HD double value(int which, double a, double b, double) const {
    const double x = d == 0 ? s : a, y = d == 0 ? a : d == 1 ? s : b, z = d == 2 ? s : b;
    if (which == 0) return ev.value(0, x, y, z);
    if (which == 1) return d == 0 ? ev.value(P3_DY, x, y, z) : ev.value(P3_DX, x, y, z);
    return d == 2 ? ev.value(P3_DY, x, y, z) : ev.value(P3_DZ, x, y, z);
  }
};
template <class Eval>
using SliceBody = ProgBody<SliceEval<Eval>>;
template <class Eval>
PG_HD SliceBody<Eval> slice_body(const Prog3Body<Eval>& bs, int d, double s) {
  return SliceBody<Eval>{2, 0, bs.sgn, SliceEval<Eval>{bs.ev, d, s}};
}

struct Axes3 {
  int u, v, w;                  // a permutation of 0, 1, 2
};
PG_HD double pick3(int i, double a0, double a1, double a2) { return i == 0 ? a0 : i == 1 ? a1 : a2; }
PG_HD double pick3(int i, const double* a) { return pick3(i, a[0], a[1], a[2]); }

// phi at the point whose coordinates along (u, v, w) are (cu, cv, cw)
template <class Body>
PG_HD double f_uvw(const Body& b, const Axes3& ax, double cu, double cv, double cw) {
  return b.f(ax.u == 0 ? cu : ax.v == 0 ? cv : cw, ax.u == 1 ? cu : ax.v == 1 ? cv : cw, ax.u == 2 ? cu : ax.v == 2 ? cv : cw);
}
template <class Body>
struct AlongU {
  const Body& b; const Axes3& ax; double cv, cw;
  PG_HD double operator()(double s) const { return f_uvw(b, ax, s, cv, cw); }
};
template <class Body>
struct AlongV {
  const Body& b; const Axes3& ax; double cu, cw;
  PG_HD double operator()(double s) const { return f_uvw(b, ax, cu, s, cw); }
};
template <class Body>
struct AlongW {
  const Body& b; const Axes3& ax; double cu, cv;
  PG_HD double operator()(double s) const { return f_uvw(b, ax, cu, cv, s); }
};

// seg_measure of pg_geom_program.h along v at (u, w) = (cu, cw), the surface weight from the 3-D gradient
template <class Body>
PG_HD void seg_measure3(const Body& bs, const Axes3& ax, double cu, double cw, double a, double b, bool want_surface, SegOut& o) {
  const AlongV<Body> f{bs, ax, cu, cw};
  o.len = o.mom = o.nroots = o.rsum = o.gw = o.gwr = 0.0;
  double p = a;
  auto piece = [&](double q) {
    if (q > p) {
      if (f(0.5 * (p + q)) <= 0.0) {
        o.len += q - p;
        o.mom += (q - p) * (0.5 * ((q - a) + (p - a)));
      }
      p = q;
    }
  };
  auto root = [&](double q) {
    o.nroots += 1.0;
    o.rsum += q - a;
    if (want_surface && q > a && q < b) {
      double g[3];
      bs.grad(ax.u == 0 ? cu : ax.v == 0 ? q : cw, ax.u == 1 ? cu : ax.v == 1 ? q : cw, ax.u == 2 ? cu : ax.v == 2 ? q : cw, g);
      const double gv = fabs(pick3(ax.v, g));
      const double w = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) / gv;
      if (gv > 0.0 && w < 1e300) {                // (a NaN or an infinite weight adds nothing)
        o.gw += w;
        o.gwr += w * (q - a);
      }
    }
    piece(q);
  };
  double xp = a, fp = f(a);
  o.all_in = fp <= 0.0;
  o.all_out = fp > 0.0;
  for (int k = 1; k <= LS_NS; ++k) {
    const double xk = ls_sample(a, b, k), fk = f(xk);
    o.all_in = o.all_in && fk <= 0.0;
    o.all_out = o.all_out && fk > 0.0;
    if (fp == 0.0) root(xp);
    else if ((fp < 0.0 && fk > 0.0) || (fp > 0.0 && fk < 0.0)) root(refine_root(f, xp, fp, xk, fk));
    xp = xk;
    fp = fk;
  }
  if (fp == 0.0 && b > a) root(b);
  piece(b);
}

// FULL / EMPTY / CUT of a box on the sample lattice: 12 edges x 9 samples (a corner is looked at once), 6 face centres, the centre
template <class Eval>
PG_HD int prog3_box_type(const Prog3Body<Eval>& bs, const double* lo, const double* hi) {
  bool in = true, out = true;
  auto look = [&](double x, double y, double z) {
    const double v = bs.f(x, y, z);
    in = in && v <= 0.0;
    out = out && v >= 0.0;
  };
  for (int k = 0; k <= LS_NS && (in || out); ++k) {                 // the 4 edges along x, corners included
    const double x = ls_sample(lo[0], hi[0], k);
    look(x, lo[1], lo[2]); look(x, hi[1], lo[2]); look(x, lo[1], hi[2]); look(x, hi[1], hi[2]);
  }
  for (int k = 1; k < LS_NS && (in || out); ++k) {
    const double y = ls_sample(lo[1], hi[1], k);
    look(lo[0], y, lo[2]); look(hi[0], y, lo[2]); look(lo[0], y, hi[2]); look(hi[0], y, hi[2]);
  }
  for (int k = 1; k < LS_NS && (in || out); ++k) {
    const double z = ls_sample(lo[2], hi[2], k);
    look(lo[0], lo[1], z); look(hi[0], lo[1], z); look(lo[0], hi[1], z); look(hi[0], hi[1], z);
  }
  if (in || out) {
    const double cx = 0.5 * (lo[0] + hi[0]), cy = 0.5 * (lo[1] + hi[1]), cz = 0.5 * (lo[2] + hi[2]);
    look(lo[0], cy, cz); look(hi[0], cy, cz);
    look(cx, lo[1], cz); look(cx, hi[1], cz);
    look(cx, cy, lo[2]); look(cx, cy, hi[2]);
    look(cx, cy, cz);
  }
  return in ? PG_FULL : out ? PG_EMPTY : PG_CUT;
}

template <class Eval>
PG_HD int pick_ball(const Prog3Body<Eval>& bs, const double* lo, const double* hi, int& type) {
  type = prog3_box_type(bs, lo, hi);
  return 0;
}

// partial moments about the lower corner, along the box's own (u, v, w)
struct Acc3 {
  double vol, mu, mv, mw, gam, gu, gv, gw;
};

// the 2-D rule in the plane w = cw, its results weighted by wo (the outer Gauss-Legendre weight); this caller takes the inner
// nodes ilane, ilane + istride, ... of every piece
template <class Body>
PG_HD void plane_measure3(const Body& bs, const Axes3& ax, double cw, double wo, double dw, double ua, double ub, double va,
                          double vb, bool want_surface, const GLTable& gl, int ilane, int istride, Acc3& m) {
  const AlongU<Body> e0{bs, ax, va, cw}, e1{bs, ax, vb, cw};
  double p = ua;
  auto piece = [&](double q) {
    if (!(q > p)) return;
    const double um = 0.5 * (p + q), uh = 0.5 * (q - p);
    for (int k = ilane; k < NGL; k += istride) {
      const double uu = um + uh * gl.x[k], w = wo * (gl.w[k] * uh);
      SegOut s;
      seg_measure3(bs, ax, uu, cw, va, vb, want_surface, s);
      m.vol += w * s.len;
      m.mv += w * s.mom;
      m.mu += w * (s.len * (uu - ua));
      m.mw += w * (s.len * dw);
      if (want_surface) {
        m.gam += w * s.gw;
        m.gv += w * s.gwr;
        m.gu += w * (s.gw * (uu - ua));
        m.gw += w * (s.gw * dw);
      }
    }
    p = q;
  };
  double xp = ua, f0p = e0(ua), f1p = e1(ua);
  for (int k = 1; k <= LS_NS; ++k) {
    const double xk = ls_sample(ua, ub, k), f0k = e0(xk), f1k = e1(xk);
    if (f0p == 0.0 || f1p == 0.0) piece(xp);
    const bool h0 = (f0p < 0.0 && f0k > 0.0) || (f0p > 0.0 && f0k < 0.0);
    const bool h1 = (f1p < 0.0 && f1k > 0.0) || (f1p > 0.0 && f1k < 0.0);
    const double r0 = h0 ? refine_root(e0, xp, f0p, xk, f0k) : ub;
    const double r1 = h1 ? refine_root(e1, xp, f1p, xk, f1k) : ub;
    if (h0 || h1) piece(dmin(r0, r1));                              // (a missing root is ub: the larger of the two)
    if (h0 && h1) piece(dmax(r0, r1));
    xp = xk; f0p = f0k; f1p = f1k;
  }
  piece(ub);
}

PG_HD bool ls_crosses(double fp, double fk) { return (fp < 0.0 && fk > 0.0) || (fp > 0.0 && fk < 0.0); }

// qlane / qstride: this caller's share of the quadrature.  With o = min(qstride, 16) it takes the outer nodes qlane % o,
// qlane % o + o, ... of every outer piece and, at each, the inner nodes qlane / o, qlane / o + qstride / o, ... of every inner
// piece: (0, 1) is everything (the host form), (l, 64) is one wave per box, lane l at outer node l & 15 and inner nodes
// l >> 4, (l >> 4) + 4, ...  `group` adds the partial moments up.
// (PG_HD_FLAT: in a kernel the rule is part of its one caller, so the result is never returned through memory)
template <class Eval, class Group = NoGroup>
PG_HD_FLAT BoxMeasure box_measure(const Prog3Body<Eval>& bs, const double* lo, const double* hi, bool want_surface, const GLTable& gl,
                             int qlane = 0, int qstride = 1, Group group = Group()) {
  BoxMeasure o;
  o.vol = 0.0; o.gamma = 0.0;
  bool degenerate = false;
  for (int d = 0; d < 3; ++d) {
    o.cg[d] = 0.0;
    o.cen[d] = 0.5 * (lo[d] + hi[d]);
    if (!(hi[d] - lo[d] > 0.0)) degenerate = true;
  }
  o.type = prog3_box_type(bs, lo, hi);
  const double full = prod_ext(lo, hi, 3, -1);
  if (degenerate || o.type != PG_CUT) {
    o.vol = (!degenerate && o.type == PG_FULL) ? full : 0.0;
    return o;
  }
  const int ostride = qstride < NGL ? qstride : NGL, olane = qlane % ostride;
  const int istride = qstride / ostride, ilane = qlane / ostride;
  double g[3];
  bs.grad(o.cen[0], o.cen[1], o.cen[2], g);
  g[0] = fabs(g[0]); g[1] = fabs(g[1]); g[2] = fabs(g[2]);
  Axes3 ax;
  ax.v = 0;
  if (g[1] >= g[0]) ax.v = 1;
  if (g[2] >= pick3(ax.v, g)) ax.v = 2;
  {
    const int a = ax.v == 0 ? 1 : 0, b = ax.v == 2 ? 1 : 2;         // the two others, a < b
    ax.u = pick3(a, g) > pick3(b, g) ? a : b;
    ax.w = ax.u == a ? b : a;
  }
  const double ua = pick3(ax.u, lo), ub = pick3(ax.u, hi), va = pick3(ax.v, lo), vb = pick3(ax.v, hi);
  const double wa = pick3(ax.w, lo), wb = pick3(ax.w, hi);
  Acc3 m;
  m.vol = m.mu = m.mv = m.mw = m.gam = m.gu = m.gv = m.gw = 0.0;
  const AlongW<Prog3Body<Eval>> e0{bs, ax, ua, va}, e1{bs, ax, ub, va}, e2{bs, ax, ua, vb}, e3{bs, ax, ub, vb};
  double p = wa;
  auto piece = [&](double q) {
    if (!(q > p)) return;
    const double wm = 0.5 * (p + q), wh = 0.5 * (q - p);
    for (int k = olane; k < NGL; k += ostride) {
      const double ww = wm + wh * gl.x[k];
      plane_measure3(bs, ax, ww, gl.w[k] * wh, ww - wa, ua, ub, va, vb, want_surface, gl, ilane, istride, m);
    }
    p = q;
  };
  double xp = wa, f0p = e0(wa), f1p = e1(wa), f2p = e2(wa), f3p = e3(wa);
  for (int k = 1; k <= LS_NS; ++k) {
    const double xk = ls_sample(wa, wb, k), f0k = e0(xk), f1k = e1(xk), f2k = e2(xk), f3k = e3(xk);
    if (f0p == 0.0 || f1p == 0.0 || f2p == 0.0 || f3p == 0.0) piece(xp);
    const bool h0 = ls_crosses(f0p, f0k), h1 = ls_crosses(f1p, f1k), h2 = ls_crosses(f2p, f2k), h3 = ls_crosses(f3p, f3k);
    const int nh = (h0 ? 1 : 0) + (h1 ? 1 : 0) + (h2 ? 1 : 0) + (h3 ? 1 : 0);
    if (nh > 0) {
      // the roots of this sample interval in ascending order (a missing one is wb, the largest): a 5-comparator network
      const double r0 = h0 ? refine_root(e0, xp, f0p, xk, f0k) : wb, r1 = h1 ? refine_root(e1, xp, f1p, xk, f1k) : wb;
      const double r2 = h2 ? refine_root(e2, xp, f2p, xk, f2k) : wb, r3 = h3 ? refine_root(e3, xp, f3p, xk, f3k) : wb;
      const double a0 = dmin(r0, r1), a1 = dmax(r0, r1), b0 = dmin(r2, r3), b1 = dmax(r2, r3);
      const double c1 = dmax(a0, b0), c2 = dmin(a1, b1);
      piece(dmin(a0, b0));
      if (nh > 1) piece(dmin(c1, c2));
      if (nh > 2) piece(dmax(c1, c2));
      if (nh > 3) piece(dmax(a1, b1));
    }
    xp = xk; f0p = f0k; f1p = f1k; f2p = f2k; f3p = f3k;
  }
  piece(wb);
  Mom mm;
  mm.vol = m.vol;
  mm.gamma = m.gam;
  for (int d = 0; d < 3; ++d) {
    mm.m[d] = ax.u == d ? m.mu : ax.v == d ? m.mv : m.mw;
    mm.gm[d] = ax.u == d ? m.gu : ax.v == d ? m.gv : m.gw;
  }
  group(mm);
  double vol = mm.vol;
  if (!(vol > 0.0)) vol = 0.0;                    // (also a NaN)
  if (vol > full) vol = full;
  o.vol = vol;
  if (vol > 0.0)
    for (int d = 0; d < 3; ++d) {
      const double c = lo[d] + mm.m[d] / vol;
      if (c >= lo[d] && c <= hi[d]) o.cen[d] = c;
      else if (c < lo[d]) o.cen[d] = lo[d];
      else if (c > hi[d]) o.cen[d] = hi[d];
    }
  if (mm.gamma > 0.0 && mm.gamma < 1e300) {
    o.gamma = mm.gamma;
    for (int d = 0; d < 3; ++d) {
      const double c = lo[d] + mm.gm[d] / mm.gamma;
      o.cg[d] = c >= lo[d] ? (c <= hi[d] ? c : hi[d]) : lo[d];
    }
  }
  return o;
}

// fluid measure of {x_d = s} /\ box: the 2-D box rule of pg_geom_program.h on the slice, its axis choice made at the section's
// centre -- restated here for the area alone (a face has no moments to take), with the axes picked by selects and the sum in one
// scalar, so that nothing is indexed in private memory; term for term the sum of the 2-D box_measure.  A section whose lattice
// (4 edges x 9 samples and the centre) is all fluid returns the caller's full measure, so that A - B between full neighbours
// stays an exact zero; one whose lattice is all solid returns 0.  qlane / qstride / group: as the 2-D box_measure.
template <class Eval, class Group = NoGroup>
PG_HD double section_measure(const Prog3Body<Eval>& bs, int d, double s, const double* lo, const double* hi, double full_measure,
                             const GLTable& gl, int qlane = 0, int qstride = 1, Group group = Group()) {
  const int a = d == 0 ? 1 : 0, b = d == 2 ? 1 : 2;
  const double lo2[2] = {pick3(a, lo), pick3(b, lo)}, hi2[2] = {pick3(a, hi), pick3(b, hi)};
  const double ext = (hi2[0] - lo2[0]) * (hi2[1] - lo2[1]);
  if (!(hi2[0] - lo2[0] > 0.0) || !(hi2[1] - lo2[1] > 0.0)) return 0.0;
  const SliceBody<Eval> sb = slice_body(bs, d, s);
  const int type = prog_box_type(sb, lo2, hi2);
  if (type == PG_FULL) return full_measure >= 0.0 ? full_measure : ext;
  if (type == PG_EMPTY) return 0.0;
  double gx, gy;
  sb.grad(0.5 * (lo2[0] + hi2[0]), 0.5 * (lo2[1] + hi2[1]), gx, gy);
  const int v = fabs(gx) > fabs(gy) ? 0 : 1, u = 1 - v;
  const double ua = v == 0 ? lo2[1] : lo2[0], ub = v == 0 ? hi2[1] : hi2[0], va = v == 0 ? lo2[0] : lo2[1], vb = v == 0 ? hi2[0] : hi2[1];
  const LineFn<SliceBody<Eval>> e0{sb, u, va}, e1{sb, u, vb};
  double area = 0.0, p = ua;
  auto piece = [&](double q) {
    if (!(q > p)) return;
    const double um = 0.5 * (p + q), uh = 0.5 * (q - p);
    for (int k = qlane; k < NGL; k += qstride) {
      SegOut so;
      seg_measure(sb, v, um + uh * gl.x[k], va, vb, false, so);
      area += (gl.w[k] * uh) * so.len;
    }
    p = q;
  };
  double xp = ua, f0p = e0(ua), f1p = e1(ua);
  for (int k = 1; k <= LS_NS; ++k) {
    const double xk = ls_sample(ua, ub, k), f0k = e0(xk), f1k = e1(xk);
    if (f0p == 0.0 || f1p == 0.0) piece(xp);
    const bool h0 = ls_crosses(f0p, f0k), h1 = ls_crosses(f1p, f1k);
    const double r0 = h0 ? refine_root(e0, xp, f0p, xk, f0k) : ub;
    const double r1 = h1 ? refine_root(e1, xp, f1p, xk, f1k) : ub;
    if (h0 || h1) piece(dmin(r0, r1));
    if (h0 && h1) piece(dmax(r0, r1));
    xp = xk; f0p = f0k; f1p = f1k;
  }
  piece(ub);
  Mom mm;
  mm.vol = area;
  mm.gamma = 0.0;
  for (int q = 0; q < 3; ++q) mm.m[q] = mm.gm[q] = 0.0;
  group(mm);
  if (!(mm.vol > 0.0)) return 0.0;                // (also a NaN)
  return mm.vol < ext ? mm.vol : ext;
}

// Host only: what pg_capacity_create_program3 refuses before it allocates anything, each with its own message: a missing
// program, a mesh that is not 3-D, more than one rank, invalid programs, a program that reads t, and a gradient that disagrees
// with central differences of phi (step 1e-6 h_d) at the centres of up to 64 real cells spread over the mesh, within
// 1e-4 max(|grad phi|, 1).  A point where either side is not finite decides nothing.
inline bool program3_body_check(int N, const int64_t* n, const double* const* nodes /* n_d + 1 each */, const pg_program* phi,
                                const pg_program* grad, bool single_rank, std::string* why) {
  auto fail = [&](const std::string& m) {
    if (why) *why = m;
    return false;
  };
  if (!phi) return fail("NULL level-set program");
  if (!grad) return fail("grad == NULL: the 3 programs of d phi / d x_d are needed (DeviceFunction.gradient_programs(3) builds them)");
  if (N != 3) return fail("the mesh must be 3-D, it is " + std::to_string(N) + "-D (1-D and 2-D: pg_capacity_create_program)");
  if (!single_rank) return fail("single rank only (program bodies on slabs are not supported yet)");
  for (int k = 0; k <= 3; ++k) {
    const pg_program* p = k == 0 ? phi : grad + (k - 1);
    const std::string name = k == 0 ? std::string("the level-set program") : "gradient program " + std::to_string(k - 1);
    std::string w;
    if (!pgprog::program_validate(p, &w)) return fail(name + " is invalid: " + w);
    for (int q = 0; q < p->n_ops; ++q)
      if (p->op[q] == PG_OP_VAR && p->arg[q] == 3)
        return fail(name + " reads t (instruction " + std::to_string(q) + "): a body does not depend on time");
  }
  int64_t M = 1;
  for (int d = 0; d < 3; ++d) M *= n[d];
  const int64_t npts = M < 64 ? M : 64;
  pgprog::HostStack S;
  for (int64_t k = 0; k < npts; ++k) {
    int64_t cell = npts > 1 ? (k * (M - 1)) / (npts - 1) : 0;
    double x[3], h[3];
    for (int d = 0; d < 3; ++d) {
      const int64_t j = cell % n[d];
      x[d] = 0.5 * (nodes[d][j] + nodes[d][j + 1]);
      h[d] = (nodes[d][n[d]] - nodes[d][0]) / (double)n[d];
      cell /= n[d];
    }
    double g[3], fd[3], gn = 0.0;
    for (int d = 0; d < 3; ++d) {
      const double e = 1e-6 * h[d];
      double xp[3] = {x[0], x[1], x[2]}, xm[3] = {x[0], x[1], x[2]};
      xp[d] += e; xm[d] -= e;
      fd[d] = (pgprog::prog_eval(*phi, xp[0], xp[1], xp[2], 0.0, S) - pgprog::prog_eval(*phi, xm[0], xm[1], xm[2], 0.0, S)) / (xp[d] - xm[d]);
      g[d] = pgprog::prog_eval(grad[d], x[0], x[1], x[2], 0.0, S);
      gn += g[d] * g[d];
    }
    const double tol = 1e-4 * dmax(sqrt(gn), 1.0);
    for (int d = 0; d < 3; ++d)
      if (fabs(g[d] - fd[d]) > tol)                 // (false for a NaN)
        return fail("gradient program " + std::to_string(d) + " gives " + std::to_string(g[d]) + " at (" + std::to_string(x[0]) + ", " +
                    std::to_string(x[1]) + ", " + std::to_string(x[2]) + ") where central differences of the level set give " +
                    std::to_string(fd[d]));
  }
  return true;
}

}  // namespace pggeom
