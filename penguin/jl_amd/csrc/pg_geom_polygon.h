// pg_geom_polygon.h -- cut-cell geometry of a MARKER POLYGON (the reference's FrontTracker, src/front_tracking.jl): the three
// primitives the capacity kernels reach a body through (pick_ball, box_measure, section_measure of pg_geom.h) for a simple
// closed polygon of M >= 3 markers in 2-D, counter-clockwise.  Fluid is the interior (get_fluid_polygon); flip = 1
// (PG_FLAG_COMPLEMENT) makes it the exterior.  Usable from HIP kernels and from a host (g++) build, like pg_geom.h; compile with
// -ffp-contract=off.  No transcendental is evaluated: every capacity is a finite sum of polynomial terms in the markers and the
// box, one division per crossing and one square root per piece of the front.
//
// Conventions (tests/polygon_reference.py restates them in exact rational arithmetic):
//   crossing    edge (p, q) crosses the line x_d = s iff (p_d <= s) != (q_d <= s); the crossing's coordinate on the other axis
//               o is p_o + (s - p_d)(q_o - p_o) / (q_d - p_d), clamped to the edge's own range
//   inside      even-odd: the point (x, y) is inside iff an odd number of crossings of the line x_1 = y have a coordinate <= x
//   section     the fluid length of {x_d = s} and [lo_o, hi_o]: the parity at lo_o (the crossings <= lo_o), then the crossings
//               strictly inside (lo_o, hi_o) in ascending order; with none of them the caller's exact `full`, or 0
//   pieces      an edge is clipped to the CLOSED box (Liang-Barsky); only a piece of positive length counts
//   box type    CUT iff some piece has its midpoint strictly inside the OPEN box; otherwise FULL or EMPTY by the box centre.  A
//               box that only touches the polygon is not CUT, as every other kind has it
//   box         Green's theorem about the box's lower corner, over the pieces (in the polygon's direction) and the fluid parts of
//               the box's right and top edges (taken with the section rule):
//                 V = sum int (x - lo_0) dy + (hi_0 - lo_0) L_right,  M_0 = sum int (x - lo_0)^2 / 2 dy + (hi_0 - lo_0)^2 / 2 L_right,
//                 M_1 = - sum int (y - lo_1)^2 / 2 dx + (hi_1 - lo_1)^2 / 2 L_top;  the exterior: the pieces reversed
//   front       Gamma is the length of the pieces whose midpoint m has lo <= m < hi on both axes -- every point of the front
//               belongs to one cell, an edge along a node line to the cell above / to the right of it, whatever that cell's type
//               -- and C_gamma their length-weighted mean midpoint
//   a box over several cells (the staggered boxes of W) is the sum over those cells of measure(box and cell): a cell's edge list
//   serves the part of the box inside that cell, no edge is visited twice.  Boxes lie inside the mesh.
//
// Edge lookup: one CSR table over nx + ny + nx ny bins -- the columns, the rows, the cells -- of the edges whose bounding box
// meets the bin's closed extent (cells: of the edges that pass within one row of it inside its column), edge ids ascending in
// every bin, so every floating-point sum has one order.  A line x_0 = s is served by the bucket of the column that holds s (every
// edge that can cross it is there), a line x_1 = s by a row's: the work of a cell is bounded by its own row, column and cell
// lists, never by M.  Listing an edge in a bin it does not reach is harmless: it crosses and clips to nothing there.
// No loop has a bound other than a list length, an index range of the mesh or a constant, and nothing is indexed in private
// memory: crossings are consumed in ascending order by a repeated "next larger than the last" scan, never stored.
#pragma once
#include "pg_geom.h"

#include <cmath>
#include <string>
#include <vector>

namespace pggeom {

struct PolyBody {
  int N;                        // 2
  int complement;               // always 0: the phase lives in flip, the kernels' own complement flip must not apply
  int flip;                     // 1: PG_FLAG_COMPLEMENT (fluid is the exterior)
  int M;                        // markers = edges; edge k runs from marker k to marker (k + 1) mod M
  const double* xy;             // 2 M: x0 y0 x1 y1 ..., counter-clockwise
  int n[2];                     // cells of the mesh
  const double* nodes[2];       // n_d + 1 each
  const int* ptr;               // n0 + n1 + n0 n1 + 1: bin b holds idx[ptr[b] .. ptr[b + 1])
  const int* idx;               // edge ids, ascending in every bin
};

// A MOVING polygon inside one time slab [t0, t1] (the reference's interpolate_front, src/front_tracking.jl:2289-2307): two marker
// arrays of the same length and order, every marker on a straight line at constant speed.  The view is the polygon at ONE time:
// vertex i is xy[i] + s (xy1[i] - xy[i]) in this order of operations, s = (tau - t0) / (t1 - t0), interpolated when it is read --
// nothing is stored per time.  The two time faces are taken by slot, not by s: face 1 reads xy, face 2 reads xy1, exactly.
// Its edge lookup lists the SWEPT edge (poly_edge_bins below), so one table serves every time of the slab.  Its front measure
// carries the space-time factor: Gamma is the sum over the owned pieces of len sqrt(1 + v_n^2), v_n the normal speed at the
// piece's midpoint, and C_gamma the mean of the midpoints with the same weights (box_measure below).
struct MovingPoly : PolyBody {
  const double* xy1;            // 2 M: the markers at t1 (xy: at t0), the same normalisation applied to both
  double s;                     // (tau - t0) / (t1 - t0) of this view; not read at a face
  double dt;                    // t1 - t0
  int face;                     // 0: a time inside the slab, 1: the face t0, 2: the face t1
};

PG_HD void poly_vertex(const PolyBody& b, int k, double& x, double& y) {
  x = b.xy[2 * k];
  y = b.xy[2 * k + 1];
}
PG_HD void poly_vertex(const MovingPoly& b, int k, double& x, double& y) {
  if (b.face == 2) { x = b.xy1[2 * k]; y = b.xy1[2 * k + 1]; return; }
  x = b.xy[2 * k];
  y = b.xy[2 * k + 1];
  if (b.face == 1) return;
  x = x + b.s * (b.xy1[2 * k] - x);
  y = y + b.s * (b.xy1[2 * k + 1] - y);
}
// the velocity of marker k: (p1 - p0) / (t1 - t0)
PG_HD void poly_velocity(const MovingPoly& b, int k, double& ux, double& uy) {
  ux = (b.xy1[2 * k] - b.xy[2 * k]) / b.dt;
  uy = (b.xy1[2 * k + 1] - b.xy[2 * k + 1]) / b.dt;
}

PG_HD int poly_col_bin(const PolyBody&, int i) { return i; }
PG_HD int poly_row_bin(const PolyBody& b, int j) { return b.n[0] + j; }
PG_HD int poly_cell_bin(const PolyBody& b, int i, int j) { return b.n[0] + b.n[1] + j * b.n[0] + i; }

template <class P>
PG_HD void poly_edge(const P& b, int k, double& px, double& py, double& qx, double& qy) {
  const int k1 = k + 1 < b.M ? k + 1 : 0;
  poly_vertex(b, k, px, py);
  poly_vertex(b, k1, qx, qy);
}

// the cell of axis d that holds s: the largest i in [0, n_d - 1] with nodes_d[i] <= s, 0 if there is none
PG_HD int poly_locate(const PolyBody& b, int d, double s) {
  const double* x = b.nodes[d];
  int lo = 0, hi = b.n[d] - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (x[mid] <= s) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// the cells of axis d whose closed extent meets [a, z]; false: none (the interval lies outside the mesh)
PG_HD bool poly_range(const PolyBody& b, int d, double a, double z, int& i0, int& i1) {
  const double* x = b.nodes[d];
  if (z < x[0] || a > x[b.n[d]]) return false;
  i0 = poly_locate(b, d, a);
  if (i0 > 0 && x[i0] == a) --i0;               // on a node: the cell below touches it too
  i1 = poly_locate(b, d, z);
  return true;
}

// Every bin edge k belongs to, each once: its columns, its rows, and in each of its columns the cells of the rows it passes
// through inside that column, one more row on either side (its heights at the column's ends are rounded).  At most
// 2 (n0 + n1) + 3 n0 + n1 visits.
template <class Visit>
PG_HD void poly_edge_bins(const PolyBody& b, int k, Visit visit) {
  double px, py, qx, qy;
  poly_edge(b, k, px, py, qx, qy);
  const double xa = dmin(px, qx), xz = dmax(px, qx), ya = dmin(py, qy), yz = dmax(py, qy);
  int c0 = 0, c1 = -1, r0 = 0, r1 = -1;
  const bool hc = poly_range(b, 0, xa, xz, c0, c1), hr = poly_range(b, 1, ya, yz, r0, r1);
  if (hc)
    for (int i = c0; i <= c1; ++i) visit(poly_col_bin(b, i));
  if (hr)
    for (int j = r0; j <= r1; ++j) visit(poly_row_bin(b, j));
  if (!(hc && hr)) return;
  for (int i = c0; i <= c1; ++i) {
    double ylo = ya, yhi = yz;
    if (qx != px) {
      const double sa = dmax(b.nodes[0][i], xa), sz = dmin(b.nodes[0][i + 1], xz);
      const double slope = (qy - py) / (qx - px);
      const double y0 = py + (sa - px) * slope, y1 = py + (sz - px) * slope;
      ylo = dmax(ya, dmin(y0, y1));
      yhi = dmin(yz, dmax(y0, y1));
    }
    int j0, j1;
    if (!poly_range(b, 1, ylo, yhi, j0, j1)) { j0 = r0; j1 = r1; }     // (rounding at the mesh's border: the whole range)
    j0 = j0 - 1 > r0 ? j0 - 1 : r0;
    j1 = j1 + 1 < r1 ? j1 + 1 : r1;
    for (int j = j0; j <= j1; ++j) visit(poly_cell_bin(b, i, j));
  }
}

// The bins of the SWEPT edge k of a moving polygon: the bounding box of p0_k, q0_k, p1_k, q1_k.  Both ends move on straight
// lines, so by convexity every position of the edge during the slab lies inside that box, and the interpolated coordinates
// leave it by rounding only: the box is widened by 2^-50 of its largest coordinate.  Its columns, its rows and every cell of
// both; listing an edge where it does not reach is harmless, so the one table serves every time node and both faces.
template <class Visit>
PG_HD void poly_edge_bins(const MovingPoly& b, int k, Visit visit) {
  const int k1 = k + 1 < b.M ? k + 1 : 0;
  const double x[4] = {b.xy[2 * k], b.xy[2 * k1], b.xy1[2 * k], b.xy1[2 * k1]};
  const double y[4] = {b.xy[2 * k + 1], b.xy[2 * k1 + 1], b.xy1[2 * k + 1], b.xy1[2 * k1 + 1]};
  double xa = dmin(dmin(x[0], x[1]), dmin(x[2], x[3])), xz = dmax(dmax(x[0], x[1]), dmax(x[2], x[3]));
  double ya = dmin(dmin(y[0], y[1]), dmin(y[2], y[3])), yz = dmax(dmax(y[0], y[1]), dmax(y[2], y[3]));
  const double ex = 0x1p-50 * dmax(fabs(xa), fabs(xz)), ey = 0x1p-50 * dmax(fabs(ya), fabs(yz));
  xa -= ex; xz += ex; ya -= ey; yz += ey;
  int c0 = 0, c1 = -1, r0 = 0, r1 = -1;
  const bool hc = poly_range(b, 0, xa, xz, c0, c1), hr = poly_range(b, 1, ya, yz, r0, r1);
  if (hc)
    for (int i = c0; i <= c1; ++i) visit(poly_col_bin(b, i));
  if (hr)
    for (int j = r0; j <= r1; ++j) visit(poly_row_bin(b, j));
  if (!(hc && hr)) return;
  for (int j = r0; j <= r1; ++j)
    for (int i = c0; i <= c1; ++i) visit(poly_cell_bin(b, i, j));
}

// does the edge cross the line x_d = s, and where on the other axis
PG_HD bool poly_cross(double pd, double po, double qd, double qo, double s, double& c) {
  if ((pd <= s) == (qd <= s)) return false;
  const double v = po + (s - pd) * (qo - po) / (qd - pd);
  const double a = dmin(po, qo), z = dmax(po, qo);
  c = v < a ? a : v > z ? z : v;
  return true;
}

template <class P>
PG_HD bool poly_cross_edge(const P& b, int k, int d, double s, double& c) {
  double px, py, qx, qy;
  poly_edge(b, k, px, py, qx, qy);
  return d == 0 ? poly_cross(px, py, qx, qy, s, c) : poly_cross(py, px, qy, qx, s, c);
}

PG_HD int poly_line_bin(const PolyBody& b, int d, double s) {
  const int i = poly_locate(b, d, s);
  return d == 0 ? poly_col_bin(b, i) : poly_row_bin(b, i);
}

// is the point fluid
template <class P>
PG_HD bool poly_fluid_at(const P& b, double x, double y) {
  const int bin = poly_line_bin(b, 1, y);
  int below = 0;
  for (int e = b.ptr[bin]; e < b.ptr[bin + 1]; ++e) {
    double c;
    if (poly_cross_edge(b, b.idx[e], 1, y, c) && c <= x) ++below;
  }
  return ((below & 1) != 0) != (b.flip != 0);
}

// fluid length of {x_d = s} and [a, z] on the other axis, z > a; `full`: what a wholly fluid section returns
template <class P>
PG_HD double poly_section(const P& b, int d, double s, double a, double z, double full) {
  const int bin = poly_line_bin(b, d, s);
  const int e0 = b.ptr[bin], e1 = b.ptr[bin + 1];
  int below = 0, inside = 0;
  for (int e = e0; e < e1; ++e) {
    double c;
    if (!poly_cross_edge(b, b.idx[e], d, s, c)) continue;
    if (c <= a) ++below;
    else if (c < z) ++inside;
  }
  bool fluid = ((below & 1) != 0) != (b.flip != 0);
  if (inside == 0) return fluid ? full : 0.0;
  double len = 0.0, last = a;
  for (int it = 0; it < inside; ++it) {          // the next crossing above `last`, with its multiplicity
    double best = z;
    int mult = 0;
    for (int e = e0; e < e1; ++e) {
      double c;
      if (!poly_cross_edge(b, b.idx[e], d, s, c) || !(c > last && c < z)) continue;
      if (c < best) { best = c; mult = 1; }
      else if (c == best) ++mult;
    }
    if (mult == 0) break;
    if (fluid) len += best - last;
    if (mult & 1) fluid = !fluid;
    last = best;
  }
  if (fluid) len += z - last;
  return len < z - a ? len : z - a;
}

// Liang-Barsky: the piece of p -> q inside the closed box, in the edge's direction; false: none of positive length.  lambda: the
// parameter of the piece's midpoint on the edge, m = p + lambda (q - p)
PG_HD bool poly_clip(double px, double py, double qx, double qy, double lo0, double lo1, double hi0, double hi1, double& ax,
                     double& ay, double& bx, double& by, double& lambda) {
  double t0 = 0.0, t1 = 1.0;
  const double dx = qx - px, dy = qy - py;
  auto side = [&](double p, double q) {          // p t <= q
    if (p == 0.0) return q >= 0.0;
    const double r = q / p;
    if (p < 0.0) {
      if (r > t1) return false;
      if (r > t0) t0 = r;
    } else {
      if (r < t0) return false;
      if (r < t1) t1 = r;
    }
    return true;
  };
  if (!side(-dx, px - lo0) || !side(dx, hi0 - px) || !side(-dy, py - lo1) || !side(dy, hi1 - py)) return false;
  if (!(t1 > t0)) return false;
  lambda = 0.5 * (t0 + t1);
  ax = t0 == 0.0 ? px : px + t0 * dx;
  ay = t0 == 0.0 ? py : py + t0 * dy;
  bx = t1 == 1.0 ? qx : px + t1 * dx;
  by = t1 == 1.0 ? qy : py + t1 * dy;
  ax = dmin(dmax(ax, lo0), hi0); bx = dmin(dmax(bx, lo0), hi0);
  ay = dmin(dmax(ay, lo1), hi1); by = dmin(dmax(by, lo1), hi1);
  return true;
}
PG_HD bool poly_clip(double px, double py, double qx, double qy, double lo0, double lo1, double hi0, double hi1, double& ax,
                     double& ay, double& bx, double& by) {
  double lambda;
  return poly_clip(px, py, qx, qy, lo0, lo1, hi0, hi1, ax, ay, bx, by, lambda);
}

// what a piece of the front weighs: its length -- and for a moving polygon len sqrt(1 + v_n^2), the space-time measure of the
// strip it sweeps per unit time: v_n = u(m) . n, u(m) = u_p + lambda (u_q - u_p) the velocity of the edge's point at the piece's
// midpoint (u_i = (p1_i - p0_i) / (t1 - t0)) and n = (dy, -dx) / len the edge's unit normal at this time.  One speed per PIECE:
// a corner inside a cell has two normals.  Exact for a rigid translation.
PG_HD double poly_piece_weight(const PolyBody&, int, double, double, double, double len) { return len; }
PG_HD double poly_piece_weight(const MovingPoly& b, int k, double lambda, double dx, double dy, double len) {
  const int k1 = k + 1 < b.M ? k + 1 : 0;
  double upx, upy, uqx, uqy;
  poly_velocity(b, k, upx, upy);
  poly_velocity(b, k1, uqx, uqy);
  const double ux = upx + lambda * (uqx - upx), uy = upy + lambda * (uqy - upy);
  const double vn = (ux * dy - uy * dx) / len;
  return len * sqrt(1.0 + vn * vn);
}

// the cells a box of positive extent overlaps, from the nodes
PG_HD void poly_box_cells(const PolyBody& b, const double* lo, const double* hi, int& i0, int& i1, int& j0, int& j1) {
  i0 = poly_locate(b, 0, lo[0]);
  i1 = poly_locate(b, 0, hi[0]);
  if (i1 > i0 && b.nodes[0][i1] >= hi[0]) --i1;
  j0 = poly_locate(b, 1, lo[1]);
  j1 = poly_locate(b, 1, hi[1]);
  if (j1 > j0 && b.nodes[1][j1] >= hi[1]) --j1;
}

// part (i, j) of the box: the cell's extent, the box's own ends at the first and last cell
PG_HD void poly_part(const PolyBody& b, const double* lo, const double* hi, int i, int i0, int i1, int j, int j0, int j1, double& s0,
                     double& s1, double& z0, double& z1) {
  s0 = i == i0 ? lo[0] : b.nodes[0][i];
  z0 = i == i1 ? hi[0] : b.nodes[0][i + 1];
  s1 = j == j0 ? lo[1] : b.nodes[1][j];
  z1 = j == j1 ? hi[1] : b.nodes[1][j + 1];
}

// type of a box, and (the return value) whether it owns a piece of the front
template <class P>
PG_HD int poly_pick(const P& b, const double* lo, const double* hi, int& type) {
  bool cut = false, own = false;
  if (hi[0] - lo[0] > 0.0 && hi[1] - lo[1] > 0.0) {
    int i0, i1, j0, j1;
    poly_box_cells(b, lo, hi, i0, i1, j0, j1);
    for (int j = j0; j <= j1; ++j)
      for (int i = i0; i <= i1; ++i) {
        double s0, s1, z0, z1;
        poly_part(b, lo, hi, i, i0, i1, j, j0, j1, s0, s1, z0, z1);
        if (!(z0 > s0 && z1 > s1)) continue;
        const int bin = poly_cell_bin(b, i, j);
        for (int e = b.ptr[bin]; e < b.ptr[bin + 1]; ++e) {
          double px, py, qx, qy, ax, ay, bx, by;
          poly_edge(b, b.idx[e], px, py, qx, qy);
          if (!poly_clip(px, py, qx, qy, s0, s1, z0, z1, ax, ay, bx, by)) continue;
          const double mx = 0.5 * (ax + bx), my = 0.5 * (ay + by);
          if (mx > lo[0] && mx < hi[0] && my > lo[1] && my < hi[1]) cut = true;
          if (mx >= s0 && mx < z0 && my >= s1 && my < z1) own = true;
        }
      }
  }
  type = cut ? PG_CUT : poly_fluid_at(b, 0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1])) ? PG_FULL : PG_EMPTY;
  return own ? 1 : 0;
}

PG_HD int pick_ball(const PolyBody& b, const double* lo, const double* hi, int& type) { return poly_pick(b, lo, hi, type); }
PG_HD int pick_ball(const MovingPoly& b, const double* lo, const double* hi, int& type) { return poly_pick(b, lo, hi, type); }

// qlane / qstride: as ball_box_moments -- this caller takes the edges qlane, qlane + qstride, ... of every cell's list and `group`
// adds the partial sums up; lane 0 adds the box's own right and top edges.  Mom::m[2], unused in 2-D, counts the pieces that
// make the box CUT, so that the group's sum carries the type.
template <class P, class Group>
PG_HD BoxMeasure poly_box(const P& b, const double* lo, const double* hi, bool want_surface, int qlane, int qstride, Group group) {
  BoxMeasure o;
  o.vol = 0.0; o.gamma = 0.0;
  for (int d = 0; d < 3; ++d) { o.cen[d] = 0.0; o.cg[d] = 0.0; }
  o.cen[0] = 0.5 * (lo[0] + hi[0]);
  o.cen[1] = 0.5 * (lo[1] + hi[1]);
  const bool degenerate = !(hi[0] - lo[0] > 0.0) || !(hi[1] - lo[1] > 0.0);
  Mom m;
  m.vol = m.gamma = 0.0;
  for (int d = 0; d < 3; ++d) m.m[d] = m.gm[d] = 0.0;
  const double sgn = b.flip ? -1.0 : 1.0;
  if (!degenerate) {
    int i0, i1, j0, j1;
    poly_box_cells(b, lo, hi, i0, i1, j0, j1);
    for (int j = j0; j <= j1; ++j)
      for (int i = i0; i <= i1; ++i) {
        double s0, s1, z0, z1;
        poly_part(b, lo, hi, i, i0, i1, j, j0, j1, s0, s1, z0, z1);
        if (!(z0 > s0 && z1 > s1)) continue;
        const int bin = poly_cell_bin(b, i, j);
        double sv = 0.0, sm0 = 0.0, sm1 = 0.0;                  // about the part's own lower corner
        for (int e = b.ptr[bin] + qlane; e < b.ptr[bin + 1]; e += qstride) {
          double px, py, qx, qy, ax, ay, bx, by, lambda;
          poly_edge(b, b.idx[e], px, py, qx, qy);
          if (!poly_clip(px, py, qx, qy, s0, s1, z0, z1, ax, ay, bx, by, lambda)) continue;
          const double mx = 0.5 * (ax + bx), my = 0.5 * (ay + by);
          if (mx > lo[0] && mx < hi[0] && my > lo[1] && my < hi[1]) m.m[2] += 1.0;
          const double ua = ax - s0, ub = bx - s0, va = ay - s1, vb = by - s1, dx = bx - ax, dy = by - ay;
          sv += 0.5 * (ua + ub) * dy;
          sm0 += (ua * ua + ua * ub + ub * ub) / 6.0 * dy;
          sm1 -= (va * va + va * vb + vb * vb) / 6.0 * dx;
          if (want_surface && mx >= s0 && mx < z0 && my >= s1 && my < z1) {
            const double len = poly_piece_weight(b, b.idx[e], lambda, dx, dy, sqrt(dx * dx + dy * dy));
            m.gamma += len;
            m.gm[0] += len * (mx - lo[0]);
            m.gm[1] += len * (my - lo[1]);
          }
        }
        sv *= sgn; sm0 *= sgn; sm1 *= sgn;
        if (qlane == 0) {
          const double w = z0 - s0, h = z1 - s1;
          const double lr = poly_section(b, 0, z0, s1, z1, h), lt = poly_section(b, 1, z1, s0, z0, w);
          sv += w * lr;
          sm0 += 0.5 * w * w * lr;
          sm1 += 0.5 * h * h * lt;
        }
        m.vol += sv;
        m.m[0] += sm0 + (s0 - lo[0]) * sv;
        m.m[1] += sm1 + (s1 - lo[1]) * sv;
      }
  }
  group(m);
  o.type = m.m[2] > 0.0 ? PG_CUT : poly_fluid_at(b, o.cen[0], o.cen[1]) ? PG_FULL : PG_EMPTY;
  if (degenerate) return o;
  const double full = prod_ext(lo, hi, 2, -1);
  if (o.type != PG_CUT) o.vol = o.type == PG_FULL ? full : 0.0;
  else {
    double vol = m.vol;
    if (!(vol > 0.0)) vol = 0.0;                  // (also a NaN)
    if (vol > full) vol = full;
    o.vol = vol;
    if (vol > 0.0)
      for (int d = 0; d < 2; ++d) {
        const double c = lo[d] + m.m[d] / vol;
        if (c >= lo[d] && c <= hi[d]) o.cen[d] = c;
        else if (c < lo[d]) o.cen[d] = lo[d];
        else if (c > hi[d]) o.cen[d] = hi[d];
      }
  }
  if (m.gamma > 0.0 && m.gamma < 1e300) {         // (a box that only touches the front may own a piece of it)
    o.gamma = m.gamma;
    for (int d = 0; d < 2; ++d) {
      const double c = lo[d] + m.gm[d] / m.gamma;
      o.cg[d] = c >= lo[d] ? (c <= hi[d] ? c : hi[d]) : lo[d];
    }
  }
  return o;
}

template <class Group = NoGroup>
PG_HD BoxMeasure box_measure(const PolyBody& b, const double* lo, const double* hi, bool want_surface, const GLTable&, int qlane = 0,
                             int qstride = 1, Group group = Group()) {
  return poly_box(b, lo, hi, want_surface, qlane, qstride, group);
}
template <class Group = NoGroup>
PG_HD BoxMeasure box_measure(const MovingPoly& b, const double* lo, const double* hi, bool want_surface, const GLTable&,
                             int qlane = 0, int qstride = 1, Group group = Group()) {
  return poly_box(b, lo, hi, want_surface, qlane, qstride, group);
}

// fluid measure of {x_d = s} and the box.  With no crossing strictly inside: the caller's full measure, or 0
template <class P>
PG_HD double poly_section_measure(const P& b, int d, double s, const double* lo, const double* hi, double full_measure) {
  const double a = d == 0 ? lo[1] : lo[0], z = d == 0 ? hi[1] : hi[0];
  if (!(z - a > 0.0)) return 0.0;
  return poly_section(b, d, s, a, z, full_measure >= 0.0 ? full_measure : z - a);
}
PG_HD double section_measure(const PolyBody& b, int d, double s, const double* lo, const double* hi, double full_measure = -1.0) {
  return poly_section_measure(b, d, s, lo, hi, full_measure);
}
PG_HD double section_measure(const MovingPoly& b, int d, double s, const double* lo, const double* hi, double full_measure = -1.0) {
  return poly_section_measure(b, d, s, lo, hi, full_measure);
}

// ---- host only -----------------------------------------------------------------------------------------------------------------

// twice the signed area, about the first marker
inline double polygon_area2(const double* xy, int64_t M) {
  double a = 0.0;
  for (int64_t k = 1; k + 1 < M; ++k)
    a += (xy[2 * k] - xy[0]) * (xy[2 * k + 3] - xy[1]) - (xy[2 * k + 2] - xy[0]) * (xy[2 * k + 1] - xy[1]);
  return a;
}

// markers without a closing duplicate of the first
inline int64_t polygon_open_count(const double* xy, int64_t M) {
  return (M >= 2 && xy && xy[0] == xy[2 * M - 2] && xy[1] == xy[2 * M - 1]) ? M - 1 : M;
}

// Host only: what pg_capacity_create_polygon refuses before it allocates anything, each with its own message.  M: without the
// closing duplicate.
inline bool polygon_body_check(const double* xy, int64_t M, std::string* why) {
  auto fail = [&](const std::string& m) {
    if (why) *why = m;
    return false;
  };
  if (!xy) return fail("NULL marker array");
  if (M < 3) return fail("a polygon needs at least 3 markers (got " + std::to_string((long long)(M < 0 ? 0 : M)) + ")");
  if (M > 100000000) return fail("more than 1e8 markers");
  for (int64_t k = 0; k < 2 * M; ++k)
    if (!std::isfinite(xy[k])) return fail("marker " + std::to_string((long long)(k / 2)) + " has a non-finite coordinate");
  for (int64_t k = 0; k < M; ++k) {
    const int64_t k1 = (k + 1) % M;
    if (xy[2 * k] == xy[2 * k1] && xy[2 * k + 1] == xy[2 * k1 + 1])
      return fail("zero-length edge: markers " + std::to_string((long long)k) + " and " + std::to_string((long long)k1) + " coincide");
  }
  if (polygon_area2(xy, M) == 0.0) return fail("the polygon has zero signed area");
  auto orient = [&](int64_t a, int64_t b, int64_t c) {
    const double v = (xy[2 * b] - xy[2 * a]) * (xy[2 * c + 1] - xy[2 * a + 1]) - (xy[2 * b + 1] - xy[2 * a + 1]) * (xy[2 * c] - xy[2 * a]);
    return v > 0.0 ? 1 : v < 0.0 ? -1 : 0;
  };
  auto within = [&](int64_t a, int64_t b, int64_t c) {        // c collinear with a b: inside its bounding box
    return dmin(xy[2 * a], xy[2 * b]) <= xy[2 * c] && xy[2 * c] <= dmax(xy[2 * a], xy[2 * b]) &&
           dmin(xy[2 * a + 1], xy[2 * b + 1]) <= xy[2 * c + 1] && xy[2 * c + 1] <= dmax(xy[2 * a + 1], xy[2 * b + 1]);
  };
  auto self = [&](int64_t i, int64_t j) {
    return fail("the polygon intersects itself: edges " + std::to_string((long long)i) + " and " + std::to_string((long long)j));
  };
  for (int64_t i = 0; i < M; ++i) {
    const int64_t i1 = (i + 1) % M, i2 = (i + 2) % M;
    // the next edge folds back onto this one
    if (orient(i, i1, i2) == 0 &&
        (xy[2 * i1] - xy[2 * i]) * (xy[2 * i2] - xy[2 * i1]) + (xy[2 * i1 + 1] - xy[2 * i + 1]) * (xy[2 * i2 + 1] - xy[2 * i1 + 1]) < 0.0)
      return self(i, i1);
    const double ax0 = dmin(xy[2 * i], xy[2 * i1]), ax1 = dmax(xy[2 * i], xy[2 * i1]);
    const double ay0 = dmin(xy[2 * i + 1], xy[2 * i1 + 1]), ay1 = dmax(xy[2 * i + 1], xy[2 * i1 + 1]);
    for (int64_t j = i + 2; j < M; ++j) {
      const int64_t j1 = (j + 1) % M;
      if (j1 == i) continue;                                  // neighbours share a marker
      if (dmax(xy[2 * j], xy[2 * j1]) < ax0 || dmin(xy[2 * j], xy[2 * j1]) > ax1 || dmax(xy[2 * j + 1], xy[2 * j1 + 1]) < ay0 ||
          dmin(xy[2 * j + 1], xy[2 * j1 + 1]) > ay1)
        continue;
      const int o1 = orient(i, i1, j), o2 = orient(i, i1, j1), o3 = orient(j, j1, i), o4 = orient(j, j1, i1);
      if ((o1 != o2 && o3 != o4) || (o1 == 0 && within(i, i1, j)) || (o2 == 0 && within(i, i1, j1)) || (o3 == 0 && within(j, j1, i)) ||
          (o4 == 0 && within(j, j1, i1)))
        return self(i, j);
    }
  }
  return true;
}

// the markers the kernels see: no closing duplicate, counter-clockwise (reversed about the first marker if the signed area is
// negative)
inline std::vector<double> polygon_normalise(const double* xy, int64_t M) {
  std::vector<double> out(xy, xy + 2 * M);
  if (polygon_area2(xy, M) < 0.0)
    for (int64_t k = 1; k < M; ++k) {
      out[2 * k] = xy[2 * (M - k)];
      out[2 * k + 1] = xy[2 * (M - k) + 1];
    }
  return out;
}

// the markers the kernels see of a moving polygon: the reversal is decided by the signed area at t0 and applied to both arrays
inline std::vector<double> polygon_normalise_as(const double* xy, const double* like, int64_t M) {
  std::vector<double> out(xy, xy + 2 * M);
  if (polygon_area2(like, M) < 0.0)
    for (int64_t k = 1; k < M; ++k) {
      out[2 * k] = xy[2 * (M - k)];
      out[2 * k + 1] = xy[2 * (M - k) + 1];
    }
  return out;
}

// markers of a moving polygon without the closing duplicate: it is dropped where BOTH arrays close (one that closes alone keeps
// it, and is refused for its zero-length edge)
inline int64_t moving_polygon_open_count(const double* xy0, const double* xy1, int64_t M) {
  return (xy0 && xy1 && polygon_open_count(xy0, M) == M - 1 && polygon_open_count(xy1, M) == M - 1) ? M - 1 : M;
}

// Host only: what pg_capacity_create_spacetime_polygon refuses before it allocates anything, each with its own message (the
// mesh, the output pointer and the ranks are the caller's to check).  M: without the closing duplicate.  The polygon must be
// simple (polygon_body_check's rules) at t0, at t1 and at mid time -- NOT at every time in between -- and keep its orientation.
inline bool spacetime_polygon_check(int N, const double* xy0, const double* xy1, int64_t M, double t0, double t1, int nq,
                                    const double* tau_w /* nq x 2 */, std::string* why) {
  auto fail = [&](const std::string& m) {
    if (why) *why = m;
    return false;
  };
  if (!xy0) return fail("xy0 == NULL: the markers at t0 are needed");
  if (!xy1) return fail("xy1 == NULL: the markers at t1 are needed");
  if (!tau_w) return fail("tau_w == NULL: the time nodes and weights are needed");
  if (N != 2) return fail("a moving marker polygon is a 2-D body, the mesh is " + std::to_string(N) + "-D");
  if (M < 3) return fail("a polygon needs at least 3 markers (got " + std::to_string((long long)(M < 0 ? 0 : M)) + ")");
  if (M > 100000000) return fail("more than 1e8 markers");
  for (int e = 0; e < 2; ++e)
    for (int64_t k = 0; k < 2 * M; ++k)
      if (!std::isfinite((e ? xy1 : xy0)[k]))
        return fail("marker " + std::to_string((long long)(k / 2)) + " has a non-finite coordinate at " + (e ? "t1" : "t0"));
  if (nq < 1 || nq > 4096) return fail("1 .. 4096 time nodes");
  if (!(t1 > t0)) return fail("empty time slab");
  double wsum = 0.0;
  for (int k = 0; k < nq; ++k) {
    if (!(tau_w[2 * k] > t0 && tau_w[2 * k] < t1)) return fail("time nodes must lie inside (t0, t1)");
    wsum += tau_w[2 * k + 1];
  }
  if (!(fabs(wsum - (t1 - t0)) <= 1e-12 * (t1 - t0))) return fail("time weights must add up to t1 - t0");
  std::vector<double> mid((size_t)(2 * M));
  for (int64_t k = 0; k < 2 * M; ++k) mid[(size_t)k] = xy0[k] + 0.5 * (xy1[k] - xy0[k]);
  for (int e = 0; e < 3; ++e) {
    std::string w;
    if (!polygon_body_check(e == 0 ? xy0 : e == 1 ? xy1 : mid.data(), M, &w))
      return fail(std::string(e == 0 ? "at t0: " : e == 1 ? "at t1: " : "at mid time: ") + w);
  }
  if ((polygon_area2(xy0, M) > 0.0) != (polygon_area2(xy1, M) > 0.0) || (polygon_area2(xy0, M) > 0.0) != (polygon_area2(mid.data(), M) > 0.0))
    return fail("the orientation of the polygon differs between t0 and t1 (the front turns inside out during the slab)");
  return true;
}

// the edge lookup, built on the host (the CPU tests; the product builds it on the device with the same poly_edge_bins)
struct PolyBinsHost {
  std::vector<int> ptr, idx;
};
template <class P>
inline PolyBinsHost polygon_bins_host(P b) {
  const int nb = b.n[0] + b.n[1] + b.n[0] * b.n[1];
  PolyBinsHost t;
  t.ptr.assign((size_t)nb + 1, 0);
  for (int k = 0; k < b.M; ++k) poly_edge_bins(b, k, [&](int bin) { ++t.ptr[(size_t)bin + 1]; });
  for (int q = 0; q < nb; ++q) t.ptr[(size_t)q + 1] += t.ptr[q];
  t.idx.assign((size_t)t.ptr[nb], 0);
  std::vector<int> cur(t.ptr.begin(), t.ptr.end() - 1);
  for (int k = 0; k < b.M; ++k) poly_edge_bins(b, k, [&](int bin) { t.idx[(size_t)cur[bin]++] = k; });
  return t;
}

}  // namespace pggeom
