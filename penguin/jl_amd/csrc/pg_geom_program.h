// pg_geom_program.h -- cut-cell geometry of a TRACED level set: the three primitives the capacity kernels reach a body through
// (pick_ball, box_measure, section_measure of pg_geom.h) for a body given as a pg_program phi(x_1 .. x_N) and the N programs of
// its partial derivatives.  Fluid is where phi <= 0.  1-D and 2-D.  Usable from HIP kernels and from a host (g++) build, like
// pg_geom.h; compile with -ffp-contract=off.  The operand stack of the evaluator is a template parameter as in prog_eval: a
// plain array on the host, a column of LDS in the kernels.  A body carries a time t (VAR 3 of its programs): a static body
// passes 0, a moving one phi(x, t) is the static body "phi at t" for every primitive here, and a fourth program gives d phi / dt.
//
// Conventions (the test-side arbiters restate them):
//   samples     a segment [a, b] is looked at in NS + 1 = 9 points a + (b - a) (k / 8), k = 0 .. 7, and b itself
//   roots       a sample that is exactly 0 is a root; two consecutive samples of opposite sign bracket ONE root, refined by
//               regula falsi (Illinois) safeguarded by bisection, at most 64 iterations, until the bracket is <= 2 ulp or f = 0
//   segment     the fluid measure is the sum of the pieces between consecutive roots / ends whose midpoint has phi <= 0
//   box type    1-D: the 9 samples of the interval; 2-D: the 9 samples of each of the 4 edges and the centre (33 points).
//               FULL if all are <= 0, else EMPTY if all are >= 0, else CUT: a feature narrower than h / 8 is not seen.  A box
//               that only TOUCHES the interface (phi = 0 at some samples, > 0 at the others) is EMPTY, as the closed-form
//               kinds have it (ball: near >= r^2, plane: near >= offset): a plane on a node line gives the same types
//   box, 2-D    heights along the axis v with the larger |d phi / d x_v| at the centre (tie: the last axis), integrated along
//               the other axis u with 16 Gauss-Legendre nodes per piece between the box ends and the roots of phi on the two
//               edges v = lo_v, v = hi_v.  Every moment is taken about the box's lower corner
//   a NaN of phi counts as solid (phi = 1)
// No loop has a data-dependent bound above the iteration cap, and nothing is indexed in private memory (no scratch in a kernel):
// roots and breakpoints are consumed in ascending order as they are found, never stored.
#pragma once
#include "pg_geom.h"
#include "pg_program.h"

namespace pggeom {

constexpr int LS_NS = 8;        // sample intervals per segment
constexpr int LS_ITMAX = 64;    // root refinement cap

// Eval: value(which, x, y, t) runs program `which` (0: phi, 1 + d: d phi / d x_d, 3: d phi / dt) at a point.  `which` is a literal at every
// call: in a kernel the evaluator is ONE function that is called, not inlined (dozens of inlined interpreters, each with its
// own exp, pow, erf ..., do not fit the register file), and it fetches the instructions with scalar loads, which needs the
// program to be the same for all lanes of the wave.
template <class Eval>
struct ProgBody {
  int N;
  int complement;               // always 0: the sign lives in sgn, the kernels' own complement flip must not apply
  double sgn;                   // -1: PG_FLAG_COMPLEMENT (-phi, -grad phi)
  Eval ev;
  double t = 0.0;               // the time every evaluation runs at (a static body: 0, its programs read no t)
  PG_HD double f(double x, double y) const {
    const double v = sgn * ev.value(0, x, y, t);
    return v == v ? v : 1.0;
  }
  PG_HD void grad(double x, double y, double& g0, double& g1) const {
    g0 = sgn * ev.value(1, x, y, t);
    g1 = N > 1 ? sgn * ev.value(2, x, y, t) : 0.0;
  }
  PG_HD double dfdt(double x, double y) const { return sgn * ev.value(3, x, y, t); }   // moving bodies only
  // the normal speed of the interface at a point, - d_t phi / |grad phi|; a zero or non-finite |grad phi| gives 0
  PG_HD double normal_speed(double x, double y) const {
    double g0, g1;
    grad(x, y, g0, g1);
    const double gn = sqrt(g0 * g0 + g1 * g1);
    if (!(gn > 0.0 && gn < 1e300)) return 0.0;
    return -dfdt(x, y) / gn;
  }
};

// the host's evaluator: the programs through pointers, prog_eval on a plain array
struct HostEval {
  const pg_program* phi;
  const pg_program* grad;       // N programs
  pgprog::HostStack* S;
  const pg_program* dt = nullptr;   // d phi / dt of a moving body
  double value(int which, double x, double y, double t) const {
    return pgprog::prog_eval(which == 0 ? *phi : which == 3 ? *dt : grad[which - 1], x, y, 0.0, t, *S);
  }
};

// phi along the axis `axis` with the other coordinate fixed (1-D: other = 0)
template <class Body>
struct LineFn {
  const Body& b;
  int axis;
  double other;
  PG_HD double operator()(double s) const { return axis == 0 ? b.f(s, other) : b.f(other, s); }
};

PG_HD double ls_sample(double a, double b, int k) { return k == LS_NS ? b : a + (b - a) * ((double)k * (1.0 / LS_NS)); }

// the root inside (a, b), f(a) = fa and f(b) = fb of opposite sign, neither zero
template <class F>
PG_HD double refine_root(const F& f, double a, double fa, double b, double fb) {
  int side = 0;
  for (int it = 0; it < LS_ITMAX; ++it) {
    const double big = dmax(fabs(a), fabs(b));
    if (b - a <= 4.44089209850062616e-16 * big) break;          // 2 ulp
    const double mid = 0.5 * (a + b), tol = 2.22044604925031308e-16 * big;
    double x = b - fb * ((b - a) / (fb - fa));
    // a step that lands within an ulp of an end is taken an ulp inside it: the bracket then closes from BOTH sides
    if (x < a + tol) x = a + tol;
    if (x > b - tol) x = b - tol;
    if (!(x > a && x < b)) x = mid;
    if (!(x > a && x < b)) break;                               // no double strictly inside
    const double fx = f(x);
    if (fx == 0.0) return x;
    if ((fx < 0.0) == (fb < 0.0)) {
      b = x; fb = fx;
      if (side == 1) fa *= 0.5;
      side = 1;
    } else {
      a = x; fa = fx;
      if (side == -1) fb *= 0.5;
      side = -1;
    }
  }
  return 0.5 * (a + b);
}

struct SegOut {
  double len, mom;      // fluid length of [a, b] and its first moment about a
  double nroots, rsum;  // roots in the closed segment: their number and the sum of (root - a)
  double gw, gwr;       // roots strictly inside: sum of |grad phi| / |d phi / d axis|, and of that weight times (root - a)
  bool all_in, all_out; // every sample <= 0 / every sample > 0
};

// One pass over [a, b] along `axis` at the fixed coordinate `other`: roots in ascending order, pieces closed as they end.
template <class Body>
PG_HD void seg_measure(const Body& bs, int axis, double other, double a, double b, bool want_surface, SegOut& o) {
  const LineFn<Body> f{bs, axis, other};
  o.len = o.mom = o.nroots = o.rsum = o.gw = o.gwr = 0.0;
  double p = a;                                   // where the open piece began
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
      double g0, g1;
      bs.grad(axis == 0 ? q : other, axis == 0 ? other : q, g0, g1);
      const double gv = fabs(axis == 0 ? g0 : g1);
      const double w = sqrt(g0 * g0 + g1 * g1) / gv;
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

// FULL / EMPTY / CUT of a box on the sample lattice (FULL is tested first: a box where phi = 0 at every sample is FULL)
template <class Eval>
PG_HD int prog_box_type(const ProgBody<Eval>& bs, const double* lo, const double* hi) {
  bool in = true, out = true;
  if (bs.N == 1) {
    for (int k = 0; k <= LS_NS && (in || out); ++k) {
      const double v = bs.f(ls_sample(lo[0], hi[0], k), 0.0);
      in = in && v <= 0.0;
      out = out && v >= 0.0;
    }
  } else {
    for (int k = 0; k <= LS_NS && (in || out); ++k) {
      const double x = ls_sample(lo[0], hi[0], k);
      const double v0 = bs.f(x, lo[1]), v1 = bs.f(x, hi[1]);
      in = in && v0 <= 0.0 && v1 <= 0.0;
      out = out && v0 >= 0.0 && v1 >= 0.0;
    }
    for (int k = 1; k < LS_NS && (in || out); ++k) {
      const double y = ls_sample(lo[1], hi[1], k);
      const double v0 = bs.f(lo[0], y), v1 = bs.f(hi[0], y);
      in = in && v0 <= 0.0 && v1 <= 0.0;
      out = out && v0 >= 0.0 && v1 >= 0.0;
    }
    if (in || out) {
      const double v = bs.f(0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]));
      in = in && v <= 0.0;
      out = out && v >= 0.0;
    }
  }
  return in ? PG_FULL : out ? PG_EMPTY : PG_CUT;
}

template <class Eval>
PG_HD int pick_ball(const ProgBody<Eval>& bs, const double* lo, const double* hi, int& type) {
  type = prog_box_type(bs, lo, hi);
  return 0;
}

// The cheap test of a space-time cell (box) x [t0, t1] of a MOVING body: +1 the box is fluid during the whole slab, -1 solid,
// 0 not decided here.  Decided only if, at t0, mid time and t1, the sample lattice of prog_box_type (9 points in 1-D, 33 in 2-D)
// has ONE strict sign, and the smallest |phi| over those samples exceeds (t1 - t0) max |d phi / dt| over the same samples:
// twice the first-order change of phi over half a slab, the farthest any time is from one of the three.  A NaN of d phi / dt
// decides nothing.  What is not decided goes to the all-nodes rule, so the margin costs time and never a type.
template <class Eval>
PG_HD int prog_st_far(ProgBody<Eval> bs, const double* lo, const double* hi, double t0, double t1) {
  bool in = true, out = true, ok = true;
  double amin = 1e300, rate = 0.0;
  auto look = [&](double x, double y) {
    const double v = bs.f(x, y), r = fabs(bs.dfdt(x, y));
    in = in && v < 0.0;
    out = out && v > 0.0;
    amin = dmin(amin, fabs(v));
    ok = ok && r == r;
    rate = dmax(rate, r);
  };
  for (int e = 0; e < 3 && (in || out) && ok; ++e) {
    bs.t = e == 0 ? t0 : e == 1 ? 0.5 * (t0 + t1) : t1;
    if (bs.N == 1) {
      for (int k = 0; k <= LS_NS && (in || out); ++k) look(ls_sample(lo[0], hi[0], k), 0.0);
    } else {
      for (int k = 0; k <= LS_NS && (in || out); ++k) {
        const double x = ls_sample(lo[0], hi[0], k);
        look(x, lo[1]);
        look(x, hi[1]);
      }
      for (int k = 1; k < LS_NS && (in || out); ++k) {
        const double y = ls_sample(lo[1], hi[1], k);
        look(lo[0], y);
        look(hi[0], y);
      }
      if (in || out) look(0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]));
    }
  }
  if (!(in || out) || !ok) return 0;
  if (!(amin > (t1 - t0) * rate)) return 0;
  return in ? 1 : -1;
}

// qlane / qstride: as ball_box_moments -- this caller takes the Gauss-Legendre nodes qlane, qlane + qstride, ... of every piece
// and `group` adds the partial moments up; the 1-D case has no quadrature (lane 0 returns all of it)
template <class Eval, class Group = NoGroup>
PG_HD BoxMeasure box_measure(const ProgBody<Eval>& bs, const double* lo, const double* hi, bool want_surface,
                             const GLTable& gl, int qlane = 0, int qstride = 1, Group group = Group()) {
  const int N = bs.N;
  BoxMeasure o;
  o.vol = 0.0; o.gamma = 0.0;
  bool degenerate = false;
  for (int d = 0; d < 3; ++d) { o.cen[d] = 0.0; o.cg[d] = 0.0; }
  for (int d = 0; d < N; ++d) {
    o.cen[d] = 0.5 * (lo[d] + hi[d]);
    if (!(hi[d] - lo[d] > 0.0)) degenerate = true;
  }
  o.type = prog_box_type(bs, lo, hi);
  const double full = prod_ext(lo, hi, N, -1);
  if (degenerate || o.type != PG_CUT) {
    o.vol = (!degenerate && o.type == PG_FULL) ? full : 0.0;
    return o;
  }
  Mom m;
  m.vol = m.gamma = 0.0;
  for (int d = 0; d < 3; ++d) m.m[d] = m.gm[d] = 0.0;
  if (N == 1) {
    if (qlane == 0) {
      SegOut s;
      seg_measure(bs, 0, 0.0, lo[0], hi[0], false, s);
      m.vol = s.len; m.m[0] = s.mom;
      m.gamma = s.nroots; m.gm[0] = s.rsum;
    }
  } else {
    double gx, gy;
    bs.grad(o.cen[0], o.cen[1], gx, gy);
    gx = fabs(gx); gy = fabs(gy);
    const int v = gx > gy ? 0 : 1, u = 1 - v;
    const double ua = lo[u], ub = hi[u], va = lo[v], vb = hi[v];
    const LineFn<ProgBody<Eval>> e0{bs, u, va}, e1{bs, u, vb};       // phi along the two edges v = lo_v, v = hi_v
    double p = ua;
    auto piece = [&](double q) {
      if (!(q > p)) return;
      const double um = 0.5 * (p + q), uh = 0.5 * (q - p);
      for (int k = qlane; k < NGL; k += qstride) {
        const double uu = um + uh * gl.x[k], w = gl.w[k] * uh;
        SegOut s;
        seg_measure(bs, v, uu, va, vb, want_surface, s);
        m.vol += w * s.len;
        m.m[v] += w * s.mom;
        m.m[u] += w * (s.len * (uu - ua));
        if (want_surface) {
          m.gamma += w * s.gw;
          m.gm[v] += w * s.gwr;
          m.gm[u] += w * (s.gw * (uu - ua));
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
  group(m);
  double vol = m.vol;
  if (!(vol > 0.0)) vol = 0.0;                    // (also a NaN)
  if (vol > full) vol = full;
  o.vol = vol;
  if (vol > 0.0)
    for (int d = 0; d < N; ++d) {
      const double c = lo[d] + m.m[d] / vol;
      if (c >= lo[d] && c <= hi[d]) o.cen[d] = c;
      else if (c < lo[d]) o.cen[d] = lo[d];
      else if (c > hi[d]) o.cen[d] = hi[d];
    }
  if (m.gamma > 0.0 && m.gamma < 1e300) {
    o.gamma = m.gamma;
    for (int d = 0; d < N; ++d) {
      const double c = lo[d] + m.gm[d] / m.gamma;
      o.cg[d] = c >= lo[d] ? (c <= hi[d] ? c : hi[d]) : lo[d];
    }
  }
  return o;
}

// fluid measure of {x_d = s} ∩ box.  A section whose 9 samples are all fluid (solid) returns the caller's full measure (0), as
// the closed-form kinds return it for a section their classification finds FULL (EMPTY)
template <class Eval>
PG_HD double section_measure(const ProgBody<Eval>& bs, int d, double s, const double* lo, const double* hi,
                             double full_measure = -1.0) {
  if (bs.N == 1) return bs.f(s, 0.0) <= 0.0 ? 1.0 : 0.0;
  const int o = 1 - d;
  const double ext = hi[o] - lo[o];
  const double full = full_measure >= 0.0 ? full_measure : ext;
  if (!(ext > 0.0)) return 0.0;
  SegOut so;
  seg_measure(bs, o, s, lo[o], hi[o], false, so);
  if (so.all_in) return full;
  if (so.all_out) return 0.0;
  return so.len < ext ? so.len : ext;
}

// Host only: what pg_capacity_create_program refuses before it allocates anything.  true: phi and the N gradient programs are
// valid, read no t and no coordinate >= N, N is 1 or 2, and the gradient agrees with central differences of phi (step 1e-6 h_d)
// at the centres of up to 64 real cells spread over the mesh, within 1e-4 max(|grad phi|, 1) -- a wrong derivative from a C
// caller, not rounding, is what this catches.  A point where either side is not finite decides nothing.
inline bool program_body_check(int N, const int64_t* n, const double* const* nodes /* n_d + 1 each */, const pg_program* phi,
                               const pg_program* grad, std::string* why) {
  auto fail = [&](const std::string& m) {
    if (why) *why = m;
    return false;
  };
  if (!phi) return fail("NULL level-set program");
  if (!grad) return fail("grad == NULL: the N programs of d phi / d x_d are needed (DeviceFunction.gradient_programs builds them)");
  if (N == 3) return fail("3-D program bodies are not supported yet (1-D and 2-D)");
  if (N != 1 && N != 2) return fail("the mesh must be 1-D or 2-D");
  for (int k = 0; k <= N; ++k) {
    const pg_program* p = k == 0 ? phi : grad + (k - 1);
    const std::string name = k == 0 ? std::string("the level-set program") : "gradient program " + std::to_string(k - 1);
    std::string w;
    if (!pgprog::program_validate(p, &w)) return fail(name + " is invalid: " + w);
    for (int q = 0; q < p->n_ops; ++q) {
      if (p->op[q] != PG_OP_VAR) continue;
      if (p->arg[q] == 3) return fail(name + " reads t (instruction " + std::to_string(q) + "): a body does not depend on time");
      if (p->arg[q] >= N)
        return fail(name + " reads coordinate " + std::to_string((int)p->arg[q]) + " (instruction " + std::to_string(q) + ") on a " +
                    std::to_string(N) + "-D mesh");
    }
  }
  int64_t M = 1;
  for (int d = 0; d < N; ++d) M *= n[d];
  const int64_t npts = M < 64 ? M : 64;
  pgprog::HostStack S;
  for (int64_t k = 0; k < npts; ++k) {
    int64_t cell = npts > 1 ? (k * (M - 1)) / (npts - 1) : 0;
    double x[2] = {0.0, 0.0};
    double h[2] = {1.0, 1.0};
    for (int d = 0; d < N; ++d) {
      const int64_t j = cell % n[d];
      x[d] = 0.5 * (nodes[d][j] + nodes[d][j + 1]);
      h[d] = (nodes[d][n[d]] - nodes[d][0]) / (double)n[d];
      cell /= n[d];
    }
    double g[2] = {0.0, 0.0}, fd[2] = {0.0, 0.0}, gn = 0.0;
    for (int d = 0; d < N; ++d) {
      const double e = 1e-6 * h[d];
      double xp[2] = {x[0], x[1]}, xm[2] = {x[0], x[1]};
      xp[d] += e; xm[d] -= e;
      fd[d] = (pgprog::prog_eval(*phi, xp[0], xp[1], 0.0, 0.0, S) - pgprog::prog_eval(*phi, xm[0], xm[1], 0.0, 0.0, S)) / (xp[d] - xm[d]);
      g[d] = pgprog::prog_eval(grad[d], x[0], x[1], 0.0, 0.0, S);
      gn += g[d] * g[d];
    }
    const double tol = 1e-4 * dmax(sqrt(gn), 1.0);
    for (int d = 0; d < N; ++d)
      if (fabs(g[d] - fd[d]) > tol)                 // (false for a NaN)
        return fail("gradient program " + std::to_string(d) + " gives " + std::to_string(g[d]) + " at (" + std::to_string(x[0]) +
                    (N > 1 ? ", " + std::to_string(x[1]) : std::string()) + ") where central differences of the level set give " +
                    std::to_string(fd[d]));
  }
  return true;
}

// Host only: what pg_capacity_create_spacetime_program refuses before it allocates anything (the mesh, the output pointer and
// the ranks are the caller's to check).  The derivative rule is program_body_check's, with its tolerances, taken at t0, mid time
// and t1, and d phi / dt against central differences of phi in time with the step 1e-6 (t1 - t0).
inline bool spacetime_program_check(int N, const int64_t* n, const double* const* nodes /* n_d + 1 each */, const pg_program* phi,
                                    const pg_program* grad, const pg_program* dphidt, double t0, double t1, int nq,
                                    const double* tau_w /* nq x 2 */, std::string* why) {
  auto fail = [&](const std::string& m) {
    if (why) *why = m;
    return false;
  };
  if (N != 1 && N != 2) return fail("space-time capacities: 1-D+t and 2-D+t (the reference's 3-D+t blocks drop the z direction)");
  if (!phi) return fail("NULL level-set program");
  if (!grad) return fail("grad == NULL: the N programs of d phi / d x_d are needed (DeviceFunction.moving_gradient_programs builds them)");
  if (!dphidt) return fail("dphidt == NULL: the program of d phi / dt is needed (DeviceFunction.moving_gradient_programs builds it)");
  if (!tau_w) return fail("tau_w == NULL: the time nodes and weights are needed");
  for (int k = 0; k <= N + 1; ++k) {
    const pg_program* p = k == 0 ? phi : k <= N ? grad + (k - 1) : dphidt;
    const std::string name = k == 0 ? std::string("the level-set program")
                             : k <= N ? "gradient program " + std::to_string(k - 1) : std::string("the time-derivative program");
    std::string w;
    if (!pgprog::program_validate(p, &w)) return fail(name + " is invalid: " + w);
    for (int q = 0; q < p->n_ops; ++q)
      if (p->op[q] == PG_OP_VAR && p->arg[q] != 3 && p->arg[q] >= N)
        return fail(name + " reads coordinate " + std::to_string((int)p->arg[q]) + " (instruction " + std::to_string(q) + ") on a " +
                    std::to_string(N) + "-D mesh");
  }
  if (nq < 1 || nq > 4096) return fail("1 .. 4096 time nodes");
  if (!(t1 > t0)) return fail("empty time slab");
  double wsum = 0.0;
  for (int k = 0; k < nq; ++k) {
    if (!(tau_w[2 * k] > t0 && tau_w[2 * k] < t1)) return fail("time nodes must lie inside (t0, t1)");
    wsum += tau_w[2 * k + 1];
  }
  if (!(fabs(wsum - (t1 - t0)) <= 1e-12 * (t1 - t0))) return fail("time weights must add up to t1 - t0");
  int64_t M = 1;
  for (int d = 0; d < N; ++d) M *= n[d];
  const int64_t npts = M < 64 ? M : 64;
  pgprog::HostStack S;
  const double et = 1e-6 * (t1 - t0);
  for (int e = 0; e < 3; ++e) {
    const double t = e == 0 ? t0 : e == 1 ? 0.5 * (t0 + t1) : t1;
    for (int64_t k = 0; k < npts; ++k) {
      int64_t cell = npts > 1 ? (k * (M - 1)) / (npts - 1) : 0;
      double x[2] = {0.0, 0.0};
      double h[2] = {1.0, 1.0};
      for (int d = 0; d < N; ++d) {
        const int64_t j = cell % n[d];
        x[d] = 0.5 * (nodes[d][j] + nodes[d][j + 1]);
        h[d] = (nodes[d][n[d]] - nodes[d][0]) / (double)n[d];
        cell /= n[d];
      }
      double g[3] = {0.0, 0.0, 0.0}, fd[3] = {0.0, 0.0, 0.0}, gn = 0.0;
      for (int d = 0; d < N; ++d) {
        const double e1 = 1e-6 * h[d];
        double xp[2] = {x[0], x[1]}, xm[2] = {x[0], x[1]};
        xp[d] += e1; xm[d] -= e1;
        fd[d] = (pgprog::prog_eval(*phi, xp[0], xp[1], 0.0, t, S) - pgprog::prog_eval(*phi, xm[0], xm[1], 0.0, t, S)) / (xp[d] - xm[d]);
        g[d] = pgprog::prog_eval(grad[d], x[0], x[1], 0.0, t, S);
        gn += g[d] * g[d];
      }
      const double tp = t + et, tm = t - et;
      fd[2] = (pgprog::prog_eval(*phi, x[0], x[1], 0.0, tp, S) - pgprog::prog_eval(*phi, x[0], x[1], 0.0, tm, S)) / (tp - tm);
      g[2] = pgprog::prog_eval(*dphidt, x[0], x[1], 0.0, t, S);
      const double tol = 1e-4 * dmax(sqrt(gn), 1.0);
      const std::string at = " at (" + std::to_string(x[0]) + (N > 1 ? ", " + std::to_string(x[1]) : std::string()) + "), t = " +
                             std::to_string(t) + " where central differences of the level set give ";
      for (int d = 0; d < N; ++d)
        if (fabs(g[d] - fd[d]) > tol)                 // (false for a NaN)
          return fail("gradient program " + std::to_string(d) + " gives " + std::to_string(g[d]) + at + std::to_string(fd[d]));
      if (fabs(g[2] - fd[2]) > tol)
        return fail("the time-derivative program gives " + std::to_string(g[2]) + at + std::to_string(fd[2]));
    }
  }
  return true;
}

}  // namespace pggeom
