// Host (g++) build of the program-body geometry (penguin/jl_amd/csrc/pg_geom_program.h) for a MOVING body phi(x, t), for the CPU
// unit tests and as the arbiter of the GPU tests (tests/spacetime_program_reference.py restates the slab rule on top of it in
// numpy).  The product never loads this library.  Compile with -ffp-contract=off.  With -DSPACETIME_MAIN: a stand-alone program
// for the sanitizers that integrates degenerate bodies over a slab cell by cell.
#include "../penguin/jl_amd/csrc/pg_geom_program.h"

#include <cstdio>
#include <cstring>

using namespace pggeom;
using pgprog::HostStack;

static GLTable g_gl;
static bool g_init = false;
static void init() { if (!g_init) { gl_init(g_gl); g_init = true; } }

// derivs: N spatial derivative programs, then d phi / dt (contiguous, as DeviceFunction.moving_gradient_programs lists them)
static ProgBody<HostEval> body_at(int N, int complement, const pg_program* phi, const pg_program* derivs, double t, HostStack* S) {
  ProgBody<HostEval> b;
  b.N = N; b.complement = 0; b.sgn = complement ? -1.0 : 1.0; b.ev.phi = phi; b.ev.grad = derivs; b.ev.dt = derivs + N; b.ev.S = S;
  b.t = t;
  return b;
}

extern "C" {
// the box at each of nt times.  out: nt rows of (type, vol, cen[3], gamma, cg[3], v_n at cg -- 0 without an interface)
void stp_box_nodes(int N, int complement, const pg_program* phi, const pg_program* derivs, int nt, const double* times,
                   const double* lo, const double* hi, int want_surface, double* out) {
  init();
  HostStack S;
  for (int k = 0; k < nt; ++k) {
    const ProgBody<HostEval> b = body_at(N, complement, phi, derivs, times[k], &S);
    const BoxMeasure m = box_measure(b, lo, hi, want_surface != 0, g_gl);
    double* o = out + 10 * k;
    o[0] = m.type; o[1] = m.vol; o[2] = m.cen[0]; o[3] = m.cen[1]; o[4] = m.cen[2];
    o[5] = m.gamma; o[6] = m.cg[0]; o[7] = m.cg[1]; o[8] = m.cg[2];
    o[9] = m.gamma > 0.0 ? b.normal_speed(m.cg[0], N > 1 ? m.cg[1] : 0.0) : 0.0;
  }
}
void stp_section_nodes(int N, int complement, const pg_program* phi, const pg_program* derivs, int nt, const double* times, int d,
                       double s, const double* lo, const double* hi, double full_measure, double* out) {
  HostStack S;
  for (int k = 0; k < nt; ++k) {
    const ProgBody<HostEval> b = body_at(N, complement, phi, derivs, times[k], &S);
    out[k] = section_measure(b, d, s, lo, hi, full_measure);
  }
}
int stp_type(int N, int complement, const pg_program* phi, const pg_program* derivs, double t, const double* lo, const double* hi) {
  HostStack S;
  const ProgBody<HostEval> b = body_at(N, complement, phi, derivs, t, &S);
  int type;
  pick_ball(b, lo, hi, type);
  return type;
}
// the cheap rule of k_st_classify: 1 fluid during the whole slab, -1 solid, 0 left to the list
int stp_far(int N, int complement, const pg_program* phi, const pg_program* derivs, const double* lo, const double* hi, double t0,
            double t1) {
  HostStack S;
  return prog_st_far(body_at(N, complement, phi, derivs, t0, &S), lo, hi, t0, t1);
}
// 0: accepted; 1: refused, the reason in msg.  dphidt apart: a caller may pass a wrong or missing one
int stp_check(int N, const int64_t* n, const double* nodes0, const double* nodes1, const pg_program* phi, const pg_program* grad,
              const pg_program* dphidt, double t0, double t1, int nq, const double* tau_w, char* msg, int msglen) {
  const double* nodes[2] = {nodes0, nodes1};
  std::string why;
  if (spacetime_program_check(N, n, nodes, phi, grad, dphidt, t0, t1, nq, tau_w, &why)) return 0;
  std::snprintf(msg, (size_t)msglen, "%s", why.c_str());
  return 1;
}
}

#ifdef SPACETIME_MAIN
#include <vector>

namespace {
struct Builder {
  pg_program p;
  Builder() { std::memset(&p, 0, sizeof(p)); }
  Builder& k(double v) { p.konst[p.n_const] = v; return op(PG_OP_CONST, p.n_const++); }
  Builder& var(int i) { return op(PG_OP_VAR, i); }
  Builder& op(int o, int a = 0) { p.op[p.n_ops] = (uint8_t)o; p.arg[p.n_ops] = (uint8_t)a; ++p.n_ops; return *this; }
};

int g_checked = 0;
void die(const char* name, const char* what, double v, double bound) {
  std::printf("%s: %s = %.17g outside [0, %.17g]\n", name, what, v, bound);
  std::exit(1);
}

// every cell of an n^N mesh over [x0, x0 + L]^N integrated over [t0, t1] with the midpoint rule on nq panels: V, Gamma with the
// normal speed, A and B of both directions, the cheap rule -- every figure finite and inside [0, box x dt]
void sweep(const char* name, int N, const pg_program* phi, const pg_program* derivs, int n, double x0, double L, double t0, double t1,
           int nq) {
  const double h = L / n, dt = t1 - t0;
  std::vector<double> tau(nq + 2), out(10 * (nq + 2)), sec(nq + 2);
  for (int k = 0; k < nq; ++k) tau[k] = t0 + dt * (k + 0.5) / nq;
  tau[nq] = t0; tau[nq + 1] = t1;
  const double w = dt / nq;
  for (int comp = 0; comp < 2; ++comp)
    for (int j = 0; j < (N > 1 ? n : 1); ++j)
      for (int i = 0; i < n; ++i) {
        const double lo[3] = {x0 + i * h, x0 + j * h, 0.0}, hi[3] = {x0 + (i + 1) * h, x0 + (j + 1) * h, 0.0};
        const double area = N > 1 ? (hi[0] - lo[0]) * (hi[1] - lo[1]) : hi[0] - lo[0];
        stp_box_nodes(N, comp, phi, derivs, nq + 2, tau.data(), lo, hi, 1, out.data());
        double V = 0.0, G = 0.0, mom[2] = {0.0, 0.0};
        bool full = true, empty = true;
        for (int k = 0; k < nq + 2; ++k) {
          const double* o = &out[10 * k];
          for (int q = 0; q < 10; ++q)
            if (!std::isfinite(o[q])) { std::printf("%s: field %d of cell (%d, %d) at node %d is not finite\n", name, q, i, j, k); std::exit(1); }
          if (!(o[1] >= 0.0 && o[1] <= area)) die(name, "V(tau)", o[1], area);
          full = full && (int)o[0] == PG_FULL;
          empty = empty && (int)o[0] == PG_EMPTY;
          if (k >= nq) continue;
          V += w * o[1];
          G += w * o[5] * std::sqrt(1.0 + o[9] * o[9]);
          for (int d = 0; d < N; ++d) mom[d] += w * o[1] * o[2 + d];
        }
        if (!(V >= 0.0 && V <= area * dt * (1.0 + 1e-14))) die(name, "V", V, area * dt);
        if (!(G >= 0.0) || !std::isfinite(G)) die(name, "Gamma", G, INFINITY);
        const int far = stp_far(N, comp, phi, derivs, lo, hi, t0, t1);
        if ((far == 1 && !full) || (far == -1 && !empty)) {
          std::printf("%s: the cheap rule finished cell (%d, %d) as %d, the all-nodes rule does not agree\n", name, i, j, far);
          std::exit(1);
        }
        for (int d = 0; d < N; ++d) {
          const double ext = N > 1 ? hi[1 - d] - lo[1 - d] : 1.0;
          const double c = V > 0.0 ? mom[d] / V : 0.5 * (lo[d] + hi[d]);
          for (int which = 0; which < 2; ++which) {
            stp_section_nodes(N, comp, phi, derivs, nq, tau.data(), d, which ? c : lo[d], lo, hi, -1.0, sec.data());
            double a = 0.0;
            for (int k = 0; k < nq; ++k) a += w * sec[k];
            if (!(a >= 0.0 && a <= ext * dt * (1.0 + 1e-14))) die(name, which ? "B" : "A", a, ext * dt);
          }
        }
        ++g_checked;
      }
}
}  // namespace

int main() {
  const int nqs[3] = {1, 3, 7};
  for (int nq : nqs) {
    {                                                   // 0 everywhere, at every time
      Builder z;
      z.k(0.0);
      pg_program d[3] = {z.p, z.p, z.p};
      sweep("zero", 2, &z.p, d, 6, 0.0, 1.0, 0.0, 0.1, nq);
      sweep("zero 1-D", 1, &z.p, d, 6, 0.0, 1.0, 0.0, 0.1, nq);
    }
    {                                                   // sqrt(x - 0.5 - t) - 0.4: NaN on the half plane x < 0.5 + t
      Builder f, g0, g1, gt;
      f.var(0).k(0.5).op(PG_OP_SUB).var(3).op(PG_OP_SUB).op(PG_OP_SQRT).k(0.4).op(PG_OP_SUB);
      g0.k(0.5).var(0).k(0.5).op(PG_OP_SUB).var(3).op(PG_OP_SUB).op(PG_OP_SQRT).op(PG_OP_DIV);
      g1.k(0.0);
      gt.k(-0.5).var(0).k(0.5).op(PG_OP_SUB).var(3).op(PG_OP_SUB).op(PG_OP_SQRT).op(PG_OP_DIV);
      pg_program d2[3] = {g0.p, g1.p, gt.p}, d1[2] = {g0.p, gt.p};
      sweep("half NaN", 2, &f.p, d2, 10, 0.0, 1.0, 0.0, 0.05, nq);
      sweep("half NaN 1-D", 1, &f.p, d1, 10, 0.0, 1.0, 0.0, 0.05, nq);
    }
    {                                                   // a disc that appears at t = 0.025 and has radius 0.6 h at mid slab:
      const double hh = 4.0 / 16, r = 0.6 * hh;         // (x - cx)^2 + (y - cy)^2 - r^2 (1 - 40 (0.05 - t))
      Builder f, g0, g1, gt;
      f.var(0).k(2.03).op(PG_OP_SUB).var(0).k(2.03).op(PG_OP_SUB).op(PG_OP_MUL);
      f.var(1).k(2.01).op(PG_OP_SUB).var(1).k(2.01).op(PG_OP_SUB).op(PG_OP_MUL).op(PG_OP_ADD).k(r * r).op(PG_OP_SUB);
      f.k(40.0 * r * r).k(0.05).var(3).op(PG_OP_SUB).op(PG_OP_MUL).op(PG_OP_ADD);
      g0.k(2.0).var(0).k(2.03).op(PG_OP_SUB).op(PG_OP_MUL);
      g1.k(2.0).var(1).k(2.01).op(PG_OP_SUB).op(PG_OP_MUL);
      gt.k(-40.0 * r * r);
      pg_program d[3] = {g0.p, g1.p, gt.p};
      sweep("small disc appearing", 2, &f.p, d, 16, 0.0, 4.0, 0.0, 0.1, nq);
    }
    {                                                   // 1-D: x - (0.37 + 2 t)
      Builder f, g, gt;
      f.var(0).k(0.37).k(2.0).var(3).op(PG_OP_MUL).op(PG_OP_ADD).op(PG_OP_SUB);
      g.k(1.0);
      gt.k(-2.0);
      pg_program d[2] = {g.p, gt.p};
      sweep("moving wall", 1, &f.p, d, 10, 0.0, 1.0, 0.0, 0.1, nq);
    }
  }
  std::printf("spacetime_program_host: %d space-time cells checked\n", g_checked);
  return 0;
}
#endif
