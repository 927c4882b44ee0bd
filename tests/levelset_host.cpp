// Host (g++) build of the program-body geometry (penguin/jl_amd/csrc/pg_geom_program.h), for CPU unit tests only
// (tests/test_levelset_host.py).  The product never loads this library.  With -DLEVELSET_MAIN: a stand-alone program for the
// sanitizers (valid bodies, a body that is 0 everywhere, one that is NaN on half the plane, an under-resolved disc).
#include "../penguin/jl_amd/csrc/pg_geom_program.h"

#include <cstdio>
#include <cstring>

using namespace pggeom;
using pgprog::HostStack;

static GLTable g_gl;
static bool g_init = false;
static void init() { if (!g_init) { gl_init(g_gl); g_init = true; } }

static ProgBody<HostEval> body_of(int N, int complement, const pg_program* phi, const pg_program* grad, HostStack* S) {
  ProgBody<HostEval> b;
  b.N = N; b.complement = 0; b.sgn = complement ? -1.0 : 1.0; b.ev.phi = phi; b.ev.grad = grad; b.ev.S = S;
  return b;
}

extern "C" {
// out: type, vol, cen[3], gamma, cg[3]  (9 doubles)
void ls_box(int N, int complement, const pg_program* phi, const pg_program* grad, const double* lo, const double* hi,
            int want_surface, double* out) {
  init();
  HostStack S;
  const ProgBody<HostEval> b = body_of(N, complement, phi, grad, &S);
  BoxMeasure m = box_measure(b, lo, hi, want_surface != 0, g_gl);
  out[0] = m.type; out[1] = m.vol; out[2] = m.cen[0]; out[3] = m.cen[1]; out[4] = m.cen[2];
  out[5] = m.gamma; out[6] = m.cg[0]; out[7] = m.cg[1]; out[8] = m.cg[2];
}
double ls_section(int N, int complement, const pg_program* phi, const pg_program* grad, int d, double s, const double* lo,
                  const double* hi, double full_measure) {
  HostStack S;
  const ProgBody<HostEval> b = body_of(N, complement, phi, grad, &S);
  return section_measure(b, d, s, lo, hi, full_measure);
}
int ls_type(int N, int complement, const pg_program* phi, const pg_program* grad, const double* lo, const double* hi) {
  HostStack S;
  const ProgBody<HostEval> b = body_of(N, complement, phi, grad, &S);
  int t;
  pick_ball(b, lo, hi, t);
  return t;
}
// roots of phi along `axis` in [a, b] at the fixed coordinate `other`: number, and their sum (test of seg_roots' conventions)
void ls_segment(int N, const pg_program* phi, const pg_program* grad, int axis, double other, double a, double b, double* out) {
  HostStack S;
  const ProgBody<HostEval> bd = body_of(N, 0, phi, grad, &S);
  SegOut s;
  seg_measure(bd, axis, other, a, b, false, s);
  out[0] = s.len; out[1] = s.mom; out[2] = s.nroots; out[3] = s.rsum;
}
// 0: accepted; 1: refused, the reason in msg
int ls_check(int N, const int64_t* n, const double* nodes0, const double* nodes1, const pg_program* phi, const pg_program* grad,
             char* msg, int msglen) {
  const double* nodes[2] = {nodes0, nodes1};
  std::string why;
  if (program_body_check(N, n, nodes, phi, grad, &why)) return 0;
  std::snprintf(msg, (size_t)msglen, "%s", why.c_str());
  return 1;
}
}

#ifdef LEVELSET_MAIN
#include <cassert>
#include <vector>

namespace {
struct Builder {
  pg_program p;
  Builder() { std::memset(&p, 0, sizeof(p)); }
  Builder& k(double v) { p.konst[p.n_const] = v; return op(PG_OP_CONST, p.n_const++); }
  Builder& var(int i) { return op(PG_OP_VAR, i); }
  Builder& op(int o, int a = 0) { p.op[p.n_ops] = (uint8_t)o; p.arg[p.n_ops] = (uint8_t)a; ++p.n_ops; return *this; }
};

// (x - cx)^2 + (y - cy)^2 - r^2 and its gradient
void disc(double cx, double cy, double r, pg_program* phi, pg_program* grad) {
  Builder f;
  f.var(0).k(cx).op(PG_OP_SUB).var(0).k(cx).op(PG_OP_SUB).op(PG_OP_MUL);
  f.var(1).k(cy).op(PG_OP_SUB).var(1).k(cy).op(PG_OP_SUB).op(PG_OP_MUL).op(PG_OP_ADD).k(r * r).op(PG_OP_SUB);
  *phi = f.p;
  for (int d = 0; d < 2; ++d) {
    Builder g;
    g.k(2.0).var(d).k(d ? cy : cx).op(PG_OP_SUB).op(PG_OP_MUL);
    grad[d] = g.p;
  }
}

int g_checked = 0;
void sweep(const char* name, int N, const pg_program* phi, const pg_program* grad, int n, double x0, double L) {
  const double h = L / n;
  for (int comp = 0; comp < 2; ++comp)
    for (int j = 0; j < (N > 1 ? n : 1); ++j)
      for (int i = 0; i < n; ++i) {
        const double lo[3] = {x0 + i * h, x0 + j * h, 0.0}, hi[3] = {x0 + (i + 1) * h, x0 + (j + 1) * h, 0.0};
        const double area = N > 1 ? (hi[0] - lo[0]) * (hi[1] - lo[1]) : hi[0] - lo[0];
        double o[9];
        ls_box(N, comp, phi, grad, lo, hi, 1, o);
        for (int q = 0; q < 9; ++q)
          if (!std::isfinite(o[q])) { std::printf("%s: field %d of cell (%d, %d) is not finite\n", name, q, i, j); std::exit(1); }
        if (!(o[1] >= 0.0 && o[1] <= area)) { std::printf("%s: V = %.17g outside [0, %.17g]\n", name, o[1], area); std::exit(1); }
        if (!(o[5] >= 0.0)) { std::printf("%s: Gamma = %.17g\n", name, o[5]); std::exit(1); }
        for (int d = 0; d < N; ++d) {
          const double ext = N > 1 ? hi[1 - d] - lo[1 - d] : 1.0;
          const double a = ls_section(N, comp, phi, grad, d, lo[d], lo, hi, -1.0);
          const double b = ls_section(N, comp, phi, grad, d, o[2 + d], lo, hi, -1.0);
          if (!(a >= 0.0 && a <= ext && b >= 0.0 && b <= ext)) { std::printf("%s: section %.17g / %.17g outside [0, %.17g]\n", name, a, b, ext); std::exit(1); }
        }
        const int t = ls_type(N, comp, phi, grad, lo, hi);
        if (t != (int)o[0]) { std::printf("%s: pick_ball and box_measure disagree on the type\n", name); std::exit(1); }
        ++g_checked;
      }
}
}  // namespace

int main() {
  pg_program phi, grad[2];
  disc(2.01, 1.97, 1.0, &phi, grad);
  sweep("disc", 2, &phi, grad, 12, 0.0, 4.0);
  disc(2.0, 2.0, 1.0, &phi, grad);                    // the interface through nodes
  sweep("disc on nodes", 2, &phi, grad, 8, 0.0, 4.0);
  disc(2.03, 2.01, 0.6 * (4.0 / 16), &phi, grad);     // under-resolved: radius 0.6 h
  sweep("small disc", 2, &phi, grad, 16, 0.0, 4.0);
  {                                                   // 0 everywhere
    Builder z, g;
    z.k(0.0);
    g.k(0.0);
    pg_program gz[2] = {g.p, g.p};
    sweep("zero", 2, &z.p, gz, 6, 0.0, 1.0);
    sweep("zero 1-D", 1, &z.p, gz, 6, 0.0, 1.0);
  }
  {                                                   // sqrt(x - 0.5) - 0.4: NaN for x < 0.5
    Builder f, g0, g1;
    f.var(0).k(0.5).op(PG_OP_SUB).op(PG_OP_SQRT).k(0.4).op(PG_OP_SUB);
    g0.k(0.5).var(0).k(0.5).op(PG_OP_SUB).op(PG_OP_SQRT).op(PG_OP_DIV);
    g1.k(0.0);
    pg_program gr[2] = {g0.p, g1.p};
    sweep("half NaN", 2, &f.p, gr, 10, 0.0, 1.0);
    sweep("half NaN 1-D", 1, &f.p, gr, 10, 0.0, 1.0);
  }
  {                                                   // 1-D: x - 0.37
    Builder f, g;
    f.var(0).k(0.37).op(PG_OP_SUB);
    g.k(1.0);
    sweep("x - 0.37", 1, &f.p, &g.p, 10, 0.0, 1.0);
  }
  std::printf("levelset_host: %d boxes checked\n", g_checked);
  return 0;
}
#endif
