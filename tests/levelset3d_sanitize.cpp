// Stand-alone program for the sanitizers (tests/test_levelset3d_host.py builds it with -fsanitize=address,undefined and runs
// it): box type, box measure and section measure of penguin/jl_amd/csrc/pg_geom_program3.h on boxes of a torus and of an oblique
// plane, both phases, and of a body that is 0 everywhere.  It asserts finite results within [0, box measure] itself.
#include "../penguin/jl_amd/csrc/pg_geom_program3.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace pggeom;

namespace {
struct Builder {
  pg_program p;
  Builder() { std::memset(&p, 0, sizeof(p)); }
  Builder& k(double v) { p.konst[p.n_const] = v; return op(PG_OP_CONST, p.n_const++); }
  Builder& var(int i) { return op(PG_OP_VAR, i); }
  Builder& op(int o, int a = 0) { p.op[p.n_ops] = (uint8_t)o; p.arg[p.n_ops] = (uint8_t)a; ++p.n_ops; return *this; }
  Builder& sq_diff(int i, double c) { return var(i).k(c).op(PG_OP_SUB).var(i).k(c).op(PG_OP_SUB).op(PG_OP_MUL); }
  Builder& rho(double cx, double cy) { return sq_diff(0, cx).sq_diff(1, cy).op(PG_OP_ADD).op(PG_OP_SQRT); }
};

// (sqrt((x - cx)^2 + (y - cy)^2) - R)^2 + (z - cz)^2 - r^2 and its gradient
void torus(const double* c, double R, double r, pg_program* phi, pg_program* grad) {
  Builder f;
  f.rho(c[0], c[1]).k(R).op(PG_OP_SUB).rho(c[0], c[1]).k(R).op(PG_OP_SUB).op(PG_OP_MUL).sq_diff(2, c[2]).op(PG_OP_ADD).k(r * r).op(PG_OP_SUB);
  *phi = f.p;
  for (int d = 0; d < 2; ++d) {                  // 2 (rho - R) (x_d - c_d) / rho
    Builder g;
    g.k(2.0).rho(c[0], c[1]).k(R).op(PG_OP_SUB).op(PG_OP_MUL).var(d).k(c[d]).op(PG_OP_SUB).op(PG_OP_MUL).rho(c[0], c[1]).op(PG_OP_DIV);
    grad[d] = g.p;
  }
  Builder gz;
  gz.k(2.0).var(2).k(c[2]).op(PG_OP_SUB).op(PG_OP_MUL);
  grad[2] = gz.p;
}

GLTable g_gl;
int g_checked = 0;

void fail(const char* name, const char* what, double v) {
  std::printf("%s: %s = %.17g\n", name, what, v);
  std::exit(1);
}

void sweep(const char* name, const pg_program* phi, const pg_program* grad, int n, double x0, double L, int stride) {
  const double h = L / n;
  pgprog::HostStack S;
  int cell = 0;
  for (int comp = 0; comp < 2; ++comp)
    for (int k = 0; k < n; ++k)
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
          if (cell++ % stride) continue;
          Prog3Body<HostEval3> b;
          b.N = 3; b.complement = 0; b.sgn = comp ? -1.0 : 1.0; b.ev.phi = phi; b.ev.grad = grad; b.ev.S = &S;
          const double lo[3] = {x0 + i * h, x0 + j * h, x0 + k * h}, hi[3] = {x0 + (i + 1) * h, x0 + (j + 1) * h, x0 + (k + 1) * h};
          const double vol = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]);
          const BoxMeasure m = box_measure(b, lo, hi, true, g_gl);
          int t;
          pick_ball(b, lo, hi, t);
          if (t != m.type) fail(name, "pick_ball and box_measure disagree, type", m.type);
          if (!(m.vol >= 0.0 && m.vol <= vol)) fail(name, "V", m.vol);
          if (!(m.gamma >= 0.0 && std::isfinite(m.gamma))) fail(name, "Gamma", m.gamma);
          for (int d = 0; d < 3; ++d) {
            if (!(m.cen[d] >= lo[d] && m.cen[d] <= hi[d])) fail(name, "centroid", m.cen[d]);
            if (!std::isfinite(m.cg[d])) fail(name, "interface centroid", m.cg[d]);
            const int p = d == 0 ? 1 : 0, q = d == 2 ? 1 : 2;
            const double face = (hi[p] - lo[p]) * (hi[q] - lo[q]);
            const double a = section_measure(b, d, lo[d], lo, hi, -1.0, g_gl), c = section_measure(b, d, m.cen[d], lo, hi, -1.0, g_gl);
            if (!(a >= 0.0 && a <= face)) fail(name, "A", a);
            if (!(c >= 0.0 && c <= face)) fail(name, "B", c);
          }
          // the 64 shares of the quadrature, as the kernels take them
          double part = 0.0;
          if (m.type == PG_CUT && g_checked % 8 == 0)
            for (int l = 0; l < 64; ++l) part += box_measure(b, lo, hi, false, g_gl, l, 64).vol;
          if (part != 0.0 && !(std::fabs(part - m.vol) <= 1e-12 * vol)) fail(name, "sum of the lane shares", part);
          ++g_checked;
        }
}
}  // namespace

int main() {
  gl_init(g_gl);
  pg_program phi, grad[3];
  const double c[3] = {2.03, 1.96, 2.07};
  torus(c, 1.2, 0.5, &phi, grad);
  sweep("torus", &phi, grad, 6, 0.0, 4.0, 11);
  {
    Builder f, g0, g1, g2;
    f.k(0.6).var(0).op(PG_OP_MUL).k(-0.64).var(1).op(PG_OP_MUL).op(PG_OP_ADD).k(0.48).var(2).op(PG_OP_MUL).op(PG_OP_ADD).k(0.37).op(PG_OP_SUB);
    g0.k(0.6); g1.k(-0.64); g2.k(0.48);
    pg_program gr[3] = {g0.p, g1.p, g2.p};
    sweep("plane", &f.p, gr, 4, -1.0, 3.0, 5);
  }
  {                                                   // 0 everywhere
    Builder z;
    z.k(0.0);
    pg_program gz[3] = {z.p, z.p, z.p};
    sweep("zero", &z.p, gz, 2, 0.0, 1.0, 3);
  }
  std::printf("levelset3d_sanitize: %d boxes checked\n", g_checked);
  return 0;
}
