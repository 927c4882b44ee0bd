// Host (g++) build of the 3-D program-body geometry (penguin/jl_amd/csrc/pg_geom_program3.h), for CPU unit tests only
// (tests/test_levelset3d_host.py).  The product never loads this library.
#include "../penguin/jl_amd/csrc/pg_geom_program3.h"

#include <cstdio>
#include <cstring>

using namespace pggeom;
using pgprog::HostStack;

static GLTable g_gl;
static bool g_init = false;
static void init() { if (!g_init) { gl_init(g_gl); g_init = true; } }

static Prog3Body<HostEval3> body_of(int complement, const pg_program* phi, const pg_program* grad, HostStack* S) {
  Prog3Body<HostEval3> b;
  b.N = 3; b.complement = 0; b.sgn = complement ? -1.0 : 1.0; b.ev.phi = phi; b.ev.grad = grad; b.ev.S = S;
  return b;
}

extern "C" {
// out: type, vol, cen[3], gamma, cg[3]  (9 doubles).  (qlane, qstride): the share of the quadrature, (0, 1) is all of it
void ls3_box(int complement, const pg_program* phi, const pg_program* grad, const double* lo, const double* hi, int want_surface,
             int qlane, int qstride, double* out) {
  init();
  HostStack S;
  const Prog3Body<HostEval3> b = body_of(complement, phi, grad, &S);
  BoxMeasure m = box_measure(b, lo, hi, want_surface != 0, g_gl, qlane, qstride);
  out[0] = m.type; out[1] = m.vol; out[2] = m.cen[0]; out[3] = m.cen[1]; out[4] = m.cen[2];
  out[5] = m.gamma; out[6] = m.cg[0]; out[7] = m.cg[1]; out[8] = m.cg[2];
}
double ls3_section(int complement, const pg_program* phi, const pg_program* grad, int d, double s, const double* lo, const double* hi,
                   double full_measure) {
  init();
  HostStack S;
  const Prog3Body<HostEval3> b = body_of(complement, phi, grad, &S);
  return section_measure(b, d, s, lo, hi, full_measure, g_gl);
}
int ls3_type(int complement, const pg_program* phi, const pg_program* grad, const double* lo, const double* hi) {
  HostStack S;
  const Prog3Body<HostEval3> b = body_of(complement, phi, grad, &S);
  int t;
  pick_ball(b, lo, hi, t);
  return t;
}
// 0: accepted; 1: refused, the reason in msg
int ls3_check(int N, const int64_t* n, const double* nodes0, const double* nodes1, const double* nodes2, const pg_program* phi,
              const pg_program* grad, int single_rank, char* msg, int msglen) {
  const double* nodes[3] = {nodes0, nodes1, nodes2};
  std::string why;
  if (program3_body_check(N, n, nodes, phi, grad, single_rank != 0, &why)) return 0;
  std::snprintf(msg, (size_t)msglen, "%s", why.c_str());
  return 1;
}
}
