// Host (g++) build of the oblique half-space device functions of pg_geom.h, for CPU unit tests only
// (tests/test_plane_host.py).  The product never loads this library.
#include <string.h>

#include "../penguin/jl_amd/csrc/pg_geom.h"
using namespace pggeom;
static GLTable g_gl;
static bool g_init = false;
static void init() { if (!g_init) { gl_init(g_gl); g_init = true; } }

static BallSet plane_set(int N, int complement, const double* normal, double offset) {
  BallSet bs;
  memset(&bs, 0, sizeof(bs));
  bs.kind = BODY_PLANE; bs.N = N; bs.nballs = 1; bs.complement = complement; bs.r = 1.0;
  bs.ax[0] = bs.ax[1] = bs.ax[2] = 1.0;
  for (int d = 0; d < N; ++d) bs.c[0][d] = normal[d];
  bs.pos = offset;
  return bs;
}

static BallSet halfspace_set(int N, int complement, int axis, double pos, double sgn) {
  BallSet bs;
  memset(&bs, 0, sizeof(bs));
  bs.kind = BODY_HALFSPACE; bs.N = N; bs.nballs = 1; bs.complement = complement; bs.r = 1.0;
  bs.ax[0] = bs.ax[1] = bs.ax[2] = 1.0;
  bs.axis = axis; bs.pos = pos; bs.sgn = sgn < 0.0 ? -1.0 : 1.0;
  return bs;
}

static void put(const BoxMeasure& m, double* out) {
  out[0] = m.type; out[1] = m.vol; out[2] = m.cen[0]; out[3] = m.cen[1]; out[4] = m.cen[2];
  out[5] = m.gamma; out[6] = m.cg[0]; out[7] = m.cg[1]; out[8] = m.cg[2];
}

extern "C" {
// out: type, vol, cen[3], gamma, cg[3]  (9 doubles)
void plane_box(int N, int complement, const double* normal, double offset, const double* lo, const double* hi,
               int want_surface, double* out) {
  init();
  put(box_measure(plane_set(N, complement, normal, offset), lo, hi, want_surface != 0, g_gl), out);
}
// full_measure < 0: the section computes the measure of a full section itself
double plane_section(int N, int complement, const double* normal, double offset, int d, double s, const double* lo,
                     const double* hi, double full_measure) {
  return section_measure(plane_set(N, complement, normal, offset), d, s, lo, hi, full_measure);
}
// the type pick_ball gives the kernels (with respect to the body as given; its callers apply the complement)
int plane_pick_type(int N, const double* normal, double offset, const double* lo, const double* hi) {
  int t;
  pick_ball(plane_set(N, 0, normal, offset), lo, hi, t);
  return t;
}
void halfspace_box(int N, int complement, int axis, double pos, double sgn, const double* lo, const double* hi,
                   int want_surface, double* out) {
  init();
  put(box_measure(halfspace_set(N, complement, axis, pos, sgn), lo, hi, want_surface != 0, g_gl), out);
}
double halfspace_section(int N, int complement, int axis, double pos, double sgn, int d, double s, const double* lo,
                         const double* hi) {
  return section_measure(halfspace_set(N, complement, axis, pos, sgn), d, s, lo, hi);
}
}
