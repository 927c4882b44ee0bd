// Host (g++) build of the MOVING marker polygon (MovingPoly of penguin/jl_amd/csrc/pg_geom_polygon.h: the interpolating view, the
// lookup of the swept edges, the per-piece space-time weight of the front and spacetime_polygon_check), for CPU unit tests only
// (tests/test_moving_polygon_host.py).  The product never loads this library.  A slot is what the space-time kernels hand to the
// primitives: a time node (s = (tau - t0) / (t1 - t0)) or one of the two time faces; one lane measures a box, as in k_st_cells.
// With -DSTP_MAIN: a stand-alone program for the sanitizers.
#include "../penguin/jl_amd/csrc/pg_geom_polygon.h"

#include <cstdio>
#include <cstring>

using namespace pggeom;

namespace {
struct Moving {
  std::vector<double> xy0, xy1, nodes[2];
  PolyBinsHost bins;
  MovingPoly b;
};
MovingPoly view(void* h, int slot, double s) {
  MovingPoly v = ((Moving*)h)->b;
  v.face = slot;
  v.s = slot == 0 ? s : 0.0;
  return v;
}
void say(char* msg, int msglen, const std::string& why) {
  if (msg) std::snprintf(msg, (size_t)msglen, "%s", why.c_str());
}
}  // namespace

extern "C" {
// what the C entry refuses on the host, with its message (1: accepted)
int stp_check(int N, const double* xy0, const double* xy1, int64_t M, double t0, double t1, int nq, const double* tau_w, char* msg,
              int msglen) {
  std::string why;
  M = moving_polygon_open_count(xy0, xy1, M);
  const bool ok = spacetime_polygon_check(N, xy0, xy1, M, t0, t1, nq, tau_w, &why);
  say(msg, msglen, why);
  return ok ? 1 : 0;
}
// 0 on a refusal (the reason in msg)
void* stp_new(const double* xy0, const double* xy1, int64_t M, int complement, int n0, int n1, const double* nodes0,
              const double* nodes1, double t0, double t1, int nq, const double* tau_w, char* msg, int msglen) {
  if (!stp_check(2, xy0, xy1, M, t0, t1, nq, tau_w, msg, msglen)) return nullptr;
  M = moving_polygon_open_count(xy0, xy1, M);
  Moving* p = new Moving();
  p->xy0 = polygon_normalise_as(xy0, xy0, M);
  p->xy1 = polygon_normalise_as(xy1, xy0, M);
  p->nodes[0].assign(nodes0, nodes0 + n0 + 1);
  p->nodes[1].assign(nodes1, nodes1 + n1 + 1);
  MovingPoly& b = p->b;
  b.N = 2; b.complement = 0; b.flip = complement ? 1 : 0; b.M = (int)M; b.xy = p->xy0.data(); b.xy1 = p->xy1.data();
  b.n[0] = n0; b.n[1] = n1; b.nodes[0] = p->nodes[0].data(); b.nodes[1] = p->nodes[1].data();
  b.ptr = nullptr; b.idx = nullptr; b.s = 0.0; b.dt = t1 - t0; b.face = 1;
  p->bins = polygon_bins_host(b);
  b.ptr = p->bins.ptr.data();
  b.idx = p->bins.idx.data();
  return p;
}
void stp_free(void* h) { delete (Moving*)h; }
// out: type, vol, cen[3], gamma, cg[3]  (9 doubles).  slot 0: the time node with this s; 1 / 2: the faces t0 / t1
void stp_box(void* h, int slot, double s, const double* lo, const double* hi, int want_surface, double* out) {
  GLTable gl;                   // (not read)
  const BoxMeasure m = box_measure(view(h, slot, s), lo, hi, want_surface != 0, gl);
  out[0] = m.type; out[1] = m.vol; out[2] = m.cen[0]; out[3] = m.cen[1]; out[4] = m.cen[2];
  out[5] = m.gamma; out[6] = m.cg[0]; out[7] = m.cg[1]; out[8] = m.cg[2];
}
double stp_section(void* h, int slot, double s, int d, double x, const double* lo, const double* hi, double full_measure) {
  return section_measure(view(h, slot, s), d, x, lo, hi, full_measure);
}
// type, and 256 if the box owns a piece of the front
int stp_type(void* h, int slot, double s, const double* lo, const double* hi) {
  int t;
  const int own = pick_ball(view(h, slot, s), lo, hi, t);
  return (t & 255) | (own << 8);
}
// the cheap pass of cell (i, j): 0 its swept list is not empty, 1 / -1 fluid / not by the parity of its centre at t0
int stp_far(void* h, int i, int j) {
  const MovingPoly f = view(h, 1, 0.0);
  const int bin = poly_cell_bin(f, i, j);
  if (f.ptr[bin + 1] > f.ptr[bin]) return 0;
  return poly_fluid_at(f, 0.5 * (f.nodes[0][i] + f.nodes[0][i + 1]), 0.5 * (f.nodes[1][j] + f.nodes[1][j + 1])) ? 1 : -1;
}
int stp_bin_size(void* h, int bin) { return ((Moving*)h)->bins.ptr[bin + 1] - ((Moving*)h)->bins.ptr[bin]; }
int stp_bin_entry(void* h, int bin, int k) { return ((Moving*)h)->bins.idx[((Moving*)h)->bins.ptr[bin] + k]; }
// the normalised markers at the face t0 (which = 0) or t1 (1), or of the view at s (2)
void stp_markers(void* h, int which, double s, double* out) {
  const MovingPoly v = view(h, which == 0 ? 1 : which == 1 ? 2 : 0, s);
  for (int k = 0; k < v.M; ++k) poly_vertex(v, k, out[2 * k], out[2 * k + 1]);
}
}

#ifdef STP_MAIN
namespace {
int g_checked = 0;
void fail(const char* name, const char* what, int i, int j) {
  std::printf("%s: %s at cell (%d, %d)\n", name, what, i, j);
  std::exit(1);
}
// every cell at every slot of an nq-node midpoint rule: finite, within [0, box measure], the types of pick_ball and box_measure
// agree, the bins ascend, and a cell the cheap pass finishes has the same type at every slot
void sweep(const char* name, const std::vector<double>& a, const std::vector<double>& b, int n0, int n1, double x0, double L, int nq) {
  std::vector<double> nx(n0 + 1), ny(n1 + 1), tw;
  for (int i = 0; i <= n0; ++i) nx[i] = x0 + i * (L / n0);
  for (int j = 0; j <= n1; ++j) ny[j] = x0 + j * (L / n1);
  const double t0 = 0.25, t1 = 0.375;
  for (int k = 0; k < nq; ++k) { tw.push_back(t0 + (k + 0.5) * (t1 - t0) / nq); tw.push_back((t1 - t0) / nq); }
  for (int comp = 0; comp < 2; ++comp) {
    char msg[512];
    void* h = stp_new(a.data(), b.data(), (int64_t)a.size() / 2, comp, n0, n1, nx.data(), ny.data(), t0, t1, nq, tw.data(), msg, 512);
    if (!h) { std::printf("%s: refused: %s\n", name, msg); std::exit(1); }
    const int nb = n0 + n1 + n0 * n1;
    for (int bin = 0; bin < nb; ++bin)
      for (int k = 1; k < stp_bin_size(h, bin); ++k)
        if (!(stp_bin_entry(h, bin, k - 1) < stp_bin_entry(h, bin, k))) fail(name, "a bin is not in ascending edge order", bin, k);
    double total = 0.0;
    for (int j = 0; j < n1; ++j)
      for (int i = 0; i < n0; ++i) {
        const double lo[3] = {nx[i], ny[j], 0.0}, hi[3] = {nx[i + 1], ny[j + 1], 0.0};
        const double area = (hi[0] - lo[0]) * (hi[1] - lo[1]);
        const int far = stp_far(h, i, j);
        for (int slot = 0; slot < nq + 2; ++slot) {
          const int kind = slot < nq ? 0 : slot - nq + 1;
          const double s = slot < nq ? (tw[2 * slot] - t0) / (t1 - t0) : 0.0;
          double o[9];
          stp_box(h, kind, s, lo, hi, 1, o);
          for (int q = 0; q < 9; ++q)
            if (!std::isfinite(o[q])) fail(name, "a field is not finite", i, j);
          if (!(o[1] >= 0.0 && o[1] <= area)) fail(name, "V outside [0, area]", i, j);
          if (!(o[5] >= 0.0)) fail(name, "Gamma < 0", i, j);
          const int t = stp_type(h, kind, s, lo, hi) & 255;
          if ((t == 255 ? -1 : t) != (int)o[0]) fail(name, "pick_ball and box_measure disagree on the type", i, j);
          if (far != 0 && (int)o[0] != (far == 1 ? 1 : 0)) fail(name, "the cheap pass disagrees with a slot", i, j);
          for (int d = 0; d < 2; ++d) {
            const double ext = hi[1 - d] - lo[1 - d];
            const double sa = stp_section(h, kind, s, d, lo[d], lo, hi, -1.0), sb = stp_section(h, kind, s, d, o[2 + d], lo, hi, -1.0);
            if (!(sa >= 0.0 && sa <= ext && sb >= 0.0 && sb <= ext)) fail(name, "a section outside [0, extent]", i, j);
          }
          if (i > 0) {                                            // the staggered box between two centres
            const double slo[3] = {0.5 * (nx[i - 1] + nx[i]), ny[j], 0.0}, shi[3] = {0.5 * (nx[i] + nx[i + 1]), ny[j + 1], 0.0};
            double w[9];
            stp_box(h, kind, s, slo, shi, 0, w);
            if (!(w[1] >= 0.0 && w[1] <= area * (1.0 + 1e-12))) fail(name, "W outside [0, area]", i, j);
          }
          if (slot < nq) total += tw[2 * slot + 1] * o[1];
          ++g_checked;
        }
      }
    std::printf("%s (complement %d): sum V = %.15g\n", name, comp, total);
    stp_free(h);
  }
}
}  // namespace

int main() {
  const double pi = 3.14159265358979323846;
  // a triangle that collapses towards a line at t1 (its apex ends 1e-9 above the base), and a single time node
  sweep("collapsing triangle, nq = 1", {0.7, 1.1, 3.3, 1.2, 2.1, 3.4}, {0.7, 1.1, 3.3, 1.2, 2.0, 1.15 + 1e-9}, 8, 8, 0.0, 4.0, 1);
  sweep("collapsing triangle, nq = 5", {0.7, 1.1, 3.3, 1.2, 2.1, 3.4}, {0.7, 1.1, 3.3, 1.2, 2.0, 1.15 + 1e-9}, 9, 7, -0.3, 4.0, 5);
  std::vector<double> c0, c1, far0, far1;
  for (int i = 0; i < 40; ++i) {
    const double a = 2.0 * pi * ((double)i / 40);
    c0.push_back(2.01 + 1.5 * std::cos(a)); c0.push_back(2.01 + 1.5 * std::sin(a));       // markers leave the mesh during the slab
    c1.push_back(3.41 + 1.5 * std::cos(a)); c1.push_back(1.21 + 1.5 * std::sin(a));
    far0.push_back(9.0 + std::cos(a)); far0.push_back(9.0 + std::sin(a));                  // never in the mesh: every swept list empty
    far1.push_back(9.5 + std::cos(a)); far1.push_back(9.0 + std::sin(a));
  }
  sweep("circle with markers outside the mesh", c0, c1, 7, 5, 0.0, 4.0, 3);
  sweep("polygon outside the mesh (empty swept lists)", far0, far1, 6, 6, 0.0, 4.0, 2);
  std::printf("spacetime_polygon_host: %d boxes checked\n", g_checked);
  return 0;
}
#endif
