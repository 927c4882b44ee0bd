// Host (g++) build of the marker-polygon geometry (penguin/jl_amd/csrc/pg_geom_polygon.h), for CPU unit tests only
// (tests/test_polygon_host.py).  The product never loads this library.  A box is measured as the kernels measure it: 16 lanes
// stride over the edge lists and their partial sums go through the butterfly of LaneGroup<16>, emulated here lane by lane.
// With -DPOLYGON_MAIN: a stand-alone program for the sanitizers (the host binning and the three primitives on a circle of 2000
// markers over 8^2 cells and on a square whose markers and edges lie on node lines).
#include "../penguin/jl_amd/csrc/pg_geom_polygon.h"

#include <cstdio>
#include <cstring>

using namespace pggeom;

namespace {
struct Poly {
  std::vector<double> xy, nodes[2];
  PolyBinsHost bins;
  PolyBody b;
};

struct Record {                 // lanes 1 .. 15: keep the partial sums
  Mom* slot;
  void operator()(Mom& m) const { *slot = m; }
};
struct Butterfly {              // lane 0: what __shfl_xor with offsets 8, 4, 2, 1 leaves in it
  Mom* part;                    // 16, [0] is filled here
  static void add(Mom& a, const Mom& b) {
    a.vol += b.vol; a.gamma += b.gamma;
    for (int d = 0; d < 3; ++d) { a.m[d] += b.m[d]; a.gm[d] += b.gm[d]; }
  }
  void operator()(Mom& m) const {
    part[0] = m;
    for (int off = 8; off > 0; off >>= 1) {
      Mom next[16];
      for (int l = 0; l < 16; ++l) { next[l] = part[l]; add(next[l], part[l ^ off]); }
      for (int l = 0; l < 16; ++l) part[l] = next[l];
    }
    m = part[0];
  }
};
}  // namespace

extern "C" {
// 0 on a refusal (the reason in msg)
void* poly_new(const double* xy, int64_t M, int complement, int n0, int n1, const double* nodes0, const double* nodes1, char* msg,
               int msglen) {
  M = polygon_open_count(xy, M);
  std::string why;
  if (!polygon_body_check(xy, M, &why)) {
    if (msg) std::snprintf(msg, (size_t)msglen, "%s", why.c_str());
    return nullptr;
  }
  Poly* p = new Poly();
  p->xy = polygon_normalise(xy, M);
  p->nodes[0].assign(nodes0, nodes0 + n0 + 1);
  p->nodes[1].assign(nodes1, nodes1 + n1 + 1);
  PolyBody& b = p->b;
  b.N = 2; b.complement = 0; b.flip = complement ? 1 : 0; b.M = (int)M; b.xy = p->xy.data();
  b.n[0] = n0; b.n[1] = n1; b.nodes[0] = p->nodes[0].data(); b.nodes[1] = p->nodes[1].data();
  b.ptr = nullptr; b.idx = nullptr;
  p->bins = polygon_bins_host(b);
  b.ptr = p->bins.ptr.data();
  b.idx = p->bins.idx.data();
  return p;
}
void poly_free(void* h) { delete (Poly*)h; }
// out: type, vol, cen[3], gamma, cg[3]  (9 doubles); lanes: 1 or 16
void poly_box(void* h, const double* lo, const double* hi, int want_surface, int lanes, double* out) {
  const PolyBody& b = ((Poly*)h)->b;
  GLTable gl;                   // (not read)
  BoxMeasure m;
  if (lanes == 16) {
    Mom part[16];
    for (int l = 1; l < 16; ++l) box_measure(b, lo, hi, want_surface != 0, gl, l, 16, Record{&part[l]});
    m = box_measure(b, lo, hi, want_surface != 0, gl, 0, 16, Butterfly{part});
  } else {
    m = box_measure(b, lo, hi, want_surface != 0, gl);
  }
  out[0] = m.type; out[1] = m.vol; out[2] = m.cen[0]; out[3] = m.cen[1]; out[4] = m.cen[2];
  out[5] = m.gamma; out[6] = m.cg[0]; out[7] = m.cg[1]; out[8] = m.cg[2];
}
double poly_section_c(void* h, int d, double s, const double* lo, const double* hi, double full_measure) {
  return section_measure(((Poly*)h)->b, d, s, lo, hi, full_measure);
}
// type, and 256 if the box owns a piece of the front
int poly_type(void* h, const double* lo, const double* hi) {
  int t;
  const int own = pick_ball(((Poly*)h)->b, lo, hi, t);
  return (t & 255) | (own << 8);
}
int poly_bin_size(void* h, int bin) { return ((Poly*)h)->bins.ptr[bin + 1] - ((Poly*)h)->bins.ptr[bin]; }
int poly_bin_entry(void* h, int bin, int k) { return ((Poly*)h)->bins.idx[((Poly*)h)->bins.ptr[bin] + k]; }
void poly_markers(void* h, double* out) { std::memcpy(out, ((Poly*)h)->xy.data(), ((Poly*)h)->xy.size() * sizeof(double)); }
}

#ifdef POLYGON_MAIN
namespace {
int g_checked = 0;
void fail(const char* name, const char* what, int i, int j) {
  std::printf("%s: %s at cell (%d, %d)\n", name, what, i, j);
  std::exit(1);
}
void sweep(const char* name, const std::vector<double>& xy, int n0, int n1, double x0, double L) {
  std::vector<double> nx(n0 + 1), ny(n1 + 1);
  for (int i = 0; i <= n0; ++i) nx[i] = x0 + i * (L / n0);
  for (int j = 0; j <= n1; ++j) ny[j] = x0 + j * (L / n1);
  for (int comp = 0; comp < 2; ++comp) {
    char msg[256];
    void* h = poly_new(xy.data(), (int64_t)xy.size() / 2, comp, n0, n1, nx.data(), ny.data(), msg, 256);
    if (!h) { std::printf("%s: refused: %s\n", name, msg); std::exit(1); }
    const int nb = n0 + n1 + n0 * n1;
    for (int bin = 0; bin < nb; ++bin)
      for (int k = 1; k < poly_bin_size(h, bin); ++k)
        if (!(poly_bin_entry(h, bin, k - 1) < poly_bin_entry(h, bin, k))) fail(name, "a bin is not in ascending edge order", bin, k);
    double total = 0.0;
    for (int j = 0; j < n1; ++j)
      for (int i = 0; i < n0; ++i) {
        const double lo[3] = {nx[i], ny[j], 0.0}, hi[3] = {nx[i + 1], ny[j + 1], 0.0};
        const double area = (hi[0] - lo[0]) * (hi[1] - lo[1]);
        double o[9], o1[9];
        poly_box(h, lo, hi, 1, 16, o);
        poly_box(h, lo, hi, 1, 1, o1);
        for (int q = 0; q < 9; ++q)
          if (!std::isfinite(o[q]) || !std::isfinite(o1[q])) fail(name, "a field is not finite", i, j);
        if (!(o[1] >= 0.0 && o[1] <= area)) fail(name, "V outside [0, area]", i, j);
        if (!(o[5] >= 0.0)) fail(name, "Gamma < 0", i, j);
        if ((int)o[0] != (int)o1[0] || std::fabs(o[1] - o1[1]) > 1e-12 * area) fail(name, "1 lane and 16 lanes disagree", i, j);
        if (((poly_type(h, lo, hi) & 255) == 255 ? -1 : (poly_type(h, lo, hi) & 255)) != (int)o[0])
          fail(name, "pick_ball and box_measure disagree on the type", i, j);
        for (int d = 0; d < 2; ++d) {
          const double ext = hi[1 - d] - lo[1 - d];
          const double a = poly_section_c(h, d, lo[d], lo, hi, -1.0), b = poly_section_c(h, d, o[2 + d], lo, hi, -1.0);
          if (!(a >= 0.0 && a <= ext && b >= 0.0 && b <= ext)) fail(name, "a section outside [0, extent]", i, j);
        }
        if (i > 0) {                                              // the staggered box between two centres
          const double slo[3] = {0.5 * (nx[i - 1] + nx[i]), ny[j], 0.0}, shi[3] = {0.5 * (nx[i] + nx[i + 1]), ny[j + 1], 0.0};
          poly_box(h, slo, shi, 0, 16, o1);
          if (!(o1[1] >= 0.0 && o1[1] <= area * (1.0 + 1e-12))) fail(name, "W outside [0, area]", i, j);
        }
        total += o[1];
        ++g_checked;
      }
    std::printf("%s (complement %d): sum V = %.15g\n", name, comp, total);
    poly_free(h);
  }
}
}  // namespace

int main() {
  const double pi = 3.14159265358979323846;
  std::vector<double> circle;
  for (int i = 0; i < 2000; ++i) {
    const double a = 2.0 * pi * ((double)i / 2000);
    circle.push_back(2.01 + std::cos(a));
    circle.push_back(2.01 + std::sin(a));
  }
  sweep("fine_circle_8", circle, 8, 8, 0.0, 4.0);
  const std::vector<double> square = {1.0, 1.0, 3.0, 1.0, 3.0, 3.0, 1.0, 3.0};
  sweep("aligned_square_16", square, 16, 16, 0.0, 4.0);
  std::vector<double> outside = circle;                       // markers beyond the mesh on every side
  for (double& v : outside) v = 2.0 * v - 2.0;
  sweep("circle larger than the mesh", outside, 7, 5, 0.0, 4.0);
  std::printf("polygon_host: %d boxes checked\n", g_checked);
  return 0;
}
#endif
