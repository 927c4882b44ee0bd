// Host test of the marching-unit planner's EDGE ROWS (pg_host_algos.h plan_march_units with an EdgePlan; pg_spmv.hip "edge
// rows").  A stand-alone program, built and run by tests/test_march_edge_rows_host.py -- plain, and once with
// -fsanitize=address,undefined:
//     g++ -std=c++17 -O1 -ffp-contract=off tests/march_host.cpp -o march_host && ./march_host
// A compact cut-cell numbering is synthesised (a 3-D ball of chords on 24^3, a 2-D disc on 48^2): cells with all their
// neighbours form the runs of one stencil, every other cell is an irregular row whose entries are its existing neighbours, in
// the slot order of the assembled rows, with values of its own.  The planner's records are then EXECUTED the way the kernel
// executes them -- window positions, lines, lateral lines, the value stream of the edge rows -- on a vector with the 8
// elements of slack the device vectors have (NaN there: nothing initialises them on the device, and an absent slot of an edge
// row is still multiplied, +0.0 times the element it points to), every index checked, and compared with the rows applied one
// by one.
// The line with a gap (a cell taken out of a chord): the two cells at the gap are consecutive rows, but the lateral and plane
// offsets of the rows behind the gap are one more than those of the rows before it.  So no unit may carry a row across the
// gap -- the row behind it can only be a LOW-end edge row of the run that follows, the row before it only a HIGH-end edge row
// of the run that precedes -- and that, not fallback membership, is what the case asserts: either row computes correctly
// from the lines of its own side.
// Prints one line of counts per case; exit code = number of failed checks.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../penguin/jl_amd/csrc/pg_host_algos.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++g_fail <= 20) {                                \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);                      \
        fprintf(stderr, "\n");                             \
      }                                                    \
    }                                                      \
  } while (0)

using pghost::MRun;
constexpr int INFO = 24;

struct Problem {
  int64_t n = 0;
  int cnt = 7;
  std::vector<MRun> runs;
  std::vector<int> info;
  // every row as CSR (the reference), and the irregular rows as the planner's candidates
  std::vector<int> rowptr, col;
  std::vector<double> val;
  std::vector<int> c_rows, c_ptr, c_col;
  std::vector<char> in_run;
  std::vector<int> id;   // cell -> row or -1
  int nx = 0, ny = 0;
  int row_of(int i, int j, int k) const { return id[(size_t)i + (size_t)nx * (j + (size_t)ny * k)]; }
};

static double coef(int e, int cnt) { return e + 1 == cnt ? 1.0 : -0.1 - 0.01 * e; }

// active(i, j, k) cells of an nx x ny x nz box, numbered x fastest; hole: one cell taken out (a line with a gap)
template <class F>
static Problem synth(int nx, int ny, int nz, F active, std::mt19937_64& rng) {
  Problem P;
  const bool two_d = nz == 1;
  P.cnt = two_d ? 5 : 7;
  std::vector<int> id((size_t)nx * ny * nz, -1);
  auto at = [&](int i, int j, int k) -> int& { return id[(size_t)i + (size_t)nx * (j + (size_t)ny * k)]; };
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i)
        if (active(i, j, k)) at(i, j, k) = (int)P.n++;
  auto nb = [&](int a, int b, int c) { return (a < 0 || b < 0 || c < 0 || a >= nx || b >= ny || c >= nz) ? -1 : at(a, b, c); };
  std::uniform_real_distribution<double> V(-1.0, 1.0);
  P.rowptr.push_back(0);
  P.in_run.assign(P.n, 0);
  const int m = P.cnt - 1;
  std::vector<std::vector<int>> offs(P.n);
  std::vector<char> full(P.n, 0);
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) {
        const int r = at(i, j, k);
        if (r < 0) continue;
        const int q[6] = {nb(i + 1, j, k), nb(i - 1, j, k), nb(i, j + 1, k), nb(i, j - 1, k), nb(i, j, k + 1), nb(i, j, k - 1)};
        bool all = true;
        for (int e = 0; e < m; ++e) {
          all = all && q[e] >= 0;
          offs[r].push_back(q[e] >= 0 ? q[e] - r : 0x7fffffff);
        }
        offs[r].push_back(0);
        full[r] = all;
      }
  // runs: >= 3 consecutive full rows with the same offsets (consecutive rows of one line)
  for (int64_t r = 0; r < P.n;) {
    int64_t e = r + 1;
    if (full[r])
      while (e < P.n && full[e] && offs[e] == offs[r]) ++e;
    if (full[r] && e - r >= 3) {
      P.runs.push_back(MRun{(int)r, (int)(e - r), P.cnt});
      for (int s = 0; s < 8; ++s) P.info.push_back(s < P.cnt ? offs[r][s] : 0);
      for (int s = 0; s < 8; ++s) {
        const double v = s < P.cnt ? coef(s, P.cnt) : 0.0;
        int w[2];
        std::memcpy(w, &v, 8);
        P.info.push_back(w[0]);
        P.info.push_back(w[1]);
      }
      for (int64_t q = r; q < e; ++q) P.in_run[q] = 1;
    }
    r = e;
  }
  for (int64_t r = 0; r < P.n; ++r) {
    for (int s = 0; s < P.cnt; ++s) {
      if (offs[r][s] == 0x7fffffff) continue;
      P.col.push_back((int)r + offs[r][s]);
      P.val.push_back(P.in_run[r] ? coef(s, P.cnt) : V(rng));
    }
    P.rowptr.push_back((int)P.col.size());
  }
  P.id = id;
  P.nx = nx;
  P.ny = ny;
  return P;
}

// one more entry in row r (a coupling no stencil slot has): the row cannot ride with a unit
static void add_entry(Problem& P, int r, int c, double v) {
  const int at = P.rowptr[r + 1];
  P.col.insert(P.col.begin() + at, c);
  P.val.insert(P.val.begin() + at, v);
  for (size_t q = r + 1; q < P.rowptr.size(); ++q) ++P.rowptr[q];
}

static void candidates(Problem& P) {
  P.c_rows.clear(); P.c_col.clear();
  P.c_ptr.assign(1, 0);
  for (int64_t r = 0; r < P.n; ++r) {
    if (P.in_run[r]) continue;
    P.c_rows.push_back((int)r);
    for (int k = P.rowptr[r]; k < P.rowptr[r + 1]; ++k) P.c_col.push_back(P.col[k]);
    P.c_ptr.push_back((int)P.c_col.size());
  }
}

static double dword_pair(const int* w) {
  double c;
  std::memcpy(&c, w, 8);
  return c;
}

struct Counts { int64_t rows, marched, edge, fallback, units; std::vector<char> taken, side; };   // side: 1 below lo, 2 above hi

// plans, checks and executes; must_stay: rows that have to end up outside the units
static Counts run_case(const char* name, Problem& P, const pghost::MarchGeometry& geo, const std::vector<int>& must_stay,
                       std::mt19937_64& rng) {
  candidates(P);
  pghost::EdgePlan ep;
  ep.cand = pghost::EdgeCands{P.c_rows.data(), (int64_t)P.c_rows.size(), P.c_ptr.data(), P.c_col.data()};
  std::vector<int> mrec;
  std::vector<pghost::RowRange> fb;
  int64_t rows_m = 0;
  pghost::plan_march_units(P.n, P.runs, P.info, geo, mrec, fb, rows_m, nullptr, &ep);
  const int64_t nunits = (int64_t)mrec.size() / geo.REC, ne = ep.rows_e;
  CHECK((int64_t)ep.meta.size() == 4 * ne, "%s: meta holds %zu ints for %lld edge rows", name, ep.meta.size(), (long long)ne);
  // the value stream, filled as k_fill_edges fills it
  std::vector<double> ev((size_t)pghost::EDGE_SLOTS * ne + 8, -7.0);   // (-7: a slot nobody wrote would show in y)
  for (int64_t q = 0; q < ne; ++q) {
    const int r = ep.meta[4 * q], dst = ep.meta[4 * q + 1], dist = ep.meta[4 * q + 2], sm = ep.meta[4 * q + 3];
    const int a = P.rowptr[r], len = sm >> 24;
    CHECK(len == P.rowptr[r + 1] - a, "%s: edge row %d: %d entries mapped, %d stored", name, r, len, P.rowptr[r + 1] - a);
    for (int j = 0; j < pghost::EDGE_SLOTS; ++j) {
      const int64_t at = dst + (int64_t)(j >> 1) * dist + (j & 1);
      CHECK(at >= 0 && at < (int64_t)pghost::EDGE_SLOTS * ne, "%s: slot outside the stream", name);
      if (at >= 0 && at < (int64_t)ev.size()) ev[at] = 0.0;
    }
    for (int k = 0; k < len; ++k) {
      const int j = (sm >> (3 * k)) & 7;
      CHECK(j < P.cnt && (k == 0 || j > ((sm >> (3 * (k - 1))) & 7)), "%s: edge row %d: slots not ascending", name, r);
      ev[dst + (int64_t)(j >> 1) * dist + (j & 1)] = P.val[a + k];
    }
  }
  // execute the units
  std::vector<double> x(P.n + 8), y(P.n, 0.0), yref(P.n, 0.0);
  std::vector<int> covered(P.n, 0);
  std::uniform_real_distribution<double> V(-1.0, 1.0);
  for (auto& v : x) v = V(rng);
  for (int q = 0; q < 8; ++q) x[P.n + q] = std::nan("");
  std::vector<char> side(P.n, 0);
  for (int64_t r = 0; r < P.n; ++r) {
    double acc = 0.0;
    for (int k = P.rowptr[r]; k < P.rowptr[r + 1]; ++k) acc += P.val[k] * x[P.col[k]];
    yref[r] = acc;
  }
  auto xat = [&](int64_t idx) {
    CHECK(idx >= 0 && idx < P.n + 8, "%s: x index %lld outside the vector", name, (long long)idx);
    return (idx >= 0 && idx < P.n + 8) ? x[idx] : 0.0;
  };
  int64_t marched = 0, edge = 0, stream_next = 0;
  const int cnt = P.cnt;
  const bool Y = cnt == 7;
  for (int64_t u = 0; u < nunits; ++u) {
    const int* rec = mrec.data() + geo.REC * u;
    const int K = rec[0] & 255, lanes = rec[0] >> 16;
    CHECK(((rec[0] >> 8) & 255) == cnt && (K == geo.K || K == geo.KS), "%s: unit header", name);
    const int first = rec[pghost::EDGE_REC], ne_u = rec[pghost::EDGE_REC + 1];
    CHECK(first == stream_next && ne_u >= 0 && ne_u <= pghost::EDGE_PER_UNIT, "%s: unit %lld: edge rows %d from %d (expected %lld)", name,
          (long long)u, ne_u, first, (long long)stream_next);
    stream_next += ne_u;
    int seen = 0;
    for (int i = 0; i < K; ++i) {
      const int rb = rec[18 + 4 * i], lo = rec[21 + 4 * i] & 255, hi = rec[21 + 4 * i] >> 8;
      const int below = i == 0 ? rec[16] : rec[18 + 4 * (i - 1)], above = i == K - 1 ? rec[17] : rec[18 + 4 * (i + 1)];
      const int ei = rec[pghost::EDGE_REC + 2 + i], nlo = ei & 255, nhi = (ei >> 8) & 255, eoff = ei >> 16;
      CHECK(nlo <= pghost::EDGE_PER_END && nhi <= pghost::EDGE_PER_END, "%s: %d / %d edge rows at the ends of a plane", name, nlo, nhi);
      CHECK(eoff == seen, "%s: plane %d starts at edge row %d of its unit, %d counted", name, i, eoff, seen);
      CHECK(lo - nlo >= 1 && hi + nhi <= 127, "%s: rows [%d, %d) outside window positions 1..126", name, lo - nlo, hi + nhi);
      CHECK(hi + nhi <= lo || (hi + nhi) / 2 + 1 <= lanes || lanes == 64, "%s: row %d beyond the unit's %d active lanes", name, hi + nhi - 1, lanes);
      if (hi <= lo) CHECK(nlo == 0 && nhi == 0, "%s: edge rows on a plane without marched rows", name);
      for (int p = lo - nlo; p < hi + nhi; ++p) {
        const int r = rb + p;
        const bool is_edge = p < lo || p >= hi;
        const int e = p < lo ? eoff + (p - (lo - nlo)) : eoff + nlo + (p - hi);
        if (is_edge) CHECK(first + e < ne && ep.meta[4 * (size_t)(first + e)] == r, "%s: edge row %d of unit %lld is not row %d", name, e, (long long)u, r);
        double op[7];
        int j = 0;
        op[j++] = xat((int64_t)rb + p + 1);
        op[j++] = xat((int64_t)rb + p - 1);
        if (Y) {
          op[j++] = xat((int64_t)rb + rec[20 + 4 * i] + p);
          op[j++] = xat((int64_t)rb + rec[19 + 4 * i] + p);
        }
        op[j++] = xat((int64_t)above + p);
        op[j++] = xat((int64_t)below + p);
        op[j++] = xat((int64_t)rb + p);
        double acc = 0.0;
        for (int s = 0; s < cnt; ++s) {
          const double c = is_edge ? ev[(size_t)pghost::EDGE_SLOTS * first + 2 * ((size_t)(s >> 1) * ne_u + e) + (s & 1)] : dword_pair(rec + 2 + 2 * s);
          acc += c * op[s];
        }
        if (r >= 0 && r < P.n) {
          y[r] = acc;
          ++covered[r];
          if (is_edge) side[r] = p < lo ? 1 : 2;
          CHECK(is_edge != (bool)P.in_run[r], "%s: row %d: %s", name, r, is_edge ? "edge row out of a run" : "marched row outside the runs");
        } else {
          CHECK(false, "%s: computed row %d outside the matrix", name, r);
        }
        (is_edge ? edge : marched) += 1;
      }
      seen += nlo + nhi;
    }
    CHECK(seen == ne_u, "%s: unit %lld: %d edge rows on its planes, %d in its header", name, (long long)u, seen, ne_u);
  }
  CHECK(marched == rows_m && edge == ne && stream_next == ne, "%s: %lld marched (%lld planned), %lld edge (%lld planned)", name,
        (long long)marched, (long long)rows_m, (long long)edge, (long long)ne);
  // fallback: the ranges the planner returns, and the candidates it did not take -- every row exactly once
  int64_t fallback = 0;
  for (const auto& f : fb)
    for (int64_t r = f.a; r < f.b; ++r) { ++covered[r]; ++fallback; y[r] = yref[r]; }
  std::vector<char> taken(P.n, 0);
  for (int64_t q = 0; q < ne; ++q) taken[ep.meta[4 * q]] = 1;
  for (int r : P.c_rows)
    if (!taken[r]) { ++covered[r]; ++fallback; y[r] = yref[r]; }
  for (int64_t r = 0; r < P.n; ++r) {
    CHECK(covered[r] == 1, "%s: row %lld covered %d times", name, (long long)r, covered[r]);
    CHECK(y[r] == yref[r], "%s: row %lld: %.17g from the units, %.17g row by row", name, (long long)r, y[r], yref[r]);
  }
  for (int r : must_stay) CHECK(!taken[r] && !P.in_run[r], "%s: row %d rides with a unit", name, r);
  printf("%s rows %lld marched %lld edge %lld fallback %lld units %lld\n", name, (long long)P.n, (long long)marched, (long long)edge,
         (long long)fallback, (long long)nunits);
  return Counts{P.n, marched, edge, fallback, nunits, taken, side};
}

int main() {
  std::mt19937_64 rng(20241);
  const pghost::MarchGeometry geo{4, 2, 64, 126, INFO, 4};
  {   // 3-D ball of chords on 24^3
    auto ball = [](int i, int j, int k) {
      const double dx = i + 0.5 - 12.2, dy = j + 0.5 - 11.9, dz = k + 0.5 - 12.1;
      return dx * dx + dy * dy + dz * dz < 10.6 * 10.6;
    };
    Problem P = synth(24, 24, 24, ball, rng);
    const Counts c = run_case("ball24", P, geo, {}, rng);
    CHECK(c.edge > 0 && c.marched > 0 && c.units > 0, "ball24: nothing planned");
    // a row with an eighth entry next to a run, and the row behind it (which alone would qualify): the edge rows of a plane
    // are consecutive from the marched rows outwards, so both stay where they are
    int stuck = -1;
    for (const MRun& r : P.runs) {
      const int a = r.r0 + r.len;   // first row after the run
      if (a + 1 < P.n && c.taken[a] && c.taken[a + 1]) {   // both ride with the run's units as things are
        stuck = a;
        break;
      }
    }
    CHECK(stuck >= 0, "ball24: no run with two edge rows behind it");
    if (stuck >= 0) {
      add_entry(P, stuck, stuck >= 40 ? stuck - 37 : stuck + 37, 0.25);
      const Counts d = run_case("ball24+entry", P, geo, {stuck, stuck + 1}, rng);
      CHECK(d.edge < c.edge, "ball24+entry: %lld edge rows, %lld without the extra entry", (long long)d.edge, (long long)c.edge);
    }
  }
  {   // the same ball with a cell taken out of a chord: a line with a gap -- two runs on it, the cells at the gap irregular
    auto holed = [](int i, int j, int k) {
      const double dx = i + 0.5 - 12.2, dy = j + 0.5 - 11.9, dz = k + 0.5 - 12.1;
      return dx * dx + dy * dy + dz * dz < 10.6 * 10.6 && !(i == 12 && j == 12 && k == 12);
    };
    Problem P = synth(24, 24, 24, holed, rng);
    const Counts c = run_case("ball24+gap", P, geo, {}, rng);
    CHECK(c.edge > 0, "ball24+gap: no edge rows");
    const int before = P.row_of(11, 12, 12), behind = P.row_of(13, 12, 12);
    CHECK(before >= 0 && behind == before + 1 && !P.in_run[before] && !P.in_run[behind], "ball24+gap: rows at the gap %d, %d", before, behind);
    CHECK(P.in_run[before - 1] && P.in_run[behind + 1], "ball24+gap: no runs on both sides of the gap");
    // no unit reaches across the gap
    CHECK(!c.taken[before] || c.side[before] == 2, "ball24+gap: the row before the gap rides with the run behind it");
    CHECK(!c.taken[behind] || c.side[behind] == 1, "ball24+gap: the row behind the gap rides with the run before it");
    CHECK(c.taken[before] || c.taken[behind], "ball24+gap: neither row at the gap is an edge row");
  }
  {   // a strip of 20 lines of 130 cells whose LAST line is 4 cells shorter: the window over the last full line ends one element
      // behind the vector (the loads are allowed 8 of slack), and the cells of that line that stick out have no neighbour above
      // -- the slot of that neighbour points behind the vector (NaN in this test), so they must stay out of the unit
    auto strip = [](int i, int j, int) { return j < 19 || i < 126; };
    Problem P = synth(130, 20, 1, strip, rng);
    const Counts c = run_case("strip130", P, geo, {}, rng);
    CHECK(c.edge > 0 && c.marched > 0, "strip130: nothing planned");
    const int out = P.row_of(126, 18, 0);
    CHECK(out >= 0 && P.in_run[out - 1] && !P.in_run[out] && out + P.info[INFO * (P.runs.size() - 1) + 2] >= P.n,
          "strip130: row %d does not point behind the vector", out);
    CHECK(!c.taken[out], "strip130: row %d multiplies an element behind the vector", out);
  }
  {   // 2-D disc on 48^2 (5-point units)
    auto disc = [](int i, int j, int) {
      const double dx = i + 0.5 - 24.3, dy = j + 0.5 - 23.8;
      return dx * dx + dy * dy < 21.4 * 21.4;
    };
    Problem P = synth(48, 48, 1, disc, rng);
    const Counts c = run_case("disc48", P, geo, {}, rng);
    CHECK(c.edge > 0 && c.marched > 0, "disc48: nothing planned");
  }
  {   // units of one plane (kmax = 1) and no candidates at all: the records carry no edge rows
    auto ball = [](int i, int j, int k) {
      const double dx = i + 0.5 - 12.0, dy = j + 0.5 - 12.0, dz = k + 0.5 - 12.0;
      return dx * dx + dy * dy + dz * dz < 9.7 * 9.7;
    };
    Problem P = synth(24, 24, 24, ball, rng);
    const pghost::MarchGeometry g1{4, 2, 64, 126, INFO, 1};
    run_case("ball24 kmax 1", P, g1, {}, rng);
  }
  if (g_fail) fprintf(stderr, "%d check(s) failed\n", g_fail);
  return g_fail > 255 ? 255 : g_fail;
}
