// pg_host_algos.h -- the pure HOST algorithms of the library, free of HIP so that the CPU test-suite can compile them with
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/host_asan.cpp): the slab partition of the
// planes and the planning of the SpMV's marching units (index arithmetic over run descriptors: the place where an
// off-by-one reads outside a vector on the GPU), the host side of the multigrid set-up (tests/mg_host_asan.cpp) and the
// eigenvalues of the spectral estimate's Hessenberg matrix (tests/specest_host.cpp), and the one-thread scalar steps of BiCGStab(l),
// IDR(s) and GMRES, compiled for the device too (tests/bicgstabl_host.cpp, idrs_host.cpp, gmres_host.cpp).  Included by pg_context.hip, pg_spmv.hip,
// pg_multigrid.hip and pg_specest.hip.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace pghost {

// contiguous plane ranges whose cumulated weight is closest to r / nranks of the total; every rank gets at least one
// plane (+1 per plane so that empty regions are still spread).  bounds: nranks + 1 entries.  nplanes >= nranks >= 1.
inline void partition_planes(const int64_t* weight, int64_t nplanes, int nranks, int64_t* bounds) {
  std::vector<double> cum(nplanes + 1, 0.0);
  for (int64_t k = 0; k < nplanes; ++k) cum[k + 1] = cum[k] + static_cast<double>(weight[k]) + 1.0;
  const double total = cum[nplanes];
  bounds[0] = 0;
  for (int r = 1; r < nranks; ++r) {
    const double target = total * r / nranks;
    int64_t k = std::lower_bound(cum.begin(), cum.end(), target) - cum.begin();
    if (k > 0 && (target - cum[k - 1]) < (cum[k] - target)) --k;
    const int64_t lo = bounds[r - 1] + 1;
    const int64_t hi = nplanes - (nranks - r);
    bounds[r] = std::min(std::max(k, lo), hi);
  }
  bounds[nranks] = nplanes;
}

// ---- local numbering of one slab (K10, the layout pg_comm.hip's halo exchange rests on) -----------------------------
// Local vector layout: [kind 0 owned | kind 1 owned | ... | lower ghosts: kind 0, kind 1, ... | upper ghosts: kind 0, ...].
// Owned unknowns of a kind are ordered by padded cell index, so the actives of the first / last owned plane are the
// contiguous chunks at the start / end of each kind's segment: they are what goes to the lower / upper neighbour, and what
// arrives from a neighbour lands in one contiguous ghost segment per kind -- no pack / unpack kernels.
// Inputs per kind k: the number of active unknowns of the stored planes that lie BEFORE the first owned plane (posO), before
// the end of the last owned plane (posU), before the end of the first owned plane (posFE), before the start of the last
// owned plane (posLB), and in all stored planes (tot); actives outside the one ghost plane each side do not exist (their
// flags are cleared before the count).  build_numbering (device scans) and pg_slab_numbering_host (CPU prefix sums: the
// gloo test of the CPU suite) both end here.
constexpr int SLAB_MAX_KINDS = 4;
struct SlabNumbering {
  int K = 0;
  int64_t n_own = 0, n_ghost = 0;
  int64_t cnt_own[SLAB_MAX_KINDS], off_own[SLAB_MAX_KINDS], cntL[SLAB_MAX_KINDS], offL[SLAB_MAX_KINDS], cntU[SLAB_MAX_KINDS],
      offU[SLAB_MAX_KINDS], sendL_off[SLAB_MAX_KINDS], sendL_cnt[SLAB_MAX_KINDS], sendU_off[SLAB_MAX_KINDS], sendU_cnt[SLAB_MAX_KINDS];
};
inline void slab_numbering(int K, const int64_t* posO, const int64_t* posU, const int64_t* posFE, const int64_t* posLB,
                           const int64_t* tot, bool has_lower, bool has_upper, SlabNumbering& out) {
  out.K = K;
  int64_t off = 0;
  for (int k = 0; k < K; ++k) {
    out.cntL[k] = posO[k];
    out.cnt_own[k] = posU[k] - posO[k];
    out.cntU[k] = tot[k] - posU[k];
    out.off_own[k] = off;
    off += out.cnt_own[k];
  }
  out.n_own = off;
  for (int k = 0; k < K; ++k) { out.offL[k] = off; off += out.cntL[k]; }
  for (int k = 0; k < K; ++k) { out.offU[k] = off; off += out.cntU[k]; }
  out.n_ghost = off - out.n_own;
  for (int k = 0; k < K; ++k) {
    // owned actives of the first owned plane go to the lower neighbour, of the last to the upper one
    out.sendL_off[k] = out.off_own[k];
    out.sendL_cnt[k] = has_lower ? posFE[k] - posO[k] : 0;
    out.sendU_cnt[k] = has_upper ? posU[k] - posLB[k] : 0;
    out.sendU_off[k] = out.off_own[k] + out.cnt_own[k] - out.sendU_cnt[k];
  }
  for (int k = K; k < SLAB_MAX_KINDS; ++k)
    out.cnt_own[k] = out.off_own[k] = out.cntL[k] = out.offL[k] = out.cntU[k] = out.offU[k] = out.sendL_off[k] = out.sendL_cnt[k] =
        out.sendU_off[k] = out.sendU_cnt[k] = 0;
}

// stored / exact-flag plane ranges of a slab that owns planes [p0, p1): stored = [p0 - halo, p1 + halo) clipped, flags are
// exact on [p0 - 1, p1 + 1) clipped (one ghost plane each side)
struct SlabPlanes { int64_t s0, s1, a0, a1; };
inline SlabPlanes slab_planes(int64_t p0, int64_t p1, int64_t nplanes, int halo) {
  SlabPlanes g;
  g.s0 = p0 - halo < 0 ? 0 : p0 - halo;
  g.s1 = p1 + halo > nplanes ? nplanes : p1 + halo;
  g.a0 = p0 - 1 < 0 ? 0 : p0 - 1;
  g.a1 = p1 + 1 > nplanes ? nplanes : p1 + 1;
  return g;
}

struct MRun {
  int r0, len, cnt;   // rows [r0, r0 + len) with one stencil (offsets and values), cnt = 5 / 7 entries
};
struct RowRange {
  int64_t a, b;       // rows [a, b) that cannot march: they go back to the U slices
  int cnt;
};
struct MarchGeometry {
  int K, KS;          // planes per full / short unit (shorter units are closed with empty planes)
  int REC;            // dwords per unit record
  int W;              // rows computed per window (the window holds W + 2 elements of every line)
  int INFO;           // dwords per run descriptor: 8 offsets, 8 values (lo, hi)
  int kmax;           // planes per unit actually used (<= K)
  // optional grid geometry (3-D units only): dword 24 of a run descriptor is then the grid cell of the run's first row,
  // cell = (plane * lines + line) * ext0 + i, and the units are ordered strip by strip (see below)
  int64_t ext0 = 0, lines = 0;
  int strip = 0;      // lateral lines per strip (0: order by first row)
  // 1 (needs the grid geometry): units are cut at COMMON planes (every unit starts at a multiple of kmax or at the start of
  // its chain) and ordered window-major inside a (strip, plane group): the four waves of a block then hold four
  // neighbouring lines of one window over the same planes, and a unit's lateral lines are its block mates' own lines
  int unit_order = 0;
};

// Edge rows (pg_spmv.hip "edge rows"): irregular rows that sit next to the marched rows of a plane, on the same line of
// consecutive row numbers, and couple to the same neighbours -- the cells at the ends of a chord, whose values differ from
// the interior's and whose missing neighbours are missing entries.  A unit computes them from the lines it holds, with
// per-row values from a stream of their own.  cand: the rows that may become edge rows (the irregular rows), as a compact CSR.
struct EdgeCands {
  const int* rows = nullptr;     // row numbers, ascending
  int64_t nrows = 0;
  const int* rowptr = nullptr;   // nrows + 1: the entries of candidate q are [rowptr[q], rowptr[q + 1])
  const int* col = nullptr;
};
constexpr int EDGE_SLOTS = 8;      // value slots per edge row in the stream: the 7 of the stencil (5 in 2-D) and padding to 64 bytes
constexpr int EDGE_PER_END = 8;    // edge rows at one end of a plane
constexpr int EDGE_PER_UNIT = 64;  // ... of a unit: one lane each
constexpr int EDGE_REC = 34;       // unit record: dword 34 = first edge row of the unit in the stream, 35 = edge rows of the
                                   // unit, 36 + i = plane i: rows at the low end | at the high end << 8 | first edge row of the
                                   // plane, counted from the unit's first << 16
struct EdgePlan {
  EdgeCands cand;
  // out, 4 ints per edge row in stream order: row; index of its slot 0 in the value stream; distance between two of its
  // PAIRS of slots (the rows of a unit are stored pair-major: slots 2p, 2p + 1 of the unit's e-th row at
  // 8 first + 2 (p rows_of_unit + e)); slot of the stored entry k in bits 3k..3k+2 | entries << 24
  std::vector<int> meta;
  int64_t rows_e = 0;
  int64_t slots_read = 0;   // value slots the units read for them (the stencil's entries per row)
};

// place of a grid cell in the order of the work items: strip of lateral lines, then plane; ties by row number
inline int64_t march_order(int64_t cell, int64_t ext0, int64_t lines, int strip) {
  const int64_t line = (cell / ext0) % lines, plane = cell / (ext0 * lines);
  return (line / strip) * ((int64_t)1 << 20) + plane;
}

// Chains of runs that face each other across the slowest stencil direction (entry cnt-3 / cnt-2 of a row lead to the row of
// the same lateral position one plane up / down), cut into windows of W computed rows and units of <= kmax planes
// (pg_spmv.hip "marching units" has the record layout).  info: INFO dwords per run -- the col - row offsets (8) and the
// values (8 doubles as lo / hi dwords) of the run's first row, in the entry order of the assembled rows:
// +1, -1, [+Y, -Y,] +Z, -Z, 0.  n = rows of the matrix (= guaranteed length of every vector the kernel reads).
// mrec: the unit records, sorted by first row -- or, when the grid geometry is known, 3-D units strip by strip: all planes
// of `strip` neighbouring lateral lines before the next strip.  A unit reads the line below its first and above its last
// plane (6 lines of the chain for 4 computed ones); in first-row order a plane of units lies between a unit and the unit
// above it in the chain, which is more than an XCD's L2 holds at 512^3 (PMC: x crossed the fabric 1.54 times per launch),
// in strip order it is strip x windows units.  fallback: rows that cannot march (another entry order, windows that would read
// outside the vector); rows_m: rows covered by units.
inline void plan_march_units(int64_t n, const std::vector<MRun>& runs, const std::vector<int>& info, const MarchGeometry& geo,
                             std::vector<int>& mrec, std::vector<RowRange>& fallback, int64_t& rows_m,
                             std::vector<int64_t>* okeys = nullptr, EdgePlan* edges = nullptr) {
  typedef int64_t i64;
  rows_m = 0;
  const i64 nr = (i64)runs.size();
  const int RI = geo.INFO;
  auto off = [&](i64 i, int k) { return info[RI * i + k]; };
  auto same_values = [&](i64 i, i64 j, int cnt) {
    for (int k = 0; k < 2 * cnt; ++k)
      if (info[RI * i + 8 + k] != info[RI * j + 8 + k]) return false;
    return true;
  };
  // entries of a marching row, in the order eval_row emits them: +1, -1, [+Y, -Y,] +Z, -Z, 0 with 1 < Y < Z
  std::vector<char> ok(nr, 0);
  for (i64 i = 0; i < nr; ++i) {
    const int cnt = runs[i].cnt;
    bool good = (cnt == 5 || cnt == 7) && off(i, 0) == 1 && off(i, 1) == -1 && off(i, cnt - 1) == 0;
    if (good) {
      const int up_e = cnt - 3, dn_e = cnt - 2;
      good = off(i, up_e) > 1 && off(i, dn_e) < -1;
      if (good && cnt == 7) good = off(i, 2) > 1 && off(i, 2) < off(i, up_e) && off(i, 3) < -1 && off(i, 3) > off(i, dn_e);
    }
    ok[i] = good;
    if (!ok[i]) fallback.push_back(RowRange{runs[i].r0, (i64)runs[i].r0 + runs[i].len, cnt});
  }
  // successor of run i: the run that holds most of the rows r + o[up], r in run i, if it mirrors the offset and carries
  // the same values; every run has at most one predecessor
  std::vector<int> succ(nr, -1), pred(nr, -1);
  for (i64 i = 0; i < nr; ++i) {
    if (!ok[i]) continue;
    const int cnt = runs[i].cnt, up_off = off(i, cnt - 3);
    const i64 lo = (i64)runs[i].r0 + up_off, hi = lo + runs[i].len;
    i64 j = std::upper_bound(runs.begin(), runs.end(), lo, [](i64 v, const MRun& r) { return v < (i64)r.r0; }) - runs.begin();
    if (j > 0) --j;
    i64 best = -1, best_ov = 0;
    for (; j < nr && (i64)runs[j].r0 < hi; ++j) {
      const i64 a = runs[j].r0, b = a + runs[j].len;
      if (b <= lo || j == i || !ok[j] || pred[j] >= 0 || runs[j].cnt != cnt || off(j, cnt - 2) != -up_off || !same_values(i, j, cnt)) continue;
      const i64 ov = std::min(hi, b) - std::max(lo, a);
      if (ov > best_ov) { best_ov = ov; best = j; }
    }
    if (best >= 0) { succ[i] = (int)best; pred[best] = (int)i; }
  }
  struct Unit { int key; int64_t order; int64_t sub; std::vector<int> rec; std::vector<int> erows; };   // erows: (row, slots) pairs
  // edge rows: candidate `row` against the stencil of run `run` -- its entries, in stored order, must be a subsequence of the
  // run's entries with the same col - row offsets (and no ghost column); smap: slot per entry (EdgePlan::meta)
  const bool want_edges = edges && edges->cand.nrows > 0 && geo.REC >= EDGE_REC + 2 + geo.K;
  std::vector<char> claimed(want_edges ? (size_t)edges->cand.nrows : 0, 0);
  auto edge_row = [&](i64 row, i64 run, int cnt, int& smap, i64& q) {
    const EdgeCands& c = edges->cand;
    if (row < 0 || row >= n) return false;
    q = std::lower_bound(c.rows, c.rows + c.nrows, (int)row) - c.rows;
    if (q >= c.nrows || c.rows[q] != row || claimed[q]) return false;
    const int a = c.rowptr[q], len = c.rowptr[q + 1] - a;
    if (len < 1 || len > cnt) return false;
    // a slot the row has no entry for is still multiplied, +0.0 times the element the slot points to: that element must be
    // one of the matrix' own unknowns too (finite), not the slack behind the vector or a ghost that has not arrived
    auto inside = [&](int s) { const i64 t = row + off(run, s); return t >= 0 && t < n; };
    int sl = 0;
    smap = len << 24;
    for (int e = 0; e < len; ++e) {
      const i64 cc = c.col[a + e];
      if (cc < 0 || cc >= n) return false;
      while (sl < cnt && off(run, sl) != cc - row) {
        if (!inside(sl)) return false;
        ++sl;
      }
      if (sl == cnt) return false;
      smap |= sl << (3 * e);
      ++sl;
    }
    for (; sl < cnt; ++sl)
      if (!inside(sl)) return false;
    return true;
  };
  const bool aligned = geo.unit_order == 1 && geo.strip > 0 && geo.ext0 > 0 && geo.lines > 0 && RI > 24;
  // absolute plane of a run (-1: unknown)
  auto plane_of = [&](i64 run) -> i64 {
    const i64 cell = info[RI * run + 24];
    return cell >= 0 ? cell / (geo.ext0 * geo.lines) : -1;
  };
  std::vector<Unit> units;
  // every load of a unit reads elements idx0 .. idx0 + 129 of a vector of >= n elements (+ 8 of slack, DevBuf)
  auto safe = [&](i64 idx0) { return idx0 >= 0 && idx0 + 130 <= n + 8; };
  std::vector<i64> chain, B;
  for (i64 h = 0; h < nr; ++h) {
    if (!ok[h] || pred[h] >= 0) continue;
    chain.clear(); B.clear();
    const int cnt = runs[h].cnt;
    const bool Y = cnt == 7;
    const int up_e = cnt - 3, dn_e = cnt - 2;   // entries of the +plane / -plane taps
    i64 base = runs[h].r0;
    for (i64 i = h; i >= 0; i = succ[i]) {
      chain.push_back(i);
      B.push_back(base);
      base += off(i, up_e);
    }
    const i64 L = (i64)chain.size();
    i64 cmin = 0, cmax = 0;
    for (i64 k = 0; k < L; ++k) {
      const i64 a = runs[chain[k]].r0 - B[k], b = a + runs[chain[k]].len;
      cmin = k == 0 ? a : std::min(cmin, a);
      cmax = k == 0 ? b : std::max(cmax, b);
    }
    for (i64 W = cmin - 1; W + 1 < cmax; W += geo.W) {
      auto range = [&](i64 k, i64& lo, i64& hi) {
        const i64 a = runs[chain[k]].r0 - B[k], b = a + runs[chain[k]].len;
        lo = std::max(a, W + 1);
        hi = std::min(b, W + 1 + geo.W);
        return lo < hi;
      };
      i64 k = 0;
      while (k < L) {
        i64 lo, hi;
        if (!range(k, lo, hi)) { ++k; continue; }
        i64 k1 = k;
        while (k1 < L && k1 - k < geo.kmax && range(k1, lo, hi)) {
          ++k1;
          if (aligned && Y && k1 < L && plane_of(chain[k1]) >= 0 && plane_of(chain[k1]) % geo.kmax == 0) break;   // common cut
        }
        const int K = (int)(k1 - k);
        bool fits = safe(B[k] + off(chain[k], dn_e) + W) && safe(B[k1 - 1] + off(chain[k1 - 1], up_e) + W);
        for (i64 q = k; q < k1 && fits; ++q) {
          fits = safe(B[q] + W);
          if (Y) fits = fits && safe(B[q] + W + off(chain[q], 2)) && safe(B[q] + W + off(chain[q], 3));
        }
        if (!fits) {
          for (i64 q = k; q < k1; ++q) {
            range(q, lo, hi);
            fallback.push_back(RowRange{B[q] + lo, B[q] + hi, cnt});
          }
          k = k1;
          continue;
        }
        Unit u;
        u.rec.assign(geo.REC, 0);
        range(k, lo, hi);
        u.key = (int)(B[k] + lo);
        u.order = 0;
        u.sub = 0;
        if (Y && geo.strip > 0 && geo.ext0 > 0 && geo.lines > 0 && RI > 24) {
          const i64 cell = info[RI * chain[k] + 24];
          if (cell >= 0) {
            u.order = march_order(cell, geo.ext0, geo.lines, geo.strip);
            if (aligned) {
              // plane GROUP instead of plane; then the window (grid position of the unit's first row along the line), then the line
              const i64 line = (cell / geo.ext0) % geo.lines, plane = cell / (geo.ext0 * geo.lines);
              u.order = (line / geo.strip) * ((i64)1 << 20) + plane / geo.kmax;
              const i64 x0 = cell % geo.ext0 + ((B[k] + lo) - (i64)runs[chain[k]].r0);
              u.sub = (x0 / geo.W) * ((i64)1 << 20) + line;
            }
          }
        }
        const int Kp = K <= geo.KS ? geo.KS : geo.K;   // the kernel's two unit sizes: shorter units end with empty planes
        u.rec[0] = Kp | (cnt << 8);   // | active lanes << 16, below
        u.rec[1] = u.key;
        for (int q = 0; q < 2 * cnt; ++q) u.rec[2 + q] = info[RI * chain[k] + 8 + q];
        u.rec[16] = (int)(B[k] + off(chain[k], dn_e) + W);
        u.rec[17] = (int)(B[k1 - 1] + off(chain[k1 - 1], up_e) + W);
        int hi_max = 0;
        for (int i = 0; i < K; ++i) {
          const i64 q = k + i;
          range(q, lo, hi);
          hi_max = std::max(hi_max, (int)(hi - W));
          u.rec[18 + 4 * i] = (int)(B[q] + W);
          u.rec[19 + 4 * i] = Y ? off(chain[q], 3) : 0;   // -lateral
          u.rec[20 + 4 * i] = Y ? off(chain[q], 2) : 0;   // +lateral
          u.rec[21 + 4 * i] = (int)(lo - W) | ((int)(hi - W) << 8);
          rows_m += hi - lo;
        }
        if (want_edges) {
          // rows next to [lo, hi) where the run ends inside the window, outwards until one does not qualify
          int budget = EDGE_PER_UNIT;
          for (int i = 0; i < K; ++i) {
            const i64 q = k + i, run = chain[q];
            range(q, lo, hi);
            const i64 a = runs[run].r0 - B[q], b = a + runs[run].len;
            std::vector<int> lows, highs;
            int smap = 0;
            i64 cq = 0;
            if (lo == a)
              for (i64 pos = lo - 1; pos >= W + 1 && lo - pos <= EDGE_PER_END && budget > 0 && edge_row(B[q] + pos, run, cnt, smap, cq); --pos) {
                claimed[cq] = 1; --budget;
                lows.push_back(smap); lows.push_back((int)(B[q] + pos));
              }
            if (hi == b)
              for (i64 pos = hi; pos <= W + geo.W && pos - hi < EDGE_PER_END && budget > 0 && edge_row(B[q] + pos, run, cnt, smap, cq); ++pos) {
                claimed[cq] = 1; --budget;
                highs.push_back((int)(B[q] + pos)); highs.push_back(smap);
              }
            const int nlo = (int)lows.size() / 2, nhi = (int)highs.size() / 2;
            u.rec[EDGE_REC + 2 + i] = nlo | (nhi << 8) | ((int)(u.erows.size() / 2) << 16);
            u.erows.insert(u.erows.end(), lows.rbegin(), lows.rend());   // ascending rows
            u.erows.insert(u.erows.end(), highs.begin(), highs.end());
            hi_max = std::max(hi_max, (int)(hi - W) + nhi);
          }
          u.rec[EDGE_REC + 1] = (int)(u.erows.size() / 2);
          for (int i = K; i < Kp; ++i) u.rec[EDGE_REC + 2 + i] = u.rec[EDGE_REC + 1] << 16;   // closing planes: none
        }
        // rows < hi_max need elements <= hi_max of the lines: lanes 0 .. hi_max / 2
        u.rec[0] |= std::min(64, hi_max / 2 + 1) << 16;
        for (int i = K; i < Kp; ++i) {
          // closing planes compute nothing (lo = hi); their line is the one ABOVE the last real plane -- the line that
          // plane's +plane tap reads, and a valid address for every load of the closing plane
          u.rec[18 + 4 * i] = u.rec[17];
          u.rec[19 + 4 * i] = 0;
          u.rec[20 + 4 * i] = 0;
          u.rec[21 + 4 * i] = 1 | (1 << 8);
        }
        units.push_back(std::move(u));
        k = k1;
      }
    }
  }
  std::sort(units.begin(), units.end(), [](const Unit& a, const Unit& b) {
    if (a.order != b.order) return a.order < b.order;
    return a.sub != b.sub ? a.sub < b.sub : a.key < b.key;
  });
  mrec.reserve(units.size() * geo.REC);
  if (want_edges) {   // the value stream follows the order of the units
    i64 first = 0;
    edges->meta.clear();
    edges->slots_read = 0;
    for (auto& u : units) {
      const int ne = (int)(u.erows.size() / 2);
      u.rec[EDGE_REC] = (int)first;
      for (int e = 0; e < ne; ++e) {
        edges->meta.push_back(u.erows[2 * e]);
        edges->meta.push_back((int)(EDGE_SLOTS * first + 2 * e));
        edges->meta.push_back(2 * ne);
        edges->meta.push_back(u.erows[2 * e + 1]);
      }
      first += ne;
      edges->slots_read += (int64_t)ne * ((((u.rec[0] >> 8) & 255) + 1) & ~1);   // whole pairs
    }
    edges->rows_e = first;
  }
  for (auto& u : units) mrec.insert(mrec.end(), u.rec.begin(), u.rec.end());
  if (okeys) {   // the order as one number per unit (build_tiles lines the slices up with it)
    okeys->clear();
    okeys->reserve(units.size());
    for (auto& u : units) okeys->push_back(u.order * ((i64)1 << 32) + u.key);
  }
}

// Tile table of the slice kernel (pg_spmv.hip k_spmv_s): the units (sorted by ukey) and the slices that need no halo
// (sorted by skey, the same order) are both split into 8 equal parts -- one per XCD, as the kernel without tiles does --
// and every part into `T` tiles: equal numbers of units, and the slices whose keys lie between the tile's first unit and
// the next tile's.  tab[(q (T + 1) + t) 2 + {0, 1}] = first unit / first slice of tile t of XCD q (t = T: the ends).
inline void plan_tiles(const std::vector<int64_t>& ukey, const std::vector<int64_t>& skey, int T, std::vector<int>& tab) {
  typedef int64_t i64;
  const i64 nu = (i64)ukey.size(), ns = (i64)skey.size();
  tab.assign((size_t)8 * (T + 1) * 2, 0);
  for (int q = 0; q < 8; ++q) {
    const i64 u0 = nu * q / 8, u1 = nu * (q + 1) / 8, s0 = ns * q / 8, s1 = ns * (q + 1) / 8;
    i64 sprev = s0;
    for (int t = 0; t <= T; ++t) {
      const i64 u = u0 + (u1 - u0) * t / T;
      i64 sl;
      if (t == 0) sl = s0;
      else if (t == T || u >= nu) sl = s1;
      else sl = std::lower_bound(skey.begin(), skey.end(), ukey[u]) - skey.begin();
      sl = std::min(std::max(sl, sprev), s1);
      sprev = sl;
      tab[((size_t)q * (T + 1) + t) * 2] = (int)u;
      tab[((size_t)q * (T + 1) + t) * 2 + 1] = (int)sl;
    }
  }
}

// ---- multigrid preconditioner (pg_multigrid.hip): the host side of its set-up ----------------------------------------
// Row-major inverse of the n x n matrix a (row-major) by Gauss-Jordan elimination with partial pivoting, carried in long double
// and rounded once: the exact solve of the hierarchy's last level (<= 200 rows), applied on the device as one small
// matrix-vector product.  false: a pivot vanished (singular to working precision); inv is then unspecified.
inline bool mg_dense_inverse(int n, const double* a, double* inv) {
  if (n <= 0) return true;
  const size_t w = 2 * (size_t)n;
  std::vector<long double> m((size_t)n * w, 0.0L);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) m[i * w + j] = a[(size_t)i * n + j];
    m[i * w + n + i] = 1.0L;
  }
  for (int c = 0; c < n; ++c) {
    int piv = c;
    long double best = m[c * w + c] < 0 ? -m[c * w + c] : m[c * w + c];
    for (int i = c + 1; i < n; ++i) {
      const long double v = m[i * w + c] < 0 ? -m[i * w + c] : m[i * w + c];
      if (v > best) { best = v; piv = i; }
    }
    if (!(best > 0.0L)) return false;
    if (piv != c)
      for (size_t j = 0; j < w; ++j) std::swap(m[c * w + j], m[piv * w + j]);
    const long double d = 1.0L / m[c * w + c];
    for (size_t j = 0; j < w; ++j) m[c * w + j] *= d;
    for (int i = 0; i < n; ++i) {
      if (i == c) continue;
      const long double f = m[i * w + c];
      if (f == 0.0L) continue;
      for (size_t j = 0; j < w; ++j) m[i * w + j] -= f * m[c * w + j];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) inv[(size_t)i * n + j] = (double)m[i * w + n + j];
  return true;
}

// First level of the multigrid's fused tail -- the levels [t, L) that one workgroup runs in one launch with their vectors in
// LDS: the smallest t with rows[t] <= tail_rows whose levels fit lds_doubles (three vectors per level, two on the last).  The
// last level always runs there (its exact solve is part of that kernel): L - 1 when nothing more fits.  L >= 1.
inline int mg_plan_tail(const int64_t* rows, int L, int64_t tail_rows, int64_t lds_doubles) {
  int t = L - 1;
  int64_t need = 2 * rows[L - 1];
  while (t > 0 && rows[t - 1] <= tail_rows && need + 3 * rows[t - 1] <= lds_doubles) {
    --t;
    need += 3 * rows[t];
  }
  return t;
}

// ---- spectral estimate (pg_specest.hip): the Ritz values of an Arnoldi recursion -------------------------------------------
// Eigenvalues (wr + i wi, n each) of the leading n x n block of a real upper Hessenberg matrix h, stored column major with
// leading dimension ld (entry (i, j) at h[j * ld + i]; entries below the subdiagonal are not read): EISPACK's `hqr` (Martin,
// Peters and Wilkinson, "The QR algorithm for real Hessenberg matrices", Numer. Math. 14, 1970) restated for 0-based column-major
// storage -- compare it against that routine; only the sweep limit differs (60 here, 30 there).  Francis' double-shift QR
// iteration on a copy, deflating at negligible subdiagonal entries, complex pairs read off the final 2 x 2 blocks (the pair's
// member with the positive imaginary part first), exceptional shifts after 10 and 20 sweeps on the same block.  Eigenvalues
// only: rows above the active block are not updated.  false: a block took more than 60 sweeps (n <= 200 expected: never seen).
inline bool hessenberg_eigenvalues(int n, const double* h, int ld, double* wr, double* wi) {
  if (n <= 0) return true;
  std::vector<double> A((size_t)n * n, 0.0);
  auto a = [&](int i, int j) -> double& { return A[(size_t)i * n + j]; };
  auto fabs_ = [](double v) { return v < 0.0 ? -v : v; };
  auto sign_ = [](double v, double s) { return s < 0.0 ? (v < 0.0 ? v : -v) : (v < 0.0 ? -v : v); };
  double anorm = 0.0;
  for (int i = 0; i < n; ++i)
    for (int j = (i > 0 ? i - 1 : 0); j < n; ++j) {
      a(i, j) = h[(size_t)j * ld + i];
      anorm += fabs_(a(i, j));
    }
  int nn = n - 1;
  double t = 0.0;
  while (nn >= 0) {
    int its = 0, l;
    do {
      for (l = nn; l >= 1; --l) {   // a negligible subdiagonal entry splits the matrix
        double s = fabs_(a(l - 1, l - 1)) + fabs_(a(l, l));
        if (s == 0.0) s = anorm;
        if (fabs_(a(l, l - 1)) + s == s) { a(l, l - 1) = 0.0; break; }
      }
      double x = a(nn, nn);
      if (l == nn) {                // one root
        wr[nn] = x + t; wi[nn] = 0.0;
        --nn;
      } else {
        double y = a(nn - 1, nn - 1), w = a(nn, nn - 1) * a(nn - 1, nn);
        if (l == nn - 1) {          // two roots
          const double p = 0.5 * (y - x), q = p * p + w;
          double z = std::sqrt(fabs_(q));
          x += t;
          if (q >= 0.0) {
            z = p + sign_(z, p);
            wr[nn - 1] = wr[nn] = x + z;
            if (z != 0.0) wr[nn] = x - w / z;
            wi[nn - 1] = wi[nn] = 0.0;
          } else {
            wr[nn - 1] = wr[nn] = x + p;
            wi[nn - 1] = z; wi[nn] = -z;
          }
          nn -= 2;
        } else {                    // no root yet: one double-shift sweep on rows / columns l .. nn
          if (its >= 60) return false;
          if (its == 10 || its == 20) {   // exceptional shift
            t += x;
            for (int i = 0; i <= nn; ++i) a(i, i) -= x;
            const double s = fabs_(a(nn, nn - 1)) + fabs_(a(nn - 1, nn - 2));
            y = x = 0.75 * s;
            w = -0.4375 * s * s;
          }
          ++its;
          int m;
          double p = 0.0, q = 0.0, r = 0.0, z;
          for (m = nn - 2; m >= l; --m) {   // two consecutive small subdiagonal entries: the sweep may start at m
            z = a(m, m);
            r = x - z;
            double s = y - z;
            p = (r * s - w) / a(m + 1, m) + a(m, m + 1);
            q = a(m + 1, m + 1) - z - r - s;
            r = a(m + 2, m + 1);
            s = fabs_(p) + fabs_(q) + fabs_(r);
            if (s != 0.0) { p /= s; q /= s; r /= s; }
            if (m == l) break;
            const double u = fabs_(a(m, m - 1)) * (fabs_(q) + fabs_(r));
            const double v = fabs_(p) * (fabs_(a(m - 1, m - 1)) + fabs_(z) + fabs_(a(m + 1, m + 1)));
            if (u + v == v) break;
          }
          for (int i = m + 2; i <= nn; ++i) {
            a(i, i - 2) = 0.0;
            if (i != m + 2) a(i, i - 3) = 0.0;
          }
          for (int k = m; k <= nn - 1; ++k) {
            if (k != m) {
              p = a(k, k - 1);
              q = a(k + 1, k - 1);
              r = k != nn - 1 ? a(k + 2, k - 1) : 0.0;
              x = fabs_(p) + fabs_(q) + fabs_(r);
              if (x != 0.0) { p /= x; q /= x; r /= x; }
            }
            const double s = sign_(std::sqrt(p * p + q * q + r * r), p);
            if (s == 0.0) continue;
            if (k == m) {
              if (l != m) a(k, k - 1) = -a(k, k - 1);
            } else {
              a(k, k - 1) = -s * x;
            }
            p += s;
            x = p / s; y = q / s; z = r / s;
            q /= p; r /= p;
            for (int j = k; j <= nn; ++j) {           // rows k .. k+2
              double pp = a(k, j) + q * a(k + 1, j);
              if (k != nn - 1) { pp += r * a(k + 2, j); a(k + 2, j) -= pp * z; }
              a(k + 1, j) -= pp * y;
              a(k, j) -= pp * x;
            }
            const int mmin = nn < k + 3 ? nn : k + 3;
            for (int i = l; i <= mmin; ++i) {         // columns k .. k+2
              double pp = x * a(i, k) + y * a(i, k + 1);
              if (k != nn - 1) { pp += z * a(i, k + 2); a(i, k + 2) -= pp * r; }
              a(i, k + 1) -= pp * q;
              a(i, k) -= pp;
            }
          }
        }
      }
    } while (l < nn - 1);
  }
  return true;
}

// ---- minimal-residual step of BiCGStab(l) (pg_bicgstabl.hip; tests/bicgstabl_host.cpp) --------------------------------------
// G: the Gram matrix of the power basis R[0..l] of the residual, (l+1) x (l+1), row major with leading dimension BL_LD.
// Solves  G[1..k, 1..k] gamma[1..k] = G[1..k, 0]  by Cholesky with diagonal pivoting for the largest k <= l whose pivots all
// exceed BL_PIV_TOL times their own diagonal entry (the squared sine of the angle between that basis vector and the span of
// the ones eliminated before it); gamma[i] = 0 beyond k, gamma[0] = 0.  Returns k; 0: not even G11 is positive and finite
// (Â r = 0).  Whatever gamma comes back, x += Σ gamma_i R[i-1] and r -= Σ gamma_i R[i] keep r the residual of x: a shrunk block
// costs optimality of the step, never consistency.  Compiled for the device too (one thread), and by g++ for the host tests.
#if defined(__HIPCC__)
#define PGHOST_HD __host__ __device__
#else
#define PGHOST_HD
#endif
constexpr int BL_MAX_L = 8;
constexpr int BL_LD = BL_MAX_L + 1;
constexpr double BL_PIV_TOL = 1e-13;

PGHOST_HD inline bool bl_finite(double v) { return v == v && v <= 1.7976931348623157e308 && v >= -1.7976931348623157e308; }

PGHOST_HD inline int bicgstabl_small_solve(const double* G, int l, double* gamma) {
  for (int i = 0; i <= BL_MAX_L; ++i) gamma[i] = 0.0;
  if (l < 1 || l > BL_MAX_L) return 0;
  double M[BL_MAX_L][BL_MAX_L], c[BL_MAX_L], d0[BL_MAX_L], y[BL_MAX_L];
  int perm[BL_MAX_L];
  for (int k = l; k >= 1; --k) {
    for (int i = 0; i < k; ++i) {
      for (int j = 0; j < k; ++j) M[i][j] = G[(i + 1) * BL_LD + (j + 1)];
      c[i] = G[(i + 1) * BL_LD];
      d0[i] = M[i][i];
      perm[i] = i;
    }
    bool ok = true;
    for (int s = 0; s < k && ok; ++s) {
      int p = s;
      for (int q = s + 1; q < k; ++q)
        if (M[q][q] > M[p][p]) p = q;
      if (p != s) {
        for (int j = 0; j < k; ++j) { const double t = M[s][j]; M[s][j] = M[p][j]; M[p][j] = t; }
        for (int i = 0; i < k; ++i) { const double t = M[i][s]; M[i][s] = M[i][p]; M[i][p] = t; }
        { const double t = c[s]; c[s] = c[p]; c[p] = t; }
        { const double t = d0[s]; d0[s] = d0[p]; d0[p] = t; }
        { const int t = perm[s]; perm[s] = perm[p]; perm[p] = t; }
      }
      const double piv = M[s][s];
      if (!(piv > BL_PIV_TOL * d0[s]) || !bl_finite(piv)) { ok = false; break; }
      const double root = sqrt(piv);
      M[s][s] = root;
      c[s] = c[s] / root;
      for (int q = s + 1; q < k; ++q) M[q][s] = M[q][s] / root;
      for (int q = s + 1; q < k; ++q) {
        for (int t = s + 1; t <= q; ++t) {
          M[q][t] -= M[q][s] * M[t][s];
          M[t][q] = M[q][t];
        }
        c[q] -= M[q][s] * c[s];
      }
    }
    if (!ok) continue;
    for (int s = k - 1; s >= 0; --s) {
      double v = c[s];
      for (int q = s + 1; q < k; ++q) v -= M[q][s] * y[q];
      y[s] = v / M[s][s];
      if (!bl_finite(y[s])) ok = false;
    }
    if (!ok) continue;
    for (int s = 0; s < k; ++s) gamma[1 + perm[s]] = y[s];
    return k;
  }
  return 0;
}

// ---- scalars of IDR(s) (pg_idrs.hip; tests/idrs_host.cpp) --------------------------------------------------------------------
// The shadow vectors are never stored: p_k[i] is a pure integer function of the row number i and k, the splitmix64 finaliser of
// i + (k + 1) 0x9E3779B97F4A7C15 mapped to (z >> 11) 2^-52 - 1 in [-1, 1) -- 53 bits times a power of two less one: exact in fp64,
// bit-identical here, on the device and in numpy (tests/idrs_reference.py shadow).
constexpr int IDR_MAX_S = 8;
constexpr double IDR_PIV_TOL = 1e-15;   // ~ 9 eps.  |M_kk| <= IDR_PIV_TOL |p_k| |G_k|: the pivot is the rounding of its own dot product
constexpr double IDR_KAPPA = 0.7;       // ω is enlarged when the angle between t = Âr and r has a cosine below it
constexpr uint64_t IDR_GOLDEN = 0x9E3779B97F4A7C15ull;

PGHOST_HD inline double idr_shadow_mixed(uint64_t z) {   // z = i + (k + 1) IDR_GOLDEN
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * 2.220446049250313e-16 - 1.0;
}

PGHOST_HD inline double idr_shadow(uint64_t i, int k) { return idr_shadow_mixed(i + (uint64_t)(k + 1) * IDR_GOLDEN); }

// Forward substitution on the lower triangle of M (s x s, row major, leading dimension IDR_MAX_S):
//   M[lo..hi, lo..hi] out[lo..hi] = rhs[lo..hi],  0 <= lo <= hi <= s;  out = 0 outside [lo, hi).
// Used with (k, s) for c and with (0, k) for α.  False -- and out all zero -- when s is not in 1 .. IDR_MAX_S, the range is
// not inside it, or an entry of the solution is not finite (a zero or non-finite pivot included): the caller restarts.
PGHOST_HD inline bool idr_lower_solve(const double* M, int s, int lo, int hi, const double* rhs, double* out) {
  for (int i = 0; i < IDR_MAX_S; ++i) out[i] = 0.0;
  if (s < 1 || s > IDR_MAX_S || lo < 0 || hi > s || lo > hi) return false;
  bool ok = true;
  for (int i = lo; i < hi; ++i) {
    double v = rhs[i];
    for (int j = lo; j < i; ++j) v -= M[i * IDR_MAX_S + j] * out[j];
    out[i] = v / M[i * IDR_MAX_S + i];
    if (!bl_finite(out[i])) ok = false;
  }
  if (!ok)
    for (int i = 0; i < IDR_MAX_S; ++i) out[i] = 0.0;
  return ok;
}

// ---- scalars of restarted GMRES (pg_gmres.hip; tests/gmres_host.cpp) ---------------------------------------------------------
// The scalar block `gm` of a solve with restart length m -- H, cs, sn, g, y and the two coefficient arrays the reductions write --
// and the three one-thread steps that work on it: the verdict at a restart, one column of the Hessenberg matrix, the back
// substitution.  The kernels of pg_gmres.hip are one-line wrappers of these; tests/gmres_reference.py GmScalars restates them.
struct GmLayout {
  int m;
  PGHOST_HD int H(int i, int j) const { return (m + 1) * j + i; }        // (m+1) x m, column major
  PGHOST_HD int cs(int i) const { return (m + 1) * m + i; }
  PGHOST_HD int sn(int i) const { return (m + 1) * m + m + i; }
  PGHOST_HD int g(int i) const { return (m + 1) * m + 2 * m + i; }       // m + 1
  PGHOST_HD int y(int i) const { return (m + 1) * m + 3 * m + 1 + i; }   // m
  PGHOST_HD int h1(int i) const { return (m + 1) * m + 4 * m + 1 + i; }  // m + 2: first-pass coefficients
  PGHOST_HD int h2(int i) const { return (m + 1) * m + 5 * m + 3 + i; }  // m + 2: second pass, then ||w||^2
  PGHOST_HD int J() const { return (m + 1) * m + 6 * m + 5; }            // columns of the current cycle
  PGHOST_HD int invn() const { return J() + 1; }                          // 1 / norm of the vector to scale
  PGHOST_HD int size() const { return J() + 2; }
};

// where the steps find their scalars in `sc` (the device: the S_* slots of pg_spmv.h, pg_gmres.hip gm_slots)
struct GmSlots {
  int bb, rr, rr0, iters, reltol2, abstol2, tol2, tolw2, done, notfinite;
  // bb: (b,b)_W    rr: (r,r)_W of the last true residual    rr0: (b,b), the inner tolerance's reference    tol2: the inner tolerance
  // (Givens estimate)    tolw2: the weighted one (acceptance)    notfinite: set with done = 2 when a norm was NaN or Inf
};
// done: 0 the cycle runs; 1 converged; 2 stopped, unconverged (singular, or not finite); 3 the cycle has ended, no verdict yet
constexpr double GM_RUNS = 0.0, GM_CONVERGED = 1.0, GM_STOPPED = 2.0, GM_CYCLE_ENDED = 3.0;

// start of a restart cycle (and verdict on the one before): gm[h2(0)] = (r,r), gm[h2(1)] = (r,r)_W of the TRUE residual.
// Inner tolerance from the first residual (zero initial guess: ||r0|| = ||b||), lowered when the estimate was met and the weighted
// test was not; acceptance on the weighted norm.  A norm that is not finite stops the solve: never converged.
PGHOST_HD inline void gm_begin(GmLayout L, GmSlots S, double* gm, double* sc, int first) {
  const double rr = gm[L.h2(0)], rrw = gm[L.h2(1)];
  if (first) {
    sc[S.bb] = rrw;
    sc[S.rr0] = rr;
    sc[S.iters] = 0.0;
    const double t2 = sc[S.reltol2] * rr;
    sc[S.tol2] = t2 > sc[S.abstol2] ? t2 : sc[S.abstol2];
    const double tw = sc[S.reltol2] * rrw;
    sc[S.tolw2] = tw > sc[S.abstol2] ? tw : sc[S.abstol2];
  }
  sc[S.rr] = rrw;
  const bool finite = bl_finite(rr) && bl_finite(rrw);
  const double beta = finite && rr > 0.0 ? sqrt(rr) : 0.0;
  for (int i = 0; i <= L.m; ++i) gm[L.g(i)] = 0.0;
  gm[L.g(0)] = beta;
  gm[L.J()] = 0.0;
  gm[L.invn()] = beta > 0.0 ? 1.0 / beta : 0.0;
  if (!finite) {
    sc[S.done] = GM_STOPPED;
    sc[S.notfinite] = 1.0;
    return;
  }
  if (sc[S.done] == GM_STOPPED) return;   // singular (gm_hess): stays
  const bool ok = rrw <= sc[S.tolw2] || beta == 0.0;
  sc[S.done] = ok ? GM_CONVERGED : GM_RUNS;
  if (!ok && !first && rrw > 0.0) {
    // the estimate may already be below the inner tolerance: aim the next cycle at the weighted test
    const double aim = 0.25 * rr * (sc[S.tolw2] / rrw);
    if (aim < sc[S.tol2]) sc[S.tol2] = aim;
  }
}

// column j of the Hessenberg matrix: h = h1 + h2 (CGS2), previous rotations, new rotation, residual estimate
PGHOST_HD inline void gm_hess(GmLayout L, GmSlots S, int j, double* gm, double* sc) {
  if (sc[S.done] != GM_RUNS) return;
  const double nn = gm[L.h2(j + 1)];
  bool finite = bl_finite(nn);
  for (int i = 0; i <= j; ++i) {
    gm[L.H(i, j)] = gm[L.h1(i)] + gm[L.h2(i)];
    finite = finite && bl_finite(gm[L.H(i, j)]);
  }
  const double hn = nn > 0.0 ? sqrt(nn) : 0.0;
  gm[L.H(j + 1, j)] = hn;
  sc[S.iters] += 1.0;
  if (!finite) {   // keep the previous columns only; the caller does not hand the state back
    gm[L.J()] = (double)j;
    sc[S.done] = GM_STOPPED;
    sc[S.notfinite] = 1.0;
    return;
  }
  for (int i = 0; i < j; ++i) {
    const double c = gm[L.cs(i)], s = gm[L.sn(i)];
    const double a = gm[L.H(i, j)], b = gm[L.H(i + 1, j)];
    gm[L.H(i, j)] = c * a + s * b;
    gm[L.H(i + 1, j)] = -s * a + c * b;
  }
  const double a = gm[L.H(j, j)];
  const double d = hypot(a, hn);
  gm[L.J()] = (double)(j + 1);
  if (d == 0.0) {   // A v_j = 0: singular system; keep the previous columns only
    gm[L.J()] = (double)j;
    sc[S.done] = GM_STOPPED;
    return;
  }
  const double c = a / d, s = hn / d;
  gm[L.cs(j)] = c;
  gm[L.sn(j)] = s;
  gm[L.H(j, j)] = d;
  gm[L.H(j + 1, j)] = 0.0;
  const double gj = gm[L.g(j)];
  gm[L.g(j)] = c * gj;
  gm[L.g(j + 1)] = -s * gj;
  const double rr = gm[L.g(j + 1)] * gm[L.g(j + 1)];
  gm[L.invn()] = hn > 0.0 ? 1.0 / hn : 0.0;
  // the cycle ends here (not a verdict -- the true weighted residual at the restart decides, gm_begin);
  // hn == 0: the Krylov space is exhausted (exact solution)
  if (rr <= sc[S.tol2] || hn == 0.0) sc[S.done] = GM_CYCLE_ENDED;
}

// y = H(0:J,0:J)^-1 g(0:J)   (back substitution on the rotated, upper-triangular H)
PGHOST_HD inline void gm_solve_y(GmLayout L, double* gm) {
  const int J = (int)gm[L.J()];
  for (int i = J - 1; i >= 0; --i) {
    double s = gm[L.g(i)];
    for (int k = i + 1; k < J; ++k) s -= gm[L.H(i, k)] * gm[L.y(k)];
    gm[L.y(i)] = s / gm[L.H(i, i)];
  }
}

// ---- schedule of the mixed-precision Horner chain (pg_krylov.hip) ------------------------------------------
// The chain applies the m factors (I - Â/λ_k), λ_k the Chebyshev nodes of [1 - g, 1 + g] (index 0 = the largest), in m - 1
// launches: the first applied root is folded into the first launch's coefficients, launch i = 0 .. m-2 applies root
// order[i + 1].  The mixed chain stores the results of its first n32 = m - 1 - j launches in fp32 and runs the last j launches
// -- the TAIL, whose first launch reads fp32 and writes fp64 (the hand-over) -- as they have always run.  What a rounded
// intermediate contributes to the result is its rounding times the product of the factors still to come, so
//   * the tail is a DAMPING set: the j roots nearest the Chebyshev nodes of degree j of the same interval (a tie goes to the
//     larger root), whose product is close to the minimax polynomial of degree j, 1 / T_j(1/g) ~ 2 ρ^j, ρ = g / (1 + √(1 - g²));
//   * the other m - j roots come first, the largest and the smallest remaining root in turn, and the tail's own roots in
//     the same manner: no product of the factors before or after a stored intermediate grows beyond what the all-fp64 order
//     (the same alternation, applied from its far end) shows for the same m.
// j = 0 would leave nothing between the last fp32 store and the result; the chain's result is fp64 anyway, so the smallest
// tail is the hand-over launch alone and a request for j = 0 is served with j = 1.
constexpr int MIXED_MAX_DEGREE = 40;
constexpr double MIXED_FLOOR32 = 1e-7;   // reduction ||s|| / ||r|| an application reaches with every intermediate stored in fp32
constexpr double MIXED_DAMP = 0.45;      // what one more fp64 launch at the end takes off that floor (g <= 0.72; ρ(g) beyond)
constexpr double MIXED_SAFETY = 0.5;     // the floor left by the tail must be below this share of the reduction the solve needs
enum { CHAIN_F64 = 0, CHAIN_FIRST = 1, CHAIN_MIDDLE = 2, CHAIN_HANDOVER = 3 };

struct MixedChain {
  int m = 0, j = 0, n32 = 0;          // degree, launches of the tail (hand-over included), launches that write fp32
  int order[MIXED_MAX_DEGREE];        // order[i]: index of the root applied i-th (0 = the largest)
  int kind[MIXED_MAX_DEGREE];         // kind[i], i = 0 .. m-2: CHAIN_* of the launch that applies order[i + 1]
};

inline double mixed_root(int m, double g, int k) { return 1.0 + g * std::cos(M_PI * (2.0 * k + 1.0) / (2.0 * m)); }
inline double mixed_rho(double g) { return g / (1.0 + std::sqrt(std::max(0.0, 1.0 - g * g))); }

// idx[0..n): root indices in ascending order (descending roots) -> out: first, last, second, last but one, ...
inline void mixed_alternate(const int* idx, int n, int* out) {
  for (int k = 0, lo = 0, hi = n - 1; k < n; ++k) out[k] = (k & 1) ? idx[hi--] : idx[lo++];
}

// the schedule for (m, g, j); false: fewer than two fp32 launches would remain (or m out of range) -- the chain runs all fp64,
// in its own order, and `out` is not to be used
inline bool mixed_chain_schedule(int m, double g, int j, MixedChain& out) {
  if (m < 2 || m > MIXED_MAX_DEGREE || j < 0) return false;
  if (j < 1) j = 1;
  const int n32 = m - 1 - j;
  if (n32 < 2) return false;
  out.m = m; out.j = j; out.n32 = n32;
  bool taken[MIXED_MAX_DEGREE];
  for (int k = 0; k < m; ++k) taken[k] = false;
  int tail[MIXED_MAX_DEGREE], head[MIXED_MAX_DEGREE];
  for (int q = 0; q < j; ++q) {
    const double c = mixed_root(j, g, q);
    int best = -1;
    double dbest = 0.0;
    for (int k = 0; k < m; ++k) {
      if (taken[k]) continue;
      const double d = std::fabs(mixed_root(m, g, k) - c);
      if (best < 0 || d < dbest) { best = k; dbest = d; }   // (strict: a tie keeps the smaller index, the larger root)
    }
    taken[best] = true;
  }
  int nt = 0, nh = 0;
  for (int k = 0; k < m; ++k) (taken[k] ? tail[nt++] : head[nh++]) = k;
  mixed_alternate(head, nh, out.order);
  mixed_alternate(tail, nt, out.order + nh);
  for (int i = 0; i < m - 1; ++i)
    out.kind[i] = i == 0 ? CHAIN_FIRST : (i < n32 ? CHAIN_MIDDLE : (i == n32 ? CHAIN_HANDOVER : CHAIN_F64));
  out.kind[m - 1] = CHAIN_F64;
  return true;
}

// the tail for a solve whose application must reduce the residual by `needed` (||s|| / ||r||, 0 < needed < 1): the smallest
// j >= 1 with  floor32 damp^j <= safety needed,  damp = max(MIXED_DAMP, ρ(g));  -1: all fp64 (fewer than two fp32 launches
// would remain, or `needed` is no such number)
inline int mixed_chain_tail(double needed, double g, int m) {
  if (!(needed > 0.0) || !(needed < 1.0) || m < 2 || m > MIXED_MAX_DEGREE) return -1;
  const double damp = std::max(MIXED_DAMP, mixed_rho(g));
  int j = 1;
  double left = MIXED_FLOOR32 * damp;
  while (left > MIXED_SAFETY * needed && j < m) { left *= damp; ++j; }
  return m - 1 - j >= 2 ? j : -1;
}

// max over [1 - g, 1 + g] of |Π (1 - λ / r)| over the tail's roots, in extended precision: the end points and the one
// critical point between every two neighbouring roots (the logarithmic derivative Σ 1 / (λ - r) falls from +∞ to -∞ there:
// bisection)
inline long double mixed_tail_max(const MixedChain& c, double g) {
  const int j = c.j;
  long double r[MIXED_MAX_DEGREE];
  for (int q = 0; q < j; ++q) {
    const int k = c.order[c.m - j + q];
    r[q] = 1.0L + (long double)g * cosl(3.141592653589793238462643383279502884L * (2.0L * k + 1.0L) / (2.0L * c.m));
  }
  std::sort(r, r + j);
  auto P = [&](long double x) { long double p = 1.0L; for (int q = 0; q < j; ++q) p *= 1.0L - x / r[q]; return fabsl(p); };
  long double best = std::max(P(1.0L - (long double)g), P(1.0L + (long double)g));
  for (int q = 0; q + 1 < j; ++q) {
    long double a = r[q], b = r[q + 1];
    for (int it = 0; it < 200; ++it) {
      const long double x = 0.5L * (a + b);
      if (!(x > a && x < b)) break;
      long double d = 0.0L;
      for (int t = 0; t < j; ++t) d += 1.0L / (x - r[t]);
      if (d > 0.0L) a = x; else b = x;
    }
    best = std::max(best, P(0.5L * (a + b)));
  }
  return best;
}

}  // namespace pghost
