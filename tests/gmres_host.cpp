// AddressSanitizer + UndefinedBehaviorSanitizer build of the scalars of restarted GMRES (pg_host_algos.h: pghost::GmLayout, gm_begin,
// gm_hess, gm_solve_y -- the code the device's one-thread kernels run), as a stand-alone program:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/gmres_host.cpp
// argv[1]: a file of commands, one per line; every command prints one line.
//     case m reltol2 abstol2                    a new solve: gm = a HEAP block of exactly GmLayout{m}.size() doubles, zeroed as the
//                                               device zeroes it, sc = a heap block of exactly the ten scalars the steps use
//                                               -> "C size"
//     begin first rr rrw                        what the reduction writes, then gm_begin
//                                               -> "B done notfinite iters tol2 tolw2 bb rr J invn g_0 .. g_m"
//     hess j h1_0 .. h1_j h2_0 .. h2_j nn       what the reductions write, then gm_hess
//                                               -> "H done notfinite iters J invn cs_j sn_j g_j g_j+1 H_0j .. H_j+1,j"
//     solve                                     gm_solve_y -> "Y J y_0 .. y_J-1"
// tests/test_gmres_host.py writes the commands from the Arnoldi coefficients of the numpy restatement (tests/gmres_reference.py)
// and compares every line with it.  Any slip of the layout arithmetic is a sanitizer report: the blocks have no slack.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../penguin/jl_amd/csrc/pg_host_algos.h"

namespace {

enum { BB = 0, RR, RR0, ITERS, RELTOL2, ABSTOL2, TOL2, TOLW2, DONE, NOTFINITE, SC_COUNT };
constexpr pghost::GmSlots SLOTS{BB, RR, RR0, ITERS, RELTOL2, ABSTOL2, TOL2, TOLW2, DONE, NOTFINITE};

bool number(FILE* f, double& v) {
  char word[64];
  if (std::fscanf(f, "%63s", word) != 1) return false;
  char* end = nullptr;
  v = std::strtod(word, &end);   // (reads nan / inf / -inf as well)
  return end != word && *end == '\0';
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  std::unique_ptr<double[]> gm, sc;
  pghost::GmLayout L{0};
  char cmd[16];
  long count = 0;
  int status = 0;
  while (status == 0 && std::fscanf(f, "%15s", cmd) == 1) {
    if (std::strcmp(cmd, "case") == 0) {
      int m = 0;
      double r2 = 0.0, a2 = 0.0;
      if (std::fscanf(f, "%d", &m) != 1 || m < 1 || m > 200 || !number(f, r2) || !number(f, a2)) { status = 3; break; }
      L = pghost::GmLayout{m};
      gm.reset(new double[(size_t)L.size()]);
      sc.reset(new double[SC_COUNT]);
      for (int i = 0; i < L.size(); ++i) gm[i] = 0.0;
      for (int i = 0; i < SC_COUNT; ++i) sc[i] = 0.0;
      sc[RELTOL2] = r2;
      sc[ABSTOL2] = a2;
      std::printf("C %d\n", L.size());
    } else if (std::strcmp(cmd, "begin") == 0) {
      int first = 0;
      double rr = 0.0, rrw = 0.0;
      if (!gm || std::fscanf(f, "%d", &first) != 1 || !number(f, rr) || !number(f, rrw)) { status = 3; break; }
      gm[L.h2(0)] = rr;
      gm[L.h2(1)] = rrw;
      pghost::gm_begin(L, SLOTS, gm.get(), sc.get(), first);
      std::printf("B %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g", sc[DONE], sc[NOTFINITE], sc[ITERS], sc[TOL2], sc[TOLW2],
                  sc[BB], sc[RR], gm[L.J()], gm[L.invn()]);
      for (int i = 0; i <= L.m; ++i) std::printf(" %.17g", gm[L.g(i)]);
      std::printf("\n");
    } else if (std::strcmp(cmd, "hess") == 0) {
      int j = -1;
      if (!gm || std::fscanf(f, "%d", &j) != 1 || j < 0 || j >= L.m) { status = 3; break; }
      for (int i = 0; i <= j && status == 0; ++i)
        if (!number(f, gm[L.h1(i)])) status = 3;
      for (int i = 0; i <= j + 1 && status == 0; ++i)     // (the last one is ||w||^2)
        if (!number(f, gm[L.h2(i)])) status = 3;
      if (status) break;
      pghost::gm_hess(L, SLOTS, j, gm.get(), sc.get());
      std::printf("H %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g", sc[DONE], sc[NOTFINITE], sc[ITERS], gm[L.J()], gm[L.invn()],
                  gm[L.cs(j)], gm[L.sn(j)], gm[L.g(j)], gm[L.g(j + 1)]);
      for (int i = 0; i <= j + 1; ++i) std::printf(" %.17g", gm[L.H(i, j)]);
      std::printf("\n");
    } else if (std::strcmp(cmd, "solve") == 0) {
      if (!gm) { status = 3; break; }
      pghost::gm_solve_y(L, gm.get());
      const int J = (int)gm[L.J()];
      std::printf("Y %d", J);
      for (int i = 0; i < J; ++i) std::printf(" %.17g", gm[L.y(i)]);
      std::printf("\n");
    } else {
      status = 3;
      break;
    }
    ++count;
  }
  std::fclose(f);
  if (status) return status;
  std::printf("all commands done %ld\n", count);
  return 0;
}
