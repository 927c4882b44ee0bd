// AddressSanitizer + UndefinedBehaviorSanitizer build of the scalars of IDR(s) (pg_host_algos.h: pghost::idr_lower_solve and
// pghost::idr_shadow, the code the device runs), as a stand-alone program:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/idrs_host.cpp
// argv[1] = "solve": reads systems from the file argv[2] -- per system a line "s lo hi", a line with the s^2 entries of M, row
// major, and a line with the s entries of the right-hand side -- and prints "ok out_0 .. out_7" for each.
// argv[1] = "shadow": prints the bit patterns of idr_shadow(i, k), i = 0 .. argv[2]-1, k = 0 .. 7, one row number per line.
// tests/test_idrs_host.py feeds it and compares with the numpy restatement.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../penguin/jl_amd/csrc/pg_host_algos.h"

static int solve(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 2;
  int s = 0, lo = 0, hi = 0, count = 0;
  while (std::fscanf(f, "%d %d %d", &s, &lo, &hi) == 3) {
    if (s < 0 || s > 64) { std::fclose(f); return 3; }
    std::vector<double> in((size_t)s * s), rhs_in((size_t)s);
    for (double& v : in)
      if (std::fscanf(f, "%lf", &v) != 1) { std::fclose(f); return 3; }
    for (double& v : rhs_in)
      if (std::fscanf(f, "%lf", &v) != 1) { std::fclose(f); return 3; }
    // exactly the storage the device kernel hands over: IDR_MAX_S x IDR_MAX_S and IDR_MAX_S entries
    constexpr int LD = pghost::IDR_MAX_S;
    std::vector<double> M((size_t)LD * LD, 0.0), rhs((size_t)LD, 0.0), out((size_t)LD, -1.0);
    for (int a = 0; a < s && a < LD; ++a) {
      for (int b = 0; b < s && b < LD; ++b) M[(size_t)a * LD + b] = in[(size_t)a * s + b];
      rhs[a] = rhs_in[a];
    }
    const bool ok = pghost::idr_lower_solve(M.data(), s, lo, hi, rhs.data(), out.data());
    std::printf("%d", ok ? 1 : 0);
    for (int i = 0; i < LD; ++i) std::printf(" %.17g", out[i]);
    std::printf("\n");
    ++count;
  }
  std::fclose(f);
  std::printf("all systems done %d\n", count);
  return 0;
}

static int shadow(long rows) {
  for (long i = 0; i < rows; ++i) {
    for (int k = 0; k < pghost::IDR_MAX_S; ++k) {
      const double v = pghost::idr_shadow((uint64_t)i, k);
      uint64_t bits;
      std::memcpy(&bits, &v, sizeof bits);
      std::printf("%016" PRIx64 "%c", bits, k + 1 < pghost::IDR_MAX_S ? ' ' : '\n');
    }
  }
  std::printf("all rows done %ld\n", rows);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  if (std::strcmp(argv[1], "solve") == 0) return solve(argv[2]);
  if (std::strcmp(argv[1], "shadow") == 0) return shadow(std::atol(argv[2]));
  return 2;
}
