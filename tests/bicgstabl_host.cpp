// AddressSanitizer + UndefinedBehaviorSanitizer build of the small solve of BiCGStab(l)'s minimal-residual step
// (pg_host_algos.h: pghost::bicgstabl_small_solve, the code the device runs on one thread), as a stand-alone program:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/bicgstabl_host.cpp
// Reads Gram matrices from the file given as argv[1] -- per matrix a line "l" and a line with the (l+1)^2 entries, row major --
// and prints "k gamma_0 .. gamma_l" for each.  tests/test_bicgstabl_host.py feeds it and compares with the numpy restatement.
#include <cstdio>
#include <vector>

#include "../penguin/jl_amd/csrc/pg_host_algos.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int l = 0, count = 0;
  while (std::fscanf(f, "%d", &l) == 1) {
    if (l < 0 || l > 64) { std::fclose(f); return 3; }
    std::vector<double> in((size_t)(l + 1) * (l + 1));
    for (double& v : in)
      if (std::fscanf(f, "%lf", &v) != 1) { std::fclose(f); return 3; }
    // exactly the storage the device kernel hands over: BL_LD x BL_LD, entries beyond l untouched (zero here)
    std::vector<double> G((size_t)pghost::BL_LD * pghost::BL_LD, 0.0);
    for (int a = 0; a <= l && a < pghost::BL_LD; ++a)
      for (int b = 0; b <= l && b < pghost::BL_LD; ++b) G[(size_t)a * pghost::BL_LD + b] = in[(size_t)a * (l + 1) + b];
    std::vector<double> gamma(pghost::BL_MAX_L + 1, -1.0);
    const int k = pghost::bicgstabl_small_solve(G.data(), l, gamma.data());
    std::printf("%d", k);
    for (int i = 0; i <= pghost::BL_MAX_L; ++i) std::printf(" %.17g", gamma[i]);
    std::printf("\n");
    ++count;
  }
  std::fclose(f);
  std::printf("all matrices done %d\n", count);
  return 0;
}
