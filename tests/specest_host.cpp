// AddressSanitizer + UndefinedBehaviorSanitizer build of the host side of the spectral estimate (pg_host_algos.h): the
// eigenvalues of the Arnoldi recursion's Hessenberg matrix.  Compiled and run by tests/test_specest_host.py:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/specest_host.cpp
//     specest_host FILE
// FILE: any number of matrices, each "n ld" followed by ld * n numbers, column major (what the library downloads: ld = n + 1).
// Three hand-made matrices follow them.  For every matrix it prints "matrix n", the n x n block row by row, and "eig re im" per
// eigenvalue; the test compares with numpy.linalg.eigvals of the block printed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../penguin/jl_amd/csrc/pg_host_algos.h"

static int run(int n, int ld, const std::vector<double>& h) {
  // exact-size buffers: a read or write outside them is the sanitizer's to find
  std::vector<double> wr((size_t)n, -7.0), wi((size_t)n, -7.0);
  const bool ok = pghost::hessenberg_eigenvalues(n, h.data(), ld, wr.data(), wi.data());
  if (!ok) { fprintf(stderr, "FAIL: no convergence, n = %d\n", n); return 1; }
  printf("matrix %d\n", n);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) printf("%.17g ", j + 1 >= i ? h[(size_t)j * ld + i] : 0.0);
    printf("\n");
  }
  for (int i = 0; i < n; ++i) printf("eig %.17g %.17g\n", wr[i], wi[i]);
  return 0;
}

int main(int argc, char** argv) {
  int fail = 0;
  if (argc > 1) {
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n, ld;
    while (fscanf(f, "%d %d", &n, &ld) == 2) {
      if (n < 1 || ld < n || n > 1000) { fprintf(stderr, "bad header %d %d\n", n, ld); fclose(f); return 2; }
      std::vector<double> h((size_t)ld * n);
      for (double& v : h)
        if (fscanf(f, "%lf", &v) != 1) { fprintf(stderr, "short matrix\n"); fclose(f); return 2; }
      fail += run(n, ld, h);
    }
    fclose(f);
  }
  {  // a rotation block: eigenvalues 0.8 +- 0.6 i
    const std::vector<double> h = {0.8, 0.6, -0.6, 0.8};
    fail += run(2, 2, h);
  }
  {  // a zero subdiagonal entry (2,1): two uncoupled 2 x 2 blocks on the diagonal, one of them with a complex pair
    const int n = 4, ld = 5;
    std::vector<double> h((size_t)ld * n, 0.0);
    auto H = [&](int i, int j) -> double& { return h[(size_t)j * ld + i]; };
    H(0, 0) = 1.0; H(0, 1) = 2.0; H(0, 2) = 0.3; H(0, 3) = -0.7;
    H(1, 0) = 0.5; H(1, 1) = 1.5; H(1, 2) = 0.9; H(1, 3) = 0.2;
    H(2, 1) = 0.0; H(2, 2) = 1.0; H(2, 3) = -2.0;
    H(3, 2) = 1.0; H(3, 3) = 1.2;
    H(4, 3) = 0.25;   // the row the Arnoldi recursion appends: never read
    fail += run(n, ld, h);
  }
  {  // 1 x 1
    const std::vector<double> h = {1.75, 1e-3};
    fail += run(1, 2, h);
  }
  if (fail == 0) printf("all matrices done\n");
  return fail == 0 ? 0 : 1;
}
