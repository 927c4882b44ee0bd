// AddressSanitizer + UndefinedBehaviorSanitizer build of the host side of the multigrid set-up (pg_host_algos.h): the dense
// inverse of the hierarchy's last level and the choice of the fused tail.  Compiled and run by tests/test_mg_host_sanitizers.py:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/mg_host_asan.cpp
// Seeded random inputs, functional checks, exit code 0 = all passed.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../penguin/jl_amd/csrc/pg_host_algos.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      ++g_fail;                                           \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                       \
      fprintf(stderr, "\n");                              \
    }                                                     \
  } while (0)

int main() {
  std::mt19937_64 rng(20240611);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  // 1. inverse: diagonally dominant, badly row-scaled (cut-cell rows differ by 1e5), and matrices that NEED pivoting
  for (int n : {1, 2, 3, 7, 64, 200}) {
    for (int kind = 0; kind < 3; ++kind) {
      std::vector<double> a((size_t)n * n), inv((size_t)n * n, -7.0);
      for (int i = 0; i < n; ++i) {
        double row = 0.0;
        for (int j = 0; j < n; ++j) { a[(size_t)i * n + j] = U(rng); row += std::fabs(a[(size_t)i * n + j]); }
        if (kind != 2) a[(size_t)i * n + i] = row + 1.0;
        if (kind == 1) { const double s = std::pow(10.0, 5.0 * U(rng)); for (int j = 0; j < n; ++j) a[(size_t)i * n + j] *= s; }
      }
      if (kind == 2 && n >= 2) a[0] = 0.0;   // a zero in the first pivot position
      const bool ok = pghost::mg_dense_inverse(n, a.data(), inv.data());
      CHECK(ok, "inverse refused, n = %d kind %d", n, kind);
      double worst = 0.0;
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
          long double s = 0.0L;
          for (int k = 0; k < n; ++k) s += (long double)inv[(size_t)i * n + k] * a[(size_t)k * n + j];   // (rows of a differ by 1e10 in
                                                                                                      //  scale: inv(A) A is the product whose terms are O(1))
          worst = std::fmax(worst, std::fabs((double)(s - (i == j ? 1.0L : 0.0L))));
        }
      CHECK(worst <= (kind == 2 ? 1e-9 : 1e-11), "inv(A) A - I = %.3e, n = %d kind %d", worst, n, kind);
    }
  }
  {  // singular: refused, nothing written outside inv
    const int n = 5;
    std::vector<double> a((size_t)n * n, 0.0), inv((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) a[(size_t)i * n + i] = 1.0;
    for (int j = 0; j < n; ++j) a[(size_t)3 * n + j] = a[(size_t)1 * n + j];
    CHECK(!pghost::mg_dense_inverse(n, a.data(), inv.data()), "a singular matrix was inverted");
    CHECK(pghost::mg_dense_inverse(0, nullptr, nullptr), "n = 0");
  }
  // 2. tail plan: the last level always; never a level above the threshold; never more than the LDS holds; maximal
  for (int rep = 0; rep < 2000; ++rep) {
    const int L = 1 + (int)(rng() % 12);
    std::vector<int64_t> rows(L);
    int64_t r = 1 + (int64_t)(rng() % 200);
    for (int l = L - 1; l >= 0; --l) { rows[l] = r; r = r * (2 + (int64_t)(rng() % 7)) + (int64_t)(rng() % 5); }
    const int64_t thr = (int64_t)(rng() % 5000), lds = 400 + (int64_t)(rng() % 9000);
    const int t = pghost::mg_plan_tail(rows.data(), L, thr, lds);
    CHECK(t >= 0 && t <= L - 1, "tail %d of %d levels", t, L);
    int64_t need = 2 * rows[L - 1];
    for (int l = t; l < L - 1; ++l) { need += 3 * rows[l]; CHECK(rows[l] <= thr, "level %d of %lld rows in the tail, threshold %lld", l, (long long)rows[l], (long long)thr); }
    CHECK(need <= lds || t == L - 1, "tail needs %lld doubles of %lld", (long long)need, (long long)lds);
    if (t > 0) CHECK(rows[t - 1] > thr || need + 3 * rows[t - 1] > lds, "level %d would have fitted", t - 1);
  }
  if (g_fail == 0) printf("all checks passed\n");
  return g_fail == 0 ? 0 : 1;
}
