// AddressSanitizer + UndefinedBehaviorSanitizer build of the schedule of the mixed-precision Horner chain (pg_host_algos.h:
// pghost::mixed_chain_schedule, mixed_chain_tail, mixed_tail_max).  Compiled and run by tests/test_host_mixed_chain.py:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/mixed_chain_host.cpp
//     mixed_chain_host G [G ...]
// For every g given, every m = 4 .. 40 and every j = 0 .. m it prints
//     sched m g j ok | j_served n32 | order[0..m) | kind[0..m-1) | tail_max
// (ok = 0: "all fp64", nothing after it), then for every m and a ladder of needed reductions 10^(-k/4), k = 1 .. 60,
//     tail m g needed j
// and at the end the named constants:  const floor32 damp safety.
#include <cstdio>
#include <cstdlib>

#include "../penguin/jl_amd/csrc/pg_host_algos.h"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    const double g = atof(argv[a]);
    for (int m = 4; m <= 40; ++m) {
      for (int j = 0; j <= m; ++j) {
        pghost::MixedChain c;
        const bool ok = pghost::mixed_chain_schedule(m, g, j, c);
        printf("sched %d %.17g %d %d", m, g, j, ok ? 1 : 0);
        if (ok) {
          printf(" | %d %d |", c.j, c.n32);
          for (int i = 0; i < m; ++i) printf(" %d", c.order[i]);
          printf(" |");
          for (int i = 0; i < m - 1; ++i) printf(" %d", c.kind[i]);
          printf(" | %.21Lg", pghost::mixed_tail_max(c, g));
        }
        printf("\n");
      }
      for (int k = 1; k <= 60; ++k) {
        const double needed = std::pow(10.0, -0.25 * k);
        printf("tail %d %.17g %.17g %d\n", m, g, needed, pghost::mixed_chain_tail(needed, g, m));
      }
      printf("tail %d %.17g %.17g %d\n", m, g, 0.0, pghost::mixed_chain_tail(0.0, g, m));
      printf("tail %d %.17g %.17g %d\n", m, g, 1.0, pghost::mixed_chain_tail(1.0, g, m));
    }
  }
  printf("const %.17g %.17g %.17g\n", pghost::MIXED_FLOOR32, pghost::MIXED_DAMP, pghost::MIXED_SAFETY);
  return 0;
}
