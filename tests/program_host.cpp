// The validator and the host interpreter of device-function programs (penguin/jl_amd/csrc/pg_program.h) as a stand-alone
// program for the CPU suite, built with -fsanitize=address,undefined (tests/test_device_function_cpu.py).
//   program_host FILE NPTS   FILE: records of sizeof(pg_program) bytes, anything in them.  Per record one line:
//                            "bad <reason>"  or  "ok <NPTS results as hex bit patterns>" at the fixed points below.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../penguin/jl_amd/csrc/pg_program.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  const int npts = atoi(argv[2]);
  if (npts < 1 || npts > 4096) return 4;
  std::vector<double> xyz(3 * (size_t)npts), out(npts);
  for (int i = 0; i < npts; ++i) {              // the points of the test: a fixed lattice walk in [0.5, 1.5)^3
    xyz[3 * i] = 0.5 + ((i * 37) % 101) / 101.0;
    xyz[3 * i + 1] = 0.5 + ((i * 53) % 103) / 103.0;
    xyz[3 * i + 2] = 0.5 + ((i * 71) % 107) / 107.0;
  }
  std::vector<unsigned char> rec(sizeof(pg_program));
  long records = 0;
  while (fread(rec.data(), 1, rec.size(), f) == rec.size()) {
    pg_program p;
    memcpy(&p, rec.data(), sizeof p);
    std::string why;
    if (!pgprog::program_eval_host(&p, npts, xyz.data(), 0.375, out.data(), &why)) {
      printf("bad %s\n", why.c_str());
    } else {
      printf("ok");
      for (int i = 0; i < npts; ++i) {
        uint64_t bits;
        memcpy(&bits, &out[i], 8);
        printf(" %016" PRIx64, bits);
      }
      printf("\n");
    }
    ++records;
  }
  fclose(f);
  // the entry points' other refusals
  std::string why;
  if (pgprog::program_validate(nullptr, &why) || why.empty()) return 5;
  printf("all records done %ld\n", records);
  return 0;
}
