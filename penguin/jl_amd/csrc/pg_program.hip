// pg_program.hip -- device functions on the device: the per-step kernel that evaluates a pg_program at the listed points of a
// slot of time-dependent data and adds the weighted result to the right-hand side (DESIGN.md "Device functions"), the same
// evaluator on caller-supplied points (test support), and the exported host interpreter and validator.
#include "pg_program.h"

#include "pg_common.h"
#include "pg_solver_internal.h"

namespace pg {

// the operand stack of one lane: column `lane` of stack[depth][256] in LDS.  A wave's access to one depth is 64 consecutive
// doubles (no bank conflict), no lane reads another's column (no barrier anywhere), and nothing is indexed in private memory
// (no scratch).  The top of the stack is prog_eval's register.
struct LdsStack {
  double* col;
  __host__ __device__ double get(int d) const { return col[d * TD_EVAL_BLOCK]; }
  __host__ __device__ void set(int d, double x) { col[d * TD_EVAL_BLOCK] = x; }
};

// entry e: out[row_e] += w_e (c0 P(p_e, t0) + c1 P(p_e, t1)); c0 == 0 skips the evaluation at t0 (BE, border values).  The
// rows of a list are unique and no other kernel of the step writes them at the same time: no atomics, the same bits every
// run.  row == nullptr (pg_debug_program_eval): out[e] = that sum itself, w taken as 1.
__global__ __launch_bounds__(TD_EVAL_BLOCK) void k_td_eval(pg_program P, i64 n, const int* __restrict__ row,
                                                           const double* __restrict__ w, const double* __restrict__ p0,
                                                           const double* __restrict__ p1, const double* __restrict__ p2,
                                                           double c0, double c1, double t0, double t1, double* __restrict__ out) {
  __shared__ double stack[PG_PROG_MAX_STACK * TD_EVAL_BLOCK];
  LdsStack S{stack + threadIdx.x};
  const i64 stride = (i64)gridDim.x * TD_EVAL_BLOCK;
  for (i64 e = blockIdx.x * (i64)TD_EVAL_BLOCK + threadIdx.x; e < n; e += stride) {
    const double x0 = p0[e], x1 = p1[e], x2 = p2[e];
    double v = 0.0;
    for (int k = c0 != 0.0 ? 0 : 1; k < 2; ++k)  // (one copy of the evaluator in the kernel's code)
      v += (k ? c1 : c0) * pgprog::prog_eval(P, x0, x1, x2, k ? t1 : t0, S);
    if (row) out[row[e]] += w[e] * v;
    else out[e] = v;
  }
}

void td_eval_launch(const pg_program& P, i64 n, const int* row, const double* w, const double* p0, const double* p1,
                    const double* p2, double c0, double c1, double t0, double t1, double* out, hipStream_t st) {
  if (n <= 0) return;                           // an empty list: no launch
  hipLaunchKernelGGL(k_td_eval, dim3(grid_for(n, TD_EVAL_BLOCK)), dim3(TD_EVAL_BLOCK), 0, st, P, n, row, w, p0, p1, p2, c0, c1,
                     t0, t1, out);
  PG_HIP(hipGetLastError());
}

}  // namespace pg

using namespace pg;

extern "C" {

int32_t pg_program_validate(const pg_program* prog) {
  PG_API_BEGIN
  std::string why;
  PG_REQUIRE(pgprog::program_validate(prog, &why), "invalid program: " + why);
  PG_API_END
}

int32_t pg_program_eval_host(const pg_program* prog, int64_t npts, const double* xyz, double t, double* out) {
  PG_API_BEGIN
  std::string why;
  PG_REQUIRE(pgprog::program_eval_host(prog, npts, xyz, t, out, &why), "pg_program_eval_host refused: " + why);
  PG_API_END
}

int32_t pg_debug_program_eval(const pg_program* prog, int64_t npts, const double* xyz, double t, double* out) {
  PG_API_BEGIN
  require_init();
  std::string why;
  PG_REQUIRE(pgprog::program_validate(prog, &why), "pg_debug_program_eval refused: invalid program: " + why);
  PG_REQUIRE(npts >= 0 && (npts == 0 || (xyz && out)), "pg_debug_program_eval: points and an output array are needed");
  if (npts == 0) return 0;
  std::vector<double> soa((size_t)3 * npts);
  for (i64 i = 0; i < npts; ++i)
    for (int d = 0; d < 3; ++d) soa[(size_t)d * npts + i] = xyz[3 * i + d];
  DevBuf<double> pts(3 * npts), res(npts);
  pts.upload(soa.data(), 3 * npts);
  td_eval_launch(*prog, npts, nullptr, nullptr, pts.p, pts.p + npts, pts.p + 2 * npts, 0.0, 1.0, t, t, res.p, ctx().stream);
  res.download(out, npts);
  PG_API_END
}

}  // extern "C"
