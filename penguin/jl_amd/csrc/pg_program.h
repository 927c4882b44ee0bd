// pg_program.h -- device functions: the validator and the evaluator of pg_program (include/penguin_hip.h), free of HIP so that
// the CPU test-suite can compile them with g++ under ASan / UBSan (tests/program_host.cpp).  ONE evaluator, prog_eval, serves
// the host interpreter and the per-step kernel: its operand stack is a template parameter (a plain array on the host, one
// column of LDS per lane on the device), the switch over the opcodes is the same code.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/penguin_hip.h"

#if defined(__HIPCC__)
#define PG_PROG_HD __host__ __device__
#else
#define PG_PROG_HD
#endif

namespace pgprog {

// operands an instruction takes from the stack (it always leaves one)
PG_PROG_HD inline int op_arity(int op) {
  if (op == PG_OP_CONST || op == PG_OP_VAR) return 0;
  if (op == PG_OP_SELECT) return 3;
  if ((op >= PG_OP_NEG && op <= PG_OP_TANH) || op == PG_OP_ERF || op == PG_OP_ERFC) return 1;
  return 2;
}

// Host only.  true: every instruction is known, every index in range, the stack never underflows, never holds more than
// PG_PROG_MAX_STACK values and ends with one.  Nothing of the program is executed.  Reads n_ops and n_const first and nothing
// beyond the arrays' bounds whatever they hold.
inline bool program_validate(const pg_program* p, std::string* why) {
  auto fail = [&](const std::string& m) {
    if (why) *why = m;
    return false;
  };
  if (!p) return fail("NULL program");
  if (p->n_ops < 1 || p->n_ops > PG_PROG_MAX_OPS)
    return fail("n_ops = " + std::to_string(p->n_ops) + " is outside 1 .. " + std::to_string((int)PG_PROG_MAX_OPS));
  if (p->n_const < 0 || p->n_const > PG_PROG_MAX_CONST)
    return fail("n_const = " + std::to_string(p->n_const) + " is outside 0 .. " + std::to_string((int)PG_PROG_MAX_CONST));
  int depth = 0;
  for (int q = 0; q < p->n_ops; ++q) {
    const int op = p->op[q], arg = p->arg[q];
    const std::string at = "instruction " + std::to_string(q) + ": ";
    if (op >= PG_OP_COUNT) return fail(at + "unknown opcode " + std::to_string(op));
    if (op == PG_OP_CONST && arg >= p->n_const)
      return fail(at + "constant index " + std::to_string(arg) + " with " + std::to_string(p->n_const) + " constants");
    if (op == PG_OP_VAR && arg > 3) return fail(at + "variable index " + std::to_string(arg) + " (0 .. 2: coordinates, 3: t)");
    const int need = op_arity(op);
    if (depth < need)
      return fail(at + "stack underflow (" + std::to_string(need) + " operands needed, " + std::to_string(depth) + " there)");
    depth += 1 - need;
    if (depth > PG_PROG_MAX_STACK) return fail(at + "stack deeper than " + std::to_string((int)PG_PROG_MAX_STACK));
  }
  if (depth != 1) return fail("the program ends with " + std::to_string(depth) + " values on the stack, not 1");
  return true;
}

// The evaluator.  Stack: get(d) / set(d, v) on the slots d = 0 .. PG_PROG_MAX_STACK - 2; the top of the stack lives in a
// register, so a program of depth D touches D - 1 slots.  The program must have passed program_validate.  The instruction
// stream is the same for every point: in a kernel the switch is uniform over the wave.
template <class Stack>
PG_PROG_HD inline double prog_eval(const pg_program& P, double x0, double x1, double x2, double t, Stack& S) {
  double top = 0.0;
  int sp = 0;                                   // values on the stack, the cached top included
  for (int q = 0; q < P.n_ops; ++q) {
    const int op = P.op[q];
    if (op <= PG_OP_VAR) {
      if (sp > 0) S.set(sp - 1, top);
      ++sp;
      if (op == PG_OP_CONST) {
        top = P.konst[P.arg[q]];
      } else {
        const int v = P.arg[q];
        top = v == 0 ? x0 : v == 1 ? x1 : v == 2 ? x2 : t;
      }
      continue;
    }
    if (op == PG_OP_SELECT) {
      const double a = S.get(sp - 2), c = S.get(sp - 3);
      sp -= 2;
      top = c != 0.0 ? a : top;
      continue;
    }
    switch (op) {                               // unary: the top alone
      case PG_OP_NEG: top = -top; continue;
      case PG_OP_ABS: top = fabs(top); continue;
      case PG_OP_SQRT: top = sqrt(top); continue;
      case PG_OP_EXP: top = exp(top); continue;
      case PG_OP_LOG: top = log(top); continue;
      case PG_OP_SIN: top = sin(top); continue;
      case PG_OP_COS: top = cos(top); continue;
      case PG_OP_TANH: top = tanh(top); continue;
      case PG_OP_ERF: top = erf(top); continue;
      case PG_OP_ERFC: top = erfc(top); continue;
      default: break;
    }
    const double a = S.get(sp - 2), b = top;    // binary: a below b
    --sp;
    switch (op) {
      case PG_OP_ADD: top = a + b; break;
      case PG_OP_SUB: top = a - b; break;
      case PG_OP_MUL: top = a * b; break;
      case PG_OP_DIV: top = a / b; break;
      case PG_OP_POW: top = pow(a, b); break;
      case PG_OP_ATAN2: top = atan2(a, b); break;
      case PG_OP_MIN: top = fmin(a, b); break;
      case PG_OP_MAX: top = fmax(a, b); break;
      case PG_OP_LT: top = a < b ? 1.0 : 0.0; break;
      case PG_OP_LE: top = a <= b ? 1.0 : 0.0; break;
      case PG_OP_GT: top = a > b ? 1.0 : 0.0; break;
      case PG_OP_GE: top = a >= b ? 1.0 : 0.0; break;
      default: break;
    }
  }
  return top;
}

struct HostStack {
  double v[PG_PROG_MAX_STACK];
  double get(int d) const { return v[d]; }
  void set(int d, double x) { v[d] = x; }
};

// the host interpreter behind pg_program_eval_host; false and *why when the program is invalid or an argument missing
inline bool program_eval_host(const pg_program* p, int64_t npts, const double* xyz, double t, double* out, std::string* why) {
  if (!program_validate(p, why)) return false;
  if (npts < 0 || (npts > 0 && (!xyz || !out))) {
    if (why) *why = "npts >= 0, and points and an output array, are needed";
    return false;
  }
  HostStack S;
  for (int64_t i = 0; i < npts; ++i) out[i] = prog_eval(*p, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], t, S);
  return true;
}

}  // namespace pgprog
