// sbm_observable_program.hpp -- the postfix programs of custom observables (include/sbm.h, SBM_OP_*): the interpreter
// the assembly kernel runs (sbm_assemble.hpp) and the checker that lets it run unchecked.  Plain C++17 with no HIP
// include, so both compile for the host too (tests/test_project_checks_cpu.py pins the interpreter against
// oracle/program_oracle.py and walks every refusal of the checker).
#ifndef SBM_OBSERVABLE_PROGRAM_HPP
#define SBM_OBSERVABLE_PROGRAM_HPP

#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/sbm.h"

#if defined(__HIPCC__)
#define SBM_PROG_FN __host__ __device__ inline
#else
#define SBM_PROG_FN inline
#endif

enum { SBM_E_ARG = -1 };   // what every refused argument returns (sbm_core.hip adds the codes of its HIP and plugin errors)

// the refusal of a host-side check: the message into the caller's buffer, SBM_E_ARG back
inline int sbm_refuse(char* msg, size_t msg_len, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, msg_len, fmt, ap);
  va_end(ap);
  return SBM_E_ARG;
}

// One subprogram of a custom observable: a postfix stack machine.  sbm_prog_check has passed every program at load time
// (opcodes, operand ranges, stack depth <= SBM_PROG_MAX_STACK).
SBM_PROG_FN double sbm_prog_eval(const int32_t* __restrict__ code, const double* __restrict__ consts,
                                 const double* __restrict__ Yb, const int32_t* __restrict__ vars, double t) {
  double st[SBM_PROG_MAX_STACK];
  int sp = 0;
  for (int pc = 0;; ++pc) {
    const int op = code[pc];
    if (op == SBM_OP_END) break;
    switch (op) {
      case SBM_OP_VAR: st[sp++] = Yb[vars[code[++pc]]]; break;
      case SBM_OP_CONST: st[sp++] = consts[code[++pc]]; break;
      case SBM_OP_TIME: st[sp++] = t; break;
      case SBM_OP_ADD: --sp; st[sp - 1] += st[sp]; break;
      case SBM_OP_SUB: --sp; st[sp - 1] -= st[sp]; break;
      case SBM_OP_MUL: --sp; st[sp - 1] *= st[sp]; break;
      case SBM_OP_DIV: --sp; st[sp - 1] /= st[sp]; break;
      case SBM_OP_POW: --sp; st[sp - 1] = pow(st[sp - 1], st[sp]); break;
      case SBM_OP_POWI: {
        int n = code[++pc];
        const bool inv = n < 0;
        n = inv ? -n : n;
        double b = st[sp - 1], r = 1.0;
        while (n) { if (n & 1) r *= b; b *= b; n >>= 1; }
        st[sp - 1] = inv ? 1.0 / r : r;
        break;
      }
      case SBM_OP_NEG: st[sp - 1] = -st[sp - 1]; break;
      case SBM_OP_EXP: st[sp - 1] = exp(st[sp - 1]); break;
      case SBM_OP_LOG: st[sp - 1] = log(st[sp - 1]); break;
      case SBM_OP_SQRT: st[sp - 1] = sqrt(st[sp - 1]); break;
      case SBM_OP_TANH: st[sp - 1] = tanh(st[sp - 1]); break;
      case SBM_OP_SIN: st[sp - 1] = sin(st[sp - 1]); break;
      case SBM_OP_COS: st[sp - 1] = cos(st[sp - 1]); break;
      case SBM_OP_ABS: st[sp - 1] = fabs(st[sp - 1]); break;
      case SBM_OP_SIGN: st[sp - 1] = st[sp - 1] > 0.0 ? 1.0 : (st[sp - 1] < 0.0 ? -1.0 : 0.0); break;
      default: return __builtin_nan("");
    }
  }
  return sp == 1 ? st[0] : __builtin_nan("");
}

// The subprogram code[pc .. end) of program c, which lists n_vars variables: known opcodes, operands present and in
// range, never fewer values on the stack than an operator takes nor more than SBM_PROG_MAX_STACK, closed by SBM_OP_END
// with exactly one value left.  0, or the refusal (message in msg).
inline int sbm_prog_check(const int32_t* code, int n_code, int pc, int end, int n_vars, int n_const, const char* who, int c,
                          char* msg, size_t msg_len) {
  if (pc < 0 || end > n_code || pc >= end) return sbm_refuse(msg, msg_len, "%s: program %d: bad subprogram bounds", who, c);
  int depth = 0;
  bool closed = false;
  for (; pc < end && !closed; ++pc) {
    const int op = code[pc];
    switch (op) {
      case SBM_OP_END: closed = true; break;
      case SBM_OP_VAR:
        if (++pc >= end || code[pc] < 0 || code[pc] >= n_vars)
          return sbm_refuse(msg, msg_len, "%s: program %d: variable operand out of range", who, c);
        ++depth; break;
      case SBM_OP_CONST:
        if (++pc >= end || code[pc] < 0 || code[pc] >= n_const)
          return sbm_refuse(msg, msg_len, "%s: program %d: constant operand out of range", who, c);
        ++depth; break;
      case SBM_OP_TIME: ++depth; break;
      case SBM_OP_ADD: case SBM_OP_SUB: case SBM_OP_MUL: case SBM_OP_DIV: case SBM_OP_POW:
        if (depth < 2) return sbm_refuse(msg, msg_len, "%s: program %d: stack underflow", who, c);
        --depth; break;
      case SBM_OP_POWI:
        if (++pc >= end || code[pc] < -64 || code[pc] > 64)
          return sbm_refuse(msg, msg_len, "%s: program %d: integer power out of range", who, c);
        if (depth < 1) return sbm_refuse(msg, msg_len, "%s: program %d: stack underflow", who, c);
        break;
      case SBM_OP_NEG: case SBM_OP_EXP: case SBM_OP_LOG: case SBM_OP_SQRT: case SBM_OP_TANH: case SBM_OP_SIN:
      case SBM_OP_COS: case SBM_OP_ABS: case SBM_OP_SIGN:
        if (depth < 1) return sbm_refuse(msg, msg_len, "%s: program %d: stack underflow", who, c);
        break;
      default: return sbm_refuse(msg, msg_len, "%s: program %d: unknown opcode %d", who, c, op);
    }
    if (depth > SBM_PROG_MAX_STACK)
      return sbm_refuse(msg, msg_len, "%s: program %d needs a stack deeper than %d", who, c, SBM_PROG_MAX_STACK);
  }
  if (!closed || depth != 1)
    return sbm_refuse(msg, msg_len, "%s: program %d: subprogram does not leave exactly one value", who, c);
  return 0;
}

#endif  // SBM_OBSERVABLE_PROGRAM_HPP
