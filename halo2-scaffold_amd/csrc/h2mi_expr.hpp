// Host-side walk over an h2mi_gate_program (include/h2mi.h), shared by the constraint-system check (h2mi_prover.cpp:
// h2mi_gate_program_check) and the quotient kernel's uploader (h2mi_plonk.hip: h2mi_plonk_evaluate_h_expr_dev).  No device code.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/h2mi.h"

namespace h2 {

struct ExprShape {
  uint32_t degree = 0;     // the largest polynomial degree (query 1, constant 0, ADD / SUB max, MUL sum)
  uint32_t max_stack = 0;  // the deepest operand stack
  uint32_t n_polys = 0;
};

// Structural rules of a program: known ops, constant indices, |rotation| < 2^k, stack discipline, END placement.  `column(kind, index,
// rotation)` decides whether a query is allowed (column counts, query lists, non-NULL pointers: the caller's business).  n_challenges:
// how many challenges the caller knows of — a CHALLENGE op with an index at or beyond it is refused (0: every CHALLENGE op); the
// operand has degree 0 [RECALL halo2_proofs v2023_02_02 plonk/circuit.rs Expression::degree].
template <class ColumnOk>
inline int expr_walk(const h2mi_gate_program* g, uint32_t k, uint32_t n_challenges, ColumnOk&& column, ExprShape* out) {
  if (!g || !g->ops || g->n_ops == 0 || g->n_ops > H2MI_MAX_EXPR_OPS || g->n_constants > H2MI_MAX_EXPR_CONSTANTS || n_challenges > H2MI_MAX_CHALLENGES)
    return H2MI_EINVAL;
  if (g->n_constants && !g->constants) return H2MI_EINVAL;
  const int64_t n = (int64_t)1 << k;
  uint32_t deg[H2MI_MAX_EXPR_STACK];
  uint32_t sp = 0;
  ExprShape sh;
  for (uint32_t i = 0; i < g->n_ops; i++) {
    const h2mi_expr_op& o = g->ops[i];
    switch (o.op) {
      case H2MI_EXPR_ADVICE:
      case H2MI_EXPR_FIXED:
      case H2MI_EXPR_INSTANCE:
        if ((int64_t)o.rotation >= n || (int64_t)o.rotation <= -n || !column(o.op, o.index, o.rotation)) return H2MI_EINVAL;
        if (sp == H2MI_MAX_EXPR_STACK) return H2MI_EINVAL;
        deg[sp++] = 1;
        break;
      case H2MI_EXPR_CONSTANT:
        if (o.index >= g->n_constants || sp == H2MI_MAX_EXPR_STACK) return H2MI_EINVAL;
        deg[sp++] = 0;
        break;
      case H2MI_EXPR_CHALLENGE:
        if (o.index >= n_challenges || sp == H2MI_MAX_EXPR_STACK) return H2MI_EINVAL;
        deg[sp++] = 0;
        break;
      case H2MI_EXPR_ADD:
      case H2MI_EXPR_SUB:
      case H2MI_EXPR_MUL:
        if (sp < 2) return H2MI_EINVAL;
        deg[sp - 2] = o.op == H2MI_EXPR_MUL ? deg[sp - 2] + deg[sp - 1] : std::max(deg[sp - 2], deg[sp - 1]);
        sp--;
        break;
      case H2MI_EXPR_NEG:
        if (sp < 1) return H2MI_EINVAL;
        break;
      case H2MI_EXPR_END:
        if (sp != 1) return H2MI_EINVAL;
        sh.degree = std::max(sh.degree, deg[0]);
        sh.n_polys++;
        sp = 0;
        break;
      default:
        return H2MI_EINVAL;
    }
    sh.max_stack = std::max(sh.max_stack, sp);
  }
  if (g->ops[g->n_ops - 1].op != H2MI_EXPR_END) return H2MI_EINVAL;
  if (out) *out = sh;
  return H2MI_OK;
}

}  // namespace h2
