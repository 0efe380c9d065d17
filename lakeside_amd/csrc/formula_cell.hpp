// One cell of a formula over DataExprs: the postfix program of formula.cpp run over the cell's leaves.
//
// Restates Formula.eval (core/src/main/scala/com/cardinal/utils/ast/Formula.scala:32-69) with ASTUtils.eval
// (ASTUtils.scala:42-69) for one (timestamp, group key):
//   * both sides present: add / sub / mul are the IEEE operations; div emits nothing when e2.value == 0 (+0.0 and
//     -0.0 alike; a NaN divisor is not zero, so NaN flows through) (Formula.scala:52-63);
//   * one side absent: under add only, the missing side reads 0 and the row takes the present side's timestamp and
//     tags (Formula.scala:45-47); under every other operator the key is dropped (Formula.scala:48);
//   * the result's tags are e1's -- e2's when e1 was filled (Formula.scala:54-60);
//   * a ConstantExpr is present wherever the cell exists (ASTUtils.scala:50-64); its tag source is FX_SRC_CONST,
//     which the caller resolves (no tags without groupBys, a candidate row's tags with them).
// The same function is compiled into fx_eval_count / fx_eval_write (formula_kernels.hip) and into the host export
// lk_formula_eval_cell (formula.cpp), so the CPU tests drive exactly what the kernel runs.  Plain IEEE double
// arithmetic: no fused operations are possible (no a * b + c shape on one operator), no fast-math.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LK_FX_HD __host__ __device__
#else
#define LK_FX_HD
#endif

namespace lk {

constexpr int FX_MAXPROG = 64;    // postfix operations of one formula
constexpr int FX_MAXLEAF = 8;     // distinct base expressions one formula references
constexpr int FX_MAXSTACK = 16;   // operand stack (the parser checks the program's depth)
constexpr int32_t FX_SRC_CONST = -1;
constexpr int FX_MAXCOL = 8;      // groupBy columns of a formula's key
// Collapse ranks (smaller wins): a named row 2 * (its name's place in string order) + 4; a row without a name tag
// sorts before every named row of its key unless one of its present groupBy tags sorts after the name tag; the one
// all-absent row (queryTags) takes the odd rank between its neighbours (FxOperand::qt_rank).
constexpr uint32_t FX_RANK_ABSENT = 0xffffffffu;   // name_rank entry of a dim id whose name tag is absent
constexpr uint32_t FX_RANK_NONAME_FIRST = 1u;
constexpr uint32_t FX_RANK_NONAME_LAST = 0xfffffffcu;
enum FxXform : int { FX_XF_NONE = 0, FX_XF_MUL = 1, FX_XF_DIV = 2 };

enum FxOpc : int32_t { FX_LEAF = 0, FX_CONST = 1, FX_ADD = 2, FX_SUB = 3, FX_MUL = 4, FX_DIV = 5 };

struct FxOp {
  int32_t op;     // FxOpc
  int32_t leaf;   // FX_LEAF: leaf index
  double c;       // FX_CONST: the value
};

struct FxCell {
  bool present;
  double value;
  int32_t src;    // the leaf whose row gives the tags, or FX_SRC_CONST
};

// present / value / src: per leaf of the cell.  `ops` is a well-formed postfix program of depth <= FX_MAXSTACK.
LK_FX_HD inline FxCell fx_eval_cell(const FxOp* ops, int n, const uint8_t* present, const double* value,
                                    const int32_t* src) {
  bool sp[FX_MAXSTACK];
  double sv[FX_MAXSTACK];
  int32_t ss[FX_MAXSTACK];
  int top = 0;
  for (int i = 0; i < n; i++) {
    const FxOp o = ops[i];
    if (o.op == FX_LEAF) {
      sp[top] = present[o.leaf] != 0;
      sv[top] = value[o.leaf];
      ss[top] = src[o.leaf];
      top++;
      continue;
    }
    if (o.op == FX_CONST) {
      sp[top] = true;
      sv[top] = o.c;
      ss[top] = FX_SRC_CONST;
      top++;
      continue;
    }
    top--;   // e2 at [top], e1 at [top - 1]
    bool p1 = sp[top - 1], p2 = sp[top];
    double v1 = sv[top - 1], v2 = sv[top];
    int32_t s1 = ss[top - 1];
    if (p1 != p2) {
      if (o.op == FX_ADD) {   // the missing side reads 0 with the present side's tags
        if (!p1) {
          v1 = 0.0;
          s1 = ss[top];
        } else {
          v2 = 0.0;
        }
        p1 = p2 = true;
      } else {
        p1 = p2 = false;
      }
    }
    bool p = p1 && p2;
    double v = 0.0;
    if (p) {
      if (o.op == FX_ADD) v = v1 + v2;
      else if (o.op == FX_SUB) v = v1 - v2;
      else if (o.op == FX_MUL) v = v1 * v2;
      else if (v2 != 0.0) v = v1 / v2;   // NaN != 0: flows through
      else p = false;                    // division by +-0.0: no row
    }
    sp[top - 1] = p;
    sv[top - 1] = v;
    ss[top - 1] = s1;
  }
  FxCell r;
  r.present = top == 1 && sp[0];
  r.value = r.present ? sv[0] : 0.0;
  r.src = r.present ? ss[0] : FX_SRC_CONST;
  return r;
}

}  // namespace lk
