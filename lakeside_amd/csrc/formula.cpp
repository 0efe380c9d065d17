// Formula text -> postfix program: a hand-written recursive descent over the arithmetic the reference evaluates.
//
// Restates what FormulaListener.toFormulaAST builds from a formula string
// (core/src/main/scala/com/cardinal/utils/ast/FormulaListener.scala:26-133):
//   * a variable is [A-Za-z_][A-Za-z0-9_]* looked up in baseExpressions; an unknown name is an error
//     (FormulaListener.scala:60-69);
//   * a number is digits(.digits)?([eE][+-]?digits)? read as ConstantExpr(text.toDouble) (FormulaListener.scala:70-74);
//   * `*` and `/` bind tighter than `+` and `-`, all four associate to the left, parentheses group, blanks are skipped;
//     unbalanced parentheses fail the parse;
//   * a formula that is a single atom is an error: the popped node is cast to Formula (FormulaListener.scala:128-131);
//   * `^`, the relational operators and unary signs are not restated: the listener's extractOp ignores POW and reads a
//     unary sign as a binary operator (FormulaListener.scala:96-118), so its outcome is an accident of the parse tree.
//     They are refused (LK_ERR_UNSUPPORTED) with the token named.
#include "formula.hpp"

#include <cstdlib>
#include <cstring>

#include "../../include/lakeside_text.h"

namespace lk {
std::string java_text(double d);   // jdtoa.cpp

namespace {
constexpr int kErrArg = -1, kErrUnsupported = -2;

struct Parser {
  const std::string& s;
  const std::vector<std::string>& names;
  FxProgram& out;
  std::string& err;
  size_t i = 0;
  int code = 0;
  int depth = 0, max_depth = 0;

  void skip() {
    while (i < s.size() && (s[i] == ' ' || s[i] == '\t' || s[i] == '\r' || s[i] == '\n')) i++;
  }
  bool fail(int c, const std::string& m) {
    if (!code) {
      code = c;
      err = m;
    }
    return false;
  }
  bool emit(FxOp o) {
    if (out.n >= FX_MAXPROG) return fail(kErrUnsupported, "formula: more than " + std::to_string(FX_MAXPROG) + " operations");
    out.ops[out.n++] = o;
    if (o.op == FX_LEAF || o.op == FX_CONST) {
      if (++depth > max_depth) max_depth = depth;
      if (depth > FX_MAXSTACK) return fail(kErrUnsupported, "formula: nested deeper than " + std::to_string(FX_MAXSTACK));
    } else {
      depth--;
    }
    return true;
  }
  static bool digit(char c) { return c >= '0' && c <= '9'; }
  static bool ident0(char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '_'; }
  // tokens the reference's grammar has and this parser refuses
  bool unsupported_at(size_t p) {
    const char c = s[p];
    if (c == '^') return fail(kErrUnsupported, "formula: operator '^' is not evaluated");
    if (c == '<' || c == '>' || c == '=' || c == '!') {
      std::string t(1, c);
      if (p + 1 < s.size() && s[p + 1] == '=') t += '=';
      return fail(kErrUnsupported, "formula: relational operator '" + t + "' is not evaluated");
    }
    return true;
  }

  bool atom() {
    skip();
    if (i >= s.size()) return fail(kErrArg, "formula: unexpected end of input");
    const char c = s[i];
    if (c == '(') {
      i++;
      if (!expr()) return false;
      skip();
      if (i >= s.size() || s[i] != ')') {
        if (i < s.size() && !unsupported_at(i)) return false;
        return fail(kErrArg, "formula: unbalanced parentheses");
      }
      i++;
      return true;
    }
    if (c == '+' || c == '-')
      return fail(kErrUnsupported, std::string("formula: unary '") + c + "' is not evaluated");
    if (digit(c)) {
      const size_t b = i;
      while (i < s.size() && digit(s[i])) i++;
      if (i < s.size() && s[i] == '.') {
        i++;
        if (i >= s.size() || !digit(s[i])) return fail(kErrArg, "formula: malformed number " + s.substr(b, i - b));
        while (i < s.size() && digit(s[i])) i++;
      }
      if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
        size_t j = i + 1;
        if (j < s.size() && (s[j] == '+' || s[j] == '-')) j++;
        if (j >= s.size() || !digit(s[j])) return fail(kErrArg, "formula: malformed number " + s.substr(b, j - b));
        while (j < s.size() && digit(s[j])) j++;
        i = j;
      }
      const std::string t = s.substr(b, i - b);
      return emit(FxOp{FX_CONST, 0, strtod(t.c_str(), nullptr)});   // text.toDouble
    }
    if (ident0(c)) {
      const size_t b = i;
      while (i < s.size() && (ident0(s[i]) || digit(s[i]))) i++;
      const std::string t = s.substr(b, i - b);
      for (size_t k = 0; k < names.size(); k++)
        if (names[k] == t) return emit(FxOp{FX_LEAF, int32_t(k), 0.0});
      return fail(kErrArg, "formula: unknown variable " + t);
    }
    if (!unsupported_at(i)) return false;
    return fail(kErrArg, std::string("formula: unexpected character '") + c + "'");
  }
  bool term() {
    if (!atom()) return false;
    for (;;) {
      skip();
      if (i >= s.size() || (s[i] != '*' && s[i] != '/')) return true;
      const char op = s[i++];
      if (!atom()) return false;
      if (!emit(FxOp{op == '*' ? FX_MUL : FX_DIV, 0, 0.0})) return false;
    }
  }
  bool expr() {
    if (!term()) return false;
    for (;;) {
      skip();
      if (i >= s.size() || (s[i] != '+' && s[i] != '-')) return true;
      const char op = s[i++];
      if (!term()) return false;
      if (!emit(FxOp{op == '+' ? FX_ADD : FX_SUB, 0, 0.0})) return false;
    }
  }
};
}  // namespace

int parse_formula(const std::string& text, const std::vector<std::string>& names, FxProgram& out, std::string& err) {
  out.n = 0;
  Parser p{text, names, out, err};
  if (p.expr()) {
    p.skip();
    if (p.i < text.size()) {
      if (p.unsupported_at(p.i)) {
        if (text[p.i] == ')') p.fail(kErrArg, "formula: unbalanced parentheses");
        else p.fail(kErrArg, "formula: unexpected token at '" + text.substr(p.i, 8) + "'");
      }
    } else if (out.n < 2 || out.ops[out.n - 1].op < FX_ADD) {
      p.fail(kErrArg, "formula: a single term is not a formula");
    }
  }
  return p.code;
}

std::string formula_program_text(const FxProgram& p) {
  static const char* const sym[] = {"", "", "+", "-", "*", "/"};
  std::string o;
  for (int i = 0; i < p.n; i++) {
    if (i) o += ' ';
    if (p.ops[i].op == FX_LEAF) o += "$" + std::to_string(p.ops[i].leaf);
    else if (p.ops[i].op == FX_CONST) o += java_text(p.ops[i].c);
    else o += sym[p.ops[i].op];
  }
  return o;
}

}  // namespace lk

extern "C" int lk_formula_plan(const char* formula, const char* const* names, size_t n, char* out, size_t cap) {
  if (!formula || (n && !names) || !out || !cap) return -1;
  std::vector<std::string> nm;
  for (size_t i = 0; i < n; i++) nm.emplace_back(names[i] ? names[i] : "");
  lk::FxProgram p;
  std::string err;
  const int rc = lk::parse_formula(formula, nm, p, err);
  const std::string text = rc ? err : lk::formula_program_text(p);
  const size_t k = text.size() < cap - 1 ? text.size() : cap - 1;
  memcpy(out, text.data(), k);
  out[k] = '\0';
  return rc;
}

extern "C" int lk_formula_eval_cell(const char* formula, const char* const* names, size_t n, size_t ncells,
                                    const uint8_t* present, const double* value, const int32_t* src,
                                    uint8_t* out_present, double* out_value, int32_t* out_src) {
  if (!formula || (n && !names) || n > size_t(lk::FX_MAXLEAF)) return -1;
  if (ncells && (!present || !value || !src || !out_present || !out_value || !out_src)) return -1;
  std::vector<std::string> nm;
  for (size_t i = 0; i < n; i++) nm.emplace_back(names[i] ? names[i] : "");
  lk::FxProgram p;
  std::string err;
  const int rc = lk::parse_formula(formula, nm, p, err);
  if (rc) return rc;
  for (size_t c = 0; c < ncells; c++) {
    const lk::FxCell r = lk::fx_eval_cell(p.ops, p.n, present + c * n, value + c * n, src + c * n);
    out_present[c] = r.present ? 1 : 0;
    out_value[c] = r.value;
    out_src[c] = r.src;
  }
  return 0;
}
