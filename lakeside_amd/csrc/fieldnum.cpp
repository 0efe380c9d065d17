// Text of a VARCHAR chart field -> the double `try_cast(<field> as double)` aggregates (BaseExpr.scala:357-362).
// Only two classes of text are answered, the ones whose DuckDB cast needs no guessing:
//   number: the whole string matches -?[0-9]+(\.[0-9]+)?([eE][-+]?[0-9]+)? and strtod gives a finite double;
//   NULL:   the first byte is an ASCII letter other than i I n N (no spelling of a number, inf or nan starts so).
// Everything else -- empty, blanks, a leading `+`, inf / nan spellings, hex, underscores, a trailing dot, overflow to
// infinity -- is neither, and the evaluator fails the call rather than guess (field charts).
#include <cmath>
#include <cstdlib>
#include <string>

#include "../../include/lakeside_text.h"

extern "C" int lk_field_number(const char* s, size_t n, double* out) {
  if (n == 0) return -1;
  const unsigned char c0 = static_cast<unsigned char>(s[0]);
  if ((c0 >= 'a' && c0 <= 'z') || (c0 >= 'A' && c0 <= 'Z'))
    return (c0 == 'i' || c0 == 'I' || c0 == 'n' || c0 == 'N') ? -1 : 0;
  auto digit = [&](size_t i) { return i < n && s[i] >= '0' && s[i] <= '9'; };
  size_t i = s[0] == '-' ? 1 : 0;
  if (!digit(i)) return -1;
  while (digit(i)) i++;
  if (i < n && s[i] == '.') {
    i++;
    if (!digit(i)) return -1;
    while (digit(i)) i++;
  }
  if (i < n && (s[i] == 'e' || s[i] == 'E')) {
    i++;
    if (i < n && (s[i] == '-' || s[i] == '+')) i++;
    if (!digit(i)) return -1;
    while (digit(i)) i++;
  }
  if (i != n) return -1;
  const std::string z(s, n);   // NUL-terminated for strtod (the grammar above holds no locale-dependent byte but '.')
  const double v = strtod(z.c_str(), nullptr);
  if (!std::isfinite(v)) return -1;
  if (out) *out = v;
  return 1;
}
