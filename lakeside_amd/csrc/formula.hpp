// Formula text -> postfix program (host).  See formula.cpp.
#pragma once
#include <string>
#include <vector>

#include "formula_cell.hpp"

namespace lk {

struct FxProgram {
  int n = 0;
  FxOp ops[FX_MAXPROG];
};

// Parses `text` over the variables `names` (a leaf's index is its position in `names`).  Returns 0, or -1
// (LK_ERR_ARG) / -2 (LK_ERR_UNSUPPORTED) with the reason in `err`.
int parse_formula(const std::string& text, const std::vector<std::string>& names, FxProgram& out, std::string& err);

// The program as text, one token per operation: `$<leaf>`, a constant as Java prints it, `+ - * /`.
std::string formula_program_text(const FxProgram& p);

}  // namespace lk
