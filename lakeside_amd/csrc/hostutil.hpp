// Host-only helpers of the evaluator's translation units (never included by device code).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "plan.hpp"

#define HIP_TRY(x)                                                                              \
  do {                                                                                          \
    hipError_t _e = (x);                                                                        \
    if (_e != hipSuccess)                                                                       \
      throw PlanError(LK_ERR_DEVICE, std::string("HIP: ") + #x + ": " + hipGetErrorString(_e)); \
  } while (0)

namespace lk {

inline std::string json_escape(const std::string& s) {
  std::string o;
  for (char c : s) {
    if (c == '"' || c == '\\') o += '\\';
    if (static_cast<unsigned char>(c) < 0x20) {
      char b[8];
      snprintf(b, sizeof(b), "\\u%04x", unsigned(static_cast<unsigned char>(c)));
      o += b;
    } else {
      o += c;
    }
  }
  return o;
}

}  // namespace lk
