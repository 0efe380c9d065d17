// scan_clu instantiation for AGG_MIN, dense tables (see scan_inst.hpp).
#define LK_INST_CLU
#include "scan_inst.hpp"

namespace lk {
template void launch_clu<AGG_MIN>(const QParams& P, dim3 grid, hipStream_t st);
}  // namespace lk
