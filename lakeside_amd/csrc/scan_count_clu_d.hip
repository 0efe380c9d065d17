// scan_clu instantiation for AGG_COUNT, dense tables (see scan_inst.hpp).
#define LK_INST_CLU
#include "scan_inst.hpp"

namespace lk {
template void launch_clu<AGG_COUNT>(const QParams& P, dim3 grid, hipStream_t st);
}  // namespace lk
