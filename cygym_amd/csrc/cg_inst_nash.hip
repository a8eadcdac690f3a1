// cg_inst_nash.hip -- the instantiation unit of the support enumeration (cg_nash.hpp): nash_enum_kernel<K>, one kernel per support
// size K = 1 .. 16 (the K x (K + 1) system of a pair lives in registers under compile-time indices).
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_aux_kernels.hpp"   // (without CG_MAIN_UNIT: the templates, none of the plain kernels)
#define CG_INST(K) template __global__ void nash_enum_kernel<K>(cygym_nash_desc, NashLaunch);
CG_INST(1) CG_INST(2) CG_INST(3) CG_INST(4) CG_INST(5) CG_INST(6) CG_INST(7) CG_INST(8)
CG_INST(9) CG_INST(10) CG_INST(11) CG_INST(12) CG_INST(13) CG_INST(14) CG_INST(15) CG_INST(16)
#undef CG_INST
}  // namespace cygym_k
