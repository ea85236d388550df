// explicit instantiations: int8 x int8 context-phase GEMM (gemm_a8w8_kernel.hpp), bf16 outputs
#include "gemm_a8w8_kernel.hpp"
namespace dihip {
DIHIP_DEFINE_A8W8_LAUNCH_SET(DIHIP_BF16)
}  // namespace dihip
