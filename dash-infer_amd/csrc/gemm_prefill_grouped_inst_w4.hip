// explicit instantiations: grouped context-phase GEMM of the mixture-of-experts block (gemm_prefill_kernel.hpp, GROUPED), W4
#include "gemm_prefill_kernel.hpp"
namespace dihip {
DIHIP_DEFINE_PREFILL_GROUPED_LAUNCH_SET(4)
}  // namespace dihip
