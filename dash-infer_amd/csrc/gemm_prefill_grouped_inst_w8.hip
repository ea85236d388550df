// explicit instantiations: grouped context-phase GEMM of the mixture-of-experts block (gemm_prefill_kernel.hpp, GROUPED), W8
#include "gemm_prefill_kernel.hpp"
namespace dihip {
DIHIP_DEFINE_PREFILL_GROUPED_LAUNCH_SET(8)
}  // namespace dihip
