// Instantiations of the gfx950 kernels for Prod (MPI_PROD; every arithmetic type; the rule and its numerics: rdc_common.h RDC_OP_PROD).
#include "rdc_kernels_impl.h"

namespace rdc_amd {
bool pick_prod(int dtype, KernelSet* ks) { return pick_arith<RDC_OP_PROD>(dtype, ks); }
}  // namespace rdc_amd
