// Instantiations of the gfx950 kernels for BitXOR (MPI_BXOR; integer types only, as BitOR).
#include "rdc_kernels_impl.h"

namespace rdc_amd {
bool pick_bitxor(int dtype, KernelSet* ks) { return pick_int<RDC_OP_BITXOR>(dtype, ks); }
}  // namespace rdc_amd
