// Instantiations of the gfx950 kernels for BitAND (MPI_BAND; integer types only, as BitOR).
#include "rdc_kernels_impl.h"

namespace rdc_amd {
bool pick_bitand(int dtype, KernelSet* ks) { return pick_int<RDC_OP_BITAND>(dtype, ks); }
}  // namespace rdc_amd
