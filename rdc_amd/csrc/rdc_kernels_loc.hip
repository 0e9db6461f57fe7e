// Instantiations of the gfx950 kernels for MaxLoc / MinLoc over (value, index)
// pairs (MPI_MAXLOC / MPI_MINLOC; the rule: rdc_common.h RDC_OP_MAXLOC).
#include "rdc_kernels_impl.h"

namespace rdc_amd {
bool pick_maxloc(int dtype, KernelSet* ks) { return pick_loc<RDC_OP_MAXLOC>(dtype, ks); }
bool pick_minloc(int dtype, KernelSet* ks) { return pick_loc<RDC_OP_MINLOC>(dtype, ks); }
}  // namespace rdc_amd
