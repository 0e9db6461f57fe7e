// Instantiations of the gfx950 kernels for MaxLoc / MinLoc over (value, index)
// pairs (MPI_MAXLOC / MPI_MINLOC; the rule: rdc_common.h RDC_OP_MAXLOC).
// The 8-byte pairs here; the 16-byte ones in rdc_kernels_loc16.hip.
#include "rdc_kernels_impl.h"

namespace rdc_amd {
bool pick_maxloc16(int dtype, KernelSet* ks);
bool pick_minloc16(int dtype, KernelSet* ks);
bool pick_maxloc(int dtype, KernelSet* ks) { return pick_loc<RDC_OP_MAXLOC>(dtype, ks) || pick_maxloc16(dtype, ks); }
bool pick_minloc(int dtype, KernelSet* ks) { return pick_loc<RDC_OP_MINLOC>(dtype, ks) || pick_minloc16(dtype, ks); }
}  // namespace rdc_amd
