// Instantiations of the gfx950 kernels for MaxLoc / MinLoc over the 16-byte
// (value, index) pairs { double, int64 } and { int64, int64 } (dtypes 16 / 17;
// the rule: rdc_common.h RDC_OP_MAXLOC).  Reached through pick_maxloc /
// pick_minloc (rdc_kernels_loc.hip).
#include "rdc_kernels_impl.h"

namespace rdc_amd {
bool pick_maxloc16(int dtype, KernelSet* ks) { return pick_loc16<RDC_OP_MAXLOC>(dtype, ks); }
bool pick_minloc16(int dtype, KernelSet* ks) { return pick_loc16<RDC_OP_MINLOC>(dtype, ks); }
}  // namespace rdc_amd
