// Instantiations of the mesh family (k_mesh, k_rscatter, k_rooted) for the
// folds that are no RDC_OP_* operator (the rules: include/rdc_amd.h
// RdcAllreduceAcc32 / RdcAllreduceAvg; the arithmetic: rdc_device.h acc32 /
// avg, mesh_fold_elem / mesh_reduce_range).  Reached through get_kernels_fold
// only: get_kernels never sees kOpSumAcc32 or kOpAvg.
#include "rdc_kernels_impl.h"

namespace rdc_amd {

bool get_kernels_fold(MeshFold fold, int dtype, KernelSet* ks) {
    switch (fold) {
        case MeshFold::kAcc32:  // the float32-accumulated Sum
            switch (dtype) {
                case RDC_DT_FLOAT16: return MeshFamilyKernels<kOpSumAcc32, _Float16>::fill(ks);
                case RDC_DT_BFLOAT16: return MeshFamilyKernels<kOpSumAcc32, bf16_t>::fill(ks);
                default: return false;
            }
        case MeshFold::kAvg:  // the mean across ranks
            switch (dtype) {
                case RDC_DT_FLOAT32: return MeshFamilyKernels<kOpAvg, float>::fill(ks);
                case RDC_DT_FLOAT64: return MeshFamilyKernels<kOpAvg, double>::fill(ks);
                case RDC_DT_FLOAT16: return MeshFamilyKernels<kOpAvg, _Float16>::fill(ks);
                case RDC_DT_BFLOAT16: return MeshFamilyKernels<kOpAvg, bf16_t>::fill(ks);
                default: return false;
            }
    }
    return false;
}

}  // namespace rdc_amd
