// Instantiations of the mesh family (k_mesh, k_rscatter, k_rooted) for Avg,
// the mean across ranks of float32 / float64 / float16 / bfloat16 buffers (the
// rule: include/rdc_amd.h RdcAllreduceAvg; the fold and the division:
// rdc_device.h avg / acc32, mesh_fold_elem / mesh_reduce_range).  Reached
// through get_kernels_avg only: kOpAvg is no RDC_OP_* code and get_kernels
// never sees it.
#include "rdc_kernels_impl.h"

namespace rdc_amd {
namespace {

template <typename T>
struct AvgKernels {
    static hipError_t mesh(const CollArgs& a, int grid, hipStream_t s) {
        if (a.n <= 8)
            hipLaunchKernelGGL((k_mesh<kOpAvg, T, 8>), dim3(grid), dim3(kBlock), debug_lds_pad(), s, a);
        else
            hipLaunchKernelGGL((k_mesh<kOpAvg, T, 16>), dim3(grid), dim3(kBlock), debug_lds_pad(), s, a);
        return hipGetLastError();
    }
    static hipError_t rscatter(const CollArgs& a, int grid, hipStream_t s) {
        if (a.n <= 8)
            hipLaunchKernelGGL((k_rscatter<kOpAvg, T, 8>), dim3(grid), dim3(kBlock), debug_lds_pad(), s, a);
        else
            hipLaunchKernelGGL((k_rscatter<kOpAvg, T, 16>), dim3(grid), dim3(kBlock), debug_lds_pad(), s, a);
        return hipGetLastError();
    }
    static hipError_t rooted(const CollArgs& a, int grid, hipStream_t s) {
        if (a.n <= 8)
            hipLaunchKernelGGL((k_rooted<kOpAvg, T, 8>), dim3(grid), dim3(kBlock), debug_lds_pad(), s, a);
        else
            hipLaunchKernelGGL((k_rooted<kOpAvg, T, 16>), dim3(grid), dim3(kBlock), debug_lds_pad(), s, a);
        return hipGetLastError();
    }
    // as Kernels<OP, T>::occupancy, over the three kernels this unit has
    static int occupancy(int kind, int n) {
        // [mesh 8, mesh 16, rscatter 8, rscatter 16, rooted 8, rooted 16]; 0 = not queried yet
        static int cache[6] = {0, 0, 0, 0, 0, 0};
        const int wide = n > 8 ? 1 : 0;
        const int slot = kind == RDC_KIND_RSCATTER ? 2 + wide : kind == RDC_KIND_ROOTED ? 4 + wide : wide;
        if (cache[slot] > 0) return cache[slot];
        int b = 0;
        hipError_t e = hipSuccess;
        switch (slot) {
            case 0: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_mesh<kOpAvg, T, 8>, kBlock, debug_lds_pad()); break;
            case 1: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_mesh<kOpAvg, T, 16>, kBlock, debug_lds_pad()); break;
            case 2: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_rscatter<kOpAvg, T, 8>, kBlock, debug_lds_pad()); break;
            case 3: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_rscatter<kOpAvg, T, 16>, kBlock, debug_lds_pad()); break;
            case 4: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_rooted<kOpAvg, T, 8>, kBlock, debug_lds_pad()); break;
            default: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_rooted<kOpAvg, T, 16>, kBlock, debug_lds_pad()); break;
        }
        if (e != hipSuccess || b <= 0) {
            (void)hipGetLastError();
            b = 1;  // unknown: one block per CU is always resident
        }
        cache[slot] = b;
        return b;
    }
};

template <typename T>
void set_avg(KernelSet* ks) {
    *ks = KernelSet();  // every other member null: never called on this path
    ks->mesh = &AvgKernels<T>::mesh;
    ks->rscatter = &AvgKernels<T>::rscatter;
    ks->rooted = &AvgKernels<T>::rooted;
    ks->occupancy = &AvgKernels<T>::occupancy;
}

}  // namespace

bool get_kernels_avg(int dtype, KernelSet* ks) {
    switch (dtype) {
        case RDC_DT_FLOAT32: set_avg<float>(ks); return true;
        case RDC_DT_FLOAT64: set_avg<double>(ks); return true;
        case RDC_DT_FLOAT16: set_avg<_Float16>(ks); return true;
        case RDC_DT_BFLOAT16: set_avg<bf16_t>(ks); return true;
        default: return false;
    }
}

}  // namespace rdc_amd
