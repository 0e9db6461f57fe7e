// Host-visible launchers of the gfx950 kernels (rdc_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "rdc_common.h"
#include "rdc_plan.h"

namespace rdc_amd {

struct KernelSet {
    hipError_t (*reduce)(char* dst, const char* src, uint64_t nbytes, int grid, hipStream_t s);
    hipError_t (*mesh)(const CollArgs& a, int grid, hipStream_t s);
    hipError_t (*ring)(const CollArgs& a, int grid, hipStream_t s);
    hipError_t (*oneshot)(const CollArgs& a, int grid, hipStream_t s);
    hipError_t (*tree)(const CollArgs& a, int grid, hipStream_t s);
    hipError_t (*direct)(const CollArgs& a, int grid, hipStream_t s);  // registered user buffers (k_direct)
    // in-place reduce-scatter (chunk r of the reduction on rank r, every other byte untouched):
    hipError_t (*rscatter)(const CollArgs& a, int grid, hipStream_t s);         // scratch schedule (k_rscatter)
    hipError_t (*rscatter_direct)(const CollArgs& a, int grid, hipStream_t s);  // registered buffers (k_rscatter_direct)
    // in-place reduction to rank a.root, every other rank's buffer untouched (k_rooted, scratch schedule)
    hipError_t (*rooted)(const CollArgs& a, int grid, hipStream_t s);
    // in-place prefix reduction across ranks (Scan; a.pull = 1: Exscan), rank 0's buffer untouched (k_scan)
    hipError_t (*scan)(const CollArgs& a, int grid, hipStream_t s);
    hipError_t (*svc)(const SvcArgs& a, hipStream_t s);  // the small-allreduce service (one block)
    // resident blocks per CU of the kernel a launch of `kind` (RDC_KIND_MESH /
    // RING / ONESHOT / TREE / DIRECT / RSCATTER / RSCATTER_DIRECT / ROOTED / SCAN) on n ranks uses (hipOccupancyMaxActiveBlocksPerMultiprocessor,
    // cached); the grid clamp of ResidentGrid (rdc_plan.h)
    int (*occupancy)(int kind, int n);
};

// false if (dtype, op) is not a valid reference combination
bool get_kernels(int dtype, int op, KernelSet* ks);
// The folds of the mesh family that are no RDC_OP_* operator
// (rdc_kernels_fold.hip): kAcc32, the float32-accumulated Sum of float16 /
// bfloat16; kAvg, the mean across ranks of float32 / float64 / float16 /
// bfloat16.
enum class MeshFold { kAcc32, kAvg };
// fills mesh, rscatter, rooted and occupancy, every other member is null;
// false for a dtype the fold does not take
bool get_kernels_fold(MeshFold fold, int dtype, KernelSet* ks);
// resident blocks per CU of k_bcast / k_allgather / k_alltoall
int occupancy_bcast();
int occupancy_allgather();
int occupancy_alltoall();
hipError_t launch_bcast(const CollArgs& a, int grid, hipStream_t s);
hipError_t launch_allgather(const CollArgs& a, int grid, hipStream_t s);
// all-to-all: nb_scatter push blocks + nb_gather land blocks (rdc_plan.h PlanAlltoall)
hipError_t launch_alltoall(const CollArgs& a, int grid, hipStream_t s);
// coalesced allreduce: units[i].buf = user address; unpack = image -> buffers
hipError_t launch_pack(const PackUnit* units, int nunits, char* image, int unpack, int grid, hipStream_t s);
// plain device copy (dst may be IPC-mapped peer memory); never waits.
// With `word` (host-mapped): the last block to finish stores `value` there
// (system-scope release, after every block's system fence); `arrive` is a
// zeroed device counter owned by the stream (reset by that last block).
hipError_t launch_copy(void* dst, const void* src, uint64_t bytes, hipStream_t s, uint32_t* arrive = nullptr,
                       uint64_t* word = nullptr, uint64_t value = 0);
// xGMI probe: block b copies its share of `bytes` from src (or srcs[b % ndst]
// when set: remote reads) into dsts[b % ndst]
struct PushTargets {
    char* dst[RDC_MAX_RANKS];
    const char* src[RDC_MAX_RANKS];
};
hipError_t launch_push(const PushTargets& t, int ndst, const void* src, uint64_t bytes, int grid, hipStream_t s);
hipError_t launch_fill(void* buf, uint64_t count, int dtype, uint64_t seed, int rank, hipStream_t s);

}  // namespace rdc_amd
