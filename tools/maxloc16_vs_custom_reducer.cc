// The arg-max of a buffer of 16-byte (value, index) pairs two ways, one process
// per rank: rdc::Allreduce<op::MaxLoc>(ValueIndex<double>*) on a DEVICE buffer
// (the gfx950 kernels, dtype 16) and rdc::Reducer<Plain, f>::Allreduce on a
// HOST copy of the same input, Plain a plain { double, int64_t } struct and f
// restating the MaxLoc rule — what a caller with float64 scores or indexes
// beyond int32 had to write before the 16-byte pairs existed (the custom-reducer
// path: chunks over point-to-point, the user's function on the host).
//
//   maxloc16_vs_custom_reducer <MiB> <rounds> [key=val ...]   (RDC_RANK / rdc_world_size / tracker keys)
//
// Rounds alternate the two forms; the input is restored before every call
// (not timed).  Prints one JSON line per rank: the median and min / max ms per
// call of each form.  The two results must be equal byte for byte in every
// round, else exit 1.  Scores differ below float32's precision and the indexes
// lie beyond int32, so the 8-byte pairs could not carry this input.
//
// Build (one line):
//   g++ -O2 -std=c++11 -I include tools/maxloc16_vs_custom_reducer.cc -o tools/maxloc16_vs_custom_reducer
//       -L rdc_amd -lrdc_amd -L $ROCM_PATH/lib -lamdhip64 -Wl,-rpath,$PWD/rdc_amd -Wl,-rpath,$ROCM_PATH/lib
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "rdc.h"

extern "C" int hipMalloc(void** ptr, size_t size);
extern "C" int hipFree(void* ptr);

typedef rdc::ValueIndex<double> P;
struct Plain {  // the host reducer's element: the same 16 bytes, no library type
    double value;
    int64_t index;
};
static_assert(sizeof(Plain) == sizeof(P), "one layout");

static void f_maxloc(Plain& dst, const Plain& src) {  // NOLINT(*)
    if (dst.value < src.value || (dst.value == src.value && src.index < dst.index)) dst = src;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s <MiB> <rounds> [key=val ...]\n", argv[0]);
        return 2;
    }
    const size_t mib = (size_t)atol(argv[1]);
    const int rounds = atoi(argv[2]);
    rdc::Init(argc - 3, argv + 3);
    const int r = rdc::GetRank(), n = rdc::GetWorldSize();
    const size_t N = mib * (1u << 20) / sizeof(P);
    std::vector<P> in(N), got(N);
    std::vector<Plain> host(N);
    uint64_t s = 0x9E3779B97F4A7C15ull * (uint64_t)(r + 1);
    for (size_t i = 0; i < N; ++i) {
        // scores from a small set, so ranks tie, some apart by 2^-40 only (equal as float32); the
        // index is a global row id beyond int32: rank * 2^33 + i
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const int k = (int)((s >> 40) % 17);
        in[i].value = (double)(k / 2) - 4.0 + (k % 2) * 9.094947017729282e-13;
        in[i].index = ((int64_t)r << 33) + (int64_t)i;
    }
    void* dev = nullptr;
    if (hipMalloc(&dev, N * sizeof(P)) != 0) {
        fprintf(stderr, "rank %d: hipMalloc failed\n", r);
        return 1;
    }
    rdc::Reducer<Plain, f_maxloc> red;
    std::vector<double> ms_dev, ms_host;
    for (int it = 0; it < rounds + 1; ++it) {
        rdc::detail::Check(RdcMemcpy(dev, in.data(), N * sizeof(P)), "upload");
        rdc::Barrier();
        auto t0 = std::chrono::steady_clock::now();
        rdc::Allreduce<rdc::op::MaxLoc>(static_cast<P*>(dev), (uint64_t)N);
        const double d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        memcpy(host.data(), in.data(), N * sizeof(P));
        rdc::Barrier();
        t0 = std::chrono::steady_clock::now();
        red.Allreduce(host.data(), N);
        const double h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (it > 0) {  // the first round is a warm-up (engines, slots, registration)
            ms_dev.push_back(d);
            ms_host.push_back(h);
        }
        rdc::detail::Check(RdcMemcpy(got.data(), dev, N * sizeof(P)), "download");
        if (memcmp(got.data(), host.data(), N * sizeof(P)) != 0) {
            fprintf(stderr, "rank %d: round %d: the device MaxLoc and the host reducer differ\n", r, it);
            return 1;
        }
    }
    std::sort(ms_dev.begin(), ms_dev.end());
    std::sort(ms_host.begin(), ms_host.end());
    printf("{\"rank\": %d, \"n\": %d, \"MiB\": %zu, \"rounds\": %d, \"device_maxloc_median_ms\": %.3f, "
           "\"device_maxloc_min_max_ms\": [%.3f, %.3f], \"host_custom_reducer_median_ms\": %.3f, "
           "\"host_custom_reducer_min_max_ms\": [%.3f, %.3f], \"equal_bytes\": true}\n",
           r, n, mib, rounds, ms_dev[ms_dev.size() / 2], ms_dev.front(), ms_dev.back(), ms_host[ms_host.size() / 2],
           ms_host.front(), ms_host.back());
    hipFree(dev);
    rdc::Finalize();
    return 0;
}
