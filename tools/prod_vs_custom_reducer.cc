// The product of a float buffer across ranks two ways, one process per rank:
// rdc::Allreduce<op::Prod>(float*) on a DEVICE buffer (the gfx950 kernels) and
// rdc::Reducer<float, f>::Allreduce on a HOST copy of the same input (the
// custom-reducer path: chunks over point-to-point, the user's function on the
// host), f being `dst *= src`.
//
//   prod_vs_custom_reducer <MiB> <rounds> [key=val ...]   (RDC_RANK / rdc_world_size / tracker keys)
//
// Rounds alternate the two forms; the input is restored before every call
// (not timed).  Prints one JSON line per rank: the median and min / max ms per
// call of each form.  The two results must be equal byte for byte, else exit 1.
//
// Build (one line):
//   g++ -O2 -std=c++11 -I include tools/prod_vs_custom_reducer.cc -o tools/prod_vs_custom_reducer
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

static void f_mul(float& dst, const float& src) { dst *= src; }  // NOLINT(*)

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s <MiB> <rounds> [key=val ...]\n", argv[0]);
        return 2;
    }
    const size_t mib = (size_t)atol(argv[1]);
    const int rounds = atoi(argv[2]);
    rdc::Init(argc - 3, argv + 3);
    const int r = rdc::GetRank(), n = rdc::GetWorldSize();
    const size_t N = mib * (1u << 20) / sizeof(float);
    std::vector<float> in(N), host(N), got(N);
    uint64_t s = 0x9E3779B97F4A7C15ull * (uint64_t)(r + 1);
    for (size_t i = 0; i < N; ++i) {  // random sign, magnitude in [0.5, 2), full mantissa: every product rounds
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t bits = ((uint32_t)(s >> 63) << 31) | ((126u + (uint32_t)((s >> 62) & 1)) << 23) |
                              (uint32_t)((s >> 20) & 0x7fffffu);
        memcpy(&in[i], &bits, 4);
    }
    void* dev = nullptr;
    if (hipMalloc(&dev, N * sizeof(float)) != 0) {
        fprintf(stderr, "rank %d: hipMalloc failed\n", r);
        return 1;
    }
    rdc::Reducer<float, f_mul> red;
    std::vector<double> ms_dev, ms_host;
    for (int it = 0; it < rounds + 1; ++it) {
        rdc::detail::Check(RdcMemcpy(dev, in.data(), N * sizeof(float)), "upload");
        rdc::Barrier();
        auto t0 = std::chrono::steady_clock::now();
        rdc::Allreduce<rdc::op::Prod>(static_cast<float*>(dev), (uint64_t)N);
        const double d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        host = in;
        rdc::Barrier();
        t0 = std::chrono::steady_clock::now();
        red.Allreduce(host.data(), N);
        const double h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (it > 0) {  // the first round is a warm-up (engines, slots, registration)
            ms_dev.push_back(d);
            ms_host.push_back(h);
        }
        rdc::detail::Check(RdcMemcpy(got.data(), dev, N * sizeof(float)), "download");
        if (memcmp(got.data(), host.data(), N * sizeof(float)) != 0) {
            fprintf(stderr, "rank %d: round %d: the device Prod and the host reducer differ\n", r, it);
            return 1;
        }
    }
    std::sort(ms_dev.begin(), ms_dev.end());
    std::sort(ms_host.begin(), ms_host.end());
    printf("{\"rank\": %d, \"n\": %d, \"MiB\": %zu, \"rounds\": %d, \"device_prod_median_ms\": %.3f, "
           "\"device_prod_min_max_ms\": [%.3f, %.3f], \"host_custom_reducer_median_ms\": %.3f, "
           "\"host_custom_reducer_min_max_ms\": [%.3f, %.3f], \"equal_bytes\": true}\n",
           r, n, mib, rounds, ms_dev[ms_dev.size() / 2], ms_dev.front(), ms_dev.back(), ms_host[ms_host.size() / 2],
           ms_host.front(), ms_host.back());
    hipFree(dev);
    rdc::Finalize();
    return 0;
}
