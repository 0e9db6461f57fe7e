// rdc::Allreduce<op::Prod>(float*, N) and rdc::Allreduce<op::BitXOR>(uint32_t*,
// N) on a DEVICE buffer against rdc::Reducer<T, f>::Allreduce on a host copy of
// the same input, f the plain `dst *= src` / `dst ^= src`: the device kernels
// against the reference-order host path (ICommunicator::Allreduce(Buffer,
// ReduceFunction)), byte for byte.  Floats have random signs and magnitudes in
// [0.5, 2) with full mantissas, so every product rounds and none is NaN or
// inf; the order of a float product decides its bits, as for a sum.  Then
// ReduceScatter / ReduceTo / Scan of the same device input.
// argv: N
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rdc.h"

extern "C" int hipMalloc(void** ptr, size_t size);
extern "C" int hipFree(void* ptr);

static void f_mul(float& dst, const float& src) { dst *= src; }          // NOLINT(*)
static void f_xor(uint32_t& dst, const uint32_t& src) { dst ^= src; }    // NOLINT(*)

static uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static void fill(std::vector<float>& x, int rank, uint64_t seed) {
    for (size_t i = 0; i < x.size(); ++i) {
        const uint64_t u = mix(seed ^ ((uint64_t)rank << 40) ^ i);
        // sign | exponent 126 or 127 | 23 random mantissa bits
        const uint32_t bits = ((uint32_t)(u >> 63) << 31) | ((126u + (uint32_t)((u >> 62) & 1)) << 23) |
                              (uint32_t)(u & 0x7fffffu);
        memcpy(&x[i], &bits, 4);
    }
}
static void fill(std::vector<uint32_t>& x, int rank, uint64_t seed) {
    for (size_t i = 0; i < x.size(); ++i) x[i] = (uint32_t)mix(seed ^ ((uint64_t)rank << 40) ^ i);
}

template <typename OP, typename T, void (*F)(T&, const T&)>
static int run(int N, int R, int W, uint64_t seed, const char* name) {
    std::vector<T> in((size_t)N), host, got((size_t)N);
    fill(in, R, seed);
    host = in;
    void* dev = nullptr;
    if (hipMalloc(&dev, (size_t)N * sizeof(T)) != 0) {
        fprintf(stderr, "rank %d: hipMalloc failed\n", R);
        return 1;
    }
    T* d = static_cast<T*>(dev);
    auto upload = [&] { rdc::detail::Check(RdcMemcpy(d, in.data(), (size_t)N * sizeof(T)), "upload"); };
    auto download = [&] { rdc::detail::Check(RdcMemcpy(got.data(), d, (size_t)N * sizeof(T)), "download"); };
    rdc::Reducer<T, F> red;
    red.Allreduce(host.data(), (size_t)N);
    for (int i = 0; i < N; ++i)
        if (host[(size_t)i] != host[(size_t)i] || host[(size_t)i] - host[(size_t)i] != 0) {
            fprintf(stderr, "rank %d: %s expected data holds a NaN or an inf\n", R, name);
            return 1;
        }
    upload();
    rdc::Allreduce<OP>(d, (uint64_t)N);
    download();
    if (memcmp(got.data(), host.data(), (size_t)N * sizeof(T)) != 0) {
        for (int i = 0; i < N; ++i)
            if (memcmp(&got[(size_t)i], &host[(size_t)i], sizeof(T)) != 0) {
                fprintf(stderr, "rank %d: %s element %d is %.9g, the host reducer gives %.9g\n", R, name, i,
                        (double)got[(size_t)i], (double)host[(size_t)i]);
                break;
            }
        return 1;
    }
    // reduce-scatter: this rank's chunk holds the allreduce's bytes, the rest its input
    upload();
    const std::pair<uint64_t, uint64_t> ch = rdc::ReduceScatter<OP>(d, (uint64_t)N);
    download();
    for (uint64_t i = 0; i < (uint64_t)N; ++i) {
        const T& want = (i >= ch.first && i < ch.second) ? host[i] : in[i];
        if (memcmp(&got[i], &want, sizeof(T)) != 0) {
            fprintf(stderr, "rank %d: %s reduce-scatter element %llu differs\n", R, name, (unsigned long long)i);
            return 1;
        }
    }
    // rooted reduce: the root holds the allreduce's bytes, the others their input
    upload();
    rdc::ReduceTo<OP>(d, (uint64_t)N, W - 1);
    download();
    if (memcmp(got.data(), R == W - 1 ? host.data() : in.data(), (size_t)N * sizeof(T)) != 0) {
        fprintf(stderr, "rank %d: %s ReduceTo differs\n", R, name);
        return 1;
    }
    // scan: y[q] = f(dst = y[q-1], src = x[q]) over every rank's input, restated here
    upload();
    rdc::Scan<OP>(d, (uint64_t)N);
    download();
    std::vector<T> y((size_t)N), xq((size_t)N);
    fill(y, 0, seed);
    for (int q = 1; q <= R; ++q) {
        fill(xq, q, seed);
        for (int i = 0; i < N; ++i) F(y[(size_t)i], xq[(size_t)i]);
    }
    if (memcmp(got.data(), y.data(), (size_t)N * sizeof(T)) != 0) {
        fprintf(stderr, "rank %d: %s Scan differs\n", R, name);
        return 1;
    }
    hipFree(dev);
    return 0;
}

int main(int argc, char* argv[]) {
    rdc::Init(argc, argv);
    rdc::NewCommunicator(rdc::kMainCommName);
    const int N = argc >= 2 ? atoi(argv[1]) : 7;
    const int W = rdc::GetWorldSize(), R = rdc::GetRank();
    if (run<rdc::op::Prod, float, f_mul>(N, R, W, 0x0B50001ull, "Prod")) return 1;
    if (run<rdc::op::BitXOR, uint32_t, f_xor>(N, R, W, 0x0B50002ull, "BitXOR")) return 1;
    printf("rank %d: prod and bitxor OK (world %d, N %d)\n", R, W, N);
    rdc::Finalize();
    return 0;
}
