// rdc::Allreduce<op::MaxLoc / op::MinLoc>(ValueIndex<double>*, N) on a DEVICE
// buffer against rdc::Reducer<ValueIndex<double>, f>::Allreduce on a host copy
// of the same input, f restating the rule: the device kernels of the 16-byte
// pairs against the reference-order host path, byte for byte.  Values come from
// ten (two doubles equal as float32, two that differ in the high dword only,
// NaN, -0, +0, +-inf and +-max among them) and indexes from seven (beyond
// int32, INT64_MIN / MAX, negative), so ranks collide in both.  Then
// ReduceScatter / ReduceTo / Scan of the same device input against that result
// where it applies.
// argv: N
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "rdc.h"

extern "C" int hipMalloc(void** ptr, size_t size);
extern "C" int hipFree(void* ptr);

typedef rdc::ValueIndex<double> P;
static_assert(sizeof(P) == 16 && alignof(P) == 16, "the 16-byte pair");

static void f_max(P& dst, const P& src) {  // NOLINT(*)
    if (dst.value < src.value || (dst.value == src.value && src.index < dst.index)) dst = src;
}
static void f_min(P& dst, const P& src) {  // NOLINT(*)
    if (dst.value > src.value || (dst.value == src.value && src.index < dst.index)) dst = src;
}

static uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static void fill(std::vector<P>& x, int rank, uint64_t seed) {
    const double inf = std::numeric_limits<double>::infinity(), mx = std::numeric_limits<double>::max();
    const double vals[10] = {1.0, 1.0 + 9.094947017729282e-13 /* 2^-40 */, 2.0, -0.0, 0.0,
                             std::numeric_limits<double>::quiet_NaN(), inf, mx, -inf, -mx};
    const int64_t idx[7] = {(int64_t)1 << 32, 0, (int64_t)1 << 31, 1, -5, INT64_MIN, INT64_MAX};
    for (size_t i = 0; i < x.size(); ++i) {
        const uint64_t u = mix(seed ^ ((uint64_t)rank << 40) ^ i);
        x[i].value = vals[u % 10];
        x[i].index = idx[(u >> 8) % 7];
    }
}

template <typename OP, void (*F)(P&, const P&)>
static int run(int N, int R, int W, uint64_t seed, const char* name) {
    std::vector<P> in((size_t)N), host, got((size_t)N);
    fill(in, R, seed);
    host = in;
    void* dev = nullptr;
    if (hipMalloc(&dev, (size_t)N * sizeof(P)) != 0) {
        fprintf(stderr, "rank %d: hipMalloc failed\n", R);
        return 1;
    }
    P* d = static_cast<P*>(dev);
    auto upload = [&] { rdc::detail::Check(RdcMemcpy(d, in.data(), (size_t)N * sizeof(P)), "upload"); };
    auto download = [&] { rdc::detail::Check(RdcMemcpy(got.data(), d, (size_t)N * sizeof(P)), "download"); };
    rdc::Reducer<P, F> red;
    red.Allreduce(host.data(), (size_t)N);
    upload();
    rdc::Allreduce<OP>(d, (uint64_t)N);
    download();
    if (memcmp(got.data(), host.data(), (size_t)N * sizeof(P)) != 0) {
        for (int i = 0; i < N; ++i)
            if (memcmp(&got[(size_t)i], &host[(size_t)i], sizeof(P)) != 0) {
                fprintf(stderr, "rank %d: %s element %d is (%.17g, %lld), the host reducer gives (%.17g, %lld)\n", R, name,
                        i, got[(size_t)i].value, (long long)got[(size_t)i].index, host[(size_t)i].value,
                        (long long)host[(size_t)i].index);
                break;
            }
        return 1;
    }
    // a typed Buffer takes the same kernels
    upload();
    rdc::Buffer b(dev, (uint64_t)N * sizeof(P));
    b.set_type<P>();
    rdc::Allreduce<OP>(b);
    download();
    if (memcmp(got.data(), host.data(), (size_t)N * sizeof(P)) != 0) {
        fprintf(stderr, "rank %d: %s Allreduce(Buffer&) differs\n", R, name);
        return 1;
    }
    // reduce-scatter: this rank's chunk holds the allreduce's bytes, the rest its input
    upload();
    const std::pair<uint64_t, uint64_t> ch = rdc::ReduceScatter<OP>(d, (uint64_t)N);
    download();
    for (uint64_t i = 0; i < (uint64_t)N; ++i) {
        const P& want = (i >= ch.first && i < ch.second) ? host[i] : in[i];
        if (memcmp(&got[i], &want, sizeof(P)) != 0) {
            fprintf(stderr, "rank %d: %s reduce-scatter element %llu differs\n", R, name, (unsigned long long)i);
            return 1;
        }
    }
    // rooted reduce: the root holds the allreduce's bytes, the others their input
    upload();
    rdc::ReduceTo<OP>(d, (uint64_t)N, W - 1);
    download();
    if (memcmp(got.data(), R == W - 1 ? host.data() : in.data(), (size_t)N * sizeof(P)) != 0) {
        fprintf(stderr, "rank %d: %s ReduceTo differs\n", R, name);
        return 1;
    }
    // scan: y[q] = f(dst = y[q-1], src = x[q]) over every rank's input, restated here
    upload();
    rdc::Scan<OP>(d, (uint64_t)N);
    download();
    std::vector<P> y((size_t)N), xq((size_t)N);
    fill(y, 0, seed);
    for (int q = 1; q <= R; ++q) {
        fill(xq, q, seed);
        for (int i = 0; i < N; ++i) F(y[(size_t)i], xq[(size_t)i]);
    }
    if (memcmp(got.data(), y.data(), (size_t)N * sizeof(P)) != 0) {
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
    if (run<rdc::op::MaxLoc, f_max>(N, R, W, 0x10C1601ull, "MaxLoc")) return 1;
    if (run<rdc::op::MinLoc, f_min>(N, R, W, 0x10C1602ull, "MinLoc")) return 1;
    printf("rank %d: maxloc16 and minloc16 OK (world %d, N %d)\n", R, W, N);
    rdc::Finalize();
    return 0;
}
