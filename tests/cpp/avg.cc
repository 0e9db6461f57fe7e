// Known-answer program for rdc::AllreduceAvg / ReduceScatterAvg / ReduceToAvg
// (include/rdc.h): the mean across ranks, divided where the result is
// produced.  float16: every rank holds 40000.0, whose Sum overflows float16 at
// two ranks already while the mean is 40000.0 exactly.  double / float: rank r
// holds 1.5 * (r + 1), so the sum 0.75 * W * (W + 1) and the mean
// 0.75 * (W + 1) are exact.  bfloat16: rank 0 holds 384, every other rank 0,
// so the mean is the one rounding of 384.0f / W.  All inside guarded arrays.
// argv: N root
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rdc.h"

namespace {
const uint16_t kF16_40000 = 0x78E2;  // 2^15 * (1 + 226 / 1024)
const uint16_t kBF16_384 = 0x43C0;   // 2^8 * 1.5

// round-to-nearest-even of a finite float to bfloat16 bits
uint16_t bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

template <typename T> bool is_guard(const T& v) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
    for (size_t i = 0; i < sizeof(T); ++i)
        if (p[i] != 0xA5) return false;
    return true;
}

// N elements between G guard elements of 0xA5 bytes on either side
template <typename T> struct Guarded {
    std::vector<T> backing;
    int G, N;
    Guarded(int g, int n) : backing((size_t)(n + 2 * g)), G(g), N(n) {
        memset(backing.data(), 0xA5, backing.size() * sizeof(T));
    }
    T* data() { return backing.data() + G; }
    bool ok(int R, const char* what) const {
        for (int i = 0; i < G; ++i) {
            if (!is_guard(backing[(size_t)i]) || !is_guard(backing[(size_t)(G + N + i)])) {
                fprintf(stderr, "rank %d: %s: guard element %d changed\n", R, what, i);
                return false;
            }
        }
        return true;
    }
};
}  // namespace

int main(int argc, char* argv[]) {
    rdc::Init(argc, argv);
    rdc::NewCommunicator(rdc::kMainCommName);
    const int N = argc >= 2 ? atoi(argv[1]) : 7;
    const int root = argc >= 3 ? atoi(argv[2]) : 0;
    const int W = rdc::GetWorldSize(), R = rdc::GetRank();
    const int G = 64;
    const double mine_d = 1.5 * (R + 1), mean_d = W == 1 ? mine_d : 0.75 * (W + 1);

    // allreduce, float16: the mean of a Sum that overflows
    Guarded<rdc::Float16> hb(G, N);
    rdc::Float16* h = hb.data();
    for (int i = 0; i < N; ++i) h[i].bits = kF16_40000;
    rdc::AllreduceAvg(h, (uint64_t)N);
    for (int i = 0; i < N; ++i) {
        if (h[i].bits != kF16_40000) {
            fprintf(stderr, "rank %d: allreduce element %d is 0x%04x, want 0x%04x\n", R, i, h[i].bits, kF16_40000);
            return 1;
        }
    }
    if (!hb.ok(R, "allreduce float16")) return 1;

    // allreduce, bfloat16: one rounding of 384.0f / W
    Guarded<rdc::BFloat16> bb(G, N);
    rdc::BFloat16* b = bb.data();
    const uint16_t b_in = R == 0 ? kBF16_384 : 0, b_mean = W == 1 ? b_in : bf16_rne(384.0f / (float)W);
    for (int i = 0; i < N; ++i) b[i].bits = b_in;
    rdc::AllreduceAvg(b, (uint64_t)N);
    for (int i = 0; i < N; ++i) {
        if (b[i].bits != b_mean) {
            fprintf(stderr, "rank %d: allreduce element %d is 0x%04x, want 0x%04x\n", R, i, b[i].bits, b_mean);
            return 1;
        }
    }
    if (!bb.ok(R, "allreduce bfloat16")) return 1;

    // reduce-scatter, double: this rank's chunk holds the mean, the rest its input
    Guarded<double> db(G, N);
    double* d = db.data();
    for (int i = 0; i < N; ++i) d[i] = mine_d;
    const std::pair<uint64_t, uint64_t> mine = rdc::ReduceScatterAvg(d, (uint64_t)N);
    for (int i = 0; i < N; ++i) {
        const bool in = (uint64_t)i >= mine.first && (uint64_t)i < mine.second;
        const double want = in ? mean_d : mine_d;
        if (d[i] != want) {
            fprintf(stderr, "rank %d: reduce-scatter element %d is %.17g, want %.17g\n", R, i, d[i], want);
            return 1;
        }
    }
    if (!db.ok(R, "reduce-scatter")) return 1;

    // reduction to root, float: every other rank keeps its input
    Guarded<float> fb(G, N);
    float* f = fb.data();
    for (int i = 0; i < N; ++i) f[i] = (float)mine_d;
    rdc::ReduceToAvg(f, (uint64_t)N, root);
    for (int i = 0; i < N; ++i) {
        const float want = R == root ? (float)mean_d : (float)mine_d;
        if (f[i] != want) {
            fprintf(stderr, "rank %d: reduce-to element %d is %.9g, want %.9g\n", R, i, f[i], want);
            return 1;
        }
    }
    if (!fb.ok(R, "reduce-to")) return 1;

    printf("rank %d: avg OK (world %d, N %d, root %d)\n", R, W, N, root);
    rdc::Finalize();
    return 0;
}
