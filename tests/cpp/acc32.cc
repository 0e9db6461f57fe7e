// Known-answer program for rdc::AllreduceAcc32 / ReduceScatterAcc32 /
// ReduceToAcc32 (include/rdc.h): the Sum of 16-bit floating elements with a
// float32 accumulator and one rounding.  Rank 0 holds a value whose 16-bit ulp
// is 2 (2048 in float16, 256 in bfloat16), every other rank holds 1, inside
// guarded arrays.  The float32 sum big + (W - 1) is exact, so the result is
// its one rounding to nearest even — 256 + 1 + 1 + 1 = 260 in bfloat16, where
// a Sum that rounds at every hop stays at 256.
// argv: N root
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rdc.h"

namespace {
// round-to-nearest-even of the integer v in [big, 2 * big) to a multiple of 2
int rne2(int v) {
    int q = v / 2;
    if (v % 2 && q % 2) ++q;  // a tie goes to the even multiple
    return 2 * q;
}
uint16_t f16_bits(int v) { return v == 1 ? 0x3C00 : (uint16_t)((26 << 10) | ((v - 2048) / 2)); }   // 1, or even v in [2048, 4096)
uint16_t bf16_bits(int v) { return v == 1 ? 0x3F80 : (uint16_t)((135 << 7) | ((v - 256) / 2)); }   // 1, or even v in [256, 512)

template <typename T>
bool guards_ok(const std::vector<T>& backing, int G, int N, int R, const char* what) {
    for (int i = 0; i < G; ++i) {
        if (backing[(size_t)i].bits != 0xA5A5 || backing[(size_t)(G + N + i)].bits != 0xA5A5) {
            fprintf(stderr, "rank %d: %s: guard element %d changed\n", R, what, i);
            return false;
        }
    }
    return true;
}
}  // namespace

int main(int argc, char* argv[]) {
    rdc::Init(argc, argv);
    rdc::NewCommunicator(rdc::kMainCommName);
    const int N = argc >= 2 ? atoi(argv[1]) : 7;
    const int root = argc >= 3 ? atoi(argv[2]) : 0;
    const int W = rdc::GetWorldSize(), R = rdc::GetRank();
    const int G = 64;
    const uint16_t h_in = f16_bits(R == 0 ? 2048 : 1), b_in = bf16_bits(R == 0 ? 256 : 1);
    const uint16_t h_sum = f16_bits(W == 1 ? 2048 : rne2(2048 + W - 1));
    const uint16_t b_sum = bf16_bits(W == 1 ? 256 : rne2(256 + W - 1));

    // allreduce, float16
    std::vector<rdc::Float16> hb((size_t)(N + 2 * G), rdc::Float16{0xA5A5});
    rdc::Float16* h = hb.data() + G;
    for (int i = 0; i < N; ++i) h[i].bits = h_in;
    rdc::AllreduceAcc32(h, (uint64_t)N);
    for (int i = 0; i < N; ++i) {
        if (h[i].bits != h_sum) {
            fprintf(stderr, "rank %d: allreduce element %d is 0x%04x, want 0x%04x\n", R, i, h[i].bits, h_sum);
            return 1;
        }
    }
    if (!guards_ok(hb, G, N, R, "allreduce")) return 1;

    // reduce-scatter, bfloat16: this rank's chunk holds the sum, the rest its input
    std::vector<rdc::BFloat16> bb((size_t)(N + 2 * G), rdc::BFloat16{0xA5A5});
    rdc::BFloat16* b = bb.data() + G;
    for (int i = 0; i < N; ++i) b[i].bits = b_in;
    const std::pair<uint64_t, uint64_t> mine = rdc::ReduceScatterAcc32(b, (uint64_t)N);
    for (int i = 0; i < N; ++i) {
        const bool in = (uint64_t)i >= mine.first && (uint64_t)i < mine.second;
        const uint16_t want = in ? b_sum : b_in;
        if (b[i].bits != want) {
            fprintf(stderr, "rank %d: reduce-scatter element %d is 0x%04x, want 0x%04x\n", R, i, b[i].bits, want);
            return 1;
        }
    }
    if (!guards_ok(bb, G, N, R, "reduce-scatter")) return 1;

    // reduction to root, bfloat16: every other rank keeps its input
    for (int i = 0; i < N; ++i) b[i].bits = b_in;
    rdc::ReduceToAcc32(b, (uint64_t)N, root);
    for (int i = 0; i < N; ++i) {
        const uint16_t want = R == root ? b_sum : b_in;
        if (b[i].bits != want) {
            fprintf(stderr, "rank %d: reduce-to element %d is 0x%04x, want 0x%04x\n", R, i, b[i].bits, want);
            return 1;
        }
    }
    if (!guards_ok(bb, G, N, R, "reduce-to")) return 1;

    printf("rank %d: acc32 OK (world %d, N %d, root %d)\n", R, W, N, root);
    rdc::Finalize();
    return 0;
}
