// Known-answer program for rdc::Scan<OP, DType> and rdc::Exscan<OP, DType>
// (include/rdc.h) over the inputs of the reference's test/allreduce.cc:17-55:
// every rank holds a[i] = rank + N + i inside a guarded array.  After
// Scan<Sum> rank r holds sum_{j <= r} (j + N + i); after Exscan<Max> of
// b[i] = (i % W == rank ? 1000 + i : rank - i) rank r > 0 holds the host-side
// fold of ranks 0..r-1.  Rank 0's arrays stay as they were, and no guard
// element changes on any rank.
// argv: N
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rdc.h"

int main(int argc, char* argv[]) {
    rdc::Init(argc, argv);
    rdc::NewCommunicator(rdc::kMainCommName);
    const int N = argc >= 2 ? atoi(argv[1]) : 7;
    const int W = rdc::GetWorldSize(), R = rdc::GetRank();
    const int G = 64, kGuard = 0x5A5A5A5A;
    std::vector<int> backing((size_t)(N + 2 * G), kGuard);
    int* a = backing.data() + G;
    for (int i = 0; i < N; ++i) a[i] = R + N + i;
    rdc::Scan<rdc::op::Sum, int>(a, (uint64_t)N);
    for (int i = 0; i < N; ++i) {
        long want = 0;
        for (int j = 0; j <= R; ++j) want += j + N + i;
        if (a[i] != want) {
            fprintf(stderr, "rank %d: scan element %d is %d, want %ld\n", R, i, a[i], want);
            return 1;
        }
    }
    std::vector<int> backing2((size_t)(N + 2 * G), kGuard);
    int* b = backing2.data() + G;
    for (int i = 0; i < N; ++i) b[i] = i % W == R ? 1000 + i : R - i;
    rdc::Exscan<rdc::op::Max, int>(b, (uint64_t)N);
    for (int i = 0; i < N; ++i) {
        int want = i % W == R ? 1000 + i : R - i;  // rank 0: untouched
        if (R > 0) {
            want = i % W == 0 ? 1000 + i : 0 - i;
            for (int j = 1; j < R; ++j) {
                const int x = i % W == j ? 1000 + i : j - i;
                if (want < x) want = x;
            }
        }
        if (b[i] != want) {
            fprintf(stderr, "rank %d: exscan element %d is %d, want %d\n", R, i, b[i], want);
            return 1;
        }
    }
    for (int i = 0; i < G; ++i) {
        if (backing[(size_t)i] != kGuard || backing[(size_t)(G + N + i)] != kGuard ||
            backing2[(size_t)i] != kGuard || backing2[(size_t)(G + N + i)] != kGuard) {
            fprintf(stderr, "rank %d: guard element %d changed\n", R, i);
            return 1;
        }
    }
    printf("rank %d: scan and exscan OK (world %d, N %d)\n", R, W, N);
    rdc::Finalize();
    return 0;
}
