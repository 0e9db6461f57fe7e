// Known-answer program for rdc::ReduceTo<OP, DType> (include/rdc.h) over the
// inputs of the reference's test/allreduce.cc:17-55: every rank holds
// a[i] = rank + N + i inside a guarded array.  After ReduceTo<Sum>(root) the
// root holds sum_j (j + N + i) in every element, every other rank still holds
// its own input, and no guard element changed on any rank.
// argv: N root
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rdc.h"

int main(int argc, char* argv[]) {
    rdc::Init(argc, argv);
    rdc::NewCommunicator(rdc::kMainCommName);
    const int N = argc >= 2 ? atoi(argv[1]) : 7;
    const int root = argc >= 3 ? atoi(argv[2]) : 0;
    const int W = rdc::GetWorldSize(), R = rdc::GetRank();
    const int G = 64, kGuard = 0x5A5A5A5A;
    std::vector<int> backing((size_t)(N + 2 * G), kGuard);
    int* a = backing.data() + G;
    for (int i = 0; i < N; ++i) a[i] = R + N + i;
    rdc::ReduceTo<rdc::op::Sum, int>(a, (uint64_t)N, root);
    for (int i = 0; i < N; ++i) {
        long want = R + N + i;
        if (R == root) {
            want = 0;
            for (int j = 0; j < W; ++j) want += j + N + i;
        }
        if (a[i] != want) {
            fprintf(stderr, "rank %d: element %d is %d, want %ld\n", R, i, a[i], want);
            return 1;
        }
    }
    for (int i = 0; i < G; ++i) {
        if (backing[(size_t)i] != kGuard || backing[(size_t)(G + N + i)] != kGuard) {
            fprintf(stderr, "rank %d: guard element %d changed\n", R, i);
            return 1;
        }
    }
    printf("rank %d: reduce-to OK (world %d, N %d, root %d)\n", R, W, N, root);
    rdc::Finalize();
    return 0;
}
