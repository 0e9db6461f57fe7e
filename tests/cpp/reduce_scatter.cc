// Known-answer program for rdc::ReduceScatter<OP, DType> (include/rdc.h) over
// the inputs of the reference's test/allreduce.cc:17-55: every rank holds
// a[i] = rank + N + i.  After ReduceScatter<Sum> rank R's element range
// [lo, hi) of utils::Split(0, N, W) holds sum_j (j + N + i) — the allreduce's
// values — and every other element still holds the rank's own input.
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#include "rdc.h"

int main(int argc, char* argv[]) {
    rdc::Init(argc, argv);
    rdc::NewCommunicator(rdc::kMainCommName);
    const int N = argc >= 2 ? atoi(argv[1]) : 7;
    const int W = rdc::GetWorldSize(), R = rdc::GetRank();
    std::vector<int> a((size_t)N);
    for (int i = 0; i < N; ++i) a[(size_t)i] = R + N + i;
    const std::pair<uint64_t, uint64_t> mine = rdc::ReduceScatter<rdc::op::Sum, int>(a.data(), (uint64_t)N);
    // utils::Split: the first N % W chunks hold one element more
    const uint64_t k = (uint64_t)N / (uint64_t)W, m = (uint64_t)N % (uint64_t)W;
    const uint64_t lo = (uint64_t)R * k + ((uint64_t)R < m ? (uint64_t)R : m);
    const uint64_t hi = lo + k + ((uint64_t)R < m ? 1 : 0);
    if (mine.first != lo || mine.second != hi) {
        fprintf(stderr, "rank %d: range [%llu, %llu), want [%llu, %llu)\n", R, (unsigned long long)mine.first,
                (unsigned long long)mine.second, (unsigned long long)lo, (unsigned long long)hi);
        return 1;
    }
    for (int i = 0; i < N; ++i) {
        long want = R + N + i;
        if ((uint64_t)i >= lo && (uint64_t)i < hi) {
            want = 0;
            for (int j = 0; j < W; ++j) want += j + N + i;
        }
        if (a[(size_t)i] != want) {
            fprintf(stderr, "rank %d: element %d is %d, want %ld\n", R, i, a[(size_t)i], want);
            return 1;
        }
    }
    printf("rank %d: reduce-scatter OK (world %d, N %d)\n", R, W, N);
    rdc::Finalize();
    return 0;
}
