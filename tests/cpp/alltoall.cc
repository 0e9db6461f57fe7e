// Known-answer program for rdc::Alltoall<DType> and rdc::Alltoallv<DType>
// (include/rdc.h).  Equal split: rank R sends s[p * N + i] = R * 1000 + p * 100
// + i, so r[p * N + i] must be p * 1000 + R * 100 + i.  Alltoallv: pair
// (r -> p) carries cnt(r, p) = (2 r + p) % 4 elements (asymmetric, with zero
// segments) of value r * 10000 + p * 100 + i; the receive segments sit one
// element apart, and the gaps must keep their -1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rdc.h"

static uint64_t cnt(int r, int p) { return (uint64_t)((2 * r + p) % 4); }

int main(int argc, char* argv[]) {
    rdc::Init(argc, argv);
    rdc::NewCommunicator(rdc::kMainCommName);
    const int N = argc >= 2 ? atoi(argv[1]) : 5;
    const int W = rdc::GetWorldSize(), R = rdc::GetRank();
    std::vector<int> s((size_t)W * N), r((size_t)W * N, -1);
    for (int p = 0; p < W; ++p)
        for (int i = 0; i < N; ++i) s[(size_t)p * N + i] = R * 1000 + p * 100 + i;
    const std::vector<int> s0 = s;
    rdc::Alltoall<int>(s.data(), r.data(), (uint64_t)N);
    for (int p = 0; p < W; ++p)
        for (int i = 0; i < N; ++i)
            if (r[(size_t)p * N + i] != p * 1000 + R * 100 + i) {
                fprintf(stderr, "rank %d: alltoall element (%d, %d) is %d\n", R, p, i, r[(size_t)p * N + i]);
                return 1;
            }
    if (s != s0) {
        fprintf(stderr, "rank %d: alltoall changed the send buffer\n", R);
        return 1;
    }

    std::vector<uint64_t> sc((size_t)W), sd((size_t)W), rc((size_t)W), rd((size_t)W);
    uint64_t st = 0, rt = 1;
    for (int p = 0; p < W; ++p) {
        sc[(size_t)p] = cnt(R, p);
        sd[(size_t)p] = st;
        st += sc[(size_t)p];
        rc[(size_t)p] = cnt(p, R);
        rd[(size_t)p] = rt;
        rt += rc[(size_t)p] + 1;  // one untouched element after every segment
    }
    std::vector<int> vs((size_t)st + 1), vr((size_t)rt, -1);
    for (int p = 0; p < W; ++p)
        for (uint64_t i = 0; i < sc[(size_t)p]; ++i) vs[(size_t)(sd[(size_t)p] + i)] = R * 10000 + p * 100 + (int)i;
    rdc::Alltoallv<int>(vs.data(), sc.data(), sd.data(), vr.data(), rc.data(), rd.data());
    std::vector<int> want((size_t)rt, -1);
    for (int p = 0; p < W; ++p)
        for (uint64_t i = 0; i < rc[(size_t)p]; ++i) want[(size_t)(rd[(size_t)p] + i)] = p * 10000 + R * 100 + (int)i;
    if (vr != want) {
        fprintf(stderr, "rank %d: alltoallv result differs\n", R);
        return 1;
    }
    printf("rank %d: all-to-all OK (world %d, N %d)\n", R, W, N);
    rdc::Finalize();
    return 0;
}
