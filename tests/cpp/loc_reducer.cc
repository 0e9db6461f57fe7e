// Host-only: include/rdc.h's op::Reducer<op::MaxLoc / op::MinLoc,
// ValueIndex<V>> over a file of pairs (tests/test_loc_plan.py writes the rule
// table of tests/loc_ref.py there and compares what comes back).
// argv: maxloc|minloc f32|i32 in_file out_file
// in_file: count dst pairs, then count src pairs (8 bytes each); out_file:
// count pairs, dst after Reducer(src, dst, count).  Calls nothing of the library
// (rdc.h's inline members still need it at link time) and needs no GPU.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rdc.h"

// what must not compile (checked by tests/test_loc_plan.py with -DBAD=1 / 2)
#if defined(BAD) && BAD == 1
void bad(rdc::ValueIndex<float>* p) { rdc::Allreduce<rdc::op::Sum>(p, 1); }
#elif defined(BAD) && BAD == 2
void bad(float* p) { rdc::Allreduce<rdc::op::MaxLoc>(p, 1); }
#endif

template <typename OP, typename V>
static int run(const char* in, const char* out) {
    typedef rdc::ValueIndex<V> P;
    static_assert(sizeof(P) == 8 && alignof(P) == 8, "ValueIndex is the 8-byte element");
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % (2 * sizeof(P))) return 3;
    const size_t count = (size_t)bytes / (2 * sizeof(P));
    std::vector<P> dst(count), src(count);
    if (fread(dst.data(), sizeof(P), count, f) != count || fread(src.data(), sizeof(P), count, f) != count) return 4;
    fclose(f);
    rdc::op::Reducer<OP, P>(src.data(), dst.data(), count);
    f = fopen(out, "wb");
    if (!f || fwrite(dst.data(), sizeof(P), count, f) != count) return 5;
    fclose(f);
    return 0;
}

int main(int argc, char* argv[]) {
    if (argc != 5) return 1;
    static_assert(rdc::op::MaxLoc::kType == 4 && rdc::op::MinLoc::kType == 5, "op codes");
    if (rdc::mpi::GetType<rdc::ValueIndex<float>>() != 12 || rdc::mpi::GetType<rdc::ValueIndex<int32_t>>() != 13) return 6;
    const bool mx = strcmp(argv[1], "maxloc") == 0, f32 = strcmp(argv[2], "f32") == 0;
    if (mx && f32) return run<rdc::op::MaxLoc, float>(argv[3], argv[4]);
    if (mx) return run<rdc::op::MaxLoc, int32_t>(argv[3], argv[4]);
    if (f32) return run<rdc::op::MinLoc, float>(argv[3], argv[4]);
    return run<rdc::op::MinLoc, int32_t>(argv[3], argv[4]);
}
