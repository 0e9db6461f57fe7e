// Host-only: include/rdc.h's op::Reducer<op::MaxLoc / op::MinLoc,
// ValueIndex<double / int64_t>> over a file of 16-byte pairs
// (tests/test_loc16_plan.py writes the rule table of tests/loc16_ref.py there
// and compares what comes back).
// argv: maxloc|minloc f64|i64 in_file out_file
// in_file: count dst pairs, then count src pairs (16 bytes each); out_file:
// count pairs, dst after Reducer(src, dst, count).  Calls nothing of the library
// (rdc.h's inline members still need it at link time) and needs no GPU.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rdc.h"

// what must not compile (checked by tests/test_loc16_plan.py with -DBAD=1 / 2)
#if defined(BAD) && BAD == 1
void bad(rdc::ValueIndex<double>* p) { rdc::Allreduce<rdc::op::Sum>(p, 1); }
#elif defined(BAD) && BAD == 2
void bad(double* p) { rdc::Allreduce<rdc::op::MaxLoc>(p, 1); }
#endif

// the narrow pairs keep their layout
static_assert(sizeof(rdc::ValueIndex<float>) == 8 && alignof(rdc::ValueIndex<float>) == 8, "ValueIndex<float>");
static_assert(sizeof(rdc::ValueIndex<int32_t>) == 8 && alignof(rdc::ValueIndex<int32_t>) == 8, "ValueIndex<int32_t>");
static_assert(sizeof(rdc::ValueIndex<float>().index) == 4 && sizeof(rdc::ValueIndex<double>().index) == 8 &&
                  sizeof(rdc::ValueIndex<int64_t>().index) == 8,
              "the index type follows the value's width");

template <typename OP, typename V>
static int run(const char* in, const char* out) {
    typedef rdc::ValueIndex<V> P;
    static_assert(sizeof(P) == 16 && alignof(P) == 16, "ValueIndex is the 16-byte element");
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
    if (rdc::mpi::GetType<rdc::ValueIndex<double>>() != 16 || rdc::mpi::GetType<rdc::ValueIndex<int64_t>>() != 17) return 6;
    if (rdc::mpi::kDoubleInt64 != 16 || rdc::mpi::kInt64Int64 != 17) return 6;
    const bool mx = strcmp(argv[1], "maxloc") == 0, f64 = strcmp(argv[2], "f64") == 0;
    if (mx && f64) return run<rdc::op::MaxLoc, double>(argv[3], argv[4]);
    if (mx) return run<rdc::op::MaxLoc, int64_t>(argv[3], argv[4]);
    if (f64) return run<rdc::op::MinLoc, double>(argv[3], argv[4]);
    return run<rdc::op::MinLoc, int64_t>(argv[3], argv[4]);
}
