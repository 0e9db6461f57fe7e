// TEST SHIM — include/rdc.h's host op::Reducer<op::Prod | op::BitAND |
// op::BitXOR, T> on small arrays, host only (no GPU is touched).
//   op_prod_shim <prod|bitand|bitxor> <i8|i32|u64|f32|f64> <in.bin>
// in.bin holds the dst elements, then as many src elements; the folded dst is
// printed one element per line as the hexadecimal of its bits, for
// tests/test_ops_plan.py to compare with tests/ops_ref.apply.
// -DBAD=1: op::BitAND on float, -DBAD=2: op::BitXOR on double, -DBAD=3:
// Allreduce<op::Prod, ValueIndex<float>> — none may compile.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "rdc.h"

namespace {
template <typename OP, typename T>
int fold(const std::vector<char>& raw) {
    const size_t n = raw.size() / (2 * sizeof(T));
    std::vector<T> dst(n), src(n);
    memcpy(dst.data(), raw.data(), n * sizeof(T));
    memcpy(src.data(), raw.data() + n * sizeof(T), n * sizeof(T));
    rdc::op::Reducer<OP, T>(src.data(), dst.data(), n);
    for (size_t i = 0; i < n; ++i) {
        uint64_t bits = 0;
        memcpy(&bits, &dst[i], sizeof(T));  // little-endian host
        printf("%016" PRIx64 "\n", bits);
    }
    return 0;
}
template <typename OP>
int integer(const std::string& t, const std::vector<char>& raw) {
    if (t == "i8") return fold<OP, int8_t>(raw);
    if (t == "i32") return fold<OP, int32_t>(raw);
    if (t == "u64") return fold<OP, uint64_t>(raw);
    return 2;
}
}  // namespace

#ifdef BAD
void bad() {
#if BAD == 1
    float a = 1, b = 2;
    rdc::op::BitAND::Reduce(a, b);
#elif BAD == 2
    double a = 1, b = 2;
    rdc::op::BitXOR::Reduce(a, b);
#else
    rdc::ValueIndex<float> p[1];
    rdc::Allreduce<rdc::op::Prod>(p, 1);
#endif
}
#endif

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const std::string op = argv[1], t = argv[2];
    FILE* f = fopen(argv[3], "rb");
    if (!f) return 2;
    std::vector<char> raw;
    char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + got);
    fclose(f);
    static_assert(rdc::op::Prod::kType == 8 && rdc::op::BitAND::kType == 9 && rdc::op::BitXOR::kType == 10 &&
                      rdc::mpi::kProd == 8 && rdc::mpi::kBitwiseAND == 9 && rdc::mpi::kBitwiseXOR == 10,
                  "operator codes");
    if (op == "prod") {
        if (t == "f32") return fold<rdc::op::Prod, float>(raw);
        if (t == "f64") return fold<rdc::op::Prod, double>(raw);
        return integer<rdc::op::Prod>(t, raw);
    }
    if (op == "bitand") return integer<rdc::op::BitAND>(t, raw);
    if (op == "bitxor") return integer<rdc::op::BitXOR>(t, raw);
    return 2;
}
