// Device-side primitives for the MI355X (gfx950) rdc allreduce path.
//
//  * reduction operators with the reference's exact semantics
//    (op::Max/Min/Sum/BitOR::Reduce, include/core/mpi.h:85-112):
//        Max: dst = (dst < src) ? src : dst      (NaN in src ignored, NaN in dst sticky)
//        Min: dst = (dst > src) ? src : dst
//        Sum: dst = dst + src                    (signed ints wrap: computed unsigned)
//        BitOR: dst = dst | src
//    the MI355X-build additions (rdc_common.h RDC_OP_PROD):
//        Prod: dst = dst * src     (ints wrap modulo 2^bits: computed unsigned;
//              f32 / f64 / f16: one IEEE multiply, RNE, subnormals kept;
//              bf16: exact f32 product + one RNE to bf16)
//        BitAND: dst = dst & src,  BitXOR: dst = dst ^ src   (integers only)
//    and the MI355X-build pair operators (rdc_common.h RDC_OP_MAXLOC):
//        MaxLoc: dst = src if dst.value < src.value ||
//                           (dst.value == src.value && src.index < dst.index)
//        MinLoc: the same with >       (NaN, -0 / +0 and full ties: rdc_common.h)
//    f16: native v_add_f16 (correctly rounded); bf16: f32 add + RNE to bf16.
//  * 16-byte vector reduce (v4u reinterpreted as 16/sizeof(T) lanes)
//  * cross-GPU hand-off: write-through (sc0 sc1) payload stores into the
//    peer's scratch -> every wave's vmcnt(0) -> barrier -> one lane: relaxed
//    system-scope flag store (plus a system-scope release fence when the
//    scratch is not uncached).  Consumer: one lane per flag polls
//    relaxed/system, barrier, loads of its own uncached scratch (an acquire
//    fence when it is not uncached) (MI355X_MICROARCH.md "Workgroup dispatch
//    ... visibility"; cdna_hip_programming.md G16).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rdc_common.h"

namespace rdc_amd {

// ---------------------------------------------------------------- types ----
// native 16-byte vector (global_load/store_dwordx4)
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

struct bf16_t {
    uint16_t bits;
};

template <typename T> struct Arith { typedef T U; };
template <> struct Arith<int8_t> { typedef uint8_t U; };
template <> struct Arith<int32_t> { typedef uint32_t U; };
template <> struct Arith<int64_t> { typedef uint64_t U; };

__device__ __forceinline__ float bf16_to_f32(uint16_t b) {
    return __uint_as_float((uint32_t)b << 16);
}
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    uint32_t x = __float_as_uint(f);
    if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((x >> 16) | 0x40);
    x += 0x7fffu + ((x >> 16) & 1u);
    return (uint16_t)(x >> 16);
}

template <int OP> struct OpF;
template <> struct OpF<RDC_OP_MAX> {
    template <typename T> __device__ __forceinline__ static T apply(T d, T s) { return (d < s) ? s : d; }
    __device__ __forceinline__ static bf16_t apply(bf16_t d, bf16_t s) {
        return (bf16_to_f32(d.bits) < bf16_to_f32(s.bits)) ? s : d;
    }
};
template <> struct OpF<RDC_OP_MIN> {
    template <typename T> __device__ __forceinline__ static T apply(T d, T s) { return (d > s) ? s : d; }
    __device__ __forceinline__ static bf16_t apply(bf16_t d, bf16_t s) {
        return (bf16_to_f32(d.bits) > bf16_to_f32(s.bits)) ? s : d;
    }
};
template <> struct OpF<RDC_OP_SUM> {
    template <typename T> __device__ __forceinline__ static T apply(T d, T s) {
        typedef typename Arith<T>::U U;
        return (T)((U)d + (U)s);
    }
    __device__ __forceinline__ static float apply(float d, float s) { return d + s; }
    __device__ __forceinline__ static double apply(double d, double s) { return d + s; }
    __device__ __forceinline__ static _Float16 apply(_Float16 d, _Float16 s) { return d + s; }
    // f32 add (exact inputs) then one RNE conversion = the correctly rounded
    // bf16 add; v_cvt_pk_bf16_f32 (gfx950) does the conversion in hardware
    __device__ __forceinline__ static bf16_t apply(bf16_t d, bf16_t s) {
        const __bf16 h = (__bf16)(bf16_to_f32(d.bits) + bf16_to_f32(s.bits));
        bf16_t r;
        r.bits = __builtin_bit_cast(uint16_t, h);
        return r;
    }
};
template <> struct OpF<RDC_OP_BITOR> {
    template <typename T> __device__ __forceinline__ static T apply(T d, T s) {
        typedef typename Arith<T>::U U;
        return (T)((U)d | (U)s);
    }
};

template <> struct OpF<RDC_OP_PROD> {
    // integers on the unsigned type: the product wraps modulo 2^bits (a signed
    // `d * s` is undefined on overflow); bytes promote to int, 255 * 255 fits
    template <typename T> __device__ __forceinline__ static T apply(T d, T s) {
        typedef typename Arith<T>::U U;
        return (T)((U)d * (U)s);
    }
    __device__ __forceinline__ static float apply(float d, float s) { return d * s; }
    __device__ __forceinline__ static double apply(double d, double s) { return d * s; }
    __device__ __forceinline__ static _Float16 apply(_Float16 d, _Float16 s) { return d * s; }
    // the f32 product of two bf16 values is exact (8 x 8 significand bits), so
    // one RNE conversion gives the correctly rounded bf16 product
    __device__ __forceinline__ static bf16_t apply(bf16_t d, bf16_t s) {
        const __bf16 h = (__bf16)(bf16_to_f32(d.bits) * bf16_to_f32(s.bits));
        bf16_t r;
        r.bits = __builtin_bit_cast(uint16_t, h);
        return r;
    }
};
template <> struct OpF<RDC_OP_BITAND> {
    template <typename T> __device__ __forceinline__ static T apply(T d, T s) {
        typedef typename Arith<T>::U U;
        return (T)((U)d & (U)s);
    }
};
template <> struct OpF<RDC_OP_BITXOR> {
    template <typename T> __device__ __forceinline__ static T apply(T d, T s) {
        typedef typename Arith<T>::U U;
        return (T)((U)d ^ (U)s);
    }
};

// (value, index) pairs (RDC_DT_F32_I32 / RDC_DT_I32_I32): 8 bytes, moved as one
// 64-bit word by the element-wise paths (ld_elem_sys / st_elem_wt)
struct alignas(8) pair_f32_t {
    float value;
    int32_t index;
};
struct alignas(8) pair_i32_t {
    int32_t value;
    int32_t index;
};
static_assert(sizeof(pair_f32_t) == 8 && std::is_trivially_copyable<pair_f32_t>::value, "pair_f32_t");
static_assert(sizeof(pair_i32_t) == 8 && std::is_trivially_copyable<pair_i32_t>::value, "pair_i32_t");
// the 16-byte pairs (RDC_DT_F64_I64 / RDC_DT_I64_I64): one element per 16-byte
// vector, buffers 16-byte aligned, so every chunk, tile and piece of them
// starts on a vector boundary and the element-wise heads and tails are empty;
// where an element-wise path does run (ld_elem_sys / st_elem_wt) an element
// moves as two 64-bit words
struct alignas(16) pair_f64_t {
    double value;
    int64_t index;
};
struct alignas(16) pair_i64_t {
    int64_t value;
    int64_t index;
};
static_assert(sizeof(pair_f64_t) == 16 && std::is_trivially_copyable<pair_f64_t>::value, "pair_f64_t");
static_assert(sizeof(pair_i64_t) == 16 && std::is_trivially_copyable<pair_i64_t>::value, "pair_i64_t");

// does src replace dst?  Non-short-circuit on purpose: two compares, one
// and, one or, no branch.
template <bool MAX, typename V>
__device__ __forceinline__ bool loc_take(V dv, int32_t di, V sv, int32_t si) {
    const bool better = MAX ? (dv < sv) : (dv > sv);
    return better | ((dv == sv) & (si < di));
}
// the same on a 64-bit index (the 16-byte pairs); an overload, so the 8-byte
// pairs' calls resolve as before
template <bool MAX, typename V>
__device__ __forceinline__ bool loc_take(V dv, int64_t di, V sv, int64_t si) {
    const bool better = MAX ? (dv < sv) : (dv > sv);
    return better | ((dv == sv) & (si < di));
}
template <> struct OpF<RDC_OP_MAXLOC> {
    __device__ __forceinline__ static pair_f32_t apply(pair_f32_t d, pair_f32_t s) {
        return loc_take<true>(d.value, d.index, s.value, s.index) ? s : d;
    }
    __device__ __forceinline__ static pair_i32_t apply(pair_i32_t d, pair_i32_t s) {
        return loc_take<true>(d.value, d.index, s.value, s.index) ? s : d;
    }    __device__ __forceinline__ static pair_f64_t apply(pair_f64_t d, pair_f64_t s) {
        return loc_take<true>(d.value, d.index, s.value, s.index) ? s : d;
    }
    __device__ __forceinline__ static pair_i64_t apply(pair_i64_t d, pair_i64_t s) {
        return loc_take<true>(d.value, d.index, s.value, s.index) ? s : d;
    }
};
template <> struct OpF<RDC_OP_MINLOC> {
    __device__ __forceinline__ static pair_f32_t apply(pair_f32_t d, pair_f32_t s) {
        return loc_take<false>(d.value, d.index, s.value, s.index) ? s : d;
    }
    __device__ __forceinline__ static pair_i32_t apply(pair_i32_t d, pair_i32_t s) {
        return loc_take<false>(d.value, d.index, s.value, s.index) ? s : d;
    }    __device__ __forceinline__ static pair_f64_t apply(pair_f64_t d, pair_f64_t s) {
        return loc_take<false>(d.value, d.index, s.value, s.index) ? s : d;
    }
    __device__ __forceinline__ static pair_i64_t apply(pair_i64_t d, pair_i64_t s) {
        return loc_take<false>(d.value, d.index, s.value, s.index) ? s : d;
    }
};

// Reduce two 16-byte vectors lane-wise: returns OP(d, s) per element.
template <int OP, typename T>
__device__ __forceinline__ v4u reduce16(v4u d, v4u s) {
    constexpr int K = 16 / sizeof(T);
    T a[K], b[K];
    __builtin_memcpy(a, &d, 16);
    __builtin_memcpy(b, &s, 16);
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = OpF<OP>::apply(a[k], b[k]);
    __builtin_memcpy(&d, a, 16);
    return d;
}

// 8-bit integers, four lanes per dword without unpacking (the generic loop
// spends ~12 VALU ops and a register per byte: the int8 / uint8 one-shot
// needed 256 VGPRs and ran one wave per SIMD).  Sum wraps like the
// reference's `dst += src` on a byte: low 7 bits added without carry-out,
// top bit by XOR.  Max / Min: even and odd bytes as 16-bit lanes through
// v_pk_max_u16 / v_pk_min_u16; signed bytes compare as unsigned after
// flipping their sign bits.  Prod wraps modulo 256 and the signed product has
// the same bits: the low byte of a 16-bit lane's product depends on the
// operands' low bytes only, so the even bytes are the masked v_pk_mul_lo_u16 of
// the dwords as they are, and the odd bytes come out in place, low byte zero,
// from (a & 0xff00ff00) * (b >> 8): (x << 8) * y mod 2^16 = ((x * y) & 0xff) << 8
// whatever sits above y's low byte.  BitAND / BitXOR: one VALU op per dword.
namespace swar8 {
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t add(uint32_t a, uint32_t b) {
    return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u);
}
template <bool MAX>
__device__ __forceinline__ uint32_t pick_u(uint32_t a, uint32_t b) {
    const u16x2 ae = __builtin_bit_cast(u16x2, a & 0x00ff00ffu), be = __builtin_bit_cast(u16x2, b & 0x00ff00ffu);
    const u16x2 ao = __builtin_bit_cast(u16x2, (a >> 8) & 0x00ff00ffu), bo = __builtin_bit_cast(u16x2, (b >> 8) & 0x00ff00ffu);
    const u16x2 e = MAX ? __builtin_elementwise_max(ae, be) : __builtin_elementwise_min(ae, be);
    const u16x2 o = MAX ? __builtin_elementwise_max(ao, bo) : __builtin_elementwise_min(ao, bo);
    return __builtin_bit_cast(uint32_t, e) | (__builtin_bit_cast(uint32_t, o) << 8);
}
__device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) {
    const u16x2 e = __builtin_bit_cast(u16x2, a) * __builtin_bit_cast(u16x2, b);
    const u16x2 o = __builtin_bit_cast(u16x2, a & 0xff00ff00u) * __builtin_bit_cast(u16x2, b >> 8);
    return (__builtin_bit_cast(uint32_t, e) & 0x00ff00ffu) | __builtin_bit_cast(uint32_t, o);
}
template <int OP, bool SIGNED>
__device__ __forceinline__ v4u reduce(v4u d, v4u s) {
    constexpr uint32_t flip = SIGNED ? 0x80808080u : 0u;
    v4u out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (OP == RDC_OP_SUM) out[k] = add(d[k], s[k]);
        else if (OP == RDC_OP_BITOR) out[k] = d[k] | s[k];
        else if (OP == RDC_OP_BITAND) out[k] = d[k] & s[k];
        else if (OP == RDC_OP_BITXOR) out[k] = d[k] ^ s[k];
        else if (OP == RDC_OP_PROD) out[k] = mul(d[k], s[k]);
        else out[k] = pick_u<OP == RDC_OP_MAX>(d[k] ^ flip, s[k] ^ flip) ^ flip;
    }
    return out;
}
}  // namespace swar8
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_SUM, uint8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_SUM, false>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_SUM, int8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_SUM, true>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_BITOR, uint8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_BITOR, false>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_BITOR, int8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_BITOR, true>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_MAX, uint8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_MAX, false>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_MAX, int8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_MAX, true>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_MIN, uint8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_MIN, false>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_MIN, int8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_MIN, true>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_PROD, uint8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_PROD, false>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_PROD, int8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_PROD, true>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_BITAND, uint8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_BITAND, false>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_BITAND, int8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_BITAND, true>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_BITXOR, uint8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_BITXOR, false>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_BITXOR, int8_t>(v4u d, v4u s) { return swar8::reduce<RDC_OP_BITXOR, true>(d, s); }

// bf16 Sum, two lanes per dword: v_pk_add_f32 + v_cvt_pk_bf16_f32 instead of
// a software round per element (the generic loop runs 4.35 TB/s, ALU-bound)
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_SUM, bf16_t>(v4u d, v4u s) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef __bf16 h2 __attribute__((ext_vector_type(2)));
    v4u out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const f2 a = {__uint_as_float(d[k] << 16), __uint_as_float(d[k] & 0xffff0000u)};
        const f2 b = {__uint_as_float(s[k] << 16), __uint_as_float(s[k] & 0xffff0000u)};
        out[k] = __builtin_bit_cast(uint32_t, __builtin_convertvector(a + b, h2));
    }
    return out;
}
// ---- float32-accumulated Sum of float16 / bfloat16 (the rule: include/rdc_amd.h, RdcAllreduceAcc32) ----
// kOpSumAcc32 is a template tag for the mesh family's fold (mesh_fold_elem /
// mesh_reduce_range, rdc_kernels_impl.h), not an RDC_OP_* code: no OpF and no
// reduce16 exist for it, get_kernels never sees it, and only
// rdc_kernels_fold.hip instantiates kernels with it.  The owner of a chunk
// holds all n raw 16-bit contributions before it folds, so it widens each to
// binary32, adds them in the ring order and rounds ONCE (RNE).
constexpr int kOpSumAcc32 = 0x100;
namespace acc32 {
typedef float f2 __attribute__((ext_vector_type(2)));
// one element
template <typename T> __device__ __forceinline__ float widen(T x);
template <> __device__ __forceinline__ float widen<_Float16>(_Float16 x) { return (float)x; }
template <> __device__ __forceinline__ float widen<bf16_t>(bf16_t x) { return bf16_to_f32(x.bits); }
template <typename T> __device__ __forceinline__ T narrow(float s);
template <> __device__ __forceinline__ _Float16 narrow<_Float16>(float s) { return (_Float16)s; }
template <> __device__ __forceinline__ bf16_t narrow<bf16_t>(float s) {
    const __bf16 h = (__bf16)s;  // v_cvt_pk_bf16_f32, as OpF<RDC_OP_SUM>
    bf16_t r;
    r.bits = __builtin_bit_cast(uint16_t, h);
    return r;
}
// one dword = two elements: float16 by the hardware conversions
// (v_cvt_f32_f16 per half, v_cvt_pk_f16_f32 back), bfloat16 by a shift and a
// mask up and v_cvt_pk_bf16_f32 back; the adds between are v_pk_add_f32
template <typename T> __device__ __forceinline__ f2 widen2(uint32_t w);
template <> __device__ __forceinline__ f2 widen2<_Float16>(uint32_t w) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    return __builtin_convertvector(__builtin_bit_cast(h2, w), f2);
}
template <> __device__ __forceinline__ f2 widen2<bf16_t>(uint32_t w) {
    const f2 r = {__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
    return r;
}
template <typename T> __device__ __forceinline__ uint32_t narrow2(f2 s);
template <> __device__ __forceinline__ uint32_t narrow2<_Float16>(f2 s) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(s, h2));
}
template <> __device__ __forceinline__ uint32_t narrow2<bf16_t>(f2 s) {
    typedef __bf16 h2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(s, h2));
}
}  // namespace acc32

// ---- Avg: the mean across ranks (the rule: include/rdc_amd.h, RdcAllreduceAvg) ----
// kOpAvg is a template tag like kOpSumAcc32, not an RDC_OP_* code: get_kernels
// never sees it and only rdc_kernels_fold.hip instantiates kernels with it.
// The owner of a chunk is the only place a result is produced, so it divides
// there, before the single store.  float / double: the ordinary Sum's ring
// fold in T, then one IEEE division by T(n).  float16 / bfloat16: the acc32
// fold, one binary32 division by float(n), one rounding to 16 bits.  A true
// division (v_div_scale / v_rcp / v_div_fmas / v_div_fixup under
// -fno-fast-math), never a multiplication by a rounded 1 / n.
constexpr int kOpAvg = 0x101;
// the folds that accumulate 16-bit elements in binary32
template <int OP, typename T>
constexpr bool kAccumulateF32 = OP == kOpSumAcc32 || (OP == kOpAvg && sizeof(T) == 2);
namespace avg {
// the lanes of a 16-byte vector of float (4) / double (2), each divided by T(n)
template <typename T>
__device__ __forceinline__ v4u div16(v4u v, int n) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
    constexpr int K = 16 / sizeof(T);
    const T dn = (T)n;
    T a[K];
    __builtin_memcpy(a, &v, 16);
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = a[k] / dn;
    __builtin_memcpy(&v, a, 16);
    return v;
}
}  // namespace avg

// bf16 Prod has no such form: OpF<RDC_OP_PROD>::apply converts through __bf16,
// so the generic loop already rounds in hardware (v_cvt_pk_bf16_f32), and a
// v_pk_mul_f32 form shaped like the one above measured no faster in k_reduce on
// 1 GiB (0.5147 against 0.5144 ms)

// (value, index) pairs, two per vector, folded from the four dwords: per pair
// two compares on the value dwords, one on the index dwords, and both dwords
// selected under the one condition (v_cmp x3, two mask ops, v_cndmask x2)
namespace loc16 {
template <bool MAX, bool FLOAT>
__device__ __forceinline__ v4u reduce(v4u d, v4u s) {
    v4u out;
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        const int32_t di = (int32_t)d[k + 1], si = (int32_t)s[k + 1];
        const bool take = FLOAT ? loc_take<MAX>(__uint_as_float(d[k]), di, __uint_as_float(s[k]), si)
                                : loc_take<MAX>((int32_t)d[k], di, (int32_t)s[k], si);
        out[k] = take ? s[k] : d[k];
        out[k + 1] = take ? s[k + 1] : d[k + 1];
    }
    return out;
}
}  // namespace loc16
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_MAXLOC, pair_f32_t>(v4u d, v4u s) { return loc16::reduce<true, true>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_MINLOC, pair_f32_t>(v4u d, v4u s) { return loc16::reduce<false, true>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_MAXLOC, pair_i32_t>(v4u d, v4u s) { return loc16::reduce<true, false>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_MINLOC, pair_i32_t>(v4u d, v4u s) { return loc16::reduce<false, false>(d, s); }

// the 16-byte pairs, one per vector: the 64-bit value from dwords 0-1 and the
// 64-bit index from dwords 2-3, compared on all 64 bits (v_cmp_*_f64 or
// v_cmp_*_i64 x2 on the value, v_cmp_lt_i64 on the index), and all four dwords
// selected under the one condition
namespace loc16 {
template <bool MAX, bool FLOAT>
__device__ __forceinline__ v4u reduce_wide(v4u d, v4u s) {
    const uint64_t dvb = ((uint64_t)d[1] << 32) | d[0], svb = ((uint64_t)s[1] << 32) | s[0];
    const int64_t di = (int64_t)(((uint64_t)d[3] << 32) | d[2]), si = (int64_t)(((uint64_t)s[3] << 32) | s[2]);
    const bool take = FLOAT ? loc_take<MAX>(__builtin_bit_cast(double, dvb), di, __builtin_bit_cast(double, svb), si)
                            : loc_take<MAX>((int64_t)dvb, di, (int64_t)svb, si);
    v4u out;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = take ? s[k] : d[k];
    return out;
}
}  // namespace loc16
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_MAXLOC, pair_f64_t>(v4u d, v4u s) { return loc16::reduce_wide<true, true>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_MINLOC, pair_f64_t>(v4u d, v4u s) { return loc16::reduce_wide<false, true>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_MAXLOC, pair_i64_t>(v4u d, v4u s) { return loc16::reduce_wide<true, false>(d, s); }
template <>
__device__ __forceinline__ v4u reduce16<RDC_OP_MINLOC, pair_i64_t>(v4u d, v4u s) { return loc16::reduce_wide<false, false>(d, s); }

// ------------------------------------------------------- memory access ----
__device__ __forceinline__ v4u ld16(const void* p) { return *reinterpret_cast<const v4u*>(p); }
__device__ __forceinline__ void st16(void* p, v4u v) { *reinterpret_cast<v4u*>(p) = v; }
// streaming (non-temporal) forms for once-touched bytes
__device__ __forceinline__ v4u ld16_nt(const void* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p));
}
__device__ __forceinline__ void st16_nt(void* p, v4u v) {
    __builtin_nontemporal_store(v, reinterpret_cast<v4u*>(p));
}

// Write-through stores for bytes a PEER reads (its IPC-mapped scratch, over
// xGMI on a multi-GPU node).  `sc0 sc1` (system scope) stores leave no copy in
// this XCD's L2, so once the storing wave's vmcnt has drained they are at the
// target's memory whatever memory type the IPC import was mapped with (MTYPE
// UC if the driver carries the exporter's uncached flag over, NC — L2-cached,
// written back only by a system release — if it does not).  Plain or `nt`
// stores would depend on that mapping (MI355X_MICROARCH.md visibility table:
// `nt` is not write-through).  16-B form: buffer store with aux = sc0|sc1 from
// a wave-uniform base (cdna_hip_programming.md T8/T20); narrow form: relaxed
// system-scope atomic stores (global_store_{byte,short,dword,dwordx2} sc0 sc1).
constexpr int kWtAux = 1 | 16;  // CPol SC0 | SC1
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wt_rsrc(const void* base) {
    const uint64_t b = (uint64_t)(uintptr_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, 0xffffffffu, 0x00020000);
}
// 16 bytes at base + off (off < 4 GiB; base wave-uniform)
__device__ __forceinline__ void st16_wt(__amdgpu_buffer_rsrc_t r, uint32_t off, v4u v) {
    __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, kWtAux);
}
template <typename W>
__device__ __forceinline__ void st_wt(W* p, W v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// one element of type T (any 1/2/4/8-byte type) written through; a 16-byte
// element (the wide pairs) as two 64-bit words, each written through: there is
// no 128-bit atomic, and an element seen half-written is harmless because every
// hand-off is ordered by its flag, stored after both words were performed
template <typename T>
__device__ __forceinline__ void st_elem_wt(void* p, T v) {
    if constexpr (sizeof(T) == 16) {
        uint64_t w[2];
        __builtin_memcpy(w, &v, 16);
        st_wt(reinterpret_cast<uint64_t*>(p), w[0]);
        st_wt(reinterpret_cast<uint64_t*>(p) + 1, w[1]);
    } else {
        typedef typename std::conditional<sizeof(T) == 1, uint8_t,
                typename std::conditional<sizeof(T) == 2, uint16_t,
                typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type>::type>::type W;
        st_wt(reinterpret_cast<W*>(p), __builtin_bit_cast(W, v));
    }
}

// Where a block_copy writes: this GPU's own memory (user buffers, local
// slots: streaming `nt` stores) or a peer's scratch (write-through, above).
enum { kDstLocal = 0, kDstPeer = 1 };

// System-scope loads for bytes READ FROM a peer's scratch (pull-mode mesh):
// `sc0 sc1` loads are coherent at system scope whatever memory type the
// driver gave the IPC import, so a line of the peer's memory cached in this
// XCD's L2 by an earlier launch (an NC import) is not returned stale — the
// load-side twin of the write-through stores above.  16-B form through a
// wave-uniform descriptor, narrow form as relaxed system-scope atomic loads.
__device__ __forceinline__ v4u ld16_sys(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, kWtAux);
}
template <typename W>
__device__ __forceinline__ W ld_sys(const W* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// one element of type T (any 1/2/4/8-byte type) read at system scope; a
// 16-byte element as two 64-bit system-scope loads (st_elem_wt's twin)
template <typename T>
__device__ __forceinline__ T ld_elem_sys(const void* p) {
    if constexpr (sizeof(T) == 16) {
        const uint64_t w[2] = {ld_sys(reinterpret_cast<const uint64_t*>(p)),
                               ld_sys(reinterpret_cast<const uint64_t*>(p) + 1)};
        T v;
        __builtin_memcpy(&v, w, 16);
        return v;
    } else {
        typedef typename std::conditional<sizeof(T) == 1, uint8_t,
                typename std::conditional<sizeof(T) == 2, uint16_t,
                typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type>::type>::type W;
        return __builtin_bit_cast(T, ld_sys(reinterpret_cast<const W*>(p)));
    }
}

// ------------------------------------------------------------- hand-off ----
// Hand-off flags are 64-bit words holding a launch's sequence number:
//   seq = (counter << kTagBits) | tag
// counter: the channel's launch count (every communicator sharing a channel
// draws from one counter, 56 bits: it never wraps in practice, so a slot no
// launch has written yet (0) or one idle for any number of launches never
// looks "reached"); tag: the launching communicator's tag on that channel.
// Hand-off flags carry the whole word, so a rank waiting for launch k of
// communicator X that finds launch k of communicator Y — ranks that issued two
// communicators' collectives in different orders — fails with RDC_KERR_ORDER
// instead of folding unrelated buffers.  "Done" words (a peer finished launch
// k-1, whichever communicator issued it) compare the counter only.
constexpr uint32_t kTagBits = 8;
constexpr uint64_t kTagMask = (1ull << kTagBits) - 1ull;
__device__ __forceinline__ uint64_t flag_load(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void flag_store(uint64_t* p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint64_t seq_counter(uint64_t seq) { return seq >> kTagBits; }
// counter of v >= counter of seq (modulo 2^56)
__device__ __forceinline__ bool seq_reached(uint64_t v, uint64_t seq) {
    return (int64_t)((seq_counter(v) - seq_counter(seq)) << kTagBits) >= 0;
}
__device__ __forceinline__ bool same_tag(uint64_t v, uint64_t seq) { return ((v ^ seq) & kTagMask) == 0; }
// the previous launch's number (counter - 1, same tag; compared untagged)
__device__ __forceinline__ uint64_t seq_prev(uint64_t seq) { return seq - (1ull << kTagBits); }

// Called by EVERY thread of the block after its payload stores.  Lanes
// 0..nflags-1 of wave 0 then store flags[i] = seq.
// Every hand-off payload lives in the peers' scratch slots and is stored
// write-through (st16_wt / block_copy<kDstPeer>: sc0 sc1), so every storing
// wave's `s_waitcnt vmcnt(0)` (before the barrier) means it has been
// performed at the owner's memory: the write-through + drained-flag form of
// MI355X_MICROARCH.md ("Valid forms", R1) at system scope.  When the scratch
// is uncached (MTYPE UC, hipDeviceMallocUncached: `uc`) the owner's loads
// never hit a stale line either, and the system-scope release fence would
// only add an L2 write-back (buffer_wbl2 sc0 sc1, 1.7-6.5 us per call) of
// cached lines no peer reads, so it is issued only for fine- / coarse-grained
// scratch (alloc fallbacks).
// verify (RDC_VERIFY_PUBLISH, debug): each storing lane reads its flag back
// through the same mapping until it sees seq (bounded), and counts in
// verify[0] the stores it never saw, recording the last such flag address in
// verify[2..3] — does a store the writer made stay invisible to the writer too?
__device__ __forceinline__ void verify_flag(uint64_t* f, uint64_t seq, uint32_t* verify) {
    for (int i = 0; i < (1 << 14); ++i) {
        if (seq_counter(flag_load(f)) == seq_counter(seq)) return;
        __builtin_amdgcn_s_sleep(2);
    }
    __hip_atomic_fetch_add(verify, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<uint64_t*>(verify + 2), (uint64_t)(uintptr_t)f, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void block_publish(uint64_t* const* flags, int nflags, uint64_t seq, int uc,
                                              uint32_t* verify = nullptr) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x < (unsigned)nflags) {
        if (!uc) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        flag_store(flags[threadIdx.x], seq);
        if (verify) verify_flag(flags[threadIdx.x], seq, verify);
    }
}

__device__ __forceinline__ void block_publish1(uint64_t* flag, uint64_t seq, int uc) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        if (!uc) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        flag_store(flag, seq);
    }
}

struct Abort {
    uint32_t* err;          // local error word (device memory), 0 = ok
    uint64_t deadline;      // wall_clock64() value after which we give up
    int poll_rmw = 0;       // RDC_POLL_RMW (debug): poll with a system-scope atomic add of 0
};

// Block-wide wait until every flags[i] (i < nflags <= 64) reached seq.  Wave 0
// polls (one lane per flag), sleeping between polls; the other waves park at
// the barrier.  Returns false (uniformly) on timeout or if another block of
// this launch already aborted.  tagged (hand-off flags of this launch): a
// flag that reached the counter with another communicator's tag is an order
// violation (RDC_KERR_ORDER, immediate); untagged (done words): the counter only.  With cached scratch the matching lane then
// runs a system-scope acquire (L2 / L1 invalidate) so the block's plain loads
// of the handed-off bytes cannot hit stale lines; uncached scratch (`uc`) is
// never held in any GPU cache, so its loads after the matched poll read
// memory and need no invalidate (MI355X_MICROARCH.md: an acquire is ≈1.7 us).
__device__ __forceinline__ bool block_wait(uint64_t* const* flags, int nflags, uint64_t seq,
                                           const Abort& ab, uint32_t code, int uc, bool tagged = true) {
    __shared__ int s_ok;
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        bool mine = lane >= nflags;
        bool ok = true;
        bool wrong = false;  // this lane's flag reached the counter with another tag
        uint32_t spins = 0;
        uint64_t seen = 0;   // this lane's last flag value
        while (true) {
            if (!mine) {
                const uint64_t v = ab.poll_rmw ? __hip_atomic_fetch_add(flags[lane], (uint64_t)0, __ATOMIC_RELAXED,
                                                                        __HIP_MEMORY_SCOPE_SYSTEM)
                                               : flag_load(flags[lane]);
                seen = v;
                if (seq_reached(v, seq)) {
                    if (!tagged || same_tag(v, seq)) mine = true;
                    else wrong = true;
                }
            }
            if (__all(mine)) break;
            if (__any(wrong)) {
                code = RDC_KERR_ORDER;
                ok = false;
                break;
            }
            if ((++spins & 63) == 0) {
                bool dead = wall_clock64() > ab.deadline ||
                            __hip_atomic_load(ab.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
                if (__any(dead)) { ok = false; break; }
            }
            __builtin_amdgcn_s_sleep(1);
        }
        if (!ok) {
            // the first wait to give up records what it waited for (err words
            // 64..71: claim, -, seq, flag value, flag address), before the
            // error word tells the other blocks to give up
            const uint64_t open = __ballot(!mine);
            if (open != 0 && lane == (int)__builtin_ctzll(open)) {
                uint32_t expected = 0;
                if (__hip_atomic_compare_exchange_strong(ab.err + 64, &expected, 1u, __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    uint64_t* d = reinterpret_cast<uint64_t*>(ab.err + 66);
                    __hip_atomic_store(d, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(d + 1, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(d + 2, (uint64_t)(uintptr_t)flags[lane], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                    // the same flag read five ways once more (err words 96..107):
                    // a relaxed system-scope load, an atomic add of 0 at system
                    // scope, a load after a system-scope acquire (L1 / L2
                    // invalidate), a non-temporal load, and this wave's XCC —
                    // which view still shows the old value after the wait gave up
                    uint64_t* f = flags[lane];
                    const uint64_t v1 = flag_load(f);
                    const uint64_t v2 = __hip_atomic_fetch_add(f, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
                    const uint64_t v3 = flag_load(f);
                    const uint64_t v4 = __builtin_nontemporal_load(f);
                    const uint64_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 0xf;
                    uint64_t* pr = reinterpret_cast<uint64_t*>(ab.err + 96);
                    __hip_atomic_store(pr, v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(pr + 1, v2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(pr + 2, v3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(pr + 3, v4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(pr + 4, xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        if (lane == 0) {
            if (ok && !uc) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else if (!ok) {
                uint32_t expected = 0;
                __hip_atomic_compare_exchange_strong(ab.err, &expected, code, __ATOMIC_RELAXED,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            s_ok = ok;
        }
    }
    __syncthreads();
    const bool ok = s_ok != 0;
    __syncthreads();  // s_ok reused by the next wait
    return ok;
}

// ------------------------------------------------------ block-wide moves ----
// Byte ranges [0,len).  Scratch images sit at the buffer-relative alignment
// (offset % 16), so they are congruent with the user buffer whenever the
// user pointer is 16-B aligned: then the middle runs as 16-byte lanes and
// only the <16-byte head/tail goes element-wise.  A rank whose pointer is
// not 16-B aligned takes the narrow path (units of the widest common
// alignment), still exact.
//
// Where a block_copy reads: this rank's own bytes (user buffers, kSrcLocal:
// streaming `nt` loads) or bytes another rank handed off through scratch
// (kSrcHandoff: `sc0 sc1` loads, ld16_sys / ld_sys) — every load of a
// handed-off byte is a system-scope load, so the consumer side of every
// hand-off is the "sc0 sc1 stores and loads both sides" form of
// MI355X_MICROARCH.md ("Valid forms") whatever memory type backs the scratch
// or its IPC import.
enum { kSrcLocal = 0, kSrcHandoff = 1 };

template <int DST, typename W>
__device__ __forceinline__ void put_word(W* p, W v) {
    if (DST == kDstPeer) st_wt(p, v);
    else *p = v;
}
template <int SRC, typename W>
__device__ __forceinline__ W get_word(const W* p) {
    if (SRC == kSrcHandoff) return ld_sys(p);
    return *p;
}

// dst[i] = src[i], dst and src congruent mod 16.  The 16-B body walks windows
// of U x blockDim vectors; the window base is wave-uniform, so a peer
// destination or a handed-off source gets one buffer descriptor per window
// (offsets < 4 GiB).
template <int DST, int SRC>
__device__ __forceinline__ void block_copy_vec(char* __restrict__ dst, const char* __restrict__ src,
                                               uint64_t len) {
    const uint64_t mis = (uint64_t)(uintptr_t)src & 15;
    uint64_t head = mis ? (16 - mis) : 0;
    if (head > len) head = len;
    const uint64_t nvec = (len - head) >> 4;
    const uint64_t tail_start = head + (nvec << 4);
    const unsigned tid = threadIdx.x;
    if (tid < head) put_word<DST, char>(dst + tid, (char)get_word<SRC, uint8_t>(reinterpret_cast<const uint8_t*>(src) + tid));
    if (tid < len - tail_start)
        put_word<DST, char>(dst + tail_start + tid,
                            (char)get_word<SRC, uint8_t>(reinterpret_cast<const uint8_t*>(src) + tail_start + tid));
    const v4u* s = reinterpret_cast<const v4u*>(src + head);
    v4u* d = reinterpret_cast<v4u*>(dst + head);
    constexpr int U = 8;  // 32 KiB in flight per 256-thread block
    const uint64_t step = (uint64_t)blockDim.x;
    for (uint64_t ib = 0; ib < nvec; ib += U * step) {
        const uint64_t i = ib + tid;
        const __amdgpu_buffer_rsrc_t rsrc_s = wt_rsrc(SRC == kSrcHandoff ? s + ib : s);  // dead for kSrcLocal
        auto load = [&](int u) -> v4u {
            if (SRC == kSrcHandoff) return ld16_sys(rsrc_s, (uint32_t)((tid + u * step) * 16));
            return ld16_nt(s + i + u * step);
        };
        if (ib + U * step <= nvec) {
            v4u v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = load(u);
            if (DST == kDstPeer) {
                const __amdgpu_buffer_rsrc_t rs = wt_rsrc(d + ib);
#pragma unroll
                for (int u = 0; u < U; ++u) st16_wt(rs, (uint32_t)((tid + u * step) * 16), v[u]);
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) st16_nt(d + i + u * step, v[u]);
            }
        } else {
            const __amdgpu_buffer_rsrc_t rs = wt_rsrc(d + ib);
            for (int u = 0; u < U; ++u) {
                if (i + u * step >= nvec) break;
                const v4u v = load(u);
                if (DST == kDstPeer) st16_wt(rs, (uint32_t)((tid + u * step) * 16), v);
                else st16_nt(d + i + u * step, v);
            }
        }
    }
}

template <int DST, int SRC, typename W>
__device__ __forceinline__ void block_copy_words(char* dst, const char* src, uint64_t len) {
    const uint64_t mis = (uint64_t)(uintptr_t)src & (sizeof(W) - 1);
    uint64_t head = mis ? sizeof(W) - mis : 0;
    if (head > len) head = len;
    const uint64_t nw = (len - head) / sizeof(W);
    const uint64_t tail_start = head + nw * sizeof(W);
    const unsigned tid = threadIdx.x;
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(src);
    if (tid < head) put_word<DST, char>(dst + tid, (char)get_word<SRC, uint8_t>(sb + tid));
    if (tid < len - tail_start) put_word<DST, char>(dst + tail_start + tid, (char)get_word<SRC, uint8_t>(sb + tail_start + tid));
    const W* s = reinterpret_cast<const W*>(src + head);
    W* d = reinterpret_cast<W*>(dst + head);
    for (uint64_t i = tid; i < nw; i += blockDim.x) put_word<DST, W>(d + i, get_word<SRC, W>(s + i));
}

// DST: kDstLocal (this GPU's memory) or kDstPeer (a peer's IPC-mapped scratch);
// SRC: kSrcLocal (this rank's bytes) or kSrcHandoff (bytes a peer handed off)
template <int DST, int SRC = kSrcLocal>
__device__ __forceinline__ void block_copy(char* __restrict__ dst, const char* __restrict__ src, uint64_t len) {
    const uintptr_t x = ((uintptr_t)dst ^ (uintptr_t)src) & 15;
    if (x == 0) block_copy_vec<DST, SRC>(dst, src, len);
    else if ((x & 7) == 0) block_copy_words<DST, SRC, uint64_t>(dst, src, len);
    else if ((x & 3) == 0) block_copy_words<DST, SRC, uint32_t>(dst, src, len);
    else if ((x & 1) == 0) block_copy_words<DST, SRC, uint16_t>(dst, src, len);
    else block_copy_words<DST, SRC, uint8_t>(dst, src, len);
}

// dst (this GPU's memory) = src (a PEER's scratch or this rank's own scratch
// written by a peer), every load at system scope: landing handed-off bytes.
__device__ __forceinline__ void block_copy_pull(char* __restrict__ dst, const char* __restrict__ src, uint64_t len) {
    block_copy<kDstLocal, kSrcHandoff>(dst, src, len);
}

// ------------------------------------------------------------ poison mode ----
// RDC_POISON_SCRATCH=1 (CollArgs::poison): after its last read of a scratch
// range in a launch, the consumer overwrites it with 0xFF bytes (write-through:
// the range may be a peer's), before the signal that lets the producer reuse
// it.  A read of the range before the producer's next publish then folds or
// lands NaN / all-ones words instead of a plausible older value (DESIGN.md
// §4.2, debug mode; the tests run with it on).
__device__ __forceinline__ void block_poison(char* p, uint64_t len) {
    const uint64_t mis = (uint64_t)(uintptr_t)p & 15;
    uint64_t head = mis ? 16 - mis : 0;
    if (head > len) head = len;
    const uint64_t nvec = (len - head) >> 4;
    const uint64_t tail = head + (nvec << 4);
    const unsigned tid = threadIdx.x;
    if (tid < head) st_wt<uint8_t>(reinterpret_cast<uint8_t*>(p) + tid, 0xff);
    if (tid < len - tail) st_wt<uint8_t>(reinterpret_cast<uint8_t*>(p) + tail + tid, 0xff);
    const v4u ones = {~0u, ~0u, ~0u, ~0u};
    const uint64_t step = (uint64_t)blockDim.x;
    constexpr int U = 8;
    for (uint64_t ib = 0; ib < nvec; ib += U * step) {
        const __amdgpu_buffer_rsrc_t rs = wt_rsrc(p + head + ib * 16);
        for (int u = 0; u < U; ++u) {
            if (ib + tid + u * step >= nvec) break;
            st16_wt(rs, (uint32_t)((tid + u * step) * 16), ones);
        }
    }
}

}  // namespace rdc_amd
