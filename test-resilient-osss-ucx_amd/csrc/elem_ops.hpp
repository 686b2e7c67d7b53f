// elem_ops.hpp -- device element operations of the reduce-to-all combine.
//
// Each functor is op(acc, in) with `acc` the running accumulator (the first
// operand), exactly like the reference's function-pointer fold
// `write_to[ti] = (*the_op)(write_to[ti], pWrk[j])` (src/reductions.c:95-96)
// over the one-line ops of src/shmemu/miscops.c:12-105.
//
// The floating-point model (documented in DESIGN.md, section "Numerics"):
//  * non-NaN results: IEEE-754 RNE, subnormals kept, never contracted (this
//    file is compiled with -ffp-contract=off and the pragma below);
//  * NaN results reproduce the x86-64 SSE rule of the reference build: the
//    first source operand's NaN (quieted) wins, then the second's, and an
//    invalid operation yields the NEGATIVE default NaN (0xFFF8.. / 0xFFC0..);
//  * min/max are compare + select (`a<b?a:b`), never v_min/v_max, so NaNs and
//    signed zeros resolve to the right operand exactly like the reference;
//  * complex product = GCC's inline expansion + libgcc __mul{s,d}c3 (C99
//    Annex G recovery) as compiled for the reference (operand orders from the
//    disassembly, see oracle/oracle_ops.c);
//  * integers wrap modulo 2^w (unsigned arithmetic, no UB).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

// host + device: the kernels, and the host fold of small host-heap calls
// (host_fold.hip) -- one definition of every element op for both
#define OSGPU_EHD __host__ __device__ __forceinline__

namespace osgpu {

struct cfloat { float re, im; };
struct cdouble { double re, im; };

// ---------------------------------------------------------------- bit utils
OSGPU_EHD uint64_t bits(double x) { return __builtin_bit_cast(uint64_t, x); }
OSGPU_EHD double dbl(uint64_t u) { return __builtin_bit_cast(double, u); }
OSGPU_EHD uint32_t bits(float x) { return __builtin_bit_cast(uint32_t, x); }
OSGPU_EHD float flt(uint32_t u) { return __builtin_bit_cast(float, u); }

OSGPU_EHD bool isnan_(double x) { return (bits(x) << 1) > (0x7ff0000000000000ull << 1); }
OSGPU_EHD bool isnan_(float x) { return (bits(x) << 1) > (0x7f800000u << 1); }
OSGPU_EHD bool isinf_(double x) { return (bits(x) << 1) == (0x7ff0000000000000ull << 1); }
OSGPU_EHD bool isinf_(float x) { return (bits(x) << 1) == (0x7f800000u << 1); }

OSGPU_EHD double quiet(double x) { return dbl(bits(x) | 0x0008000000000000ull); }
OSGPU_EHD float quiet(float x) { return flt(bits(x) | 0x00400000u); }
OSGPU_EHD double defnan(double) { return dbl(0xfff8000000000000ull); }
OSGPU_EHD float defnan(float) { return flt(0xffc00000u); }

// SSE NaN selection for `r = a OP b` with first source a.  The branch is
// taken only when r is NaN, so the streaming fast path pays one compare.
template <typename F>
OSGPU_EHD F sse(F r, F a, F b)
{
    if (__builtin_expect(r != r, 0)) {
        r = isnan_(a) ? quiet(a) : (isnan_(b) ? quiet(b) : defnan(a));
    }
    return r;
}
template <typename F> OSGPU_EHD F add(F a, F b) { return sse<F>(a + b, a, b); }
template <typename F> OSGPU_EHD F sub(F a, F b) { return sse<F>(a - b, a, b); }
template <typename F> OSGPU_EHD F mul(F a, F b) { return sse<F>(a * b, a, b); }

template <typename F>
OSGPU_EHD F copysign_(F mag, F sgn);
template <>
OSGPU_EHD double copysign_(double m, double s)
{
    return dbl((bits(m) & 0x7fffffffffffffffull) | (bits(s) & 0x8000000000000000ull));
}
template <>
OSGPU_EHD float copysign_(float m, float s)
{
    return flt((bits(m) & 0x7fffffffu) | (bits(s) & 0x80000000u));
}

// libgcc2.c __mul{s,d}c3, GCC 11.4, with the operand order of its compiled
// body: ac=a*c bd=b*d ad=a*d bc=c*b; x=ac-bd; y=ad+bc; recovery
// x=(a*c-b*d)*inf, y=inf*(a*d+b*c).  Reached only when the inline product
// has a NaN part, so it lives off the fast path.
template <typename F>
struct CPair {
    F x, y;
};
// returned by value (in registers): no stack frame on the fast path's kernels
template <typename F>
__host__ __device__ __attribute__((noinline)) CPair<F> mulc3(F a, F b, F c, F d)
{
    const F one = 1, zero = 0, inf = __builtin_huge_val();
    F ac = mul(a, c), bd = mul(b, d), ad = mul(a, d), bc = mul(c, b);
    F x = sub(ac, bd), y = add(ad, bc);
    if (isnan_(x) && isnan_(y)) {
        bool recalc = false;
        if (isinf_(a) || isinf_(b)) {
            a = copysign_(isinf_(a) ? one : zero, a);
            b = copysign_(isinf_(b) ? one : zero, b);
            if (isnan_(c)) c = copysign_(zero, c);
            if (isnan_(d)) d = copysign_(zero, d);
            recalc = true;
        }
        if (isinf_(c) || isinf_(d)) {
            c = copysign_(isinf_(c) ? one : zero, c);
            d = copysign_(isinf_(d) ? one : zero, d);
            if (isnan_(a)) a = copysign_(zero, a);
            if (isnan_(b)) b = copysign_(zero, b);
            recalc = true;
        }
        if (!recalc && (isinf_(ac) || isinf_(bd) || isinf_(ad) || isinf_(bc))) {
            if (isnan_(a)) a = copysign_(zero, a);
            if (isnan_(b)) b = copysign_(zero, b);
            if (isnan_(c)) c = copysign_(zero, c);
            if (isnan_(d)) d = copysign_(zero, d);
            recalc = true;
        }
        if (recalc) {
            x = mul(sub(mul(a, c), mul(b, d)), inf);
            y = mul(inf, add(mul(a, d), mul(b, c)));
        }
    }
    return CPair<F>{x, y};
}

// --------------------------------------------------------------- functors
// Integer ops run on the unsigned image so overflow wraps (miscops.c:12-39
// compiled by gcc wraps; short is promoted to int and truncated, whose low
// 16 bits equal 16-bit wrapping arithmetic).
template <typename T> struct Unsigned;
// int16 runs in 32-bit unsigned (low 16 bits identical, no int-promotion UB)
template <> struct Unsigned<int16_t> { using type = uint32_t; };
template <> struct Unsigned<int32_t> { using type = uint32_t; };
template <> struct Unsigned<int64_t> { using type = uint64_t; };

enum OpCode { OP_SUM = 0, OP_PROD, OP_AND, OP_OR, OP_XOR, OP_MAX, OP_MIN };

template <typename T, int OP> struct Elem;

// integers ---------------------------------------------------------------
template <typename T> struct Elem<T, OP_SUM> {
    OSGPU_EHD static T f(T a, T b)
    {
        using U = typename Unsigned<T>::type;
        return (T) (U) ((U) a + (U) b);
    }
};
template <typename T> struct Elem<T, OP_PROD> {
    OSGPU_EHD static T f(T a, T b)
    {
        using U = typename Unsigned<T>::type;
        return (T) (U) ((U) a * (U) b);
    }
};
template <typename T> struct Elem<T, OP_AND> { OSGPU_EHD static T f(T a, T b) { return a & b; } };
template <typename T> struct Elem<T, OP_OR> { OSGPU_EHD static T f(T a, T b) { return a | b; } };
template <typename T> struct Elem<T, OP_XOR> { OSGPU_EHD static T f(T a, T b) { return a ^ b; } };
// compare + select: exact for every type, including NaN / signed zero
template <typename T> struct Elem<T, OP_MAX> { OSGPU_EHD static T f(T a, T b) { return a > b ? a : b; } };
template <typename T> struct Elem<T, OP_MIN> { OSGPU_EHD static T f(T a, T b) { return a < b ? a : b; } };

// real floating point ------------------------------------------------------
template <> struct Elem<float, OP_SUM> { OSGPU_EHD static float f(float a, float b) { return add(a, b); } };
template <> struct Elem<float, OP_PROD> { OSGPU_EHD static float f(float a, float b) { return mul(a, b); } };
template <> struct Elem<double, OP_SUM> { OSGPU_EHD static double f(double a, double b) { return add(a, b); } };
template <> struct Elem<double, OP_PROD> { OSGPU_EHD static double f(double a, double b) { return mul(a, b); } };

// complex ----------------------------------------------------------------
// complexd sum: compiled as addsd %xmm3,%xmm1 ; addsd %xmm2,%xmm0 (a first)
template <> struct Elem<cdouble, OP_SUM> {
    OSGPU_EHD static cdouble f(cdouble a, cdouble b)
    {
        return cdouble{add(a.re, b.re), add(a.im, b.im)};
    }
};
// complexf sum: the compiled body adds the imaginary parts as b.im + a.im
template <> struct Elem<cfloat, OP_SUM> {
    OSGPU_EHD static cfloat f(cfloat a, cfloat b)
    {
        return cfloat{add(a.re, b.re), add(b.im, a.im)};
    }
};
template <typename C, typename F>
OSGPU_EHD C cmul(C p, C q)
{
    F a = p.re, b = p.im, c = q.re, d = q.im;
    F x = a * c - b * d;   // inline fast path; any NaN part -> libgcc path
    F y = a * d + b * c;
    if (__builtin_expect(x != x || y != y, 0)) {
        const CPair<F> r = mulc3<F>(a, b, c, d);
        x = r.x;
        y = r.y;
    }
    return C{x, y};
}
template <> struct Elem<cdouble, OP_PROD> {
    OSGPU_EHD static cdouble f(cdouble a, cdouble b) { return cmul<cdouble, double>(a, b); }
};
template <> struct Elem<cfloat, OP_PROD> {
    OSGPU_EHD static cfloat f(cfloat a, cfloat b) { return cmul<cfloat, float>(a, b); }
};

// 16-bit floating point (extension types) ----------------------------------
// An element is a 16-bit pattern: IEEE-754 binary16 (half_t) or bfloat16
// (bf16_t, 1-8-7).  Two distinct class types, not int16_t: the op set and
// the fold order are picked by type (kernel_common.hpp dispatch_op).
//  * sum / prod: the correctly rounded (RNE) result in the element's own
//    format, subnormals kept, overflow to +-inf.  Defined as: widen both
//    operands to float (exact), ONE float operation, narrow RNE -- the double
//    rounding is innocuous because float's 24 significand bits are at least
//    2 * 11 + 2 and 2 * 8 + 2.  The host takes that route with an integer
//    narrowing; the device takes v_add_f16 / v_mul_f16 (v_pk_* when the
//    compiler pairs them) for half_t, which is the same function, and f32
//    arithmetic + v_cvt_pk_bf16_f32 for bf16_t;
//  * NaN results: the SSE rule at the element's width -- the first operand's
//    NaN quieted (| 0x0200 / | 0x0040, payload and sign kept), else the
//    second's, else (inf - inf, 0 * inf) the negative default NaN 0xFE00 /
//    0xFFC0;
//  * max / min: compare on the values, select the chosen operand's 16 bits.
struct half_t { uint16_t u; };
struct bf16_t { uint16_t u; };

template <typename T> struct is_f16 { static constexpr bool value = false; };
template <> struct is_f16<half_t> { static constexpr bool value = true; };
template <> struct is_f16<bf16_t> { static constexpr bool value = true; };

OSGPU_EHD bool isnan_(half_t x) { return (x.u & 0x7fffu) > 0x7c00u; }
OSGPU_EHD bool isnan_(bf16_t x) { return (x.u & 0x7fffu) > 0x7f80u; }
OSGPU_EHD half_t quiet(half_t x) { return half_t{(uint16_t) (x.u | 0x0200u)}; }
OSGPU_EHD bf16_t quiet(bf16_t x) { return bf16_t{(uint16_t) (x.u | 0x0040u)}; }
OSGPU_EHD half_t defnan(half_t) { return half_t{0xfe00u}; }
OSGPU_EHD bf16_t defnan(bf16_t) { return bf16_t{0xffc0u}; }

// exact widening (every binary16 / bfloat16 value is a float)
OSGPU_EHD float widen(bf16_t x) { return flt((uint32_t) x.u << 16); }
OSGPU_EHD float widen(half_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (float) __builtin_bit_cast(_Float16, x.u);
#else
    const uint32_t s = (uint32_t) (x.u & 0x8000u) << 16, e = (x.u >> 10) & 0x1fu, m = x.u & 0x3ffu;
    if (e == 0) return flt(s | bits((float) m * 0x1p-24f));  // zero / subnormal: m * 2^-24
    if (e == 31) return flt(s | 0x7f800000u | (m << 13));
    return flt(s | ((e + 112u) << 23) | (m << 13));
#endif
}

// RNE narrowing of a float; a NaN narrows to some NaN (callers replace it)
OSGPU_EHD bf16_t narrow(float r, bf16_t)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return bf16_t{__builtin_bit_cast(uint16_t, (__bf16) r)};  // v_cvt_pk_bf16_f32
#else
    const uint32_t x = bits(r);
    if ((x << 1) > (0x7f800000u << 1)) return bf16_t{(uint16_t) ((x >> 16) | 0x0040u)};
    return bf16_t{(uint16_t) ((x + 0x7fffu + ((x >> 16) & 1u)) >> 16)};
#endif
}
OSGPU_EHD half_t narrow(float r, half_t)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return half_t{__builtin_bit_cast(uint16_t, (_Float16) r)};
#else
    const uint32_t x = bits(r) & 0x7fffffffu, s = (bits(r) >> 16) & 0x8000u;
    uint32_t o;
    if (x > 0x7f800000u) o = 0x7e00u;
    else if (x >= 0x47800000u) o = 0x7c00u;  // 2^16 and above, inf
    else if (x < 0x38800000u)                // below 2^-14: a multiple of 2^-24, by the
        o = bits(flt(x) + 0.5f) - 0x3f000000u;  // float adder's own RNE at 0.5's ulp
    else {
        const uint32_t y = x - 0x38000000u;  // exponent rebias; a carry out of the
        o = (y + 0xfffu + ((y >> 13) & 1u)) >> 13;  // significand steps the exponent (to inf)
    }
    return half_t{(uint16_t) (s | o)};
#endif
}

// a OP b rounded once to the element's format; a NaN result is SOME NaN
template <typename H, int OP>
OSGPU_EHD H arith16(H a, H b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (__is_same(H, half_t)) {
        const _Float16 x = __builtin_bit_cast(_Float16, a.u), y = __builtin_bit_cast(_Float16, b.u);
        return half_t{__builtin_bit_cast(uint16_t, (_Float16) (OP == OP_SUM ? x + y : x * y))};
    }
#endif
    const float x = widen(a), y = widen(b);
    return narrow(OP == OP_SUM ? x + y : x * y, H{});
}
OSGPU_EHD bool gt16(bf16_t a, bf16_t b) { return widen(a) > widen(b); }
OSGPU_EHD bool lt16(bf16_t a, bf16_t b) { return widen(a) < widen(b); }
OSGPU_EHD bool eq16(bf16_t a, bf16_t b) { return widen(a) == widen(b); }
#if defined(__HIP_DEVICE_COMPILE__)
OSGPU_EHD bool eq16(half_t a, half_t b)
{
    return __builtin_bit_cast(_Float16, a.u) == __builtin_bit_cast(_Float16, b.u);
}
#else
OSGPU_EHD bool eq16(half_t a, half_t b) { return widen(a) == widen(b); }
#endif
#if defined(__HIP_DEVICE_COMPILE__)
OSGPU_EHD bool gt16(half_t a, half_t b)
{
    return __builtin_bit_cast(_Float16, a.u) > __builtin_bit_cast(_Float16, b.u);
}
OSGPU_EHD bool lt16(half_t a, half_t b)
{
    return __builtin_bit_cast(_Float16, a.u) < __builtin_bit_cast(_Float16, b.u);
}
#else
OSGPU_EHD bool gt16(half_t a, half_t b) { return widen(a) > widen(b); }
OSGPU_EHD bool lt16(half_t a, half_t b) { return widen(a) < widen(b); }
#endif

template <typename H, int OP> struct Elem16 {
    OSGPU_EHD static H f(H a, H b)
    {
        if (OP == OP_MAX) return gt16(a, b) ? a : b;
        if (OP == OP_MIN) return lt16(a, b) ? a : b;
        H r = arith16<H, OP>(a, b);
        if (__builtin_expect(isnan_(r), 0))
            r = isnan_(a) ? quiet(a) : (isnan_(b) ? quiet(b) : defnan(a));
        return r;
    }
};
template <> struct Elem<half_t, OP_SUM> : Elem16<half_t, OP_SUM> {};
template <> struct Elem<half_t, OP_PROD> : Elem16<half_t, OP_PROD> {};
template <> struct Elem<half_t, OP_MAX> : Elem16<half_t, OP_MAX> {};
template <> struct Elem<half_t, OP_MIN> : Elem16<half_t, OP_MIN> {};
template <> struct Elem<bf16_t, OP_SUM> : Elem16<bf16_t, OP_SUM> {};
template <> struct Elem<bf16_t, OP_PROD> : Elem16<bf16_t, OP_PROD> {};
template <> struct Elem<bf16_t, OP_MAX> : Elem16<bf16_t, OP_MAX> {};
template <> struct Elem<bf16_t, OP_MIN> : Elem16<bf16_t, OP_MIN> {};

// ------------------------------------------------ max / min with location
// One step of osgpu_reduce_loc's ascending fold (OP_MAX / OP_MIN over the
// ordered types): the running pair (v, i) takes member j's pair (b, ib).
//   v before b (v > b for max, v < b for min): (v, i) stays;
//   v == b:  v becomes b -- what Elem<T, OP>::f returns -- and i = min(i, ib);
//   else (b before v, or unordered): (b, ib).
// Comparisons are on values: a NaN compares false both ways, so it replaces
// what came before it and is replaced by what comes after it; +0 == -0.  The
// value part IS Elem<T, OP>::f, so the values are the uniform reduce's bits.
// Indices compare as signed 32-bit integers.
template <typename T, int OP> struct LocStep {
    static_assert(OP == OP_MAX || OP == OP_MIN, "max / min only");
    OSGPU_EHD static bool before(T a, T b)
    {
        if constexpr (is_f16<T>::value) return OP == OP_MAX ? gt16(a, b) : lt16(a, b);
        else return OP == OP_MAX ? a > b : a < b;
    }
    OSGPU_EHD static bool same(T a, T b)
    {
        if constexpr (is_f16<T>::value) return eq16(a, b);
        else return a == b;
    }
    OSGPU_EHD static void f(T &v, int32_t &i, T b, int32_t ib)
    {
        const bool keep = before(v, b), tie = same(v, b);
        const int32_t lo = i < ib ? i : ib;
        i = keep ? i : (tie ? lo : ib);
        v = Elem<T, OP>::f(v, b);
    }
};

// ------------------------------------------------ float-accumulated sum
// The steps of osgpu_reduce_wsum (include/osgpu_reduce.h Part 1i) for
// H = half_t / bf16_t: the members' values are added in a FLOAT accumulator
// and narrowed once.
//   widen   exact, NaNs included: a 16-bit NaN keeps sign, payload and its
//           signalling bit (in integers: v_cvt_f32_f16 would quiet it);
//   add     one float add by the SSE rule above (add<float>): a NaN
//           accumulator stays, quieted, else a NaN operand is taken, quieted,
//           else inf - inf gives 0xFFC00000;
//   narrow  RNE (narrow() above); a NaN accumulator is TRUNCATED -- bfloat16
//           bits >> 16, half sign | 0x7C00 | mantissa >> 13 -- which is
//           lossless: every NaN the accumulator can hold is a widened 16-bit
//           NaN, quieted or not, or the default NaN.
// widen_fast / the plain + are the streaming kernels' branch-free forms: equal
// to the exact ones whenever the FINAL accumulator is no NaN (a NaN, once met
// or made, stays through every later add).
OSGPU_EHD float widen_nan(half_t x)
{
    return flt(((uint32_t) (x.u & 0x8000u) << 16) | 0x7f800000u | ((uint32_t) (x.u & 0x3ffu) << 13));
}
OSGPU_EHD float widen_nan(bf16_t x) { return flt((uint32_t) x.u << 16); }
OSGPU_EHD half_t truncate_nan(uint32_t u, half_t)
{
    return half_t{(uint16_t) (((u >> 16) & 0x8000u) | 0x7c00u | ((u >> 13) & 0x3ffu))};
}
OSGPU_EHD bf16_t truncate_nan(uint32_t u, bf16_t) { return bf16_t{(uint16_t) (u >> 16)}; }

template <typename H> struct WsumStep {
    OSGPU_EHD static float widen(H x)
    {
        if (__builtin_expect(isnan_(x), 0)) return widen_nan(x);
        return osgpu::widen(x);
    }
    OSGPU_EHD static float widen_fast(H x) { return osgpu::widen(x); }
    OSGPU_EHD static float add(float acc, H x) { return osgpu::add<float>(acc, widen(x)); }
    OSGPU_EHD static H narrow(float acc)
    {
        if (__builtin_expect(isnan_(acc), 0)) return truncate_nan(bits(acc), H{});
        return osgpu::narrow(acc, H{});
    }
    // the target's element: the accumulator itself, or narrowed
    OSGPU_EHD static void out(float acc, float &o) { o = acc; }
    OSGPU_EHD static void out(float acc, H &o) { o = narrow(acc); }
};

// ------------------------------------------------------- branch-free folds
// Fast<T, OP>::f is Elem<T, OP>::f without its NaN handling (the SSE rule,
// the complex product's libgcc recovery): one instruction stream with no
// branch per element, so a streaming kernel keeps every load in flight.
// It differs from Elem::f only where that result has a NaN part, and a NaN
// part, once there, stays through every later + and * of a fold (x + NaN,
// x * NaN and both complex formulas give NaN in it).  So a fold whose FINAL
// value has no NaN part (Fast::bad false) is bit-identical to the exact
// fold; kernels test the final values of a tile and recompute the tile with
// Elem::f only where some lane's is flagged.  Ops without NaN handling
// (integers, min/max, which never produce a NaN of their own) are exact:
// kChecked = false and the test compiles away.
template <typename T, int OP> struct Fast {
    static constexpr bool kChecked = false;
    OSGPU_EHD static T f(T a, T b) { return Elem<T, OP>::f(a, b); }
    OSGPU_EHD static bool bad(T) { return false; }
};
template <typename F, int OP> struct FastReal {
    static constexpr bool kChecked = true;
    OSGPU_EHD static F f(F a, F b) { return OP == OP_SUM ? a + b : a * b; }
    OSGPU_EHD static bool bad(F r) { return r != r; }
};
template <> struct Fast<float, OP_SUM> : FastReal<float, OP_SUM> {};
template <> struct Fast<float, OP_PROD> : FastReal<float, OP_PROD> {};
template <> struct Fast<double, OP_SUM> : FastReal<double, OP_SUM> {};
template <> struct Fast<double, OP_PROD> : FastReal<double, OP_PROD> {};
template <typename H, int OP> struct Fast16 {
    static constexpr bool kChecked = true;
    OSGPU_EHD static H f(H a, H b) { return arith16<H, OP>(a, b); }
    OSGPU_EHD static bool bad(H r) { return isnan_(r); }
};
template <> struct Fast<half_t, OP_SUM> : Fast16<half_t, OP_SUM> {};
template <> struct Fast<half_t, OP_PROD> : Fast16<half_t, OP_PROD> {};
template <> struct Fast<bf16_t, OP_SUM> : Fast16<bf16_t, OP_SUM> {};
template <> struct Fast<bf16_t, OP_PROD> : Fast16<bf16_t, OP_PROD> {};
template <> struct Fast<cdouble, OP_SUM> {
    static constexpr bool kChecked = true;
    OSGPU_EHD static cdouble f(cdouble a, cdouble b)
    {
        return cdouble{a.re + b.re, a.im + b.im};
    }
    OSGPU_EHD static bool bad(cdouble r) { return r.re != r.re || r.im != r.im; }
};
template <> struct Fast<cfloat, OP_SUM> {
    static constexpr bool kChecked = true;
    OSGPU_EHD static cfloat f(cfloat a, cfloat b)
    {
        return cfloat{a.re + b.re, b.im + a.im};  // the compiled order, as Elem
    }
    OSGPU_EHD static bool bad(cfloat r) { return r.re != r.re || r.im != r.im; }
};
template <typename C, typename F> struct FastCplxProd {
    static constexpr bool kChecked = true;
    OSGPU_EHD static C f(C p, C q)
    {
        return C{p.re * q.re - p.im * q.im, p.re * q.im + p.im * q.re};  // cmul's inline form
    }
    OSGPU_EHD static bool bad(C r) { return r.re != r.re || r.im != r.im; }
};
template <> struct Fast<cdouble, OP_PROD> : FastCplxProd<cdouble, double> {};
template <> struct Fast<cfloat, OP_PROD> : FastCplxProd<cfloat, float> {};

}  // namespace osgpu
