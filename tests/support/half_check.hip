// half_check.hip -- TEST INFRASTRUCTURE: the half / bfloat16 element ops of
// csrc/elem_ops.hpp compiled for the HOST (the code the host fold runs) and
// checked against an oracle written here, independently of that header:
// double arithmetic, its own round-to-nearest-even narrowing and NaN rule.
//
// For each type and op, Elem::f(a, b) and Fast::f(a, b) over a = all 65536
// patterns x b = a fixed table (binary16: 88 fixed patterns and seeded fill
// up to 640; bfloat16: 1044 fixed patterns, every exponent's first and last
// significand, plus 128 seeded ones).  Also the Fast contract:
// wherever bad(Fast::f(a, b)) is false, Fast::f == Elem::f bit for bit.
// Prints one JSON line of mismatch counts per (type, op); exit status 1 on
// any mismatch.  Stand-alone: its own main, nothing preloaded.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../test-resilient-osss-ucx_amd/csrc/elem_ops.hpp"

namespace {

struct Fmt {
    const char *name;
    int mbits, ebits;
    int bias() const { return (1 << (ebits - 1)) - 1; }
    unsigned mmax() const { return (1u << mbits) - 1; }
    unsigned emax() const { return (1u << ebits) - 1; }
    unsigned quiet() const { return 1u << (mbits - 1); }
    unsigned defnan() const { return 0x8000u | (emax() << mbits) | quiet(); }
};
const Fmt kHalf{"half", 10, 5}, kBf16{"bfloat16", 7, 8};

bool is_nan(const Fmt &f, unsigned x) { return (x & 0x7fffu) > (f.emax() << f.mbits); }

// the value of a non-NaN pattern (exact in double)
double value(const Fmt &f, unsigned x)
{
    const unsigned e = (x >> f.mbits) & f.emax(), m = x & f.mmax();
    double v;
    if (e == f.emax()) v = INFINITY;
    else if (e == 0) v = ldexp((double) m, 1 - f.bias() - f.mbits);
    else v = ldexp((double) (m | (1u << f.mbits)), (int) e - f.bias() - f.mbits);
    return (x & 0x8000u) ? -v : v;
}

// round-to-nearest-even of a non-NaN double into the format.  Products of
// two elements and binary16 sums are exact in double, so this is the single
// rounding; a bfloat16 sum of distant exponents was rounded to 53 bits
// first, which cannot change the result (53 >= 2 * 8 + 2)
unsigned round_to(const Fmt &f, double v)
{
    const unsigned s = signbit(v) ? 0x8000u : 0;
    v = fabs(v);
    if (v == 0) return s;
    if (isinf(v)) return s | (f.emax() << f.mbits);
    int e;
    (void) frexp(v, &e);  // v = fr * 2^e, fr in [0.5, 1)
    int ex = e - 1;       // v in [2^ex, 2^(ex+1))
    const int emin = 1 - f.bias();
    if (ex < emin) ex = emin;  // subnormal spacing
    // units of the last place at this exponent: 2^(ex - mbits)
    const double q = ldexp(v, f.mbits - ex);  // exact scaling
    double fl = floor(q);
    const double rem = q - fl;
    if (rem > 0.5 || (rem == 0.5 && fmod(fl, 2.0) == 1.0)) fl += 1;
    unsigned long long n = (unsigned long long) fl;  // < 2^(mbits + 2)
    // n in [0, 2^(mbits+1)]; n == 2^(mbits+1) carries into the next exponent
    unsigned be = (unsigned) (ex + f.bias());
    if (ex == emin && n < (1ull << f.mbits)) be = 0;  // stays subnormal
    else if (n == (2ull << f.mbits)) {
        n >>= 1;
        be += 1;
    }
    if (be >= f.emax()) return s | (f.emax() << f.mbits);  // overflow to inf
    return s | (be << f.mbits) | (unsigned) (n & f.mmax());
}

unsigned oracle(const Fmt &f, int op, unsigned a, unsigned b)
{
    const bool na = is_nan(f, a), nb = is_nan(f, b);
    if (op == osgpu::OP_MAX || op == osgpu::OP_MIN) {
        if (na || nb) return b;  // every comparison with a NaN is false
        const double x = value(f, a), y = value(f, b);
        return (op == osgpu::OP_MAX ? x > y : x < y) ? a : b;
    }
    if (na) return a | f.quiet();
    if (nb) return b | f.quiet();
    const double x = value(f, a), y = value(f, b);
    if (op == osgpu::OP_SUM) {
        if (isinf(x) && isinf(y) && x != y) return f.defnan();
        const double r = x + y;
        if (r == 0) {  // exact zero: +0 unless both operands are negative (zeros)
            const bool neg = (x == 0 && y == 0) ? ((a & b & 0x8000u) != 0) : false;
            return neg ? 0x8000u : 0u;
        }
        return round_to(f, r);
    }
    if ((isinf(x) && y == 0) || (x == 0 && isinf(y))) return f.defnan();
    const unsigned s = (a ^ b) & 0x8000u;
    const double r = fabs(x) * fabs(y);
    return s | round_to(f, r);
}

std::vector<unsigned> table(const Fmt &f)
{
    std::vector<unsigned> v;
    auto both = [&](unsigned p) {
        v.push_back(p);
        v.push_back(p | 0x8000u);
    };
    const unsigned inf = f.emax() << f.mbits, one = (unsigned) f.bias() << f.mbits;
    both(0);
    both(1);                                  // min subnormal
    both(f.mmax());                           // max subnormal
    both(1u << f.mbits);                      // min normal
    both(one);
    both(((f.emax() - 1) << f.mbits) | f.mmax());  // largest finite
    both(inf);
    both(inf | f.quiet());                    // quiet NaNs, distinct payloads
    both(inf | f.quiet() | 5);
    both(inf | 1);                            // signalling NaNs
    both(inf | 0x15);
    both(inf | (f.mmax() >> 1));
    for (unsigned e = 0; e < f.emax(); e++) {  // every exponent's first and last significand
        both(e << f.mbits);
        both((e << f.mbits) | f.mmax());
    }
    uint64_t x = 0x9E3779B97F4A7C15ull;        // seeded fill (splitmix64)
    const size_t fixed = v.size();
    while (v.size() < 640 || v.size() < fixed + 128) {
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        v.push_back((unsigned) ((z ^ (z >> 31)) & 0xffffu));
    }
    return v;
}

template <typename H, int OP>
int check(const Fmt &f, const char *opname)
{
    const std::vector<unsigned> tb = table(f);
    unsigned long long elem_bad = 0, fast_bad = 0, fast_flagged = 0, n = 0;
    unsigned first[4] = {0, 0, 0, 0};
    for (unsigned a = 0; a < 65536; a++) {
        for (unsigned b : tb) {
            const unsigned want = oracle(f, OP, a, b);
            const H x{(uint16_t) a}, y{(uint16_t) b};
            const unsigned e = osgpu::Elem<H, OP>::f(x, y).u;
            const H fr = osgpu::Fast<H, OP>::f(x, y);
            n++;
            if (e != want) {
                if (!elem_bad++) first[0] = a, first[1] = b, first[2] = e, first[3] = want;
            }
            if (osgpu::Fast<H, OP>::bad(fr)) fast_flagged++;
            else if (fr.u != e) fast_bad++;
        }
    }
    printf("{\"type\": \"%s\", \"op\": \"%s\", \"pairs\": %llu, \"elem_mismatches\": %llu, "
           "\"fast_contract_mismatches\": %llu, \"fast_flagged\": %llu, \"first\": [%u, %u, %u, %u]}\n",
           f.name, opname, n, elem_bad, fast_bad, fast_flagged, first[0], first[1], first[2],
           first[3]);
    return elem_bad || fast_bad;
}

}  // namespace

int main()
{
    int bad = 0;
    bad |= check<osgpu::half_t, osgpu::OP_SUM>(kHalf, "sum");
    bad |= check<osgpu::half_t, osgpu::OP_PROD>(kHalf, "prod");
    bad |= check<osgpu::half_t, osgpu::OP_MAX>(kHalf, "max");
    bad |= check<osgpu::half_t, osgpu::OP_MIN>(kHalf, "min");
    bad |= check<osgpu::bf16_t, osgpu::OP_SUM>(kBf16, "sum");
    bad |= check<osgpu::bf16_t, osgpu::OP_PROD>(kBf16, "prod");
    bad |= check<osgpu::bf16_t, osgpu::OP_MAX>(kBf16, "max");
    bad |= check<osgpu::bf16_t, osgpu::OP_MIN>(kBf16, "min");
    return bad ? 1 : 0;
}
