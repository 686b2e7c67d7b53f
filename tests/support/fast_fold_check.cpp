// fast_fold_check.cpp -- TEST INFRASTRUCTURE: the premise of the branch-free
// folds (csrc/elem_ops.hpp Fast<T, OP>) on the host, with its own main, built
// plain and with ASan + UBSan by host_check_build.py.
// usage: fast_fold_check premise      every floating (type, op) with kChecked,
//                                     all triples of an alphabet
//        fast_fold_check route FILE   the kernels' route (the fast fold of a
//                                     16-byte vector, the exact one when a
//                                     final value is flagged) over records
//                                     written by tests/test_matrix_ref.py
// prints "ok ..." and exits 0, or the first failed check and 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../test-resilient-osss-ucx_amd/csrc/elem_ops.hpp"

using namespace osgpu;

template <typename T>
static bool same(T a, T b)
{
    return memcmp(&a, &b, sizeof(T)) == 0;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t next()
{
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ------------------------------------------------------------- alphabets
// specials: signed zeros, one, extremes, subnormals, infinities, quiet and
// signalling NaNs with payloads of either sign; then `more` seeded ordinary
// values (finite, exponents within 2^+-8 of 1, either sign)
static void alphabet(std::vector<float> &v, int more)
{
    const uint32_t sp[] = {0x00000000u, 0x80000000u, 0x3F800000u, 0xBF800000u, 0x7F7FFFFFu,
                           0xFF7FFFFFu, 0x00800000u, 0x00000001u, 0x80000003u, 0x7F800000u,
                           0xFF800000u, 0x7FC00000u, 0xFFC00000u, 0x7FC00123u, 0x7F800001u,
                           0xFFA00005u, 0x5F000000u, 0x1F000000u};
    for (uint32_t b : sp) v.push_back(flt(b));
    for (int i = 0; i < more; i++) {
        const uint64_t r = next();
        v.push_back(flt((uint32_t) ((r >> 63) << 31) | (uint32_t) (119 + (r >> 40) % 17) << 23
                        | (uint32_t) (r & 0x7FFFFFu)));
    }
}
static void alphabet(std::vector<double> &v, int more)
{
    const uint64_t sp[] = {0x0ull, 0x8000000000000000ull, 0x3FF0000000000000ull,
                           0xBFF0000000000000ull, 0x7FEFFFFFFFFFFFFFull, 0xFFEFFFFFFFFFFFFFull,
                           0x0010000000000000ull, 0x0000000000000001ull, 0x8000000000000003ull,
                           0x7FF0000000000000ull, 0xFFF0000000000000ull, 0x7FF8000000000000ull,
                           0xFFF8000000000000ull, 0x7FF8000000000123ull, 0x7FF0000000000001ull,
                           0xFFF4000000000005ull, 0x5FE0000000000000ull, 0x2000000000000000ull};
    for (uint64_t b : sp) v.push_back(dbl(b));
    for (int i = 0; i < more; i++) {
        const uint64_t r = next();
        v.push_back(dbl(((r >> 63) << 63) | (uint64_t) (1015 + (r >> 53) % 17) << 52
                        | (r & 0xFFFFFFFFFFFFFull)));
    }
}
static void alphabet(std::vector<half_t> &v, int more)
{
    const uint16_t sp[] = {0x0000, 0x8000, 0x3C00, 0xBC00, 0x7BFF, 0xFBFF, 0x0400, 0x0001, 0x8003,
                           0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7E15, 0x7C01, 0xFD05, 0x5C00, 0x1C00};
    for (uint16_t b : sp) v.push_back(half_t{b});
    for (int i = 0; i < more; i++) {
        const uint64_t r = next();
        v.push_back(half_t{(uint16_t) (((r >> 63) << 15) | (11 + (r >> 40) % 9) << 10 | (r & 0x3FF))});
    }
}
static void alphabet(std::vector<bf16_t> &v, int more)
{
    const uint16_t sp[] = {0x0000, 0x8000, 0x3F80, 0xBF80, 0x7F7F, 0xFF7F, 0x0080, 0x0001, 0x8003,
                           0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7FD5, 0x7F81, 0xFFA5, 0x5F00, 0x1F00};
    for (uint16_t b : sp) v.push_back(bf16_t{b});
    for (int i = 0; i < more; i++) {
        const uint64_t r = next();
        v.push_back(bf16_t{(uint16_t) (((r >> 63) << 15) | (119 + (r >> 40) % 17) << 7 | (r & 0x7F))});
    }
}
// complex: every pair of a short component alphabet, then ordinary pairs
template <typename C, typename F>
static void alphabet_c(std::vector<C> &v, int more)
{
    std::vector<F> comp, ord;
    alphabet(comp, 0);
    const size_t keep[] = {0, 1, 2, 3, 4, 9, 10, 13, 14, 15};   // zeros, ones, max, infs, NaNs
    for (size_t i : keep)
        for (size_t j : keep) v.push_back(C{comp[i], comp[j]});
    alphabet(ord, 2 * more);
    for (int i = 0; i < more; i++) v.push_back(C{ord[18 + 2 * i], ord[18 + 2 * i + 1]});
}
static void alphabet(std::vector<cfloat> &v, int more) { alphabet_c<cfloat, float>(v, more / 2); }
static void alphabet(std::vector<cdouble> &v, int more) { alphabet_c<cdouble, double>(v, more / 2); }

// ----------------------------------------------------------------- premise
//  1. where the Fast fold of three operands has no NaN part it is the Elem
//     fold, bit for bit;
//  2. a NaN part of a Fast intermediate survives the next step.
template <typename T, int OP>
static int premise(const char *name, unsigned long long *total)
{
    using F = Fast<T, OP>;
    using E = Elem<T, OP>;
    static_assert(F::kChecked, "a pair with a branch-free fold");
    std::vector<T> al;
    g_rng = 0xFA57F01Dull + OP;
    alphabet(al, 200);
    unsigned long long fast = 0, flagged = 0;
    for (const T &a : al)
        for (const T &b : al) {
            const T fab = F::f(a, b), eab = E::f(a, b);
            const bool bad_ab = F::bad(fab);
            if (!bad_ab && !same(fab, eab)) {
                printf("%s: one step differs without a NaN part\n", name);
                return 1;
            }
            for (const T &c : al) {
                const T f3 = F::f(fab, c);
                if (F::bad(f3)) {
                    flagged++;
                    continue;
                }
                if (bad_ab) {
                    printf("%s: a NaN part of a fast intermediate was lost by the next step\n", name);
                    return 1;
                }
                fast++;
                if (!same(f3, E::f(eab, c))) {
                    printf("%s: the fast fold of three has no NaN part and is not the exact fold\n",
                           name);
                    return 1;
                }
            }
        }
    if (fast == 0 || flagged == 0) {
        printf("%s: the alphabet reaches one route only\n", name);
        return 1;
    }
    *total += fast + flagged;
    return 0;
}

static int premise_all()
{
    unsigned long long total = 0;
    int rc = 0;
#define PAIR(T, OP) rc = rc ? rc : premise<T, OP>(#T " " #OP, &total)
    PAIR(float, OP_SUM);
    PAIR(float, OP_PROD);
    PAIR(double, OP_SUM);
    PAIR(double, OP_PROD);
    PAIR(half_t, OP_SUM);
    PAIR(half_t, OP_PROD);
    PAIR(bf16_t, OP_SUM);
    PAIR(bf16_t, OP_PROD);
    PAIR(cfloat, OP_SUM);
    PAIR(cfloat, OP_PROD);
    PAIR(cdouble, OP_SUM);
    PAIR(cdouble, OP_PROD);
#undef PAIR
    if (rc == 0) printf("ok %llu triples\n", total);
    return rc;
}

// ------------------------------------------------------------------- route
// One record: int32 {type code, op, P, n}, P arrays of n elements, the
// expected ascending fold of n elements.  The route of team_scan_lds_kernel
// and team_uniform_lds_kernel per 16-byte vector: the Fast fold of every
// element, and the Elem fold of the whole vector when a final value is bad.
template <typename T, int OP>
static int route(const unsigned char *p, int P, long n, long *fast, long *exact)
{
    using F = Fast<T, OP>;
    constexpr long W = 16 / sizeof(T);
    std::vector<T> in((size_t) P * n), want((size_t) n);  // allocated to the element
    memcpy(in.data(), p, in.size() * sizeof(T));
    memcpy(want.data(), p + in.size() * sizeof(T), want.size() * sizeof(T));
    for (long v0 = 0; v0 < n; v0 += W) {
        const long w = n - v0 < W ? n - v0 : W;
        T out[W];
        bool bad = false;
        for (long e = 0; e < w; e++) {
            T acc = in[v0 + e];
            for (int k = 1; k < P; k++) acc = F::f(acc, in[(size_t) k * n + v0 + e]);
            out[e] = acc;
            bad = bad || F::bad(acc);
        }
        if (F::kChecked && bad) {
            for (long e = 0; e < w; e++) {
                T acc = in[v0 + e];
                for (int k = 1; k < P; k++) acc = Elem<T, OP>::f(acc, in[(size_t) k * n + v0 + e]);
                out[e] = acc;
            }
        }
        (bad ? *exact : *fast) += 1;
        for (long e = 0; e < w; e++)
            if (!same(out[e], want[v0 + e])) {
                printf("element %ld differs (%s route)\n", v0 + e, bad ? "exact" : "fast");
                return 1;
            }
    }
    return 0;
}

static int route_file(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        printf("cannot open %s\n", path);
        return 1;
    }
    std::vector<unsigned char> buf;
    unsigned char tmp[1 << 16];
    size_t got;
    while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    fclose(f);
    const size_t sizes[] = {2, 4, 8, 8, 4, 8, 16, 8, 16, 2, 2};
    size_t at = 0;
    long records = 0, fast = 0, exact = 0;
    while (at < buf.size()) {
        int32_t h[4];
        if (buf.size() - at < sizeof(h)) {
            printf("record %ld: a short header\n", records);
            return 1;
        }
        memcpy(h, buf.data() + at, sizeof(h));
        at += sizeof(h);
        const int t = h[0], op = h[1], P = h[2];
        const long n = h[3];
        if (t < 0 || t > 10 || P < 1 || P > 64 || n < 0
            || (buf.size() - at) / sizes[t] < (size_t) (P + 1) * (size_t) n) {
            printf("record %ld: a bad header or a short body\n", records);
            return 1;
        }
        const unsigned char *p = buf.data() + at;
        int rc = -1;
#define ROUTE(CODE, T)                                                                    \
    if (t == CODE && op == OP_SUM) rc = route<T, OP_SUM>(p, P, n, &fast, &exact);         \
    if (t == CODE && op == OP_PROD) rc = route<T, OP_PROD>(p, P, n, &fast, &exact)
        ROUTE(4, float);
        ROUTE(5, double);
        ROUTE(7, cfloat);
        ROUTE(8, cdouble);
        ROUTE(9, half_t);
        ROUTE(10, bf16_t);
#undef ROUTE
        if (rc != 0) {
            printf("record %ld (type %d op %d P %d n %ld)%s\n", records, t, op, P, n,
                   rc < 0 ? ": no such pair" : "");
            return 1;
        }
        at += (size_t) (P + 1) * (size_t) n * sizes[t];
        records++;
    }
    printf("ok %ld records fast=%ld exact=%ld\n", records, fast, exact);
    return 0;
}

int main(int argc, char **argv)
{
    const char *c = argc > 1 ? argv[1] : "";
    if (!strcmp(c, "premise")) return premise_all();
    if (!strcmp(c, "route") && argc > 2) return route_file(argv[2]);
    printf("unknown case '%s'\n", c);
    return 1;
}
