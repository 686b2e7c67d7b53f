// scan_host_check.cpp -- TEST INFRASTRUCTURE: the HIP-free arithmetic of
// osgpu_scan (csrc/scan_host.hpp) with its own main, built plain and with
// ASan + UBSan by host_check_build.py.
// usage: scan_host_check CASE   (prefix | bytes | chunks | identity); prints
// "ok" and exits 0, or the first failed check and 1.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../test-resilient-osss-ucx_amd/csrc/scan_host.hpp"

using namespace osgpu::rt;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);                \
            return 1;                                                        \
        }                                                                    \
    } while (0)

// prefix lengths for P in 1..9 and both modes
static int prefix()
{
    for (int P = 1; P <= 9; P++)
        for (int m = 0; m < P; m++) {
            CHECK(scan_prefix_len(m, 0) == m + 1);
            CHECK(scan_prefix_len(m, 1) == m);
            ScanBytes b;
            for (int ex = 0; ex < 2; ex++) {
                CHECK(scan_bytes(4, 10, P, m, ex, &b));
                CHECK(b.bytes == 40 && b.pulled_bytes == (size_t) m * 40);
                CHECK(b.pulled_bound == (size_t) (P - 1) * 40);
                // what it pulls: its inputs without its own source
                const int own = ex ? 0 : 1;
                CHECK(b.pulled_bytes == (size_t) (scan_prefix_len(m, ex) - own) * b.bytes);
                CHECK(b.pulled_bytes <= b.pulled_bound);
            }
        }
    CHECK(scan_prefix_len(0, 1) == 0);
    CHECK(scan_prefix_len(-1, 0) < 0 && scan_prefix_len(0, 2) < 0 && scan_prefix_len(0, -1) < 0);
    return 0;
}

// the pulled-byte bound at nreduce = INT_MAX and 16-byte elements: no overflow
static int bytes()
{
    ScanBytes b;
    CHECK(scan_bytes(16, INT_MAX, 9, 8, 0, &b));
    CHECK(b.bytes == (size_t) INT_MAX * 16);
    CHECK(b.pulled_bytes == (size_t) 8 * INT_MAX * 16);
    CHECK(b.pulled_bound == (size_t) 8 * INT_MAX * 16);
    CHECK(b.pulled_bound / 8 == b.bytes);  // nothing wrapped
    CHECK(scan_bytes(16, INT_MAX, 64, 0, 1, &b) && b.pulled_bytes == 0);
    CHECK(b.pulled_bound == (size_t) 63 * INT_MAX * 16);
    CHECK(scan_bytes(2, 0, 3, 2, 1, &b) && b.bytes == 0 && b.pulled_bound == 0);
    // not a call
    CHECK(!scan_bytes(0, 1, 2, 0, 0, &b));
    CHECK(!scan_bytes(4, -1, 2, 0, 0, &b));
    CHECK(!scan_bytes(4, 1, 0, 0, 0, &b));
    CHECK(!scan_bytes(4, 1, 2, 2, 0, &b));
    CHECK(!scan_bytes(4, 1, 2, -1, 0, &b));
    CHECK(!scan_bytes(4, 1, 2, 0, 2, &b));
    // a byte count beyond size_t
    CHECK(!scan_bytes((size_t) -1 / 2, 3, 2, 0, 0, &b));
    CHECK(!scan_bytes((size_t) 1 << 40, (long long) 1 << 22, 8, 0, 0, &b));
    return 0;
}

// the chunk walk covers [0, n) exactly once, in order, within the chunk
static int chunks()
{
    const size_t ns[] = {1, 2, 3, 127, 128, 129, 1001, 4099};
    const size_t cbs[] = {0, 1, 16, 2048, 1 << 20};
    const size_t elems[] = {2, 4, 8, 16};
    for (size_t n : ns)
        for (size_t cb : cbs)
            for (size_t e : elems) {
                const size_t chunk = host_chunk_elems(cb, e, n);
                CHECK(chunk >= 1 && chunk % 2 == 0 && chunk <= n + 1);
                std::vector<unsigned char> hit(n, 0);  // allocated to the element
                size_t next = 0, calls = 0;
                bool ok = true;
                scan_for_chunks(n, chunk, [&](size_t off, size_t len) {
                    ok = ok && off == next && len >= 1 && len <= chunk && off + len <= n;
                    if (!ok) return;
                    for (size_t i = off; i < off + len; i++) hit[i]++;
                    next = off + len;
                    calls++;
                });
                CHECK(ok && next == n);
                CHECK(calls == (n + chunk - 1) / chunk);
                for (size_t i = 0; i < n; i++) CHECK(hit[i] == 1);
            }
    size_t calls = 0;
    scan_for_chunks(0, 8, [&](size_t, size_t) { calls++; });
    CHECK(calls == 0);
    scan_for_chunks(3, 0, [&](size_t, size_t len) { calls += len; });  // a zero chunk still ends
    CHECK(calls == 3);
    return 0;
}

static bool is_int(int t) { return t <= SCAN_T_LONGLONG; }
static bool is_complex(int t) { return t == SCAN_T_COMPLEXF || t == SCAN_T_COMPLEXD; }
static bool valid(int t, int op)
{
    if (t < 0 || t > SCAN_T_BFLOAT16 || op < 0 || op > SCAN_OP_MIN) return false;
    if (op == SCAN_OP_SUM || op == SCAN_OP_PROD) return true;
    if (op == SCAN_OP_AND || op == SCAN_OP_OR || op == SCAN_OP_XOR) return is_int(t);
    return !is_complex(t);
}

template <typename X>
static bool holds(const unsigned char *b, X v, size_t at = 0)
{
    return memcmp(b + at, &v, sizeof(v)) == 0;
}

// the identity bytes of all 52 pairs, against the host's own arithmetic
static int identity()
{
    const size_t sizes[] = {2, 4, 8, 8, 4, 8, 16, 8, 16, 2, 2};
    int pairs = 0;
    for (int t = -1; t <= SCAN_T_BFLOAT16 + 1; t++)
        for (int op = -1; op <= SCAN_OP_MIN + 1; op++) {
            unsigned char b[16];
            memset(b, 0xAB, sizeof(b));
            const size_t s = scan_identity(t, op, b);
            if (!valid(t, op)) {
                CHECK(s == 0);
                continue;
            }
            pairs++;
            CHECK(s == sizes[t]);
            for (size_t i = s; i < 16; i++) CHECK(b[i] == 0);
            const float finf = __builtin_inff();
            const double dinf = __builtin_inf();
            switch (t) {
            case SCAN_T_SHORT:
                CHECK(holds<int16_t>(b, op == SCAN_OP_PROD ? 1 : op == SCAN_OP_AND ? -1
                                        : op == SCAN_OP_MAX ? SHRT_MIN : op == SCAN_OP_MIN ? SHRT_MAX : 0));
                break;
            case SCAN_T_INT:
                CHECK(holds<int32_t>(b, op == SCAN_OP_PROD ? 1 : op == SCAN_OP_AND ? -1
                                        : op == SCAN_OP_MAX ? INT_MIN : op == SCAN_OP_MIN ? INT_MAX : 0));
                break;
            case SCAN_T_LONG: case SCAN_T_LONGLONG:
                CHECK(holds<int64_t>(b, op == SCAN_OP_PROD ? 1 : op == SCAN_OP_AND ? -1
                                        : op == SCAN_OP_MAX ? LLONG_MIN : op == SCAN_OP_MIN ? LLONG_MAX : 0));
                break;
            case SCAN_T_FLOAT:
                CHECK(holds<float>(b, op == SCAN_OP_PROD ? 1.0f : op == SCAN_OP_MAX ? -finf
                                      : op == SCAN_OP_MIN ? finf : 0.0f));
                break;
            case SCAN_T_DOUBLE:
                CHECK(holds<double>(b, op == SCAN_OP_PROD ? 1.0 : op == SCAN_OP_MAX ? -dinf
                                       : op == SCAN_OP_MIN ? dinf : 0.0));
                break;
            case SCAN_T_LONGDOUBLE: {
                const long double v = op == SCAN_OP_PROD ? 1.0L : op == SCAN_OP_MAX ? -__builtin_infl()
                                      : op == SCAN_OP_MIN ? __builtin_infl() : 0.0L;
                CHECK(memcmp(b, &v, 10) == 0);  // the value bytes; the padding is checked above
                for (size_t i = 10; i < 16; i++) CHECK(b[i] == 0);
                break;
            }
            case SCAN_T_COMPLEXF:
                CHECK(holds<float>(b, op == SCAN_OP_PROD ? 1.0f : 0.0f) && holds<float>(b, 0.0f, 4));
                break;
            case SCAN_T_COMPLEXD:
                CHECK(holds<double>(b, op == SCAN_OP_PROD ? 1.0 : 0.0) && holds<double>(b, 0.0, 8));
                break;
            case SCAN_T_HALF:
                CHECK(holds<uint16_t>(b, op == SCAN_OP_PROD ? 0x3C00 : op == SCAN_OP_MAX ? 0xFC00
                                         : op == SCAN_OP_MIN ? 0x7C00 : 0));
                break;
            case SCAN_T_BFLOAT16:
                CHECK(holds<uint16_t>(b, op == SCAN_OP_PROD ? 0x3F80 : op == SCAN_OP_MAX ? 0xFF80
                                         : op == SCAN_OP_MIN ? 0x7F80 : 0));
                break;
            }
            // the fill: n elements allocated to the byte
            std::vector<unsigned char> buf(3 * s, 0x5A);
            CHECK(scan_fill_identity(t, op, buf.data(), 3));
            for (size_t i = 0; i < 3; i++) CHECK(memcmp(buf.data() + i * s, b, s) == 0);
        }
    CHECK(pairs == 52);
    unsigned char none[1];
    CHECK(!scan_fill_identity(SCAN_T_COMPLEXF, SCAN_OP_MAX, none, 0));
    return 0;
}

int main(int argc, char **argv)
{
    const char *c = argc > 1 ? argv[1] : "";
    int rc = 1;
    if (!strcmp(c, "prefix")) rc = prefix();
    else if (!strcmp(c, "bytes")) rc = bytes();
    else if (!strcmp(c, "chunks")) rc = chunks();
    else if (!strcmp(c, "identity")) rc = identity();
    else {
        printf("unknown case '%s'\n", c);
        return 1;
    }
    if (rc == 0) printf("ok\n");
    return rc;
}
