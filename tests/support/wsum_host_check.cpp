// wsum_host_check.cpp -- TEST INFRASTRUCTURE: the HIP-free arithmetic of
// osgpu_reduce_wsum (csrc/wsum_host.hpp) and its steps (csrc/elem_ops.hpp
// WsumStep compiled for the host) with their own main, built plain and with
// ASan + UBSan by host_check_build.py.
// usage: wsum_host_check arith        the pair table, byte counts, the carry
//                                     scratch rule, GETMEM's chunk, source chunks
//        wsum_host_check fold FILE    the cases Python wrote to FILE, folded by
//                                     wsum_widen_n / wsum_add_n / wsum_narrow_n
//                                     in wsum_for_source_chunks' order with a
//                                     float carry, compared with the expected
//                                     arrays
// prints "ok" and exits 0, or the first failed check and 1.
// FILE: records until the end of the file -- int32 type, P, n; P arrays of n
// uint16; the expected uint32 accumulator array; the expected uint16 array.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../test-resilient-osss-ucx_amd/csrc/elem_ops.hpp"
#include "../../test-resilient-osss-ucx_amd/csrc/wsum_host.hpp"

using namespace osgpu;
using namespace osgpu::rt;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);                \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static int arith()
{
    // the 4 pairs
    int on = 0;
    for (int t = -2; t < 14; t++)
        for (int o = -2; o < 14; o++) on += wsum_pair(t, o) ? 1 : 0;
    CHECK(on == 4);
    CHECK(wsum_pair(SCAN_T_HALF, SCAN_T_HALF) && wsum_pair(SCAN_T_HALF, SCAN_T_FLOAT));
    CHECK(wsum_pair(SCAN_T_BFLOAT16, SCAN_T_BFLOAT16) && wsum_pair(SCAN_T_BFLOAT16, SCAN_T_FLOAT));
    CHECK(!wsum_pair(SCAN_T_HALF, SCAN_T_BFLOAT16) && !wsum_pair(SCAN_T_FLOAT, SCAN_T_FLOAT));
    CHECK(!wsum_pair(SCAN_T_HALF, SCAN_T_DOUBLE) && !wsum_pair(SCAN_T_SHORT, SCAN_T_FLOAT));
    CHECK(wsum_out_size(SCAN_T_HALF, SCAN_T_HALF) == 2 && wsum_out_size(SCAN_T_HALF, SCAN_T_FLOAT) == 4);
    CHECK(wsum_out_size(SCAN_T_FLOAT, SCAN_T_FLOAT) == 0);
    // byte counts, INT_MAX elements and 9 members included
    WsumBytes b;
    CHECK(wsum_bytes(2, 10, 3, &b) && b.sbytes == 20 && b.tbytes == 20 && b.abytes == 40 &&
          b.pulled_bound == 40);
    CHECK(wsum_bytes(4, 10, 1, &b) && b.tbytes == 40 && b.pulled_bound == 0);
    CHECK(wsum_bytes(4, INT_MAX, 9, &b));
    CHECK(b.sbytes == (size_t) INT_MAX * 2 && b.tbytes == (size_t) INT_MAX * 4 &&
          b.pulled_bound == (size_t) 8 * INT_MAX * 2);
    CHECK(wsum_bytes(2, 0, 1, &b) && b.sbytes == 0 && b.tbytes == 0 && b.abytes == 0);
    CHECK(!wsum_bytes(8, 1, 2, &b) && !wsum_bytes(2, -1, 2, &b) && !wsum_bytes(2, 1, 0, &b));
    // the carry: scratch only for a 16-bit target of more than 8 members
    CHECK(!wsum_needs_carry_scratch(8, 2) && wsum_needs_carry_scratch(9, 2));
    CHECK(!wsum_needs_carry_scratch(9, 4) && !wsum_needs_carry_scratch(1, 2));
    // GETMEM's chunk: whole groups of 8, at least one, at most the array rounded up
    CHECK(wsum_chunk_elems(2048, 100000) == 1024 && wsum_chunk_elems(2047, 100000) == 1016);
    CHECK(wsum_chunk_elems(1, 100000) == 8 && wsum_chunk_elems(1 << 20, 5) == 8);
    CHECK(wsum_chunk_elems(1 << 20, 1001) == 1008);
    for (size_t n : {(size_t) 1, (size_t) 7, (size_t) 8, (size_t) 1001}) {
        size_t covered = 0, calls = 0;
        scan_for_chunks(n, wsum_chunk_elems(16, n), [&](size_t off, size_t len) {
            if (off == covered) covered += len;
            calls++;
        });
        CHECK(covered == n && calls == (n + 7) / 8);
    }
    // the source chunks: every member once, ascending, 8 a launch, the carry
    // from the second launch on, the last launch marked
    for (int P = 1; P <= 40; P++) {
        int next = 0, calls = 0, lasts = 0;
        bool good = true;
        wsum_for_source_chunks(P, [&](int first, int count, bool carry_in, bool last) {
            good = good && first == next && count >= 1 && count <= kWsumMaxSources &&
                   carry_in == (calls > 0) && last == (first + count == P) && lasts == 0;
            next = first + count;
            lasts += last ? 1 : 0;
            calls++;
        });
        CHECK(good && next == P && lasts == 1 && calls == (P + 7) / 8);
    }
    return 0;
}

// one record folded in wsum_for_source_chunks' order into exactly-sized arrays
template <typename T>
static int fold_case(int P, size_t n, const std::vector<std::vector<uint16_t>> &srcs,
                     const uint32_t *want_acc, const uint16_t *want_out)
{
    using S = WsumStep<T>;
    float *acc = (float *) malloc(n * sizeof(float) + (n == 0));
    T *out = (T *) malloc(n * sizeof(T) + (n == 0));
    CHECK(acc && out);
    wsum_for_source_chunks(P, [&](int first, int count, bool carry_in, bool) {
        for (int j = first; j < first + count; j++) {
            const T *b = (const T *) srcs[j].data();
            if (j == first && !carry_in) wsum_widen_n<S, T>(acc, b, n);
            else wsum_add_n<S, T>(acc, b, n);
        }
    });
    wsum_narrow_n<S, T>(out, acc, n);
    int rc = 0;
    for (size_t k = 0; !rc && k < n; k++) {
        uint32_t a;
        memcpy(&a, &acc[k], 4);
        if (a != want_acc[k])
            rc = 1, printf("accumulator %zu: %08x, want %08x\n", k, a, want_acc[k]);
        else if (out[k].u != want_out[k])
            rc = 1, printf("element %zu: %04x, want %04x\n", k, out[k].u, want_out[k]);
    }
    free(acc);
    free(out);
    return rc;
}

static int fold(const char *path)
{
    FILE *f = fopen(path, "rb");
    CHECK(f);
    int records = 0;
    for (;;) {
        int32_t h[3];
        const size_t got = fread(h, 4, 3, f);
        if (got == 0) break;
        CHECK(got == 3);
        const int type = h[0], P = h[1];
        const size_t n = (size_t) h[2];
        CHECK(wsum_pair(type, type) && P >= 1 && P <= 64 && h[2] >= 0);
        std::vector<std::vector<uint16_t>> srcs(P);
        for (int j = 0; j < P; j++) {
            srcs[j].resize(n);
            CHECK(fread(srcs[j].data(), 2, n, f) == n);
        }
        std::vector<uint32_t> wa(n);
        std::vector<uint16_t> wo(n);
        CHECK(fread(wa.data(), 4, n, f) == n && fread(wo.data(), 2, n, f) == n);
        const int rc = type == SCAN_T_HALF ? fold_case<half_t>(P, n, srcs, wa.data(), wo.data())
                                           : fold_case<bf16_t>(P, n, srcs, wa.data(), wo.data());
        if (rc) {
            printf("record %d: type %d P %d n %zu\n", records, type, P, n);
            fclose(f);
            return 1;
        }
        records++;
    }
    fclose(f);
    CHECK(records > 0);
    return 0;
}

int main(int argc, char **argv)
{
    int rc = 1;
    if (argc == 2 && !strcmp(argv[1], "arith")) rc = arith();
    else if (argc == 3 && !strcmp(argv[1], "fold")) rc = fold(argv[2]);
    else return 1;
    if (rc == 0) printf("ok\n");
    return rc;
}
