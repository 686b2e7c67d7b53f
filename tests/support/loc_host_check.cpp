// loc_host_check.cpp -- TEST INFRASTRUCTURE: the HIP-free arithmetic of
// osgpu_reduce_loc (csrc/loc_host.hpp) and its step (csrc/elem_ops.hpp LocStep
// compiled for the host) with their own main, built plain and with ASan +
// UBSan by host_check_build.py.
// usage: loc_host_check arith        the pair table, byte counts, overlap rule,
//                                    vector split, GETMEM chunk, input chunks
//        loc_host_check fold FILE    the cases Python wrote to FILE, folded by
//                                    loc_fold_n<LocStep> in loc_for_input_chunks'
//                                    order, compared with the expected arrays
// prints "ok" and exits 0, or the first failed check and 1.
// FILE: records until the end of the file -- int32 type, op, P, n, has_loc;
// P value arrays of n elements; has_loc ? P int32 arrays of n : P int32 member
// numbers; the expected value array; the expected int32 index array.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../test-resilient-osss-ucx_amd/csrc/elem_ops.hpp"
#include "../../test-resilient-osss-ucx_amd/csrc/loc_host.hpp"

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
    // the 16 pairs
    int on = 0;
    for (int t = -2; t < 14; t++)
        for (int o = -2; o < 10; o++) on += loc_pair(t, o) ? 1 : 0;
    CHECK(on == 16);
    CHECK(loc_pair(SCAN_T_HALF, SCAN_OP_MIN) && loc_pair(SCAN_T_LONGLONG, SCAN_OP_MAX));
    CHECK(!loc_pair(SCAN_T_LONGDOUBLE, SCAN_OP_MAX) && !loc_pair(SCAN_T_COMPLEXF, SCAN_OP_MAX));
    CHECK(!loc_pair(SCAN_T_INT, SCAN_OP_SUM));
    // groups
    CHECK(loc_group(2) == 8 && loc_group(4) == 4 && loc_group(8) == 4);
    CHECK(loc_group(16) == 0 && loc_group(0) == 0 && loc_group(3) == 0);
    CHECK(loc_member_pe(1, 1, 2) == 5 && loc_member_pe(0, 0, 7) == 7 && loc_member_pe(4, 2, 0) == 4);
    // byte counts, INT_MAX elements of 8 bytes and 9 members included
    LocBytes b;
    CHECK(loc_bytes(4, 10, 3, true, &b) && b.vbytes == 40 && b.lbytes == 40 && b.pulled_bound == 160);
    CHECK(loc_bytes(2, 10, 3, false, &b) && b.vbytes == 20 && b.lbytes == 40 && b.pulled_bound == 40);
    CHECK(loc_bytes(8, INT_MAX, 9, true, &b));
    CHECK(b.vbytes == (size_t) INT_MAX * 8 && b.pulled_bound == (size_t) 8 * INT_MAX * 12);
    CHECK(loc_bytes(8, 0, 1, true, &b) && b.vbytes == 0 && b.pulled_bound == 0);
    CHECK(!loc_bytes(16, 1, 2, true, &b) && !loc_bytes(4, -1, 2, true, &b) && !loc_bytes(4, 1, 0, true, &b));
    // the overlap rule
    alignas(16) static char arena[4096];
    char *t = arena, *s = arena + 1024, *lt = arena + 2048, *ls = arena + 3072;
    CHECK(loc_cross_overlap(t, s, 1024, lt, ls, 1024) == nullptr);
    CHECK(loc_cross_overlap(t, t, 1024, lt, lt, 1024) == nullptr);   // in place, both streams
    CHECK(loc_cross_overlap(t, s, 1024, lt, nullptr, 1024) == nullptr);
    CHECK(loc_cross_overlap(t, t + 512, 1024, lt, lt + 4, 1020) == nullptr);  // partial overlaps
    CHECK(loc_cross_overlap(t, s, 1024, t + 1023, ls, 4) != nullptr);  // the two targets
    CHECK(loc_cross_overlap(t, s, 1024, lt, s + 1020, 8) != nullptr);  // source / loc_source
    CHECK(loc_cross_overlap(t, s, 1024, s, ls, 4) != nullptr);         // source / loc_target
    CHECK(loc_cross_overlap(t, s, 1024, lt, t, 4) != nullptr);         // target / loc_source
    CHECK(loc_cross_overlap(t, s, 0, t, s, 0) == nullptr);
    // vector split: every element size, every head, mismatches
    for (size_t elem : {(size_t) 2, (size_t) 4, (size_t) 8}) {
        const size_t g = loc_group(elem);
        for (size_t h = 0; h < g; h++)
            for (size_t n : {(size_t) 0, (size_t) 1, g - 1, g, g + 1, 5 * g + 3}) {
                // pointers h elements before a 16-byte boundary, both streams
                const void *v[2] = {arena + 256 - h * elem, arena + 512 - h * elem};
                const void *l[2] = {arena + 1024 - h * 4, arena + 2048 - h * 4};
                const LocSplit sp = loc_split(elem, n, v, 2, l, 2);
                CHECK(sp.vec);
                const size_t head = h > n ? n : h;
                CHECK(sp.head == head && sp.ngroups == (n - head) / g);
                CHECK(sp.tail_start == head + sp.ngroups * g && sp.tail_start <= n);
                CHECK((size_t) sp.nedge == head + n - sp.tail_start && (size_t) sp.nedge < 2 * g);
                if (sp.ngroups) {
                    CHECK((((uintptr_t) v[1] + sp.head * elem) & 15) == 0);
                    CHECK((((uintptr_t) l[1] + sp.head * 4) & 15) == 0);
                }
                // no index pointers at all (the form without index sources' inputs)
                CHECK(loc_split(elem, n, v, 2, l, 0).vec);
            }
        // one value pointer an element off: no common head
        const void *v[2] = {arena + 256, arena + 512 + elem};
        const void *l[1] = {arena + 1024};
        CHECK(!loc_split(elem, 100, v, 2, l, 1).vec);
        // index pointers at +4 bytes against aligned values: no common head either
        const void *v2[1] = {arena + 256};
        const void *l2[1] = {arena + 1024 + 4};
        CHECK(!loc_split(elem, 100, v2, 1, l2, 1).vec);
    }
    // an 8-byte value stream at phase 8 with the index stream at phase 12: head 1
    {
        const void *v[1] = {arena + 8};
        const void *l[1] = {arena + 1024 + 12};
        const LocSplit sp = loc_split(8, 100, v, 1, l, 1);
        CHECK(sp.vec && sp.head == 1 && sp.ngroups == 24 && sp.tail_start == 97 && sp.nedge == 4);
    }
    // GETMEM's chunk: whole groups of 8, at least one, at most the array rounded up
    CHECK(loc_chunk_elems(2048, 4, 100000) == 256 && loc_chunk_elems(2048, 8, 100000) == 168);
    CHECK(loc_chunk_elems(2048, 2, 100000) == 336 && loc_chunk_elems(1, 8, 100000) == 8);
    CHECK(loc_chunk_elems(1 << 20, 4, 5) == 8 && loc_chunk_elems(1 << 20, 4, 1001) == 1008);
    for (size_t n : {(size_t) 1, (size_t) 7, (size_t) 8, (size_t) 1001}) {
        size_t covered = 0, calls = 0;
        scan_for_chunks(n, loc_chunk_elems(64, 4, n), [&](size_t off, size_t len) {
            if (off == covered) covered += len;
            calls++;
        });
        CHECK(covered == n && calls == (n + 7) / 8);
    }
    // the input chunks: every member once, ascending, feedback from the second on
    for (int P = 1; P <= 20; P++) {
        int next = 0, calls = 0;
        bool good = true;
        loc_for_input_chunks(P, [&](int first, int count, bool feedback) {
            good = good && first == next && count >= 1 && feedback == (calls > 0) &&
                   count + (feedback ? 1 : 0) <= kLocMaxInputs;
            next = first + count;
            calls++;
        });
        CHECK(good && next == P);
        CHECK(calls == (P <= 8 ? 1 : 1 + (P - 8 + 6) / 7));
    }
    return 0;
}

// one record folded in loc_for_input_chunks' order into exactly-sized arrays
template <typename T, int OP>
static int fold_case(int P, size_t n, bool has_loc, const std::vector<std::vector<unsigned char>> &vals,
                     const std::vector<std::vector<int32_t>> &locs, const std::vector<int32_t> &member,
                     const unsigned char *want_v, const int32_t *want_i)
{
    T *v = (T *) malloc(n * sizeof(T) + (n == 0));
    int32_t *i = (int32_t *) malloc(n * sizeof(int32_t) + (n == 0));
    CHECK(v && i);
    int rc = 0;
    loc_for_input_chunks(P, [&](int first, int count, bool feedback) {
        for (int j = first; j < first + count; j++) {
            const T *b = (const T *) vals[j].data();
            const int32_t *ib = has_loc ? locs[j].data() : nullptr;
            if (j == 0 && !feedback) {  // the fold starts at member 0's pair
                if (n) memcpy(v, b, n * sizeof(T));
                for (size_t k = 0; k < n; k++) i[k] = ib ? ib[k] : member[0];
            } else {
                loc_fold_n<LocStep<T, OP>, T>(v, i, b, ib, member[j], n);
            }
        }
    });
    if (n && memcmp(v, want_v, n * sizeof(T))) rc = 1, printf("values differ\n");
    for (size_t k = 0; !rc && k < n; k++)
        if (i[k] != want_i[k]) rc = 1, printf("index %zu: %d, want %d\n", k, i[k], want_i[k]);
    free(v);
    free(i);
    return rc;
}

template <typename T>
static int fold_op(int op, int P, size_t n, bool has_loc,
                   const std::vector<std::vector<unsigned char>> &vals,
                   const std::vector<std::vector<int32_t>> &locs, const std::vector<int32_t> &member,
                   const unsigned char *wv, const int32_t *wi)
{
    if (op == OP_MAX) return fold_case<T, OP_MAX>(P, n, has_loc, vals, locs, member, wv, wi);
    if (op == OP_MIN) return fold_case<T, OP_MIN>(P, n, has_loc, vals, locs, member, wv, wi);
    return 1;
}

static int fold(const char *path)
{
    FILE *f = fopen(path, "rb");
    CHECK(f);
    int records = 0;
    for (;;) {
        int32_t h[5];
        const size_t got = fread(h, 4, 5, f);
        if (got == 0) break;
        CHECK(got == 5);
        const int type = h[0], op = h[1], P = h[2];
        const size_t n = (size_t) h[3];
        const bool has_loc = h[4] != 0;
        CHECK(loc_pair(type, op) && P >= 1 && P <= 64 && h[3] >= 0);
        unsigned char id[16];
        const size_t s = scan_identity(type, op, id);
        CHECK(s == 2 || s == 4 || s == 8);
        std::vector<std::vector<unsigned char>> vals(P);
        std::vector<std::vector<int32_t>> locs(has_loc ? P : 0);
        std::vector<int32_t> member(P, 0);
        for (int j = 0; j < P; j++) {
            vals[j].resize(n * s);
            CHECK(fread(vals[j].data(), s, n, f) == n);
        }
        if (has_loc) {
            for (int j = 0; j < P; j++) {
                locs[j].resize(n);
                CHECK(fread(locs[j].data(), 4, n, f) == n);
            }
        } else {
            CHECK(fread(member.data(), 4, P, f) == (size_t) P);
        }
        std::vector<unsigned char> wv(n * s);
        std::vector<int32_t> wi(n);
        CHECK(fread(wv.data(), s, n, f) == n && fread(wi.data(), 4, n, f) == n);
        int rc = 1;
        switch (type) {
        case SCAN_T_SHORT: rc = fold_op<int16_t>(op, P, n, has_loc, vals, locs, member, wv.data(), wi.data()); break;
        case SCAN_T_INT: rc = fold_op<int32_t>(op, P, n, has_loc, vals, locs, member, wv.data(), wi.data()); break;
        case SCAN_T_LONG:
        case SCAN_T_LONGLONG: rc = fold_op<int64_t>(op, P, n, has_loc, vals, locs, member, wv.data(), wi.data()); break;
        case SCAN_T_FLOAT: rc = fold_op<float>(op, P, n, has_loc, vals, locs, member, wv.data(), wi.data()); break;
        case SCAN_T_DOUBLE: rc = fold_op<double>(op, P, n, has_loc, vals, locs, member, wv.data(), wi.data()); break;
        case SCAN_T_HALF: rc = fold_op<half_t>(op, P, n, has_loc, vals, locs, member, wv.data(), wi.data()); break;
        case SCAN_T_BFLOAT16: rc = fold_op<bf16_t>(op, P, n, has_loc, vals, locs, member, wv.data(), wi.data()); break;
        }
        if (rc) {
            printf("record %d: type %d op %d P %d n %zu has_loc %d\n", records, type, op, P, n,
                   (int) has_loc);
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
