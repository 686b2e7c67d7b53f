// many_host_check.cpp -- TEST INFRASTRUCTURE: the HIP-free logic of the
// batched reduce-to-all (csrc/many_host.hpp) with its own main, built plain
// and with ASan + UBSan (tests/support/host_check_build.py): the routes, the
// packing plan, the overlap check of the table and the host fold's loop.
// Every array of the host-fold cases is a malloc of EXACTLY its bytes.
// Prints "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../test-resilient-osss-ucx_amd/csrc/many_host.hpp"

using namespace osgpu::rt;
using osgpu::kManySegs;

#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            printf("%s:%d: %s\n", __FILE__, __LINE__, #x);          \
            return 1;                                               \
        }                                                           \
    } while (0)

static int routes()
{
    const uintptr_t a[9] = {0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000};
    const uintptr_t p4[3] = {0x1004, 0x2004, 0x3004};
    const uintptr_t mixed[3] = {0x1004, 0x2008, 0x3004};
    const uintptr_t odd[3] = {0x1000, 0x2002, 0x3000};
    CHECK(many_route(4, false, 3, 0, 0x100, a) == MANY_SKIP);
    CHECK(many_route(4, false, 3, 9, 0x100, a) == MANY_BATCH);
    CHECK(many_route(4, false, 2, 9, 0x100, a) == MANY_BATCH);
    CHECK(many_route(4, false, 8, 9, 0x100, a) == MANY_BATCH);
    CHECK(many_route(4, false, 3, 9, 0x104, p4) == MANY_BATCH);   // one phase, not 0
    CHECK(many_route(4, false, 3, 9, 0x108, p4) == MANY_SHIFTED);  // target off the sources' phase
    CHECK(many_route(4, false, 3, 9, 0x104, mixed) == MANY_SHIFTED);
    CHECK(many_route(4, false, 3, 9, 0x100, odd) == MANY_SHIFTED);  // off the element alignment
    CHECK(many_route(4, false, 3, 9, 0x102, odd) == MANY_SHIFTED);
    CHECK(many_route(16, false, 2, 9, 0x108, a) == MANY_SHIFTED);   // complexd at phase 8
    CHECK(many_route(16, false, 2, 9, 0x100, a) == MANY_BATCH);
    CHECK(many_route(4, false, 9, 9, 0x100, a) == MANY_CHUNKS);
    CHECK(many_route(4, false, 9, 9, 0x104, a) == MANY_SHIFTED);
    CHECK(many_route(4, false, 1, 9, 0x104, a) == MANY_COPY);
    CHECK(many_route(16, true, 3, 9, 0x100, a) == MANY_LONGDOUBLE);
    CHECK(many_route(16, true, 1, 9, 0x108, a) == MANY_LONGDOUBLE);
    CHECK(many_tiles(0, 128) == 1 && many_tiles(1, 128) == 1 && many_tiles(128, 128) == 1 &&
          many_tiles(129, 128) == 2 && many_tiles(5 * 128, 128) == 5);
    return 0;
}

struct Plan {
    int launches = 0, pieces = 0, continuations = 0;
    bool ok = true;
    std::vector<std::vector<int>> seen;  // per entry, per tile: times covered
};

// pack and check the invariants every plan must keep
static int pack(const std::vector<size_t> &tiles, size_t launch_tiles, Plan *out)
{
    Plan p;
    for (size_t t : tiles) p.seen.push_back(std::vector<int>(t, 0));
    int last_entry = -1;
    size_t last_end = 0;
    const bool done = many_pack(
        tiles.data(), (int) tiles.size(), launch_tiles,
        [&](const ManyPiece *pc, int np, size_t blocks) {
            p.launches++;
            p.ok = p.ok && np >= 1 && np <= kManySegs && blocks >= 1 &&
                   blocks <= (launch_tiles ? launch_tiles : 1);
            size_t at = 0;
            for (int i = 0; i < np; i++) {
                const ManyPiece &x = pc[i];
                p.pieces++;
                p.ok = p.ok && x.first == at && x.ntiles >= 1 && x.entry >= 0 &&
                       x.entry < (int) tiles.size() && x.tile0 + x.ntiles <= tiles[x.entry];
                if (!p.ok) return false;
                // table order; a continuation carries on where the entry stopped
                p.ok = p.ok && (x.entry > last_entry ? x.tile0 == 0
                                                     : x.entry == last_entry && x.tile0 == last_end);
                if (x.tile0 > 0) p.continuations++;
                for (size_t t = x.tile0; t < x.tile0 + x.ntiles; t++) p.seen[x.entry][t]++;
                last_entry = x.entry;
                last_end = x.tile0 + x.ntiles;
                at += x.ntiles;
            }
            p.ok = p.ok && at == blocks;
            return p.ok;
        });
    CHECK(done && p.ok);
    for (auto &e : p.seen)
        for (int c : e) CHECK(c == 1);  // every tile of every entry exactly once
    *out = p;
    return 0;
}

static int packing()
{
    Plan p;
    const size_t big = (size_t) 1 << 24;
    // counts 0, 1, 15, 16, 17, 33 of one-tile entries
    const int counts[] = {0, 1, 15, 16, 17, 33};
    const int launches[] = {0, 1, 1, 1, 2, 3};
    for (int c = 0; c < 6; c++) {
        CHECK(pack(std::vector<size_t>(counts[c], 1), big, &p) == 0);
        CHECK(p.launches == launches[c] && p.pieces == counts[c] && p.continuations == 0);
    }
    // zero-length / fall-back entries (0 tiles) take no piece and no room
    CHECK(pack({0, 1, 0, 0, 3, 0}, big, &p) == 0);
    CHECK(p.launches == 1 && p.pieces == 2);
    CHECK(pack(std::vector<size_t>(40, 0), big, &p) == 0 && p.launches == 0);
    {
        std::vector<size_t> t(33, 0);
        for (int i = 0; i < 33; i += 2) t[i] = 1 + i % 3;  // 17 entries among 16 empty ones
        CHECK(pack(t, big, &p) == 0 && p.launches == 2 && p.pieces == 17);
    }
    // entries of 1 and many tiles
    CHECK(pack({1, 1000, 1, 77}, big, &p) == 0 && p.launches == 1 && p.continuations == 0);
    // a thread limit that forces a split in mid-entry: 3 tiles a launch, an entry of 5
    CHECK(pack({5}, 3, &p) == 0 && p.launches == 2 && p.pieces == 2 && p.continuations == 1);
    CHECK(pack({1, 5, 1}, 3, &p) == 0 && p.launches == 3 && p.continuations == 1);
    CHECK(pack({1, 6, 1}, 3, &p) == 0 && p.launches == 3 && p.continuations == 2);
    CHECK(pack({2, 2, 2}, 3, &p) == 0 && p.launches == 2 && p.continuations == 1);
    CHECK(pack({7}, 1, &p) == 0 && p.launches == 7 && p.continuations == 6);
    CHECK(pack({3, 3}, 0, &p) == 0 && p.launches == 6);   // no room for a workgroup: one a launch
    // both limits together
    CHECK(pack(std::vector<size_t>(20, 2), 7, &p) == 0 && p.pieces == 20 + p.continuations);
    // the emit's verdict ends the walk
    int calls = 0;
    const size_t t3[3] = {1, 1, 1};
    CHECK(!many_pack(t3, 3, 1, [&](const ManyPiece *, int, size_t) { return ++calls < 2; }));
    CHECK(calls == 2);
    return 0;
}

static int ov(std::vector<uintptr_t> t, std::vector<uintptr_t> s, std::vector<size_t> b)
{
    int other = -1;
    return many_overlap((int) t.size(), t.data(), s.data(), b.data(), &other);
}

static int overlap()
{
    CHECK(ov({}, {}, {}) == -1);
    CHECK(ov({100}, {100}, {50}) == -1);            // target i on source i: the in-place call
    CHECK(ov({100}, {120}, {50}) == -1);            // ... partly
    CHECK(ov({100, 200}, {100, 200}, {50, 50}) == -1);
    CHECK(ov({100, 150}, {300, 400}, {50, 50}) == -1);   // targets that only touch
    CHECK(ov({100, 300}, {150, 250}, {50, 50}) == -1);   // target 0 touches source 0 and 1
    CHECK(ov({100, 500}, {300, 300}, {50, 50}) == -1);   // shared sources
    CHECK(ov({100, 149}, {300, 400}, {50, 50}) >= 0);    // target against target, one byte
    CHECK(ov({100, 100}, {300, 400}, {50, 50}) >= 0);
    CHECK(ov({100, 500}, {300, 120}, {50, 50}) >= 0);    // target 0 against source 1
    CHECK(ov({500, 100}, {120, 300}, {50, 50}) >= 0);    // ... the other way round
    CHECK(ov({100, 500}, {300, 99}, {50, 2}) >= 0);      // a source that ends inside a target
    CHECK(ov({100, 500}, {300, 98}, {50, 2}) == -1);     // ... that only touches it
    CHECK(ov({100, 120}, {300, 400}, {50, 0}) == -1);    // empty entries overlap nothing
    CHECK(ov({100, 120}, {300, 400}, {0, 50}) == -1);
    // a long range that covers a later one past a short range in between
    CHECK(ov({1000, 2000, 150}, {100, 110, 3000}, {100, 5, 10}) >= 0);  // target 2 inside source 0
    CHECK(ov({1000, 2000, 250}, {100, 110, 3000}, {100, 5, 10}) == -1);
    CHECK(ov({100, 2000, 3000}, {100, 4000, 150}, {100, 5, 10}) >= 0);  // source 2 inside target 0
    // in place, and another entry's target inside it: the entry's own source
    // reaches furthest, the culprit is the second furthest
    CHECK(ov({100, 120}, {100, 900}, {100, 10}) >= 0);
    CHECK(ov({100, 900}, {100, 120}, {100, 10}) >= 0);
    // many disjoint in-place entries, then one that runs into the middle one
    std::vector<uintptr_t> t, s;
    std::vector<size_t> b;
    for (int i = 0; i < 40; i++) t.push_back(1000 + 64 * (uintptr_t) i), s.push_back(t.back()), b.push_back(64);
    CHECK(ov(t, s, b) == -1);
    t.push_back(1000 + 64 * 20 + 63), s.push_back(90000), b.push_back(1);
    CHECK(ov(t, s, b) >= 0);
    int other = -1;
    const int bad = many_overlap((int) t.size(), t.data(), s.data(), b.data(), &other);
    CHECK((bad == 20 && other == 40) || (bad == 40 && other == 20));
    return 0;
}

// P members, a table of int sums, each member folding in its own order;
// against a plain per-entry fold
static int fold(int P, std::vector<int> lens, int inplace)
{
    const int M = (int) lens.size();
    // heap[p][i]: member p's array i, malloc'ed to the byte
    std::vector<std::vector<int32_t *>> heap(P, std::vector<int32_t *>(M));
    std::vector<size_t> bytes(M), nel(M);
    size_t most = 0;
    for (int i = 0; i < M; i++) {
        nel[i] = (size_t) lens[i];
        bytes[i] = nel[i] * 4;
        most = bytes[i] > most ? bytes[i] : most;
        for (int p = 0; p < P; p++) {
            heap[p][i] = (int32_t *) malloc(bytes[i] ? bytes[i] : 1);
            for (size_t k = 0; k < nel[i]; k++) heap[p][i][k] = (int32_t) (1000 * p + 100000 * i + k);
        }
    }
    int rc = 0;
    for (int m = 0; m < P && !rc; m++) {
        std::vector<int> order;
        order.push_back(m);
        for (int p = 0; p < P; p++)
            if (p != m) order.push_back(p);
        std::vector<void *> accs(M);
        std::vector<const void *> src(M);
        for (int i = 0; i < M; i++) {
            // entry `inplace` folds onto a temporary, as the library does for an overlap
            accs[i] = malloc(bytes[i] ? bytes[i] : 1);
            src[i] = heap[m][i];
        }
        int32_t *peer = P > 1 ? (int32_t *) malloc(most ? most : 1) : nullptr;
        int gets = 0, betweens = 0, nonempty = 0;
        for (int i = 0; i < M; i++) nonempty += bytes[i] ? 1 : 0;
        const bool ok = many_host_fold(
            M, accs.data(), src.data(), bytes.data(), nel.data(), peer, order.data(), P,
            [&](void *dst, const void *s, size_t n, int pe) {
                // the runtime's getmem: `s` is MY address of a symmetric object
                int i = 0;
                while (i < M && s != (const void *) heap[m][i]) i++;
                if (i == M || n != bytes[i] || betweens != 1) { rc = 1; return; }
                memcpy(dst, heap[pe][i], n);
                gets++;
            },
            [&](void *a, const void *in, size_t n, int i) {
                if (n != nel[i] || a != accs[i]) rc = 1;
                for (size_t k = 0; k < n; k++) ((int32_t *) a)[k] += ((const int32_t *) in)[k];
                return true;
            },
            [&] { betweens++; });
        if (!ok || gets != (P - 1) * nonempty || betweens != 1) rc = 1;
        for (int i = 0; i < M && !rc; i++)
            for (size_t k = 0; k < nel[i]; k++) {
                int32_t want = 0;
                for (int p = 0; p < P; p++) want += (int32_t) (1000 * p + 100000 * i + k);
                if (((int32_t *) accs[i])[k] != want) rc = 1;
            }
        // the copy back of the in-place entry onto my own source, then restore
        if (!rc && inplace >= 0 && bytes[inplace]) {
            memcpy(heap[m][inplace], accs[inplace], bytes[inplace]);
            for (size_t k = 0; k < nel[inplace]; k++)
                heap[m][inplace][k] = (int32_t) (1000 * m + 100000 * inplace + k);
        }
        for (int i = 0; i < M; i++) free(accs[i]);
        free(peer);
    }
    for (int p = 0; p < P; p++)
        for (int i = 0; i < M; i++) free(heap[p][i]);
    if (rc) printf("fold P=%d M=%d failed\n", P, M);
    return rc;
}

static int fold_fails()
{
    int32_t a[4] = {1, 2, 3, 4}, t[4], peer[4];
    void *accs[1] = {t};
    const void *src[1] = {a};
    const size_t bytes[1] = {16}, nel[1] = {4};
    const int order[2] = {0, 1};
    const bool ok = many_host_fold(
        1, accs, src, bytes, nel, peer, order, 2,
        [&](void *dst, const void *s, size_t n, int) { memcpy(dst, s, n); },
        [&](void *, const void *, size_t, int) { return false; }, [] {});
    CHECK(!ok);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 1;
    const char *c = argv[1];
    int rc = 1;
    if (!strcmp(c, "routes")) rc = routes();
    else if (!strcmp(c, "packing")) rc = packing();
    else if (!strcmp(c, "overlap")) rc = overlap();
    else if (!strcmp(c, "fold1")) rc = fold(1, {1001, 0, 7}, 0);
    else if (!strcmp(c, "fold3")) rc = fold(3, {1001, 1, 0, 513, 3}, 3) || fold(3, {5}, -1);
    else if (!strcmp(c, "fold8")) rc = fold(8, std::vector<int>(17, 33), 16);
    else if (!strcmp(c, "fold_empty")) rc = fold(4, {0, 0, 0}, -1) || fold(2, {}, -1) || fold_fails();
    else return 1;
    if (rc == 0) printf("ok\n");
    return rc;
}
