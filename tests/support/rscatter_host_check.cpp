// rscatter_host_check.cpp -- TEST INFRASTRUCTURE: the HIP-free arithmetic of
// osgpu_reduce_scatter's host paths with its own main, built plain and with
// ASan + UBSan (tests/support/host_check_build.py): the block's bytes
// (csrc/rscatter_host.hpp), and the two helpers the call shares with the
// other collectives AS IT USES THEM -- GETMEM's chunk over the block
// (scan_host.hpp host_chunk_elems) and the host fold over a table of one
// entry whose source is block m of the source (many_host.hpp many_host_fold).
// Every "heap" is a malloc of EXACTLY the source's bytes, every target and
// peer buffer of exactly one block: a getmem or fold that leaves block m is a
// heap-buffer-overflow.  Prints "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../test-resilient-osss-ucx_amd/csrc/many_host.hpp"
#include "../../test-resilient-osss-ucx_amd/csrc/rscatter_host.hpp"
#include "../../test-resilient-osss-ucx_amd/csrc/scan_host.hpp"

using osgpu::rt::RsBlock;

#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            printf("%s:%d: %s\n", __FILE__, __LINE__, #x);          \
            return 1;                                               \
        }                                                           \
    } while (0)

static int blocks()
{
    RsBlock b;
    CHECK(osgpu::rt::rs_block(8, 1001, 3, 2, &b));
    CHECK(b.bytes == 8008 && b.offset == 16016 && b.source_bytes == 24024 && b.pulled_bytes == 16016);
    CHECK(osgpu::rt::rs_block(2, 1, 1, 0, &b));
    CHECK(b.bytes == 2 && b.offset == 0 && b.source_bytes == 2 && b.pulled_bytes == 0);
    CHECK(osgpu::rt::rs_block(16, 0, 8, 7, &b) && b.bytes == 0 && b.source_bytes == 0);
    // P * nreduce above INT_MAX: size_t throughout
    CHECK(osgpu::rt::rs_block(16, 2147483647, 8, 7, &b));
    CHECK(b.bytes == (size_t) 2147483647 * 16 && b.offset == 7 * b.bytes &&
          b.source_bytes == 8 * b.bytes);
    CHECK(!osgpu::rt::rs_block(8, -1, 2, 0, &b) && !osgpu::rt::rs_block(8, 4, 2, 2, &b) &&
          !osgpu::rt::rs_block(8, 4, 0, 0, &b) && !osgpu::rt::rs_block(0, 4, 2, 0, &b) &&
          !osgpu::rt::rs_block(8, 4, 2, -1, &b));
    return 0;
}

static int chunks()
{
    using osgpu::rt::host_chunk_elems;
    CHECK(host_chunk_elems(64 << 20, 8, 1001) == 1002);  // the block, rounded up to even
    CHECK(host_chunk_elems(2048, 2, 5000) == 1024);
    CHECK(host_chunk_elems(1, 16, 9) == 2 && host_chunk_elems(0, 4, 1) == 2);
    // the chunk walk covers [0, N) exactly once, no chunk past the block
    for (size_t N : {1u, 2u, 7u, 1024u, 1025u}) {
        const size_t c = host_chunk_elems(2048, 4, N);
        size_t seen = 0;
        for (size_t off = 0; off < N; off += c) seen += N - off < c ? N - off : c;
        CHECK(seen == N);
    }
    return 0;
}

// P members, each folding its block of int sums in its own order
static int fold(int P, int nreduce, bool overlap)
{
    std::vector<int32_t *> heap(P);
    RsBlock b0;
    CHECK(osgpu::rt::rs_block(4, nreduce, P, 0, &b0));
    for (int p = 0; p < P; p++) {
        heap[p] = (int32_t *) malloc(b0.source_bytes ? b0.source_bytes : 1);
        for (size_t i = 0; i < (size_t) P * nreduce; i++) heap[p][i] = (int32_t) (1000 * p + i);
    }
    for (int m = 0; m < P; m++) {
        RsBlock b;
        CHECK(osgpu::rt::rs_block(4, nreduce, P, m, &b));
        std::vector<int> order;
        order.push_back(m);
        for (int p = 0; p < P; p++)
            if (p != m) order.push_back(p);
        int32_t *acc = (int32_t *) malloc(b.bytes ? b.bytes : 1);
        int32_t *peer = P > 1 ? (int32_t *) malloc(b.bytes ? b.bytes : 1) : nullptr;
        int gets = 0, betweens = 0;
        bool sized = true;
        // the table of one entry: block m of my source, pre-offset
        void *accs[1] = {acc};
        const void *mine[1] = {(const char *) heap[m] + b.offset};
        const size_t bytes[1] = {b.bytes}, nelems[1] = {(size_t) nreduce};
        const bool ok = osgpu::rt::many_host_fold(
            1, accs, mine, bytes, nelems, peer, order.data(), P,
            [&](void *dst, const void *src, size_t n, int pe) {
                // the runtime's getmem: `src` is MY address of a symmetric object
                const size_t off = (const char *) src - (const char *) heap[m];
                sized = sized && n == b.bytes && off == b.offset;
                memcpy(dst, (const char *) heap[pe] + off, n);
                gets++;
            },
            [&](void *a, const void *in, size_t n, int entry) {
                sized = sized && entry == 0 && n == (size_t) nreduce;
                for (size_t i = 0; i < n; i++) ((int32_t *) a)[i] += ((const int32_t *) in)[i];
                return true;
            },
            [&] { betweens++; });
        // one getmem of exactly the block per peer; an empty block is skipped
        CHECK(ok && sized && gets == (b.bytes ? P - 1 : 0) && betweens == 1);
        for (int k = 0; k < nreduce; k++) {
            int32_t want = 0;
            for (int p = 0; p < P; p++) want += (int32_t) (1000 * p + (size_t) m * nreduce + k);
            CHECK(acc[k] == want);
        }
        if (overlap && b.bytes) {  // the copy back onto a block of my own source
            memcpy((char *) heap[m] + b.offset, acc, b.bytes);
            for (int k = 0; k < nreduce; k++) heap[m][(size_t) m * nreduce + k] =
                (int32_t) (1000 * m + (size_t) m * nreduce + k);
        }
        free(acc);
        free(peer);
    }
    for (int p = 0; p < P; p++) free(heap[p]);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 1;
    const char *c = argv[1];
    int rc = 1;
    if (!strcmp(c, "blocks")) rc = blocks();
    else if (!strcmp(c, "chunks")) rc = chunks();
    else if (!strcmp(c, "fold1")) rc = fold(1, 1001, false);
    else if (!strcmp(c, "fold3")) rc = fold(3, 1001, false) || fold(3, 1, true);
    else if (!strcmp(c, "fold8")) rc = fold(8, 77, true);
    else if (!strcmp(c, "fold_empty")) rc = fold(4, 0, false);
    else return 1;
    if (rc == 0) printf("ok\n");
    return rc;
}
