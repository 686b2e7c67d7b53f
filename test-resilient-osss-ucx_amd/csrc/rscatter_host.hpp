// rscatter_host.hpp -- the HIP-free arithmetic of osgpu_reduce_scatter's host
// paths (shmem_reduce.cpp): which bytes of the P * nreduce element source a
// member folds, and the host fold's loop over them.  No HIP, no runtime: also
// built into tests/support/rscatter_host_check with ASan + UBSan.
#pragma once
#include <stddef.h>
#include <string.h>

namespace osgpu {
namespace rt {

// Member m of P folds block m: elements [m * nreduce, (m + 1) * nreduce) of
// every member's source.  All in size_t: P * nreduce may exceed INT_MAX.
struct RsBlock {
    size_t bytes;         // of one block (what the target receives)
    size_t offset;        // of block m from `source`
    size_t source_bytes;  // of the whole source, P blocks
    size_t pulled_bytes;  // what the caller pulls from its peers: (P - 1) blocks
};

// false: the arguments are not a call (nreduce < 0, P < 1, m outside [0, P),
// elem == 0) or a byte count does not fit size_t
inline bool rs_block(size_t elem, long long nreduce, int P, int m, RsBlock *b)
{
    if (elem == 0 || nreduce < 0 || P < 1 || m < 0 || m >= P) return false;
    const size_t n = (size_t) nreduce, lim = (size_t) -1;
    if (n != 0 && (elem > lim / n || n * elem > lim / (size_t) P)) return false;
    b->bytes = n * elem;
    b->offset = (size_t) m * b->bytes;
    b->source_bytes = (size_t) P * b->bytes;
    b->pulled_bytes = (size_t) (P - 1) * b->bytes;
    return true;
}

// GETMEM's chunk in elements: chunk_bytes' worth, at least one, at most the
// block, rounded up to an even count (as run_host does)
inline size_t rs_chunk_elems(size_t chunk_bytes, size_t elem, size_t nreduce)
{
    size_t c = chunk_bytes / elem;
    if (c == 0) c = 1;
    if (c > nreduce) c = nreduce;
    return (c + 1) & ~(size_t) 1;
}

// The host fold of one member: acc = my own block, then every other member's
// block in my fold order (order[0] is me), each pulled by ONE getmem of
// exactly b.bytes from source + b.offset into `peer` (b.bytes, unused when
// P == 1: pass nullptr).  between(): called once after the own copy (the
// entry barrier).  false when a fold step fails.
template <class Getmem, class Fold, class Between>
bool rs_host_fold(const RsBlock &b, const void *source, void *acc, void *peer, const int *order,
                  int P, size_t nreduce, Getmem getmem, Fold fold, Between between)
{
    const char *mine = (const char *) source + b.offset;
    if (b.bytes) memmove(acc, mine, b.bytes);
    between();
    for (int k = 1; k < P; k++) {
        getmem(peer, mine, b.bytes, order[k]);
        if (!fold(acc, peer, nreduce)) return false;
    }
    return true;
}

}  // namespace rt
}  // namespace osgpu
