// rscatter_host.hpp -- the HIP-free arithmetic of osgpu_reduce_scatter's host
// paths (shmem_reduce.cpp): which bytes of the P * nreduce element source a
// member folds.  No HIP, no runtime: also built into
// tests/support/rscatter_host_check with ASan + UBSan.
#pragma once
#include <stddef.h>

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

// GETMEM's chunk is every collective's (scan_host.hpp host_chunk_elems) over
// the block; the host fold is the batched call's over a table of one entry
// whose source is block m, source + offset (many_host.hpp many_host_fold).

}  // namespace rt
}  // namespace osgpu
