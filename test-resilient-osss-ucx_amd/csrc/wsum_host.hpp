// wsum_host.hpp -- the HIP-free arithmetic of osgpu_reduce_wsum
// (shmem_reduce.cpp, team.hip, host_fold.hip): which (type, out_type) pairs
// exist, the byte counts of a call whose target may be wider than its source,
// GETMEM's chunk, the walk over more than 8 members with a float carry, and
// the host fold over a step passed as a type (elem_ops.hpp WsumStep: the one
// definition the kernels use too).  No HIP, no runtime: also built into
// tests/support/wsum_host_check with ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "scan_host.hpp"

namespace osgpu {
namespace rt {

constexpr int kWsumMaxSources = 8;  // 16-bit sources of one launch (combine.hpp kMaxTeam)
constexpr size_t kWsumGroup = 8;    // elements of one lane step: 16 bytes of a 16-bit stream
constexpr size_t kWsumSrcBytes = 2, kWsumAccBytes = 4;

// The 4 pairs of the call: half or bfloat16 sources, a target of the same
// type (the accumulator narrowed once) or of float (the accumulator itself).
// (type codes: scan_host.hpp's copy of include/osgpu_reduce.h's)
inline bool wsum_pair(int type, int out_type)
{
    if (type != SCAN_T_HALF && type != SCAN_T_BFLOAT16) return false;
    return out_type == type || out_type == SCAN_T_FLOAT;
}

// bytes of one target element; 0 for no pair
inline size_t wsum_out_size(int type, int out_type)
{
    if (!wsum_pair(type, out_type)) return 0;
    return out_type == SCAN_T_FLOAT ? kWsumAccBytes : kWsumSrcBytes;
}

// All in size_t.
struct WsumBytes {
    size_t sbytes;        // one source array: n * 2
    size_t tbytes;        // one target array: n * 2 or n * 4
    size_t abytes;        // one float accumulator array: n * 4
    size_t pulled_bound;  // what a member pulls from its P - 1 peers: (P - 1) * n * 2
};

// false: not a call (nreduce < 0, P < 1, no such target size) or a byte count
// does not fit size_t
inline bool wsum_bytes(size_t out_size, long long nreduce, int P, WsumBytes *b)
{
    if ((out_size != kWsumSrcBytes && out_size != kWsumAccBytes) || nreduce < 0 || P < 1)
        return false;
    const size_t n = (size_t) nreduce, lim = (size_t) -1;
    if (n != 0 && (kWsumAccBytes > lim / n || n * kWsumSrcBytes > lim / (size_t) P)) return false;
    b->sbytes = n * kWsumSrcBytes;
    b->tbytes = n * out_size;
    b->abytes = n * kWsumAccBytes;
    b->pulled_bound = (size_t) (P - 1) * n * kWsumSrcBytes;
    return true;
}

// A fold over more than 8 members keeps its intermediate result in float.  A
// float target is that carry itself; a 16-bit target needs abytes of scratch.
inline bool wsum_needs_carry_scratch(int P, size_t out_size)
{
    return P > kWsumMaxSources && out_size == kWsumSrcBytes;
}

// GETMEM's chunk in elements: chunk_bytes' worth of one 16-bit source, a whole
// number of groups of 8 (every staging slot of either element size then starts
// on a 16-byte boundary), at least one, at most the array rounded up
inline size_t wsum_chunk_elems(size_t chunk_bytes, size_t nreduce)
{
    size_t c = chunk_bytes / kWsumSrcBytes / kWsumGroup * kWsumGroup;
    if (c == 0) c = kWsumGroup;
    const size_t whole = (nreduce + kWsumGroup - 1) / kWsumGroup * kWsumGroup;
    return c > whole ? whole : c;
}

// ---------------------------------------------------- more than 8 members
// The members 0 .. P-1 in launches of at most kWsumMaxSources sources:
// fn(first, count, carry_in, last) -- members [first, first + count); carry_in:
// the float accumulator the launches so far left starts this one (it takes no
// source slot); last: this launch writes the target's type, every other one
// the float carry.  Exactly the definition's bits: every member's add happens
// once, in order, on an accumulator that was never rounded.
template <class Fn>
void wsum_for_source_chunks(int P, Fn fn)
{
    for (int first = 0; first < P; first += kWsumMaxSources) {
        const int count = P - first < kWsumMaxSources ? P - first : kWsumMaxSources;
        fn(first, count, first > 0, first + count == P);
    }
}

// ------------------------------------------------------------ the host fold
// Step: elem_ops.hpp WsumStep<T>.  acc[k] = widen(src[k]) (exact)
template <class Step, typename T>
void wsum_widen_n(float *acc, const T *src, size_t n)
{
    for (size_t k = 0; k < n; k++) acc[k] = Step::widen(src[k]);
}
// acc[k] = acc[k] + widen(b[k]): one float add, the NaN rule
template <class Step, typename T>
void wsum_add_n(float *acc, const T *b, size_t n)
{
    for (size_t k = 0; k < n; k++) acc[k] = Step::add(acc[k], b[k]);
}
// out[k] = narrow(acc[k]): RNE, a NaN truncated
template <class Step, typename T>
void wsum_narrow_n(T *out, const float *acc, size_t n)
{
    for (size_t k = 0; k < n; k++) out[k] = Step::narrow(acc[k]);
}

}  // namespace rt
}  // namespace osgpu
