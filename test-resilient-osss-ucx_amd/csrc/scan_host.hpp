// scan_host.hpp -- the HIP-free arithmetic of osgpu_scan (shmem_reduce.cpp,
// team.hip): how many members' sources a member folds, the bytes it pulls on
// the host paths, the chunk and the chunk walk of every collective's GETMEM
// form, and the identity of every (type, op) as element bytes.  No HIP, no
// runtime: also built into tests/support/scan_host_check with ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace osgpu {
namespace rt {

// Member m folds the sources of members 0 .. scan_prefix_len - 1, ascending:
// 0..m inclusive, 0..m-1 exclusive.  0: no fold, the op's identity (member 0
// of an exclusive scan); 1: a copy.  -1: not a member index or a mode.
inline int scan_prefix_len(int m, int exclusive)
{
    if (m < 0 || exclusive < 0 || exclusive > 1) return -1;
    return m + 1 - exclusive;
}

// All in size_t: the byte counts of a call of INT_MAX 16-byte elements.
struct ScanBytes {
    size_t bytes;         // of one array (what the target receives)
    size_t pulled_bytes;  // what member m pulls from its peers: m arrays in either
                          //   mode (inclusive 0..m without its own, exclusive 0..m-1)
    size_t pulled_bound;  // the last member's pull, (P - 1) arrays: a size every
                          //   member shares (the host fold's limit is tested on it)
};

// false: the arguments are not a call (nreduce < 0, P < 1, m outside [0, P),
// elem == 0, a mode other than 0 / 1) or a byte count does not fit size_t
inline bool scan_bytes(size_t elem, long long nreduce, int P, int m, int exclusive, ScanBytes *b)
{
    if (elem == 0 || nreduce < 0 || P < 1 || m < 0 || m >= P || scan_prefix_len(m, exclusive) < 0)
        return false;
    const size_t n = (size_t) nreduce, lim = (size_t) -1;
    if (n != 0 && (elem > lim / n || n * elem > lim / (size_t) P)) return false;
    b->bytes = n * elem;
    b->pulled_bytes = (size_t) m * b->bytes;
    b->pulled_bound = (size_t) (P - 1) * b->bytes;
    return true;
}

// The chunk of every GETMEM form (shmem_reduce.cpp getmem_chunks) in
// elements: chunk_bytes' worth, at least one, at most the array (the
// reduce-scatter's block), rounded up to an even count
inline size_t host_chunk_elems(size_t chunk_bytes, size_t elem, size_t nreduce)
{
    size_t c = chunk_bytes / elem;
    if (c == 0) c = 1;
    if (c > nreduce) c = nreduce;
    return (c + 1) & ~(size_t) 1;
}

// fn(off, len) over [0, n) in chunks of `chunk` elements (the last one shorter)
template <class Fn>
void scan_for_chunks(size_t n, size_t chunk, Fn fn)
{
    if (chunk == 0) chunk = 1;
    for (size_t off = 0; off < n; off += chunk) fn(off, n - off < chunk ? n - off : chunk);
}

// ------------------------------------------------------------- identities
// type / op codes: the numbering of include/osgpu_reduce.h (OSGPU_T_*,
// OSGPU_OP_*), repeated here to stay free of every other header;
// shmem_reduce.cpp asserts that they agree.
enum { SCAN_T_SHORT = 0, SCAN_T_INT, SCAN_T_LONG, SCAN_T_LONGLONG, SCAN_T_FLOAT, SCAN_T_DOUBLE,
       SCAN_T_LONGDOUBLE, SCAN_T_COMPLEXF, SCAN_T_COMPLEXD, SCAN_T_HALF, SCAN_T_BFLOAT16 };
enum { SCAN_OP_SUM = 0, SCAN_OP_PROD, SCAN_OP_AND, SCAN_OP_OR, SCAN_OP_XOR, SCAN_OP_MAX,
       SCAN_OP_MIN };

// The identity of (type, op) as the bytes of one element, little endian, in
// out[0 .. size); the rest of out[16] zero (so long double's 6 padding bytes
// are).  Returns the element's size, 0 for a pair that is no reduction of
// the library (integers take all seven ops, real types sum / prod / max /
// min, complex types sum / prod).
//   sum all-zero bits; prod 1; and all-one bits; or, xor 0;
//   max the type's lowest value (integer minimum, -inf);
//   min the type's highest value (integer maximum, +inf).
inline size_t scan_identity(int type, int op, unsigned char out[16])
{
    memset(out, 0, 16);
    if (op < SCAN_OP_SUM || op > SCAN_OP_MIN) return 0;
    const bool bitop = op == SCAN_OP_AND || op == SCAN_OP_OR || op == SCAN_OP_XOR;
    const bool minmax = op == SCAN_OP_MAX || op == SCAN_OP_MIN;
    auto put = [&](uint64_t v, size_t size, size_t at = 0) {
        for (size_t i = 0; i < size; i++) out[at + i] = (unsigned char) (v >> (8 * i));
    };
    size_t size = 0;
    switch (type) {
    case SCAN_T_SHORT: size = 2; break;
    case SCAN_T_INT: size = 4; break;
    case SCAN_T_LONG: case SCAN_T_LONGLONG: size = 8; break;
    }
    if (size) {  // integers
        const uint64_t top = (uint64_t) 1 << (8 * size - 1);
        switch (op) {
        case SCAN_OP_PROD: put(1, size); break;
        case SCAN_OP_AND: put(~(uint64_t) 0, size); break;
        case SCAN_OP_MAX: put(top, size); break;       // the minimum
        case SCAN_OP_MIN: put(top - 1, size); break;   // the maximum
        }
        return size;
    }
    if (bitop) return 0;
    // floating point: the patterns of 1, -inf and +inf per format
    uint64_t one = 0, ninf = 0, pinf = 0;
    switch (type) {
    case SCAN_T_FLOAT: case SCAN_T_COMPLEXF:
        size = 4, one = 0x3f800000u, pinf = 0x7f800000u, ninf = 0xff800000u; break;
    case SCAN_T_DOUBLE: case SCAN_T_COMPLEXD:
        size = 8, one = 0x3ff0000000000000ull, pinf = 0x7ff0000000000000ull,
        ninf = 0xfff0000000000000ull; break;
    case SCAN_T_HALF: size = 2, one = 0x3c00u, pinf = 0x7c00u, ninf = 0xfc00u; break;
    case SCAN_T_BFLOAT16: size = 2, one = 0x3f80u, pinf = 0x7f80u, ninf = 0xff80u; break;
    case SCAN_T_LONGDOUBLE: {
        // x87 extended: 64-bit significand with an explicit integer bit, then
        // sign and 15-bit exponent; bytes 10..15 padding, zero
        if (op != SCAN_OP_SUM) {
            put(0x8000000000000000ull, 8);
            put(op == SCAN_OP_PROD ? 0x3fffu : op == SCAN_OP_MAX ? 0xffffu : 0x7fffu, 2, 8);
        }
        return 16;
    }
    default: return 0;
    }
    if (type == SCAN_T_COMPLEXF || type == SCAN_T_COMPLEXD) {
        if (minmax) return 0;
        if (op == SCAN_OP_PROD) put(one, size);  // 1 + 0i
        return 2 * size;
    }
    if (op == SCAN_OP_PROD) put(one, size);
    else if (op == SCAN_OP_MAX) put(ninf, size);
    else if (op == SCAN_OP_MIN) put(pinf, size);
    return size;
}

// n elements of the identity of (type, op) into dst (host memory); false for
// a pair that is no reduction
inline bool scan_fill_identity(int type, int op, void *dst, size_t n)
{
    unsigned char id[16];
    const size_t s = scan_identity(type, op, id);
    if (!s) return false;
    for (size_t i = 0; i < n; i++) memcpy((char *) dst + i * s, id, s);
    return true;
}

}  // namespace rt
}  // namespace osgpu
