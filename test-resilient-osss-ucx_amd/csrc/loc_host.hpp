// loc_host.hpp -- the HIP-free arithmetic of osgpu_reduce_loc
// (shmem_reduce.cpp, team.hip, host_fold.hip): the byte counts of a call with
// a value and an index stream, which arrays may overlap, the vector split of
// two streams with elements of different sizes, GETMEM's chunk, the walk over
// more than 8 inputs, and the host fold over a step passed as a type
// (elem_ops.hpp LocStep: the one definition the kernels use too).  No HIP, no
// runtime: also built into tests/support/loc_host_check with ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "scan_host.hpp"

namespace osgpu {
namespace rt {

constexpr int kLocMaxInputs = 8;  // inputs of one launch (combine.hpp kMaxTeam)
constexpr size_t kLocIndexBytes = 4;

// The 16 pairs of the call: max / min of short, int, long, long long, float,
// double, half and bfloat16 (type / op codes: scan_host.hpp's copy of
// include/osgpu_reduce.h's).  Long double (no team or host fold of a pair at
// 16 bytes an element) and the complex types (unordered) are not served.
inline bool loc_pair(int type, int op)
{
    if (op != SCAN_OP_MAX && op != SCAN_OP_MIN) return false;
    switch (type) {
    case SCAN_T_SHORT: case SCAN_T_INT: case SCAN_T_LONG: case SCAN_T_LONGLONG:
    case SCAN_T_FLOAT: case SCAN_T_DOUBLE: case SCAN_T_HALF: case SCAN_T_BFLOAT16:
        return true;
    }
    return false;
}

// Elements one lane step covers: whole 16-byte vectors of both streams, so
// max(16 / elem, 4) -- 8 for 2-byte values (1 value vector, 2 index vectors),
// 4 for 4-byte (1 and 1) and 8-byte ones (2 and 1).  0: no such element size.
inline size_t loc_group(size_t elem)
{
    if (elem != 2 && elem != 4 && elem != 8) return 0;
    return 16 / elem > 4 ? 16 / elem : 4;
}

// member j's PE number: the index every element of member j carries when the
// call passes no index source
inline int loc_member_pe(int PE_start, int logPE_stride, int j)
{
    return PE_start + (int) ((unsigned) j << logPE_stride);
}

// All in size_t.
struct LocBytes {
    size_t vbytes;        // one value array
    size_t lbytes;        // one index array
    size_t pulled_bound;  // what a member pulls from its P - 1 peers: (P - 1) * n *
                          //   (elem + 4), (P - 1) * n * elem without index sources
};

// false: not a call (nreduce < 0, P < 1, no such element size) or a byte
// count does not fit size_t
inline bool loc_bytes(size_t elem, long long nreduce, int P, bool has_loc, LocBytes *b)
{
    if (loc_group(elem) == 0 || nreduce < 0 || P < 1) return false;
    const size_t n = (size_t) nreduce, lim = (size_t) -1, per = elem + kLocIndexBytes;
    if (n != 0 && (per > lim / n || n * per > lim / (size_t) P)) return false;
    b->vbytes = n * elem;
    b->lbytes = n * kLocIndexBytes;
    b->pulled_bound = (size_t) (P - 1) * n * (has_loc ? per : elem);
    return true;
}

inline bool loc_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
    return x < y + nb && y < x + na;
}

// The overlaps a call refuses: a value array with an index array, and the two
// targets (the same thing).  target with source and loc_target with
// loc_source may overlap (temporaries).  The refused pair's names, or nullptr.
inline const char *loc_cross_overlap(const void *target, const void *source, size_t vbytes,
                                     const void *loc_target, const void *loc_source, size_t lbytes)
{
    if (loc_overlap(target, vbytes, loc_target, lbytes)) return "target and loc_target";
    if (loc_overlap(target, vbytes, loc_source, lbytes)) return "target and loc_source";
    if (loc_overlap(source, vbytes, loc_target, lbytes)) return "source and loc_target";
    if (loc_overlap(source, vbytes, loc_source, lbytes)) return "source and loc_source";
    return nullptr;
}

// ------------------------------------------------------------ vector split
// n elements as [0, head) up to the first element at which EVERY value
// pointer and EVERY index pointer sits on a 16-byte boundary, ngroups whole
// groups of loc_group(elem) elements, then the tail from tail_start;
// nedge = head + tail elements (fewer than two groups).  vec false (the rest
// 0): no head below one group aligns them all, the element-granular kernel
// serves.  A head longer than n is cut to n (everything is edge).
struct LocSplit {
    bool vec;
    size_t head, ngroups, tail_start;
    int nedge;
};

inline LocSplit loc_split(size_t elem, size_t n, const void *const *vals, int nv,
                          const void *const *locs, int nl)
{
    const size_t g = loc_group(elem);
    const LocSplit none{false, 0, 0, 0, 0};
    if (g == 0 || nv < 1) return none;
    for (size_t h = 0; h < g; h++) {
        bool ok = true;
        for (int i = 0; ok && i < nv; i++) ok = (((uintptr_t) vals[i] + h * elem) & 15) == 0;
        for (int i = 0; ok && i < nl; i++)
            ok = (((uintptr_t) locs[i] + h * kLocIndexBytes) & 15) == 0;
        if (!ok) continue;
        const size_t head = h > n ? n : h;
        const size_t ngroups = (n - head) / g, tail_start = head + ngroups * g;
        return LocSplit{true, head, ngroups, tail_start, (int) (head + (n - tail_start))};
    }
    return none;
}

// GETMEM's chunk in elements: chunk_bytes' worth of both streams, a whole
// number of groups of 8 (so every slot of the staging starts on a 16-byte
// boundary for every element size), at least one
inline size_t loc_chunk_elems(size_t chunk_bytes, size_t elem, size_t nreduce)
{
    size_t c = chunk_bytes / (elem + kLocIndexBytes) / 8 * 8;
    if (c == 0) c = 8;
    const size_t whole = (nreduce + 7) / 8 * 8;
    return c > whole ? whole : c;
}

// ---------------------------------------------------- more than 8 inputs
// The members 0 .. P-1 in launches of at most kLocMaxInputs inputs:
// fn(first, count, feedback) -- members [first, first + count), and when
// feedback is set the pair the launches so far left in (target, loc_target)
// as input 0 before them (count <= kLocMaxInputs - 1 then).  The fold is
// associative over such chunks because input 0 comes first.
template <class Fn>
void loc_for_input_chunks(int P, Fn fn)
{
    int first = 0;
    while (first < P) {
        const bool feedback = first > 0;
        const int room = kLocMaxInputs - (feedback ? 1 : 0);
        const int count = P - first < room ? P - first : room;
        fn(first, count, feedback);
        first += count;
    }
}

// ------------------------------------------------------------ the host fold
// (v[k], i[k]) takes (b[k], ib ? ib[k] : ib_const) by Step::f for k < n
template <class Step, typename T>
void loc_fold_n(T *v, int32_t *i, const T *b, const int32_t *ib, int32_t ib_const, size_t n)
{
    for (size_t k = 0; k < n; k++) Step::f(v[k], i[k], b[k], ib ? ib[k] : ib_const);
}

}  // namespace rt
}  // namespace osgpu
