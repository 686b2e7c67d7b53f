// many_host.hpp -- the HIP-free logic of the batched reduce-to-all
// (osgpu_reduce_many, osgpu_combine_many): which kernel an entry of the table
// takes, how the entries of the batch kernel are packed into launches, the
// overlap check of the table, and the host fold's loop over it.  Pure
// functions from sizes and addresses to a plan.  No HIP, no runtime: also
// built into tests/support/many_host_check with ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace osgpu {

// segments of independent arrays one launch of combine_many_kernel holds
// (combine.hip: the table travels in the kernel arguments)
constexpr int kManySegs = 16;

namespace rt {

// ------------------------------------------------------------------ routes
// What launch_combine_many does with one entry of nsrc inputs of n elements
// of `elem` bytes (16 for long double): a segment of the batch kernel, or a
// launch of its own.
enum ManyRoute {
    MANY_SKIP = 0,     // n == 0
    MANY_BATCH,        // 2..8 inputs, target and inputs at one 16-byte phase
    MANY_SHIFTED,      // a phase mismatch or a pointer off its element: launch_combine_shifted
    MANY_LONGDOUBLE,   // launch_longdouble, whatever else holds
    MANY_CHUNKS,       // more than 8 inputs: launch_combine's chunks of 8 with feedback
    MANY_COPY,         // one input
    MANY_NROUTES
};

inline ManyRoute many_route(size_t elem, bool longdouble, int nsrc, size_t n, uintptr_t target,
                            const uintptr_t *srcs)
{
    if (n == 0) return MANY_SKIP;
    if (longdouble) return MANY_LONGDOUBLE;
    if (nsrc == 1) return MANY_COPY;
    // vec_split's verdict (kernel_common.hpp): one phase, a multiple of the element
    const uintptr_t phase = target & 15;
    bool same = elem <= 16 && phase % elem == 0;
    for (int k = 0; k < nsrc; k++) same = same && (srcs[k] & 15) == phase;
    if (!same) return MANY_SHIFTED;
    return nsrc > 8 ? MANY_CHUNKS : MANY_BATCH;
}

// workgroups of a batch entry of nvec whole vectors in tiles of V: edges
// alone still take one
inline size_t many_tiles(size_t nvec, size_t V)
{
    const size_t t = (nvec + V - 1) / V;
    return t ? t : 1;
}

// ----------------------------------------------------------------- packing
// One segment of a launch: tiles [tile0, tile0 + ntiles) of table entry
// `entry`, from workgroup `first` of the launch.  tile0 > 0: a continuation
// -- no edges, pointers advanced by tile0 tiles (for_each_tile_run's rule).
struct ManyPiece {
    int entry;
    size_t tile0, ntiles;
    unsigned first;
};

// Greedy, in table order: tiles[i] workgroups for entry i (0: the entry is
// not on the batch kernel), at most kManySegs pieces and launch_tiles
// workgroups per launch; an entry that does not fit the remaining room is
// split at a tile boundary.  emit(pieces, npieces, workgroups) per launch;
// false as soon as one fails.
template <class Emit>
bool many_pack(const size_t *tiles, int count, size_t launch_tiles, Emit emit)
{
    if (launch_tiles == 0) launch_tiles = 1;
    if (launch_tiles > 0xFFFFFFFFu) launch_tiles = 0xFFFFFFFFu;  // `first` and the grid are 32-bit
    ManyPiece pc[kManySegs];
    int np = 0;
    size_t used = 0;
    for (int i = 0; i < count; i++) {
        size_t t0 = 0;
        while (t0 < tiles[i]) {
            if (np == kManySegs || used == launch_tiles) {
                if (!emit((const ManyPiece *) pc, np, used)) return false;
                np = 0;
                used = 0;
            }
            const size_t room = launch_tiles - used, left = tiles[i] - t0;
            const size_t take = left < room ? left : room;
            pc[np++] = ManyPiece{i, t0, take, (unsigned) used};
            used += take;
            t0 += take;
        }
    }
    return np == 0 || emit((const ManyPiece *) pc, np, used);
}

// ----------------------------------------------------------- overlap check
// The table's contract: a non-empty targets[i] shares no byte with
// targets[j] or sources[j] of any other entry j (targets[i] against
// sources[i] is the in-place call; sources may share).  Returns -1, or the
// index of an entry whose target breaks it, *other the entry it runs into.
// Sorted sweep, O(count log count): of the ranges that start at or before
// x, only the one reaching furthest can be the first to cover x's start --
// the furthest two of each kind, since x's own entry does not count.
inline int many_overlap(int count, const uintptr_t *targets, const uintptr_t *sources,
                        const size_t *bytes, int *other)
{
    struct Range {
        uintptr_t lo, hi;
        int entry;
        bool target;
    };
    std::vector<Range> r;
    r.reserve(2 * (size_t) (count > 0 ? count : 0));
    for (int i = 0; i < count; i++) {
        if (bytes[i] == 0) continue;
        r.push_back(Range{targets[i], targets[i] + bytes[i], i, true});
        r.push_back(Range{sources[i], sources[i] + bytes[i], i, false});
    }
    std::sort(r.begin(), r.end(), [](const Range &a, const Range &b) { return a.lo < b.lo; });
    struct Far {  // the two ranges of one kind seen so far that end last (distinct entries)
        uintptr_t hi[2] = {0, 0};
        int entry[2] = {-1, -1};
        void add(uintptr_t h, int e)
        {
            if (entry[0] < 0 || h > hi[0]) {
                hi[1] = hi[0], entry[1] = entry[0];
                hi[0] = h, entry[0] = e;
            } else if (entry[1] < 0 || h > hi[1]) {
                hi[1] = h, entry[1] = e;
            }
        }
        // an entry other than e whose range passes lo, or -1
        int past(uintptr_t lo, int e) const
        {
            for (int k = 0; k < 2; k++)
                if (entry[k] >= 0 && entry[k] != e && hi[k] > lo) return entry[k];
            return -1;
        }
    } tg, sr;
    for (const Range &x : r) {
        int j = tg.past(x.lo, x.entry);          // an earlier target reaches into x
        if (j >= 0) {
            if (other) *other = x.entry;
            return j;
        }
        if (x.target && (j = sr.past(x.lo, x.entry)) >= 0) {  // x, a target, starts inside a source
            if (other) *other = j;
            return x.entry;
        }
        (x.target ? tg : sr).add(x.hi, x.entry);
    }
    return -1;
}

// ---------------------------------------------------------------- host fold
// The host fold of one member over the table: accs[i] = my own sources[i]
// for every entry, between() (the entry barrier), then per entry every other
// member's array in my fold order (order[0] is me), each pulled by ONE getmem
// of exactly bytes[i] into `peer` (the largest entry's bytes; unused at
// P == 1) and folded over nelems[i].  Empty entries are skipped.  false when
// a fold step fails.
template <class Getmem, class Fold, class Between>
bool many_host_fold(int count, void *const *accs, const void *const *sources, const size_t *bytes,
                    const size_t *nelems, void *peer, const int *order, int P, Getmem getmem,
                    Fold fold, Between between)
{
    for (int i = 0; i < count; i++)
        if (bytes[i]) memmove(accs[i], sources[i], bytes[i]);
    between();
    for (int i = 0; i < count; i++) {
        if (!bytes[i]) continue;
        for (int k = 1; k < P; k++) {
            getmem(peer, sources[i], bytes[i], order[k]);
            if (!fold(accs[i], peer, nelems[i], i)) return false;
        }
    }
    return true;
}

}  // namespace rt
}  // namespace osgpu
