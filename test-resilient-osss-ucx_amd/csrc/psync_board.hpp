// psync_board.hpp -- the job-setup message board in spare pSync words.
//
// Setup calls (map_members, osgpu_heap_create) exchange one small struct per
// member through words of the symmetric pSync that the reference's barrier
// never uses (it only touches pSync[0], src/shmemc/barrier.c:64-97):
//     fill mine() -> publish() -> read(i) / read_all()
//                 [-> post_status()] -> close()
// publish, post_status and close hold one barrier each, so a caller's barrier
// count is the number of these steps it takes.  Every member reads the same
// messages, so a verdict computed from them is the same on every member.  My
// words are zero (SHMEM_SYNC_VALUE) after close and after the board goes out
// of scope, whichever way.  HIP-free: only Coll, barrier(c) and c.ops.getmem.
#pragma once
#include <string.h>

#include <type_traits>
#include <vector>

#include "coll.hpp"

namespace osgpu {
namespace rt {

template <class Msg, int Word = 16>  // pSync[Word..63], during setup only
class PsyncBoard {
    static_assert(std::is_trivially_copyable<Msg>::value, "a message is copied as bytes");
    static_assert(alignof(Msg) <= alignof(long), "a message lies on pSync words");
    // the smallest pSync a caller hands us: SHMEM_BCAST/COLLECT/ALLTOALL_SYNC_SIZE
    static_assert(Word > 0 && sizeof(Msg) <= (64 - Word) * sizeof(long), "pSync room");

public:
    explicit PsyncBoard(const Coll &c) : c_(c), mine_(reinterpret_cast<Msg *>(c.pSync + Word))
    {
        clear();
    }
    ~PsyncBoard() { clear(); }
    PsyncBoard(const PsyncBoard &) = delete;

    Msg &mine() { return *mine_; }
    void clear() { memset(mine_, 0, sizeof(Msg)); }
    // every member's message is in place
    void publish() { barrier(c_); }
    // the message of member i of the active set
    Msg read(int i) const
    {
        Msg m = *mine_;
        if (c_.pe_at(i) != c_.me) c_.ops.getmem(&m, mine_, sizeof(Msg), c_.pe_at(i));
        return m;
    }
    std::vector<Msg> read_all() const
    {
        std::vector<Msg> v;
        for (int i = 0; i < c_.PE_size; i++) v.push_back(read(i));
        return v;
    }
    // my status into `field` of my message; every member's, by set index
    std::vector<long> post_status(long Msg::*field, long status)
    {
        mine_->*field = status;
        barrier(c_);
        std::vector<long> v(c_.PE_size, status);
        for (int i = 0; i < c_.PE_size; i++)
            if (c_.pe_at(i) != c_.me)
                c_.ops.getmem(&v[i], &(mine_->*field), sizeof(long), c_.pe_at(i));
        return v;
    }
    // every member has read what it needs: pSync back to SHMEM_SYNC_VALUE
    void close()
    {
        barrier(c_);
        clear();
    }

private:
    const Coll c_;
    Msg *const mine_;
};

}  // namespace rt
}  // namespace osgpu
