// coll.hpp -- the HIP-free core of runtime.hpp: error reporting, the debug
// trace, the PE services borrowed from the application's OpenSHMEM runtime
// and the active set of one collective call.  The job-setup pieces built on
// these alone (psync_board.hpp, fd_channel.hpp) compile and run without a GPU.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <unistd.h>

namespace osgpu {
namespace rt {

void set_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
int debug_level();

// OSGPU_DEBUG=1: one stderr line per protocol step (call entry, path,
// barriers, launches, syncs) -- for diagnosing multi-process runs
#define DBG(...)                                                               \
    do {                                                                       \
        if (::osgpu::rt::debug_level() > 0) {                                  \
            fprintf(stderr, "[osgpu pid %d] ", (int) getpid());                \
            fprintf(stderr, __VA_ARGS__);                                      \
            fputc('\n', stderr);                                               \
            fflush(stderr);                                                    \
        }                                                                      \
    } while (0)

struct PeOps {
    int (*my_pe)(void) = nullptr;
    int (*n_pes)(void) = nullptr;
    void (*barrier)(int, int, int, long *) = nullptr;
    void (*getmem)(void *, const void *, size_t, int) = nullptr;
};

// One collective call on an active set (PE_start, 2^logPE_stride, PE_size).
struct Coll {
    const char *name = nullptr;
    int PE_start = 0, logPE_stride = 0, PE_size = 0;
    long *pSync = nullptr;
    int me = -1, step = 1;
    PeOps ops;
    // index of PE `pe` in the active set, or -1
    int index_of(int pe) const
    {
        if (pe < PE_start || (pe - PE_start) % step) return -1;
        const int i = (pe - PE_start) / step;
        return i < PE_size ? i : -1;
    }
    int pe_at(int i) const { return PE_start + i * step; }
};

void barrier(const Coll &c);

}  // namespace rt
}  // namespace osgpu
