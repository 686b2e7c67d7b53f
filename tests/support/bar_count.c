/*
 * bar_count.c -- TEST INFRASTRUCTURE: a struct osgpu_pe_ops table that
 * forwards to another one (tests/support/pe_threads.c's) and counts, per PE,
 * the barriers the library asks for.  tests/test_gpu_many.py installs it to
 * assert that osgpu_reduce_many makes exactly two, whatever its count.
 */
#include <stddef.h>

typedef struct {
    int (*my_pe)(void);
    int (*n_pes)(void);
    void (*barrier)(int, int, int, long *);
    void (*getmem)(void *, const void *, size_t, int);
} pe_ops_t;

#define MAXPE 64

static pe_ops_t g_inner, g_table;
static long g_calls[MAXPE];

static void bc_barrier(int PE_start, int logPE_stride, int PE_size, long *pSync)
{
    const int me = g_inner.my_pe();
    if (me >= 0 && me < MAXPE) __atomic_add_fetch(&g_calls[me], 1, __ATOMIC_RELAXED);
    g_inner.barrier(PE_start, logPE_stride, PE_size, pSync);
}

/* the counting table over `inner` (a pe_ops_t that outlives it); counters reset */
const void *bc_wrap(const void *inner)
{
    g_inner = *(const pe_ops_t *) inner;
    g_table = g_inner;
    g_table.barrier = bc_barrier;
    for (int i = 0; i < MAXPE; i++) g_calls[i] = 0;
    return &g_table;
}

long bc_calls(int pe) { return pe >= 0 && pe < MAXPE ? __atomic_load_n(&g_calls[pe], __ATOMIC_RELAXED) : -1; }
