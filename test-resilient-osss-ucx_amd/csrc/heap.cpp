// heap.cpp -- the device symmetric heap as ONE contiguous virtual range per
// PE, mapped into every member of the job (osgpu_heap_create).
//
// The reference's symmetric heap is one contiguous region per PE
// (register_symmetric_heap, src/shmemc/ucx-init.c:174-213) and a symmetric
// object of any size is found on PE p at heap_base[p] + offset
// (translate_address, src/shmemc/comms.c:89-105).  HIP IPC
// (hipIpcGetMemHandle) cannot give that on this platform: an exported
// allocation of 2 GiB or more hangs the importer, so
// objects >= 2 GiB could not be symmetric across processes.
//
// Here every PE builds its heap with the virtual memory API instead:
//   * reserve one virtual range of the heap's size (hipMemAddressReserve);
//   * back it with physical chunks of at most OSGPU_HEAP_CHUNK_BYTES
//     (default 1 GiB, a multiple of the allocation granularity), each a
//     hipMemCreate allocation exportable as a dmabuf file descriptor;
//   * map the chunks back to back: the PE's own view is contiguous;
//   * hand the chunk descriptors to every member in another process over a
//     Unix-domain socket (SCM_RIGHTS; the socket's name and the chunk layout
//     travel through spare pSync words and the runtime's shmem_getmem, like
//     the staging setup in runtime.cpp);
//   * each member imports the chunks and maps them back to back into ONE
//     virtual range of its own: its view of the peer's heap is contiguous too.
// Members that are threads of one process share the PE's range directly.
// The result is registered as segment 0 of every member's heap, so every
// path (team, pull, fused) sees base + offset for objects of any size.
#include <hip/hip_runtime_api.h>

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/osgpu_reduce.h"
#include "fd_channel.hpp"
#include "heap_host.hpp"
#include "psync_board.hpp"
#include "runtime.hpp"

namespace osgpu {
namespace rt {

namespace {

constexpr int kMaxHeapSegment = 255; // osgpu_heap_register_segment's limit

struct Mapping {                     // one heap as mapped in this process
    int pe = -1;
    int device = -1;                 // this process's device whose HBM backs it, or -1
    char *base = nullptr;
    size_t bytes = 0;                // reserved bytes
    std::vector<hipMemGenericAllocationHandle_t> h;
    std::vector<size_t> len;         // chunk lengths
    size_t nmapped = 0;              // chunks mapped so far
};
void unmap(Mapping &m);

struct Heap {                        // the heap a PE created, with its imports
    int pe = -1;
    int seg = 0;                     // registry segment of every member's heap
    long key = 0;                    // the same on every member: identifies this creation
    std::vector<int> members;
    std::vector<char *> member_base; // every member's range as seen here, by set index
    std::vector<size_t> member_bytes;
    std::vector<char> member_remote; // backed by another GPU's HBM (reached over xGMI)
    Mapping own;                     // own.pe < 0: not begun
    std::vector<Mapping> peers;      // members in other processes
    ~Heap()
    {
        for (Mapping &m : peers) unmap(m);
        if (own.pe >= 0) unmap(own);
    }
};

std::mutex g_hmu;
std::vector<Heap *> g_heaps;
// Destroyed heaps that hold chunks imported from other processes: their HBM
// is not returned before the process exits on this ROCm, so
// they are kept, fully mapped, and handed back when the same member set
// creates a heap of at most that size again (a prefix of the kept range is
// registered; every member agrees on which kept heap).
std::vector<Heap *> g_pool;

// what a PE publishes on the pSync board during osgpu_heap_create
struct HeapMsg {
    long pid, nonce, bytes, chunk, raw_ptr, status, device, seg, pci;
};

hipMemAllocationProp chunk_prop(int dev)
{
    hipMemAllocationProp p;
    memset(&p, 0, sizeof(p));
    p.type = hipMemAllocationTypePinned;
    p.requestedHandleType = hipMemHandleTypePosixFileDescriptor;
    p.location.type = hipMemLocationTypeDevice;
    p.location.id = dev;
    return p;
}

// read-write access to a mapped range from device `dev`
bool grant_access(char *base, size_t bytes, int dev)
{
    hipMemAccessDesc d;
    memset(&d, 0, sizeof(d));
    d.location.type = hipMemLocationTypeDevice;
    d.location.id = dev;
    d.flags = hipMemAccessFlagsProtReadWrite;
    const bool ok = hipMemSetAccess(base, bytes, &d, 1) == hipSuccess;
    (void) hipGetLastError();
    return ok;
}

// Unmap and release a heap's chunks.  The virtual range of a heap imported
// from another process stays reserved: on this ROCm (7.2) a range that held
// imported chunks and is freed and reserved again -- for a later heap of
// this process or a later import -- keeps reaching the OLD chunks from the
// GPU (every unmap / release / free call succeeds; reductions in the new
// heap read and write the old memory: test_heap_create_destroy_cycles_
// processes), so such a range is never handed back (address space only).
void unmap(Mapping &m)
{
    size_t off = 0;
    int bad = 0;
    for (size_t k = 0; k < m.nmapped; off += m.len[k], k++)
        bad += hipMemUnmap(m.base + off, m.len[k]) != hipSuccess;
    for (auto h : m.h) bad += hipMemRelease(h) != hipSuccess;
    const bool imported = m.pe >= 0 && m.device < 0;
    if (m.base && !imported) bad += hipMemAddressFree(m.base, m.bytes) != hipSuccess;
    DBG("heap unmap: PE %d's range %p (%zu B, %zu chunks): %d failed calls", m.pe,
        (void *) m.base, m.bytes, m.h.size(), bad);
    (void) hipGetLastError();
    m = Mapping();
}

// reserve one range and map `h` (lengths `len`) back to back into it,
// readable and writable from this process's device
bool map_chunks(Mapping &m, size_t align, int dev)
{
    void *va = nullptr;
    if (hipMemAddressReserve(&va, m.bytes, align, nullptr, 0) != hipSuccess) return false;
    m.base = (char *) va;
    size_t off = 0;
    for (size_t k = 0; k < m.h.size(); off += m.len[k], k++) {
        if (hipMemMap(m.base + off, m.len[k], 0, m.h[k], 0) != hipSuccess) return false;
        m.nmapped = k + 1;
    }
    return grant_access(m.base, m.bytes, dev);
}

size_t heap_chunk_bytes(size_t gran)
{
    static const size_t env = [] {  // read once
        const char *e = getenv("OSGPU_HEAP_CHUNK_BYTES");
        const size_t v = e ? strtoull(e, nullptr, 0) : 0;
        return v ? v : (size_t) 1 << 30;
    }();
    return (env + gran - 1) / gran * gran;
}

// One osgpu_heap_create call: what its steps share.  The steps run in the
// order they are written; each sets the error of what it found wrong.
struct Create {
    const char *where;
    const Coll c;
    const int dev;
    hipMemAllocationProp prop;
    size_t gran = 0, total = 0, chunk = 0;
    std::unique_ptr<Heap> H;       // unmapped again unless it is registered
    PsyncBoard<HeapMsg> board;
    bool ok = true;                // this member, so far
    bool nomem = false;            // this member's failure is a lack of device memory
    bool refused = false;          // every member refused the same way
    FdSet fds;                     // my chunks, exported
    FdServer server;               // hands them to the members in other processes
    int expected = 0;              // how many of those
    std::vector<HeapMsg> msg;      // everyone's layout
    std::vector<char *> base;      // everyone's range as mapped here

    Create(const char *where, const Coll &c, int dev, size_t bytes);
    Heap *agree_reuse(int *rseg);
    int register_kept(Heap *kept, int rseg, void **base_out);
    void create_own();
    void exchange_layouts();
    void grant_threads();
    bool import_member(int i);
    void import_members();
    int conclude(void **base_out);
};

Create::Create(const char *where_, const Coll &c_, int dev_, size_t bytes)
    : where(where_), c(c_), dev(dev_), prop(chunk_prop(dev_)), H(new Heap()), board(c_)
{
    if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) !=
            hipSuccess ||
        !gran) {
        (void) hipGetLastError();
        gran = (size_t) 2 << 20;
    }
    total = (bytes + gran - 1) / gran * gran;
    chunk = std::min(heap_chunk_bytes(gran), total);
    H->pe = c.me;
    for (int i = 0; i < c.PE_size; i++) H->members.push_back(c.pe_at(i));
}

// A kept heap of this member set at least this size, if every member has
// one from the same creation: register its first `total` bytes again
// instead of making a new one (the smallest that fits).  A kept heap
// never serves a LARGER request, and its HBM is not returned: a job
// holds, per member set, the sum of every heap size that exceeded all
// the set's earlier heaps (4, then 8, then 16 GiB keeps 28 GiB) -- make
// the largest heap first and later ones fit inside it.  The candidate
// must be THIS PE's: PE threads of one process share the pool.
// Returns the kept heap every member agreed on, or nullptr; *rseg: the
// registry segment, the same on every member.
Heap *Create::agree_reuse(int *rseg)
{
    Heap *cand = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_hmu);
        for (Heap *k : g_pool)
            if (k->pe == c.me && k->members == H->members && k->own.device == dev &&
                k->own.bytes >= total && (!cand || k->own.bytes < cand->own.bytes))
                cand = k;
    }
    board.mine().nonce = cand ? cand->key : 0;
    board.mine().seg = heap_free_segment(H->members);
    board.publish();
    bool reuse = cand != nullptr;
    *rseg = 0;
    for (const HeapMsg &m : board.read_all()) {
        reuse = reuse && m.nonce == board.mine().nonce;
        *rseg = std::max(*rseg, (int) m.seg);
    }
    board.close();  // every member has read every message of this phase
    return reuse ? cand : nullptr;
}

int Create::register_kept(Heap *kept, int rseg, void **base_out)
{
    {
        std::lock_guard<std::mutex> lk(g_hmu);
        g_pool.erase(std::find(g_pool.begin(), g_pool.end(), kept));
        kept->seg = rseg;
        g_heaps.push_back(kept);
    }
    for (int i = 0; i < c.PE_size; i++) {  // cannot fail: arguments checked above
        (void) osgpu_heap_register_segment(c.pe_at(i), rseg, kept->member_base[i],
                                           std::min(total, kept->member_bytes[i]));
        heap_set_remote(c.pe_at(i), rseg, kept->member_remote[i] != 0);
    }
    *base_out = kept->own.base;
    DBG("%s PE %d: kept heap %p of %zu B registered again for %zu B (segment %d)", where, c.me,
        (void *) kept->own.base, kept->own.bytes, total, rseg);
    return OSGPU_OK;
}

// my chunks: created, exported (fds) and mapped back to back (H->own)
void Create::create_own()
{
    H->own.pe = c.me;
    H->own.device = dev;
    H->own.bytes = total;
    H->own.len = chunk_lens(total, chunk);
    {  // more than the device has free cannot succeed: fail at once instead
       // of creating chunks until the HBM runs out
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && total > fr) {
            size_t kept = 0;
            {
                std::lock_guard<std::mutex> lk(g_hmu);
                for (Heap *k : g_pool)
                    if (k->own.device == dev) kept += k->own.bytes;
            }
            set_err("%s: out of device memory: %zu B requested, %zu B free on device %d "
                    "(%zu B held by destroyed heaps kept for reuse: a later heap of the same "
                    "member set up to their size reuses them; their HBM returns at exit)",
                    where, total, fr, dev, kept);
            ok = false;
            nomem = true;
        }
        (void) hipGetLastError();
    }
    for (size_t k = 0; ok && k < H->own.len.size(); k++) {
        hipMemGenericAllocationHandle_t h;
        if (hipMemCreate(&h, H->own.len[k], &prop, 0) != hipSuccess) {
            set_err("%s: out of device memory: hipMemCreate(%zu B) failed", where,
                    H->own.len[k]);
            (void) hipGetLastError();
            ok = false;
            nomem = true;
            break;
        }
        H->own.h.push_back(h);
        int fd = -1;
        if (hipMemExportToShareableHandle(&fd, h, hipMemHandleTypePosixFileDescriptor, 0) !=
                hipSuccess ||
            fd < 0) {
            set_err("%s: hipMemExportToShareableHandle failed", where);
            ok = false;
            break;
        }
        fds.add(&fd, 1);
    }
    DBG("%s PE %d: %zu chunks of %zu B created and exported (ok=%d)", where, c.me,
        H->own.len.size(), chunk, (int) ok);
    if (ok && !map_chunks(H->own, gran, dev)) {
        set_err("%s: mapping the heap failed", where);
        ok = false;
    }
    (void) hipGetLastError();
}

// Listen for the members in other processes, publish my layout and read
// everyone's.  Every member reads the same messages, so the two refusals
// give the same verdict on every member.
void Create::exchange_layouts()
{
    static std::atomic<long> nonce_ctr{0};
    const long nonce = ((long) time(nullptr) << 20) ^ (nonce_ctr.fetch_add(1) + 1);
    if (ok && !server.listen_on((long) getpid(), nonce)) {
        set_err("%s: unix socket: %s", where, strerror(errno));
        ok = false;
    }
    HeapMsg &mine = board.mine();
    mine.pid = (long) getpid();
    mine.nonce = nonce;
    mine.bytes = ok ? (long) total : -1;
    mine.chunk = (long) chunk;
    mine.raw_ptr = (long) (uintptr_t) H->own.base;
    mine.device = dev;
    mine.pci = pci_key(dev);
    // every heap of a member set gets its own registry segment: the lowest
    // one free for every member here, agreed as the maximum over members
    mine.seg = heap_free_segment(H->members);
    DBG("%s PE %d: own heap mapped at %p, listening (ok=%d)", where, c.me, (void *) H->own.base,
        (int) ok);
    board.publish();
    msg = board.read_all();
    std::vector<long> pids;
    bool shared = false;  // some process holds several PEs of the set
    for (const HeapMsg &m : msg) {
        if (m.bytes <= 0) ok = false;
        H->seg = std::max(H->seg, (int) m.seg);
        if (std::find(pids.begin(), pids.end(), m.pid) != pids.end()) shared = true;
        else pids.push_back(m.pid);
    }
    // the registry has room for the segment
    if (H->seg > kMaxHeapSegment) {
        set_err("%s: the heap registry is full (segment %d > %d): destroy heaps first", where,
                H->seg, kMaxHeapSegment);
        refused = true;
    }
    // no mixed topology: a process holding several PE threads AND members in
    // other processes would import each remote heap once per thread, into
    // ranges only that thread's device may access, and the process-global
    // registry would keep whichever thread wrote last (a GPU fault for the
    // others).  Threads only, or one PE per process.
    if (shared && pids.size() > 1) {
        set_err("%s: unsupported topology: %zu processes, some holding several PEs of the "
                "active set; use one PE per process, or PE threads of one process only",
                where, pids.size());
        refused = true;
    }
    if (refused) ok = false;
}

// members that are threads of this process on another GPU use my range
// directly: their devices need access to it too (only theirs -- a grant
// binds this process to that GPU, which one-process-per-GPU jobs never
// need); done before the status barrier, after which they use it
void Create::grant_threads()
{
    for (int i = 0; ok && i < c.PE_size; i++) {
        if (c.pe_at(i) == c.me || msg[i].pid != (long) getpid() || msg[i].device == dev) continue;
        if (!grant_access(H->own.base, H->own.bytes, (int) msg[i].device)) {
            set_err("%s: device %ld cannot access PE %d's heap", where, msg[i].device, c.me);
            ok = false;
        }
    }
}

// member i's heap (another process) into one range of this process
bool Create::import_member(int i)
{
    const int pe = c.pe_at(i);
    Mapping m;
    m.pe = pe;
    m.bytes = (size_t) msg[i].bytes;
    m.len = chunk_lens(m.bytes, (size_t) msg[i].chunk);
    size_t npf = 0;
    bool got;
    {
        FdClient peer(msg[i].pid, msg[i].nonce);
        FdSet pf;
        got = peer.connected();
        DBG("%s PE %d: connected to PE %d: %d", where, c.me, pe, (int) got);
        got = got && peer.receive(pf);
        npf = pf.size();
        DBG("%s PE %d: %zu descriptors from PE %d", where, c.me, npf, pe);
        got = got && npf == m.len.size();
        for (size_t k = 0; got && k < npf; k++) {
            hipMemGenericAllocationHandle_t h;
            // ROCm reads the descriptor through the pointer (CUDA takes the
            // value itself): passing the fd as an address faults
            int fd = pf.get()[k];
            if (hipMemImportFromShareableHandle(&h, &fd, hipMemHandleTypePosixFileDescriptor) !=
                hipSuccess) {
                set_err("%s: importing PE %d's heap chunk %zu failed", where, pe, k);
                got = false;
                break;
            }
            m.h.push_back(h);
            DBG("%s PE %d: imported chunk %zu of PE %d", where, c.me, k, pe);
        }
        pf.close_all();
        peer.ack();
    }
    if (got && !map_chunks(m, gran, dev)) {
        set_err("%s: mapping PE %d's heap failed", where, pe);
        got = false;
    }
    (void) hipGetLastError();
    if (!got) {
        if (npf != m.len.size())
            set_err("%s: %zu of %zu chunk descriptors from PE %d", where, npf, m.len.size(), pe);
        unmap(m);
        return false;
    }
    base[i] = m.base;
    DBG("%s PE %d: PE %d's heap mapped at %p", where, c.me, pe, (void *) m.base);
    H->peers.push_back(m);
    return true;
}

// Serve my descriptors to every member in another process until all of
// them have connected, or until every member has finished importing (the
// status barrier of conclude(): a member that failed may never connect), or
// a time bound passes; meanwhile import every member's heap (same process:
// its own range).
void Create::import_members()
{
    for (int i = 0; i < c.PE_size; i++)
        if (c.pe_at(i) != c.me && msg[i].pid != (long) getpid()) expected++;
    DBG("%s PE %d: layouts read, %d members in other processes", where, c.me, expected);
    if (server.listening() && expected > 0 && board.mine().bytes > 0) server.serve(fds, expected);
    base.assign(c.PE_size, nullptr);
    for (int i = 0; i < c.PE_size && ok; i++) {
        if (c.pe_at(i) == c.me) base[i] = H->own.base;
        else if (msg[i].pid == (long) getpid()) base[i] = (char *) (uintptr_t) msg[i].raw_ptr;
        else ok = import_member(i);
    }
}

// every member's verdict, then the registration; the heap's key
int Create::conclude(void **base_out)
{
    // after this barrier every member has finished importing, so no one
    // connects any more: the server can stop
    // 1 ok, 2 failed, 3 failed for lack of device memory
    const std::vector<long> st = board.post_status(&HeapMsg::status, ok ? 1 : (nomem ? 3 : 2));
    server.stop();
    fds.close_all();
    DBG("%s PE %d: served %d of %d, ok=%d", where, c.me, server.served(), expected, (int) ok);
    bool all_ok = true;
    int nomem_pe = nomem ? c.me : -1;
    for (int i = 0; i < c.PE_size; i++) {
        all_ok = all_ok && st[i] == 1;
        if (st[i] == 3 && nomem_pe < 0) nomem_pe = c.pe_at(i);
    }
    board.close();
    if (!all_ok) {
        if (refused) return OSGPU_EINVAL;  // every member refused the same way
        if (nomem_pe >= 0) {
            if (!nomem)
                set_err("%s: PE %d is out of device memory for its heap", where, nomem_pe);
            return OSGPU_ENOMEM;
        }
        if (ok) set_err("%s: another member failed to create or map its heap", where);
        return OSGPU_EPEER;
    }
    const int me_idx = c.index_of(c.me);
    unsigned long long key = 0x9e3779b97f4a7c15ull;  // the same on every member
    for (int i = 0; i < c.PE_size; i++) {
        // cannot fail: base and size checked, segment within the registry
        (void) osgpu_heap_register_segment(c.pe_at(i), H->seg, base[i], (size_t) msg[i].bytes);
        const bool remote = msg[i].pci != msg[me_idx].pci;
        heap_set_remote(c.pe_at(i), H->seg, remote);
        H->member_remote.push_back(remote ? 1 : 0);
        H->member_base.push_back(base[i]);
        H->member_bytes.push_back((size_t) msg[i].bytes);
        key = (key ^ (unsigned long long) msg[i].pid) * 0x100000001b3ull;
        key = (key ^ (unsigned long long) msg[i].nonce) * 0x100000001b3ull;
    }
    H->key = (long) (key | 1);  // never 0 (0 = "no kept heap")
    DBG("%s PE %d: heap %zu B at %p (%zu chunks), %d members", where, c.me, total,
        (void *) H->own.base, H->own.len.size(), c.PE_size);
    *base_out = H->own.base;
    std::lock_guard<std::mutex> lk(g_hmu);
    g_heaps.push_back(H.release());
    return OSGPU_OK;
}

}  // namespace

// Inside a heap made by osgpu_heap_create (the PE's own range or a member's
// mapped into this process)?  *dev: the local device backing it, -1 for a
// member's heap in another process.
bool heap_created_range(const void *p, size_t n, int *dev)
{
    std::lock_guard<std::mutex> lk(g_hmu);
    const char *c = (const char *) p;
    for (Heap *h : g_heaps) {
        if (c >= h->own.base && c + n <= h->own.base + h->own.bytes) {
            if (dev) *dev = h->own.device;
            return true;
        }
        for (const Mapping &m : h->peers)
            if (c >= m.base && c + n <= m.base + m.bytes) {
                if (dev) *dev = -1;
                return true;
            }
    }
    return false;
}

}  // namespace rt
}  // namespace osgpu

using namespace osgpu::rt;

extern "C" int osgpu_heap_create(size_t bytes, int PE_start, int logPE_stride, int PE_size,
                                 long *pSync, void **base_out)
{
    const char *where = "osgpu_heap_create";
    if (!bytes || !pSync || !base_out || PE_size < 1) {
        set_err("%s: bad arguments", where);
        return OSGPU_EINVAL;
    }
    Coll c = make_coll(where, PE_start, logPE_stride, PE_size, pSync);
    if (PE_size > 1 && !c.ops.getmem) {
        set_err("%s: the PE runtime has no shmem_getmem", where);
        return OSGPU_ENOPE;
    }
    if (c.index_of(c.me) < 0) {
        set_err("%s: PE %d is not in the active set", where, c.me);
        return OSGPU_EINVAL;
    }
    int dev = 0;
    HIPCHK(where, hipGetDevice(&dev));
    Create k(where, c, dev, bytes);
    int rseg = 0;
    Heap *kept = k.agree_reuse(&rseg);
    // every member computes the same rseg: the same verdict everywhere
    if (rseg > kMaxHeapSegment) {
        set_err("%s: the heap registry is full (segment %d > %d): destroy heaps first", where,
                rseg, kMaxHeapSegment);
        return OSGPU_ENOMEM;
    }
    if (kept) return k.register_kept(kept, rseg, base_out);
    k.create_own();
    k.exchange_layouts();
    k.grant_threads();
    k.import_members();
    return k.conclude(base_out);
}

extern "C" int osgpu_heap_destroy(void *base)
{
    std::unique_ptr<Heap> H;
    {
        std::lock_guard<std::mutex> lk(g_hmu);
        for (size_t i = 0; i < g_heaps.size(); i++)
            if (g_heaps[i]->own.base == (char *) base) {
                H.reset(g_heaps[i]);
                g_heaps.erase(g_heaps.begin() + (long) i);
                break;
            }
    }
    if (!H) {
        set_err("osgpu_heap_destroy: %p is not a heap made by osgpu_heap_create", base);
        return OSGPU_EINVAL;
    }
    (void) hipDeviceSynchronize();
    // forget the registrations that point into these ranges
    for (int pe : H->members) heap_clear_segment(pe, H->seg);
    if (!H->peers.empty()) {  // holds imported chunks: kept for a later heap
        std::lock_guard<std::mutex> lk(g_hmu);
        g_pool.push_back(H.release());
    }
    return OSGPU_OK;  // (a heap of this process alone is unmapped here)
}

// ---------------------------------------------------------------------
// osgpu_preflight: prove every cross-process mapping of a job before its
// first collective touches it.  A mapping that is wrong (an import that
// failed silently, a peer range this GPU may not access, staging opened on
// the wrong allocation) otherwise first shows up as a GPU fault inside a
// team kernel, with no hint of which peer or chunk.  Each member writes a
// pattern that names (PE, region, chunk, end) into 64 B at both ends of
//   * every chunk of its heap made by osgpu_heap_create (if heap_base),
//   * its STAGED staging area of this active set (if the runtime has
//     shmem_getmem; the staging set is made here when it does not exist),
//   * word 31 (unused by the protocol) of its device-barrier flag area
//     (members in distinct processes only),
// then every member reads every peer's patterns through ITS OWN mapping:
// first with a host copy (hipMemcpy), then -- only where that matched --
// with the copy kernel (copy.hip, the code path of the collectives).
//
// Then the other direction, the one the team kernel (its stores of shard g
// into every member's target, team.hip) and the push form (its scatter into
// the members' staging inboxes) use: remote WRITES into 128 B at both ends
// of every heap chunk and of the staging area, 16 B per writer (its
// active-set index).  The owner first reads its blocks with plain cached
// loads, so the lines sit in its L2; every peer then writes its piece
// through its mapping -- by host copy, and in a second round by the copy
// kernel -- and after a barrier the owner re-reads the blocks by kernel and
// checks every writer's piece.  This is the reference's guarantee that a
// PE's remote puts are complete and visible at its target before the
// barrier returns (shmemc_quiet -> ucp_worker_flush ahead of the barrier,
// src/shmemc/comms.c:147-161, src/shmemc/barrier.c:176-181).
//
// Test hook: osgpu_test_preflight_fault(pe, peer) makes PE <pe> reach peer
// <peer>'s heap chunks and staging through ANOTHER member's mappings (a
// planted wrong mapping), which both legs must report.
// ---------------------------------------------------------------------

namespace {

void pattern(unsigned long long *w, size_t words, int pe, int region, int chunk, int end)
{
    unsigned long long x = 0x243f6a8885a308d3ull ^ ((unsigned long long) pe << 40) ^
                           ((unsigned long long) region << 32) ^
                           ((unsigned long long) chunk << 8) ^ (unsigned long long) end;
    for (size_t j = 0; j < words; j++) {  // splitmix64
        x += 0x9e3779b97f4a7c15ull;
        unsigned long long z = x;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        w[j] = z ^ (z >> 31);
    }
}

int region_code(const char *r) { return r[0] == 'h' ? 1 : r[0] == 's' ? 2 : 3; }

// the remote-write leg's 16-B piece of `writer` in owner's block
void wpattern(unsigned long long *w, int writer, int owner, int region, int chunk, int end,
              int leg)
{
    pattern(w, 2, writer, region + 8 * leg, (chunk << 12) ^ owner, end);
}

// planted by osgpu_test_preflight_fault (test hook; never from the
// environment, so a stray variable cannot redirect real remote writes)
std::atomic<int> g_fault_pe{-1}, g_fault_peer{-1};

// the active-set index whose mappings PE `me` uses for member index i
int probe_view(const Coll &c, int me, int i)
{
    const int fpe = g_fault_pe.load(), fpeer = g_fault_peer.load();
    if (fpe < 0 || fpe != c.me || fpeer != c.pe_at(i)) return i;
    for (int j = 0; j < c.PE_size; j++)
        if (j != i && j != me) return j;
    return me;  // two members: my own range stands in for the peer's
}

// chunk layout of the heap whose own range starts at `base` (this process)
bool own_chunks(const char *base, std::vector<size_t> *len)
{
    std::lock_guard<std::mutex> lk(g_hmu);
    for (Heap *h : g_heaps)
        if (h->own.base == base) {
            *len = h->own.len;
            return true;
        }
    return false;
}

struct Block {                // one block to check in a member's memory
    const char *region;       // "heap" / "staging" / "flags"
    int chunk;                // chunk index (heap), 0 otherwise
    int end;                  // 0 low end, 1 high end
    char *at;                 // the block as mapped in this process
    size_t bytes;             // the caller's block size, or 8 for the flag word
};

struct Preflight {            // one osgpu_preflight call: what its steps share
    const char *where;
    Coll c;
    int me;                   // my active-set index
    Heap *H;                  // the heap to check, the staging set, the flag areas:
    StageSet *S;              // each nullptr when the job has none
    SyncSet *Y;
    hipStream_t st;
    std::vector<PeerReport> rep;  // by active-set index
    int nprobes = 0, nbad = 0, nwrite = 0, nwbad = 0;
};

// The blocks of member i as this process reaches them (a peer's through the
// view probe_view() names: its own unless a fault is planted): `each` bytes
// at both ends of every heap chunk and of the staging area and, with
// `flags`, word 31 of the flag area.
std::vector<Block> blocks_of(const Preflight &p, int i, size_t each, bool flags)
{
    const int v = i == p.me ? i : probe_view(p.c, p.me, i);
    std::vector<Block> b;
    if (p.H) {
        std::vector<size_t> len;  // chunk layout of member i's heap
        if (i == p.me) len = p.H->own.len;
        for (const Mapping &m : p.H->peers)
            if (m.pe == p.c.pe_at(i)) len = m.len;
        if (len.empty()) (void) own_chunks(p.H->member_base[i], &len);  // a PE thread here
        char *at = p.H->member_base[v];
        for (size_t k = 0; k < len.size(); at += len[k], k++) {
            b.push_back({"heap", (int) k, 0, at, each});
            b.push_back({"heap", (int) k, 1, at + len[k] - each, each});
        }
    }
    if (p.S) {
        b.push_back({"staging", 0, 0, p.S->region(v), each});
        b.push_back({"staging", 0, 1, p.S->region(v) + 4 * p.S->slot - each, each});
    }
    if (flags && p.Y) b.push_back({"flags", 0, 0, (char *) (p.Y->peer[i] + 31), 8});
    return b;
}

// 1. my patterns, in place when this returns
bool write_patterns(const Preflight &p)
{
    bool wrote = true;
    for (const Block &b : blocks_of(p, p.me, 64, true)) {
        unsigned long long w[8];
        pattern(w, b.bytes / 8, p.c.me, region_code(b.region), b.chunk, b.end);
        wrote = hipMemcpy(b.at, w, b.bytes, hipMemcpyHostToDevice) == hipSuccess && wrote;
    }
    (void) hipDeviceSynchronize();
    (void) hipGetLastError();
    return wrote;
}

// 2. the peers' patterns through my mappings: by host copy, then -- only
// where that matched -- by the copy kernel
void read_leg(Preflight &p)
{
    constexpr size_t B = 64;
    char *dtmp = nullptr;
    const bool have_tmp = hipMalloc((void **) &dtmp, B) == hipSuccess;
    (void) hipGetLastError();
    for (int i = 0; i < p.c.PE_size; i++) {
        if (i == p.me) continue;
        for (const Block &b : blocks_of(p, i, B, true)) {
            p.nprobes++;
            p.rep[i].chunks += b.end == 0 && !strcmp(b.region, "heap");
            unsigned long long want[B / 8], got[B / 8];
            pattern(want, b.bytes / 8, p.c.pe_at(i), region_code(b.region), b.chunk, b.end);
            const char *what = nullptr;
            hipError_t e = hipMemcpy(got, b.at, b.bytes, hipMemcpyDeviceToHost);
            if (e != hipSuccess) what = "host copy failed";
            else if (memcmp(got, want, b.bytes)) what = "host copy read other data";
            (void) hipGetLastError();
            if (!what) {  // the copy kernel through the same mapping
                osgpu::CopySeg seg = {b.at, dtmp, b.bytes};
                e = have_tmp ? osgpu::launch_copy(&seg, 1, p.st) : hipErrorOutOfMemory;
                if (e == hipSuccess) e = hipStreamSynchronize(p.st);
                if (e == hipSuccess) e = hipMemcpy(got, dtmp, b.bytes, hipMemcpyDeviceToHost);
                if (e != hipSuccess) what = "copy kernel failed";
                else if (memcmp(got, want, b.bytes)) what = "copy kernel read other data";
                (void) hipGetLastError();
            }
            if (what) {
                p.nbad++;
                note_block(p.rep[i].read, b.region, b.chunk, b.end, what);
            }
        }
    }
    if (have_tmp) (void) hipFree(dtmp);
}

// the owner's view of a block of its own (WB bytes), read by kernel with
// cached loads, in pieces of at most kProbeLoadBytes (one probe workgroup: a
// block of a set of more than 128 members is larger)
bool owner_read(const Preflight &p, const Block &b, char *wtmp, unsigned long long *got)
{
    hipError_t e = wtmp ? hipSuccess : hipErrorOutOfMemory;
    for (size_t o = 0; e == hipSuccess && o < b.bytes; o += osgpu::kProbeLoadBytes)
        e = osgpu::launch_probe_load(b.at + o, wtmp + o,
                                     std::min(b.bytes - o, (size_t) osgpu::kProbeLoadBytes), p.st);
    if (e == hipSuccess) e = hipStreamSynchronize(p.st);
    if (e == hipSuccess) e = hipMemcpy(got, wtmp, b.bytes, hipMemcpyDeviceToHost);
    (void) hipGetLastError();
    return e == hipSuccess;
}

// 3b. my 16-B piece into every peer's blocks through my mappings: by host
// copy (leg 1) or by the copy kernel's 16-B vector store (leg 2, from `src`)
void write_pieces(Preflight &p, size_t WB, int leg, char *src)
{
    for (int i = 0; i < p.c.PE_size; i++) {
        if (i == p.me) continue;
        for (const Block &b : blocks_of(p, i, WB, false)) {
            p.nwrite++;
            unsigned long long w[2];
            wpattern(w, p.c.me, p.c.pe_at(i), region_code(b.region), b.chunk, b.end, leg);
            char *at = b.at + 16 * p.me;
            hipError_t e;
            if (leg == 1) {
                e = hipMemcpy(at, w, 16, hipMemcpyHostToDevice);
            } else {
                e = src ? hipMemcpy(src, w, 16, hipMemcpyHostToDevice) : hipErrorOutOfMemory;
                osgpu::CopySeg seg = {src, at, 16};
                if (e == hipSuccess) e = osgpu::launch_copy(&seg, 1, p.st);
                if (e == hipSuccess) e = hipStreamSynchronize(p.st);
            }
            (void) hipGetLastError();
            if (e != hipSuccess) {
                p.nwbad++;
                note_block(p.rep[i].write, b.region, b.chunk, b.end,
                           leg == 1 ? "host-copy write to the peer failed"
                                    : "copy-kernel write to the peer failed");
            }
        }
    }
    (void) hipDeviceSynchronize();
    (void) hipGetLastError();
}

// 3. remote writes: 16 B per writer in 128-B blocks at both ends of every
// heap chunk and of the staging area (what team.hip's stores into the
// members' targets and the push form's inbox scatter do)
void write_leg(Preflight &p)
{
    if (!p.H && !p.S) return;
    // 16 B per member, whole 128-B lines: sized by the active set, which may
    // exceed the team kernel's kMaxTeam (staging and PE threads allow more)
    const size_t WB = ((size_t) 16 * p.c.PE_size + 127) / 128 * 128;
    const std::vector<Block> mine = blocks_of(p, p.me, WB, false);
    char *wtmp = nullptr;  // my block as the kernel read it; behind it, leg 2's piece
    if (hipMalloc((void **) &wtmp, WB * 2) != hipSuccess) wtmp = nullptr;
    (void) hipGetLastError();
    std::vector<unsigned long long> got(WB / 8);
    // 3a. clear my blocks and pull them into my L2
    for (const Block &b : mine) {
        (void) hipMemset(b.at, 0, WB);
        (void) hipDeviceSynchronize();
        (void) owner_read(p, b, wtmp, got.data());
    }
    (void) hipGetLastError();
    barrier(p.c);
    for (int leg = 1; leg <= 2; leg++) {
        write_pieces(p, WB, leg, wtmp ? wtmp + WB : nullptr);
        barrier(p.c);  // every writer's stores are complete
        // 3c. every writer's piece in my blocks, read by kernel
        for (const Block &b : mine) {
            const bool ok = owner_read(p, b, wtmp, got.data());
            for (int j = 0; j < p.c.PE_size; j++) {
                if (j == p.me) continue;
                unsigned long long want[2];
                wpattern(want, p.c.pe_at(j), p.c.me, region_code(b.region), b.chunk, b.end, leg);
                if (ok && !memcmp(got.data() + 2 * j, want, 16)) continue;
                p.nwbad++;
                note_block(p.rep[j].write, b.region, b.chunk, b.end,
                           !ok ? "owner's read kernel failed"
                               : leg == 1 ? "its host-copy write not seen by the owner"
                                          : "its copy-kernel write not seen by the owner");
            }
        }
        barrier(p.c);  // the owners have read this round before the next one writes
    }
    if (wtmp) (void) hipFree(wtmp);
}

}  // namespace

extern "C" int osgpu_preflight(void *heap_base, int PE_start, int logPE_stride, int PE_size,
                               long *pSync, char *report, size_t report_bytes)
{
    const char *where = "osgpu_preflight";
    if (!pSync || PE_size < 1 || (report && !report_bytes)) {
        set_err("%s: bad arguments", where);
        return OSGPU_EINVAL;
    }
    Coll c = make_coll(where, PE_start, logPE_stride, PE_size, pSync);
    const int me = c.index_of(c.me);
    if (me < 0) {
        set_err("%s: PE %d is not in the active set", where, c.me);
        return OSGPU_EINVAL;
    }
    Heap *H = nullptr;
    if (heap_base) {
        std::lock_guard<std::mutex> lk(g_hmu);
        for (Heap *h : g_heaps)
            if (h->own.base == (char *) heap_base) H = h;
    }
    bool same_set = H && H->members.size() == (size_t) PE_size;
    for (int i = 0; same_set && i < PE_size; i++) same_set = H->members[i] == c.pe_at(i);
    if (heap_base && !same_set) {
        set_err("%s: %p is not a heap of this active set made by osgpu_heap_create", where,
                heap_base);
        return OSGPU_EINVAL;  // the same on every member given the same arguments
    }
    // collective setups (same decision on every member)
    StageSet *S = (PE_size > 1 && c.ops.getmem) ? stage_setup(c) : nullptr;
    // flag areas exist only when every member is its own process
    SyncSet *Y = (PE_size > 1 && c.ops.getmem) ? sync_setup(c) : nullptr;
    Preflight p = {where, c, me, H, S, Y, nullptr, std::vector<PeerReport>(PE_size)};
    for (int i = 0; i < PE_size; i++) p.rep[i].pe = c.pe_at(i);

    const bool wrote = write_patterns(p);
    barrier(c);  // every member's patterns are in place
    p.st = thread_stream(where);
    read_leg(p);
    barrier(c);  // nobody reuses the regions before every member has read them
    write_leg(p);

    p.rep.erase(p.rep.begin() + me);  // the peers
    bool all = wrote;
    for (const PeerReport &r : p.rep) all = all && r.read.empty() && r.write.empty();
    const std::string rep = preflight_report(p.rep, S != nullptr, Y != nullptr);
    DBG("%s PE %d: %d probes, %d bad; %d remote writes, %d bad", where, c.me, p.nprobes, p.nbad,
        p.nwrite, p.nwbad);
    if (report) {
        if (rep.size() + 1 > report_bytes) {
            set_err("%s: the report needs %zu bytes", where, rep.size() + 1);
            snprintf(report, report_bytes, "%s", "{}");
            return OSGPU_EINVAL;
        }
        memcpy(report, rep.c_str(), rep.size() + 1);
    }
    if (!wrote) set_err("%s: writing this PE's patterns failed", where);
    else if (!all)
        set_err("%s: %d of %d read probes and %d remote-write checks failed", where, p.nbad,
                p.nprobes, p.nwbad);
    return all ? OSGPU_OK : OSGPU_EPEER;
}

// Test hooks (tests/support/mp_worker.py).  Not in the public header
// (tests/support/osgpu_test_hooks.h) and refused unless the process runs with
// OSGPU_TEST_HOOKS=1: a production caller can never redirect preflight
// writes by accident.
static bool test_hooks_on(const char *hook)
{
    const char *on = getenv("OSGPU_TEST_HOOKS");
    if (on && !strcmp(on, "1")) return true;
    set_err("%s: test hooks are off (OSGPU_TEST_HOOKS=1 enables them)", hook);
    return false;
}

// Launch-size limit for the one-tile-per-workgroup kernels
// (combine.hpp kMaxLaunchThreads): a smaller limit runs their multi-launch
// path at small sizes.  n <= 0 restores the default.
extern "C" int osgpu_test_max_launch_threads(long long n)
{
    if (!test_hooks_on("osgpu_test_max_launch_threads")) return OSGPU_EINVAL;
    const size_t lim = n <= 0 || (size_t) n > osgpu::kMaxLaunchThreads ? osgpu::kMaxLaunchThreads
                                                                       : (size_t) n;
    osgpu::set_max_launch_threads(lim);
    if (lim != osgpu::kMaxLaunchThreads)
        fprintf(stderr, "[osgpu] test hook: at most %zu threads per kernel launch\n", lim);
    return OSGPU_OK;
}

// Plant a wrong mapping for the next osgpu_preflight calls of this process
// -- PE `pe` reaches peer `peer` through another member's ranges.  (-1, -1)
// clears it.  Logged, so a planted fault never goes unseen.
extern "C" int osgpu_test_preflight_fault(int pe, int peer)
{
    if (!test_hooks_on("osgpu_test_preflight_fault")) return OSGPU_EINVAL;
    if ((pe < 0) != (peer < 0)) return OSGPU_EINVAL;
    g_fault_pe.store(-1);
    g_fault_peer.store(peer);
    g_fault_pe.store(pe);
    if (pe >= 0)
        fprintf(stderr, "[osgpu] test hook: preflight of PE %d reaches PE %d through another "
                        "member's mappings\n", pe, peer);
    return OSGPU_OK;
}
