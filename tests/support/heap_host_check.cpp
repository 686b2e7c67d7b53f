// heap_host_check.cpp -- TEST INFRASTRUCTURE: the HIP-free parts of the job
// setup (csrc/psync_board.hpp, fd_channel.cpp, heap_host.hpp) driven on the
// CPU.  Threads stand in for PEs behind a barrier-and-getmem stub.
//   heap_host_check <case>     exit 0 and "ok", or 1 and what failed
// Built by host_check_build.py, plain and with ASan + UBSan; run by
// tests/test_heap_host.py.
#include <dirent.h>
#include <sys/mman.h>
#include <sys/socket.h>
#include <sys/stat.h>

#include <chrono>
#include <condition_variable>
#include <mutex>
#include <stdexcept>
#include <string>

#include "../../test-resilient-osss-ucx_amd/csrc/fd_channel.hpp"
#include "../../test-resilient-osss-ucx_amd/csrc/heap_host.hpp"
#include "../../test-resilient-osss-ucx_amd/csrc/psync_board.hpp"

using namespace osgpu::rt;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) throw std::runtime_error(std::string(#cond) + " (line " +           \
                                              std::to_string(__LINE__) + ")");           \
    } while (0)

// ------------------------------------------------- what the library provides

namespace osgpu {
namespace rt {
int debug_level() { return 0; }
void barrier(const Coll &c) { c.ops.barrier(c.PE_start, c.logPE_stride, c.PE_size, c.pSync); }
}  // namespace rt
}  // namespace osgpu

// ------------------------------------------------------------------- the stub

namespace {

constexpr int kPes = 10, kWords = 64;
constexpr long kSentinel = 0x5a5a5a5a5a5a5a5aL;
long g_psync[kPes][kWords];  // symmetric: the same words on every PE
thread_local int t_pe = -1;
thread_local int t_barriers = 0;

std::mutex g_mu;
std::condition_variable g_cv;
int g_waiting = 0;
long g_generation = 0;

void stub_barrier(int, int, int PE_size, long *)
{
    t_barriers++;
    std::unique_lock<std::mutex> lk(g_mu);
    const long gen = g_generation;
    if (++g_waiting == PE_size) {
        g_waiting = 0;
        g_generation++;
        g_cv.notify_all();
    } else {
        g_cv.wait(lk, [&] { return g_generation != gen; });
    }
}

void stub_getmem(void *dst, const void *src, size_t n, int pe)
{
    const size_t off = (size_t) ((const char *) src - (const char *) g_psync[t_pe]);
    if (pe < 0 || pe >= kPes || off + n > sizeof(g_psync[0])) abort();
    memcpy(dst, (const char *) g_psync[pe] + off, n);
}

int stub_my_pe() { return t_pe; }

// ------------------------------------------------------------------ the board

struct Big {  // the largest message that fits at word 16
    long w[47];
    long status;
};
static_assert(sizeof(Big) == (kWords - 16) * sizeof(long), "fills pSync[16..63]");

long word_of(int pe, int round, int k) { return ((long) pe << 40) ^ ((long) round << 20) ^ (k + 1); }

void check_psync(int pe)  // the protocol's own words untouched, the spare ones zero
{
    for (int k = 0; k < 16; k++) CHECK(g_psync[pe][k] == kSentinel);
    for (int k = 16; k < kWords; k++) CHECK(g_psync[pe][k] == 0);
}

void fill(Big &m, int pe, int round)
{
    for (int k = 0; k < 47; k++) m.w[k] = word_of(pe, round, k);
}

// every member's exact payload; the status word belongs to the status phase
// (a member that has read everything may post before the others have read)
void check_all(const Coll &c, const std::vector<Big> &all, int round)
{
    CHECK((int) all.size() == c.PE_size);
    for (int i = 0; i < c.PE_size; i++) {
        Big want;
        fill(want, c.pe_at(i), round);
        CHECK(!memcmp(all[i].w, want.w, sizeof(want.w)));
    }
}

void board_pe(int pe, int PE_start, int logPE_stride, int PE_size, std::string *err)
{
    t_pe = pe;
    Coll c;
    c.name = "heap_host_check";
    c.PE_start = PE_start;
    c.logPE_stride = logPE_stride;
    c.PE_size = PE_size;
    c.step = 1 << logPE_stride;
    c.pSync = g_psync[pe];
    c.me = pe;
    c.ops.my_pe = stub_my_pe;
    c.ops.barrier = stub_barrier;
    c.ops.getmem = stub_getmem;
    try {
        for (int round = 0; round < 100; round++) {
            PsyncBoard<Big> b(c);
            // without the status phase: osgpu_heap_create's reuse round (2 barriers)
            int before = t_barriers;
            fill(b.mine(), pe, 2 * round);
            b.publish();
            check_all(c, b.read_all(), 2 * round);
            b.close();
            CHECK(t_barriers - before == 2);
            check_psync(pe);
            // with it: map_members (3 barriers); a fresh heap takes both (5)
            fill(b.mine(), pe, 2 * round + 1);
            b.publish();
            check_all(c, b.read_all(), 2 * round + 1);
            const int failing = round % 3 == 0 ? round % PE_size : -1;  // a set index
            const std::vector<long> st =
                b.post_status(&Big::status, c.index_of(pe) == failing ? 2 : 1);
            CHECK((int) st.size() == PE_size);
            bool all_ok = true;
            for (int i = 0; i < PE_size; i++) {
                CHECK(st[i] == (i == failing ? 2 : 1));
                all_ok = all_ok && st[i] == 1;
            }
            CHECK(all_ok == (failing < 0));
            b.close();
            CHECK(t_barriers - before == 5);
            check_psync(pe);
        }
        {  // a round abandoned before close, by return and by exception
            PsyncBoard<Big> b(c);
            fill(b.mine(), pe, 1000);
            b.publish();
            check_all(c, b.read_all(), 1000);
            stub_barrier(0, 0, PE_size, nullptr);  // (the test's: nobody still reads)
        }
        check_psync(pe);
        try {
            PsyncBoard<Big> b(c);
            fill(b.mine(), pe, 1001);
            b.publish();
            stub_barrier(0, 0, PE_size, nullptr);
            throw 1;
        } catch (int) {
        }
        check_psync(pe);
    } catch (const std::exception &e) {
        *err = "PE " + std::to_string(pe) + ": " + e.what();
        // a failed PE would leave the others in a barrier for good
        fprintf(stderr, "%s\n", err->c_str());
        _exit(1);
    }
}

void board(int PE_start, int logPE_stride, int PE_size)
{
    for (auto &p : g_psync)
        for (int k = 0; k < kWords; k++) p[k] = k < 16 ? kSentinel : 0;
    std::vector<std::thread> th;
    std::vector<std::string> err(PE_size);
    for (int i = 0; i < PE_size; i++)
        th.emplace_back(board_pe, PE_start + (i << logPE_stride), PE_start, logPE_stride, PE_size,
                        &err[i]);
    for (auto &t : th) t.join();
}

// ---------------------------------------------------------------- the channel

size_t open_fds()
{
    size_t n = 0;
    DIR *d = opendir("/proc/self/fd");
    CHECK(d);
    while (readdir(d)) n++;
    closedir(d);
    return n;
}

void make_files(FdSet &fds, int n)
{
    for (int k = 0; k < n; k++) {
        const int fd = memfd_create("heap_host_check", MFD_CLOEXEC);
        CHECK(fd >= 0);
        fds.add(&fd, 1);
    }
}

void same_files(const FdSet &a, const FdSet &b, size_t n)
{
    CHECK(a.size() >= n && b.size() == n);
    for (size_t k = 0; k < n; k++) {
        struct stat sa, sb;
        CHECK(fstat(a.get()[k], &sa) == 0 && fstat(b.get()[k], &sb) == 0);
        CHECK(a.get()[k] != b.get()[k] && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino);
    }
}

double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

void transfer(int n)
{
    const size_t before = open_fds();
    {
        FdSet src, got;
        make_files(src, n);
        FdServer srv;
        CHECK(srv.listen_on((long) getpid(), 7000 + n));
        srv.serve(src, 1);
        FdClient cl((long) getpid(), 7000 + n);
        CHECK(cl.connected());
        CHECK(cl.receive(got));
        same_files(src, got, (size_t) n);
        cl.ack();
        srv.stop();
        CHECK(srv.served() == 1);
    }
    CHECK(open_fds() == before);
}

void idle_server()  // nobody connects: stop() ends it within a few poll intervals
{
    FdSet src;
    make_files(src, 1);
    FdServer srv;
    CHECK(srv.listen_on((long) getpid(), 7500));
    srv.serve(src, 2);
    const auto t0 = std::chrono::steady_clock::now();
    srv.stop();
    CHECK(seconds_since(t0) < 0.5);
    CHECK(srv.served() == 0 && !srv.listening());
}

void no_server()  // nobody listens: the client fails at once
{
    const auto t0 = std::chrono::steady_clock::now();
    FdClient cl((long) getpid(), 7600);
    FdSet got;
    CHECK(!cl.connected() && !cl.receive(got) && got.size() == 0);
    CHECK(seconds_since(t0) < 0.5);
}

void truncated()  // the sender announces 129 and closes after the first batch
{
    const size_t before = open_fds();
    {
        FdSet src, got;
        make_files(src, 129);
        int sv[2];
        CHECK(socketpair(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0, sv) == 0);
        const unsigned long long n = 129;
        CHECK(write_all(sv[0], &n, sizeof(n)));
        CHECK(send_fd_batch(sv[0], src.get().data(), kFdBatch));
        close(sv[0]);
        CHECK(!recv_fds(sv[1], got));
        same_files(src, got, kFdBatch);
        close(sv[1]);
    }
    CHECK(open_fds() == before);
}

// ------------------------------------------------------- layout and the report

void chunks()
{
    const size_t gran = (size_t) 2 << 20, chunk = (size_t) 1 << 30;
    const size_t totals[] = {3 * chunk, 3 * chunk + gran, chunk - gran};
    const size_t counts[] = {3, 4, 1};
    for (int t = 0; t < 3; t++) {
        const std::vector<size_t> v = chunk_lens(totals[t], chunk);
        CHECK(v.size() == counts[t]);
        size_t sum = 0;
        for (size_t k = 0; k < v.size(); k++) {
            sum += v[k];
            CHECK(k + 1 == v.size() || v[k] == chunk);
        }
        CHECK(sum == totals[t] && v.back() > 0 && v.back() <= chunk);
    }
}

void report()  // PE 0's view of a 3-member job
{
    std::vector<PeerReport> peers(2);
    peers[0].pe = 1;
    peers[1].pe = 2;
    peers[0].chunks = peers[1].chunks = 2;
    note_block(peers[0].read, "heap", 1, 1, "host copy read other data");
    note_block(peers[1].write, "staging", 0, 0, "its copy-kernel write not seen by the owner");
    const char *want =
        "{\"1\": {\"chunks\": 2, \"staging\": true, \"flags\": false, "
        "\"status\": \"heap chunk 1 high: host copy read other data\", \"remote_write\": \"ok\"}, "
        "\"2\": {\"chunks\": 2, \"staging\": true, \"flags\": false, \"status\": \"ok\", "
        "\"remote_write\": \"staging 0 low: its copy-kernel write not seen by the owner\"}}";
    CHECK(preflight_report(peers, true, false) == want);
    note_block(peers[0].read, "flags", 0, 0, "copy kernel failed");
    CHECK(peers[0].read == "heap chunk 1 high: host copy read other data; "
                           "flags 0 low: copy kernel failed");
    CHECK(preflight_report({}, false, true) == "{}");
}

}  // namespace

int main(int argc, char **argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    try {
        if (what == "board1") board(0, 0, 1);
        else if (what == "board2") board(0, 0, 2);
        else if (what == "board5") board(1, 1, 5);
        else if (what == "fds1") transfer(1);
        else if (what == "fds64") transfer(64);
        else if (what == "fds65") transfer(65);
        else if (what == "fds129") transfer(129);
        else if (what == "idle_server") idle_server();
        else if (what == "no_server") no_server();
        else if (what == "truncated") truncated();
        else if (what == "chunks") chunks();
        else if (what == "report") report();
        else throw std::runtime_error("unknown case '" + what + "'");
    } catch (const std::exception &e) {
        fprintf(stderr, "heap_host_check %s: %s\n", what.c_str(), e.what());
        return 1;
    }
    printf("ok\n");
    return 0;
}
