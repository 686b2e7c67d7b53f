// fd_channel.hpp -- file descriptors from one process of a job to the others
// over a Unix-domain socket (SCM_RIGHTS): how osgpu_heap_create hands the
// dmabuf descriptors of a PE's heap chunks to the members in other
// processes.  The socket's name is (pid, nonce) in the abstract namespace.
// HIP-free (fd_channel.cpp).
#pragma once
#include <unistd.h>

#include <atomic>
#include <thread>
#include <vector>

namespace osgpu {
namespace rt {

constexpr int kFdBatch = 64;  // descriptors per SCM_RIGHTS message
constexpr int kSetupTimeoutMs = 120000;

// descriptors this process must close: exported ones, or received copies
class FdSet {
public:
    FdSet() = default;
    ~FdSet() { close_all(); }
    FdSet(const FdSet &) = delete;
    FdSet &operator=(const FdSet &) = delete;
    void add(const int *fd, size_t n) { fds_.insert(fds_.end(), fd, fd + n); }
    void close_all();
    const std::vector<int> &get() const { return fds_; }
    size_t size() const { return fds_.size(); }

private:
    std::vector<int> fds_;
};

bool write_all(int fd, const void *p, size_t n);
bool read_all(int fd, void *p, size_t n);
// a count, then the descriptors in batches of kFdBatch, each batch riding on
// one byte; recv_fds appends what arrived to `fds`, also when it fails
bool send_fd_batch(int s, const int *fds, int m);
bool send_fds(int s, const std::vector<int> &fds);
bool recv_fds(int s, FdSet &fds);

// Serves one descriptor set to `expected` clients from a thread of its own,
// one at a time, each until its one-byte acknowledgement (the client has its
// copies), until stop() or kSetupTimeoutMs of waiting.
class FdServer {
public:
    ~FdServer() { stop(); }
    // bind and listen; false with errno set
    bool listen_on(long pid, long nonce);
    bool listening() const { return lfd_ >= 0; }
    // `fds` outlives the server or its stop()
    void serve(const FdSet &fds, int expected);
    // no client connects any more: join the thread, close the socket
    void stop();
    int served() const { return served_.load(); }

private:
    int lfd_ = -1;
    std::thread thread_;
    std::atomic<bool> stop_{false};
    std::atomic<int> served_{0};
};

// The client side: connects at construction, with kSetupTimeoutMs send and
// receive timeouts (a member that stopped serving must not hang this one).
class FdClient {
public:
    FdClient(long pid, long nonce);
    ~FdClient() { if (s_ >= 0) close(s_); }
    bool connected() const { return connected_; }
    bool receive(FdSet &fds) { return connected_ && recv_fds(s_, fds); }
    // the descriptors are used up: the server may go on
    void ack();

private:
    int s_ = -1;
    bool connected_ = false;
};

}  // namespace rt
}  // namespace osgpu
