// fd_channel.cpp -- see fd_channel.hpp
#include "fd_channel.hpp"

#include <errno.h>
#include <poll.h>
#include <string.h>
#include <sys/socket.h>
#include <sys/un.h>

#include <algorithm>

#include "coll.hpp"

namespace osgpu {
namespace rt {

namespace {

void sock_name(long pid, long nonce, sockaddr_un *a, socklen_t *len)
{
    memset(a, 0, sizeof(*a));
    a->sun_family = AF_UNIX;
    // abstract namespace: nothing on the file system to clean up
    const int n = snprintf(a->sun_path + 1, sizeof(a->sun_path) - 1, "osgpu-heap-%ld-%ld", pid,
                           nonce);
    *len = (socklen_t) (offsetof(sockaddr_un, sun_path) + 1 + n);
}

// one byte at `byte` with room for m descriptors of control data in `ctl`
msghdr fd_msg(iovec *iov, char *byte, std::vector<char> &ctl, int m)
{
    *iov = {byte, 1};
    ctl.assign(CMSG_SPACE(sizeof(int) * m), 0);
    msghdr msg;
    memset(&msg, 0, sizeof(msg));
    msg.msg_iov = iov;
    msg.msg_iovlen = 1;
    msg.msg_control = ctl.data();
    msg.msg_controllen = ctl.size();
    return msg;
}

}  // namespace

void FdSet::close_all()
{
    for (int fd : fds_) close(fd);
    fds_.clear();
}

bool write_all(int fd, const void *p, size_t n)
{
    const char *c = (const char *) p;
    while (n) {
        const ssize_t w = send(fd, c, n, MSG_NOSIGNAL);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return false;
        c += w;
        n -= (size_t) w;
    }
    return true;
}

bool read_all(int fd, void *p, size_t n)
{
    char *c = (char *) p;
    while (n) {
        const ssize_t r = recv(fd, c, n, 0);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        c += r;
        n -= (size_t) r;
    }
    return true;
}

bool send_fd_batch(int s, const int *fds, int m)
{
    char byte = 'F';
    iovec iov;
    std::vector<char> ctl;
    msghdr msg = fd_msg(&iov, &byte, ctl, m);
    cmsghdr *cm = CMSG_FIRSTHDR(&msg);
    cm->cmsg_level = SOL_SOCKET;
    cm->cmsg_type = SCM_RIGHTS;
    cm->cmsg_len = CMSG_LEN(sizeof(int) * m);
    memcpy(CMSG_DATA(cm), fds, sizeof(int) * m);
    ssize_t w;
    do w = sendmsg(s, &msg, MSG_NOSIGNAL); while (w < 0 && errno == EINTR);
    return w == 1;
}

bool send_fds(int s, const std::vector<int> &fds)
{
    const unsigned long long n = fds.size();
    if (!write_all(s, &n, sizeof(n))) return false;
    for (size_t i = 0; i < fds.size(); i += kFdBatch)
        if (!send_fd_batch(s, fds.data() + i, (int) std::min(fds.size() - i, (size_t) kFdBatch)))
            return false;
    return true;
}

bool recv_fds(int s, FdSet &fds)
{
    unsigned long long n = 0;
    if (!read_all(s, &n, sizeof(n)) || n > (1u << 20)) return false;
    for (const size_t at = fds.size(); fds.size() - at < n;) {
        const int m = (int) std::min<unsigned long long>(n - (fds.size() - at), kFdBatch);
        char byte = 0;
        iovec iov;
        std::vector<char> ctl;
        msghdr msg = fd_msg(&iov, &byte, ctl, m);
        ssize_t r;
        do r = recvmsg(s, &msg, MSG_CMSG_CLOEXEC); while (r < 0 && errno == EINTR);
        if (r != 1) return false;
        cmsghdr *cm = CMSG_FIRSTHDR(&msg);
        if (!cm || cm->cmsg_type != SCM_RIGHTS || (msg.msg_flags & MSG_CTRUNC)) return false;
        const int got = (int) ((cm->cmsg_len - CMSG_LEN(0)) / sizeof(int));
        if (got > 0) fds.add((const int *) CMSG_DATA(cm), (size_t) got);
        if (got <= 0 || got > m) return false;  // a batch carries 1..m descriptors
    }
    return true;
}

bool FdServer::listen_on(long pid, long nonce)
{
    sockaddr_un a;
    socklen_t al;
    sock_name(pid, nonce, &a, &al);
    lfd_ = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    if (lfd_ >= 0 && bind(lfd_, (sockaddr *) &a, al) == 0 && listen(lfd_, 64) == 0) return true;
    const int e = errno;
    stop();
    errno = e;
    return false;
}

void FdServer::serve(const FdSet &fds, int expected)
{
    thread_ = std::thread([this, &fds, expected] {
        int waited_ms = 0;
        for (int k = 0; k < expected && !stop_.load() && waited_ms < kSetupTimeoutMs;) {
            pollfd p = {lfd_, POLLIN, 0};
            const int r = poll(&p, 1, 100);
            if (r < 0 && errno != EINTR) return;
            if (r <= 0) {
                waited_ms += 100;
                continue;
            }
            const int s = accept4(lfd_, nullptr, nullptr, SOCK_CLOEXEC);
            if (s < 0) continue;
            DBG("osgpu_heap_create: serving connection %d", k);
            if (send_fds(s, fds.get())) {
                char ack;
                (void) read_all(s, &ack, 1);  // the importer has its copies
                served_.fetch_add(1);
            }
            close(s);
            k++;
        }
    });
}

void FdServer::stop()
{
    stop_.store(true);
    if (thread_.joinable()) thread_.join();
    if (lfd_ >= 0) close(lfd_);
    lfd_ = -1;
}

FdClient::FdClient(long pid, long nonce) : s_(socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0))
{
    if (s_ < 0) return;
    timeval tv = {kSetupTimeoutMs / 1000, 0};
    setsockopt(s_, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof(tv));
    setsockopt(s_, SOL_SOCKET, SO_SNDTIMEO, &tv, sizeof(tv));
    sockaddr_un a;
    socklen_t al;
    sock_name(pid, nonce, &a, &al);
    connected_ = connect(s_, (sockaddr *) &a, al) == 0;
}

void FdClient::ack()
{
    if (s_ >= 0) (void) write_all(s_, "A", 1);
}

}  // namespace rt
}  // namespace osgpu
