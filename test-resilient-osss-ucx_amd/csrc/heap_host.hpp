// heap_host.hpp -- the parts of heap.cpp that are plain data in, plain data
// out, with no HIP call: a heap's chunk layout, and the text of
// osgpu_preflight's findings (one note per bad block, one JSON object per peer).
#pragma once
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace osgpu {
namespace rt {

// chunk lengths of a heap of `bytes` (a multiple of the granularity) in
// chunks of `chunk`
inline std::vector<size_t> chunk_lens(size_t bytes, size_t chunk)
{
    std::vector<size_t> v;
    for (size_t off = 0; off < bytes; off += chunk) v.push_back(std::min(chunk, bytes - off));
    return v;
}

struct PeerReport {
    int pe = -1;
    int chunks = 0;               // heap chunks probed on the peer
    std::string read, write;      // what went wrong in either direction ("": nothing)
};

// "; "-separated "region [chunk N] low|high: what" appended to `to`
inline void note_block(std::string &to, const char *region, int chunk, int end, const char *what)
{
    const bool heap = !strcmp(region, "heap");
    char b[160];
    snprintf(b, sizeof(b), "%s%s %s%d %s: %s", to.empty() ? "" : "; ", region,
             heap ? "chunk " : "", heap ? chunk : 0, end ? "high" : "low", what);
    to += b;
}

inline std::string preflight_report(const std::vector<PeerReport> &peers, bool staging, bool flags)
{
    std::string rep = "{";
    for (const PeerReport &p : peers) {
        char b[96];
        snprintf(b, sizeof(b), "%s\"%d\": {\"chunks\": %d, \"staging\": %s, \"flags\": %s, ",
                 rep.size() > 1 ? ", " : "", p.pe, p.chunks, staging ? "true" : "false",
                 flags ? "true" : "false");
        rep += b;
        rep += "\"status\": \"" + (p.read.empty() ? "ok" : p.read) + "\", ";
        rep += "\"remote_write\": \"" + (p.write.empty() ? "ok" : p.write) + "\"}";
    }
    return rep + "}";
}

}  // namespace rt
}  // namespace osgpu
