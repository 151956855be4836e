// Controls of the CPU device stubs (engine_stubs.cpp); the entry points of
// the host engines they stand under (hipsnapshot/csrc/hsrestore.cpp,
// hsdrain.cpp) and the hooks the stubs define come from the library's header.
#pragma once

#include <atomic>
#include <cstdint>

#include "hsgpu_hooks.h"

namespace stub {

// the stub's region-copy descriptor (hsg_desc_size): `src` first, as the
// restore engine rebases the first 8 bytes of every row
struct StubDesc {
  uint64_t src;
  uint64_t dst;
  uint64_t nbytes;
  uint64_t pad;
};

extern std::atomic<int> fail_upload_every;  // every Nth host -> device upload fails (0: none)
extern std::atomic<int> fail_d2h_every;     // every Nth device -> host copy fails
extern std::atomic<uint64_t> dev_cap;       // device allocations fail above this many live bytes
extern std::atomic<uint64_t> dev_live;
extern std::atomic<int> pinned_live;        // pinned blocks not released
extern std::atomic<int> corruption;         // copy launches whose stage / workspace was reused early
extern std::atomic<int> max_delay_us;       // random delay before each queued operation

uint64_t hash_bytes(const void* p, uint64_t n);
void* new_stream();  // a stream of the caller's (a "producer" of restore destinations)
void shutdown();     // joins every stub thread

}  // namespace stub
