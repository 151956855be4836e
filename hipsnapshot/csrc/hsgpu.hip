// hsgpu: host-side state of the MI355X (gfx950 / CDNA4) data plane.
//
// What the reference does through ATen on the GPU (pageable .to("cpu") in a
// 4-thread pool in io_preparers/tensor.py; slab alloc + per-member DtoD +
// .cpu() in batcher.py; host copy_ + narrow for restore/resharding) is
// re-designed as a caching pinned pool, side streams and a few kernel
// families.  This file holds what the kernels are launched around:
//
//   * a caching PINNED host pool (THP-backed registered memory, 2 MiB
//     granularity, reused across snapshots) so every DtoH/HtoD is a DMA into
//     page-locked memory, and a pool of uncached device blocks,
//   * per-(device, slot) non-blocking copy streams ordered after the producer
//     stream with an event (no device-wide sync, no default-stream stalls),
//   * the per-thread grid cap, the managed-memory helpers, the stream gate,
//   * the library's error message (hsgpu_common.h).
//
// The kernels live in hscopy.hip (batched strided copy/cast), hsquant.hip
// (fp8 / MX8 / Hadamard), hshash.hip (hs64) and hsz.hip (HSZ1 codec).
//
// C ABI (ctypes); no torch headers.

#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "hsgpu_common.h"

namespace {

constexpr size_t kPinnedGranule = size_t(2) << 20;

thread_local char t_err[512];

struct PinnedPool {
  std::mutex mu;
  std::multimap<size_t, void*> free_blocks;      // size -> ptr
  std::unordered_map<void*, size_t> live;       // ptr -> size
  size_t cached_bytes = 0;                        // total allocated (live + free)
  size_t in_use_bytes = 0;
  std::unordered_map<void*, int> node;            // blocks bound to a NUMA node
};
PinnedPool g_pool;

struct StreamKey {
  int dev, slot;
  bool operator<(const StreamKey& o) const { return dev != o.dev ? dev < o.dev : slot < o.slot; }
};
std::mutex g_stream_mu;
std::map<StreamKey, hipStream_t> g_streams;
std::map<StreamKey, hipEvent_t> g_events;

std::map<StreamKey, int> g_stream_prio;  // slots created with a priority (hsg_stream_priority)

}  // namespace

void hs_set_error(const char* fmt, ...) {
  char text[sizeof(t_err)];  // an argument may point into t_err
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(text, sizeof(text), fmt, ap);
  va_end(ap);
  std::memcpy(t_err, text, sizeof(t_err));
}

int hs_get_stream(int dev, int slot, hipStream_t* out, hipEvent_t* ev) {
  std::lock_guard<std::mutex> g(g_stream_mu);
  StreamKey k{dev, slot};
  auto it = g_streams.find(k);
  if (it == g_streams.end()) {
    HS_CHECK(hipSetDevice(dev));
    // default priority: lowest-priority copy streams made a concurrent
    // training step 45 % slower instead of 18 % (profiles/overlap/priority.md)
    hipStream_t s;
    auto pr = g_stream_prio.find(k);
    if (pr != g_stream_prio.end())
      HS_CHECK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, pr->second));
    else
      HS_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipEvent_t e;
    HS_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    g_streams[k] = s;
    g_events[k] = e;
    it = g_streams.find(k);
  }
  *out = it->second;
  *ev = g_events[k];
  return 0;
}

extern "C" {

const char* hsg_last_error() { return t_err; }

int hsg_device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// PCI domain / bus / device of HIP device `dev` (three attribute queries:
// hipGetDeviceProperties, behind torch.cuda.get_device_properties, took
// ~130 ms the first time in a process).  0 on success.
int hsg_pci_location(int dev, int* domain, int* bus, int* device) {
  if (hipDeviceGetAttribute(domain, hipDeviceAttributePciDomainId, dev) != hipSuccess ||
      hipDeviceGetAttribute(bus, hipDeviceAttributePciBusId, dev) != hipSuccess ||
      hipDeviceGetAttribute(device, hipDeviceAttributePciDeviceId, dev) != hipSuccess) {
    hs_set_error("hipDeviceGetAttribute(PCI) failed for device %d", dev);
    return -1;
  }
  return 0;
}

// ---- pinned pool ----------------------------------------------------------
//
// Pool blocks are anonymous memory backed by transparent huge pages and
// registered with the GPU (hipHostRegister), not hipHostMalloc blocks: the
// copy engines see both the same (SDMA device -> host 56.9 GB/s, host ->
// device 57.5 GB/s), but the CPU side -- pread()s of a restore into the
// block, pwrite()s of a take out of it -- runs ~1.5x faster on 2 MiB pages
// (pread into hipHostMalloc memory 88 GB/s, into THP-backed memory 131 GB/s,
// 16 threads; scripts/probes/pinned_thp_probe.py, profiles/pinned/).  Registering
// pre-faulted huge pages costs ~2 ms per GiB, once per pool block.  Any
// failure falls back to hipHostMalloc.

struct MappedBlock {
  void* base;
  size_t len;
};
std::mutex g_mapped_mu;
std::unordered_map<void*, MappedBlock> g_mapped;  // registered block -> its mapping

static void* alloc_thp_registered(size_t want, int node = -1) {
  constexpr size_t kHuge = size_t(2) << 20;
  const size_t len = want + kHuge;
  void* base = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (base == MAP_FAILED) return nullptr;
  char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(base) + kHuge - 1) & ~(kHuge - 1));
  if (node >= 0 && node < 64) {
    // pages on `node` whichever CPU touches them first (MPOL_BIND = 2)
    unsigned long mask = 1ul << node;
    if (syscall(SYS_mbind, p, want, 2, &mask, 65ul, 0u) != 0) {
      munmap(base, len);
      return nullptr;
    }
  }
  (void)madvise(p, want, MADV_HUGEPAGE);
  // fault every page in now (a huge page per 2 MiB where the kernel grants
  // one): registration then maps resident pages, and no copy pays a fault.
  // The kernel zeroes each page on its first touch; a large block is split
  // over 4 threads so a cold process's first blocks -- a restore's first
  // reads -- wait less.
  const size_t kSplit = size_t(32) << 20;
  const int nt = static_cast<int>(std::min<size_t>(4, std::max<size_t>(1, want / kSplit)));
  auto touch = [p](size_t lo, size_t hi) {
    for (size_t off = lo; off < hi; off += 4096) p[off] = 0;
  };
  if (nt <= 1) {
    touch(0, want);
  } else {
    const size_t per = (want / nt + kHuge - 1) / kHuge * kHuge;
    std::vector<std::thread> th;
    for (int i = 1; i < nt; ++i) {
      const size_t lo = std::min(want, per * i), hi = std::min(want, per * (i + 1));
      if (lo >= hi) continue;
      try {
        th.emplace_back(touch, lo, hi);
      } catch (...) {  // no thread to be had: touch this part here
        touch(lo, hi);
      }
    }
    touch(0, std::min(want, per));
    for (auto& t : th) t.join();
  }
  if (hipHostRegister(p, want, hipHostRegisterDefault) != hipSuccess) {
    (void)hipGetLastError();
    munmap(base, len);
    return nullptr;
  }
  std::lock_guard<std::mutex> g(g_mapped_mu);
  g_mapped[p] = MappedBlock{base, len};
  return p;
}

static void free_pinned_block(void* p) {
  {
    std::lock_guard<std::mutex> g(g_pool.mu);
    g_pool.node.erase(p);
  }
  MappedBlock mb{nullptr, 0};
  {
    std::lock_guard<std::mutex> g(g_mapped_mu);
    auto it = g_mapped.find(p);
    if (it != g_mapped.end()) {
      mb = it->second;
      g_mapped.erase(it);
    }
  }
  if (mb.base != nullptr) {
    (void)hipHostUnregister(p);
    munmap(mb.base, mb.len);
  } else {
    (void)hipHostFree(p);
  }
}

void* hsg_pinned_acquire(uint64_t nbytes) {
  size_t want = (std::max<size_t>(nbytes, 1) + kPinnedGranule - 1) / kPinnedGranule * kPinnedGranule;
  {
    std::lock_guard<std::mutex> g(g_pool.mu);
    auto it = g_pool.free_blocks.lower_bound(want);
    // best fit, but do not hand out a block more than 2x the request
    if (it != g_pool.free_blocks.end() && it->first <= 2 * want) {
      void* p = it->second;
      size_t sz = it->first;
      g_pool.free_blocks.erase(it);
      g_pool.live[p] = sz;
      g_pool.in_use_bytes += sz;
      return p;
    }
  }
  void* p = alloc_thp_registered(want);
  hipError_t e = hipSuccess;
  if (p == nullptr) e = hipHostMalloc(&p, want, hipHostMallocDefault);
  if (e != hipSuccess) {
    // out of pinnable memory: drop the cache and retry once
    std::vector<void*> drop;
    {
      std::lock_guard<std::mutex> g(g_pool.mu);
      for (auto& kv : g_pool.free_blocks) { drop.push_back(kv.second); g_pool.cached_bytes -= kv.first; }
      g_pool.free_blocks.clear();
    }
    for (void* q : drop) free_pinned_block(q);
    p = alloc_thp_registered(want);
    e = p != nullptr ? hipSuccess : hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess) {
      hs_set_error("hipHostMalloc: %s", hipGetErrorString(e));
      return nullptr;
    }
  }
  std::lock_guard<std::mutex> g(g_pool.mu);
  g_pool.live[p] = want;
  g_pool.cached_bytes += want;
  g_pool.in_use_bytes += want;
  return p;
}

// Blocks released while the pool caches more than this are returned to the
// driver instead of being kept (bounds pinned host memory per process).
uint64_t g_pool_limit = ~uint64_t(0);

void hsg_pinned_set_limit(uint64_t bytes) { g_pool_limit = bytes; }

// A pinned block whose pages are bound to NUMA `node` (an async take's UVM
// capture copies a table into a block on the table's own node, then writes
// it from there: engine/uvm_capture.py).  Cached separately from the
// unplaced blocks; node < 0 is hsg_pinned_acquire.
void* hsg_pinned_acquire_on(uint64_t nbytes, int node) {
  if (node < 0) return hsg_pinned_acquire(nbytes);
  const size_t want =
      (std::max<size_t>(nbytes, 1) + kPinnedGranule - 1) / kPinnedGranule * kPinnedGranule;
  {
    std::lock_guard<std::mutex> g(g_pool.mu);
    for (auto it = g_pool.free_blocks.lower_bound(want);
         it != g_pool.free_blocks.end() && it->first <= 2 * want; ++it) {
      auto nd = g_pool.node.find(it->second);
      if (nd == g_pool.node.end() || nd->second != node) continue;
      void* p = it->second;
      const size_t sz = it->first;
      g_pool.free_blocks.erase(it);
      g_pool.live[p] = sz;
      g_pool.in_use_bytes += sz;
      return p;
    }
  }
  void* p = alloc_thp_registered(want, node);
  if (p == nullptr) return nullptr;  // the caller falls back to an unplaced block
  std::lock_guard<std::mutex> g(g_pool.mu);
  g_pool.live[p] = want;
  g_pool.node[p] = node;
  g_pool.cached_bytes += want;
  g_pool.in_use_bytes += want;
  return p;
}

int hsg_pinned_release(void* p) {
  void* drop = nullptr;
  {
    std::lock_guard<std::mutex> g(g_pool.mu);
    auto it = g_pool.live.find(p);
    if (it == g_pool.live.end()) {
      hs_set_error("hsg_pinned_release: %p is not a live pinned block", p);
      return -1;
    }
    g_pool.in_use_bytes -= it->second;
    if (g_pool.cached_bytes > g_pool_limit) {
      g_pool.cached_bytes -= it->second;
      drop = p;
    } else {
      g_pool.free_blocks.emplace(it->second, p);
    }
    g_pool.live.erase(it);
  }
  if (drop) free_pinned_block(drop);
  return 0;
}

void hsg_pinned_stats(uint64_t* cached, uint64_t* in_use) {
  std::lock_guard<std::mutex> g(g_pool.mu);
  *cached = g_pool.cached_bytes;
  *in_use = g_pool.in_use_bytes;
}

uint64_t hsg_pinned_trim() {
  std::vector<std::pair<size_t, void*>> drop;
  {
    std::lock_guard<std::mutex> g(g_pool.mu);
    for (auto& kv : g_pool.free_blocks) drop.emplace_back(kv.first, kv.second);
    g_pool.free_blocks.clear();
    for (auto& kv : drop) g_pool.cached_bytes -= kv.first;
  }
  uint64_t freed = 0;
  for (auto& kv : drop) { free_pinned_block(kv.second); freed += kv.first; }
  return freed;
}

// Test hook: overwrite every idle block of the restore's device pools (on
// `dev`) and of the pinned host pool with `byte`, so a test can show that no
// restore reads bytes an earlier one left behind.  Returns the blocks written.
int hsg_poison_idle_pools(int dev, int byte) {
  std::vector<uint64_t> ptrs(4096), sizes(4096);
  const int n = hsg_restore_idle_blocks(dev, ptrs.data(), sizes.data(), 4096);
  HS_CHECK(hipSetDevice(dev));
  for (int i = 0; i < n; ++i)
    HS_CHECK(hipMemset(reinterpret_cast<void*>(ptrs[i]), byte, sizes[i]));
  HS_CHECK(hipDeviceSynchronize());
  int m = 0;
  std::lock_guard<std::mutex> g(g_pool.mu);
  for (auto& kv : g_pool.free_blocks) {
    std::memset(kv.second, byte, kv.first);
    ++m;
  }
  return n + m;
}

// ---- uncached device blocks (SDMA upload targets, csrc/hsdma.hip) ----------
//
// hipDeviceMallocUncached memory, cached per device by size (best fit up to
// 2x, 2 MiB granules): the restore's encoded frames are uploaded into it by
// SDMA and read once by the decode kernel, never through a stale L2 line.
struct UncachedPool {
  std::mutex mu;
  std::map<int, std::multimap<size_t, void*>> free_blocks;  // dev -> size -> block
  std::unordered_map<void*, std::pair<int, size_t>> live;
  size_t cached_bytes = 0;
};
UncachedPool g_upool;

void* hsg_uncached_acquire(int dev, uint64_t nbytes) {
  constexpr size_t kGranule = size_t(2) << 20;
  const size_t want = (std::max<size_t>(nbytes, 1) + kGranule - 1) / kGranule * kGranule;
  {
    std::lock_guard<std::mutex> g(g_upool.mu);
    auto& fl = g_upool.free_blocks[dev];
    auto it = fl.lower_bound(want);
    if (it != fl.end() && it->first <= 2 * want) {
      void* p = it->second;
      g_upool.live[p] = {dev, it->first};
      fl.erase(it);
      return p;
    }
  }
  // hsg_rt_vmm_alloc (hshost.hip): a freed block's address is never handed
  // out again (re-used addresses of freed uncached blocks were written
  // through stale translations, profiles/r6/trim/)
  void* p = hsg_rt_vmm_alloc(dev, want, 1);
  if (p == nullptr) {
    // drop this device's idle blocks and retry once
    std::vector<void*> drop;
    {
      std::lock_guard<std::mutex> g(g_upool.mu);
      auto& fl = g_upool.free_blocks[dev];
      for (auto& kv : fl) { drop.push_back(kv.second); g_upool.cached_bytes -= kv.first; }
      fl.clear();
    }
    for (void* q : drop) (void)hsg_rt_vmm_free(q);
    p = hsg_rt_vmm_alloc(dev, want, 1);
    if (p == nullptr) {
      // (hsg_rt_vmm_alloc's text is this thread's current message: hs_set_error
      // formats aside before it overwrites it)
      hs_set_error("uncached block of %zu bytes: %s", want, hsg_last_error());
      return nullptr;
    }
  }
  std::lock_guard<std::mutex> g(g_upool.mu);
  g_upool.live[p] = {dev, want};
  g_upool.cached_bytes += want;
  return p;
}

// Bytes the uncached pool holds (idle + in use, every device).
uint64_t hsg_uncached_bytes() {
  std::lock_guard<std::mutex> g(g_upool.mu);
  return g_upool.cached_bytes;
}

int hsg_uncached_release(void* p) {
  std::lock_guard<std::mutex> g(g_upool.mu);
  auto it = g_upool.live.find(p);
  if (it == g_upool.live.end()) {
    hs_set_error("hsg_uncached_release: %p is not a live uncached block", p);
    return -1;
  }
  g_upool.free_blocks[it->second.first].emplace(it->second.second, p);
  g_upool.live.erase(it);
  return 0;
}

// Free every idle uncached block; returns the bytes freed.
uint64_t hsg_uncached_trim() {
  std::vector<std::pair<int, void*>> drop;
  uint64_t freed = 0;
  {
    std::lock_guard<std::mutex> g(g_upool.mu);
    for (auto& dv : g_upool.free_blocks) {
      for (auto& kv : dv.second) {
        drop.emplace_back(dv.first, kv.second);
        freed += kv.first;
      }
      dv.second.clear();
    }
    g_upool.cached_bytes -= freed;
  }
  for (auto& d : drop) (void)hsg_rt_vmm_free(d.second);
  return freed;
}

// ---- DMA copies on side streams --------------------------------------------

// Copy `n` bytes between host and device on copy stream (dev, slot), ordered
// after all work already queued on `producer` when `has_producer` is set (a
// torch stream; handle 0 = the legacy default stream).
// kind: 0 = D2H, 1 = H2D, 2 = D2D.  If `sync` is nonzero the call blocks until
// the copy is done (ctypes releases the GIL around it).
int hsg_memcpy(int dev, int slot, void* dst, const void* src, uint64_t n, int kind,
               void* producer, int has_producer, int sync) {
  HS_CHECK(hipSetDevice(dev));
  hipStream_t s;
  hipEvent_t ev;
  int r = hs_get_stream(dev, slot, &s, &ev);
  if (r) return r;
  // producer may be the legacy null stream (handle 0, torch's default stream):
  // the copy streams are non-blocking, so it must be joined explicitly too
  if (has_producer) {
    HS_CHECK(hipEventRecord(ev, static_cast<hipStream_t>(producer)));
    HS_CHECK(hipStreamWaitEvent(s, ev, 0));
  }
  hipMemcpyKind k = kind == 0 ? hipMemcpyDeviceToHost
                  : kind == 1 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  if (n) HS_CHECK(hipMemcpyAsync(dst, src, n, k, s));
  if (sync) HS_CHECK(hipStreamSynchronize(s));
  return 0;
}

// Make `consumer` (torch stream) wait for everything queued on copy stream
// (dev, slot) -- used after H2D restores so the trainer sees the data.
int hsg_stream_join(int dev, int slot, void* consumer) {
  HS_CHECK(hipSetDevice(dev));
  hipStream_t s;
  hipEvent_t ev;
  int r = hs_get_stream(dev, slot, &s, &ev);
  if (r) return r;
  HS_CHECK(hipEventRecord(ev, s));
  HS_CHECK(hipStreamWaitEvent(static_cast<hipStream_t>(consumer), ev, 0));
  return 0;
}

int hsg_stream_sync(int dev, int slot) {
  HS_CHECK(hipSetDevice(dev));
  hipStream_t s;
  hipEvent_t ev;
  int r = hs_get_stream(dev, slot, &s, &ev);
  if (r) return r;
  HS_CHECK(hipStreamSynchronize(s));
  return 0;
}

// Grid cap for the calling thread's launches (0 = none).  The async-take
// drain runs its staging threads with a cap so its kernels (HSZ1 encode,
// slab gathers) occupy only that many CUs while training continues: at full
// width the encoder made a concurrent Llama-3-8B training step ~30 % slower
// (profiles/overlap_iso/), and the drain is PCIe-bound anyway.
thread_local int t_grid_cap = 0;

int hsg_set_thread_grid_cap(int cap) {
  const int old = t_grid_cap;
  t_grid_cap = cap < 0 ? 0 : cap;
  return old;
}

int hsg_thread_grid_cap() { return t_grid_cap; }

// Create stream (dev, slot) at the device's highest priority (high != 0)
// when it is first used.  The native drain's hash stream: its tiny hs64
// launches and 8-byte read-backs otherwise queue behind a saturating
// training step's workgroups -- a GEMM loop on another stream cut a drain
// with hashing from 36 to 13.5 GB/s, without hashing it kept 35.6 GB/s
// (scripts/probes/drain_contention_probe.py, profiles/r3/drain_probe/).  Returns
// 1 if the stream already existed (its priority is unchanged).
int hsg_stream_priority(int dev, int slot, int high) {
  std::lock_guard<std::mutex> g(g_stream_mu);
  StreamKey k{dev, slot};
  if (g_streams.count(k)) return 1;
  int least = 0, greatest = 0;
  HS_CHECK(hipSetDevice(dev));
  HS_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  g_stream_prio[k] = high ? greatest : least;
  return 0;
}

void* hsg_copy_stream(int dev, int slot) {
  hipStream_t s;
  hipEvent_t ev;
  if (hs_get_stream(dev, slot, &s, &ev)) return nullptr;
  return s;
}

int hsg_sync_stream_handle(void* stream) {
  HS_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return 0;
}

// Load the code objects of the copy, hash and quantization kernels on `dev`
// now (the runtime loads each at its first kernel launch otherwise: ~3 ms
// that fell into the first async_take's freeze launch).  Called from a helper
// thread while a first take plans.
int hsg_prewarm_module(int dev) {
  HS_CHECK(hipSetDevice(dev));
  for (const void* kernel : {hs_copy_kernel(), hs_hash_kernel(), hs_quant_kernel()}) {
    hipFuncAttributes attr;
    HS_CHECK(hipFuncGetAttributes(&attr, kernel));
  }
  return 0;
}

// ---- managed (UVM) memory helpers (fbgemm uvm_to_cpu equivalent, K11) --------

int hsg_is_managed(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return attr.isManaged ? 1 : 0;
}

void* hsg_managed_alloc(int dev, uint64_t n) {
  hipError_t e = hipSetDevice(dev);
  if (e != hipSuccess) {
    hs_set_error("hipSetDevice(%d): %s", dev, hipGetErrorString(e));
    return nullptr;
  }
  void* p = nullptr;
  e = hipMallocManaged(&p, n, hipMemAttachGlobal);
  if (e != hipSuccess) {
    hs_set_error("hipMallocManaged: %s", hipGetErrorString(e));
    return nullptr;
  }
  return p;
}

int hsg_managed_free(void* p) {
  HS_CHECK(hipFree(p));
  return 0;
}

// ---- stream gates (engine/uvm_capture.py) ------------------------------------
//
// An async take of host-resident UVM tables copies them on the CPU (threads on
// the pages' NUMA node: ~160-200 GB/s vs ~55 GB/s for the HBM freeze kernel
// reading them over PCIe, profiles/r6/uvmcap/) while the trainer's stream
// waits on a host word: hipStreamWaitValue32(word >= v) armed on the stream,
// released by the CPU once the copy is done.  One word per device, values
// increase per take, and a release only ever raises the word (an older
// take's late release cannot re-block a newer gate).

struct GateWord {
  uint32_t* word = nullptr;
  uint32_t next = 0;
};
std::mutex g_gate_mu;
std::map<int, GateWord> g_gates;

// 1 if hipStreamWaitValue32 works on `dev` (else the HBM freeze is used).
int hsg_gate_supported(int dev) {
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeCanUseStreamWaitValue, dev) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return v ? 1 : 0;
}

// Arm a gate on `stream`: work queued on it from now on waits until the
// gate's value is released.  *value gets the value to release (> 0).
int hsg_gate_arm(int dev, void* stream, uint32_t* value) {
  HS_CHECK(hipSetDevice(dev));
  std::lock_guard<std::mutex> g(g_gate_mu);
  GateWord& gw = g_gates[dev];
  if (gw.word == nullptr) {
    void* p = nullptr;
    // signal memory: the command processor polls it, the CPU stores into it;
    // allocated once per device and never freed
    HS_CHECK(hipExtMallocWithFlags(&p, 8, hipMallocSignalMemory));
    gw.word = static_cast<uint32_t*>(p);
    __atomic_store_n(gw.word, 0u, __ATOMIC_SEQ_CST);
  }
  const uint32_t v = ++gw.next;
  HS_CHECK(hipStreamWaitValue32(static_cast<hipStream_t>(stream), gw.word, v,
                                hipStreamWaitValueGte, 0xffffffffu));
  *value = v;
  return 0;
}

// Release every gate of `dev` armed with a value <= `value`.
int hsg_gate_release(int dev, uint32_t value) {
  uint32_t* w;
  {
    std::lock_guard<std::mutex> g(g_gate_mu);
    auto it = g_gates.find(dev);
    if (it == g_gates.end() || it->second.word == nullptr) {
      hs_set_error("hsg_gate_release: no gate was armed on device %d", dev);
      return -1;
    }
    w = it->second.word;
  }
  uint32_t cur = __atomic_load_n(w, __ATOMIC_ACQUIRE);
  while (cur < value && !__atomic_compare_exchange_n(w, &cur, value, false, __ATOMIC_SEQ_CST,
                                                     __ATOMIC_ACQUIRE)) {
  }
  return 0;
}

// The gate word's current value (tests).
uint32_t hsg_gate_value(int dev) {
  std::lock_guard<std::mutex> g(g_gate_mu);
  auto it = g_gates.find(dev);
  if (it == g_gates.end() || it->second.word == nullptr) return 0;
  return __atomic_load_n(it->second.word, __ATOMIC_ACQUIRE);
}

// Advised placement of a managed range: *preferred / *last_prefetch get a
// device index, -1 (hipCpuDeviceId: host DRAM) or -2 (never set).
int hsg_managed_location(const void* p, uint64_t n, int* preferred, int* last_prefetch) {
  int v = -2;
  if (hipMemRangeGetAttribute(&v, sizeof(v), hipMemRangeAttributePreferredLocation,
                              const_cast<void*>(p), n) != hipSuccess) {
    (void)hipGetLastError();
    v = -2;
  }
  *preferred = v;
  v = -2;
  if (hipMemRangeGetAttribute(&v, sizeof(v), hipMemRangeAttributeLastPrefetchLocation,
                              const_cast<void*>(p), n) != hipSuccess) {
    (void)hipGetLastError();
    v = -2;
  }
  *last_prefetch = v;
  return 0;
}

// Place a managed range: preferred location `loc` (device index, or -1 for
// host DRAM) and an asynchronous prefetch there on `stream`.
int hsg_managed_place(int dev, const void* p, uint64_t n, int loc, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  HS_CHECK(hipMemAdvise(p, n, hipMemAdviseSetPreferredLocation, loc));
  HS_CHECK(hipMemPrefetchAsync(p, n, loc, static_cast<hipStream_t>(stream)));
  return 0;
}

}  // extern "C"
