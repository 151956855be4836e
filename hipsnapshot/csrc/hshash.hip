// hshash: the hs64 blob checksum on the GPU -- one blob per launch on a copy
// stream (hsg_hash64, hsg_hash64_into) or many blobs in one launch
// (hsg_hash64_batch) -- with the accumulator ring and the batch workspace.

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "hsgpu_common.h"

namespace {

// ---- hs64 blob checksum (definition: csrc/hschk.cpp) -------------------------
// Grid-stride over the blob's 64-bit words; each lane mixes its words with
// their global index, a wave reduces with shuffles and adds its partial sum
// to one device accumulator (a vector atomic per wave).  Memory-bound: a
// staged blob is hashed in HBM right before its DMA to the host.
constexpr uint64_t kHsM1 = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t hs_mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

__global__ void __launch_bounds__(kBlock)
hs_hash64(const uint8_t* __restrict__ p, uint64_t n, uint64_t first_word,
          unsigned long long* __restrict__ acc) {
  const uint64_t nw = n / 8;
  const uint64_t tid = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint64_t nthr = uint64_t(gridDim.x) * blockDim.x;
  uint64_t s = 0;
  uint64_t done = 0;  // words covered by the vector loop
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    // 16 B per lane per load; the position keys advance by adding a
    // constant instead of a 64-bit multiply per word
    // (four independent loads in flight per lane: the launch is kept narrow
    // on purpose, see hsg_hash64, so each lane must cover latency itself)
    const uint64_t npair = nw / 2;
    const ulonglong2* v = reinterpret_cast<const ulonglong2*>(p);
    uint64_t key = (first_word + 2 * tid + 1) * kHsM1;
    const uint64_t dkey = 2 * nthr * kHsM1;
    uint64_t j = tid;
    for (; j + 3 * nthr < npair; j += 4 * nthr, key += 4 * dkey) {
      const ulonglong2 w0 = v[j], w1 = v[j + nthr], w2 = v[j + 2 * nthr], w3 = v[j + 3 * nthr];
      s += hs_mix64(w0.x ^ key) + hs_mix64(w0.y ^ (key + kHsM1));
      s += hs_mix64(w1.x ^ (key + dkey)) + hs_mix64(w1.y ^ (key + dkey + kHsM1));
      s += hs_mix64(w2.x ^ (key + 2 * dkey)) + hs_mix64(w2.y ^ (key + 2 * dkey + kHsM1));
      s += hs_mix64(w3.x ^ (key + 3 * dkey)) + hs_mix64(w3.y ^ (key + 3 * dkey + kHsM1));
    }
    for (; j < npair; j += nthr, key += dkey) {
      const ulonglong2 w = v[j];
      s += hs_mix64(w.x ^ key) + hs_mix64(w.y ^ (key + kHsM1));
    }
    done = 2 * npair;
  } else if ((reinterpret_cast<uintptr_t>(p) & 7) == 0) {
    const uint64_t* w = reinterpret_cast<const uint64_t*>(p);
    uint64_t key = (first_word + tid + 1) * kHsM1;
    const uint64_t dkey = nthr * kHsM1;
    for (uint64_t i = tid; i < nw; i += nthr, key += dkey) s += hs_mix64(w[i] ^ key);
    done = nw;
  } else {
    for (uint64_t i = tid; i < nw; i += nthr) {
      uint64_t w = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) w |= uint64_t(p[8 * i + k]) << (8 * k);
      s += hs_mix64(w ^ ((first_word + i + 1) * kHsM1));
    }
    done = nw;
  }
  if (tid == 0) {
    // the odd word after the pairs, then the zero-padded tail
    for (uint64_t i = done; i < nw; ++i) {
      uint64_t w = 0;
      for (int k = 0; k < 8; ++k) w |= uint64_t(p[8 * i + k]) << (8 * k);
      s += hs_mix64(w ^ ((first_word + i + 1) * kHsM1));
    }
    const uint64_t tail = n - 8 * nw;
    if (tail) {
      uint64_t w = 0;
      for (uint64_t k = 0; k < tail; ++k) w |= uint64_t(p[8 * nw + k]) << (8 * k);
      s += hs_mix64(w ^ ((first_word + nw + 1) * kHsM1));
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(acc, static_cast<unsigned long long>(s));
}

// ---- hs64 of many blobs in one launch (incremental takes) -----------------------
// Every leaf of a take is hashed before anything is copied, so the leaves
// share ONE launch: the host cuts them into tiles (as build_tiles does for
// hs_copy_nd) and the workgroups walk the tile table.  A tile is a run of
// whole 64-bit words of one leaf that starts an even number of words into it,
// so a tile's pointer has its leaf's alignment modulo 16 and only a leaf's
// last tile can hold the odd word and the zero-padded tail.
struct HashLeaf {
  const uint8_t* p;
  uint64_t n;  // bytes
};
struct HashTile {
  uint64_t first_word;  // index of the tile's first word within its leaf
  uint32_t n_words;     // whole words in the tile
  uint32_t leaf;
};
static_assert(sizeof(HashLeaf) == 16 && sizeof(HashTile) == 16, "hash table layout");

__global__ void __launch_bounds__(kBlock)
hs_hash64_batch(const HashLeaf* __restrict__ leaves, const HashTile* __restrict__ tiles,
                int64_t ntiles, unsigned long long* __restrict__ acc) {
  const uint32_t tid = threadIdx.x;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const HashTile tile = tiles[t];
    const HashLeaf leaf = leaves[tile.leaf];
    const uint64_t fw = tile.first_word;
    const uint64_t nw = tile.n_words;
    const uint8_t* p = leaf.p + 8 * fw;
    uint64_t s = 0;
    uint64_t done = 0;  // words of the tile covered by the vector loop
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      // hs_hash64's inner loop: 16 B per lane per load, four loads in
      // flight, position keys advanced by adding a constant
      const uint64_t npair = nw / 2;
      const ulonglong2* v = reinterpret_cast<const ulonglong2*>(p);
      uint64_t key = (fw + 2 * uint64_t(tid) + 1) * kHsM1;
      const uint64_t dkey = 2 * uint64_t(kBlock) * kHsM1;
      uint64_t j = tid;
      for (; j + 3 * kBlock < npair; j += 4 * kBlock, key += 4 * dkey) {
        const ulonglong2 w0 = v[j], w1 = v[j + kBlock], w2 = v[j + 2 * kBlock],
                         w3 = v[j + 3 * kBlock];
        s += hs_mix64(w0.x ^ key) + hs_mix64(w0.y ^ (key + kHsM1));
        s += hs_mix64(w1.x ^ (key + dkey)) + hs_mix64(w1.y ^ (key + dkey + kHsM1));
        s += hs_mix64(w2.x ^ (key + 2 * dkey)) + hs_mix64(w2.y ^ (key + 2 * dkey + kHsM1));
        s += hs_mix64(w3.x ^ (key + 3 * dkey)) + hs_mix64(w3.y ^ (key + 3 * dkey + kHsM1));
      }
      for (; j < npair; j += kBlock, key += dkey) {
        const ulonglong2 w = v[j];
        s += hs_mix64(w.x ^ key) + hs_mix64(w.y ^ (key + kHsM1));
      }
      done = 2 * npair;
    } else if ((reinterpret_cast<uintptr_t>(p) & 7) == 0) {
      const uint64_t* w = reinterpret_cast<const uint64_t*>(p);
      uint64_t key = (fw + tid + 1) * kHsM1;
      const uint64_t dkey = uint64_t(kBlock) * kHsM1;
      for (uint64_t i = tid; i < nw; i += kBlock, key += dkey) s += hs_mix64(w[i] ^ key);
      done = nw;
    } else {
      for (uint64_t i = tid; i < nw; i += kBlock) {
        uint64_t w = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) w |= uint64_t(p[8 * i + k]) << (8 * k);
        s += hs_mix64(w ^ ((fw + i + 1) * kHsM1));
      }
      done = nw;
    }
    if (tid == 0) {
      // the odd word after the pairs; then, in the leaf's last tile, the
      // zero-padded tail
      for (uint64_t i = done; i < nw; ++i) {
        uint64_t w = 0;
        for (int k = 0; k < 8; ++k) w |= uint64_t(p[8 * i + k]) << (8 * k);
        s += hs_mix64(w ^ ((fw + i + 1) * kHsM1));
      }
      const uint64_t end = 8 * (fw + nw);
      if (leaf.n - end < 8) {  // fewer than 8 bytes follow: this is the last tile
        const uint64_t tail = leaf.n - end;
        if (tail) {
          uint64_t w = 0;
          for (uint64_t k = 0; k < tail; ++k) w |= uint64_t(leaf.p[end + k]) << (8 * k);
          s += hs_mix64(w ^ ((fw + nw + 1) * kHsM1));
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((tid & 63) == 0) atomicAdd(acc + tile.leaf, static_cast<unsigned long long>(s));
  }
}

// ---- hs64 on the copy streams -------------------------------------------------
// A ring of 8-byte device accumulators (+ pinned landing words) per device.
// Every hash takes the next ring entry, so threads that share a copy stream
// never share an accumulator; an entry comes round again only after
// kHashRing later hashes, long after its result was read (each thread has at
// most one hash in flight).
constexpr int kHashRing = 4096;
struct HashRing {
  unsigned long long* acc = nullptr;
  uint64_t* host = nullptr;
  std::atomic<uint32_t> next{0};
};
std::mutex g_hash_mu;
std::map<int, HashRing> g_hash_rings;

int hash_ring(int dev, HashRing** out) {
  std::lock_guard<std::mutex> g(g_hash_mu);
  HashRing& h = g_hash_rings[dev];
  if (h.acc == nullptr) {
    HS_CHECK(hipSetDevice(dev));
    HS_CHECK(hipMalloc(reinterpret_cast<void**>(&h.acc), kHashRing * sizeof(unsigned long long)));
    HS_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h.host), kHashRing * sizeof(uint64_t),
                           hipHostMallocDefault));
  }
  *out = &h;
  return 0;
}

}  // namespace

const void* hs_hash_kernel() { return reinterpret_cast<const void*>(&hs_hash64); }

extern "C" {

// Enqueue hs64's partial sum of device bytes [p, p + n) (first word index
// `first_word`) on stream (dev, slot), ordered after everything queued so far
// on stream (dev, after_slot) when after_slot >= 0: the hash of a blob then
// runs beside its device->host copy (both only read it) instead of in front.
// Nothing is synchronised; *handle names the result for hsg_hash64_result.
//
// `max_grid` bounds the launch (<= 0: whole chip).  A full-width hash reads
// HBM at ~4 TB/s and slows concurrent SDMA reads of HBM by ~20 %
// (scripts/probes/hash_probe.py), while blobs only need hashing at the PCIe rate;
// the staging path therefore launches it narrow.
int hsg_hash64(int dev, int slot, int after_slot, const void* p, uint64_t n,
               uint64_t first_word, int max_grid, int* handle) {
  HS_CHECK(hipSetDevice(dev));
  hipStream_t s;
  hipEvent_t ev;
  int r = hs_get_stream(dev,slot, &s, &ev);
  if (r) return r;
  if (after_slot >= 0 && after_slot != slot) {
    hipStream_t a;
    hipEvent_t aev;
    r = hs_get_stream(dev,after_slot, &a, &aev);
    if (r) return r;
    HS_CHECK(hipEventRecord(aev, a));
    HS_CHECK(hipStreamWaitEvent(s, aev, 0));
  }
  HashRing* h;
  r = hash_ring(dev, &h);
  if (r) return r;
  const int k = static_cast<int>(h->next.fetch_add(1) % kHashRing);
  HS_CHECK(hipMemsetAsync(h->acc + k, 0, sizeof(unsigned long long), s));
  const uint64_t words = n / 8 + 1;
  int grid = static_cast<int>(std::min<uint64_t>((words + kBlock - 1) / kBlock, 256 * 8));
  if (max_grid > 0) grid = std::min(grid, max_grid);
  const int cap = hsg_thread_grid_cap();
  if (cap > 0) grid = std::min(grid, cap);
  hipLaunchKernelGGL(hs_hash64, dim3(std::max(grid, 1)), dim3(kBlock), 0, s,
                     static_cast<const uint8_t*>(p), n, first_word, h->acc + k);
  HS_CHECK(hipGetLastError());
  *handle = k;
  return 0;
}

// hs64's partial sum of device bytes [p, p + n) into the caller's device
// accumulator `acc` (one u64, zeroed here), on the caller's `stream`: the
// native restore hashes every uploaded blob on the stream that decodes it,
// into one accumulator per blob of its own (no shared ring to outrun).
int hsg_hash64_into(int dev, void* stream, const void* p, uint64_t n, uint64_t first_word,
                    int max_grid, void* acc) {
  HS_CHECK(hipSetDevice(dev));
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto* a = static_cast<unsigned long long*>(acc);
  HS_CHECK(hipMemsetAsync(a, 0, sizeof(unsigned long long), s));
  const uint64_t words = n / 8 + 1;
  int grid = static_cast<int>(std::min<uint64_t>((words + kBlock - 1) / kBlock, 256 * 8));
  if (max_grid > 0) grid = std::min(grid, max_grid);
  hipLaunchKernelGGL(hs_hash64, dim3(std::max(grid, 1)), dim3(kBlock), 0, s,
                     static_cast<const uint8_t*>(p), n, first_word, a);
  HS_CHECK(hipGetLastError());
  return 0;
}

// The partial sum of hash `handle`, started on stream (dev, slot); waits for it.
int hsg_hash64_result(int dev, int slot, int handle, uint64_t* out) {
  HS_CHECK(hipSetDevice(dev));
  if (handle < 0 || handle >= kHashRing) {
    hs_set_error("hsg_hash64_result: handle %d is not in [0, %d)", handle, kHashRing);
    return -static_cast<int>(hipErrorInvalidValue) - 1;
  }
  hipStream_t s;
  hipEvent_t ev;
  int r = hs_get_stream(dev,slot, &s, &ev);
  if (r) return r;
  HashRing* h;
  r = hash_ring(dev, &h);
  if (r) return r;
  HS_CHECK(hipMemcpyAsync(h->host + handle, h->acc + handle, sizeof(uint64_t),
                          hipMemcpyDeviceToHost, s));
  HS_CHECK(hipStreamSynchronize(s));
  *out = h->host[handle];
  return 0;
}

// ---- hs64 of n blobs in one launch ----------------------------------------------
// Grow-only device workspace [accumulators | leaf table | tile table] and a
// pinned mirror of it per device; a call holds the device's lock from the
// table upload to the read-back, so calls never share them.
struct HashBatchWs {
  std::mutex mu;
  char* dev = nullptr;
  char* host = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
};
std::mutex g_hash_batch_mu;
std::map<int, HashBatchWs> g_hash_batch_ws;

// Tile size: 1 MiB, halved down to 32 KiB while the launch would have fewer
// than 4096 tiles (2 per workgroup of a full-width grid).
static uint64_t hash_tile_bytes(uint64_t total) {
  uint64_t tile = uint64_t(kTileBytes);
  while (tile > (32u << 10) && total / tile < 4096) tile >>= 1;
  return tile;
}

static void build_hash_tiles(const HashLeaf* leaves, int n, std::vector<HashTile>* tiles) {
  uint64_t total = 0;
  for (int i = 0; i < n; ++i) total += leaves[i].n;
  const uint64_t tile_words = hash_tile_bytes(total) / 8;  // even: 16-byte multiples
  for (int i = 0; i < n; ++i) {
    if (leaves[i].n == 0) continue;  // its accumulator stays zero
    const uint64_t nw = leaves[i].n / 8;
    uint64_t w = 0;
    do {  // (a leaf shorter than a word still gets the tile that adds its tail)
      const uint64_t c = std::min(tile_words, nw - w);
      tiles->push_back(HashTile{w, static_cast<uint32_t>(c), static_cast<uint32_t>(i)});
      w += c;
    } while (w < nw);
  }
}

// hs64's partial sums of `n` device blobs, descs = n x {ptr, nbytes}, into the
// host array `sums_out`: one memset, one table upload, ONE full-width launch
// and one read-back on `stream` (null: the default stream), which the call
// waits for.  Full width on purpose: nothing else of a take runs beside it
// (hsg_hash64's narrow grid is for hashes that run beside SDMA copies).
int hsg_hash64_batch(int dev, void* stream, const void* descs, int n, uint64_t* sums_out) {
  if (n <= 0) return 0;
  HS_CHECK(hipSetDevice(dev));
  const HashLeaf* leaves = static_cast<const HashLeaf*>(descs);
  std::vector<HashTile> tiles;
  build_hash_tiles(leaves, n, &tiles);
  if (tiles.empty()) {
    std::memset(sums_out, 0, sizeof(uint64_t) * n);
    return 0;
  }
  HashBatchWs* ws;
  {
    std::lock_guard<std::mutex> g(g_hash_batch_mu);
    ws = &g_hash_batch_ws[dev];
  }
  std::lock_guard<std::mutex> g(ws->mu);
  const size_t abytes = (sizeof(uint64_t) * n + 255) / 256 * 256;
  const size_t lbytes = (sizeof(HashLeaf) * n + 255) / 256 * 256;
  const size_t tbytes = sizeof(HashTile) * tiles.size();
  const size_t need = abytes + lbytes + tbytes;
  if (need > ws->cap) {
    if (ws->dev) HS_CHECK(hipFree(ws->dev));
    if (ws->host) HS_CHECK(hipHostFree(ws->host));
    ws->dev = ws->host = nullptr;
    ws->cap = 0;
    const size_t cap = std::max(need * 2, size_t(1) << 20);
    HS_CHECK(hipMalloc(reinterpret_cast<void**>(&ws->dev), cap));
    HS_CHECK(hipHostMalloc(reinterpret_cast<void**>(&ws->host), cap, hipHostMallocDefault));
    ws->cap = cap;
  }
  if (ws->ev == nullptr) HS_CHECK(hipEventCreateWithFlags(&ws->ev, hipEventDisableTiming));
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::memcpy(ws->host + abytes, leaves, sizeof(HashLeaf) * n);
  std::memset(ws->host + abytes + sizeof(HashLeaf) * n, 0, lbytes - sizeof(HashLeaf) * n);
  std::memcpy(ws->host + abytes + lbytes, tiles.data(), tbytes);
  HS_CHECK(hipMemsetAsync(ws->dev, 0, abytes, s));
  HS_CHECK(hipMemcpyAsync(ws->dev + abytes, ws->host + abytes, lbytes + tbytes,
                          hipMemcpyHostToDevice, s));
  const int64_t ntiles = static_cast<int64_t>(tiles.size());
  const int grid = static_cast<int>(std::min<int64_t>(ntiles, 256 * 8));
  hipLaunchKernelGGL(hs_hash64_batch, dim3(grid), dim3(kBlock), 0, s,
                     reinterpret_cast<const HashLeaf*>(ws->dev + abytes),
                     reinterpret_cast<const HashTile*>(ws->dev + abytes + lbytes), ntiles,
                     reinterpret_cast<unsigned long long*>(ws->dev));
  HS_CHECK(hipGetLastError());
  HS_CHECK(hipMemcpyAsync(ws->host, ws->dev, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, s));
  HS_CHECK(hipEventRecord(ws->ev, s));
  HS_CHECK(hipEventSynchronize(ws->ev));
  std::memcpy(sums_out, ws->host, sizeof(uint64_t) * n);
  return 0;
}

}  // extern "C"
