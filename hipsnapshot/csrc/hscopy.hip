// hscopy: ONE batched strided copy/cast kernel (hs_copy_nd) that serves as
//   K2  strided -> contiguous pack,
//   K3  multi-tensor slab gather (descriptor table, one launch),
//   K6  contiguous -> strided scatter with dtype conversion on restore,
//   K7  resharding: every saved-shard x local-shard overlap in one launch,
// and can target host-mapped pinned memory directly (kernel stores over PCIe,
// "pack-to-host") or HBM (async-snapshot arena).
//
// Work decomposition: every descriptor is cut into tiles of a fixed number of
// elements; a tile table is built on the host and the grid walks it with a
// grid-stride loop (grid capped at 256 CUs x 8), so thousands of tiny tensors
// and a few huge ones share one launch and fill all 256 CUs.  Each lane moves
// 16 bytes per access (dwordx4) wherever alignment allows (CDNA guide,
// Guideline 13).  Wave size is 64 everywhere.

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "hsgpu_common.h"

namespace {

constexpr int kMaxDims = 8;

struct CopyDesc {
  const char* src;
  char* dst;
  int64_t numel;
  int32_t ndim;
  int32_t src_dtype;
  int32_t dst_dtype;
  int32_t flags;  // bit0: both fully contiguous & same type -> byte copy
  int64_t sizes[kMaxDims];
  int64_t src_strides[kMaxDims];  // in elements
  int64_t dst_strides[kMaxDims];
};

struct Tile {
  int32_t desc;
  int32_t pad;
  int64_t begin;  // element (or byte for flag-0 byte copies) range
  int64_t end;
};

__device__ __forceinline__ int elem_size(int32_t dt) {
  switch (dt) {
    case kRaw1: return 1;
    case kRaw2: case kF16: case kBF16: return 2;
    case kRaw4: case kF32: return 4;
    case kRaw8: case kF64: return 8;
    default: return 16;
  }
}

__device__ __forceinline__ double load_as_f64(const char* p, int32_t dt) {
  switch (dt) {
    case kF16: return static_cast<double>(static_cast<float>(*reinterpret_cast<const _Float16*>(p)));
    case kBF16: return static_cast<double>(bf16_to_f32(*reinterpret_cast<const uint16_t*>(p)));
    case kF32: return static_cast<double>(*reinterpret_cast<const float*>(p));
    default: return *reinterpret_cast<const double*>(p);
  }
}

__device__ __forceinline__ void store_from_f64(char* p, int32_t dt, double v) {
  switch (dt) {
    // f64 -> f16 goes through f32 (two RNE roundings) exactly like torch's
    // copy_ on ROCm (c10::Half is constructed from float); measured on MI355X:
    // a single-rounding conversion differs from torch in ~1e-4 of values.
    case kF16: {
      // the empty asm pins the f32 intermediate: without it LLVM folds the two
      // fptruncs into one f64->f16 rounding, which torch does not do
      float f = static_cast<float>(v);
      asm volatile("" : "+v"(f));
      *reinterpret_cast<_Float16*>(p) = static_cast<_Float16>(f);
      break;
    }
    case kBF16: *reinterpret_cast<uint16_t*>(p) = f32_to_bf16(static_cast<float>(v)); break;
    case kF32: *reinterpret_cast<float*>(p) = static_cast<float>(v); break;
    default: *reinterpret_cast<double*>(p) = v; break;
  }
}

// Contiguous same-type byte copy of [begin, end) bytes: dwordx4 body when both
// pointers are 16-B aligned at the tile start, byte loop otherwise.
__device__ void copy_bytes(const char* __restrict__ src, char* __restrict__ dst,
                           int64_t begin, int64_t end) {
  const char* s = src + begin;
  char* d = dst + begin;
  int64_t n = end - begin;
  if (((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0) {
    const int64_t nv = n >> 4;
    const uint4* sv = reinterpret_cast<const uint4*>(s);
    uint4* dv = reinterpret_cast<uint4*>(d);
    int64_t i = threadIdx.x;
    // 4 independent 16-B loads in flight per lane before the stores
    for (; i + 3 * kBlock < nv; i += 4 * kBlock) {
      uint4 a = sv[i], b = sv[i + kBlock], c = sv[i + 2 * kBlock], e = sv[i + 3 * kBlock];
      dv[i] = a; dv[i + kBlock] = b; dv[i + 2 * kBlock] = c; dv[i + 3 * kBlock] = e;
    }
    for (; i < nv; i += kBlock) dv[i] = sv[i];
    for (int64_t j = (nv << 4) + threadIdx.x; j < n; j += kBlock) d[j] = s[j];
  } else if (((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 3) == 0) {
    const int64_t nv = n >> 2;
    const uint32_t* sv = reinterpret_cast<const uint32_t*>(s);
    uint32_t* dv = reinterpret_cast<uint32_t*>(d);
    for (int64_t i = threadIdx.x; i < nv; i += kBlock) dv[i] = sv[i];
    for (int64_t j = (nv << 2) + threadIdx.x; j < n; j += kBlock) d[j] = s[j];
  } else {
    for (int64_t j = threadIdx.x; j < n; j += kBlock) d[j] = s[j];
  }
}

template <int ES>
struct RawT;
template <> struct RawT<1> { using T = uint8_t; };
template <> struct RawT<2> { using T = uint16_t; };
template <> struct RawT<4> { using T = uint32_t; };
template <> struct RawT<8> { using T = uint64_t; };
template <> struct RawT<16> { using T = uint4; };

// Each lane owns kRun consecutive logical elements: decode the N-d index once,
// then walk with carry propagation (one divide chain per run instead of per
// element).  ND is a template parameter so the coordinate arrays stay in VGPRs
// (a runtime-indexed array would spill to scratch -- CDNA guide 5.4 rule 20);
// the host collapses mergeable dims first so ND <= 4 covers practically every
// view (narrow/transpose/column shard).
constexpr int kRun = 8;

template <int ND>
__device__ __forceinline__ void decode(const CopyDesc& d, int64_t linear, int64_t* coord,
                                       int64_t* soff, int64_t* doff) {
  int64_t s = 0, t = 0;
#pragma unroll
  for (int k = ND - 1; k >= 0; --k) {
    const int64_t sz = d.sizes[k];
    int64_t c;
    if (k == 0) {
      c = linear;
    } else {
      c = linear % sz;
      linear /= sz;
    }
    coord[k] = c;
    s += c * d.src_strides[k];
    t += c * d.dst_strides[k];
  }
  *soff = s;
  *doff = t;
}

template <int ND>
__device__ __forceinline__ void advance(const CopyDesc& d, int64_t* coord, int64_t* soff,
                                        int64_t* doff) {
#pragma unroll
  for (int k = ND - 1; k >= 0; --k) {
    coord[k] += 1;
    *soff += d.src_strides[k];
    *doff += d.dst_strides[k];
    if (k == 0 || coord[k] < d.sizes[k]) return;
    *soff -= coord[k] * d.src_strides[k];
    *doff -= coord[k] * d.dst_strides[k];
    coord[k] = 0;
  }
}

template <int ND, int ES>
__device__ void copy_strided_same(const CopyDesc& d, int64_t begin, int64_t end) {
  using T = typename RawT<ES>::T;
  const T* __restrict__ src = reinterpret_cast<const T*>(d.src);
  T* __restrict__ dst = reinterpret_cast<T*>(d.dst);
  for (int64_t base = begin + int64_t(threadIdx.x) * kRun; base < end;
       base += int64_t(kBlock) * kRun) {
    int64_t coord[ND];
    int64_t so, dof;
    decode<ND>(d, base, coord, &so, &dof);
    const int64_t cnt = min(int64_t(kRun), end - base);
    T buf[kRun];
    int64_t doffs[kRun];
#pragma unroll
    for (int r = 0; r < kRun; ++r) {
      if (r < cnt) {
        buf[r] = src[so];
        doffs[r] = dof;
        advance<ND>(d, coord, &so, &dof);
      }
    }
#pragma unroll
    for (int r = 0; r < kRun; ++r) {
      if (r < cnt) dst[doffs[r]] = buf[r];
    }
  }
}

template <int ND>
__device__ void copy_strided_cast(const CopyDesc& d, int64_t begin, int64_t end) {
  const int ses = elem_size(d.src_dtype);
  const int des = elem_size(d.dst_dtype);
  const bool wide = (d.src_dtype == kF64) || (d.dst_dtype == kF64);
  for (int64_t base = begin + int64_t(threadIdx.x) * kRun; base < end;
       base += int64_t(kBlock) * kRun) {
    int64_t coord[ND];
    int64_t so, dof;
    decode<ND>(d, base, coord, &so, &dof);
    const int64_t lim = min(base + kRun, end);
    for (int64_t e = base; e < lim; ++e) {
      const char* sp = d.src + so * ses;
      char* dp = d.dst + dof * des;
      if (wide) store_from_f64(dp, d.dst_dtype, load_as_f64(sp, d.src_dtype));
      else store_from_f32(dp, d.dst_dtype, load_as_f32(sp, d.src_dtype));
      advance<ND>(d, coord, &so, &dof);
    }
  }
}

// Contiguous -> contiguous cast between f16 / bf16 / f32 (the restore of an
// fp32 checkpoint into a bf16 model, and back): 8 elements per lane per step
// with 16-B vector loads and stores, same conversions as store_from_f32(
// load_as_f32()) (bit-identical to torch's copy_).  Unaligned tiles and the
// tail take the scalar path.
template <int DT>
__device__ __forceinline__ void load8_f32(const char* p, float* f) {
  if constexpr (DT == kF32) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0];
    const uint4 b = reinterpret_cast<const uint4*>(p)[1];
    f[0] = __uint_as_float(a.x); f[1] = __uint_as_float(a.y);
    f[2] = __uint_as_float(a.z); f[3] = __uint_as_float(a.w);
    f[4] = __uint_as_float(b.x); f[5] = __uint_as_float(b.y);
    f[6] = __uint_as_float(b.z); f[7] = __uint_as_float(b.w);
  } else {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0];
    const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint16_t lo = static_cast<uint16_t>(w[i] & 0xffffu);
      const uint16_t hi = static_cast<uint16_t>(w[i] >> 16);
      if constexpr (DT == kBF16) {
        f[2 * i] = bf16_to_f32(lo);
        f[2 * i + 1] = bf16_to_f32(hi);
      } else {
        _Float16 x, y;
        __builtin_memcpy(&x, &lo, 2);
        __builtin_memcpy(&y, &hi, 2);
        f[2 * i] = static_cast<float>(x);
        f[2 * i + 1] = static_cast<float>(y);
      }
    }
  }
}

template <int DT>
__device__ __forceinline__ void store8_f32(char* p, const float* f) {
  if constexpr (DT == kF32) {
    reinterpret_cast<uint4*>(p)[0] = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]),
                                                __float_as_uint(f[2]), __float_as_uint(f[3]));
    reinterpret_cast<uint4*>(p)[1] = make_uint4(__float_as_uint(f[4]), __float_as_uint(f[5]),
                                                __float_as_uint(f[6]), __float_as_uint(f[7]));
  } else {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint16_t lo, hi;
      if constexpr (DT == kBF16) {
        lo = f32_to_bf16(f[2 * i]);
        hi = f32_to_bf16(f[2 * i + 1]);
      } else {
        const _Float16 a = static_cast<_Float16>(f[2 * i]);
        const _Float16 b = static_cast<_Float16>(f[2 * i + 1]);
        __builtin_memcpy(&lo, &a, 2);
        __builtin_memcpy(&hi, &b, 2);
      }
      w[i] = uint32_t(lo) | (uint32_t(hi) << 16);
    }
    reinterpret_cast<uint4*>(p)[0] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

template <int SD, int DD>
__device__ void copy_contig_cast(const CopyDesc& d, int64_t begin, int64_t end) {
  constexpr int SES = (SD == kF32) ? 4 : 2;
  constexpr int DES = (DD == kF32) ? 4 : 2;
  const char* s = d.src + begin * SES;
  char* o = d.dst + begin * DES;
  const int64_t n = end - begin;
  int64_t done = 0;
  if (((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(o)) & 15) == 0) {
    const int64_t nv = n / 8;
    for (int64_t i = threadIdx.x; i < nv; i += kBlock) {
      float f[8];
      load8_f32<SD>(s + i * 8 * SES, f);
      store8_f32<DD>(o + i * 8 * DES, f);
    }
    done = nv * 8;
  }
  for (int64_t j = done + threadIdx.x; j < n; j += kBlock)
    store_from_f32(o + j * DES, DD, load_as_f32(s + j * SES, SD));
}

template <int ND>
__device__ __forceinline__ bool try_contig_cast(const CopyDesc& d, int64_t b, int64_t e) {
  if constexpr (ND != 1) {
    return false;
  } else {
    if (d.src_strides[0] != 1 || d.dst_strides[0] != 1) return false;
    const int sd = d.src_dtype, dd = d.dst_dtype;
#define HS_CAST_CASE(S, D) \
    if (sd == S && dd == D) { copy_contig_cast<S, D>(d, b, e); return true; }
    HS_CAST_CASE(kF32, kBF16) HS_CAST_CASE(kBF16, kF32)
    HS_CAST_CASE(kF32, kF16) HS_CAST_CASE(kF16, kF32)
    HS_CAST_CASE(kBF16, kF16) HS_CAST_CASE(kF16, kBF16)
#undef HS_CAST_CASE
    return false;
  }
}

template <int ND>
__device__ __forceinline__ void copy_tile_nd(const CopyDesc& d, int64_t b, int64_t e) {
  if (d.src_dtype == d.dst_dtype || d.src_dtype < kF16) {
    switch (elem_size(d.src_dtype)) {
      case 1: copy_strided_same<ND, 1>(d, b, e); break;
      case 2: copy_strided_same<ND, 2>(d, b, e); break;
      case 4: copy_strided_same<ND, 4>(d, b, e); break;
      case 8: copy_strided_same<ND, 8>(d, b, e); break;
      default: copy_strided_same<ND, 16>(d, b, e); break;
    }
  } else if (!try_contig_cast<ND>(d, b, e)) {
    copy_strided_cast<ND>(d, b, e);
  }
}

// ---- rows mode (flags & 2): 2-D copy whose inner dim is contiguous on both
// sides (column shards, narrowed views).  Work unit = one vector of `vw` bytes
// (vw = flags >> 8, the widest power of two dividing the row length, both row
// strides and both base addresses); the tile range indexes the flattened
// (row, vector) space so long and short rows balance the same way.
template <int VW>
__device__ void copy_rows(const CopyDesc& d, int64_t begin, int64_t end, int es) {
  using V = typename RawT<VW>::T;
  const int64_t vpr = d.sizes[1] * es / VW;  // vectors per row
  const int64_t s_row = d.src_strides[0] * es, d_row = d.dst_strides[0] * es;
  for (int64_t v = begin + threadIdx.x; v < end; v += kBlock) {
    const int64_t r = v / vpr, c = v - r * vpr;
    const V* s = reinterpret_cast<const V*>(d.src + r * s_row) + c;
    V* o = reinterpret_cast<V*>(d.dst + r * d_row) + c;
    *o = *s;
  }
}

// ---- transpose mode (flags & 4): canonical [B, I, J] with src contiguous along
// I and dst contiguous along J.  64x64 tiles staged through LDS (padded to 65
// words per row: conflict-free column reads), loads coalesced along I, stores
// coalesced along J.  A tile range is a range of 64x64 blocks.
template <int ES>
__device__ void transpose_blocks(const CopyDesc& d, int64_t begin, int64_t end, char* lds_raw) {
  using T = typename RawT<ES>::T;
  using W = typename std::conditional<ES == 8, uint64_t, uint32_t>::type;
  W(*lds)[65] = reinterpret_cast<W(*)[65]>(lds_raw);
  const int64_t I = d.sizes[1], J = d.sizes[2];
  const int64_t ti_n = (I + 63) / 64, tj_n = (J + 63) / 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int64_t blk = begin; blk < end; ++blk) {
    const int64_t b = blk / (ti_n * tj_n);
    const int64_t rr = blk - b * (ti_n * tj_n);
    const int64_t i0 = (rr / tj_n) * 64, j0 = (rr % tj_n) * 64;
    const T* src = reinterpret_cast<const T*>(d.src) + b * d.src_strides[0];
    T* dst = reinterpret_cast<T*>(d.dst) + b * d.dst_strides[0];
    const int64_t sj = d.src_strides[2], di = d.dst_strides[1];
#pragma unroll 4
    for (int jj = ty; jj < 64; jj += kBlock / 64) {
      const int64_t i = i0 + tx, j = j0 + jj;
      if (i < I && j < J) lds[jj][tx] = static_cast<W>(src[i + j * sj]);
    }
    __syncthreads();
#pragma unroll 4
    for (int ii = ty; ii < 64; ii += kBlock / 64) {
      const int64_t i = i0 + ii, j = j0 + tx;
      if (i < I && j < J) dst[i * di + j] = static_cast<T>(lds[tx][ii]);
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kBlock)
hs_copy_nd(const CopyDesc* __restrict__ descs, const Tile* __restrict__ tiles, int64_t ntiles) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const Tile tile = tiles[t];
    const CopyDesc& d = descs[tile.desc];
    if (d.flags & 1) {
      copy_bytes(d.src, d.dst, tile.begin, tile.end);
    } else if (d.flags & 2) {
      const int es = elem_size(d.src_dtype);
      switch (d.flags >> 8) {
        case 16: copy_rows<16>(d, tile.begin, tile.end, es); break;
        case 8: copy_rows<8>(d, tile.begin, tile.end, es); break;
        case 4: copy_rows<4>(d, tile.begin, tile.end, es); break;
        case 2: copy_rows<2>(d, tile.begin, tile.end, es); break;
        default: copy_rows<1>(d, tile.begin, tile.end, es); break;
      }
    } else if (d.flags & 4) {
      switch (elem_size(d.src_dtype)) {
        case 1: transpose_blocks<1>(d, tile.begin, tile.end, lds_raw); break;
        case 2: transpose_blocks<2>(d, tile.begin, tile.end, lds_raw); break;
        case 4: transpose_blocks<4>(d, tile.begin, tile.end, lds_raw); break;
        default: transpose_blocks<8>(d, tile.begin, tile.end, lds_raw); break;
      }
    } else {
      switch (d.ndim) {
        case 1: copy_tile_nd<1>(d, tile.begin, tile.end); break;
        case 2: copy_tile_nd<2>(d, tile.begin, tile.end); break;
        case 3: copy_tile_nd<3>(d, tile.begin, tile.end); break;
        case 4: copy_tile_nd<4>(d, tile.begin, tile.end); break;
        case 5: copy_tile_nd<5>(d, tile.begin, tile.end); break;
        case 6: copy_tile_nd<6>(d, tile.begin, tile.end); break;
        case 7: copy_tile_nd<7>(d, tile.begin, tile.end); break;
        default: copy_tile_nd<8>(d, tile.begin, tile.end); break;
      }
    }
  }
}

// Build the tile table for a descriptor batch.  Tile size adapts to the
// batch so that a launch always has >= ~4096 tiles when there is enough work
// (>> 256 CUs: every CU gets several 4-wave workgroups and enough loads in
// flight to reach HBM / PCIe bandwidth), and never below 32 KiB (tile-table
// overhead) or above 1 MiB.
int elem_bytes_host(int32_t dt) {
  switch (dt) {
    case kRaw1: return 1;
    case kRaw2: case kF16: case kBF16: return 2;
    case kRaw4: case kF32: return 4;
    case kRaw8: case kF64: return 8;
    default: return 16;
  }
}

void build_tiles(const CopyDesc* descs, int n, std::vector<Tile>* tiles) {
  int64_t total_bytes = 0;
  for (int i = 0; i < n; ++i) total_bytes += descs[i].numel * elem_bytes_host(descs[i].src_dtype);
  int64_t tile_bytes = total_bytes / 4096;
  tile_bytes = (tile_bytes + 16383) / 16384 * 16384;
  tile_bytes = std::max<int64_t>(32 << 10, std::min<int64_t>(kTileBytes, tile_bytes));
  for (int i = 0; i < n; ++i) {
    const CopyDesc& d = descs[i];
    const int es = elem_bytes_host(d.src_dtype);
    int64_t total, step;
    if (d.flags & 1) {
      total = d.numel * es;  // bytes
      step = tile_bytes;
    } else if (d.flags & 2) {
      const int vw = d.flags >> 8;
      total = d.sizes[0] * (d.sizes[1] * es / vw);  // vectors
      step = std::max<int64_t>(kBlock, tile_bytes / vw);
    } else if (d.flags & 4) {
      total = d.sizes[0] * ((d.sizes[1] + 63) / 64) * ((d.sizes[2] + 63) / 64);  // 64x64 blocks
      step = std::max<int64_t>(1, tile_bytes / (64 * 64 * es));
    } else {
      total = d.numel;
      // elements per tile on the strided/cast path (multiple of the per-block run)
      step = std::max<int64_t>(kBlock * 8, tile_bytes / es / (kBlock * 8) * (kBlock * 8));
    }
    for (int64_t b = 0; b < total; b += step) {
      tiles->push_back(Tile{i, 0, b, std::min(total, b + step)});
    }
  }
}

}  // namespace

const void* hs_copy_kernel() { return reinterpret_cast<const void*>(&hs_copy_nd); }

extern "C" {

uint64_t hsg_desc_size() { return sizeof(CopyDesc); }

// Batched strided copy / cast.  `descs` is a host array of `n` CopyDesc (see
// hipsnapshot/ops/native.py for the packing); `scratch` is a device (or
// host-mapped) workspace of at least hsg_copy_workspace_bytes() bytes used for
// the descriptor + tile tables (copied H2D on `stream`, so the host arrays may
// be reused as soon as this returns).  `stream` == null -> copy stream (dev,slot).
uint64_t hsg_copy_workspace_bytes(const void* descs, int n) {
  std::vector<Tile> tiles;
  build_tiles(static_cast<const CopyDesc*>(descs), n, &tiles);
  return sizeof(CopyDesc) * n + sizeof(Tile) * tiles.size() + 256;
}

int hsg_copy_nd(int dev, const void* descs, int n, void* workspace, uint64_t ws_bytes,
                void* pinned_stage, void* stream, int sync) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  std::vector<Tile> tiles;
  const CopyDesc* d = static_cast<const CopyDesc*>(descs);
  build_tiles(d, n, &tiles);
  if (tiles.empty()) return 0;
  const size_t dbytes = sizeof(CopyDesc) * n;
  const size_t tbytes = sizeof(Tile) * tiles.size();
  const size_t toff = (dbytes + 255) / 256 * 256;
  if (toff + tbytes > ws_bytes) {
    hs_set_error("workspace too small: need %zu have %llu", toff + tbytes,
                 (unsigned long long)ws_bytes);
    return -1000;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  // stage tables through pinned memory so the H2D is a true async DMA
  char* stage = static_cast<char*>(pinned_stage);
  std::memcpy(stage, d, dbytes);
  std::memcpy(stage + toff, tiles.data(), tbytes);
  char* ws = static_cast<char*>(workspace);
  HS_CHECK(hipMemcpyAsync(ws, stage, toff + tbytes, hipMemcpyHostToDevice, s));
  const int64_t ntiles = static_cast<int64_t>(tiles.size());
  int grid = static_cast<int>(std::min<int64_t>(ntiles, 256 * 8));
  const int cap = hsg_thread_grid_cap();
  if (cap > 0) grid = std::min(grid, cap);
  // dynamic LDS only when a transpose descriptor is present (64x65 words)
  size_t lds = 0;
  for (int i = 0; i < n; ++i) {
    if (d[i].flags & 4) {
      const size_t w = elem_bytes_host(d[i].src_dtype) == 8 ? 8 : 4;
      lds = std::max(lds, 64 * 65 * w);
    }
  }
  hipLaunchKernelGGL(hs_copy_nd, dim3(grid), dim3(kBlock), lds, s,
                     reinterpret_cast<const CopyDesc*>(ws),
                     reinterpret_cast<const Tile*>(ws + toff), ntiles);
  HS_CHECK(hipGetLastError());
  if (sync) HS_CHECK(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
