// hsquant: K5/K9 quantization kernels of the lossy checkpoint formats --
// blockwise OCP-fp8 (e4m3fn) with an f32 scale per block, MX fp8 (one E8M0
// scale byte per 32 elements) and Hadamard-rotated fp8 on the matrix cores --
// and their hsg_*quantize / hsg_*dequantize entry points.  Wave size is 64.

#include <algorithm>
#include <cstdint>

#include "hsgpu_common.h"

namespace {

// ---------------------------------------------------------------------------
// fp8 (OCP e4m3fn) blockwise quantization.  One 64-lane wave owns one block of
// `block` elements (block = 64 * VPT); amax via 64-wide xor-shuffle reduction,
// scale = max(amax / 448, 2^-126) (fp8_block_scale), payload via
// v_cvt_pk_fp8_f32 (gfx950: OCP encoding).
// ---------------------------------------------------------------------------

constexpr float kFp8Max = 448.0f;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Non-finite inputs of the blockwise (f32-scale) formats, as in the MX ones:
// they do not set their block's scale (|x| of inf / nan counts as 0), and
// their code is the e4m3fn NaN with the input's sign (torch's cast).  So one
// inf no longer turns every element of its block into NaN, and the GPU codes
// equal ops/quant.py's reference for every input.
__device__ __forceinline__ float finite_abs(float x) {
  const float a = fabsf(x);
  return a < __builtin_huge_valf() ? a : 0.f;
}

// Block scale of the f32-scale formats (plain and Hadamard): amax / 448,
// floored at the smallest normal float (2^-126), 1 for an all-zero block.
// Without the floor a block with amax below ~1.3e-36 gets a subnormal (or
// zero) scale whose reciprocal is inf: 0 * inf = NaN, and every non-zero
// saturates.  With it 1 / scale <= 2^126 is finite, |x| / scale < 448 inside
// a floored block, zeros stay zeros, and values below 2^-136 flush to zero:
// that is the format's floor.  Blocks with amax / 448 >= 2^-126 keep the scale
// and codes they always had.  ops/quant.py _scale_and_quant applies the same
// rule.
constexpr float kFp8MinScale = 0x1p-126f;

__device__ __forceinline__ float fp8_block_scale(float amax) {
  return amax > 0.f ? fmaxf(amax / kFp8Max, kFp8MinScale) : 1.f;
}

// `word` holds the codes of x[0..3] (byte j <- x[j]); j >= nvalid are left as is
__device__ __forceinline__ uint32_t fp8_fix_nonfinite(uint32_t word, const float* x,
                                                      int nvalid = 4) {
  uint32_t fix = 0, mask = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j >= nvalid) break;
    const uint32_t b = __float_as_uint(x[j]);
    if ((b & 0x7f800000u) == 0x7f800000u) {
      mask |= 0xffu << (8 * j);
      fix |= ((b >> 31) ? 0xffu : 0x7fu) << (8 * j);
    }
  }
  return (word & ~mask) | fix;
}

template <int VPT>
__global__ void __launch_bounds__(kBlock)
hs_fp8_quant(const char* __restrict__ src, int32_t src_dtype, int64_t n,
             uint8_t* __restrict__ out, float* __restrict__ scales) {
  constexpr int kBlk = 64 * VPT;
  const int lane = threadIdx.x & 63;
  const int64_t nblocks = (n + kBlk - 1) / kBlk;
  const int64_t wave0 = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const int ses = (src_dtype == kF32) ? 4 : 2;
  const bool out_aligned = (reinterpret_cast<uintptr_t>(out) & 3) == 0;  // 4-B stores below
  for (int64_t b = wave0; b < nblocks; b += nwaves) {
    const int64_t e0 = b * kBlk + int64_t(lane) * VPT;
    float v[VPT];
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int64_t e = e0 + j;
      v[j] = (e < n) ? load_as_f32(src + e * ses, src_dtype) : 0.f;
      amax = fmaxf(amax, finite_abs(v[j]));
    }
    amax = wave_max(amax);
    // two correctly rounded divisions per BLOCK (scale, then its reciprocal)
    // and one multiply per element -- the torch reference (ops/quant.py
    // _scale_and_quant) applies the same rule, so payloads are bit-identical;
    // a division per element made this kernel VALU-bound (profiles/pmc_r2)
    const float scale = fp8_block_scale(amax);
    const float inv = 1.f / scale;
    if (lane == 0) scales[b] = scale;
    uint32_t words[(VPT + 3) / 4];
#pragma unroll
    for (int w = 0; w < (VPT + 3) / 4; ++w) {
      float a0 = fminf(fmaxf(v[4 * w + 0] * inv, -kFp8Max), kFp8Max);
      float a1 = (4 * w + 1 < VPT) ? fminf(fmaxf(v[4 * w + 1] * inv, -kFp8Max), kFp8Max) : 0.f;
      float a2 = (4 * w + 2 < VPT) ? fminf(fmaxf(v[4 * w + 2] * inv, -kFp8Max), kFp8Max) : 0.f;
      float a3 = (4 * w + 3 < VPT) ? fminf(fmaxf(v[4 * w + 3] * inv, -kFp8Max), kFp8Max) : 0.f;
      int word = __builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, 0, false);
      word = __builtin_amdgcn_cvt_pk_fp8_f32(a2, a3, word, true);
      words[w] = fp8_fix_nonfinite(static_cast<uint32_t>(word), v + 4 * w,
                                   VPT - 4 * w < 4 ? VPT - 4 * w : 4);
    }
    if (out_aligned && e0 + VPT <= n && (VPT % 4) == 0) {
#pragma unroll
      for (int w = 0; w < VPT / 4; ++w)
        reinterpret_cast<uint32_t*>(out + e0)[w] = words[w];
    } else {
      for (int j = 0; j < VPT; ++j)
        if (e0 + j < n) out[e0 + j] = static_cast<uint8_t>(words[j >> 2] >> (8 * (j & 3)));
    }
  }
}

template <int VPT>
__global__ void __launch_bounds__(kBlock)
hs_fp8_dequant(const uint8_t* __restrict__ q, const float* __restrict__ scales, int64_t n,
               char* __restrict__ dst, int32_t dst_dtype) {
  constexpr int kBlk = 64 * VPT;
  const int des = (dst_dtype == kF32) ? 4 : (dst_dtype == kF64 ? 8 : 2);
  const int64_t nthreads = int64_t(gridDim.x) * kBlock;
  const bool q_aligned = (reinterpret_cast<uintptr_t>(q) & 3) == 0;  // 4-B loads below
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i * 4 < n; i += nthreads) {
    const int64_t e0 = i * 4;
    uint32_t word;
    if (q_aligned && e0 + 4 <= n) {
      word = reinterpret_cast<const uint32_t*>(q)[i];
    } else {
      word = 0;
      for (int j = 0; j < 4 && e0 + j < n; ++j) word |= uint32_t(q[e0 + j]) << (8 * j);
    }
    const float s = scales[e0 / kBlk];
    float f[4];
    f[0] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(word), 0);
    f[1] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(word), 1);
    f[2] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(word), 2);
    f[3] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(word), 3);
    for (int j = 0; j < 4 && e0 + j < n; ++j) store_from_f32(dst + (e0 + j) * des, dst_dtype, f[j] * s);
  }
}

// ---------------------------------------------------------------------------
// MX fp8: OCP e4m3fn elements + one E8M0 (power-of-two) scale byte per
// 32-element block.  Scale 2^k with the smallest k such that amax <= 448*2^k
// (exact, from frexp: amax = m*2^e, k = e-9 if m <= 0.875 else e-8), so
// x * 2^-k is exact (v_ldexp_f32, no division, no clamp needed) and restore is
// q * 2^k, exact in f32.  Streaming layout for the HBM roof:
//   * every 16-B load instruction is contiguous across the wave (lane l
//     reads bytes [16 l, 16 l + 16) of a 1 KiB wave segment), U = 4 of them in
//     flight per lane;
//   * a 32-element block spans LPB = 32 / (16 / es) lanes (4 for bf16/f16, 8
//     for f32): amax is an in-register max over the lane's 16 B then a
//     log2(LPB)-step xor-shuffle;
//   * fp8 bytes leave as one 8-B (bf16) / 4-B (f32) store per lane per load,
//     again contiguous across the wave.
// ---------------------------------------------------------------------------

constexpr int kMxBlock = 32;
typedef unsigned int mx_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int mx_u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float fp8_byte_to_f32(uint32_t w, int b) {
  switch (b) {  // the byte select must be an immediate
    case 0: return __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w), 0);
    case 1: return __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w), 1);
    case 2: return __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w), 2);
    default: return __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w), 3);
  }
}

__device__ __forceinline__ int mx_exp(float amax) {
  if (!(amax > 0.f) || !(amax < __builtin_huge_valf())) return 0;  // zero / inf / nan
  int e;
  const float m = frexpf(amax, &e);
  const int k = (m <= 0.875f) ? e - 9 : e - 8;
  return k < -127 ? -127 : (k > 127 ? 127 : k);
}

template <int DT>
__device__ __forceinline__ float mx_unpack(uint32_t w, int half) {
  if constexpr (DT == kBF16) return __uint_as_float(half ? (w & 0xffff0000u) : (w << 16));
  else {
    _Float16 h;
    const uint16_t b = static_cast<uint16_t>(half ? (w >> 16) : (w & 0xffffu));
    __builtin_memcpy(&h, &b, 2);
    return static_cast<float>(h);
  }
}

template <int DT>
__global__ void __launch_bounds__(kBlock)
hs_mx8_quant(const char* __restrict__ src, int64_t n, int64_t payload,
             uint8_t* __restrict__ out, uint8_t* __restrict__ scales) {
  constexpr int ES = (DT == kF32) ? 4 : 2;
  constexpr int EPL = 16 / ES;
  constexpr int LPB = kMxBlock / EPL;
  constexpr int U = 4;
  constexpr int64_t kChunk = 64LL * EPL * U;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  // wave-uniform: the 16-B loads of `src` and the EPL-byte stores of `out`
  // need their natural alignment (a view with a storage offset has neither);
  // a misaligned call takes the element path of the tail for every chunk
  const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                       (reinterpret_cast<uintptr_t>(out) & (EPL - 1)) == 0;
  for (int64_t c = wave0; c < nchunks; c += nwaves) {
    const int64_t base = c * kChunk;
    const bool full = aligned && base + kChunk <= n;
    uint4 raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      if (full) {
        const mx_u32x4 t =
            __builtin_nontemporal_load(reinterpret_cast<const mx_u32x4*>(src + e0 * ES));
        raw[u] = make_uint4(t.x, t.y, t.z, t.w);
      } else {
        uint32_t w[4] = {0, 0, 0, 0};
        for (int j = 0; j < EPL; ++j) {
          if (e0 + j >= n) break;
          uint32_t bits;
          if constexpr (ES == 4) bits = *reinterpret_cast<const uint32_t*>(src + (e0 + j) * 4);
          else bits = *reinterpret_cast<const uint16_t*>(src + (e0 + j) * 2);
          w[(j * ES) >> 2] |= bits << (((j * ES) & 3) * 8);
        }
        raw[u] = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t ws[4] = {raw[u].x, raw[u].y, raw[u].z, raw[u].w};
      float v[EPL];
#pragma unroll
      for (int j = 0; j < EPL; ++j) {
        if constexpr (ES == 4) v[j] = __uint_as_float(ws[j]);
        else v[j] = mx_unpack<DT>(ws[j >> 1], j & 1);
      }
      float amax = 0.f;  // over the finite elements (inf / nan do not set the scale)
#pragma unroll
      for (int j = 0; j < EPL; ++j) {
        const float a = fabsf(v[j]);
        amax = fmaxf(amax, a < __builtin_huge_valf() ? a : 0.f);
      }
#pragma unroll
      for (int o = 1; o < LPB; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
      const int k = mx_exp(amax);
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      if ((lane % LPB) == 0 && e0 < n) scales[e0 / kMxBlock] = static_cast<uint8_t>(k + 127);
      uint32_t q[EPL / 4];
#pragma unroll
      for (int w = 0; w < EPL / 4; ++w) {
        int word = __builtin_amdgcn_cvt_pk_fp8_f32(ldexpf(v[4 * w], -k), ldexpf(v[4 * w + 1], -k),
                                                   0, false);
        word = __builtin_amdgcn_cvt_pk_fp8_f32(ldexpf(v[4 * w + 2], -k),
                                               ldexpf(v[4 * w + 3], -k), word, true);
        // non-finite elements: e4m3fn NaN with the element's sign (torch's cast)
        uint32_t fix = 0, fixmask = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t b = __float_as_uint(v[4 * w + j]);
          if ((b & 0x7f800000u) == 0x7f800000u) {
            fixmask |= 0xffu << (8 * j);
            fix |= ((b >> 31) ? 0xffu : 0x7fu) << (8 * j);
          }
        }
        q[w] = (static_cast<uint32_t>(word) & ~fixmask) | fix;
      }
      if (full) {
        if constexpr (EPL == 8) {
          mx_u32x2 t;
          t.x = q[0];
          t.y = q[1];
          __builtin_nontemporal_store(t, reinterpret_cast<mx_u32x2*>(out + e0));
        } else
          __builtin_nontemporal_store(q[0], reinterpret_cast<uint32_t*>(out + e0));
      } else {
        for (int j = 0; j < EPL; ++j) {
          const int64_t e = e0 + j;
          if (e < payload) out[e] = e < n ? static_cast<uint8_t>(q[j >> 2] >> (8 * (j & 3))) : 0;
        }
      }
    }
  }
}

template <int DT>
__device__ __forceinline__ void mx_store(char* p, const float* f) {
  // 16 B of output: 8 x bf16/f16, 4 x f32 or 2 x f64
  if constexpr (DT == kF32) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  } else if constexpr (DT == kF64) {
    *reinterpret_cast<double2*>(p) = make_double2(static_cast<double>(f[0]),
                                                  static_cast<double>(f[1]));
  } else {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint16_t lo, hi;
      if constexpr (DT == kBF16) {
        lo = f32_to_bf16(f[2 * i]);
        hi = f32_to_bf16(f[2 * i + 1]);
      } else {
        const _Float16 a = static_cast<_Float16>(f[2 * i]), b = static_cast<_Float16>(f[2 * i + 1]);
        __builtin_memcpy(&lo, &a, 2);
        __builtin_memcpy(&hi, &b, 2);
      }
      w[i] = uint32_t(lo) | (uint32_t(hi) << 16);
    }
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

template <int DT>
__global__ void __launch_bounds__(kBlock)
hs_mx8_dequant(const uint8_t* __restrict__ q, const uint8_t* __restrict__ scales, int64_t n,
               char* __restrict__ dst) {
  constexpr int DES = (DT == kF32) ? 4 : (DT == kF64 ? 8 : 2);
  constexpr int EPL = 16 / DES;  // fp8 bytes per lane per step = one 16-B store
  constexpr int U = 4;
  constexpr int64_t kChunk = 64LL * EPL * U;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  // wave-uniform: the EPL-byte loads of `q` and the 16-B stores of `dst` need
  // their natural alignment; a misaligned call takes the element path
  const bool aligned = (reinterpret_cast<uintptr_t>(q) & (EPL - 1)) == 0 &&
                       (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  for (int64_t c = wave0; c < nchunks; c += nwaves) {
    const int64_t base = c * kChunk;
    const bool full = aligned && base + kChunk <= n;
    uint32_t raw[U][(EPL + 3) / 4];
    uint8_t sb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      if (full) {
        if constexpr (EPL == 8) {
          const uint2 t = *reinterpret_cast<const uint2*>(q + e0);
          raw[u][0] = t.x;
          raw[u][1] = t.y;
        } else if constexpr (EPL == 4) {
          raw[u][0] = *reinterpret_cast<const uint32_t*>(q + e0);
        } else {
          raw[u][0] = *reinterpret_cast<const uint16_t*>(q + e0);
        }
      } else {
        for (int w = 0; w < (EPL + 3) / 4; ++w) raw[u][w] = 0;
        for (int j = 0; j < EPL && e0 + j < n; ++j)
          raw[u][j >> 2] |= uint32_t(q[e0 + j]) << (8 * (j & 3));
      }
      sb[u] = e0 < n ? scales[e0 / kMxBlock] : 127;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      const int k = int(sb[u]) - 127;
      float f[EPL];
#pragma unroll
      for (int j = 0; j < EPL; ++j)
        f[j] = ldexpf(fp8_byte_to_f32(raw[u][j >> 2], j & 3), k);
      if (full) {
        mx_store<DT>(dst + e0 * DES, f);
      } else {
        for (int j = 0; j < EPL && e0 + j < n; ++j) store_from_f32(dst + (e0 + j) * DES, DT, f[j]);
      }
    }
  }
}

// Blockwise fp8 restore in the same streaming layout (hs_mx8_dequant's):
// lane l reads EPL = 16 / dst-element-size codes and writes 16 B, U = 4 in
// flight; x = f32(q) * scale[e / BLK] (the scale is per lane: BLK % EPL == 0).
template <int DT, int BLK>
__global__ void __launch_bounds__(kBlock)
hs_fp8_dequant_v(const uint8_t* __restrict__ q, const float* __restrict__ scales, int64_t n,
                 char* __restrict__ dst) {
  constexpr int DES = (DT == kF32) ? 4 : (DT == kF64 ? 8 : 2);
  constexpr int EPL = 16 / DES;
  constexpr int U = 4;
  constexpr int64_t kChunk = 64LL * EPL * U;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  for (int64_t c = wave0; c < nchunks; c += nwaves) {
    const int64_t base = c * kChunk;
    const bool full = base + kChunk <= n;
    uint32_t raw[U][(EPL + 3) / 4];
    float sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      if (full) {
        if constexpr (EPL == 8) {
          const uint2 t = *reinterpret_cast<const uint2*>(q + e0);
          raw[u][0] = t.x;
          raw[u][1] = t.y;
        } else if constexpr (EPL == 4) {
          raw[u][0] = *reinterpret_cast<const uint32_t*>(q + e0);
        } else {
          raw[u][0] = *reinterpret_cast<const uint16_t*>(q + e0);
        }
      } else {
        for (int w = 0; w < (EPL + 3) / 4; ++w) raw[u][w] = 0;
        for (int j = 0; j < EPL && e0 + j < n; ++j)
          raw[u][j >> 2] |= uint32_t(q[e0 + j]) << (8 * (j & 3));
      }
      sc[u] = e0 < n ? scales[e0 / BLK] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      float f[EPL];
#pragma unroll
      for (int j = 0; j < EPL; ++j) f[j] = fp8_byte_to_f32(raw[u][j >> 2], j & 3) * sc[u];
      if (full) {
        mx_store<DT>(dst + e0 * DES, f);
      } else {
        for (int j = 0; j < EPL && e0 + j < n; ++j) store_from_f32(dst + (e0 + j) * DES, DT, f[j]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Blockwise fp8 (f32 scale per BLK elements, format "fp8_e4m3fn_block") in the
// streaming layout of hs_mx8_quant: lane l of a wave reads 16 contiguous bytes
// (EPL elements) of a 1 KiB wave segment, U = 4 segments in flight per lane,
// a block spans LPB = BLK / EPL adjacent lanes (amax: log2(LPB) xor shuffles),
// and each lane stores its EPL fp8 codes with one vector store.  Same numerics
// as hs_fp8_quant: scale = fp8_block_scale(amax), q = cvt(clamp(x * (1 /
// scale))).  hs_fp8_quant (one block per wave, two 2-B loads per lane) ran at
// 1.9 TB/s: too little in flight per wave.
// ---------------------------------------------------------------------------

template <int DT, int BLK>
__global__ void __launch_bounds__(kBlock)
hs_fp8_quant_v(const char* __restrict__ src, int64_t n, uint8_t* __restrict__ out,
               float* __restrict__ scales) {
  constexpr int ES = (DT == kF32) ? 4 : 2;
  constexpr int EPL = 16 / ES;
  constexpr int LPB = BLK / EPL;
  static_assert(LPB >= 1 && LPB <= 64 && (64 % LPB) == 0, "block must fit a wave");
  constexpr int U = 4;
  constexpr int64_t kChunk = 64LL * EPL * U;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  for (int64_t c = wave0; c < nchunks; c += nwaves) {
    const int64_t base = c * kChunk;
    const bool full = base + kChunk <= n;
    uint4 raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      if (full) {
        const mx_u32x4 t =
            __builtin_nontemporal_load(reinterpret_cast<const mx_u32x4*>(src + e0 * ES));
        raw[u] = make_uint4(t.x, t.y, t.z, t.w);
      } else {
        uint32_t w[4] = {0, 0, 0, 0};
        for (int j = 0; j < EPL; ++j) {
          if (e0 + j >= n) break;
          uint32_t bits;
          if constexpr (ES == 4) bits = *reinterpret_cast<const uint32_t*>(src + (e0 + j) * 4);
          else bits = *reinterpret_cast<const uint16_t*>(src + (e0 + j) * 2);
          w[(j * ES) >> 2] |= bits << (((j * ES) & 3) * 8);
        }
        raw[u] = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t ws[4] = {raw[u].x, raw[u].y, raw[u].z, raw[u].w};
      float v[EPL];
#pragma unroll
      for (int j = 0; j < EPL; ++j) {
        if constexpr (ES == 4) v[j] = __uint_as_float(ws[j]);
        else v[j] = mx_unpack<DT>(ws[j >> 1], j & 1);
      }
      float amax = 0.f;
#pragma unroll
      for (int j = 0; j < EPL; ++j) amax = fmaxf(amax, finite_abs(v[j]));
#pragma unroll
      for (int o = 1; o < LPB; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
      const float scale = fp8_block_scale(amax);
      const float inv = 1.f / scale;
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      if ((lane % LPB) == 0 && e0 < n) scales[e0 / BLK] = scale;
      uint32_t q[EPL / 4];
#pragma unroll
      for (int w = 0; w < EPL / 4; ++w) {
        int word = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(v[4 * w] * inv, -kFp8Max), kFp8Max),
                                                   fminf(fmaxf(v[4 * w + 1] * inv, -kFp8Max), kFp8Max),
                                                   0, false);
        word = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(v[4 * w + 2] * inv, -kFp8Max), kFp8Max),
                                               fminf(fmaxf(v[4 * w + 3] * inv, -kFp8Max), kFp8Max),
                                               word, true);
        q[w] = fp8_fix_nonfinite(static_cast<uint32_t>(word), v + 4 * w);
      }
      if (full) {
        if constexpr (EPL == 8) {
          mx_u32x2 t;
          t.x = q[0];
          t.y = q[1];
          __builtin_nontemporal_store(t, reinterpret_cast<mx_u32x2*>(out + e0));
        } else {
          __builtin_nontemporal_store(q[0], reinterpret_cast<uint32_t*>(out + e0));
        }
      } else {
        for (int j = 0; j < EPL && e0 + j < n; ++j)
          out[e0 + j] = static_cast<uint8_t>(q[j >> 2] >> (8 * (j & 3)));
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Hadamard-rotated fp8 (MFMA).  The flat tensor is viewed as rows of 32
// ("groups"); every group is rotated by the 32x32 Sylvester Hadamard matrix H
// (entries +-1, H*H = 32 I) before blockwise e4m3 quantization, which spreads
// outliers across the group and cuts fp8 error on heavy-tailed weights.
//
// One wave owns a tile of 32 groups (1024 elements) and computes
// Y[32x32] = X[32x32] * H with 16 x v_mfma_f32_32x32x2_f32 (exact f32 inputs,
// k-ordered fmaf chain -> bit-reproducible by a sequential fp32 reference).
// Operand maps (CDNA guide 3): lane l, r = l&31, h = l>>5:
//   A[i=r][k=h] per instruction t -> X[row r][2t+h];  B[k=h][j=r] -> H[2t+h][r]
//   C/D reg i -> row (i&3) + 8(i>>2) + 4h, col r
// so register quad g4 of lane-half h is exactly quantization block 2*g4+h of
// the tile (4 rows x 32 cols = 128 elements): amax = 4 regs + xor-shuffle over
// the 32 lanes of the half.  Restore inverts with X = (Y' * H) / 32.
// ---------------------------------------------------------------------------

typedef float floatx16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float hada(int k, int c) {
  return (__popc(k & c) & 1) ? -1.f : 1.f;
}

// Half-row operand layout: lane (r, h) owns X[r][16h .. 16h + 15] -- 32 B
// (bf16/f16) or 64 B (f32) contiguous in memory, loaded with 16-B vector
// loads -- and MFMA step t contracts k = t (h = 0 lanes) and k = 16 + t
// (h = 1 lanes): the accumulation order is k = 0, 16, 1, 17, ..., 15, 31
// (``ops/quant.py`` HADAMARD_K_ORDER; the torch reference sums in the same
// order, so the blobs stay bit-identical).
template <int DT>
__device__ __forceinline__ void load_half_row(const char* src, int64_t e0, int64_t n, float* x) {
  constexpr int ES = (DT == kF32) ? 4 : 2;
  if (e0 + 16 <= n && ((reinterpret_cast<uintptr_t>(src + e0 * ES) & 15) == 0)) {
    const uint4* v = reinterpret_cast<const uint4*>(src + e0 * ES);
    if constexpr (ES == 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint4 w = v[q];
        x[4 * q] = __uint_as_float(w.x);
        x[4 * q + 1] = __uint_as_float(w.y);
        x[4 * q + 2] = __uint_as_float(w.z);
        x[4 * q + 3] = __uint_as_float(w.w);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const uint4 w = v[q];
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          x[8 * q + 2 * i] = mx_unpack<DT>(ws[i], 0);
          x[8 * q + 2 * i + 1] = mx_unpack<DT>(ws[i], 1);
        }
      }
    }
  } else {
#pragma unroll
    for (int t = 0; t < 16; ++t)
      x[t] = (e0 + t < n) ? load_as_f32(src + (e0 + t) * ES, DT) : 0.f;
  }
}

// max over the 32 lanes of a wave half: quad xor-1 / xor-2 and the 8- and
// 16-lane mirrors on DPP (no LDS traffic), one ds_bpermute for lane ^ 16
__device__ __forceinline__ float max_over_32(float v) {
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, false)));
  return fmaxf(v, __shfl_xor(v, 16, 64));
}

template <int DT>
__global__ void __launch_bounds__(kBlock)
hs_fp8_hadamard_quant(const char* __restrict__ src, int64_t n, int64_t n_pad,
                      uint8_t* __restrict__ out, float* __restrict__ scales) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  const int64_t ntiles = (n_pad + 1023) / 1024;
  const int64_t nblocks = (n_pad + 127) / 128;
  const int64_t wave0 = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  // (prefetching the next tile's half rows before the MFMA chain was tried:
  // 100 VGPRs instead of 48, no faster -- profiles/r3/s2/fp8_host_timed_callE.jsonl)
  for (int64_t tile = wave0; tile < ntiles; tile += nwaves) {
    float x[16];
    load_half_row<DT>(src, (tile * 32 + r) * 32 + 16 * h, n, x);
    floatx16 acc = {};
#pragma unroll
    for (int t = 0; t < 16; ++t)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[t], hada(16 * h + t, r), acc, 0, 0, 0);
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      float amax = fmaxf(fmaxf(finite_abs(acc[4 * g4]), finite_abs(acc[4 * g4 + 1])),
                         fmaxf(finite_abs(acc[4 * g4 + 2]), finite_abs(acc[4 * g4 + 3])));
      amax = max_over_32(amax);
      const float scale = fp8_block_scale(amax);
      const float inv = 1.f / scale;
      const int64_t blk = tile * 8 + 2 * g4 + h;
      if (r == 0 && blk < nblocks) scales[blk] = scale;
      float v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = fminf(fmaxf(acc[4 * g4 + q] * inv, -kFp8Max), kFp8Max);
      // byte q of `w` = row q + 8 g4 + 4 h, column r.  A 4x4 byte transpose
      // over each quad of lanes (two DPP quad-perm exchanges + v_perm_b32)
      // leaves lane r with row (r & 3) + 8 g4 + 4 h, columns (r & ~3) .. +3:
      // one 4-B store per lane, 256 contiguous bytes per wave instruction,
      // instead of 4 one-byte stores.
      uint32_t w = static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false));
      w = static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], static_cast<int>(w), true));
      {
        const float a4[4] = {acc[4 * g4], acc[4 * g4 + 1], acc[4 * g4 + 2], acc[4 * g4 + 3]};
        w = fp8_fix_nonfinite(w, a4);
      }
      uint32_t o = static_cast<uint32_t>(
          __builtin_amdgcn_mov_dpp(static_cast<int>(w), 0xB1, 0xF, 0xF, false));  // lane ^ 1
      w = __builtin_amdgcn_perm(o, w, (r & 1) ? 0x03070105u : 0x06020400u);
      o = static_cast<uint32_t>(
          __builtin_amdgcn_mov_dpp(static_cast<int>(w), 0x4E, 0xF, 0xF, false));  // lane ^ 2
      w = __builtin_amdgcn_perm(o, w, (r & 2) ? 0x03020706u : 0x05040100u);
      const int64_t row0 = (tile * 32 + (r & 3) + 8 * g4 + 4 * h) * 32;
      if (row0 < n_pad) *reinterpret_cast<uint32_t*>(out + row0 + (r & ~3)) = w;
    }
  }
}

// 16-bit inputs (bf16 / f16): the same rotation on the 16-bit MFMA,
// v_mfma_f32_32x32x16_{bf16,f16}: K = 16 per instruction, so a 32x32 tile
// takes 2 MFMAs instead of 16 f32 ones (~64 matrix-pipe cycles per KiB of
// output instead of ~256, which no longer hide under the tile's HBM traffic).
// The +-1 entries and the 16-bit inputs are exact; the products are summed
// inside the MFMA in fp32, in the hardware's own order, so a result can differ
// from the k-ordered fp32 reference in its last bit (tests bound the fp8 codes).
// Operand maps (CDNA guide 3, 32x32x16): lane l, r = l&31, h = l>>5 holds
//   A[row r][k = 8h + j], B[k = 8h + j][col r], j = 0..7, per K-step s (+16 s)
// i.e. the A fragment of step s is the 16 contiguous bytes X[r][16s + 8h ..+7]:
// one 16-B load, and the two loads of a wave cover the tile's 2 KiB exactly.
// C/D is the f32 form's map, so the epilogue is the one above.
typedef short hs_i16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 hs_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 hs_f16x8 __attribute__((ext_vector_type(8)));

template <int DT>
__device__ __forceinline__ floatx16 mfma16(hs_i16x8 a, hs_i16x8 b, floatx16 c) {
  if constexpr (DT == kBF16)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(hs_bf16x8, a),
                                                   __builtin_bit_cast(hs_bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(hs_f16x8, a),
                                                  __builtin_bit_cast(hs_f16x8, b), c, 0, 0, 0);
}

template <int DT>
__device__ __forceinline__ hs_i16x8 load_a_frag(const char* src, int64_t e0, int64_t n) {
  hs_i16x8 a;
  if (e0 + 8 <= n && ((reinterpret_cast<uintptr_t>(src + e0 * 2) & 15) == 0)) {
    const mx_u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const mx_u32x4*>(src + e0 * 2));
    a = __builtin_bit_cast(hs_i16x8, t);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      a[j] = (e0 + j < n) ? *reinterpret_cast<const short*>(src + (e0 + j) * 2) : short(0);
  }
  return a;
}

// Epilogue of one rotated tile: blockwise scales + e4m3 codes (see above).
__device__ __forceinline__ void hadamard_tile_store(const floatx16& acc, int64_t tile, int r,
                                                    int h, int64_t n_pad, int64_t nblocks,
                                                    uint8_t* __restrict__ out,
                                                    float* __restrict__ scales) {
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    float amax = fmaxf(fmaxf(finite_abs(acc[4 * g4]), finite_abs(acc[4 * g4 + 1])),
                       fmaxf(finite_abs(acc[4 * g4 + 2]), finite_abs(acc[4 * g4 + 3])));
    amax = max_over_32(amax);
    const float scale = fp8_block_scale(amax);
    const float inv = 1.f / scale;
    const int64_t blk = tile * 8 + 2 * g4 + h;
    if (r == 0 && blk < nblocks) scales[blk] = scale;
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = fminf(fmaxf(acc[4 * g4 + q] * inv, -kFp8Max), kFp8Max);
    uint32_t w = static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false));
    w = static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], static_cast<int>(w), true));
    {
      const float a4[4] = {acc[4 * g4], acc[4 * g4 + 1], acc[4 * g4 + 2], acc[4 * g4 + 3]};
      w = fp8_fix_nonfinite(w, a4);
    }
    uint32_t o = static_cast<uint32_t>(
        __builtin_amdgcn_mov_dpp(static_cast<int>(w), 0xB1, 0xF, 0xF, false));  // lane ^ 1
    w = __builtin_amdgcn_perm(o, w, (r & 1) ? 0x03070105u : 0x06020400u);
    o = static_cast<uint32_t>(
        __builtin_amdgcn_mov_dpp(static_cast<int>(w), 0x4E, 0xF, 0xF, false));  // lane ^ 2
    w = __builtin_amdgcn_perm(o, w, (r & 2) ? 0x03020706u : 0x05040100u);
    const int64_t row0 = (tile * 32 + (r & 3) + 8 * g4 + 4 * h) * 32;
    if (row0 < n_pad) __builtin_nontemporal_store(w, reinterpret_cast<uint32_t*>(out + row0 + (r & ~3)));
  }
}

// U tiles per iteration (2 A-fragment loads each): 2U 16-B loads in flight
// per lane before the first MFMA (one tile per iteration ran at 4.2 TB/s,
// latency-bound with 2 loads in flight).
template <int DT, int U>
__global__ void __launch_bounds__(kBlock)
hs_fp8_hadamard_quant16(const char* __restrict__ src, int64_t n, int64_t n_pad,
                        uint8_t* __restrict__ out, float* __restrict__ scales) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  const int64_t ntiles = (n_pad + 1023) / 1024;
  const int64_t nblocks = (n_pad + 127) / 128;
  const int64_t wave0 = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  // B fragments: H[16 s + 8 h + j][r] as 16-bit +-1 (bf16 0x3F80/0xBF80, f16 0x3C00/0xBC00)
  const short one = (DT == kBF16) ? short(0x3F80) : short(0x3C00);
  hs_i16x8 b0, b1;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    b0[j] = (__popc((8 * h + j) & r) & 1) ? short(one | 0x8000) : one;
    b1[j] = (__popc((16 + 8 * h + j) & r) & 1) ? short(one | 0x8000) : one;
  }
  // wave-uniform fast path: every load of the U tiles in bounds and 16-B
  // aligned -> 2U vector loads issued back to back (a per-load bounds branch
  // made the compiler wait for each load before the next one)
  const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  for (int64_t t0 = wave0 * U; t0 < ntiles; t0 += nwaves * U) {
    hs_i16x8 a[U][2];
    if (aligned && (t0 + U) * 1024 <= n) {
      const mx_u32x4* p = reinterpret_cast<const mx_u32x4*>(src) + ((t0 * 32 + r) * 32 + 8 * h) / 8;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a[u][0] = __builtin_bit_cast(hs_i16x8, __builtin_nontemporal_load(p + u * 128));
        a[u][1] = __builtin_bit_cast(hs_i16x8, __builtin_nontemporal_load(p + u * 128 + 2));
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t e0 = ((t0 + u) * 32 + r) * 32 + 8 * h;  // past the end: zeros
        a[u][0] = load_a_frag<DT>(src, e0, n);
        a[u][1] = load_a_frag<DT>(src, e0 + 16, n);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (t0 + u >= ntiles) break;
      floatx16 acc = {};
      acc = mfma16<DT>(a[u][0], b0, acc);
      acc = mfma16<DT>(a[u][1], b1, acc);
      hadamard_tile_store(acc, t0 + u, r, h, n_pad, nblocks, out, scales);
    }
  }
}

// Dequantization on the matrix cores: X = (Q H) * s / 32 with Q the e4m3
// codes widened to bf16 (exact: 3 mantissa bits, exponents -9..8) and fed to
// v_mfma_f32_32x32x16_bf16 (2 per tile).  Every e4m3 value is a multiple of
// 2^-9 below 448, so a row sum of 32 of them (|sum| < 2^14) is exact in fp32
// whatever order the MFMA adds in: the only rounding is the product with the
// block scale (the /32 is exact) -- ``ops/quant.py`` computes the same, so GPU
// and CPU restores of a blob are bit-identical.  (The fp8 MFMA,
// v_mfma_f32_32x32x16_fp8_fp8, is not used: on a 65 613-element test its
// sums differed from the exact ones in the last bit -- subnormal e4m3 inputs
// are the suspect.)
// Operands (lane l, r = l&31, h = l>>5): the lane's 16 contiguous codes of
// row r, k = 16h .. 16h+15, are its A fragments of steps 0 and 1 (k = 16h +
// 8s + j); B holds H[16h + 8s + j][r] (bf16 +-1).  C/D as the quant kernels:
// register quad g4 = rows 8g4 + 4h + 0..3, column r, one block scale.
// 16-bit destinations leave through a 4x4 lane-quad transpose (3 DPP moves
// per quad) as 8-B stores, 256 contiguous bytes per wave instruction.
// 8 e4m3 codes (two words) -> 8 bf16 (exact: the f32 value's upper half)
__device__ __forceinline__ hs_i16x8 fp8x8_to_bf16x8(uint32_t w0, uint32_t w1) {
  hs_i16x8 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j] = static_cast<short>(__float_as_uint(fp8_byte_to_f32(w0, j)) >> 16);
    o[4 + j] = static_cast<short>(__float_as_uint(fp8_byte_to_f32(w1, j)) >> 16);
  }
  return o;
}

template <int DT>
__device__ __forceinline__ uint32_t pack16(float lo, float hi) {
  uint32_t a, b;
  if constexpr (DT == kBF16) {
    a = f32_to_bf16(lo);
    b = f32_to_bf16(hi);
  } else {
    asm volatile("" : "+v"(lo), "+v"(hi));  // f32 products, then RNE (store_from_f32)
    a = __builtin_bit_cast(uint16_t, static_cast<_Float16>(lo));
    b = __builtin_bit_cast(uint16_t, static_cast<_Float16>(hi));
  }
  return a | (b << 16);
}

template <int DT, int U>
__global__ void __launch_bounds__(kBlock)
hs_fp8_hadamard_dequant8(const uint8_t* __restrict__ q, const float* __restrict__ scales,
                         int64_t n, int64_t n_pad, char* __restrict__ dst) {
  constexpr int DES = (DT == kF32) ? 4 : (DT == kF64 ? 8 : 2);
  const int lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  const int64_t ntiles = (n_pad + 1023) / 1024;
  const int64_t wave0 = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  hs_i16x8 b0, b1;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    b0[j] = (__popc((16 * h + j) & r) & 1) ? short(0xBF80) : short(0x3F80);
    b1[j] = (__popc((16 * h + 8 + j) & r) & 1) ? short(0xBF80) : short(0x3F80);
  }
  const bool vec_out = (DES == 2) && (reinterpret_cast<uintptr_t>(dst) & 7) == 0;
  // wave-uniform: the 16-B loads of `q` need a 16-B aligned payload (e0 is a
  // multiple of 16); a misaligned one is read byte by byte
  const bool q_aligned = (reinterpret_cast<uintptr_t>(q) & 15) == 0;
  for (int64_t t0 = wave0 * U; t0 < ntiles; t0 += nwaves * U) {
    mx_u32x4 a[U];
    float sc[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // q holds n_pad bytes (a multiple of 32)
      const int64_t e0 = ((t0 + u) * 32 + r) * 32 + 16 * h;
      if (q_aligned) {
        a[u] = (e0 + 16 <= n_pad) ? __builtin_nontemporal_load(reinterpret_cast<const mx_u32x4*>(q + e0))
                                  : mx_u32x4{0, 0, 0, 0};
      } else {
        a[u] = mx_u32x4{0, 0, 0, 0};
        if (e0 + 16 <= n_pad) {
#pragma unroll
          for (int j = 0; j < 16; ++j) a[u][j >> 2] |= uint32_t(q[e0 + j]) << (8 * (j & 3));
        }
      }
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int64_t blk = (t0 + u) * 8 + 2 * g4 + h;
        sc[u][g4] = (blk * 128 < n_pad) ? scales[blk] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t tile = t0 + u;
      if (tile >= ntiles) break;
      floatx16 acc = {};
      acc = mfma16<kBF16>(fp8x8_to_bf16x8(a[u].x, a[u].y), b0, acc);
      acc = mfma16<kBF16>(fp8x8_to_bf16x8(a[u].z, a[u].w), b1, acc);
      if (vec_out && (tile + 1) * 1024 <= n) {
        if constexpr (DES == 2) {
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const float s = sc[u][g4] * (1.f / 32.f);
            // lane slot i = row 8 g4 + 4 h + i, column r (two 16-bit rows per word)
            uint32_t A = pack16<DT>(acc[4 * g4] * s, acc[4 * g4 + 1] * s);
            uint32_t B = pack16<DT>(acc[4 * g4 + 2] * s, acc[4 * g4 + 3] * s);
            // stage 1 (lanes ^ 1): 2x2 transposes of 16-bit elements
            const uint32_t A1 = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(A), 0xB1, 0xF, 0xF, false));
            const uint32_t B1 = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(B), 0xB1, 0xF, 0xF, false));
            if (r & 1) {
              A = __builtin_amdgcn_perm(A, A1, 0x07060302u);  // (partner.hi, mine.hi)
              B = __builtin_amdgcn_perm(B, B1, 0x07060302u);
            } else {
              A = __builtin_amdgcn_perm(A1, A, 0x05040100u);  // (mine.lo, partner.lo)
              B = __builtin_amdgcn_perm(B1, B, 0x05040100u);
            }
            // stage 2 (lanes ^ 2): swap 32-bit words
            const uint32_t X = (r & 2) ? A : B;
            const uint32_t R = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(X), 0x4E, 0xF, 0xF, false));
            if (r & 2) A = R; else B = R;
            const int64_t row = tile * 32 + 8 * g4 + 4 * h + (r & 3);
            mx_u32x2 w;
            w.x = A;
            w.y = B;
            __builtin_nontemporal_store(w, reinterpret_cast<mx_u32x2*>(dst + (row * 32 + (r & ~3)) * 2));
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
          const int64_t e = (tile * 32 + row) * 32 + r;
          if (e < n) store_from_f32(dst + e * DES, DT, acc[i] * (sc[u][i >> 2] * (1.f / 32.f)));
        }
      }
    }
  }
}

}  // namespace

const void* hs_quant_kernel() { return reinterpret_cast<const void*>(&hs_mx8_quant<kBF16>); }

extern "C" {

// fp8 quantize: src (bf16/f16/f32, contiguous, device) -> out fp8 bytes [n] +
// scales fp32 [ceil(n/block)], block = 64*vpt with vpt in {2,4,8,16}.
int hsg_fp8_quantize(int dev, const void* src, int src_dtype, int64_t n, void* out,
                     void* scales, int vpt, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t blk = 64LL * vpt;
  const int64_t nblocks = (n + blk - 1) / blk;
  const int64_t waves_per_wg = kBlock / 64;
  const int grid = static_cast<int>(std::min<int64_t>((nblocks + waves_per_wg - 1) / waves_per_wg, 256 * 8));
  const char* sp = static_cast<const char*>(src);
  uint8_t* op = static_cast<uint8_t*>(out);
  float* sc = static_cast<float*>(scales);
  // streaming kernel: 16-B aligned source, 8-B aligned payload, a block
  // within one wave (bf16/f16 blocks of 128..512, f32 of 128..256)
  const bool aligned = (reinterpret_cast<uintptr_t>(src) % 16) == 0 &&
                       (reinterpret_cast<uintptr_t>(out) % 8) == 0;
  if (aligned && (src_dtype == kBF16 || src_dtype == kF16 || src_dtype == kF32)) {
    const int epl = src_dtype == kF32 ? 4 : 8;
    const int64_t chunk = 64LL * epl * 4;
    const int vgrid = static_cast<int>(std::max<int64_t>(
        1, std::min<int64_t>((n + chunk - 1) / chunk / waves_per_wg + 1, 256 * 16)));
#define HS_FP8V(DT, B)                                                                     \
  hipLaunchKernelGGL((hs_fp8_quant_v<DT, B>), dim3(vgrid), dim3(kBlock), 0, s, sp, n, op, sc); \
  HS_CHECK(hipGetLastError());                                                             \
  return 0
    if (src_dtype == kBF16) {
      if (vpt == 2) { HS_FP8V(kBF16, 128); }
      if (vpt == 4) { HS_FP8V(kBF16, 256); }
      if (vpt == 8) { HS_FP8V(kBF16, 512); }
    } else if (src_dtype == kF16) {
      if (vpt == 2) { HS_FP8V(kF16, 128); }
      if (vpt == 4) { HS_FP8V(kF16, 256); }
      if (vpt == 8) { HS_FP8V(kF16, 512); }
    } else {
      if (vpt == 2) { HS_FP8V(kF32, 128); }
      if (vpt == 4) { HS_FP8V(kF32, 256); }
    }
#undef HS_FP8V
  }
  switch (vpt) {
    case 2: hipLaunchKernelGGL(hs_fp8_quant<2>, dim3(grid), dim3(kBlock), 0, s, sp, src_dtype, n, op, sc); break;
    case 4: hipLaunchKernelGGL(hs_fp8_quant<4>, dim3(grid), dim3(kBlock), 0, s, sp, src_dtype, n, op, sc); break;
    case 8: hipLaunchKernelGGL(hs_fp8_quant<8>, dim3(grid), dim3(kBlock), 0, s, sp, src_dtype, n, op, sc); break;
    case 16: hipLaunchKernelGGL(hs_fp8_quant<16>, dim3(grid), dim3(kBlock), 0, s, sp, src_dtype, n, op, sc); break;
    default: hs_set_error("unsupported vpt %d", vpt); return -1001;
  }
  HS_CHECK(hipGetLastError());
  return 0;
}

int hsg_fp8_dequantize(int dev, const void* q, const void* scales, int64_t n, void* dst,
                       int dst_dtype, int vpt, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t words = (n + 3) / 4;
  const int grid = static_cast<int>(std::min<int64_t>((words + kBlock - 1) / kBlock, 256 * 8));
  const uint8_t* qp = static_cast<const uint8_t*>(q);
  const float* sc = static_cast<const float*>(scales);
  char* dp = static_cast<char*>(dst);
  // streaming kernel: 8-B aligned codes, 16-B aligned destination
  if ((reinterpret_cast<uintptr_t>(q) % 8) == 0 && (reinterpret_cast<uintptr_t>(dst) % 16) == 0 &&
      (vpt == 2 || vpt == 4 || vpt == 8 || vpt == 16) &&
      (dst_dtype == kBF16 || dst_dtype == kF16 || dst_dtype == kF32 || dst_dtype == kF64)) {
    const int64_t epl = (dst_dtype == kF32) ? 4 : (dst_dtype == kF64 ? 2 : 8);
    const int64_t waves = (n + 64 * epl * 4 - 1) / (64 * epl * 4);
    const int vgrid = static_cast<int>(std::min<int64_t>((waves + 3) / 4, 256 * 16));
#define HS_FP8DV(DT)                                                                          \
  switch (vpt) {                                                                              \
    case 2: hipLaunchKernelGGL((hs_fp8_dequant_v<DT, 128>), dim3(vgrid), dim3(kBlock), 0, s, qp, sc, n, dp); break; \
    case 4: hipLaunchKernelGGL((hs_fp8_dequant_v<DT, 256>), dim3(vgrid), dim3(kBlock), 0, s, qp, sc, n, dp); break; \
    case 8: hipLaunchKernelGGL((hs_fp8_dequant_v<DT, 512>), dim3(vgrid), dim3(kBlock), 0, s, qp, sc, n, dp); break; \
    default: hipLaunchKernelGGL((hs_fp8_dequant_v<DT, 1024>), dim3(vgrid), dim3(kBlock), 0, s, qp, sc, n, dp); break; \
  }
    switch (dst_dtype) {
      case kBF16: HS_FP8DV(kBF16); break;
      case kF16: HS_FP8DV(kF16); break;
      case kF32: HS_FP8DV(kF32); break;
      default: HS_FP8DV(kF64); break;
    }
#undef HS_FP8DV
    HS_CHECK(hipGetLastError());
    return 0;
  }
  switch (vpt) {
    case 2: hipLaunchKernelGGL(hs_fp8_dequant<2>, dim3(grid), dim3(kBlock), 0, s, qp, sc, n, dp, dst_dtype); break;
    case 4: hipLaunchKernelGGL(hs_fp8_dequant<4>, dim3(grid), dim3(kBlock), 0, s, qp, sc, n, dp, dst_dtype); break;
    case 8: hipLaunchKernelGGL(hs_fp8_dequant<8>, dim3(grid), dim3(kBlock), 0, s, qp, sc, n, dp, dst_dtype); break;
    case 16: hipLaunchKernelGGL(hs_fp8_dequant<16>, dim3(grid), dim3(kBlock), 0, s, qp, sc, n, dp, dst_dtype); break;
    default: hs_set_error("unsupported vpt %d", vpt); return -1001;
  }
  HS_CHECK(hipGetLastError());
  return 0;
}

// MX fp8: src (bf16/f16/f32, contiguous) -> out [payload = round_up(n, 16)
// bytes; [n, payload) zero-filled] + scales [ceil(n / 32) E8M0 bytes].  Every
// output byte is written (the blob needs no zero-fill).
int hsg_mx8_quantize(int dev, const void* src, int src_dtype, int64_t n, void* out,
                     void* scales, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t payload = (n + 15) / 16 * 16;
  const int64_t chunk = (src_dtype == kF32) ? 64 * 4 * 4 : 64 * 8 * 4;
  const int64_t waves = (n + chunk - 1) / chunk;
  const int grid = static_cast<int>(std::min<int64_t>((waves + 3) / 4, 256 * 16));
  const char* sp = static_cast<const char*>(src);
  uint8_t* op = static_cast<uint8_t*>(out);
  uint8_t* sc = static_cast<uint8_t*>(scales);
  switch (src_dtype) {
    case kBF16: hipLaunchKernelGGL(hs_mx8_quant<kBF16>, dim3(grid), dim3(kBlock), 0, s, sp, n, payload, op, sc); break;
    case kF16: hipLaunchKernelGGL(hs_mx8_quant<kF16>, dim3(grid), dim3(kBlock), 0, s, sp, n, payload, op, sc); break;
    case kF32: hipLaunchKernelGGL(hs_mx8_quant<kF32>, dim3(grid), dim3(kBlock), 0, s, sp, n, payload, op, sc); break;
    default: hs_set_error("unsupported mx8 source dtype %d", src_dtype); return -1002;
  }
  HS_CHECK(hipGetLastError());
  return 0;
}

int hsg_mx8_dequantize(int dev, const void* q, const void* scales, int64_t n, void* dst,
                       int dst_dtype, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t epl = (dst_dtype == kF32) ? 4 : (dst_dtype == kF64 ? 2 : 8);
  const int64_t waves = (n + 64 * epl * 4 - 1) / (64 * epl * 4);
  const int grid = static_cast<int>(std::min<int64_t>((waves + 3) / 4, 256 * 16));
  const uint8_t* qp = static_cast<const uint8_t*>(q);
  const uint8_t* sc = static_cast<const uint8_t*>(scales);
  char* dp = static_cast<char*>(dst);
  switch (dst_dtype) {
    case kBF16: hipLaunchKernelGGL(hs_mx8_dequant<kBF16>, dim3(grid), dim3(kBlock), 0, s, qp, sc, n, dp); break;
    case kF16: hipLaunchKernelGGL(hs_mx8_dequant<kF16>, dim3(grid), dim3(kBlock), 0, s, qp, sc, n, dp); break;
    case kF32: hipLaunchKernelGGL(hs_mx8_dequant<kF32>, dim3(grid), dim3(kBlock), 0, s, qp, sc, n, dp); break;
    case kF64: hipLaunchKernelGGL(hs_mx8_dequant<kF64>, dim3(grid), dim3(kBlock), 0, s, qp, sc, n, dp); break;
    default: hs_set_error("unsupported mx8 dest dtype %d", dst_dtype); return -1002;
  }
  HS_CHECK(hipGetLastError());
  return 0;
}

// Hadamard-rotated fp8: payload `out` has n_pad = round_up(n, 32) bytes,
// `scales` ceil(n_pad / 128) floats.
int hsg_fp8_hadamard_quantize(int dev, const void* src, int src_dtype, int64_t n, void* out,
                              void* scales, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  const int64_t n_pad = (n + 31) / 32 * 32;
  const int64_t ntiles = (n_pad + 1023) / 1024;
  const int grid = static_cast<int>(std::min<int64_t>((ntiles + 3) / 4, 256 * 8));
  constexpr int kHadU = 2;
  const int grid16 = static_cast<int>(std::min<int64_t>((ntiles + 4 * kHadU - 1) / (4 * kHadU), 256 * 8));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const char* sp = static_cast<const char*>(src);
  uint8_t* op = static_cast<uint8_t*>(out);
  float* sc = static_cast<float*>(scales);
  switch (src_dtype) {
    case kBF16: hipLaunchKernelGGL((hs_fp8_hadamard_quant16<kBF16, kHadU>), dim3(grid16), dim3(kBlock), 0, st, sp, n, n_pad, op, sc); break;
    case kF16: hipLaunchKernelGGL((hs_fp8_hadamard_quant16<kF16, kHadU>), dim3(grid16), dim3(kBlock), 0, st, sp, n, n_pad, op, sc); break;
    case kF32: hipLaunchKernelGGL(hs_fp8_hadamard_quant<kF32>, dim3(grid), dim3(kBlock), 0, st, sp, n, n_pad, op, sc); break;
    default: hs_set_error("unsupported hadamard source dtype %d", src_dtype); return -1002;
  }
  HS_CHECK(hipGetLastError());
  return 0;
}

int hsg_fp8_hadamard_dequantize(int dev, const void* q, const void* scales, int64_t n, void* dst,
                                int dst_dtype, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  const int64_t n_pad = (n + 31) / 32 * 32;
  const int64_t ntiles = (n_pad + 1023) / 1024;
  constexpr int U = 2;
  const int grid = static_cast<int>(std::min<int64_t>((ntiles + 4 * U - 1) / (4 * U), 256 * 8));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint8_t* qp = static_cast<const uint8_t*>(q);
  const float* sp = static_cast<const float*>(scales);
  char* dp = static_cast<char*>(dst);
  switch (dst_dtype) {
    case kBF16: hipLaunchKernelGGL((hs_fp8_hadamard_dequant8<kBF16, U>), dim3(grid), dim3(kBlock), 0, st, qp, sp, n, n_pad, dp); break;
    case kF16: hipLaunchKernelGGL((hs_fp8_hadamard_dequant8<kF16, U>), dim3(grid), dim3(kBlock), 0, st, qp, sp, n, n_pad, dp); break;
    case kF32: hipLaunchKernelGGL((hs_fp8_hadamard_dequant8<kF32, U>), dim3(grid), dim3(kBlock), 0, st, qp, sp, n, n_pad, dp); break;
    case kF64: hipLaunchKernelGGL((hs_fp8_hadamard_dequant8<kF64, U>), dim3(grid), dim3(kBlock), 0, st, qp, sp, n, n_pad, dp); break;
    default: hs_set_error("unsupported hadamard dest dtype %d", dst_dtype); return -1002;
  }
  HS_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
