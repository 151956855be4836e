// hsquant: K5/K9 quantization kernels of the lossy checkpoint formats --
// blockwise OCP-fp8 (e4m3fn) with an f32 scale per block, MX fp8 (one E8M0
// scale byte per 32 elements), Hadamard-rotated fp8 on the matrix cores and
// MXFP4 (e2m1 nibbles, one E8M0 scale byte per 32 elements, gfx950's scaled
// fp4 conversions), MXFP6 (e2m3 codes, 32 in 24 bytes, the same scale, a
// whole block per conversion) and two-level-scaled FP4 (e2m1 nibbles, one
// e4m3fn scale byte per 16 elements under one f32 scale for the tensor, found
// by a reduction pass of its own) -- and their hsg_*quantize /
// hsg_*dequantize entry points.
// Wave size is 64.

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "hsgpu_common.h"

namespace {

// ---------------------------------------------------------------------------
// Scale rules.  A policy states one format's rule once, for every kernel of
// that format: the block length, the stored scale, how a scale is formed from
// a block's amax (`set`, which also prepares `scaled`), how a value is scaled
// before the fp8 conversion, whether that needs a clamp, whether the payload's
// pad bytes are zeroed, and how a code's f32 value is restored.
//
// Non-finite inputs, in every format: they do not set their block's scale
// (|x| of inf / nan counts as 0), and their code is the e4m3fn NaN with the
// input's sign (torch's cast).  So one inf does not turn every element of its
// block into NaN, and the GPU codes equal ops/quant.py's reference for every
// input.
// ---------------------------------------------------------------------------

constexpr float kFp8Max = 448.0f;

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

// f32 scale per BLK elements (formats "fp8_e4m3fn_block" and Hadamard):
// q = cvt(clamp(x * (1 / scale))), x = f32(q) * scale.  Two correctly rounded
// divisions per BLOCK (scale, then its reciprocal) and one multiply per
// element -- the torch reference (ops/quant.py _scale_and_quant) applies the
// same rule, so payloads are bit-identical; a division per element made the
// quantizer VALU-bound (profiles/pmc_r2).
template <int BLK>
struct BlockScale {
  static constexpr int kBlk = BLK;
  static constexpr bool kClamp = true;
  static constexpr bool kZeroPad = false;
  using stored_t = float;
  float inv;
  __device__ __forceinline__ stored_t set(float amax) {
    const float scale = fp8_block_scale(amax);
    inv = 1.f / scale;
    return scale;
  }
  __device__ __forceinline__ float scaled(float x) const { return x * inv; }
  static __device__ __forceinline__ float restore(float q, stored_t s) { return q * s; }
};

// MX fp8: one E8M0 (power-of-two) scale byte per 32-element block.  Scale 2^k
// with the smallest k such that amax <= 448*2^k (exact, from frexp: amax =
// m*2^e, k = e-9 if m <= 0.875 else e-8), so x * 2^-k is exact (v_ldexp_f32,
// no division, no clamp needed) and restore is q * 2^k, exact in f32.  The
// payload is round_up(n, 16) bytes with [n, payload) zero-filled.
struct MxScale {
  static constexpr int kBlk = 32;
  static constexpr bool kClamp = false;
  static constexpr bool kZeroPad = true;
  using stored_t = uint8_t;
  int k;
  __device__ __forceinline__ stored_t set(float amax) {
    k = 0;  // zero / inf / nan
    if (amax > 0.f && amax < __builtin_huge_valf()) {
      int e;
      const float m = frexpf(amax, &e);
      k = (m <= 0.875f) ? e - 9 : e - 8;
      k = k < -127 ? -127 : (k > 127 ? 127 : k);
    }
    return static_cast<uint8_t>(k + 127);
  }
  __device__ __forceinline__ float scaled(float x) const { return ldexpf(x, -k); }
  static __device__ __forceinline__ float restore(float q, stored_t s) {
    return ldexpf(q, int(s) - 127);
  }
};

// The codes of x[0..3] under policy `p` (byte j <- x[j]; j >= nvalid encode
// 0): v_cvt_pk_fp8_f32 (gfx950: OCP encoding), then the signed NaN code for
// the non-finite x[j].
template <class P>
__device__ __forceinline__ uint32_t fp8_pack4(const float* x, const P& p, int nvalid = 4) {
  float a[4];
  uint32_t fix = 0, mask = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[j] = 0.f;
    if (j >= nvalid) continue;
    a[j] = p.scaled(x[j]);
    if constexpr (P::kClamp) a[j] = fminf(fmaxf(a[j], -kFp8Max), kFp8Max);
    const uint32_t b = __float_as_uint(x[j]);
    if ((b & 0x7f800000u) == 0x7f800000u) {
      mask |= 0xffu << (8 * j);
      fix |= ((b >> 31) ? 0xffu : 0x7fu) << (8 * j);
    }
  }
  int word = __builtin_amdgcn_cvt_pk_fp8_f32(a[0], a[1], 0, false);
  word = __builtin_amdgcn_cvt_pk_fp8_f32(a[2], a[3], word, true);
  return (static_cast<uint32_t>(word) & ~mask) | fix;
}

__device__ __forceinline__ float fp8_byte_to_f32(uint32_t w, int b) {
  switch (b) {  // the byte select must be an immediate
    case 0: return __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w), 0);
    case 1: return __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w), 1);
    case 2: return __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w), 2);
    default: return __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w), 3);
  }
}

// ---------------------------------------------------------------------------
// 16-byte pieces of a source or destination, shared by the streaming and the
// Hadamard kernels.
// ---------------------------------------------------------------------------

typedef unsigned int mx_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int mx_u32x2 __attribute__((ext_vector_type(2)));

// the 16 / ES elements from e0 on, read one by one (any alignment); zeros
// from element n on
template <int ES>
__device__ __forceinline__ mx_u32x4 load16_elems(const char* src, int64_t e0, int64_t n) {
  mx_u32x4 w = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 16 / ES; ++j) {
    if (e0 + j >= n) break;
    uint32_t bits;
    if constexpr (ES == 4) bits = *reinterpret_cast<const uint32_t*>(src + (e0 + j) * 4);
    else bits = *reinterpret_cast<const uint16_t*>(src + (e0 + j) * 2);
    w[(j * ES) >> 2] |= bits << (((j * ES) & 3) * 8);
  }
  return w;
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

// 16 B of bf16 / f16 / f32 -> 8 or 4 floats
template <int DT>
__device__ __forceinline__ void unpack16(const mx_u32x4& w, float* v) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (DT == kF32) v[i] = __uint_as_float(w[i]);
    else {
      v[2 * i] = mx_unpack<DT>(w[i], 0);
      v[2 * i + 1] = mx_unpack<DT>(w[i], 1);
    }
  }
}

// two floats -> one word of bf16 / f16, the file's one f32 -> 16-bit rounding
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

template <int DT>
__device__ __forceinline__ void mx_store(char* p, const float* f) {
  // 16 B of output: 8 x bf16/f16, 4 x f32 or 2 x f64
  if constexpr (DT == kF32) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  } else if constexpr (DT == kF64) {
    *reinterpret_cast<double2*>(p) = make_double2(static_cast<double>(f[0]),
                                                  static_cast<double>(f[1]));
  } else {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack16<DT>(f[0], f[1]), pack16<DT>(f[2], f[3]),
                                              pack16<DT>(f[4], f[5]), pack16<DT>(f[6], f[7]));
  }
}

// ---------------------------------------------------------------------------
// Streaming quantize / dequantize for the HBM roof, one body for the MX and
// the blockwise format (policy P above).  Quantize:
//   * every 16-B load instruction is contiguous across the wave (lane l
//     reads bytes [16 l, 16 l + 16) of a 1 KiB wave segment), U = 4 of them in
//     flight per lane;
//   * a block spans LPB = P::kBlk / EPL adjacent lanes, EPL = 16 / es elements
//     per lane (MX: 4 lanes for bf16/f16, 8 for f32): amax is an in-register
//     max over the lane's 16 B then a log2(LPB)-step xor-shuffle;
//   * fp8 bytes leave as one 8-B (bf16) / 4-B (f32) store per lane per load,
//     again contiguous across the wave.
// Dequantize mirrors it: lane l reads EPL = 16 / dst-element-size codes and
// writes 16 B, U = 4 in flight; the scale is per lane (P::kBlk % EPL == 0).
// The vector loads and stores need their natural alignment (a view with a
// storage offset has neither): a misaligned call -- a wave-uniform test --
// takes the element path of the tail for every chunk.
// hs_fp8_quant (one block per wave, two 2-B loads per lane) ran at 1.9 TB/s:
// too little in flight per wave.
// ---------------------------------------------------------------------------

constexpr int kStreamU = 4;

// `out` holds `payload` >= n bytes; [n, payload) is zeroed where P asks for it
template <int DT, class P>
__device__ __forceinline__ void stream_quant(const char* __restrict__ src, int64_t n,
                                             int64_t payload, uint8_t* __restrict__ out,
                                             typename P::stored_t* __restrict__ scales) {
  constexpr int ES = (DT == kF32) ? 4 : 2;
  constexpr int EPL = 16 / ES;
  constexpr int LPB = P::kBlk / EPL;
  static_assert(LPB >= 1 && LPB <= 64 && (64 % LPB) == 0, "block must fit a wave");
  constexpr int U = kStreamU;
  constexpr int64_t kChunk = 64LL * EPL * U;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const int64_t end = P::kZeroPad ? payload : n;
  const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                       (reinterpret_cast<uintptr_t>(out) & (EPL - 1)) == 0;
  for (int64_t base = wave0 * kChunk; base < n; base += nwaves * kChunk) {
    const bool full = aligned && base + kChunk <= n;
    mx_u32x4 raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      raw[u] = full ? __builtin_nontemporal_load(reinterpret_cast<const mx_u32x4*>(src + e0 * ES))
                    : load16_elems<ES>(src, e0, n);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float v[EPL];
      unpack16<DT>(raw[u], v);
      float amax = 0.f;
#pragma unroll
      for (int j = 0; j < EPL; ++j) amax = fmaxf(amax, finite_abs(v[j]));
#pragma unroll
      for (int o = 1; o < LPB; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
      P p;
      const typename P::stored_t stored = p.set(amax);
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      if ((lane % LPB) == 0 && e0 < n) scales[e0 / P::kBlk] = stored;
      uint32_t q[EPL / 4];
#pragma unroll
      for (int w = 0; w < EPL / 4; ++w) q[w] = fp8_pack4(v + 4 * w, p);
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
        for (int j = 0; j < EPL; ++j) {
          const int64_t e = e0 + j;
          if (e < end) out[e] = e < n ? static_cast<uint8_t>(q[j >> 2] >> (8 * (j & 3))) : 0;
        }
      }
    }
  }
}

template <int DT, class P>
__device__ __forceinline__ void stream_dequant(const uint8_t* __restrict__ q,
                                               const typename P::stored_t* __restrict__ scales,
                                               int64_t n, char* __restrict__ dst) {
  constexpr int DES = (DT == kF32) ? 4 : (DT == kF64 ? 8 : 2);
  constexpr int EPL = 16 / DES;  // fp8 bytes per lane per step = one 16-B store
  static_assert(P::kBlk % EPL == 0, "one scale per lane");
  constexpr int U = kStreamU;
  constexpr int64_t kChunk = 64LL * EPL * U;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const bool aligned = (reinterpret_cast<uintptr_t>(q) & (EPL - 1)) == 0 &&
                       (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  for (int64_t base = wave0 * kChunk; base < n; base += nwaves * kChunk) {
    const bool full = aligned && base + kChunk <= n;
    uint32_t raw[U][(EPL + 3) / 4];
    typename P::stored_t sc[U];
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
      sc[u] = e0 < n ? scales[e0 / P::kBlk] : typename P::stored_t(0);  // past n: nothing stored
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      float f[EPL];
#pragma unroll
      for (int j = 0; j < EPL; ++j) f[j] = P::restore(fp8_byte_to_f32(raw[u][j >> 2], j & 3), sc[u]);
      if (full) {
        mx_store<DT>(dst + e0 * DES, f);
      } else {
        for (int j = 0; j < EPL && e0 + j < n; ++j) store_from_f32(dst + (e0 + j) * DES, DT, f[j]);
      }
    }
  }
}

template <int DT>
__global__ void __launch_bounds__(kBlock)
hs_mx8_quant(const char* __restrict__ src, int64_t n, int64_t payload,
             uint8_t* __restrict__ out, uint8_t* __restrict__ scales) {
  stream_quant<DT, MxScale>(src, n, payload, out, scales);
}

template <int DT>
__global__ void __launch_bounds__(kBlock)
hs_mx8_dequant(const uint8_t* __restrict__ q, const uint8_t* __restrict__ scales, int64_t n,
               char* __restrict__ dst) {
  stream_dequant<DT, MxScale>(q, scales, n, dst);
}

template <int DT, int BLK>
__global__ void __launch_bounds__(kBlock)
hs_fp8_quant_v(const char* __restrict__ src, int64_t n, uint8_t* __restrict__ out,
               float* __restrict__ scales) {
  stream_quant<DT, BlockScale<BLK>>(src, n, n, out, scales);
}

template <int DT, int BLK>
__global__ void __launch_bounds__(kBlock)
hs_fp8_dequant_v(const uint8_t* __restrict__ q, const float* __restrict__ scales, int64_t n,
                 char* __restrict__ dst) {
  stream_dequant<DT, BlockScale<BLK>>(q, scales, n, dst);
}

// ---------------------------------------------------------------------------
// MXFP4 (format "fp4_e2m1_mx"): e2m1 codes -- sign in bit 3, bits 0-2 an index
// into {0, 0.5, 1, 1.5, 2, 3, 4, 6} -- two per byte, element 2i in the low
// nibble, and one E8M0 scale byte k + 127 per 32 elements.  The rules
// (ops/quant.py mxfp4_quantize_reference applies the same ones):
//   * k is the smallest exponent with amax <= 6 * 2^k over the block's finite
//     elements (frexp: amax = m 2^e, k = e - 3 if m <= 0.75 else e - 2), clamped
//     to [-127, 127], 0 for a block without a finite non-zero: x * 2^-k is
//     exact and at most 6, so there is no division and no clamp;
//   * round to nearest, ties to the even index, the source's sign kept;
//   * +-inf is code +-6 and does not set the scale;
//   * e2m1 has no NaN: a block that holds one stores the MX NaN scale 0xFF
//     and 16 zero payload bytes, and restores as positive quiet NaNs;
//   * restore is q * 2^k, exact in f32, then the one rounding to the
//     destination (pack16 / store_from_f32).
// payload = round_up(ceil(n / 2), 16) bytes, zero from element n on.
//
// Quantize (hs_mxfp4_quant): as in the fp8 streams every 16-B load is
// contiguous across the wave and U = 4 of them are in flight per lane.  A
// nibble payload has no one-byte-per-element store, so the lanes map
// differently:
//   * amax is an unsigned max of |x| bit patterns (monotonic for finite
//     values; v_pk_max_u16 on the packed 16-bit words), then a 2- or 3-step
//     xor-shuffle over the 4 (bf16/f16) or 8 (f32) lanes of a block.  A lane
//     whose max pattern is non-finite -- rare -- goes through its elements once
//     more, leaves inf out and marks a NaN with the key 0xffffffff, which
//     survives the max;
//   * bf16 / f16: the lane's 8 elements go from their packed words straight
//     through v_cvt_scalef32_pk_fp4_{bf16,f16}, one byte each, into one 4-B
//     store; the wave's stores are 256 contiguous bytes;
//   * f32: a 16-B load gives only 2 payload bytes.  Lanes are paired over two
//     loads u, u + 1: the even lane keeps its half-word of load u and takes
//     its neighbour's, the odd lane does the same for load u + 1 -- one DPP
//     quad-perm move per two loads -- so every lane again has one 4-B store
//     and a store instruction covers 256 contiguous bytes.  (Two adjacent
//     loads per lane would make each load instruction touch every other 16 B:
//     the loads, not the stores, carry two thirds of this kernel's traffic.)
//   * scale bytes: a lane keeps the U bytes of its blocks in one register;
//     four wave shuffles per chunk collect them so that the chunk's 64 (f32:
//     32) scale bytes leave as 4-B stores of adjacent lanes.
// The scaled conversions take the scale as an f32 and read its exponent field
// only, which is the E8M0 byte itself: k = -127 is the field 0.  On an MI355X
// they gave the reference's code for every tested input (tests/
// test_gpu_mxfp4.py): ties go to the even code, a magnitude that rounds to
// zero keeps its sign, subnormal sources and k = -127 scale exactly, and the
// first element of a pair lands in the low nibble.  So only what the format
// defines differently is patched: inf and the NaN block.
// Dequantize (hs_mxfp4_dequant): a lane reads 4 / 2 / 1 payload bytes and
// writes 16 B with a nontemporal store, U = 4 steps in flight, the scale per
// lane.  (With plain stores the f32 restore of 2 GiB took 0.544 ms beside MX
// fp8's 0.529 ms; nontemporal ones brought it to 0.535 ms and the bf16 restore
// from 0.272 to 0.263 ms -- docs/architecture.md section 4.)
// v_cvt_scalef32_pk_f32_fp4 decodes the nibbles with scale 1; 2^k is applied
// by v_ldexp_f32 as in MX fp8, which is exact down to subnormals and gives inf
// on overflow (a finite |x| >= 0.875 * 2^128 rounds to a code whose product
// overflows f32: the format's known edge, as in MX fp8).  The scaled forms
// v_cvt_scalef32_pk_{bf16,f16}_fp4 are not used: what they do with subnormal
// or overflowing 16-bit results is not documented, and the restore rule is
// stated on the f32 product.
// A source, payload, scale array or destination without the vector alignment
// (wave-uniform test) and the tail chunk take the element path.
// ---------------------------------------------------------------------------

constexpr uint32_t kFp4NanKey = 0xffffffffu;
constexpr uint32_t kE8m0Nan = 0xffu;

// a decoded code q under the E8M0 byte sb (MXFP4, MXFP6): q * 2^k, exact in
// f32; the NaN byte makes a positive quiet NaN
__device__ __forceinline__ float e8m0_restore(float q, uint32_t sb) {
  return sb == kE8m0Nan ? __builtin_nanf("") : ldexpf(q, int(sb) - 127);
}

typedef unsigned short mx_u16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 mx_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 mx_f16x2 __attribute__((ext_vector_type(2)));
typedef float mx_f32x2 __attribute__((ext_vector_type(2)));

template <int DT>
constexpr uint32_t kInfBits = DT == kF32 ? 0x7f800000u : (DT == kBF16 ? 0x7f80u : 0x7c00u);

// |x| bits and sign of element j of a 16-B piece
template <int DT>
__device__ __forceinline__ uint32_t fp4_abs_bits(const mx_u32x4& w, int j) {
  if constexpr (DT == kF32) return w[j] & 0x7fffffffu;
  else return (w[j >> 1] >> (16 * (j & 1))) & 0x7fffu;
}

template <int DT>
__device__ __forceinline__ uint32_t fp4_sign(const mx_u32x4& w, int j) {
  if constexpr (DT == kF32) return w[j] >> 31;
  else return (w[j >> 1] >> (16 * (j & 1) + 15)) & 1u;
}

// largest finite |x| pattern of a lane's 16 B, kFp4NanKey if one is a NaN
// (kKeyNan; without it a NaN is left out like an inf); `nonfinite`: the piece
// holds an inf or a NaN
template <int DT, bool kKeyNan = true>
__device__ __forceinline__ uint32_t fp4_lane_key(const mx_u32x4& w, bool& nonfinite) {
  constexpr uint32_t kInf = kInfBits<DT>;
  uint32_t a;
  if constexpr (DT == kF32) {
    a = max(max(w[0] & 0x7fffffffu, w[1] & 0x7fffffffu),
            max(w[2] & 0x7fffffffu, w[3] & 0x7fffffffu));
  } else {
    mx_u16x2 m = __builtin_bit_cast(mx_u16x2, w[0] & 0x7fff7fffu);
#pragma unroll
    for (int i = 1; i < 4; ++i)
      m = __builtin_elementwise_max(m, __builtin_bit_cast(mx_u16x2, w[i] & 0x7fff7fffu));
    a = max(uint32_t(m[0]), uint32_t(m[1]));
  }
  nonfinite = a >= kInf;
  if (nonfinite) {
    a = 0;
#pragma unroll
    for (int j = 0; j < (DT == kF32 ? 4 : 8); ++j) {
      const uint32_t p = fp4_abs_bits<DT>(w, j);
      a = (kKeyNan && p > kInf) ? kFp4NanKey : (p < kInf ? max(a, p) : a);
    }
  }
  return a;
}

// E8M0 byte of a block from its amax key (finite pattern or kFp4NanKey), for
// the element formats whose largest magnitude is in [4, 8): frexp gives amax =
// m 2^e, and `top` is that magnitude / 8 (e2m1: 0.75, e2m3: 0.9375)
template <int DT>
__device__ __forceinline__ uint32_t mxfp4_scale_byte(uint32_t key, float top = 0.75f) {
  if (key == kFp4NanKey) return kE8m0Nan;
  float amax;
  if constexpr (DT == kF32) amax = __uint_as_float(key);
  else amax = mx_unpack<DT>(key, 0);
  int k = 0;
  if (amax > 0.f) {
    int e;
    const float m = frexpf(amax, &e);
    k = (m <= top) ? e - 3 : e - 2;
    k = k < -127 ? -127 : (k > 127 ? 127 : k);
  }
  return static_cast<uint32_t>(k + 127);
}

// codes of a lane's 16 B under scale byte `sb`: 8 nibbles (bf16 / f16) or 4
// (f32, low half-word), element j in nibble j.  The conversions divide by
// 2^(exponent field of `scale`) and round to nearest even.  Patched after
// them: the code of an inf (sign | 7, whatever the conversion saturates to)
// and the all-zero payload of a NaN block.
template <int DT>
__device__ __forceinline__ uint32_t fp4_pack(const mx_u32x4& w, uint32_t sb, bool nonfinite) {
  if (sb == kE8m0Nan) return 0;
  const float scale = __uint_as_float(sb << 23);
  // (the words as scalars first: __builtin_bit_cast of a vector element
  // `w[i]` reads element 0 whatever i is)
  const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
  uint32_t r = 0;
  if constexpr (DT == kF32) {
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, __uint_as_float(w0), __uint_as_float(w1), scale, 0);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, __uint_as_float(w2), __uint_as_float(w3), scale, 1);
  } else if constexpr (DT == kBF16) {
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(r, __builtin_bit_cast(mx_bf16x2, w0), scale, 0);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(r, __builtin_bit_cast(mx_bf16x2, w1), scale, 1);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(r, __builtin_bit_cast(mx_bf16x2, w2), scale, 2);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(r, __builtin_bit_cast(mx_bf16x2, w3), scale, 3);
  } else {
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(r, __builtin_bit_cast(mx_f16x2, w0), scale, 0);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(r, __builtin_bit_cast(mx_f16x2, w1), scale, 1);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(r, __builtin_bit_cast(mx_f16x2, w2), scale, 2);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(r, __builtin_bit_cast(mx_f16x2, w3), scale, 3);
  }
  if (nonfinite) {
#pragma unroll
    for (int j = 0; j < (DT == kF32 ? 4 : 8); ++j)
      if (fp4_abs_bits<DT>(w, j) == kInfBits<DT>)
        r = (r & ~(0xfu << (4 * j))) | ((7u | (fp4_sign<DT>(w, j) << 3)) << (4 * j));
  }
  return r;
}

// A chunk's nibbles and scale bytes to memory, for blocks of BLK elements (32:
// MXFP4, 16: the two-level format below): `code[u]` holds the lane's EPL
// nibbles of load u, byte u of `sbytes` the scale byte of its block.  `full`:
// the 4-B stores described above; otherwise byte by byte, zeros from element
// n up to `payload`, and the lane of the last scale byte also zeroes
// scales[nblocks .. scale_end).
template <int EPL, int BLK>
__device__ __forceinline__ void fp4_store_chunk(const uint32_t* code, uint32_t sbytes,
                                                int64_t base, int lane, bool full, int64_t n,
                                                int64_t payload, int64_t scale_end,
                                                uint8_t* __restrict__ out,
                                                uint8_t* __restrict__ scales) {
  constexpr int LPB = BLK / EPL;  // lanes per block
  constexpr int BPL = 64 / LPB;   // blocks (scale bytes) per wave load
  constexpr int U = kStreamU;
  if (full) {
    if constexpr (EPL == 8) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
        __builtin_nontemporal_store(code[u], reinterpret_cast<uint32_t*>(out + (e0 >> 1)));
      }
    } else {
      const bool odd = lane & 1;
#pragma unroll
      for (int u = 0; u < U; u += 2) {
        // even lane: (own, lane + 1) half-words of load u; odd lane:
        // (lane - 1, own) of load u + 1
        const uint32_t other = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(
            static_cast<int>(odd ? code[u] : code[u + 1]), 0xB1, 0xF, 0xF, false));  // lane ^ 1
        const uint32_t word = odd ? ((other & 0xffffu) | (code[u + 1] << 16))
                                  : ((code[u] & 0xffffu) | (other << 16));
        const int64_t e0 = base + (int64_t(u + odd) * 64 + (lane & ~1)) * EPL;
        __builtin_nontemporal_store(word, reinterpret_cast<uint32_t*>(out + (e0 >> 1)));
      }
    }
    // scale byte s of the chunk is byte s / BPL of `sbytes` in lane
    // (s % BPL) * LPB; lane l < U * BPL / 4 stores bytes 4 l .. 4 l + 3
    const int s = (4 * lane) % (U * BPL);
    const int l0 = (s % BPL) * LPB;
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      word |= ((uint32_t(__shfl(int(sbytes), l0 + j * LPB, 64)) >> (8 * (s / BPL))) & 0xffu)
              << (8 * j);
    if (lane < U * BPL / 4)
      __builtin_nontemporal_store(word, reinterpret_cast<uint32_t*>(scales + base / BLK) + lane);
  } else {
    const int64_t nblocks = (n + BLK - 1) / BLK;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      if ((lane % LPB) == 0 && e0 < n) {
        scales[e0 / BLK] = static_cast<uint8_t>(sbytes >> (8 * u));
        if (e0 / BLK == nblocks - 1)
          for (int64_t at = nblocks; at < scale_end; ++at) scales[at] = 0;
      }
      for (int b = 0; b < EPL / 2; ++b) {
        const int64_t at = (e0 >> 1) + b;
        if (at < payload) out[at] = 2 * at < n ? static_cast<uint8_t>(code[u] >> (8 * b)) : 0;
      }
    }
  }
}

// `out` holds `payload` >= ceil(n / 2) bytes, `scales` ceil(n / 32)
template <int DT>
__global__ void __launch_bounds__(kBlock)
hs_mxfp4_quant(const char* __restrict__ src, int64_t n, int64_t payload,
               uint8_t* __restrict__ out, uint8_t* __restrict__ scales) {
  constexpr int ES = (DT == kF32) ? 4 : 2;
  constexpr int EPL = 16 / ES;   // elements per lane per load
  constexpr int LPB = 32 / EPL;  // lanes per block
  constexpr int U = kStreamU;
  static_assert(U == 4, "a lane packs its U scale bytes into one word");
  constexpr int64_t kChunk = 64LL * EPL * U;
  const int lane = threadIdx.x & 63;
  // the wave index through readfirstlane: `base` and `full` are then scalars and
  // the choice between the vector and the element path is a scalar branch
  const int64_t wave0 = int64_t(blockIdx.x) * (kBlock / 64) +
                        __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                       (reinterpret_cast<uintptr_t>(out) & 3) == 0 &&
                       (reinterpret_cast<uintptr_t>(scales) & 3) == 0;
  for (int64_t base = wave0 * kChunk; base < n; base += nwaves * kChunk) {
    const bool full = aligned && base + kChunk <= n;
    mx_u32x4 raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      raw[u] = full ? __builtin_nontemporal_load(reinterpret_cast<const mx_u32x4*>(src + e0 * ES))
                    : load16_elems<ES>(src, e0, n);
    }
    uint32_t code[U];
    uint32_t sbytes = 0;  // byte u: the scale of this lane's block of load u
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bool nonfinite;
      uint32_t key = fp4_lane_key<DT>(raw[u], nonfinite);
#pragma unroll
      for (int o = 1; o < LPB; o <<= 1) key = max(key, uint32_t(__shfl_xor(int(key), o, 64)));
      const uint32_t sb = mxfp4_scale_byte<DT>(key);
      sbytes |= sb << (8 * u);
      code[u] = fp4_pack<DT>(raw[u], sb, nonfinite);
    }
    fp4_store_chunk<EPL, 32>(code, sbytes, base, lane, full, n, payload, (n + 31) / 32, out,
                             scales);
  }
}

// 16 B of restored output (8 x bf16/f16, 4 x f32 or 2 x f64), written once
// and not read again by this kernel: a nontemporal store
template <int DT>
__device__ __forceinline__ mx_u32x4 fp4_piece16(const float* f) {
  if constexpr (DT == kF32) {
    return mx_u32x4{__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]),
                    __float_as_uint(f[3])};
  } else if constexpr (DT == kF64) {
    const uint64_t a = __builtin_bit_cast(uint64_t, static_cast<double>(f[0]));
    const uint64_t b = __builtin_bit_cast(uint64_t, static_cast<double>(f[1]));
    return mx_u32x4{uint32_t(a), uint32_t(a >> 32), uint32_t(b), uint32_t(b >> 32)};
  } else {
    return mx_u32x4{pack16<DT>(f[0], f[1]), pack16<DT>(f[2], f[3]), pack16<DT>(f[4], f[5]),
                    pack16<DT>(f[6], f[7])};
  }
}

template <int DT>
__device__ __forceinline__ void fp4_store16(char* p, const float* f) {
  __builtin_nontemporal_store(fp4_piece16<DT>(f), reinterpret_cast<mx_u32x4*>(p));
}

template <int DT>
__global__ void __launch_bounds__(kBlock)
hs_mxfp4_dequant(const uint8_t* __restrict__ q, const uint8_t* __restrict__ scales, int64_t n,
                 char* __restrict__ dst) {
  constexpr int DES = (DT == kF32) ? 4 : (DT == kF64 ? 8 : 2);
  constexpr int EPL = 16 / DES;  // elements per lane per step = one 16-B store
  constexpr int QB = EPL / 2;    // payload bytes per lane per step
  constexpr int U = kStreamU;
  constexpr int64_t kChunk = 64LL * EPL * U;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = int64_t(blockIdx.x) * (kBlock / 64) +
                        __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // scalar
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const bool aligned = (reinterpret_cast<uintptr_t>(q) & (QB - 1)) == 0 &&
                       (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  for (int64_t base = wave0 * kChunk; base < n; base += nwaves * kChunk) {
    const bool full = aligned && base + kChunk <= n;
    uint32_t raw[U];
    uint32_t sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      if (full) {
        if constexpr (QB == 4) raw[u] = *reinterpret_cast<const uint32_t*>(q + (e0 >> 1));
        else if constexpr (QB == 2) raw[u] = *reinterpret_cast<const uint16_t*>(q + (e0 >> 1));
        else raw[u] = q[e0 >> 1];
      } else {
        raw[u] = 0;
        for (int b = 0; b < QB && e0 + 2 * b < n; ++b) raw[u] |= uint32_t(q[(e0 >> 1) + b]) << (8 * b);
      }
      sc[u] = e0 < n ? scales[e0 / 32] : 0u;  // past n: nothing stored
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      mx_f32x2 p[4];  // the byte select must be an immediate
      p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw[u], 1.0f, 0);
      if constexpr (QB >= 2) p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw[u], 1.0f, 1);
      if constexpr (QB == 4) {
        p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw[u], 1.0f, 2);
        p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw[u], 1.0f, 3);
      }
      float f[EPL];
#pragma unroll
      for (int j = 0; j < EPL; ++j) f[j] = e8m0_restore(p[j >> 1][j & 1], sc[u]);
      if (full) {
        fp4_store16<DT>(dst + e0 * DES, f);
      } else {
        for (int j = 0; j < EPL && e0 + j < n; ++j) store_from_f32(dst + (e0 + j) * DES, DT, f[j]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Two-level-scaled FP4 (format "fp4_e2m1_nv", the "NVFP4" layout): MXFP4's e2m1
// nibbles in MXFP4's order, one e4m3fn scale byte s8 per 16 elements and one
// fp32 A, the tensor's amax over its finite elements, behind the scale bytes
// (zero-padded to a multiple of 4).  Every step of the rule is one fp32
// operation, so ops/quant.py nvfp4_quantize_reference gives the same bytes:
//   * ts = max(A / 2688, 2^-117) (2688 = 448 * 6; quantizer and restore
//     evaluate the same expression; the floor keeps d >= 2^-126 below);
//   * s8 = e4m3fn_rne(min(bamax / (6 * ts), 448)), bamax the block's amax over
//     its finite elements; d = f32(s8) * ts;
//   * code = e2m1_rne(clamp(x * (1 / d), -6, 6)), ties to the even index, the
//     source's sign kept on zero; the clamp is part of the rule (s8 is rounded
//     to nearest, so bamax / d can exceed 6) and turns +-inf into +-6;
//   * s8 == 0 (bamax is 0 or more than about 2^22 below A): 1 / d is inf, so
//     every code of the block is its element's sign bit alone;
//   * a block that holds a NaN stores the e4m3fn NaN 0x7F and 8 zero bytes and
//     restores as positive quiet NaNs; a NaN takes no part in A;
//   * restore is q * d, one fp32 product, then the one rounding to the
//     destination (pack16 / store_from_f32).
// payload = round_up(ceil(n / 2), 16) bytes, zero from element n on.
//
// Three kernels on one stream; a small one clears the A slot first.
// hs_nvfp4_amax, the project's one tensor-wide reduction: a grid-stride stream
// of wave-contiguous 16-B loads, 8 in flight, fp4_lane_key without the NaN key
// per piece (unsigned max of |x| patterns, which orders finite values), a
// 6-step xor-shuffle at the end of the wave's stride and at most one vector
// atomic max per workgroup on the slot -- the f32 pattern, to which a 16-bit
// key is widened first.  A max does not depend on the order of the atomics.  The
// loads are plain ones: hs_nvfp4_quant reads the same bytes again.
// hs_nvfp4_quant has hs_mxfp4_quant's shape and stores (fp4_store_chunk): a
// block is 2 lanes (bf16 / f16) or 4 (f32), so its key needs one or two DPP
// quad moves, and a chunk carries 128 or 64 scale bytes.  Every lane forms ts
// from A, then per load the two correctly rounded divisions of its block
// (bamax / (6 ts) and 1 / d); s8 comes from v_cvt_pk_fp8_f32 and goes back
// through v_cvt_f32_fp8.  The 16-bit scaled fp4 conversions read only an
// exponent field, so every source is unpacked to f32, multiplied by 1 / d,
// clamped by v_med3_f32 and converted by v_cvt_scalef32_pk_fp4_f32 at scale 1.
// The clamp makes +-6 of an inf before the conversion sees it; patched are the
// NaN block and the s8 == 0 block (inf * inf and 0 * inf are not what the rule
// says).
// hs_nvfp4_dequant is hs_mxfp4_dequant with d = f32(s8) * ts per lane (16 is a
// multiple of the 8 / 4 / 2 elements of a lane) and one v_mul_f32 per element.
// These kernels are compiled without the packed f32 instructions
// (HS_NO_PK_F32): their per-element products are plain v_mul_f32.
// ---------------------------------------------------------------------------

#if defined(__HIP_DEVICE_COMPILE__)
#define HS_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define HS_NO_PK_F32
#endif

constexpr float kNvfp4Top = 2688.0f;       // 448 * 6
constexpr float kNvfp4MinTs = 0x1p-117f;   // ts * 2^-9 (the smallest s8) >= 2^-126
constexpr uint32_t kE4m3Nan = 0x7fu;

__device__ __forceinline__ float nvfp4_tensor_scale(float amax) {
  return fmaxf(amax / kNvfp4Top, kNvfp4MinTs);
}

// a decoded code q under block scale byte s8 and tensor scale ts: q * d with
// d = f32(s8) * ts (signed zero when s8 == 0); the byte of a NaN block makes a
// positive quiet NaN
__device__ __forceinline__ float nvfp4_restore(float q, uint32_t s8, float ts) {
  const bool nan = (s8 & 0x7fu) == kE4m3Nan;
  const float d = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(s8), 0) * ts;
  return nan ? __builtin_nanf("") : q * d;
}

// the f32 value of a finite |x| pattern of the source dtype
template <int DT>
__device__ __forceinline__ float fp4_key_value(uint32_t key) {
  if constexpr (DT == kF32) return __uint_as_float(key);
  else return mx_unpack<DT>(key, 0);
}

__global__ void hs_nvfp4_clear(uint32_t* __restrict__ amax) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *amax = 0;
}

constexpr int kAmaxU = 8;           // 16-B loads in flight per lane of hs_nvfp4_amax
constexpr int kAmaxGrid = 256 * 4;  // its workgroups at most

template <int DT>
__global__ void HS_NO_PK_F32 __launch_bounds__(kBlock)
hs_nvfp4_amax(const char* __restrict__ src, int64_t n, uint32_t* __restrict__ amax) {
  constexpr int ES = (DT == kF32) ? 4 : 2;
  constexpr int EPL = 16 / ES;
  constexpr int U = kAmaxU;
  __shared__ uint32_t wave_key[kBlock / 64];
  constexpr int64_t kChunk = 64LL * EPL * U;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = int64_t(blockIdx.x) * (kBlock / 64) +
                        __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // scalar
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  uint32_t key = 0;
  for (int64_t base = wave0 * kChunk; base < n; base += nwaves * kChunk) {
    const bool full = aligned && base + kChunk <= n;
    mx_u32x4 raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      raw[u] = full ? *reinterpret_cast<const mx_u32x4*>(src + e0 * ES)
                    : load16_elems<ES>(src, e0, n);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bool nonfinite;
      key = max(key, fp4_lane_key<DT, false>(raw[u], nonfinite));
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) key = max(key, uint32_t(__shfl_xor(int(key), o, 64)));
  // Atomics on one address complete one after the other, about 12 ns each on
  // an MI355X: 16384 waves, each with its atomic, took 0.2 ms whatever the
  // tensor's size (waves that end together all read an empty slot, so a test
  // before the atomic alone did not help).  So a workgroup joins its waves'
  // keys in LDS and issues one atomic, the grid is kAmaxGrid workgroups at
  // most with kAmaxU loads in flight per lane to make up for the fewer waves,
  // and the atomic is left out if the slot already holds as much (a stale read
  // only costs a needless atomic).
  if (lane == 0) wave_key[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < kBlock / 64; ++i) key = max(key, wave_key[i]);
    const uint32_t bits = __float_as_uint(fp4_key_value<DT>(key));
    if (bits > __hip_atomic_load(amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(amax, bits);
  }
}

// s8 of a block from its key (finite pattern or kFp4NanKey), and 1 / d for its
// elements: inf when s8 == 0
template <int DT>
__device__ __forceinline__ uint32_t nvfp4_block_scale(uint32_t key, float ts, float six_ts,
                                                      float& inv) {
  const float quot = fminf(fp4_key_value<DT>(key) / six_ts, kFp8Max);
  const int word = __builtin_amdgcn_cvt_pk_fp8_f32(quot, 0.f, 0, false);
  inv = 1.f / (__builtin_amdgcn_cvt_f32_fp8(word, 0) * ts);
  return key == kFp4NanKey ? kE4m3Nan : (static_cast<uint32_t>(word) & 0xffu);
}

// codes of a lane's 16 B under scale byte `s8`, `inv` = 1 / d: 8 nibbles
// (bf16 / f16) or 4 (f32, low half-word), element j in nibble j
template <int DT>
__device__ __forceinline__ uint32_t nvfp4_pack(const mx_u32x4& w, uint32_t s8, float inv) {
  if (s8 == kE4m3Nan) return 0;
  const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
  if (s8 == 0) {  // the sign bits alone: bit 3 of each nibble
    if constexpr (DT == kF32) {
      return ((w0 >> 31) << 3) | ((w1 >> 31) << 7) | ((w2 >> 31) << 11) | ((w3 >> 31) << 15);
    } else {
      const uint32_t ws[4] = {w0, w1, w2, w3};
      uint32_t r = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        r |= (((ws[i] >> 15) & 1u) << (8 * i + 3)) | ((ws[i] >> 31) << (8 * i + 7));
      return r;
    }
  }
  constexpr int EPL = (DT == kF32) ? 4 : 8;
  float v[EPL];
  unpack16<DT>(w, v);
#pragma unroll
  for (int j = 0; j < EPL; ++j) v[j] = __builtin_amdgcn_fmed3f(v[j] * inv, -6.f, 6.f);
  uint32_t r = 0;
  r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, v[0], v[1], 1.0f, 0);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, v[2], v[3], 1.0f, 1);
  if constexpr (EPL == 8) {
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, v[4], v[5], 1.0f, 2);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, v[6], v[7], 1.0f, 3);
  }
  return r;
}

// `out` holds `payload` >= ceil(n / 2) bytes, `scales` round_up(ceil(n / 16), 4)
template <int DT>
__global__ void HS_NO_PK_F32 __launch_bounds__(kBlock)
hs_nvfp4_quant(const char* __restrict__ src, int64_t n, int64_t payload,
               uint8_t* __restrict__ out, uint8_t* __restrict__ scales,
               const float* __restrict__ amax) {
  constexpr int ES = (DT == kF32) ? 4 : 2;
  constexpr int EPL = 16 / ES;   // elements per lane per load
  constexpr int LPB = 16 / EPL;  // lanes per block: 2 or 4, inside a quad
  constexpr int U = kStreamU;
  static_assert(U == 4, "a lane packs its U scale bytes into one word");
  constexpr int64_t kChunk = 64LL * EPL * U;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = int64_t(blockIdx.x) * (kBlock / 64) +
                        __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // scalar
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                       (reinterpret_cast<uintptr_t>(out) & 3) == 0 &&
                       (reinterpret_cast<uintptr_t>(scales) & 3) == 0;
  const float ts = nvfp4_tensor_scale(*amax);
  const float six_ts = 6.f * ts;
  const int64_t scale_end = ((n + 15) / 16 + 3) / 4 * 4;
  for (int64_t base = wave0 * kChunk; base < n; base += nwaves * kChunk) {
    const bool full = aligned && base + kChunk <= n;
    mx_u32x4 raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      raw[u] = full ? __builtin_nontemporal_load(reinterpret_cast<const mx_u32x4*>(src + e0 * ES))
                    : load16_elems<ES>(src, e0, n);
    }
    uint32_t code[U];
    uint32_t sbytes = 0;  // byte u: the scale of this lane's block of load u
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bool nonfinite;
      uint32_t key = fp4_lane_key<DT>(raw[u], nonfinite);
      key = max(key, uint32_t(__builtin_amdgcn_mov_dpp(int(key), 0xB1, 0xF, 0xF, false)));  // ^ 1
      if constexpr (LPB == 4)
        key = max(key, uint32_t(__builtin_amdgcn_mov_dpp(int(key), 0x4E, 0xF, 0xF, false)));  // ^ 2
      float inv;
      const uint32_t s8 = nvfp4_block_scale<DT>(key, ts, six_ts, inv);
      sbytes |= s8 << (8 * u);
      code[u] = nvfp4_pack<DT>(raw[u], s8, inv);
    }
    fp4_store_chunk<EPL, 16>(code, sbytes, base, lane, full, n, payload, scale_end, out, scales);
  }
}

template <int DT>
__global__ void HS_NO_PK_F32 __launch_bounds__(kBlock)
hs_nvfp4_dequant(const uint8_t* __restrict__ q, const uint8_t* __restrict__ scales,
                 const float* __restrict__ amax, int64_t n, char* __restrict__ dst) {
  constexpr int DES = (DT == kF32) ? 4 : (DT == kF64 ? 8 : 2);
  constexpr int EPL = 16 / DES;  // elements per lane per step = one 16-B store
  constexpr int QB = EPL / 2;    // payload bytes per lane per step
  static_assert(16 % EPL == 0, "one scale per lane");
  constexpr int U = kStreamU;
  constexpr int64_t kChunk = 64LL * EPL * U;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = int64_t(blockIdx.x) * (kBlock / 64) +
                        __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // scalar
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const bool aligned = (reinterpret_cast<uintptr_t>(q) & (QB - 1)) == 0 &&
                       (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  const float ts = nvfp4_tensor_scale(*amax);
  for (int64_t base = wave0 * kChunk; base < n; base += nwaves * kChunk) {
    const bool full = aligned && base + kChunk <= n;
    uint32_t raw[U];
    uint32_t sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      if (full) {
        if constexpr (QB == 4) raw[u] = *reinterpret_cast<const uint32_t*>(q + (e0 >> 1));
        else if constexpr (QB == 2) raw[u] = *reinterpret_cast<const uint16_t*>(q + (e0 >> 1));
        else raw[u] = q[e0 >> 1];
      } else {
        raw[u] = 0;
        for (int b = 0; b < QB && e0 + 2 * b < n; ++b) raw[u] |= uint32_t(q[(e0 >> 1) + b]) << (8 * b);
      }
      sc[u] = e0 < n ? scales[e0 / 16] : 0u;  // past n: nothing stored
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      mx_f32x2 p[4];  // the byte select must be an immediate
      p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw[u], 1.0f, 0);
      if constexpr (QB >= 2) p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw[u], 1.0f, 1);
      if constexpr (QB == 4) {
        p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw[u], 1.0f, 2);
        p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw[u], 1.0f, 3);
      }
      float f[EPL];
#pragma unroll
      for (int j = 0; j < EPL; ++j) f[j] = nvfp4_restore(p[j >> 1][j & 1], sc[u], ts);
      if (full) {
        fp4_store16<DT>(dst + e0 * DES, f);
      } else {
        for (int j = 0; j < EPL && e0 + j < n; ++j) store_from_f32(dst + (e0 + j) * DES, DT, f[j]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// MXFP6 (format "fp6_e2m3_mx"): e2m3 codes -- sign in bit 5, exponent in bits
// 4-3 (bias 1), mantissa in bits 2-0: magnitudes 0 .. 1.875 in steps of 1/8,
// 2 .. 3.75 in steps of 1/4, 4 .. 7.5 in steps of 1/2 -- and one E8M0 scale
// byte k + 127 per 32 elements.  Block b is payload bytes [24 b, 24 b + 24)
// read as a little-endian 192-bit string, element j its bits [6 j, 6 j + 6).
// The rules are MXFP4's with the other grid (ops/quant.py
// mxfp6_quantize_reference applies the same ones): k is the smallest exponent
// with amax <= 7.5 * 2^k over the finite elements (frexp: k = e - 3 if m <=
// 0.9375 else e - 2), ties go to the even index, the sign is kept on zero,
// +-inf is code +-7.5 and sets no scale, a block with a NaN stores 0xFF and 24
// zero bytes and restores as positive quiet NaNs, restore is q * 2^k in f32
// and one rounding.  payload = round_up(24 * nblocks, 16) bytes; elements
// from n on are code 0 and the bytes past the last block are zero.
//
// gfx950 converts a whole block in one instruction (v_cvt_scalef32_pk32_fp6_
// {bf16,f16}, v_cvt_scalef32_2xpk16_fp6_f32, v_cvt_scalef32_pk32_f32_fp6), so
// here a LANE owns a block, where the fp8 and fp4 streams spread one over 4 or
// 8 lanes: a wave step is 64 blocks, 2048 elements, and turns into 1536
// contiguous payload bytes and 64 contiguous scale bytes.
//   * amax is the unsigned max of the |x| bit patterns of the lane's own 16 or
//     32 registers (fp4_lane_key per 16 B): no shuffle;
//   * per lane the results would be 24 B at a 24-B stride (quantize) or 64 /
//     128 / 256 B at that stride (dequantize), and strided 16-B stores cost the
//     rotated MXFP4 restore a factor of 2.3 to 3.3 (docs/architecture.md
//     section 4).  So every result goes through the wave's own piece of LDS
//     and every global store instruction covers one contiguous span: three
//     8-B stores per lane for the payload, 16-B nontemporal stores for
//     restored values, one 4-B store from every fourth lane for the scales
//     (bytes gathered over the quad by two DPP moves);
//   * LDS patterns: a lane writes its six payload dwords as three 8-B pieces
//     at a stride of three such pieces, and its restored values as 16-B pieces
//     in a row of NP + 1 pieces (NP = 4, 8 or 16 pieces of payload per lane).
//     Both strides are odd in units of the access width, so the lanes of one
//     instruction spread over all banks; a 6-dword stride with 4-B writes
//     would put two lanes on each bank.  The reads are contiguous.  An f64
//     destination goes in two passes of 32 lanes, so that it needs the LDS of
//     an f32 one (about 9 KiB per wave) and its stores still cover a span;
//   * a wave only ever touches its own LDS, whose instructions complete in
//     order: wave_lds_fence() orders the compiler, no s_barrier is needed.
// Loads are wave-contiguous as well: the source's 16-B pieces (and the
// restore's 8-B payload pieces) go through the same LDS rows into block
// ownership.  The other plan, every lane loading its own block at a 64- or
// 128-B stride (and its 24 payload bytes at a 24-B stride) with no LDS on the
// way in, was measured in the same build on 512 Mi elements and was slower in
// all four cases: quantize bf16 0.276 ms against 0.267, f32 0.482 against
// 0.474; restore bf16 0.281 against 0.278, f32 0.485 against 0.477 (medians;
// profiles/mxfp6_kernels/strided_loads_*.jsonl, docs/architecture.md section
// 4).
// Found on an MI355X with a probe of the four conversions and by tests/
// test_gpu_mxfp6.py: element j of a block lands in bits [6 j, 6 j + 6) of the
// six result registers, for the 16-bit sources and for the decode;
// v_cvt_scalef32_2xpk16_fp6_f32 interleaves its operands (element 2 i from the
// first, 2 i + 1 from the second); ties go to the even code, subnormal codes
// and sources and the scale field 0 (k = -127) are exact, a zero result keeps
// its sign, larger magnitudes and inf saturate to +-7.5, a NaN becomes +7.5.
// As for fp4 only inf (by rule, not by need) and the NaN block are patched.
// The scale operand is an f32 of which only the exponent field, the E8M0
// byte, is read.
// A misaligned source, payload, scale array or destination (wave-uniform
// test) and the tail chunk take the element path: the lane still owns its
// block, reads it element by element (zeros from n on) and writes its bytes
// one by one; the lane of the last block also zeroes the bytes up to `payload`.
// ---------------------------------------------------------------------------

constexpr int kFp6Step = 64 * 32;  // elements of a wave step: one block per lane

typedef unsigned int mx_u32x6 __attribute__((ext_vector_type(6)));
typedef unsigned int mx_u32x16 __attribute__((ext_vector_type(16)));
typedef float mx_f32x16 __attribute__((ext_vector_type(16)));
typedef float mx_f32x32 __attribute__((ext_vector_type(32)));
typedef __bf16 mx_bf16x32 __attribute__((ext_vector_type(32)));
typedef _Float16 mx_f16x32 __attribute__((ext_vector_type(32)));

// between a wave's LDS writes and its reads of what other lanes wrote
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the six payload dwords of a lane's block (NP 16-B pieces `w`) under scale
// byte `sb`.  The conversions divide by 2^(exponent field of `scale`) and
// round to nearest even.  Patched after them: the code of an inf (sign | 31)
// and the all-zero payload of a NaN block.
// A block conversion writes its result registers before it has read all of
// its operands, and this compiler does not keep the two apart: the f32
// quantizer came out as `v_cvt_scalef32_2xpk16_fp6_f32 v[32:37], v[0:15],
// v[16:31], v32` and gave garbage codes from the third element on.  The empty
// asm after each conversion uses the operands once more, so they are live
// across it and share no register with the result.
template <int DT>
__device__ __forceinline__ mx_u32x6 fp6_pack(const mx_u32x4* w, uint32_t sb, bool nonfinite) {
  mx_u32x6 r = {0, 0, 0, 0, 0, 0};
  if (sb == kE8m0Nan) return r;
  const float scale = __uint_as_float(sb << 23);
  constexpr int NW = (DT == kF32) ? 32 : 16;
  uint32_t e[NW];  // scalars first (see fp4_pack)
#pragma unroll
  for (int j = 0; j < NW; ++j) e[j] = w[j >> 2][j & 3];
  if constexpr (DT == kF32) {
    // element 2 i of the result is element i of the first operand, element
    // 2 i + 1 element i of the second
    mx_f32x16 a, b;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      a[j] = __uint_as_float(e[2 * j]);
      b[j] = __uint_as_float(e[2 * j + 1]);
    }
    r = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, scale);
    asm volatile("" ::"v"(a), "v"(b), "v"(scale));  // no register shared with r (see above)
  } else {
    mx_u32x16 v;
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = e[j];
    if constexpr (DT == kBF16)
      r = __builtin_amdgcn_cvt_scalef32_pk32_fp6_bf16(__builtin_bit_cast(mx_bf16x32, v), scale);
    else
      r = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(__builtin_bit_cast(mx_f16x32, v), scale);
    asm volatile("" ::"v"(v), "v"(scale));  // no register shared with r (see above)
  }
  if (nonfinite) {
    uint32_t c[6] = {r[0], r[1], r[2], r[3], r[4], r[5]};
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      uint32_t bits;
      if constexpr (DT == kF32) bits = e[j];
      else bits = (e[j >> 1] >> (16 * (j & 1))) << 16;  // as the f32's upper half
      if ((bits & 0x7fffffffu) != (kInfBits<DT> << (DT == kF32 ? 0 : 16))) continue;
      const uint32_t code = 31u | ((bits >> 31) << 5);
      constexpr uint32_t kMask = 0x3fu;
      const int wd = (6 * j) >> 5, sh = (6 * j) & 31;
      c[wd] = (c[wd] & ~(kMask << sh)) | (code << sh);
      if (sh > 26) c[wd + 1] = (c[wd + 1] & ~(kMask >> (32 - sh))) | (code >> (32 - sh));
    }
    r = mx_u32x6{c[0], c[1], c[2], c[3], c[4], c[5]};
  }
  return r;
}

// `out` holds `payload` >= 24 * ceil(n / 32) bytes, `scales` ceil(n / 32)
template <int DT>
__global__ void __launch_bounds__(kBlock)
hs_mxfp6_quant(const char* __restrict__ src, int64_t n, int64_t payload,
               uint8_t* __restrict__ out, uint8_t* __restrict__ scales) {
  constexpr int ES = (DT == kF32) ? 4 : 2;
  constexpr int EPP = 16 / ES;     // elements per 16-B piece
  constexpr int NP = 32 / EPP;     // pieces per block: 4 or 8
  constexpr int ROW = NP + 1;      // LDS row of a block, in pieces
  __shared__ mx_u32x4 lds_all[kBlock / 64][64 * ROW];  // source rows, then 1536 B of payload
  mx_u32x4* lds = lds_all[threadIdx.x >> 6];
  mx_u32x2* lds8 = reinterpret_cast<mx_u32x2*>(lds);
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = int64_t(blockIdx.x) * (kBlock / 64) +
                        __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // scalar
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const int64_t nblocks = (n + 31) / 32;
  const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                       (reinterpret_cast<uintptr_t>(out) & 7) == 0 &&
                       (reinterpret_cast<uintptr_t>(scales) & 3) == 0;
  for (int64_t base = wave0 * kFp6Step; base < n; base += nwaves * kFp6Step) {
    const bool full = aligned && base + kFp6Step <= n;
    const int64_t blk = base / 32 + lane;
    mx_u32x4 raw[NP];
    if (full) {
      const mx_u32x4* p = reinterpret_cast<const mx_u32x4*>(src + base * ES);
      // wave-contiguous loads, then piece 64 i + lane to its block's row
#pragma unroll
      for (int i = 0; i < NP; ++i) raw[i] = __builtin_nontemporal_load(p + 64 * i + lane);
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int q = 64 * i + lane;
        lds[(q / NP) * ROW + (q % NP)] = raw[i];
      }
      wave_lds_fence();
#pragma unroll
      for (int i = 0; i < NP; ++i) raw[i] = lds[lane * ROW + i];
      wave_lds_fence();
    } else {
#pragma unroll
      for (int i = 0; i < NP; ++i) raw[i] = load16_elems<ES>(src, blk * 32 + i * EPP, n);
    }
    uint32_t key = 0;
    bool nonfinite = false;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      bool nf;
      key = max(key, fp4_lane_key<DT>(raw[i], nf));
      nonfinite |= nf;
    }
    const uint32_t sb = mxfp4_scale_byte<DT>(key, 0.9375f);
    const mx_u32x6 code = fp6_pack<DT>(raw, sb, nonfinite);
    const uint32_t c[6] = {code[0], code[1], code[2], code[3], code[4], code[5]};
    if (full) {
#pragma unroll
      for (int i = 0; i < 3; ++i) lds8[3 * lane + i] = mx_u32x2{c[2 * i], c[2 * i + 1]};
      wave_lds_fence();
      mx_u32x2* o = reinterpret_cast<mx_u32x2*>(out + 24 * (base / 32));
#pragma unroll
      for (int i = 0; i < 3; ++i) __builtin_nontemporal_store(lds8[64 * i + lane], o + 64 * i + lane);
      wave_lds_fence();
      // the quad's four scale bytes into one word, stored by its first lane
      uint32_t word = sb << (8 * (lane & 3));
      word |= static_cast<uint32_t>(
          __builtin_amdgcn_mov_dpp(static_cast<int>(word), 0xB1, 0xF, 0xF, false));  // lane ^ 1
      word |= static_cast<uint32_t>(
          __builtin_amdgcn_mov_dpp(static_cast<int>(word), 0x4E, 0xF, 0xF, false));  // lane ^ 2
      if ((lane & 3) == 0)
        __builtin_nontemporal_store(word,
                                    reinterpret_cast<uint32_t*>(scales + base / 32) + (lane >> 2));
    } else if (blk < nblocks) {
      scales[blk] = static_cast<uint8_t>(sb);
      const bool last = blk == nblocks - 1;
#pragma unroll
      for (int t = 0; t < 32; ++t) {
        const int64_t at = 24 * blk + t;
        if (t < 24) out[at] = static_cast<uint8_t>(c[t >> 2] >> (8 * (t & 3)));
        else if (last && at < payload) out[at] = 0;
      }
    }
  }
}

// the f32 values of the 32 codes in six payload dwords, at scale 1
__device__ __forceinline__ mx_f32x32 fp6_decode32(const uint32_t* c) {
  const mx_u32x6 cv = {c[0], c[1], c[2], c[3], c[4], c[5]};
  const mx_f32x32 dec = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(cv, 1.0f);
  asm volatile("" ::"v"(cv));  // no register shared with dec (see fp6_pack)
  return dec;
}

template <int DT>
__global__ void __launch_bounds__(kBlock)
hs_mxfp6_dequant(const uint8_t* __restrict__ q, const uint8_t* __restrict__ scales, int64_t n,
                 char* __restrict__ dst) {
  constexpr int DES = (DT == kF32) ? 4 : (DT == kF64 ? 8 : 2);
  constexpr int EPP = 16 / DES;             // elements per 16-B piece
  constexpr int NP = 32 / EPP;              // pieces per block: 4, 8 or 16
  constexpr int PASSES = NP == 16 ? 2 : 1;  // f64: 32 lanes at a time
  constexpr int LPP = 64 / PASSES;          // lanes per pass
  constexpr int ROW = NP + 1;               // LDS row of a block, in pieces
  __shared__ mx_u32x4 lds_all[kBlock / 64][LPP * ROW];
  mx_u32x4* lds = lds_all[threadIdx.x >> 6];
  mx_u32x2* lds8 = reinterpret_cast<mx_u32x2*>(lds);
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = int64_t(blockIdx.x) * (kBlock / 64) +
                        __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // scalar
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const int64_t nblocks = (n + 31) / 32;
  const bool aligned = (reinterpret_cast<uintptr_t>(q) & 7) == 0 &&
                       (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  for (int64_t base = wave0 * kFp6Step; base < n; base += nwaves * kFp6Step) {
    const bool full = aligned && base + kFp6Step <= n;
    const int64_t blk = base / 32 + lane;
    uint32_t c[6] = {0, 0, 0, 0, 0, 0};
    uint32_t sb = 0;  // past n: nothing stored
    if (full) {
      const mx_u32x2* p = reinterpret_cast<const mx_u32x2*>(q + 24 * (base / 32));
      sb = scales[blk];
      mx_u32x2 t[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = __builtin_nontemporal_load(p + 64 * i + lane);
#pragma unroll
      for (int i = 0; i < 3; ++i) lds8[64 * i + lane] = t[i];
      wave_lds_fence();
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = lds8[3 * lane + i];
      wave_lds_fence();
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        c[2 * i] = t[i].x;
        c[2 * i + 1] = t[i].y;
      }
    } else if (blk < nblocks) {
      sb = scales[blk];
#pragma unroll
      for (int t = 0; t < 24; ++t) c[t >> 2] |= uint32_t(q[24 * blk + t]) << (8 * (t & 3));
    }
    const mx_f32x32 dec = fp6_decode32(c);
    float f[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) f[j] = e8m0_restore(dec[j], sb);
    if (full) {
#pragma unroll
      for (int h = 0; h < PASSES; ++h) {
        if (PASSES == 1 || lane / LPP == h) {
#pragma unroll
          for (int i = 0; i < NP; ++i) lds[(lane % LPP) * ROW + i] = fp4_piece16<DT>(f + i * EPP);
        }
        wave_lds_fence();
        mx_u32x4* o = reinterpret_cast<mx_u32x4*>(dst + (base + h * LPP * 32) * DES);
#pragma unroll
        for (int i = 0; i < NP / PASSES; ++i) {
          const int piece = 64 * i + lane;
          __builtin_nontemporal_store(lds[(piece / NP) * ROW + (piece % NP)], o + piece);
        }
        wave_lds_fence();
      }
    } else {
#pragma unroll
      for (int j = 0; j < 32; ++j)
        if (blk * 32 + j < n) store_from_f32(dst + (blk * 32 + j) * DES, DT, f[j]);
    }
  }
}

// ---------------------------------------------------------------------------
// Blockwise fp8 for misaligned calls, and for blocks wider than the streaming
// quantizer's wave share (bf16/f16 vpt 16, f32 vpt 8 and 16).  Quantize: one
// 64-lane wave owns one block of 64 * VPT elements; amax via 64-wide
// xor-shuffle reduction.  Dequantize: four codes per lane.  On a destination
// off by one element it restores 1 GiB of bf16 at 2.48 TB/s; the streaming
// kernel's element path, in a build whose host code sent such calls to it,
// ran at 1.71 TB/s (scripts/fp8_kernels_bench.py --offset none).
// ---------------------------------------------------------------------------

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
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
    BlockScale<kBlk> p;
    const float scale = p.set(wave_max(amax));
    if (lane == 0) scales[b] = scale;
    uint32_t words[(VPT + 3) / 4];
#pragma unroll
    for (int w = 0; w < (VPT + 3) / 4; ++w)
      words[w] = fp8_pack4(v + 4 * w, p, VPT - 4 * w < 4 ? VPT - 4 * w : 4);
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
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = fp8_byte_to_f32(word, j);
    for (int j = 0; j < 4 && e0 + j < n; ++j) store_from_f32(dst + (e0 + j) * des, dst_dtype, f[j] * s);
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
typedef short hs_i16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 hs_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 hs_f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ bool hada_neg(int k, int c) { return __popc(k & c) & 1; }

__device__ __forceinline__ float hada(int k, int c) { return hada_neg(k, c) ? -1.f : 1.f; }

// H[k0 + j][c], j = 0..7, as 16-bit +-1 (bf16 0x3F80/0xBF80, f16 0x3C00/0xBC00):
// a B fragment of the 16-bit MFMA
template <int DT>
__device__ __forceinline__ hs_i16x8 hada_frag16(int k0, int c) {
  const short one = (DT == kBF16) ? short(0x3F80) : short(0x3C00);
  hs_i16x8 b;
#pragma unroll
  for (int j = 0; j < 8; ++j) b[j] = hada_neg(k0 + j, c) ? short(one | 0x8000) : one;
  return b;
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
  constexpr int EPL = 16 / ES;
  if (e0 + 16 <= n && ((reinterpret_cast<uintptr_t>(src + e0 * ES) & 15) == 0)) {
    const mx_u32x4* v = reinterpret_cast<const mx_u32x4*>(src + e0 * ES);
#pragma unroll
    for (int q = 0; q < 16 / EPL; ++q) unpack16<DT>(v[q], x + EPL * q);
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

// Epilogue of one rotated tile (C/D map above): blockwise scales + e4m3 codes.
__device__ __forceinline__ void hadamard_tile_store(const floatx16& acc, int64_t tile, int r,
                                                    int h, int64_t n_pad, int64_t nblocks,
                                                    uint8_t* __restrict__ out,
                                                    float* __restrict__ scales) {
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const float a4[4] = {acc[4 * g4], acc[4 * g4 + 1], acc[4 * g4 + 2], acc[4 * g4 + 3]};
    const float amax = max_over_32(fmaxf(fmaxf(finite_abs(a4[0]), finite_abs(a4[1])),
                                         fmaxf(finite_abs(a4[2]), finite_abs(a4[3]))));
    BlockScale<128> p;
    const float scale = p.set(amax);
    const int64_t blk = tile * 8 + 2 * g4 + h;
    if (r == 0 && blk < nblocks) scales[blk] = scale;
    // byte q of `w` = row q + 8 g4 + 4 h, column r.  A 4x4 byte transpose
    // over each quad of lanes (two DPP quad-perm exchanges + v_perm_b32)
    // leaves lane r with row (r & 3) + 8 g4 + 4 h, columns (r & ~3) .. +3:
    // one 4-B store per lane, 256 contiguous bytes per wave instruction,
    // instead of 4 one-byte stores.
    uint32_t w = fp8_pack4(a4, p);
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
    hadamard_tile_store(acc, tile, r, h, n_pad, nblocks, out, scales);
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
// C/D is the f32 form's map, so the epilogue is the same.
template <int DT>
__device__ __forceinline__ floatx16 mfma16(hs_i16x8 a, hs_i16x8 b, floatx16 c) {
  if constexpr (DT == kBF16)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(hs_bf16x8, a),
                                                   __builtin_bit_cast(hs_bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(hs_f16x8, a),
                                                  __builtin_bit_cast(hs_f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ hs_i16x8 load_a_frag(const char* src, int64_t e0, int64_t n) {
  const bool vec = e0 + 8 <= n && (reinterpret_cast<uintptr_t>(src + e0 * 2) & 15) == 0;
  return __builtin_bit_cast(
      hs_i16x8, vec ? __builtin_nontemporal_load(reinterpret_cast<const mx_u32x4*>(src + e0 * 2))
                    : load16_elems<2>(src, e0, n));
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
  // B fragments: H[16 s + 8 h + j][r]
  const hs_i16x8 b0 = hada_frag16<DT>(8 * h, r), b1 = hada_frag16<DT>(16 + 8 * h, r);
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
        a[u][0] = load_a_frag(src, e0, n);
        a[u][1] = load_a_frag(src, e0 + 16, n);
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

// The 4x4 transpose of 16-bit elements over a quad of lanes and its store.
// In: lane r holds rows 0..3 of column r as (A.lo, A.hi, B.lo, B.hi); `rows`
// points at row 0, rows are 64 B apart.  Out: lane r writes row r & 3, columns
// (r & ~3) .. +3, as one 8-B store.
__device__ __forceinline__ void hada_store_quad16(uint32_t A, uint32_t B, int r, char* rows) {
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
  mx_u32x2 w;
  w.x = A;
  w.y = B;
  __builtin_nontemporal_store(w, reinterpret_cast<mx_u32x2*>(rows + ((r & 3) * 32 + (r & ~3)) * 2));
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
  const hs_i16x8 b0 = hada_frag16<kBF16>(16 * h, r), b1 = hada_frag16<kBF16>(16 * h + 8, r);
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
            hada_store_quad16(pack16<DT>(acc[4 * g4] * s, acc[4 * g4 + 1] * s),
                              pack16<DT>(acc[4 * g4 + 2] * s, acc[4 * g4 + 3] * s), r,
                              dst + (tile * 32 + 8 * g4 + 4 * h) * 64);
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

// ---------------------------------------------------------------------------
// Hadamard-rotated MXFP4 (format "fp4_e2m1_mx", rotation "hadamard32"): every
// group of 32 is rotated by H and the 32 rotated values are ONE MX block --
// one E8M0 byte and 16 bytes of e2m1 nibbles per group, under the MXFP4 rules
// above except that a group with any non-finite rotated value (an inf, a NaN
// or an overflowed sum) stores 0xFF and zeros and restores as quiet NaNs.
// blob = n_pad / 2 payload bytes + n_pad / 32 scale bytes, n_pad =
// round_up(n, 32); ops/quant.py states the rules.
//
// One wave owns a tile of 32 groups, as the fp8 Hadamard kernels do, but the
// operands are swapped: H is symmetric, so D = H * X^T puts Y[group j]
// [element i] at D[i][j], and with the C/D map (register i of lane (r, h) =
// row (i&3) + 8(i>>2) + 4h, column r) lane (r, h) holds, for group r, the 16
// rotated elements 8g + 4h + 0..3 (g = 0..3) in its own registers.  The group
// is the scale block, so nothing of the epilogue crosses more than the two
// lanes r and r + 32 (v_permlane32_swap: no LDS), where the fp8 epilogue does
// four 32-lane reductions per tile:
//   * loads as in the fp8 kernels, now the B operand: f32 lane (r, h) reads
//     X[r][16h .. 16h+15] and runs 16 x v_mfma_f32_32x32x2_f32 with A =
//     H[r][16h + t] -- the products and the k order of HADAMARD_K_ORDER, so an
//     f32 source reproduces the reference byte for byte; bf16 / f16 read the
//     fragments X[r][16s + 8h ..+7] for 2 x v_mfma_f32_32x32x16, which sums in
//     the hardware's order (a code on a rounding boundary can move, as for
//     hadamard32);
//   * amax: unsigned max over the lane's 16 |y| patterns, one swap with the
//     other half; a pattern >= inf makes the group a NaN group;
//   * codes: v_cvt_scalef32_pk_fp4_f32 on register pairs.  Quad g becomes
//     half-word 2g + h of the group's 16 bytes; one swap of the two packed
//     words and two v_perm leave lane (r, h) with bytes 8h .. 8h+7: an 8-B
//     store per lane, 512 contiguous bytes per store instruction;
//   * scale bytes: OR-ed over each quad of lanes (two DPP moves), 4-B stores.
// Dequantize: lane (r, h) reads the 8 payload bytes of codes 16h .. 16h+15 of
// group r (512 contiguous bytes per tile) and decodes them to bf16 (exact) for
// 2 x v_mfma_f32_32x32x16_bf16 against H[16h + 8s + j][r].  A sum of 32 e2m1
// values is a multiple of 0.5 of magnitude <= 192: exact in any order, so
// restores are bit-identical to the torch reference; v_ldexp_f32 by k - 5 is
// the only other step.  The codes are the A operand here, NOT the transposed
// form of the quantizer.  Transposed, a lane owns 16 consecutive elements of
// one group after eight half-wave swaps, one scale byte per lane, but a store
// instruction then writes 16-B pieces 32 B (bf16) or 64 B (f32) apart: the
// restore of 512 Mi elements took 0.63 ms (bf16) and 1.91 ms (f32) beside
// hadamard32's 0.44 and 0.58 ms (profiles/mxfp4_hadamard/first_design_*).
// With the codes as A, register i is group (i&3) + 8(i>>2) + 4h, element r,
// as in hs_fp8_hadamard_dequant8: every store instruction writes whole groups
// (16-bit: through that kernel's lane-quad transpose, 8 B per lane), and a
// lane reads its 16 scale bytes as four words.  bf16: 0.28 ms, f32: 0.80 ms.
// The last tiles, and a source / payload / scale array / destination without
// the vector alignment (wave-uniform test), load and store element by element.
// ---------------------------------------------------------------------------

// tiles per iteration: 4 (bf16 / f16) or 8 (f32) 16-B loads in flight per lane
// (one f32 tile per iteration: 0.58 - 0.66 ms for 2 GiB, two: 0.57 - 0.64 ms)
constexpr int kFp4hQuantU = 2;
constexpr int kFp4hDequantU = 2;

// v_permlane32_swap: `a` of lanes 32..63 <-> `b` of lanes 0..31
__device__ __forceinline__ void half_swap(uint32_t& a, uint32_t& b) {
  const auto s = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  a = s[0];
  b = s[1];
}

// Scale byte and payload bytes 8h .. 8h+7 (`lo`, `hi`) of group r from the
// rotated tile.  Called by the whole wave.
__device__ __forceinline__ void fp4h_encode(const floatx16& acc, uint32_t& sb, uint32_t& lo,
                                            uint32_t& hi) {
  uint32_t key = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) key = max(key, __float_as_uint(acc[i]) & 0x7fffffffu);
  uint32_t other = key;
  half_swap(key, other);  // one of the two is the partner's, the other this lane's
  key = max(key, other);
  const bool nan = key >= kInfBits<kF32>;
  sb = nan ? kE8m0Nan : mxfp4_scale_byte<kF32>(key);
  const float scale = __uint_as_float(sb << 23);
  // w0: quads 0, 1 = half-words (h, 2 + h); w1: quads 2, 3 = (4 + h, 6 + h)
  uint32_t w0 = 0, w1 = 0;
  w0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w0, acc[0], acc[1], scale, 0);
  w0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w0, acc[2], acc[3], scale, 1);
  w0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w0, acc[4], acc[5], scale, 2);
  w0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w0, acc[6], acc[7], scale, 3);
  w1 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w1, acc[8], acc[9], scale, 0);
  w1 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w1, acc[10], acc[11], scale, 1);
  w1 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w1, acc[12], acc[13], scale, 2);
  w1 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w1, acc[14], acc[15], scale, 3);
  if (nan) w0 = w1 = 0;
  // h = 0 gives (4, 6) and takes (1, 3); h = 1 gives (1, 3) and takes (4, 6):
  // both then hold (even, even + 2) in w0 and (odd, odd + 2) in w1
  half_swap(w0, w1);
  lo = __builtin_amdgcn_perm(w1, w0, 0x05040100u);  // (w0.lo, w1.lo)
  hi = __builtin_amdgcn_perm(w1, w0, 0x07060302u);  // (w0.hi, w1.hi)
}

// `out` holds 16 * nblocks bytes, `scales` nblocks, nblocks = ceil(n / 32)
template <int DT, int U>
__global__ void __launch_bounds__(kBlock)
hs_mxfp4_hadamard_quant(const char* __restrict__ src, int64_t n, int64_t nblocks,
                        uint8_t* __restrict__ out, uint8_t* __restrict__ scales) {
  constexpr int ES = (DT == kF32) ? 4 : 2;
  constexpr int NV = ES;  // 16-B pieces of a lane's 16 elements
  const int lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  const int64_t ntiles = (nblocks + 31) / 32;
  const int64_t wave0 = int64_t(blockIdx.x) * (kBlock / 64) +
                        __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // scalar
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                       (reinterpret_cast<uintptr_t>(out) & 7) == 0 &&
                       (reinterpret_cast<uintptr_t>(scales) & 3) == 0;
  for (int64_t t0 = wave0 * U; t0 < ntiles; t0 += nwaves * U) {
    const bool full = aligned && (t0 + U) * 1024 <= n;
    mx_u32x4 x[U][NV];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        // f32: X[r][16h + 4v ..+3]; 16-bit: X[r][16v + 8h ..+7]
        const int64_t e0 = ((t0 + u) * 32 + r) * 32 + (DT == kF32 ? 16 * h + 4 * v : 16 * v + 8 * h);
        // plain loads: a 128-B line is shared by the pieces of several lanes and
        // load instructions, and nontemporal loads were slower (f32, 2 GiB: 0.82
        // - 0.88 ms against 0.57 - 0.64 ms; bf16: 0.272 against 0.262 ms)
        x[u][v] = full ? *reinterpret_cast<const mx_u32x4*>(src + e0 * ES)
                       : load16_elems<ES>(src, e0, n);  // past n: zeros
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (t0 + u >= ntiles) break;
      floatx16 acc = {};
      if constexpr (DT == kF32) {
#pragma unroll
        for (int t = 0; t < 16; ++t)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(hada(16 * h + t, r),
                                                     __uint_as_float(x[u][t >> 2][t & 3]), acc, 0, 0, 0);
      } else {
        acc = mfma16<DT>(hada_frag16<DT>(8 * h, r), __builtin_bit_cast(hs_i16x8, x[u][0]), acc);
        acc = mfma16<DT>(hada_frag16<DT>(16 + 8 * h, r), __builtin_bit_cast(hs_i16x8, x[u][1]), acc);
      }
      uint32_t sb, lo, hi;
      fp4h_encode(acc, sb, lo, hi);
      const int64_t group = (t0 + u) * 32 + r;
      if (full) {
        mx_u32x2 w;
        w.x = lo;
        w.y = hi;
        __builtin_nontemporal_store(w, reinterpret_cast<mx_u32x2*>(out + group * 16 + 8 * h));
        // byte (r & 3) of the quad's word, OR-ed over the quad
        uint32_t s4 = sb << (8 * (r & 3));
        s4 |= static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(s4), 0xB1, 0xF, 0xF, false));
        s4 |= static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(s4), 0x4E, 0xF, 0xF, false));
        if (h == 0 && (r & 3) == 0)
          __builtin_nontemporal_store(s4, reinterpret_cast<uint32_t*>(scales + group));
      } else if (group < nblocks) {
        if (h == 0) scales[group] = static_cast<uint8_t>(sb);
#pragma unroll
        for (int b = 0; b < 8; ++b)
          out[group * 16 + 8 * h + b] = static_cast<uint8_t>((b < 4 ? lo : hi) >> (8 * (b & 3)));
      }
    }
  }
}

// 8 e2m1 codes (one payload word, code j in nibble j) -> 8 bf16, exact
__device__ __forceinline__ hs_i16x8 fp4x8_to_bf16x8(uint32_t w) {
  mx_f32x2 p[4];  // the byte select must be an immediate
  p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 0);
  p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 1);
  p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 2);
  p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 3);
  hs_i16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = static_cast<short>(__float_as_uint(p[j >> 1][j & 1]) >> 16);
  return o;
}

// `q` holds 16 * nblocks bytes, `scales` nblocks; writes dst[0 .. n)
template <int DT, int U>
__global__ void __launch_bounds__(kBlock)
hs_mxfp4_hadamard_dequant(const uint8_t* __restrict__ q, const uint8_t* __restrict__ scales,
                          int64_t n, int64_t nblocks, char* __restrict__ dst) {
  constexpr int DES = (DT == kF32) ? 4 : (DT == kF64 ? 8 : 2);
  const int lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  const int64_t ntiles = (nblocks + 31) / 32;
  const int64_t wave0 = int64_t(blockIdx.x) * (kBlock / 64) +
                        __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // scalar
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const hs_i16x8 b0 = hada_frag16<kBF16>(16 * h, r), b1 = hada_frag16<kBF16>(16 * h + 8, r);
  const bool aligned = (reinterpret_cast<uintptr_t>(q) & 7) == 0 &&
                       (reinterpret_cast<uintptr_t>(scales) & 3) == 0 &&
                       (reinterpret_cast<uintptr_t>(dst) & (DES == 2 ? 7 : DES - 1)) == 0;
  for (int64_t t0 = wave0 * U; t0 < ntiles; t0 += nwaves * U) {
    const bool full = aligned && (t0 + U) * 1024 <= n;
    uint32_t raw[U][2];
    uint32_t sc[U][4];  // byte j of sc[u][g]: the scale of group 8g + 4h + j of tile u
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t g0 = (t0 + u) * 32;
      const uint8_t* p = q + (g0 + r) * 16 + 8 * h;
      if (full) {
        const mx_u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const mx_u32x2*>(p));
        raw[u][0] = w.x;
        raw[u][1] = w.y;
#pragma unroll
        for (int g = 0; g < 4; ++g)
          sc[u][g] = *reinterpret_cast<const uint32_t*>(scales + g0 + 8 * g + 4 * h);
      } else {
        raw[u][0] = raw[u][1] = 0;
        if (g0 + r < nblocks) {
#pragma unroll
          for (int b = 0; b < 8; ++b) raw[u][b >> 2] |= uint32_t(p[b]) << (8 * (b & 3));
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          sc[u][g] = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int64_t group = g0 + 8 * g + 4 * h + j;
            if (group < nblocks) sc[u][g] |= uint32_t(scales[group]) << (8 * j);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t tile = t0 + u;
      if (tile >= ntiles) break;
      floatx16 acc = {};
      acc = mfma16<kBF16>(fp4x8_to_bf16x8(raw[u][0]), b0, acc);
      acc = mfma16<kBF16>(fp4x8_to_bf16x8(raw[u][1]), b1, acc);
      float f[16];  // register i: group (i&3) + 8(i>>2) + 4h, element r
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t sb = (sc[u][i >> 2] >> (8 * (i & 3))) & 0xffu;
        f[i] = sb == kE8m0Nan ? __builtin_nanf("") : ldexpf(acc[i], int(sb) - 127 - 5);
      }
      if (full && DES == 2) {
        if constexpr (DES == 2) {
#pragma unroll
          for (int g = 0; g < 4; ++g)
            hada_store_quad16(pack16<DT>(f[4 * g], f[4 * g + 1]), pack16<DT>(f[4 * g + 2], f[4 * g + 3]),
                              r, dst + (tile * 32 + 8 * g + 4 * h) * 64);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int64_t e = (tile * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r;
          if (full || e < n) store_from_f32(dst + e * DES, DT, f[i]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Format probe (hs_quant_probe): what would each of the four un-rotated
// layouts lose on this tensor?  One read of the source, no payload.  For a
// format F with restore r_F into fp32 (ops/quant.py format_errors_reference
// states the sums once):
//   sumsq = sum x^2 and n_finite over the finite x; err2_F = sum (x - r_F)^2
//   over the elements where x and r_F are finite; spoiled_F = the number of
//   finite x whose r_F is not (the finite neighbours of a NaN in a NaN block,
//   the fp32-overflow edge of a code that rounds up).
// Work split: hs_mxfp4_quant's stream -- wave-contiguous 16-B loads, kStreamU
// in flight per lane, a grid-stride over chunks.  A lane's finite amax key
// (fp4_lane_key without the NaN key: MX fp8 keeps a NaN in its own element,
// so the block's finite amax is needed beside the NaN flag) is joined over
// the quad by DPP moves: after the step that covers 16 elements it is the
// two-level format's sub-block key, one step later the 32-block's, from whose
// one frexp the three E8M0 exponents (448, 7.5, 6) follow.  The NaN flags of
// the 16- and the 32-block take the same steps, but only in a wave that holds
// a non-finite value at all (one ballot).
// Round trips, all in registers, element for element the rules above:
//   * MX fp8: v_ldexp_f32, v_cvt_pk_fp8_f32, v_cvt_f32_fp8, v_ldexp_f32;
//   * MXFP4: the scaled fp4 conversion of the source words (fp4_pack), back
//     through v_cvt_scalef32_pk_f32_fp4 at scale 1 and v_ldexp_f32;
//   * two-level FP4: hs_nvfp4_quant's two divisions per block, v_med3_f32,
//     the fp4 conversion at scale 1, the decode and one product with d;
//   * MXFP6: gfx950 converts e2m3 a whole block at a time, which wants a lane
//     to own a block (hs_mxfp6_quant goes through LDS for that), while every
//     other step here wants a block across 4 or 8 lanes.  So the scaled value
//     is rounded to the e2m3 grid arithmetically: |y| <= 7.5 has the grid's
//     step 2^(max(e, 0) - 3) for |y| in [2^e, 2^(e + 1)), and (|y| + C) - C
//     with C = 2^(max(e, 0) + 20) is fp32's own round to nearest, ties to the
//     even multiple of that step, which is the even index (every segment of
//     the grid starts at an even index, a tie at a segment's end goes to the
//     next power of two).  Two additions and three integer operations per
//     element, no LDS, no second layout of the data.
// An element past n is a zero and an element that is not finite takes no part
// in any sum, so what its round trips give does not matter.
// Accumulation: e = x - r in fp32 (one rounding; finite for finite x and r,
// which have one sign), widened, squared and added in f64: first the lane's 8
// or 4 elements of a load, then, if that partial sum is finite (no x or r was
// not), into the lane's total.  Otherwise the elements go one by one under the
// mask of the lane's finite elements, which is also what is counted.  f64
// never overflows on fp32 squares; fp32 squares of bf16 values would.
// Reduction, in a fixed order: lanes by xor-shuffle, the workgroup's waves
// through LDS in wave order, each workgroup's ten partials into its own row of
// the scratch area behind the report (vector stores), then hs_quant_probe_sum,
// one wave per column, adds the rows: lane l rows l, l + 64, ..., then the
// same shuffle tree.  No atomics; the grid depends on n and the dtype only, so
// the report is a function of the tensor's bytes.
// ---------------------------------------------------------------------------

constexpr int kProbeMxfp4 = 1, kProbeNvfp4 = 2, kProbeMxfp6 = 4, kProbeMx8 = 8;  // candidates_mask
constexpr int kProbeFormats = 4;                // columns in that order: by size
constexpr int kProbeCols = 2 + 2 * kProbeFormats;  // sumsq, err2[4] (f64); n_finite, spoiled[4] (u64)
constexpr int kProbeAmaxWord = kProbeCols;      // low half: the tensor's amax A (f32)
constexpr int kProbeRowWords = 16;              // 8-byte words of a row: the report, then a row per workgroup
constexpr int kProbeGrid = 1024;                // workgroups at most

// one load's restored values `r` of format F against its sources `v`; `fin`:
// bit j set where element j is inside the tensor and finite
template <int EPL>
__device__ __forceinline__ void probe_add(const float* v, const float* r, uint32_t fin,
                                          double& err2, uint32_t& spoiled) {
  float e[EPL];
  double part = 0.;
#pragma unroll
  for (int j = 0; j < EPL; ++j) {
    e[j] = v[j] - r[j];
    part = __builtin_fma(static_cast<double>(e[j]), static_cast<double>(e[j]), part);
  }
  if (part < __builtin_huge_val()) {  // every x and r finite (an element past n: 0 - 0)
    err2 += part;
    return;
  }
#pragma unroll
  for (int j = 0; j < EPL; ++j) {
    if (!((fin >> j) & 1u)) continue;
    if (fabsf(e[j]) < __builtin_huge_valf())
      err2 = __builtin_fma(static_cast<double>(e[j]), static_cast<double>(e[j]), err2);
    else
      ++spoiled;
  }
}

// lane ^ o's `v`: a DPP quad move inside a quad, a wave shuffle beyond
__device__ __forceinline__ uint32_t probe_xor(uint32_t v, int o) {
  if (o == 1) return static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(int(v), 0xB1, 0xF, 0xF, false));
  if (o == 2) return static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(int(v), 0x4E, 0xF, 0xF, false));
  return static_cast<uint32_t>(__shfl_xor(int(v), o, 64));
}

// the wave's sum in every lane, by the xor tree: one order whatever the values
template <class T>
__device__ __forceinline__ T probe_wave_sum(T v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    if constexpr (std::is_same<T, double>::value) v += __shfl_xor(v, o, 64);
    else v += static_cast<T>(__shfl_xor(static_cast<long long>(v), o, 64));
  }
  return v;
}

template <int DT>
__global__ void HS_NO_PK_F32 __launch_bounds__(kBlock)
hs_quant_probe(const char* __restrict__ src, int64_t n, int mask,
               const uint32_t* __restrict__ amax, uint64_t* __restrict__ rows) {
  constexpr int ES = (DT == kF32) ? 4 : 2;
  constexpr int EPL = 16 / ES;    // elements per lane per load
  constexpr int LPB = 32 / EPL;   // lanes of a 32-block: 4 or 8
  constexpr int U = kStreamU;
  constexpr int64_t kChunk = 64LL * EPL * U;
  constexpr uint32_t kAll = (1u << EPL) - 1;
  __shared__ uint64_t wave_part[kBlock / 64][kProbeCols];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t wave0 = int64_t(blockIdx.x) * (kBlock / 64) + wave;  // scalar
  const int64_t nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  const bool want4 = mask & kProbeMxfp4, wantnv = mask & kProbeNvfp4;
  const bool want6 = mask & kProbeMxfp6, want8 = mask & kProbeMx8;
  const float ts = wantnv ? nvfp4_tensor_scale(__uint_as_float(*amax)) : 1.f;
  const float six_ts = 6.f * ts;
  double sumsq = 0., err2_4 = 0., err2_nv = 0., err2_6 = 0., err2_8 = 0.;
  uint32_t n_finite = 0, bad_4 = 0, bad_nv = 0, bad_6 = 0, bad_8 = 0;  // of this lane
  for (int64_t base = wave0 * kChunk; base < n; base += nwaves * kChunk) {
    const bool full = aligned && base + kChunk <= n;
    mx_u32x4 raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
      raw[u] = full ? __builtin_nontemporal_load(reinterpret_cast<const mx_u32x4*>(src + e0 * ES))
                    : load16_elems<ES>(src, e0, n);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const mx_u32x4 w = raw[u];
      bool nonfinite;
      uint32_t key32 = fp4_lane_key<DT, false>(w, nonfinite);
      uint32_t key16 = 0;
#pragma unroll
      for (int o = 1; o < LPB; o <<= 1) {
        key32 = max(key32, probe_xor(key32, o));
        if (2 * o == LPB / 2) key16 = key32;  // 16 elements joined: the two-level sub-block
      }
      // the lane's finite elements inside the tensor, and its blocks' NaN flags
      uint32_t fin = kAll;
      bool nan16 = false, nan32 = false;
      if (!full) {
        const int64_t e0 = base + (int64_t(u) * 64 + lane) * EPL;
        const int64_t left = n - e0;
        fin = left >= EPL ? kAll : (left > 0 ? (1u << left) - 1 : 0u);
      }
      if (__builtin_amdgcn_ballot_w64(nonfinite) != 0) {  // rare, wave-uniform
        uint32_t nan = 0;
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
          const uint32_t p = fp4_abs_bits<DT>(w, j);
          if (p >= kInfBits<DT>) fin &= ~(1u << j);
          if (p > kInfBits<DT>) nan = 1;
        }
#pragma unroll
        for (int o = 1; o < LPB; o <<= 1) {
          nan |= probe_xor(nan, o);
          if (2 * o == LPB / 2) nan16 = nan;
        }
        nan32 = nan;
      }
      n_finite += __popc(fin);
      float v[EPL], r[EPL];
      unpack16<DT>(w, v);
      {
        double part = 0.;
#pragma unroll
        for (int j = 0; j < EPL; ++j)
          part = __builtin_fma(static_cast<double>(v[j]), static_cast<double>(v[j]), part);
        if (part < __builtin_huge_val()) {
          sumsq += part;
        } else {
#pragma unroll
          for (int j = 0; j < EPL; ++j)
            if ((fin >> j) & 1u)
              sumsq = __builtin_fma(static_cast<double>(v[j]), static_cast<double>(v[j]), sumsq);
        }
      }
      // the three E8M0 exponents from one frexp of the block's amax
      int k8 = 0, k6 = 0, k4 = 0;
      const float bamax = fp4_key_value<DT>(key32);
      if (bamax > 0.f) {
        int e;
        const float m = frexpf(bamax, &e);
        k8 = max(-127, min(127, m <= 0.875f ? e - 9 : e - 8));
        k6 = max(-127, min(127, m <= 0.9375f ? e - 3 : e - 2));
        k4 = max(-127, min(127, m <= 0.75f ? e - 3 : e - 2));
      }
      const float qnan = __builtin_nanf("");
      if (want4) {
        const uint32_t code = fp4_pack<DT>(w, uint32_t(k4 + 127), false);
        mx_f32x2 p[EPL / 2];  // the byte select must be an immediate
        p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(code, 1.0f, 0);
        p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(code, 1.0f, 1);
        if constexpr (EPL == 8) {
          p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(code, 1.0f, 2);
          p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(code, 1.0f, 3);
        }
#pragma unroll
        for (int j = 0; j < EPL; ++j) r[j] = nan32 ? qnan : ldexpf(p[j >> 1][j & 1], k4);
        probe_add<EPL>(v, r, fin, err2_4, bad_4);
      }
      if (wantnv) {
        const float quot = fminf(fp4_key_value<DT>(key16) / six_ts, kFp8Max);
        const int s8 = __builtin_amdgcn_cvt_pk_fp8_f32(quot, 0.f, 0, false);
        const float d = __builtin_amdgcn_cvt_f32_fp8(s8, 0) * ts;
        const float inv = d > 0.f ? 1.f / d : 0.f;  // d == 0: the block restores as zeros
        float y[EPL];
#pragma unroll
        for (int j = 0; j < EPL; ++j) y[j] = __builtin_amdgcn_fmed3f(v[j] * inv, -6.f, 6.f);
        uint32_t code = 0;
        code = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(code, y[0], y[1], 1.0f, 0);
        code = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(code, y[2], y[3], 1.0f, 1);
        if constexpr (EPL == 8) {
          code = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(code, y[4], y[5], 1.0f, 2);
          code = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(code, y[6], y[7], 1.0f, 3);
        }
        mx_f32x2 p[EPL / 2];
        p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(code, 1.0f, 0);
        p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(code, 1.0f, 1);
        if constexpr (EPL == 8) {
          p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(code, 1.0f, 2);
          p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(code, 1.0f, 3);
        }
#pragma unroll
        for (int j = 0; j < EPL; ++j) r[j] = nan16 ? qnan : p[j >> 1][j & 1] * d;
        probe_add<EPL>(v, r, fin, err2_nv, bad_nv);
      }
      if (want6) {
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
          const uint32_t a = __float_as_uint(ldexpf(v[j], -k6)) & 0x7fffffffu;
          const float c = __uint_as_float((max(a >> 23, 127u) + 20u) << 23);
          const float q = (__uint_as_float(a) + c) - c;
          r[j] = nan32 ? qnan : copysignf(ldexpf(q, k6), v[j]);
        }
        probe_add<EPL>(v, r, fin, err2_6, bad_6);
      }
      if (want8) {
        float y[EPL];
#pragma unroll
        for (int j = 0; j < EPL; ++j) y[j] = ldexpf(v[j], -k8);
#pragma unroll
        for (int i = 0; i < EPL / 4; ++i) {
          int word = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * i], y[4 * i + 1], 0, false);
          word = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * i + 2], y[4 * i + 3], word, true);
#pragma unroll
          for (int b = 0; b < 4; ++b)
            r[4 * i + b] = ldexpf(fp8_byte_to_f32(static_cast<uint32_t>(word), b), k8);
        }
        probe_add<EPL>(v, r, fin, err2_8, bad_8);
      }
    }
  }
  // lanes, then waves, then this workgroup's row
  const double f[1 + kProbeFormats] = {probe_wave_sum(sumsq), probe_wave_sum(err2_4),
                                       probe_wave_sum(err2_nv), probe_wave_sum(err2_6),
                                       probe_wave_sum(err2_8)};
  const uint64_t c[1 + kProbeFormats] = {
      probe_wave_sum(uint64_t(n_finite)), probe_wave_sum(uint64_t(bad_4)),
      probe_wave_sum(uint64_t(bad_nv)), probe_wave_sum(uint64_t(bad_6)),
      probe_wave_sum(uint64_t(bad_8))};
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i <= kProbeFormats; ++i) {
      wave_part[wave][i] = __builtin_bit_cast(uint64_t, f[i]);
      wave_part[wave][1 + kProbeFormats + i] = c[i];
    }
  }
  __syncthreads();
  if (threadIdx.x < kProbeCols) {
    const int col = threadIdx.x;
    uint64_t word;
    if (col <= kProbeFormats) {
      double s = 0.;
      for (int i = 0; i < kBlock / 64; ++i) s += __builtin_bit_cast(double, wave_part[i][col]);
      word = __builtin_bit_cast(uint64_t, s);
    } else {
      word = 0;
      for (int i = 0; i < kBlock / 64; ++i) word += wave_part[i][col];
    }
    rows[int64_t(blockIdx.x) * kProbeRowWords + col] = word;
  }
}

// one wave per column: report[col] = the sum of rows[0 .. nrows)[col]
__global__ void __launch_bounds__(64)
hs_quant_probe_sum(const uint64_t* __restrict__ rows, int nrows, uint64_t* __restrict__ report) {
  const int col = blockIdx.x;
  const int lane = threadIdx.x;
  double f = 0.;
  uint64_t c = 0;
  for (int row = lane; row < nrows; row += 64) {
    const uint64_t word = rows[int64_t(row) * kProbeRowWords + col];
    if (col <= kProbeFormats) f += __builtin_bit_cast(double, word);
    else c += word;
  }
  f = probe_wave_sum(f);
  c = probe_wave_sum(c);
  if (lane == 0) report[col] = col <= kProbeFormats ? __builtin_bit_cast(uint64_t, f) : c;
}

// ---------------------------------------------------------------------------
// Region-scatter dequantizer (hs_dequant_regions): one launch decodes any
// number of N-d boxes of ONE quantized piece in HBM into strided destinations
// (the restore of a quantized FSDP / DTensor shard into another layout, and of
// a quantized tensor into a non-contiguous view).  Formats: MX fp8, MXFP4
// without rotation, MXFP6 and the two-level-scaled FP4 -- the ones whose
// element i is decodable on its own, its code and its scale byte at offsets
// computed from i.  The rotated formats need whole groups of 32 through the
// matrix cores and keep their kernels; so does the f32-scale block layout.
// The rules are the streaming kernels': the same device functions decode
// (fp8_byte_to_f32 + MxScale::restore, v_cvt_scalef32_pk_f32_fp4 +
// e8m0_restore / nvfp4_restore, fp6_decode32 + e8m0_restore) and round
// (pack16 / store_from_f32), so a region equals the whole piece's restore,
// narrowed, bit for bit.  One thing is stated here and nowhere else, and it is
// no rule of the format: the region restore is held to the bits of the torch
// CPU reference (ops/quant.py
// mx_dequantize_reference) also for the e4m3fn NaN codes of MX fp8 (a stored
// inf / NaN): torch widens the code 0x7F / 0xFF to the f32 sign | 0x7FF00000,
// which an f16 destination truncates to sign | 0x7F80 and which torch's
// vector f32 -> bf16 turns into 0xFFFF whatever the sign (qnan_store).
// hs_mx8_dequant leaves such an element as the NaN of v_cvt_f32_fp8 and of
// the destination's rounding, as it always did.
//
// Host: a region arrives with its dims collapsed against the piece's C order
// and the destination's strides (ops/native.py), innermost dim a run of
// consecutive source elements.  build_qtiles cuts every region into tiles
// {region, begin, end} in region-linear elements: whole runs where a run is
// shorter than a tile, else pieces of one run cut where the SOURCE index is a
// multiple of 32, so that no block, byte or 3-byte group is shared by two
// tiles' full groups.  Descriptors and tiles go up through a pinned stage into
// a device workspace, as in hsg_copy_nd.
//
// Device: workgroups of 256 walk the tile table.  The unit is an aligned group
// of 8 consecutive source elements -- 8 B of fp8, 4 B of fp4, 6 B of fp6; 8
// divides 16 and 32, so a group has one scale byte, loaded once.  A tile of R
// runs has R * G slots, G the largest number of groups a run of that length
// can touch; slot w is group w % G of run w / G (a 32-bit division), so
// adjacent lanes own adjacent groups of a run and a wave's payload loads are
// contiguous; a run that touches fewer groups leaves its last slot idle.  The
// run's outer coordinates cost one 64-bit division per outer dim but the first,
// per group.  The first and the last group of a run are masked per element.
// When the destination's innermost stride is 1, the group is whole and its
// address is 16-B aligned, it leaves as one nontemporal 16-B store (bf16 /
// f16) or two (f32); otherwise element by element.  The 6-bit codes of a group
// come out of two aligned dwords by a shift (a group starts 6 g bytes into the
// payload: 0 or 2 past a dword) and go through the block conversion with the
// other 24 codes zero.  No LDS.  A and ts of the two-level format are formed
// once, before the tile loop.
// ---------------------------------------------------------------------------

constexpr int kQMaxDims = 8;

enum QFormat : int32_t { kQMx8 = 0, kQMxfp4 = 1, kQMxfp6 = 2, kQNvfp4 = 3, kQFormats = 4 };

struct QRegion {
  char* dst;        // destination of the region's first element
  int64_t src0;     // piece-linear index of the region's first element
  int64_t numel;
  int32_t ndim;     // collapsed dims; the last one is a run of the source
  int32_t dst_dtype;
  int64_t sizes[kQMaxDims];
  int64_t src_strides[kQMaxDims];  // in elements of the piece
  int64_t dst_strides[kQMaxDims];  // in elements
};

struct QTile {
  int32_t region;
  int32_t pad;
  int64_t begin;  // region-linear elements
  int64_t end;
};

constexpr int64_t kQTileElems = 8192;  // smallest tile: 4 groups per lane (ops/native.py)

// an e4m3fn NaN code with sign bit `neg`, as the torch reference restores it
template <int DT>
__device__ __forceinline__ void qnan_store(char* p, uint32_t neg) {
  if constexpr (DT == kF32) *reinterpret_cast<uint32_t*>(p) = (neg << 31) | 0x7ff00000u;
  else if constexpr (DT == kF16) *reinterpret_cast<uint16_t*>(p) = uint16_t((neg << 15) | 0x7f80u);
  else *reinterpret_cast<uint16_t*>(p) = 0xffffu;
}

// the 8 decoded f32 values of the group at source element gs (a multiple of
// 8); MX fp8: bit j of `nan` for an e4m3fn NaN code, bit 8 + j its sign
template <int F>
__device__ __forceinline__ void qgroup_decode(const uint8_t* __restrict__ q,
                                              const uint8_t* __restrict__ scales, float ts,
                                              int64_t gs, float* f, uint32_t& nan) {
  nan = 0;
  if constexpr (F == kQMx8) {
    const uint2 w = *reinterpret_cast<const uint2*>(q + gs);
    const uint8_t sb = scales[gs >> 5];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = MxScale::restore(fp8_byte_to_f32(j < 4 ? w.x : w.y, j & 3), sb);
      const uint32_t code = ((j < 4 ? w.x : w.y) >> (8 * (j & 3))) & 0xffu;
      if ((code & 0x7fu) == 0x7fu) nan |= (1u << j) | ((code >> 7) << (8 + j));
    }
  } else if constexpr (F == kQMxfp6) {
    // 6 bytes at 6 * (gs / 8): the two dwords around them, shifted
    const int64_t at = (gs >> 3) * 6;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(q + (at & ~int64_t(3)));
    const uint64_t bits = ((uint64_t(w[1]) << 32) | w[0]) >> (8 * int(at & 3));
    const uint32_t c[6] = {uint32_t(bits), uint32_t(bits >> 32) & 0xffffu, 0, 0, 0, 0};
    const mx_f32x32 dec = fp6_decode32(c);
    const uint32_t sb = scales[gs >> 5];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = e8m0_restore(dec[j], sb);
  } else {
    const uint32_t raw = *reinterpret_cast<const uint32_t*>(q + (gs >> 1));
    mx_f32x2 p[4];  // the byte select must be an immediate
    p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw, 1.0f, 0);
    p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw, 1.0f, 1);
    p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw, 1.0f, 2);
    p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw, 1.0f, 3);
    const uint32_t sb = scales[F == kQNvfp4 ? gs >> 4 : gs >> 5];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      f[j] = F == kQNvfp4 ? nvfp4_restore(p[j >> 1][j & 1], sb, ts)
                          : e8m0_restore(p[j >> 1][j & 1], sb);
  }
}

template <int F, int DT>
__device__ __forceinline__ void qtile(const QRegion& r, int64_t begin, int64_t end,
                                      const uint8_t* __restrict__ q,
                                      const uint8_t* __restrict__ scales, float ts) {
  constexpr int DES = (DT == kF32) ? 4 : 2;
  const int nd = r.ndim;
  const int64_t L = r.sizes[nd - 1];
  const int64_t dinner = r.dst_strides[nd - 1];
  // whole runs [run0, run0 + nruns) of the region, or [lo, hi) of run run0
  const int64_t run0 = begin / L;
  int64_t lo = begin - run0 * L, hi = lo + (end - begin);
  uint32_t nruns = 1;
  if (lo == 0 && hi >= L) {
    nruns = static_cast<uint32_t>(hi / L);
    hi = L;
  }
  const uint32_t G = static_cast<uint32_t>((hi - lo + 6) / 8 + 1);  // groups a run can touch
  const uint32_t slots = nruns * G;
  for (uint32_t w = threadIdx.x; w < slots; w += kBlock) {
    const uint32_t lr = w / G, g = w - lr * G;
    int64_t rest = run0 + lr, soff = r.src0, doff = 0;
    for (int k = nd - 2; k >= 0; --k) {
      int64_t c = rest;
      if (k > 0) {
        const int64_t sz = r.sizes[k];
        rest = rest / sz;
        c -= rest * sz;
      }
      soff += c * r.src_strides[k];
      doff += c * r.dst_strides[k];
    }
    const int64_t S = soff + lo, E = soff + hi;  // the run's source elements
    const int64_t gs = (S & ~int64_t(7)) + 8 * int64_t(g);
    if (gs >= E) continue;
    float f[8];
    uint32_t nan;
    qgroup_decode<F>(q, scales, ts, gs, f, nan);
    char* p = r.dst + (doff + (gs - soff) * dinner) * DES;  // of element gs (maybe masked)
    if (nan) {  // rare: element stores, the NaN codes by their bits
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (gs + j < S || gs + j >= E) continue;
        if ((nan >> j) & 1) qnan_store<DT>(p + j * dinner * DES, (nan >> (8 + j)) & 1);
        else store_from_f32(p + j * dinner * DES, DT, f[j]);
      }
    } else if (dinner == 1 && gs >= S && gs + 8 <= E && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      if constexpr (DT == kF32) {
        fp4_store16<kF32>(p, f);
        fp4_store16<kF32>(p + 16, f + 4);
      } else {
        fp4_store16<DT>(p, f);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (gs + j >= S && gs + j < E) store_from_f32(p + j * dinner * DES, DT, f[j]);
    }
  }
}

template <int F>
__global__ void HS_NO_PK_F32 __launch_bounds__(kBlock)
hs_dequant_regions(const QRegion* __restrict__ regions, const QTile* __restrict__ tiles,
                   int64_t ntiles, const uint8_t* __restrict__ q,
                   const uint8_t* __restrict__ scales, const float* __restrict__ amax) {
  float ts = 0.f;
  if constexpr (F == kQNvfp4) ts = nvfp4_tensor_scale(*amax);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const QTile tile = tiles[t];
    const QRegion& r = regions[tile.region];
    switch (r.dst_dtype) {
      case kBF16: qtile<F, kBF16>(r, tile.begin, tile.end, q, scales, ts); break;
      case kF16: qtile<F, kF16>(r, tile.begin, tile.end, q, scales, ts); break;
      default: qtile<F, kF32>(r, tile.begin, tile.end, q, scales, ts); break;
    }
  }
}

// The tile table of a validated region batch.  Tiles grow with the batch so
// that a launch has about 4096 of them when there is that much work.
void build_qtiles(const QRegion* regions, int n, std::vector<QTile>* tiles) {
  int64_t total = 0;
  for (int i = 0; i < n; ++i) total += regions[i].numel;
  const int64_t tile = std::max(kQTileElems, std::min<int64_t>(kQTileElems * 32,
                                                               total / 4096 / 2048 * 2048));
  for (int i = 0; i < n; ++i) {
    const QRegion& r = regions[i];
    const int64_t L = r.sizes[r.ndim - 1], nruns = r.numel / L;
    if (L <= tile) {
      const int64_t per = tile / L;  // whole runs per tile
      for (int64_t run = 0; run < nruns; run += per)
        tiles->push_back(QTile{i, 0, run * L, std::min(nruns, run + per) * L});
      continue;
    }
    for (int64_t run = 0; run < nruns; ++run) {
      int64_t rest = run, s = r.src0;
      for (int k = r.ndim - 2; k >= 0; --k) {
        const int64_t c = k > 0 ? rest % r.sizes[k] : rest;
        rest = k > 0 ? rest / r.sizes[k] : 0;
        s += c * r.src_strides[k];
      }
      // cut where the source index is a multiple of 32 (tile % 32 == 0)
      for (int64_t b = 0, e = tile - (s & 31); b < L; b = e, e += tile)
        tiles->push_back(QTile{i, 0, run * L + b, run * L + std::min(e, L)});
    }
  }
}

// 0 if every region lies inside the piece of n elements and is well formed;
// else the error is set.  Nothing of a rejected batch is read on the device.
int check_qregions(const QRegion* regions, int nregions, int64_t n) {
  for (int i = 0; i < nregions; ++i) {
    const QRegion& r = regions[i];
    if (r.ndim < 1 || r.ndim > kQMaxDims) {
      hs_set_error("region %d: %d dims (1 to %d are supported)", i, r.ndim, kQMaxDims);
      return -1004;
    }
    if (r.dst_dtype != kBF16 && r.dst_dtype != kF16 && r.dst_dtype != kF32) {
      hs_set_error("region %d: unsupported destination dtype %d", i, r.dst_dtype);
      return -1002;
    }
    int64_t numel = 1, last = r.src0;
    bool ok = r.src0 >= 0 && r.src0 < n && r.dst != nullptr &&
              r.src_strides[r.ndim - 1] == 1;
    for (int k = 0; ok && k < r.ndim; ++k) {
      const int64_t sz = r.sizes[k], st = r.src_strides[k];
      // by division: no product is formed before it is known to stay below n
      ok = sz >= 1 && st >= 0 && numel <= n / sz &&
           (sz == 1 || st == 0 || sz - 1 <= (n - 1 - last) / st);
      if (!ok) break;
      numel *= sz;
      last += (sz - 1) * st;
    }
    if (!ok || numel != r.numel) {
      hs_set_error("region %d reaches outside the piece of %lld elements or is malformed", i,
                   static_cast<long long>(n));
      return -1005;
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Host dispatch: a runtime dtype code or vpt becomes a template argument by
// calling `f` with an integral_constant of it; kNoKernel where none fits.
// ---------------------------------------------------------------------------

constexpr int kNoKernel = 1;

template <int V>
using int_c = std::integral_constant<int, V>;

template <bool kWithF64, class F>
int for_dtype(int dt, F&& f) {
  switch (dt) {
    case kBF16: return f(int_c<kBF16>{});
    case kF16: return f(int_c<kF16>{});
    case kF32: return f(int_c<kF32>{});
    case kF64:
      if constexpr (kWithF64) return f(int_c<kF64>{});
      return kNoKernel;
    default: return kNoKernel;
  }
}

// blockwise fp8: block = 64 * vpt
template <class F>
int for_vpt(int vpt, F&& f) {
  switch (vpt) {
    case 2: return f(int_c<2>{});
    case 4: return f(int_c<4>{});
    case 8: return f(int_c<8>{});
    case 16: return f(int_c<16>{});
    default: hs_set_error("unsupported vpt %d", vpt); return -1001;
  }
}

int unsupported_dtype(const char* what, int dt) {
  hs_set_error("unsupported %s dtype %d", what, dt);
  return -1002;
}

int misaligned_amax(const void* amax) {
  hs_set_error("nvfp4 amax slot %p is not 4-byte aligned", amax);
  return -1003;
}

template <class... P, class... A>
int launch(void (*kernel)(P...), int grid, void* stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     static_cast<P>(args)...);
  HS_CHECK(hipGetLastError());
  return 0;
}

// workgroups of 4 waves, one wave per `per_wave` elements, at most `cap`
int grid_for(int64_t n, int64_t per_wave, int cap) {
  const int64_t waves = (n + per_wave - 1) / per_wave;
  return static_cast<int>(std::min<int64_t>((waves + 3) / 4, cap));
}

// elements of a streaming kernel's chunk: 16 B per lane, kStreamU deep
int64_t stream_chunk(int dtype) {
  return 64LL * kStreamU * (dtype == kF32 ? 4 : (dtype == kF64 ? 2 : 8));
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
  // streaming kernel: 16-B aligned source, 8-B aligned payload, a block
  // within one wave (bf16/f16 blocks of 128..512, f32 of 128..256)
  const bool aligned = (reinterpret_cast<uintptr_t>(src) % 16) == 0 &&
                       (reinterpret_cast<uintptr_t>(out) % 8) == 0;
  const int64_t chunk = stream_chunk(src_dtype);
  const int vgrid = static_cast<int>(std::max<int64_t>(
      1, std::min<int64_t>((n + chunk - 1) / chunk / 4 + 1, 256 * 16)));
  return for_vpt(vpt, [&](auto v) {
    constexpr int kVpt = decltype(v)::value;
    int rc = kNoKernel;
    if (aligned)
      rc = for_dtype<false>(src_dtype, [&](auto dt) {
        constexpr int kDt = decltype(dt)::value;
        if constexpr (kVpt <= (kDt == kF32 ? 4 : 8))  // lanes per block = 64 * vpt / EPL <= 64
          return launch(hs_fp8_quant_v<kDt, 64 * kVpt>, vgrid, stream, src, n, out, scales);
        else
          return kNoKernel;
      });
    if (rc != kNoKernel) return rc;
    return launch(hs_fp8_quant<kVpt>, grid_for(n, 64 * kVpt, 256 * 8), stream, src, src_dtype, n,
                  out, scales);
  });
}

int hsg_fp8_dequantize(int dev, const void* q, const void* scales, int64_t n, void* dst,
                       int dst_dtype, int vpt, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  // streaming kernel: 8-B aligned codes, 16-B aligned destination
  const bool aligned = (reinterpret_cast<uintptr_t>(q) % 8) == 0 &&
                       (reinterpret_cast<uintptr_t>(dst) % 16) == 0;
  const int vgrid = grid_for(n, stream_chunk(dst_dtype), 256 * 16);
  return for_vpt(vpt, [&](auto v) {
    constexpr int kVpt = decltype(v)::value;
    int rc = kNoKernel;
    if (aligned)
      rc = for_dtype<true>(dst_dtype, [&](auto dt) {
        return launch(hs_fp8_dequant_v<decltype(dt)::value, 64 * kVpt>, vgrid, stream, q, scales,
                      n, dst);
      });
    if (rc != kNoKernel) return rc;
    return launch(hs_fp8_dequant<kVpt>, grid_for(n, 4 * 64, 256 * 8), stream, q, scales, n, dst,
                  dst_dtype);
  });
}

// MX fp8: src (bf16/f16/f32, contiguous) -> out [payload = round_up(n, 16)
// bytes; [n, payload) zero-filled] + scales [ceil(n / 32) E8M0 bytes].  Every
// output byte is written (the blob needs no zero-fill).
int hsg_mx8_quantize(int dev, const void* src, int src_dtype, int64_t n, void* out,
                     void* scales, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  const int64_t payload = (n + 15) / 16 * 16;
  const int grid = grid_for(n, stream_chunk(src_dtype), 256 * 16);
  const int rc = for_dtype<false>(src_dtype, [&](auto dt) {
    return launch(hs_mx8_quant<decltype(dt)::value>, grid, stream, src, n, payload, out, scales);
  });
  return rc == kNoKernel ? unsupported_dtype("mx8 source", src_dtype) : rc;
}

int hsg_mx8_dequantize(int dev, const void* q, const void* scales, int64_t n, void* dst,
                       int dst_dtype, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  const int grid = grid_for(n, stream_chunk(dst_dtype), 256 * 16);
  const int rc = for_dtype<true>(dst_dtype, [&](auto dt) {
    return launch(hs_mx8_dequant<decltype(dt)::value>, grid, stream, q, scales, n, dst);
  });
  return rc == kNoKernel ? unsupported_dtype("mx8 dest", dst_dtype) : rc;
}

// MXFP4: src (bf16/f16/f32, contiguous, n elements) -> out [payload =
// round_up(ceil(n / 2), 16) bytes of e2m1 nibbles, zero from element n on] +
// scales [ceil(n / 32) E8M0 bytes].  Every output byte is written.
int hsg_mxfp4_quantize(int dev, const void* src, int src_dtype, int64_t n, void* out,
                       void* scales, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  const int64_t payload = ((n + 1) / 2 + 15) / 16 * 16;
  const int grid = grid_for(n, stream_chunk(src_dtype), 256 * 16);
  const int rc = for_dtype<false>(src_dtype, [&](auto dt) {
    return launch(hs_mxfp4_quant<decltype(dt)::value>, grid, stream, src, n, payload, out, scales);
  });
  return rc == kNoKernel ? unsupported_dtype("mxfp4 source", src_dtype) : rc;
}

int hsg_mxfp4_dequantize(int dev, const void* q, const void* scales, int64_t n, void* dst,
                         int dst_dtype, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  const int grid = grid_for(n, stream_chunk(dst_dtype), 256 * 16);
  const int rc = for_dtype<true>(dst_dtype, [&](auto dt) {
    return launch(hs_mxfp4_dequant<decltype(dt)::value>, grid, stream, q, scales, n, dst);
  });
  return rc == kNoKernel ? unsupported_dtype("mxfp4 dest", dst_dtype) : rc;
}

// Two-level-scaled FP4: src (bf16/f16/f32, contiguous, n elements) -> out
// [payload = round_up(ceil(n / 2), 16) bytes of e2m1 nibbles, zero from element
// n on] + scales [ceil(n / 16) e4m3fn bytes, zero-padded to a multiple of 4] +
// amax [one f32, 4-byte aligned: the amax over the finite elements].  Every
// output byte is written.  Three launches on `stream`: clear, amax, quantize.
int hsg_nvfp4_quantize(int dev, const void* src, int src_dtype, int64_t n, void* out,
                       void* scales, void* amax, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  if (reinterpret_cast<uintptr_t>(amax) & 3) return misaligned_amax(amax);
  const int64_t payload = ((n + 1) / 2 + 15) / 16 * 16;
  const int grid = grid_for(n, stream_chunk(src_dtype), 256 * 16);
  const int rc = for_dtype<false>(src_dtype, [&](auto dt) {
    constexpr int kDt = decltype(dt)::value;
    int r = launch(hs_nvfp4_clear, 1, stream, amax);
    if (r == 0)
      r = launch(hs_nvfp4_amax<kDt>,
                 grid_for(n, stream_chunk(src_dtype) / kStreamU * kAmaxU, kAmaxGrid), stream, src,
                 n, amax);
    if (r == 0) r = launch(hs_nvfp4_quant<kDt>, grid, stream, src, n, payload, out, scales, amax);
    return r;
  });
  return rc == kNoKernel ? unsupported_dtype("nvfp4 source", src_dtype) : rc;
}

int hsg_nvfp4_dequantize(int dev, const void* q, const void* scales, const void* amax, int64_t n,
                         void* dst, int dst_dtype, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  if (reinterpret_cast<uintptr_t>(amax) & 3) return misaligned_amax(amax);
  const int grid = grid_for(n, stream_chunk(dst_dtype), 256 * 16);
  const int rc = for_dtype<true>(dst_dtype, [&](auto dt) {
    return launch(hs_nvfp4_dequant<decltype(dt)::value>, grid, stream, q, scales, amax, n, dst);
  });
  return rc == kNoKernel ? unsupported_dtype("nvfp4 dest", dst_dtype) : rc;
}

// MXFP6: src (bf16/f16/f32, contiguous, n elements) -> out [payload =
// round_up(24 * ceil(n / 32), 16) bytes of e2m3 codes, zero from element n on]
// + scales [ceil(n / 32) E8M0 bytes].  Every output byte is written.
int hsg_mxfp6_quantize(int dev, const void* src, int src_dtype, int64_t n, void* out,
                       void* scales, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  const int64_t payload = (24 * ((n + 31) / 32) + 15) / 16 * 16;
  const int grid = grid_for(n, kFp6Step, 256 * 16);
  const int rc = for_dtype<false>(src_dtype, [&](auto dt) {
    return launch(hs_mxfp6_quant<decltype(dt)::value>, grid, stream, src, n, payload, out, scales);
  });
  return rc == kNoKernel ? unsupported_dtype("mxfp6 source", src_dtype) : rc;
}

int hsg_mxfp6_dequantize(int dev, const void* q, const void* scales, int64_t n, void* dst,
                         int dst_dtype, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  const int grid = grid_for(n, kFp6Step, 256 * 16);
  const int rc = for_dtype<true>(dst_dtype, [&](auto dt) {
    return launch(hs_mxfp6_dequant<decltype(dt)::value>, grid, stream, q, scales, n, dst);
  });
  return rc == kNoKernel ? unsupported_dtype("mxfp6 dest", dst_dtype) : rc;
}

// Hadamard-rotated MXFP4: src (bf16/f16/f32, contiguous, n elements) -> out
// [n_pad / 2 bytes of e2m1 nibbles] + scales [n_pad / 32 E8M0 bytes], n_pad =
// round_up(n, 32).  Every output byte is written.
int hsg_mxfp4_hadamard_quantize(int dev, const void* src, int src_dtype, int64_t n, void* out,
                                void* scales, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  const int64_t nblocks = (n + 31) / 32;
  const int rc = for_dtype<false>(src_dtype, [&](auto dt) {
    constexpr int kDt = decltype(dt)::value;
    constexpr int kU = kFp4hQuantU;
    return launch(hs_mxfp4_hadamard_quant<kDt, kU>, grid_for(nblocks * 32, 1024 * kU, 256 * 8),
                  stream, src, n, nblocks, out, scales);
  });
  return rc == kNoKernel ? unsupported_dtype("mxfp4 hadamard source", src_dtype) : rc;
}

int hsg_mxfp4_hadamard_dequantize(int dev, const void* q, const void* scales, int64_t n,
                                  void* dst, int dst_dtype, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  const int64_t nblocks = (n + 31) / 32;
  const int grid = grid_for(nblocks * 32, 1024 * kFp4hDequantU, 256 * 8);
  const int rc = for_dtype<true>(dst_dtype, [&](auto dt) {
    return launch(hs_mxfp4_hadamard_dequant<decltype(dt)::value, kFp4hDequantU>, grid, stream, q,
                  scales, n, nblocks, dst);
  });
  return rc == kNoKernel ? unsupported_dtype("mxfp4 hadamard dest", dst_dtype) : rc;
}

// Region-scatter dequantize (hs_dequant_regions above).  `regions` is a host
// array of `nregions` QRegion (ops/native.py DEQUANT_REGION_DTYPE) over ONE
// piece of `n` elements in format `format` (QFormat: 0 MX fp8, 1 MXFP4, 2
// MXFP6, 3 two-level FP4): `q` its payload (8-byte aligned; whole groups of 8
// codes are read, so it must be padded as the four layouts pad it, to a
// multiple of 16 bytes), `scales` its scale bytes, `amax` the f32 of format 3 (4-byte aligned; unused otherwise).
// `workspace` (device) and `pinned_stage` (host) hold at least
// hsg_dequant_regions_workspace_bytes() bytes: the tables go up on `stream`, so
// the host array may be reused when this returns.  A batch with a region that
// reaches outside the piece, has more than 8 dims or another destination
// dtype than bf16 / f16 / f32 is refused before anything is launched.
uint64_t hsg_dequant_region_size() { return sizeof(QRegion); }

// 0 and the error set for a batch that hsg_dequant_regions would refuse
uint64_t hsg_dequant_regions_workspace_bytes(const void* regions, int nregions, int64_t n) {
  const QRegion* r = static_cast<const QRegion*>(regions);
  if (!r) hs_set_error("null region table");
  if (!r || nregions <= 0 || n <= 0 || check_qregions(r, nregions, n) != 0) return 0;
  std::vector<QTile> tiles;
  build_qtiles(r, nregions, &tiles);
  return sizeof(QRegion) * nregions + sizeof(QTile) * tiles.size() + 256;
}

int hsg_dequant_regions(int dev, int format, const void* q, const void* scales, const void* amax,
                        int64_t n, const void* regions, int nregions, void* workspace,
                        uint64_t ws_bytes, void* pinned_stage, void* stream, int sync) {
  HS_CHECK(hipSetDevice(dev));
  if (nregions <= 0) return 0;
  if (format < 0 || format >= kQFormats) {
    hs_set_error("unknown quantized format id %d", format);
    return -1006;
  }
  if (!workspace || !pinned_stage || !regions) {
    hs_set_error("null %s", !regions ? "region table" : workspace ? "pinned stage" : "workspace");
    return -1007;
  }
  if (n <= 0 || !q || !scales || (reinterpret_cast<uintptr_t>(q) & 7)) {
    hs_set_error("payload %p of %lld elements: null, empty or not 8-byte aligned", q,
                 static_cast<long long>(n));
    return -1008;
  }
  if (format == kQNvfp4 && (!amax || (reinterpret_cast<uintptr_t>(amax) & 3)))
    return misaligned_amax(amax);
  const QRegion* r = static_cast<const QRegion*>(regions);
  if (const int rc = check_qregions(r, nregions, n)) return rc;
  std::vector<QTile> tiles;
  build_qtiles(r, nregions, &tiles);
  const size_t dbytes = sizeof(QRegion) * nregions;
  const size_t tbytes = sizeof(QTile) * tiles.size();
  const size_t toff = (dbytes + 255) / 256 * 256;
  if (toff + tbytes > ws_bytes) {
    hs_set_error("workspace too small: need %zu have %llu", toff + tbytes,
                 static_cast<unsigned long long>(ws_bytes));
    return -1000;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* stage = static_cast<char*>(pinned_stage);
  std::memcpy(stage, r, dbytes);
  std::memcpy(stage + toff, tiles.data(), tbytes);
  char* ws = static_cast<char*>(workspace);
  HS_CHECK(hipMemcpyAsync(ws, stage, toff + tbytes, hipMemcpyHostToDevice, s));
  const int64_t ntiles = static_cast<int64_t>(tiles.size());
  int grid = static_cast<int>(std::min<int64_t>(ntiles, 256 * 8));
  const int cap = hsg_thread_grid_cap();
  if (cap > 0) grid = std::min(grid, cap);
  const QRegion* dr = reinterpret_cast<const QRegion*>(ws);
  const QTile* dt = reinterpret_cast<const QTile*>(ws + toff);
  int rc;
  switch (format) {
    case kQMx8: rc = launch(hs_dequant_regions<kQMx8>, grid, stream, dr, dt, ntiles, q, scales, amax); break;
    case kQMxfp4: rc = launch(hs_dequant_regions<kQMxfp4>, grid, stream, dr, dt, ntiles, q, scales, amax); break;
    case kQMxfp6: rc = launch(hs_dequant_regions<kQMxfp6>, grid, stream, dr, dt, ntiles, q, scales, amax); break;
    default: rc = launch(hs_dequant_regions<kQNvfp4>, grid, stream, dr, dt, ntiles, q, scales, amax); break;
  }
  if (rc != 0) return rc;
  if (sync) HS_CHECK(hipStreamSynchronize(s));
  return 0;
}

// bytes of the `out` buffer of hsg_quant_probe: the report row, then a row of
// partial sums per workgroup
uint64_t hsg_quant_probe_out_bytes() {
  return uint64_t(1 + kProbeGrid) * kProbeRowWords * 8;
}

// Format probe: src (bf16/f16/f32, contiguous, n elements) -> the first 11
// 8-byte words of `out` (device memory, 8-byte aligned, hsg_quant_probe_out_
// bytes() long): sumsq and err2 of mxfp4, nvfp4, mxfp6, mx as f64; n_finite and
// spoiled of the same four as u64; the tensor's finite amax as an f32 in the
// low half of word 10 (only with the nvfp4 candidate).  `candidates_mask`: bit
// 0 mxfp4, 1 nvfp4, 2 mxfp6, 3 mx; the columns of the others are 0.  Launches
// on `stream` (clear and amax for nvfp4, probe, sum); copying the words to the
// host and waiting for them is the caller's.
int hsg_quant_probe(int dev, const void* src, int src_dtype, int64_t n, int candidates_mask,
                    void* out, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (reinterpret_cast<uintptr_t>(out) & 7) {
    hs_set_error("quant probe buffer %p is not 8-byte aligned", out);
    return -1004;
  }
  if (candidates_mask <= 0 || candidates_mask >= (1 << kProbeFormats)) {
    hs_set_error("quant probe candidates mask %d", candidates_mask);
    return -1005;
  }
  uint64_t* report = static_cast<uint64_t*>(out);
  uint64_t* rows = report + kProbeRowWords;
  uint32_t* amax = reinterpret_cast<uint32_t*>(report + kProbeAmaxWord);
  const int grid = n > 0 ? grid_for(n, stream_chunk(src_dtype), kProbeGrid) : 0;
  const int rc = for_dtype<false>(src_dtype, [&](auto dt) {
    constexpr int kDt = decltype(dt)::value;
    int r = 0;
    if (n > 0 && (candidates_mask & kProbeNvfp4)) {
      r = launch(hs_nvfp4_clear, 1, stream, amax);
      if (r == 0)
        r = launch(hs_nvfp4_amax<kDt>,
                   grid_for(n, stream_chunk(src_dtype) / kStreamU * kAmaxU, kAmaxGrid), stream,
                   src, n, amax);
    }
    if (r == 0 && n > 0)
      r = launch(hs_quant_probe<kDt>, grid, stream, src, n, candidates_mask, amax, rows);
    return r;
  });
  if (rc == kNoKernel) return unsupported_dtype("quant probe source", src_dtype);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(hs_quant_probe_sum, dim3(kProbeCols), dim3(64), 0,
                     static_cast<hipStream_t>(stream), rows, grid, report);
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
  constexpr int kHadU = 2;
  const int rc = for_dtype<false>(src_dtype, [&](auto dt) {
    constexpr int kDt = decltype(dt)::value;
    if constexpr (kDt == kF32)
      return launch(hs_fp8_hadamard_quant<kF32>, grid_for(n_pad, 1024, 256 * 8), stream, src, n,
                    n_pad, out, scales);
    else
      return launch(hs_fp8_hadamard_quant16<kDt, kHadU>, grid_for(n_pad, 1024 * kHadU, 256 * 8),
                    stream, src, n, n_pad, out, scales);
  });
  return rc == kNoKernel ? unsupported_dtype("hadamard source", src_dtype) : rc;
}

int hsg_fp8_hadamard_dequantize(int dev, const void* q, const void* scales, int64_t n, void* dst,
                                int dst_dtype, void* stream) {
  HS_CHECK(hipSetDevice(dev));
  if (n <= 0) return 0;
  const int64_t n_pad = (n + 31) / 32 * 32;
  constexpr int U = 2;
  const int grid = grid_for(n_pad, 1024 * U, 256 * 8);
  const int rc = for_dtype<true>(dst_dtype, [&](auto dt) {
    return launch(hs_fp8_hadamard_dequant8<decltype(dt)::value, U>, grid, stream, q, scales, n,
                  n_pad, dst);
  });
  return rc == kNoKernel ? unsupported_dtype("hadamard dest", dst_dtype) : rc;
}

}  // extern "C"
