// Internal to _hsgpu.so (not part of the ABI): what more than one of its
// files needs -- the launch block size, the dtype codes, the error channel,
// the conversion helpers the copy and the quantization kernels share, and the
// few host functions one file calls in another.  Everything declared here has
// hidden visibility or internal linkage: nothing of it is exported.

#ifndef HIPSNAPSHOT_HSGPU_COMMON_H_
#define HIPSNAPSHOT_HSGPU_COMMON_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hsgpu_hooks.h"

#define HS_HIDDEN __attribute__((visibility("hidden")))

constexpr int kBlock = 256;              // 4 waves of 64
constexpr int64_t kTileBytes = 1 << 20;  // largest tile of a tile table (copy, batched hash)

// dtype codes shared with python (hipsnapshot/ops/native.py)
enum DType : int32_t {
  kRaw1 = 0, kRaw2 = 1, kRaw4 = 2, kRaw8 = 3, kRaw16 = 4,  // same-type copies
  kF16 = 10, kBF16 = 11, kF32 = 12, kF64 = 13,
};

// ---- the library's one error channel ---------------------------------------
// A message per thread, read with hsg_last_error().  Every exported hsg_*
// function sets it before it returns a failure, so a caller reads the text of
// the call it just made, on the thread it made it on.  The text is formatted
// aside and then copied, so an argument may be the current message itself.
// Defined in hsgpu.hip.
HS_HIDDEN void hs_set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

#define HS_CHECK(expr)                                      \
  do {                                                      \
    hipError_t _e = (expr);                                 \
    if (_e != hipSuccess) {                                 \
      hs_set_error("%s: %s", #expr, hipGetErrorString(_e)); \
      return -static_cast<int>(_e) - 1;                     \
    }                                                       \
  } while (0)

// ---- host functions used across files --------------------------------------
// Copy stream (dev, slot) and its event, created on first use (hsgpu.hip).
HS_HIDDEN int hs_get_stream(int dev, int slot, hipStream_t* out, hipEvent_t* ev);
// One kernel of each kernel file, for hsg_prewarm_module: every file is a
// code object of its own, loaded when one of its kernels is first needed.
HS_HIDDEN const void* hs_copy_kernel();   // hscopy.hip
HS_HIDDEN const void* hs_quant_kernel();  // hsquant.hip
HS_HIDDEN const void* hs_hash_kernel();   // hshash.hip

// ---- conversions shared by the copy and the quantization kernels -----------

static __device__ __forceinline__ float bf16_to_f32(uint16_t v) {
  return __uint_as_float(static_cast<uint32_t>(v) << 16);
}

static __device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  // round-to-nearest-even, NaN preserved (matches torch's c10::BFloat16)
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<uint16_t>((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return static_cast<uint16_t>(u >> 16);
}

static __device__ __forceinline__ float load_as_f32(const char* p, int32_t dt) {
  switch (dt) {
    case kF16: return static_cast<float>(*reinterpret_cast<const _Float16*>(p));
    case kBF16: return bf16_to_f32(*reinterpret_cast<const uint16_t*>(p));
    case kF32: return *reinterpret_cast<const float*>(p);
    default: return static_cast<float>(*reinterpret_cast<const double*>(p));
  }
}

static __device__ __forceinline__ void store_from_f32(char* p, int32_t dt, float v) {
  switch (dt) {
    case kF16: {
      // the empty asm pins v as an f32: otherwise a caller's f32 multiply and
      // this fptrunc may be fused into one mixed-precision FMA (a single
      // rounding to f16), which differs from torch's f32 -> f16 in rare ties
      asm volatile("" : "+v"(v));
      *reinterpret_cast<_Float16*>(p) = static_cast<_Float16>(v);
      break;
    }
    case kBF16: *reinterpret_cast<uint16_t*>(p) = f32_to_bf16(v); break;
    case kF32: *reinterpret_cast<float*>(p) = v; break;
    default: *reinterpret_cast<double*>(p) = static_cast<double>(v); break;
  }
}

#endif  // HIPSNAPSHOT_HSGPU_COMMON_H_
