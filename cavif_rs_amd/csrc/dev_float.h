// dev_float.h -- float sources: binary16 and binary32 pictures in device memory -> the deep slot of a batch (dev_deep.h), and the conversions
// between the float formats and the slot's 16-bit samples that decoded_deep_kernel (dev_decoded16.h) shares.
//   half_to_float / float_to_half   binary16 <-> binary32 in integer bit arithmetic (the emulated build compiles them with g++): exact one way (subnormal halves
//                          are values), round to nearest even the other
//   float_to_deep          the sample map of include/mi_avif.h: NaN and v <= 0 give 0, v >= full_scale gives 65535, else rint((double)v * 65535 / full_scale).
//                          The product is exact in binary64 (24 by 16 bits) and the division is its one rounding, skipped when full_scale is 1
//   wide_load_run          NDW dwords of contiguous samples in the widest loads the address allows: 16 bytes, 8, 4, halfwords
//   ingest_float_kernel    ingest16_kernel's counterpart: HWC or CHW pictures, any byte strides that are multiples of the sample size, in the row groups of
//                          dev_slot.h.  A thread's four pixels of a packed f32 row are 48 (RGB) or 64 (RGBA) bytes: three or four 16-byte loads where the
//                          address is 16-byte aligned; of a packed f16 row 24 or 32 bytes; of a plane 16 (f32) or 8 (f16) bytes.  Any other stride and a last
//                          partial group: one load per sample.  Decided per thread from its own addresses.  No LDS, no scratch; one launch for all images of a call.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_slot.h"
#include "dev_ingest.h"                   // IngestSrc

namespace mi {

constexpr int SAMPLE_U16 = 1, SAMPLE_F16 = 2, SAMPLE_F32 = 3;   // MI_SAMPLE_*

struct IngestFloatSrc : IngestSrc {                             // strides all multiples of the sample size; 3 channels into an RGBA slot: alpha 65535
  int sample;                                                   // SAMPLE_F16 | SAMPLE_F32
  float full_scale;                                             // finite, > 0
};

// the bits of a binary16 as the binary32 of the same value
__device__ __forceinline__ float half_to_float(const uint32_t h) {
  const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
  if (e == 0) {                                                 // zero or subnormal: m * 2^-24, a normal binary32
    const float f = (float)(int)m * 5.9604644775390625e-8f;     // (exact: a power of two times an integer below 2^10)
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) | sign);
  }
  return __builtin_bit_cast(float, sign | (e == 31 ? 0x7F800000u : (e + 112u) << 23) | (m << 13));
}

// the bits of the binary16 nearest to f, ties to even; beyond 65504 + half an ulp: infinity
__device__ __forceinline__ uint32_t float_to_half(const float f) {
  uint32_t x = __builtin_bit_cast(uint32_t, f);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7FFFFFFFu;
  if (x > 0x7F800000u) return sign | 0x7E00u | ((x >> 13) & 0x3FFu);                          // NaN
  if (x >= 0x477FF000u) return sign | 0x7C00u;                  // 65520 and above (infinity included)
  if (x <= 0x33000000u) return sign;                            // up to 2^-25: half of the smallest subnormal goes to the even neighbour, zero
  if (x < 0x38800000u) {                                        // below 2^-14: a subnormal half, mant * 2^(exp - 150) in units of 2^-24
    const uint32_t shift = 126u - (x >> 23), mant = (x & 0x7FFFFFu) | 0x800000u;              // shift = 14 .. 24
    uint32_t h = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), tie = 1u << (shift - 1u);
    if (rem > tie || (rem == tie && (h & 1u))) h++;             // (a carry out of the mantissa gives the smallest normal half: the right bits)
    return sign | h;
  }
  uint32_t h = (x - 0x38000000u) >> 13;
  const uint32_t rem = x & 0x1FFFu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;       // (a carry goes into the exponent; infinity was decided above)
  return sign | h;
}

// ONE = full_scale is 1: the division by it changes nothing and is left out
template <bool ONE> __device__ __forceinline__ uint32_t float_to_deep(const float v, const float full_scale) {
  if (!(v > 0.0f)) return 0u;                                   // NaN, -inf, negatives, both zeros
  if (v >= full_scale) return 65535u;                           // +inf included
  const double p = (double)v * 65535.0;
  return (uint32_t)__builtin_rint(ONE ? p : p / (double)full_scale);
}

// NDW (even) dwords of contiguous samples of SB bytes (2 | 4) at p, which is aligned to SB
template <int NDW, int SB> __device__ __forceinline__ void wide_load_run(const uint8_t *p, uint32_t d[NDW]) {
  const uintptr_t a = (uintptr_t)p;
  if ((a & 15) == 0) {
#pragma unroll
    for (int k = 0; k + 4 <= NDW; k += 4) { const uint4 v = *(const uint4 *)(p + 4 * k); d[k] = v.x; d[k + 1] = v.y; d[k + 2] = v.z; d[k + 3] = v.w; }
    if (NDW & 2) { const uint2 v = *(const uint2 *)(p + 4 * (NDW - 2)); d[NDW - 2] = v.x; d[NDW - 1] = v.y; }
  } else if ((a & 7) == 0) {
#pragma unroll
    for (int k = 0; k < NDW; k += 2) { const uint2 v = *(const uint2 *)(p + 4 * k); d[k] = v.x; d[k + 1] = v.y; }
  } else if (SB == 4 || (a & 3) == 0) {
#pragma unroll
    for (int k = 0; k < NDW; k++) d[k] = ((const uint32_t *)p)[k];
  } else {
#pragma unroll
    for (int k = 0; k < NDW; k++) d[k] = (uint32_t)((const uint16_t *)p)[2 * k] | ((uint32_t)((const uint16_t *)p)[2 * k + 1] << 16);
  }
}

// sample j of such a run as a binary32
template <int SB> __device__ __forceinline__ float run_sample(const uint32_t *d, const int j) {
  if (SB == 4) return __builtin_bit_cast(float, d[j]);
  return half_to_float((d[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
}
template <int SB> __device__ __forceinline__ float one_sample(const uint8_t *q) {
  if (SB == 4) return *(const float *)q;
  return half_to_float(*(const uint16_t *)q);
}

// v[k][c] = sample c of pixel x0 + k of the row at `row` (k < n; channels the source does not have and pixels past n are left at 0)
template <int SB> __device__ __forceinline__ void ingest_float_load4(const IngestSrc &s, const uint8_t *row, const uint32_t x0, const uint32_t n, float v[4][4]) {
#pragma unroll
  for (int k = 0; k < 4; k++) { v[k][0] = v[k][1] = v[k][2] = v[k][3] = 0.0f; }
  if (s.layout == 0) {
    const uint8_t *p = row + (size_t)x0 * s.inner_stride;
    const bool packed = n == 4 && s.inner_stride == (unsigned long long)(s.channels * SB);
    if (packed && s.channels == 4) {
      uint32_t d[4 * SB];
      wide_load_run<4 * SB, SB>(p, d);
#pragma unroll
      for (int k = 0; k < 4; k++) { v[k][0] = run_sample<SB>(d, 4 * k); v[k][1] = run_sample<SB>(d, 4 * k + 1); v[k][2] = run_sample<SB>(d, 4 * k + 2); v[k][3] = run_sample<SB>(d, 4 * k + 3); }
    } else if (packed) {
      uint32_t d[3 * SB];
      wide_load_run<3 * SB, SB>(p, d);
#pragma unroll
      for (int k = 0; k < 4; k++) { v[k][0] = run_sample<SB>(d, 3 * k); v[k][1] = run_sample<SB>(d, 3 * k + 1); v[k][2] = run_sample<SB>(d, 3 * k + 2); }
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) if (k < n) {
        const uint8_t *q = p + (size_t)k * s.inner_stride;
        v[k][0] = one_sample<SB>(q); v[k][1] = one_sample<SB>(q + SB); v[k][2] = one_sample<SB>(q + 2 * SB);
        if (s.channels == 4) v[k][3] = one_sample<SB>(q + 3 * SB);
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++) if (c < s.channels) {
      const uint8_t *q = row + (size_t)c * s.inner_stride + (size_t)x0 * SB;
      if (n == 4) {
        uint32_t d[SB];
        wide_load_run<SB, SB>(q, d);
#pragma unroll
        for (int k = 0; k < 4; k++) v[k][c] = run_sample<SB>(d, k);
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) if (k < n) v[k][c] = one_sample<SB>(q + k * SB);
      }
    }
  }
}

template <bool ONE> __device__ __forceinline__ void float_to_deep4(const float v[4][4], const int channels, const float full_scale, uint2 px[4]) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t r = float_to_deep<ONE>(v[k][0], full_scale), g = float_to_deep<ONE>(v[k][1], full_scale), b = float_to_deep<ONE>(v[k][2], full_scale);
    const uint32_t a = channels == 4 ? float_to_deep<ONE>(v[k][3], full_scale) : 0xFFFFu;
    px[k].x = r | (g << 16); px[k].y = b | (a << 16);
  }
}

// slots = deep slot of the first image
template <int DC> __global__ void __launch_bounds__(64) ingest_float_kernel(const IngestFloatSrc s, uint16_t *slots) {
  RowGroup4 g;
  if (!row_group4(s.w, s.h, g)) return;
  const uint8_t *row = s.base + (size_t)g.img * s.image_stride + (size_t)g.y * s.row_stride;
  float v[4][4];
  if (s.sample == SAMPLE_F32) ingest_float_load4<4>(s, row, g.x0, g.n, v);
  else ingest_float_load4<2>(s, row, g.x0, g.n, v);
  uint2 px[4];
  if (s.full_scale == 1.0f) float_to_deep4<true>(v, s.channels, s.full_scale, px);
  else float_to_deep4<false>(v, s.channels, s.full_scale, px);
  slot16_store4<DC>(slot_ptr<DC>(slots, s.w, s.h, g), px, g.n);
}

}  // namespace mi
