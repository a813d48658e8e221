// dev_decoded16.h -- full-depth decoded pixels: decoded_kernel's (dev_decoded.h) planes and formulas with 65535 in the place of 255, stored as
// uint16, binary16 or binary32 samples in memory the caller describes (HWC or CHW, any byte strides that are multiples of the sample size).
//   decoded_q16          q16(n, d) = clamp(floor((2 * 65535 * n + d * peak) / (2 * d * peak)), 0, 65535), d and peak template arguments: the division is by a
//                        constant.  The BT.601 numerators reach 1.2e14: 64-bit words there, 32-bit ones where the bound allows (the RGB model, alpha)
//   deep_to_sample       D -> the bits of the target sample: D itself, or (float)((double)D * full_scale / 65535) -- an exact product, one binary64 division, one
//                        rounding to binary32 -- and for binary16 that value through float_to_half (dev_float.h)
//   wide_store_run       NDW dwords of contiguous samples in the widest stores the address allows: 16 bytes, 8, 4, halfwords
//   decoded_deep_kernel  decoded_kernel's launch, frame descriptors and plane loads.  A thread's four pixels of a packed HWC row are 24 / 32 bytes (16-bit
//                        samples, RGB / RGBA) or 48 / 64 (binary32); of a plane 8 or 16 bytes.  Any other stride and a last partial group: one store per sample.
//                        Decided per thread from its own addresses.  No LDS, no scratch.
// Loads stay inside the padded plane as decoded_kernel's do.  Only the visible w x h samples are stored.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_common.h"
#include "dev_slot.h"
#include "dev_decoded.h"                  // DecodedDst
#include "dev_float.h"                    // SAMPLE_*, float_to_half

namespace mi {

struct DecodedDeepDst : DecodedDst {                            // strides all multiples of the sample size
  int sample;                                                   // SAMPLE_U16 | SAMPLE_F16 | SAMPLE_F32
  float full_scale;                                             // floats only: finite, > 0
};

// D = d * peak.  NUM_MAX bounds 2 * 65535 * |n| + D over every sample value: where it fits 31 bits the quotient is taken in 32-bit words.
template <long long D, long long NUM_MAX> __device__ __forceinline__ uint32_t decoded_q16(const long long n) {
  if (NUM_MAX < (1ll << 31)) {
    const int num = 131070 * (int)n + (int)D;
    if (num < 0) return 0u;
    const uint32_t v = (uint32_t)num / (uint32_t)(2 * D);
    return v > 65535u ? 65535u : v;
  }
  const long long num = 131070 * n + D;
  if (num < 0) return 0u;
  const unsigned long long v = (unsigned long long)num / (unsigned long long)(2 * D);
  return v > 65535ull ? 65535u : (uint32_t)v;
}

// (r, g, b) of one pixel at full scale; MODEL 0 = YCbCr (matrix 6, full range), 1 = RGB (matrix 0, planes G, B, R)
template <int BD, int MODEL> __device__ __forceinline__ void decoded_rgb16(const int p0, const int p1, const int p2, uint32_t out[4]) {
  constexpr long long PEAK = (1 << BD) - 1, HALF = 1 << (BD - 1);
  if (MODEL == 1) {
    constexpr long long M = 131070 * PEAK + PEAK;
    out[0] = decoded_q16<PEAK, M>(p2); out[1] = decoded_q16<PEAK, M>(p0); out[2] = decoded_q16<PEAK, M>(p1);
    return;
  }
  const long long y = p0, cb = p1 - HALF, cr = p2 - HALF;
  out[0] = decoded_q16<1000 * PEAK, 131070 * (1000 * PEAK + 1402 * HALF) + 1000 * PEAK>(1000 * y + 1402 * cr);
  out[1] = decoded_q16<587000 * PEAK, 131070 * (587000 * PEAK + (202008 + 419198) * HALF) + 587000 * PEAK>(587000 * y - 202008 * cb - 419198 * cr);
  out[2] = decoded_q16<1000 * PEAK, 131070 * (1000 * PEAK + 1772 * HALF) + 1000 * PEAK>(1000 * y + 1772 * cb);
}

// the bits of the target sample of D (0..65535)
template <int SAMPLE> __device__ __forceinline__ uint32_t deep_to_sample(const uint32_t D, const float full_scale) {
  if (SAMPLE == SAMPLE_U16) return D;
  const float f = (float)(((double)D * (double)full_scale) / 65535.0);
  return SAMPLE == SAMPLE_F32 ? __builtin_bit_cast(uint32_t, f) : float_to_half(f);
}

// (all four samples, also for a target of three channels: leaving the fourth out costs registers and time, profiles/float_io.md)
template <int SAMPLE> __device__ __forceinline__ void deep_to_samples(const uint32_t D[4][4], const float full_scale, uint32_t o[4][4]) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
#pragma unroll
    for (int c = 0; c < 4; c++) o[j][c] = deep_to_sample<SAMPLE>(D[j][c], full_scale);
  }
}

// NDW (even) dwords of contiguous samples of SB bytes (2 | 4) to p, which is aligned to SB
template <int NDW, int SB> __device__ __forceinline__ void wide_store_run(uint8_t *p, const uint32_t d[NDW]) {
  const uintptr_t a = (uintptr_t)p;
  if ((a & 15) == 0) {
#pragma unroll
    for (int k = 0; k + 4 <= NDW; k += 4) { uint4 v; v.x = d[k]; v.y = d[k + 1]; v.z = d[k + 2]; v.w = d[k + 3]; *(uint4 *)(p + 4 * k) = v; }
    if (NDW & 2) { uint2 v; v.x = d[NDW - 2]; v.y = d[NDW - 1]; *(uint2 *)(p + 4 * (NDW - 2)) = v; }
  } else if ((a & 7) == 0) {
#pragma unroll
    for (int k = 0; k < NDW; k += 2) { uint2 v; v.x = d[k]; v.y = d[k + 1]; *(uint2 *)(p + 4 * k) = v; }
  } else if (SB == 4 || (a & 3) == 0) {
#pragma unroll
    for (int k = 0; k < NDW; k++) ((uint32_t *)p)[k] = d[k];
  } else {
#pragma unroll
    for (int k = 0; k < NDW; k++) { ((uint16_t *)p)[2 * k] = (uint16_t)d[k]; ((uint16_t *)p)[2 * k + 1] = (uint16_t)(d[k] >> 16); }
  }
}

// C samples of SB bytes per pixel: sample j (0 .. 4 C - 1) of a run into its dword
template <int SB> __device__ __forceinline__ void run_put(uint32_t *d, const int j, const uint32_t bits) {
  if (SB == 4) d[j] = bits;
  else if (j & 1) d[j >> 1] |= bits << 16;
  else d[j >> 1] = bits;
}
template <int SB> __device__ __forceinline__ void one_put(uint8_t *q, const uint32_t bits) {
  if (SB == 4) *(uint32_t *)q = bits;
  else *(uint16_t *)q = (uint16_t)bits;
}

// o[k][c] = the bits of sample c of pixel x0 + k (k < n) into the row at `row`
template <int SB> __device__ __forceinline__ void decoded_deep_store4(const DecodedDst &d, uint8_t *row, const uint32_t x0, const uint32_t n, const uint32_t o[4][4]) {
  if (d.layout == 0) {
    uint8_t *dst = row + (size_t)x0 * d.inner_stride;
    const bool packed = n == 4 && d.inner_stride == (unsigned long long)(d.channels * SB);
    if (packed && d.channels == 4) {
      uint32_t r[4 * SB];
#pragma unroll
      for (int k = 0; k < 4; k++) { run_put<SB>(r, 4 * k, o[k][0]); run_put<SB>(r, 4 * k + 1, o[k][1]); run_put<SB>(r, 4 * k + 2, o[k][2]); run_put<SB>(r, 4 * k + 3, o[k][3]); }
      wide_store_run<4 * SB, SB>(dst, r);
    } else if (packed) {
      uint32_t r[3 * SB];
#pragma unroll
      for (int k = 0; k < 4; k++) { run_put<SB>(r, 3 * k, o[k][0]); run_put<SB>(r, 3 * k + 1, o[k][1]); run_put<SB>(r, 3 * k + 2, o[k][2]); }
      wide_store_run<3 * SB, SB>(dst, r);
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) if (k < n) {
        uint8_t *q = dst + (size_t)k * d.inner_stride;
        one_put<SB>(q, o[k][0]); one_put<SB>(q + SB, o[k][1]); one_put<SB>(q + 2 * SB, o[k][2]);
        if (d.channels == 4) one_put<SB>(q + 3 * SB, o[k][3]);
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++) if (c < d.channels) {
      uint8_t *q = row + (size_t)c * d.inner_stride + (size_t)x0 * SB;
      if (n == 4) {
        uint32_t r[SB];
#pragma unroll
        for (int k = 0; k < 4; k++) run_put<SB>(r, k, o[k][c]);
        wide_store_run<SB, SB>(q, r);
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) if (k < n) one_put<SB>(q + k * SB, o[k][c]);
      }
    }
  }
}

// grid: (ceil(ceil(w / 4) / 64), h, images of the call)
template <int BD, int MODEL> __global__ void __launch_bounds__(64) decoded_deep_kernel(const FrameDev *frames, const DecodedDeepDst d) {
  const FrameDev *f = frames + d.first + blockIdx.z;
  RowGroup4 g;
  if (!row_group4((uint32_t)f->w, (uint32_t)f->h, g)) return;
  const uint32_t x0 = g.x0, y = g.y, k = g.img, n = g.n;
  constexpr long long PEAK = (1 << BD) - 1;
  uint32_t D[4][4];                                             // [pixel][R, G, B, A] at full scale
  {
    const size_t at = (size_t)y * f->stride + x0;               // 8-byte aligned, as in decoded_kernel
    const uint16_t *const *pl = d.source ? f->src : (f->enable_restoration ? f->lrp : f->fin);
    const uint2 a = *(const uint2 *)(pl[0] + at), b = *(const uint2 *)(pl[1] + at), c = *(const uint2 *)(pl[2] + at);
    const int s0[4] = { (int)(a.x & 0xFFFFu), (int)(a.x >> 16), (int)(a.y & 0xFFFFu), (int)(a.y >> 16) };
    const int s1[4] = { (int)(b.x & 0xFFFFu), (int)(b.x >> 16), (int)(b.y & 0xFFFFu), (int)(b.y >> 16) };
    const int s2[4] = { (int)(c.x & 0xFFFFu), (int)(c.x >> 16), (int)(c.y & 0xFFFFu), (int)(c.y >> 16) };
#pragma unroll
    for (int j = 0; j < 4; j++) { decoded_rgb16<BD, MODEL>(s0[j], s1[j], s2[j], D[j]); D[j][3] = 65535u; }
  }
  if (d.alpha_frames) {
    const FrameDev *fa = frames + d.n + d.first + k;
    if (!frame_idle(fa)) {
      const uint16_t *pa = d.source ? fa->src[0] : (fa->enable_restoration ? fa->lrp[0] : fa->fin[0]);
      const uint2 a = *(const uint2 *)(pa + (size_t)y * fa->stride + x0);
      const int s[4] = { (int)(a.x & 0xFFFFu), (int)(a.x >> 16), (int)(a.y & 0xFFFFu), (int)(a.y >> 16) };
#pragma unroll
      for (int j = 0; j < 4; j++) D[j][3] = decoded_q16<PEAK, 131070 * PEAK + PEAK>(s[j]);
    }
  }
  uint8_t *row = d.base + (size_t)k * d.image_stride + (size_t)y * d.row_stride;
  uint32_t o[4][4];
  if (d.sample == SAMPLE_F32) { deep_to_samples<SAMPLE_F32>(D, d.full_scale, o); decoded_deep_store4<4>(d, row, x0, n, o); }
  else {
    if (d.sample == SAMPLE_F16) deep_to_samples<SAMPLE_F16>(D, d.full_scale, o);
    else deep_to_samples<SAMPLE_U16>(D, d.full_scale, o);
    decoded_deep_store4<2>(d, row, x0, n, o);
  }
}

}  // namespace mi
