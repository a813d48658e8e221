// dev_decoded.h -- decoded pixels of a finished encode: the final reconstruction (lrp when the frame runs loop restoration, else fin) or the
// source planes of every image of a call -> 8-bit RGB or RGBA in memory the caller describes (HWC or CHW, any byte strides that do not make rows overlap).
//   decoded_q         q(n, d) = clamp(floor((2 * 255 * n + d * peak) / (2 * d * peak)), 0, 255): 255 n / (d peak) rounded half up, in integers.  d and peak are
//                     template arguments, so the division is by a constant (multiply-high); the word size is the smallest that holds every numerator.
//   decoded_kernel    one launch for images [first, first + count), driven by the frame descriptors the encode left on the device (as quality_kernel is): the
//                     colour frame of image i is frames[i], its alpha frame frames[n + i] when the batch has four channels and the frame is not idle.  In the
//                     row groups of dev_slot.h over the frame's own w x h: one 8-byte load per plane and
//                     thread, then slot_store4 for packed HWC (16 bytes for RGBA, three dwords for RGB), one dword per plane for CHW, byte stores for any other
//                     stride or alignment and for a last partial group: decided per thread from its own addresses.  No LDS, no scratch.
// Loads stay inside the padded plane: columns come in fours from x0 < w, and the stride is a multiple of 64.  Only the visible w x h pixels are stored.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_common.h"
#include "dev_slot.h"

namespace mi {

struct DecodedDst {
  uint8_t *base;                                                // image k of the call at base + k * image_stride
  unsigned long long image_stride, row_stride, inner_stride;    // bytes; inner: from pixel to pixel (HWC) or from plane to plane (CHW)
  int layout, channels;                                         // 0 = HWC, 1 = CHW; 3 | 4
  int first, n;                                                 // first image of the call; images of the run (the alpha frame of image i is frame n + i)
  int alpha_frames;                                             // the batch has four channels: alpha frames exist
  int source;                                                   // 0 = the final reconstruction, 1 = the source planes
};

// D = d * peak.  NUM_MAX bounds 2 * 255 * |n| + D over every sample value: where it fits 31 bits the quotient is taken in 32-bit words.
template <long long D, long long NUM_MAX> __device__ __forceinline__ uint32_t decoded_q(const long long n) {
  if (NUM_MAX < (1ll << 31)) {
    const int num = 510 * (int)n + (int)D;
    if (num < 0) return 0u;
    const uint32_t v = (uint32_t)num / (uint32_t)(2 * D);
    return v > 255u ? 255u : v;
  }
  const long long num = 510 * n + D;
  if (num < 0) return 0u;
  const unsigned long long v = (unsigned long long)num / (unsigned long long)(2 * D);
  return v > 255ull ? 255u : (uint32_t)v;
}

// r | g << 8 | b << 16 of one pixel; MODEL 0 = YCbCr (matrix 6, full range), 1 = RGB (matrix 0, planes G, B, R)
template <int BD, int MODEL> __device__ __forceinline__ uint32_t decoded_rgb(const int p0, const int p1, const int p2) {
  constexpr long long PEAK = (1 << BD) - 1, HALF = 1 << (BD - 1);
  if (MODEL == 1) {
    constexpr long long M = 510 * PEAK + PEAK;
    return decoded_q<PEAK, M>(p2) | (decoded_q<PEAK, M>(p0) << 8) | (decoded_q<PEAK, M>(p1) << 16);
  }
  const long long y = p0, cb = p1 - HALF, cr = p2 - HALF;
  const uint32_t r = decoded_q<1000 * PEAK, 510 * (1000 * PEAK + 1402 * HALF) + 1000 * PEAK>(1000 * y + 1402 * cr);
  const uint32_t g = decoded_q<587000 * PEAK, 510 * (587000 * PEAK + (202008 + 419198) * HALF) + 587000 * PEAK>(587000 * y - 202008 * cb - 419198 * cr);
  const uint32_t b = decoded_q<1000 * PEAK, 510 * (1000 * PEAK + 1772 * HALF) + 1000 * PEAK>(1000 * y + 1772 * cb);
  return r | (g << 8) | (b << 16);
}

// grid: (ceil(ceil(w / 4) / 64), h, images of the call)
template <int BD, int MODEL> __global__ void __launch_bounds__(64) decoded_kernel(const FrameDev *frames, const DecodedDst d) {
  const FrameDev *f = frames + d.first + blockIdx.z;
  RowGroup4 g;
  if (!row_group4((uint32_t)f->w, (uint32_t)f->h, g)) return;
  const uint32_t x0 = g.x0, y = g.y, k = g.img, n = g.n;
  constexpr long long PEAK = (1 << BD) - 1;
  uint32_t px[4];
  {
    const size_t at = (size_t)y * f->stride + x0;                                                       // 8-byte aligned: planes are 256-byte aligned, x0 and the stride multiples of 4
    const uint16_t *const *pl = d.source ? f->src : (f->enable_restoration ? f->lrp : f->fin);
    const uint2 a = *(const uint2 *)(pl[0] + at), b = *(const uint2 *)(pl[1] + at), c = *(const uint2 *)(pl[2] + at);
    const int s0[4] = { (int)(a.x & 0xFFFFu), (int)(a.x >> 16), (int)(a.y & 0xFFFFu), (int)(a.y >> 16) };
    const int s1[4] = { (int)(b.x & 0xFFFFu), (int)(b.x >> 16), (int)(b.y & 0xFFFFu), (int)(b.y >> 16) };
    const int s2[4] = { (int)(c.x & 0xFFFFu), (int)(c.x >> 16), (int)(c.y & 0xFFFFu), (int)(c.y >> 16) };
#pragma unroll
    for (int j = 0; j < 4; j++) px[j] = decoded_rgb<BD, MODEL>(s0[j], s1[j], s2[j]) | 0xFF000000u;
  }
  if (d.alpha_frames) {
    const FrameDev *fa = frames + d.n + d.first + k;
    if (!frame_idle(fa)) {
      const uint16_t *pa = d.source ? fa->src[0] : (fa->enable_restoration ? fa->lrp[0] : fa->fin[0]);
      const uint2 a = *(const uint2 *)(pa + (size_t)y * fa->stride + x0);
      const int s[4] = { (int)(a.x & 0xFFFFu), (int)(a.x >> 16), (int)(a.y & 0xFFFFu), (int)(a.y >> 16) };
#pragma unroll
      for (int j = 0; j < 4; j++) px[j] = (px[j] & 0xFFFFFFu) | (decoded_q<PEAK, 510 * PEAK + PEAK>(s[j]) << 24);
    }
  }
  uint8_t *row = d.base + (size_t)k * d.image_stride + (size_t)y * d.row_stride;
  if (d.layout == 0) {
    uint8_t *dst = row + (size_t)x0 * d.inner_stride;
    const bool packed = d.inner_stride == (unsigned long long)d.channels;
    if (packed && d.channels == 4 && ((uintptr_t)dst & 3) == 0) slot_store4<4>(dst, px, n);
    else if (packed && d.channels == 3) slot_store4<3>(dst, px, n);
    else {
#pragma unroll
      for (uint32_t j = 0; j < 4; j++) if (j < n) {
        uint8_t *q = dst + (size_t)j * d.inner_stride;
        q[0] = (uint8_t)px[j]; q[1] = (uint8_t)(px[j] >> 8); q[2] = (uint8_t)(px[j] >> 16);
        if (d.channels == 4) q[3] = (uint8_t)(px[j] >> 24);
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++) if (c < d.channels) {
      uint8_t *q = row + (size_t)c * d.inner_stride + x0;
      const uint32_t v = ((px[0] >> (8 * c)) & 255u) | (((px[1] >> (8 * c)) & 255u) << 8) | (((px[2] >> (8 * c)) & 255u) << 16) | (((px[3] >> (8 * c)) & 255u) << 24);
      if (n == 4 && ((uintptr_t)q & 3) == 0) *(uint32_t *)q = v;
      else {
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) if (j < n) q[j] = (uint8_t)(v >> (8 * j));
      }
    }
  }
}

}  // namespace mi
