// dev_ingest.h -- pictures that already live in HBM -> the packed layout of a batch's input slot (w*h*channels bytes, rows packed, images back to back).
//   slot_store4     four adjacent pixels of a slot row: one 16-byte store (RGBA slot) or three dword stores (RGB slot) where the address allows it,
//                   4-byte (RGBA) / 1-byte (RGB) stores otherwise and for the pixels of a last partial group.  dev_jpeg.h's colour kernels end in it too.
//   ingest_kernel   uint8 HWC or CHW pictures with arbitrary byte strides (torch views: crops, permuted tensors, padded rows) -> slot.  One thread =
//                   four adjacent pixels of a row, the 64 lanes of a wavefront = 256 adjacent pixels: a wavefront reads one contiguous run of an
//                   interleaved row (1 KiB for packed RGBA) or one 256-byte run per plane.  No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mi {

// px[k] = r | g << 8 | b << 16 | a << 24 of pixel k; n = pixels that exist (1..4); DC = channels of the slot.  vec: dst is 16-byte (DC 4) / 4-byte (DC 3)
// aligned.  An RGBA slot row is always 4-byte aligned (the slot is, and a pixel is four bytes).
template <int DC> __device__ __forceinline__ void slot_store4(uint8_t *dst, const uint32_t px[4], const uint32_t n, const bool vec) {
  if (DC == 4) {
    if (vec && n == 4) { uint4 v; v.x = px[0]; v.y = px[1]; v.z = px[2]; v.w = px[3]; *(uint4 *)dst = v; }
    else for (uint32_t k = 0; k < 4 && k < n; k++) ((uint32_t *)dst)[k] = px[k];
  } else {
    if (vec && n == 4) {
      const uint32_t c0 = px[0] & 0xFFFFFFu, c1 = px[1] & 0xFFFFFFu, c2 = px[2] & 0xFFFFFFu, c3 = px[3] & 0xFFFFFFu;
      ((uint32_t *)dst)[0] = c0 | (c1 << 24); ((uint32_t *)dst)[1] = (c1 >> 8) | (c2 << 16); ((uint32_t *)dst)[2] = (c2 >> 16) | (c3 << 8);
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) if (k < n) { dst[3 * k] = (uint8_t)px[k]; dst[3 * k + 1] = (uint8_t)(px[k] >> 8); dst[3 * k + 2] = (uint8_t)(px[k] >> 16); }
    }
  }
}

struct IngestSrc {
  const uint8_t *base;
  unsigned long long image_stride, row_stride, inner_stride;    // bytes; inner: from pixel to pixel (HWC) or from plane to plane (CHW)
  uint32_t w, h;
  int layout, channels;                                         // 0 = HWC, 1 = CHW; 3 | 4 (3 into an RGBA slot: alpha 255)
};

// grid: (ceil(ceil(w / 4) / 64), h, images); dst = slot of the first image.  Wide loads where the source is packed and aligned for them (16 bytes for RGBA
// pixels, three dwords for RGB pixels, one dword per plane), byte loads otherwise and for a last partial group: decided per thread from its own addresses.
template <int DC> __global__ void __launch_bounds__(64) ingest_kernel(const IngestSrc s, uint8_t *slots) {
  const uint32_t x0 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y, img = blockIdx.z;
  if (x0 >= s.w || y >= s.h) return;
  const uint32_t n = s.w - x0 < 4 ? s.w - x0 : 4;
  const uint8_t *row = s.base + (size_t)img * s.image_stride + (size_t)y * s.row_stride;
  const uint32_t opaque = s.channels == 4 ? 0u : 0xFF000000u;
  uint32_t px[4] = { 0, 0, 0, 0 };
  if (s.layout == 0) {
    const uint8_t *p = row + (size_t)x0 * s.inner_stride;
    const bool packed = n == 4 && s.inner_stride == (unsigned long long)s.channels;
    if (packed && s.channels == 4 && ((uintptr_t)p & 15) == 0) {
      const uint4 v = *(const uint4 *)p;
      px[0] = v.x; px[1] = v.y; px[2] = v.z; px[3] = v.w;
    } else if (packed && s.channels == 3 && ((uintptr_t)p & 3) == 0) {
      const uint32_t d0 = ((const uint32_t *)p)[0], d1 = ((const uint32_t *)p)[1], d2 = ((const uint32_t *)p)[2];
      px[0] = (d0 & 0xFFFFFFu) | opaque; px[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8) | opaque;
      px[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16) | opaque; px[3] = (d2 >> 8) | opaque;
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) if (k < n) {
        const uint8_t *q = p + (size_t)k * s.inner_stride;
        px[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | (s.channels == 4 ? (uint32_t)q[3] << 24 : opaque);
      }
    }
  } else {
    uint32_t v[4] = { 0, 0, 0, 0xFFFFFFFFu };                   // four samples of each plane, sample k in byte k
#pragma unroll
    for (int c = 0; c < 4; c++) if (c < s.channels) {
      const uint8_t *q = row + (size_t)c * s.inner_stride + x0;
      if (n == 4 && ((uintptr_t)q & 3) == 0) v[c] = *(const uint32_t *)q;
      else {
        uint32_t a = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) if (k < n) a |= (uint32_t)q[k] << (8 * k);
        v[c] = a;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) px[k] = ((v[0] >> (8 * k)) & 255u) | (((v[1] >> (8 * k)) & 255u) << 8) | (((v[2] >> (8 * k)) & 255u) << 16) | ((v[3] >> (8 * k)) << 24);
  }
  uint8_t *dst = slots + ((size_t)img * s.h * s.w + (size_t)y * s.w + x0) * DC;
  slot_store4<DC>(dst, px, n, ((uintptr_t)dst & (DC == 4 ? 15 : 3)) == 0);
}

}  // namespace mi
