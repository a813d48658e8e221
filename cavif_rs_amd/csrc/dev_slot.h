// dev_slot.h -- the slot row group: what every kernel with one thread per four adjacent pixels of a slot row shares.  A batch's input slot holds w*h*channels
// samples per image (uint8_t, or uint16_t for the deep slots of DESIGN.md 5g), rows packed, images back to back.  One thread = four adjacent pixels of a row, the
// 64 lanes of a wavefront = 256 adjacent pixels: a wavefront reads or writes one contiguous run of a slot row (1 KiB of an RGBA row, 2 KiB of a deep one); grid
// (ceil(ceil(w / 4) / 64), h, images), what grid_by_four (host_input.h) builds.  Here: which pixels a thread has, their address, and their loads and stores, each
// in the widest form its own address allows, decided per thread, with narrow accesses for the pixels of a last partial group.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mi {

struct RowGroup4 { uint32_t x0, y, img, n; };                   // pixels x0 .. x0 + n - 1 (n = 1..4) of row y of image img

// the group of this thread in row y of an extent of w x h pixels; false = the thread is outside it (g is not to be used then)
__device__ __forceinline__ bool row_group4(const uint32_t w, const uint32_t h, const uint32_t y, RowGroup4 &g) {
  g.x0 = (blockIdx.x * 64 + threadIdx.x) * 4; g.y = y; g.img = blockIdx.z;
  g.n = w - g.x0 < 4 ? w - g.x0 : 4;
  return g.x0 < w && y < h;
}
// a grid row per picture row
__device__ __forceinline__ bool row_group4(const uint32_t w, const uint32_t h, RowGroup4 &g) { return row_group4(w, h, blockIdx.y, g); }

// the first sample of the group in rows of `pitch` pixels of C samples, image g.img starting image_at pixels after base
template <int C, class T> __device__ __forceinline__ T *group_ptr(T *base, const size_t image_at, const size_t pitch, const RowGroup4 &g) {
  return base + (image_at + (size_t)g.y * pitch + g.x0) * C;
}
template <int DC, class T> __device__ __forceinline__ T *slot_ptr(T *slots, const uint32_t w, const uint32_t h, const RowGroup4 &g) {
  return group_ptr<DC>(slots, (size_t)g.img * h * w, w, g);
}

// four 8-bit pixels at p can go as one 16-byte access (C 4) / three dwords (C 3).  An RGBA slot row is always 4-byte aligned (the slot is, and a pixel is four bytes).
template <int C> __device__ __forceinline__ bool slot_aligned4(const void *p) { return ((uintptr_t)p & (C == 4 ? 15 : 3)) == 0; }

// px[k] = r | g << 8 | b << 16 | a << 24 of pixel k; n = pixels that exist (1..4); DC = channels of the slot.  Where dst is not aligned for the wide form, 4-byte
// (RGBA) / 1-byte (RGB) stores.
template <int DC> __device__ __forceinline__ void slot_store4(uint8_t *dst, const uint32_t px[4], const uint32_t n) {
  const bool vec = slot_aligned4<DC>(dst);
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

// its inverse: C = 4 needs p 4-byte aligned, as the store does; a pixel of three channels comes with a = 0, and px[k] = 0 for k >= n
template <int C> __device__ __forceinline__ void slot_load4(const uint8_t *p, uint32_t px[4], const uint32_t n) {
  px[0] = px[1] = px[2] = px[3] = 0;
  const bool vec = n == 4 && slot_aligned4<C>(p);
  if (vec && C == 4) { const uint4 v = *(const uint4 *)p; px[0] = v.x; px[1] = v.y; px[2] = v.z; px[3] = v.w; }
  else if (vec) {
    const uint32_t d0 = ((const uint32_t *)p)[0], d1 = ((const uint32_t *)p)[1], d2 = ((const uint32_t *)p)[2];
    px[0] = d0 & 0xFFFFFFu; px[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8); px[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16); px[3] = d2 >> 8;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) if (k < n) {
      if (C == 4) px[k] = ((const uint32_t *)p)[k];
      else px[k] = (uint32_t)p[3 * k] | ((uint32_t)p[3 * k + 1] << 8) | ((uint32_t)p[3 * k + 2] << 16);
    }
  }
}

// four adjacent 8-bit samples of a plane, sample k in byte k (0 for k >= n): one dword where the address allows it
__device__ __forceinline__ uint32_t plane_load4(const uint8_t *q, const uint32_t n) {
  if (n == 4 && ((uintptr_t)q & 3) == 0) return *(const uint32_t *)q;
  uint32_t v = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) if (k < n) v |= (uint32_t)q[k] << (8 * k);
  return v;
}

// ---------------------------------------------------------------- 16-bit samples
// px[k] = { r | g << 16, b | a << 16 } of pixel k; n = pixels that exist (1..4); DC = channels of the slot.  The widest access the address allows, decided per
// thread: a deep RGBA pixel is 8 bytes (a row is always 8-byte aligned), a deep RGB pixel 6 (a row is 2-byte aligned, 4-byte aligned when it starts at an even pixel).
template <int DC> __device__ __forceinline__ void slot16_store4(uint16_t *dst, const uint2 px[4], const uint32_t n) {
  const uintptr_t a = (uintptr_t)dst;
  if (DC == 4) {
    if (n == 4 && (a & 15) == 0) {
      uint4 v0, v1;
      v0.x = px[0].x; v0.y = px[0].y; v0.z = px[1].x; v0.w = px[1].y; v1.x = px[2].x; v1.y = px[2].y; v1.z = px[3].x; v1.w = px[3].y;
      ((uint4 *)dst)[0] = v0; ((uint4 *)dst)[1] = v1;
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) if (k < n) ((uint2 *)dst)[k] = px[k];
    }
  } else {
    // the 24 bytes of four RGB pixels as six dwords: r0 g0 | b0 r1 | g1 b1 | r2 g2 | b2 r3 | g3 b3
    if (n == 4 && (a & 3) == 0) {
      uint32_t d[6];
      d[0] = px[0].x; d[1] = (px[0].y & 0xFFFFu) | (px[1].x << 16); d[2] = (px[1].x >> 16) | (px[1].y << 16);
      d[3] = px[2].x; d[4] = (px[2].y & 0xFFFFu) | (px[3].x << 16); d[5] = (px[3].x >> 16) | (px[3].y << 16);
      if ((a & 7) == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) { uint2 v; v.x = d[2 * k]; v.y = d[2 * k + 1]; ((uint2 *)dst)[k] = v; }
      } else {
#pragma unroll
        for (int k = 0; k < 6; k++) ((uint32_t *)dst)[k] = d[k];
      }
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) if (k < n) { dst[3 * k] = (uint16_t)px[k].x; dst[3 * k + 1] = (uint16_t)(px[k].x >> 16); dst[3 * k + 2] = (uint16_t)px[k].y; }
    }
  }
}

// NDW dwords of contiguous, 2-byte aligned samples: 16- or 8-byte loads where the address allows them, dwords at 4-byte alignment, halfwords otherwise
template <int NDW> __device__ __forceinline__ void deep_load_run(const uint8_t *p, uint32_t d[NDW]) {
  const uintptr_t a = (uintptr_t)p;
  if (NDW == 8 && (a & 15) == 0) {
    const uint4 v0 = ((const uint4 *)p)[0], v1 = ((const uint4 *)p)[1];
    d[0] = v0.x; d[1] = v0.y; d[2] = v0.z; d[3] = v0.w; d[4] = v1.x; d[5] = v1.y; d[6] = v1.z; d[7] = v1.w;
  } else if ((a & 7) == 0) {
#pragma unroll
    for (int k = 0; k < NDW / 2; k++) { const uint2 v = ((const uint2 *)p)[k]; d[2 * k] = v.x; d[2 * k + 1] = v.y; }
  } else if ((a & 3) == 0) {
#pragma unroll
    for (int k = 0; k < NDW; k++) d[k] = ((const uint32_t *)p)[k];
  } else {
#pragma unroll
    for (int k = 0; k < NDW; k++) d[k] = (uint32_t)((const uint16_t *)p)[2 * k] | ((uint32_t)((const uint16_t *)p)[2 * k + 1] << 16);
  }
}
__device__ __forceinline__ uint32_t deep_half(const uint32_t *d, const int j) { return (d[j >> 1] >> (16 * (j & 1))) & 0xFFFFu; }

// the inverse of slot16_store4 for any 2-byte aligned p: a pixel of three channels comes with a = 0, and px[k] = { 0, 0 } for k >= n
template <int C> __device__ __forceinline__ void slot16_load4(const uint16_t *p, uint2 px[4], const uint32_t n) {
#pragma unroll
  for (int k = 0; k < 4; k++) { px[k].x = 0; px[k].y = 0; }
  if (n == 4) {
    uint32_t d[2 * C];
    deep_load_run<2 * C>((const uint8_t *)p, d);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      px[k].x = deep_half(d, C * k) | (deep_half(d, C * k + 1) << 16);
      px[k].y = deep_half(d, C * k + 2) | (C == 4 ? deep_half(d, C * k + 3) << 16 : 0u);
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) if (k < n) {
      px[k].x = (uint32_t)p[C * k] | ((uint32_t)p[C * k + 1] << 16);
      px[k].y = (uint32_t)p[C * k + 2] | (C == 4 ? (uint32_t)p[C * k + 3] << 16 : 0u);
    }
  }
}

}  // namespace mi
