// dev_deep.h -- 16-bit sources: the deep input slot of a batch (w*h*channels uint16 samples per image, rows packed, images back to back, full
// scale 0..65535, (R, G, B[, A])), the kernels that fill it and the front end that reads it.  A slot of input kind MI_INPUT_RGB16 lives here, not in the 8-bit slot.
//   slot16_store4          four adjacent pixels of a deep slot row: two 16-byte stores (RGBA) or three 8-byte stores (RGB) where the address allows it, dwords
//                          at 4-byte alignment, halfwords otherwise and for the pixels of a last partial group.
//   ingest16_kernel        uint16 HWC or CHW pictures with arbitrary even byte strides -> deep slot, ingest_kernel's shape: one thread = four adjacent pixels
//                          of a row, a wavefront = 256 adjacent pixels (one contiguous run of 2 KiB of a packed RGBA row, 512 bytes per plane), all images of a
//                          call in grid z.  A sample is reduced to its `bits` (masked, or shifted down when msb-aligned) and widened by bit replication.
//   png_expand16_kernel    the unfiltered scanlines of a PNG of bit depth 16 (colour types 0, 2, 4, 6, Adam7) -> deep slot: both bytes of every sample, grey
//                          replicated, the tRNS colour key compared on all 16 bits (A = 0, else 65535).  png_expand_kernel's shape and pass arithmetic.
//   frontend_deep_kernel   deep slot -> the planes of a colour frame (+ alpha plane), frontend_kernel's launch shape and edge replication.  The planes are
//                          specified exactly, in integers (include/mi_avif.h): BT.601 with Kr = 0.299, Kb = 0.114 rounded half up, or G, B, R.  Dividends
//                          stay below 2^38 and every divisor is a compile-time constant: the divisions are multiply-high sequences.  A lane reads its pixel
//                          with one 8-byte load (RGBA) or three halfword loads (RGB): a wavefront reads one contiguous run of 512 / 384 bytes of a slot row.
// No LDS, no scratch in any of them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_png.h"

namespace mi {

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

struct Ingest16Src {
  const uint8_t *base;
  unsigned long long image_stride, row_stride, inner_stride;    // bytes, all even; inner: from pixel to pixel (HWC) or from plane to plane (CHW)
  uint32_t w, h;
  int layout, channels;                                         // 0 = HWC, 1 = CHW; 3 | 4 (3 into an RGBA slot: alpha 65535)
  int bits, msb_aligned;                                        // 8..16 significant bits, in the low bits of a sample or (msb_aligned) in its high bits
};

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
// a sample reduced to its `bits` and widened to 16 by bit replication: (v << (16 - bits)) | (v >> (2 bits - 16)); 16 bits pass unchanged, 8 bits give 257 v
__device__ __forceinline__ uint32_t deep_widen(uint32_t v, const int bits, const int msb_aligned) {
  v = msb_aligned ? v >> (16 - bits) : v & ((1u << bits) - 1u);
  return ((v << (16 - bits)) | (v >> (2 * bits - 16))) & 0xFFFFu;
}

// grid: (ceil(ceil(w / 4) / 64), h, images); slots = deep slot of the first image
template <int DC> __global__ void __launch_bounds__(64) ingest16_kernel(const Ingest16Src s, uint16_t *slots) {
  const uint32_t x0 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y, img = blockIdx.z;
  if (x0 >= s.w || y >= s.h) return;
  const uint32_t n = s.w - x0 < 4 ? s.w - x0 : 4;
  const uint8_t *row = s.base + (size_t)img * s.image_stride + (size_t)y * s.row_stride;
  uint32_t c[4][4];                                             // [pixel][channel]
#pragma unroll
  for (int k = 0; k < 4; k++) { c[k][0] = c[k][1] = c[k][2] = 0; c[k][3] = 0xFFFFu; }
  if (s.layout == 0) {
    const uint8_t *p = row + (size_t)x0 * s.inner_stride;
    if (n == 4 && s.channels == 4 && s.inner_stride == 8) {
      uint32_t d[8];
      deep_load_run<8>(p, d);
#pragma unroll
      for (int k = 0; k < 4; k++) { c[k][0] = deep_half(d, 4 * k); c[k][1] = deep_half(d, 4 * k + 1); c[k][2] = deep_half(d, 4 * k + 2); c[k][3] = deep_half(d, 4 * k + 3); }
    } else if (n == 4 && s.channels == 3 && s.inner_stride == 6) {
      uint32_t d[6];
      deep_load_run<6>(p, d);
#pragma unroll
      for (int k = 0; k < 4; k++) { c[k][0] = deep_half(d, 3 * k); c[k][1] = deep_half(d, 3 * k + 1); c[k][2] = deep_half(d, 3 * k + 2); }
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) if (k < n) {
        const uint16_t *q = (const uint16_t *)(p + (size_t)k * s.inner_stride);
        c[k][0] = q[0]; c[k][1] = q[1]; c[k][2] = q[2];
        if (s.channels == 4) c[k][3] = q[3];
      }
    }
  } else {
#pragma unroll
    for (int ch = 0; ch < 4; ch++) if (ch < s.channels) {
      const uint8_t *q = row + (size_t)ch * s.inner_stride + (size_t)x0 * 2;
      if (n == 4) {
        uint32_t d[2];
        deep_load_run<2>(q, d);
#pragma unroll
        for (int k = 0; k < 4; k++) c[k][ch] = deep_half(d, k);
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) if (k < n) c[k][ch] = ((const uint16_t *)q)[k];
      }
    }
  }
  uint2 px[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t r = deep_widen(c[k][0], s.bits, s.msb_aligned), g = deep_widen(c[k][1], s.bits, s.msb_aligned), b = deep_widen(c[k][2], s.bits, s.msb_aligned);
    const uint32_t a = s.channels == 4 ? deep_widen(c[k][3], s.bits, s.msb_aligned) : 0xFFFFu;
    px[k].x = r | (g << 16); px[k].y = b | (a << 16);
  }
  slot16_store4<DC>(slots + ((size_t)img * s.h * s.w + (size_t)y * s.w + x0) * DC, px, n);
}

// pixel (x, y) of a picture of bit depth 16 as { r | g << 16, b | a << 16 }: png_pixel's pass arithmetic, both bytes of every sample (big-endian in the file)
__device__ __forceinline__ uint2 png_pixel16(const uint8_t *buf, const PngImageDev &im, const uint32_t x, const uint32_t y) {
  uint32_t p = 0, xx = x, yy = y;
  if (im.interlace) {
    p = (y & 1) ? 6 : (x & 1) ? 5 : (y & 2) ? 4 : (x & 2) ? 3 : (y & 4) ? 2 : (x & 4) ? 1 : 0;
    xx = (x - ((0x0102040u >> (4 * p)) & 15u)) >> ((0x0112233u >> (4 * p)) & 15u);
    yy = (y - ((0x1020400u >> (4 * p)) & 15u)) >> ((0x1122333u >> (4 * p)) & 15u);
  }
  const uint8_t *row = buf + im.pass_off[p] + (size_t)yy * ((size_t)im.pass_rowbytes[p] + 1) + 1;
  const uint32_t ctype = im.ctype;
  const uint32_t channels = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 4 ? 2 : 4;
  const uint8_t *q = row + (size_t)xx * channels * 2;
  uint32_t s[4] = { 0, 0, 0, 0 };
#pragma unroll
  for (uint32_t c = 0; c < 4; c++) if (c < channels) s[c] = ((uint32_t)q[2 * c] << 8) | q[2 * c + 1];
  uint32_t r, g, b, a = 0xFFFFu;
  if (ctype == 0 || ctype == 4) {
    r = g = b = s[0];
    if (ctype == 4) a = s[1];
    else if (im.has_key && s[0] == im.key[0]) a = 0;
  } else {
    r = s[0]; g = s[1]; b = s[2];
    if (ctype == 6) a = s[3];
    else if (im.has_key && s[0] == im.key[0] && s[1] == im.key[1] && s[2] == im.key[2]) a = 0;
  }
  uint2 o; o.x = r | (g << 16); o.y = b | (a << 16);
  return o;
}

// grid: (ceil(ceil(w / 4) / 64), h, images); slots = deep slot of the first image; every image of the call has bit depth 16 and is not palette-coded
template <int DC> __global__ void __launch_bounds__(64) png_expand16_kernel(const uint8_t *buf, const PngImageDev *imgs, const uint32_t w, const uint32_t h, uint16_t *slots) {
  const uint32_t x0 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y, img = blockIdx.z;
  if (x0 >= w || y >= h) return;
  const PngImageDev &im = imgs[img];
  const uint32_t n = w - x0 < 4 ? w - x0 : 4;
  uint2 px[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) { px[k].x = 0; px[k].y = 0; if (k < n) px[k] = png_pixel16(buf, im, x0 + k, y); }
  slot16_store4<DC>(slots + ((size_t)img * h * w + (size_t)y * w + x0) * DC, px, n);
}

// ---------------------------------------------------------------- K0 for deep slots
// M = 65535, peak = 2^bd - 1, half = 2^(bd-1), floor division (every dividend below is offset to stay positive):
//   YCbCr:  S = 299 R + 587 G + 114 B,  Y = floor((2 peak S + 1000 M) / (2000 M)),
//           Cb = clamp(half + floor((2 peak (1000 B - S) + 1772 M) / (3544 M)), 0, peak),  Cr = clamp(half + floor((2 peak (1000 R - S) + 1402 M) / (2804 M)), 0, peak)
//   RGB (planes G, B, R) and alpha:  p = floor((2 peak v + M) / (2 M))
// half is folded into the chroma dividends (half * 3544 M, half * 2804 M): they run from 2 * 1772 M (2 * 1402 M) to 2^(bd+1) * 1772 M < 2^38, so the quotient
// lies in [1, 2^bd] and only the upper clamp can act.
struct FrontDeepParams { int depth, color_model; };
__device__ __forceinline__ uint32_t deep_scale(const uint32_t v, const uint32_t peak) { return (2u * peak * v + 65535u) / (2u * 65535u); }
template <int DC> __global__ __launch_bounds__(256) void frontend_deep_kernel(const uint16_t *pix, int w, int h, FrontDeepParams fp,
                                                                              uint16_t *p0, uint16_t *p1, uint16_t *p2, uint16_t *pa, int pw, int ph, int *alpha_flag) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= pw || y >= ph) return;
  const int sx = x < w - 1 ? x : w - 1, sy = y < h - 1 ? y : h - 1;
  const uint16_t *p = pix + ((size_t)sy * w + sx) * DC;
  uint32_t R, G, B, A = 65535u;
  if (DC == 4) { const uint2 v = *(const uint2 *)p; R = v.x & 0xFFFFu; G = v.x >> 16; B = v.y & 0xFFFFu; A = v.y >> 16; }
  else { R = p[0]; G = p[1]; B = p[2]; }
  const uint32_t peak = (1u << fp.depth) - 1u, half = 1u << (fp.depth - 1);
  uint32_t o0, o1, o2;
  if (fp.color_model == 1) { o0 = deep_scale(G, peak); o1 = deep_scale(B, peak); o2 = deep_scale(R, peak); }
  else {
    constexpr long long M = 65535;
    const long long S = 299ll * R + 587ll * G + 114ll * B, k = 2ll * peak;
    o0 = (uint32_t)((unsigned long long)(k * S + 1000 * M) / (unsigned long long)(2000 * M));
    const uint32_t cb = (uint32_t)((unsigned long long)(k * (1000ll * B - S) + 1772 * M + (long long)half * (3544 * M)) / (unsigned long long)(3544 * M));
    const uint32_t cr = (uint32_t)((unsigned long long)(k * (1000ll * R - S) + 1402 * M + (long long)half * (2804 * M)) / (unsigned long long)(2804 * M));
    o1 = cb < peak ? cb : peak; o2 = cr < peak ? cr : peak;
  }
  const size_t o = (size_t)y * pw + x;
  p0[o] = (uint16_t)o0; p1[o] = (uint16_t)o1; p2[o] = (uint16_t)o2;
  if (pa) pa[o] = (uint16_t)deep_scale(A, peak);
  if (A != 65535u && x < w && y < h && alpha_flag) *alpha_flag = 1;
}

}  // namespace mi
