// dev_deep.h -- 16-bit sources: the deep input slot of a batch (w*h*channels uint16 samples per image, rows packed, images back to back, full
// scale 0..65535, (R, G, B[, A])), the kernels that fill it and the front end that reads it.  A slot of input kind MI_INPUT_RGB16 lives here, not in the 8-bit slot.
// The two kernels that fill it work in the row groups of dev_slot.h, which has the deep slot's loads and stores (slot16_load4, slot16_store4).
//   ingest16_kernel        uint16 HWC or CHW pictures with arbitrary even byte strides -> deep slot (a wavefront reads one contiguous run of 2 KiB of a packed
//                          RGBA row, 512 bytes per plane).  A sample is reduced to its `bits` (masked, or shifted down when msb-aligned) and widened by bit replication.
//   png_expand16_kernel    the unfiltered scanlines of a PNG of bit depth 16 (colour types 0, 2, 4, 6, Adam7) -> deep slot: both bytes of every sample, grey
//                          replicated, the tRNS colour key compared on all 16 bits (A = 0, else 65535).  png_pass_row (dev_png.h) finds the sample.
//   frontend_deep_kernel   deep slot -> the planes of a colour frame (+ alpha plane), frontend_kernel's launch shape and edge replication.  The planes are
//                          specified exactly, in integers (include/mi_avif.h): BT.601 with Kr = 0.299, Kb = 0.114 rounded half up, or G, B, R.  Dividends
//                          stay below 2^38 and every divisor is a compile-time constant: the divisions are multiply-high sequences.  A lane reads its pixel
//                          with one 8-byte load (RGBA) or three halfword loads (RGB): a wavefront reads one contiguous run of 512 / 384 bytes of a slot row.
//                          The same kernel reads a slot of kind MI_INPUT_YCBCR16: a scale per sample in place of the matrix.
// No LDS, no scratch in any of them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_slot.h"
#include "dev_ingest.h"                   // IngestSrc
#include "dev_png.h"                      // PngImageDev, png_pass_row

namespace mi {

struct Ingest16Src : IngestSrc {                                // strides all even; 3 channels into an RGBA slot: alpha 65535
  int bits, msb_aligned;                                        // 8..16 significant bits, in the low bits of a sample or (msb_aligned) in its high bits
};

// a sample reduced to its `bits` and widened to 16 by bit replication: (v << (16 - bits)) | (v >> (2 bits - 16)); 16 bits pass unchanged, 8 bits give 257 v
__device__ __forceinline__ uint32_t deep_widen(uint32_t v, const int bits, const int msb_aligned) {
  v = msb_aligned ? v >> (16 - bits) : v & ((1u << bits) - 1u);
  return ((v << (16 - bits)) | (v >> (2 * bits - 16))) & 0xFFFFu;
}

// slots = deep slot of the first image
template <int DC> __global__ void __launch_bounds__(64) ingest16_kernel(const Ingest16Src s, uint16_t *slots) {
  RowGroup4 g;
  if (!row_group4(s.w, s.h, g)) return;
  const uint32_t x0 = g.x0, n = g.n;
  const uint8_t *row = s.base + (size_t)g.img * s.image_stride + (size_t)g.y * s.row_stride;
  uint2 px[4];                                                  // the samples as the source holds them
  if (s.layout == 0) {
    const uint8_t *p = row + (size_t)x0 * s.inner_stride;
    if (s.channels == 4 && s.inner_stride == 8) slot16_load4<4>((const uint16_t *)p, px, n);
    else if (s.channels == 3 && s.inner_stride == 6) slot16_load4<3>((const uint16_t *)p, px, n);
    else {
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) {
        px[k].x = 0; px[k].y = 0;
        if (k >= n) continue;
        const uint16_t *q = (const uint16_t *)(p + (size_t)k * s.inner_stride);
        px[k].x = (uint32_t)q[0] | ((uint32_t)q[1] << 16); px[k].y = (uint32_t)q[2] | (s.channels == 4 ? (uint32_t)q[3] << 16 : 0u);
      }
    }
  } else {
    uint32_t d[4][2] = { { 0, 0 }, { 0, 0 }, { 0, 0 }, { 0, 0 } };   // four samples of each plane
#pragma unroll
    for (int ch = 0; ch < 4; ch++) if (ch < s.channels) {
      const uint8_t *q = row + (size_t)ch * s.inner_stride + (size_t)x0 * 2;
      if (n == 4) deep_load_run<2>(q, d[ch]);
      else {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) if (k < n) d[ch][k >> 1] |= (uint32_t)((const uint16_t *)q)[k] << (16 * (k & 1));
      }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) { px[k].x = deep_half(d[0], k) | (deep_half(d[1], k) << 16); px[k].y = deep_half(d[2], k) | (deep_half(d[3], k) << 16); }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t r = deep_widen(px[k].x & 0xFFFFu, s.bits, s.msb_aligned), gg = deep_widen(px[k].x >> 16, s.bits, s.msb_aligned), b = deep_widen(px[k].y & 0xFFFFu, s.bits, s.msb_aligned);
    const uint32_t a = s.channels == 4 ? deep_widen(px[k].y >> 16, s.bits, s.msb_aligned) : 0xFFFFu;
    px[k].x = r | (gg << 16); px[k].y = b | (a << 16);
  }
  slot16_store4<DC>(slot_ptr<DC>(slots, s.w, s.h, g), px, n);
}

// pixel (x, y) of a picture of bit depth 16 as { r | g << 16, b | a << 16 }: both bytes of every sample (big-endian in the file)
__device__ __forceinline__ uint2 png_pixel16(const uint8_t *buf, const PngImageDev &im, const uint32_t x, const uint32_t y) {
  uint32_t xx;
  const uint8_t *row = png_pass_row(buf, im, x, y, xx);
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

// slots = deep slot of the first image; every image of the call has bit depth 16 and is not palette-coded
template <int DC> __global__ void __launch_bounds__(64) png_expand16_kernel(const uint8_t *buf, const PngImageDev *imgs, const uint32_t w, const uint32_t h, uint16_t *slots) {
  RowGroup4 g;
  if (!row_group4(w, h, g)) return;
  const PngImageDev &im = imgs[g.img];
  uint2 px[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) { px[k].x = 0; px[k].y = 0; if (k < g.n) px[k] = png_pixel16(buf, im, g.x0 + k, g.y); }
  slot16_store4<DC>(slot_ptr<DC>(slots, w, h, g), px, g.n);
}

// ---------------------------------------------------------------- K0 for deep slots
// M = 65535, peak = 2^bd - 1, half = 2^(bd-1), floor division (every dividend below is offset to stay positive):
//   YCbCr:  S = 299 R + 587 G + 114 B,  Y = floor((2 peak S + 1000 M) / (2000 M)),
//           Cb = clamp(half + floor((2 peak (1000 B - S) + 1772 M) / (3544 M)), 0, peak),  Cr = clamp(half + floor((2 peak (1000 R - S) + 1402 M) / (2804 M)), 0, peak)
//   RGB (planes G, B, R) and alpha:  p = floor((2 peak v + M) / (2 M))
// half is folded into the chroma dividends (half * 3544 M, half * 2804 M): they run from 2 * 1772 M (2 * 1402 M) to 2^(bd+1) * 1772 M < 2^38, so the quotient
// lies in [1, 2^bd] and only the upper clamp can act.
// A slot of kind MI_INPUT_YCBCR16 (fp.ycc; filled by planes_ingest16_kernel, dev_planes.h) holds canonical (Y, Cb, Cr[, 65535]): no matrix,
//   p0 = deep_scale(Y),  p_k = clamp(half + floor((2 peak (C_k - 32768) + M) / (2 M)), 0, peak)
// with half and the centre folded into the dividend (half * 2 M - 65536 peak + M = 130815 at depth 8, 130047 at depth 10: positive, so only the upper clamp can
// act).  Such an image is opaque: its fourth sample is not looked at, its alpha plane is peak and the flag stays 0.
struct FrontDeepParams { int depth, color_model, ycc; };
__device__ __forceinline__ uint32_t deep_scale(const uint32_t v, const uint32_t peak) { return (2u * peak * v + 65535u) / (2u * 65535u); }
__device__ __forceinline__ uint32_t deep_scale_chroma(const uint32_t c, const uint32_t peak, const uint32_t half) {
  const uint32_t q = (2u * peak * c + (half * (2u * 65535u) - 65536u * peak + 65535u)) / (2u * 65535u);
  return q < peak ? q : peak;
}
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
  if (fp.ycc) { o0 = deep_scale(R, peak); o1 = deep_scale_chroma(G, peak, half); o2 = deep_scale_chroma(B, peak, half); A = 65535u; }
  else if (fp.color_model == 1) { o0 = deep_scale(G, peak); o1 = deep_scale(B, peak); o2 = deep_scale(R, peak); }
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
