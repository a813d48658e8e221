// dev_resample16.h -- deep resize: a 16-bit picture of any size in HBM -> a batch's deep input slot, the 16-bit forms of the three kernels of
// dev_resample.h.  Same grids, same table layout (bounds + tap-major taps from resample_axis), same tile roles and access patterns; what differs:
//   samples        a pixel is the uint2 of dev_slot.h, r | g << 16, b | a << 16, in LDS, in the intermediate (8 bytes a pixel, rows `pitch` = dst_w rounded up to 4
//                  pixels apart: the vertical pass loads two aligned 16-byte words per tap and thread) and on its way into slot16_store4.
//   taps           28 fractional bits (MI_RS16_BITS).  A pass is out = clamp((2^27 + sum k_j s_j) >> 28, 0, 65535) over a signed 64-bit sum that does not wrap
//                  (|sum| < 2^46: the order of summation is free); the multiply-add is plain C++, (int64_t)k * (int32_t)s, one 32 x 32 + 64 instruction.
//   sources        Ingest16Src: a sample is reduced to its `bits` and widened by bit replication (deep_widen, what ingest16_kernel stores) before anything else;
//                  4-channel sources are then premultiplied: t = c a + 32768, p = (t + (t >> 16)) >> 16 = floor((2 c a + 65535) / 131070), all inside 32 bits.
//   resample_h16_kernel   stages MI_RS16_CHUNK source pixels of each of its four rows in LDS (4 x 512 x 8 B = 16 KiB), a thread four adjacent pixels at a time: a
//                         packed HWC source of 3 or 4 channels through slot16_load4 (the widest loads the address allows), any other strides sample by sample.
//                         Orientations 2..4 are addressing, as in resample_h_kernel: the group is taken from the mirrored columns and written back to front.
//   resample_t16_kernel   the first pass of a source turned by orientation 5..8; 16 int64 accumulators per thread, then the 64 x 64 turning tile.
//   resample_v16_kernel   intermediate -> deep slot in the row groups of dev_slot.h, 16 int64 accumulators per thread, un-premultiplies (for a not 0 and not
//                         65535: c = min(65535, 65535 c / a), integer division), stores through slot16_store4.  No LDS.
//
// resample_t16_kernel's LDS layout: TWO dword planes of the 8-bit kernel's tile, plane 0 = the low words (r | g << 16), plane 1 = the high words (b | a << 16), each
// 64 rows of MI_RS_TP = 65 dwords: 2 x 16640 = 33280 bytes.  Every access is a ds_read_b32 / ds_write_b32 into one plane, so dev_resample.h's argument holds for
// each plane word for word: banks are (dword address) mod 32 and a wave64 access is served in its two halves of 32 lanes.
//   write (row-wise): a half wave writes 32 adjacent dwords of one row of a plane -- 32 banks, no conflict, whatever the pitch.
//   read (transposed): lane l of a half wave reads dword l * 65 + column of a plane: banks (l + column) mod 32 for 32 consecutive l -- 32 lanes, 32 banks, no conflict.
//   the second plane starts 64 * 65 = 4160 dwords after the first, a multiple of 32: both planes map to the banks alike, and the two accesses of a pixel are two
//   instructions, never one access that could meet itself.  (An 8-byte element read with ds_read_b64 at a pitch of 65 elements would put lane l on dword banks
//   2 (l + column) and 2 (l + column) + 1: that needs its own argument about how the hardware splits a 64-lane b64 access; the planes avoid the question.)
// No scratch in any of the three (profiles/deep_resize.md has the compiler's report).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_slot.h"
#include "dev_deep.h"                     // Ingest16Src, deep_widen
#include "dev_resample.h"                 // the tile sizes the grids share: MI_RS_TW, MI_RS_TH, MI_RS_TT, MI_RS_TP

namespace mi {

#define MI_RS16_BITS 28                   /* fractional bits of a tap: the largest |tap| is about 1.25, the sum of products stays below 2^46 */
#define MI_RS16_CHUNK 512                 /* source pixels of a row staged at once: 4 x 512 x 8 bytes = 16 KiB of LDS */

__device__ __forceinline__ uint32_t rs16_clip(const int64_t acc) {
  const int64_t v = acc >> MI_RS16_BITS;                                           // arithmetic shift
  return (uint32_t)(v < 0 ? 0 : v > 65535 ? 65535 : v);
}
// c * a / 65535 rounded: floor((2 c a + 65535) / 131070); t <= 65535^2 + 32768 and t + (t >> 16) stay below 2^32
__device__ __forceinline__ uint32_t rs16_premul(const uint32_t c, const uint32_t a) { const uint32_t t = c * a + 32768u; return (t + (t >> 16)) >> 16; }
__device__ __forceinline__ void rs16_mac(int64_t acc[4], const uint2 v, const int32_t k, const bool alpha) {
  acc[0] += (int64_t)k * (int32_t)(v.x & 0xFFFFu); acc[1] += (int64_t)k * (int32_t)(v.x >> 16); acc[2] += (int64_t)k * (int32_t)(v.y & 0xFFFFu);
  if (alpha) acc[3] += (int64_t)k * (int32_t)(v.y >> 16);
}
__device__ __forceinline__ uint2 rs16_clip_px(const int64_t acc[4], const bool alpha) {
  uint2 o;
  o.x = rs16_clip(acc[0]) | (rs16_clip(acc[1]) << 16); o.y = rs16_clip(acc[2]) | ((alpha ? rs16_clip(acc[3]) : 0xFFFFu) << 16);
  return o;
}

// the samples of a pixel as the source holds them -> reduced to `bits`, widened, 3 channels: alpha 65535; 4 channels: colour premultiplied
__device__ __forceinline__ uint2 rs16_prepare(const uint2 v, const bool alpha, const int bits, const int msb_aligned) {
  uint32_t r = deep_widen(v.x & 0xFFFFu, bits, msb_aligned), g = deep_widen(v.x >> 16, bits, msb_aligned), b = deep_widen(v.y & 0xFFFFu, bits, msb_aligned), a = 0xFFFFu;
  if (alpha) { a = deep_widen(v.y >> 16, bits, msb_aligned); r = rs16_premul(r, a); g = rs16_premul(g, a); b = rs16_premul(b, a); }
  uint2 o; o.x = r | (g << 16); o.y = b | (a << 16);
  return o;
}
// pixel x of a source row, sample by sample; px / ch: bytes from pixel to pixel / channel to channel (all even)
__device__ __forceinline__ uint2 rs16_raw_px(const uint8_t *row, const uint32_t x, const size_t px, const size_t ch, const int channels) {
  const uint8_t *q = row + (size_t)x * px;
  uint2 v;
  v.x = (uint32_t)*(const uint16_t *)q | ((uint32_t)*(const uint16_t *)(q + ch) << 16);
  v.y = (uint32_t)*(const uint16_t *)(q + 2 * ch) | (channels == 4 ? (uint32_t)*(const uint16_t *)(q + 3 * ch) << 16 : 0u);
  return v;
}

// grid: (ceil(dst_w / 64), ceil(s.h / 4), images); block 256.  s.w x s.h is the SOURCE extent; o = 1..4 as in resample_h_kernel.
__global__ void __launch_bounds__(64 * MI_RS_TH) resample_h16_kernel(const Ingest16Src s, const int o, const uint32_t *bounds, const int32_t *taps, const uint32_t dst_w, const uint32_t pitch, uint2 *inter) {
  __shared__ uint2 tile[MI_RS_TH * MI_RS16_CHUNK];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t ox0 = blockIdx.x * MI_RS_TW, ox = ox0 + lane, y0 = blockIdx.y * MI_RS_TH, y = y0 + wave, img = blockIdx.z;
  const bool live = ox < dst_w && y < s.h;
  const int xmin = ox < dst_w ? (int)bounds[2 * ox] : 0, cnt = live ? (int)bounds[2 * ox + 1] : 0;
  // the tile's span of the source row: first samples and ends both grow with the column
  const uint32_t last = ox0 + MI_RS_TW - 1 < dst_w ? ox0 + MI_RS_TW - 1 : dst_w - 1;
  const uint32_t lo = bounds[2 * ox0], hi = bounds[2 * last] + bounds[2 * last + 1];
  const uint32_t rows = s.h - y0 < MI_RS_TH ? s.h - y0 : MI_RS_TH;
  const size_t px = s.layout == 0 ? (size_t)s.inner_stride : 2, ch = s.layout == 0 ? 2 : (size_t)s.inner_stride;
  const bool packed = s.layout == 0 && s.inner_stride == 2ull * (unsigned)s.channels;
  const uint8_t *const image = s.base + (size_t)img * s.image_stride;
  const bool alpha = s.channels == 4, flip_r = o == 3 || o == 4, flip_c = o == 2 || o == 3;
  int64_t acc[4] = { (int64_t)1 << (MI_RS16_BITS - 1), (int64_t)1 << (MI_RS16_BITS - 1), (int64_t)1 << (MI_RS16_BITS - 1), (int64_t)1 << (MI_RS16_BITS - 1) };
  for (uint32_t c0 = lo; c0 < hi; c0 += MI_RS16_CHUNK) {                           // uniform in the workgroup
    const uint32_t len = hi - c0 < MI_RS16_CHUNK ? hi - c0 : MI_RS16_CHUNK;
    for (uint32_t r = 0; r < rows; r++) {
      const uint8_t *const row = image + (size_t)(flip_r ? s.h - 1 - (y0 + r) : y0 + r) * s.row_stride;
      for (uint32_t i = threadIdx.x * 4; i < len; i += 64 * MI_RS_TH * 4) {        // oriented columns c0 + i .. c0 + i + n - 1 <= hi - 1 < s.w
        const uint32_t n = len - i < 4 ? len - i : 4;
        const uint32_t xs = flip_c ? s.w - (c0 + i + n) : c0 + i;                  // the group's first source column: mirrored, the group lies back to front
        uint2 v[4];
        if (packed && alpha) slot16_load4<4>((const uint16_t *)(row + (size_t)xs * 8), v, n);
        else if (packed) slot16_load4<3>((const uint16_t *)(row + (size_t)xs * 6), v, n);
        else {
#pragma unroll
          for (uint32_t k = 0; k < 4; k++) { v[k].x = 0; v[k].y = 0; if (k < n) v[k] = rs16_raw_px(row, xs + k, px, ch, s.channels); }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) if (k < n) tile[r * MI_RS16_CHUNK + i + (flip_c ? n - 1 - k : k)] = rs16_prepare(v[k], alpha, s.bits, s.msb_aligned);
      }
    }
    __syncthreads();
    // this lane's taps inside the chunk: j0 <= j < j1
    const int j0 = (int)c0 > xmin ? (int)c0 - xmin : 0, j1 = xmin + cnt < (int)(c0 + len) ? cnt : (int)(c0 + len) - xmin;
    const int at = (int)(wave * MI_RS16_CHUNK) + xmin - (int)c0;                   // of tap 0 in the tile: 0 <= at + j < the row's len for j0 <= j < j1
    for (int j = j0; j < j1; j++) rs16_mac(acc, tile[at + j], taps[(size_t)j * dst_w + ox], alpha);
    __syncthreads();                                                               // before the next chunk overwrites the tile
  }
  if (live) inter[((size_t)img * s.h + y) * pitch + ox] = rs16_clip_px(acc, alpha);
}

// one pixel of a source row for the turning pass: a packed, 8-byte aligned RGBA pixel in one load, anything else sample by sample
__device__ __forceinline__ uint2 rs16_load_px(const uint8_t *row, const uint32_t x, const size_t px, const size_t ch, const int channels) {
  const uint8_t *q = row + (size_t)x * px;
  if (channels == 4 && px == 8 && ch == 2 && ((uintptr_t)q & 7) == 0) return *(const uint2 *)q;
  return rs16_raw_px(row, x, px, ch, channels);
}

// grid: (ceil(dst_w / 64), ceil(s.w / 64), images); block 256.  s.w x s.h is the SOURCE extent, o = 5..8; the tables are those of the axis s.h -> dst_w.
// Intermediate row c (7, 8: s.w - 1 - c) is source column c; its sample x sums source rows bounds[2 x] + j (6, 7: counted from the bottom).
__global__ void __launch_bounds__(256) resample_t16_kernel(const Ingest16Src s, const int o, const uint32_t *bounds, const int32_t *taps, const uint32_t dst_w, const uint32_t pitch, uint2 *inter) {
  __shared__ uint32_t tile[2][MI_RS_TT * MI_RS_TP];
  const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));     // uniform: bounds, taps and range tests stay scalar
  const uint32_t ox0 = blockIdx.x * MI_RS_TT, c0 = blockIdx.y * MI_RS_TT, img = blockIdx.z;
  const bool flip_r = o == 6 || o == 7, flip_c = o == 7 || o == 8, alpha = s.channels == 4;
  const uint32_t c = c0 + lane;
  const bool has = c < s.w;
  const size_t px = s.layout == 0 ? (size_t)s.inner_stride : 2, ch = s.layout == 0 ? 2 : (size_t)s.inner_stride;
  const uint8_t *const image = s.base + (size_t)img * s.image_stride;
  for (uint32_t g = 0; g < MI_RS_TT / 16; g++) {
    const uint32_t o0 = wave * 16 + g * 4, oxg = ox0 + o0;                         // this wavefront's four output samples: tile rows o0 .. o0 + 3
    if (oxg >= dst_w) break;
    const uint32_t n = dst_w - oxg < 4 ? dst_w - oxg : 4;
    uint32_t xmin[4], cnt[4], hi = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      xmin[q] = q < n ? bounds[2 * (oxg + q)] : 0; cnt[q] = q < n ? bounds[2 * (oxg + q) + 1] : 0;
      hi = xmin[q] + cnt[q] > hi ? xmin[q] + cnt[q] : hi;
    }
    int64_t acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int k = 0; k < 4; k++) acc[q][k] = (int64_t)1 << (MI_RS16_BITS - 1);
    for (uint32_t t = xmin[0]; t < hi; t++) {                                      // rows of the oriented x axis: 0 <= t < s.h (the tables' input extent)
      const uint8_t *const row = image + (size_t)(flip_r ? s.h - 1 - t : t) * s.row_stride;
      uint2 v; v.x = 0; v.y = 0;
      if (has) v = rs16_prepare(rs16_load_px(row, c, px, ch, s.channels), alpha, s.bits, s.msb_aligned);
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t j = t - xmin[q];                                            // wraps to a large number below the range
        if (j < cnt[q]) rs16_mac(acc[q], v, taps[(size_t)j * dst_w + oxg + q], alpha);
      }
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; q++)
      if (q < n) { const uint2 p = rs16_clip_px(acc[q], alpha); tile[0][(o0 + q) * MI_RS_TP + lane] = p.x; tile[1][(o0 + q) * MI_RS_TP + lane] = p.y; }
  }
  __syncthreads();
  const uint32_t nc = s.w - c0 < MI_RS_TT ? s.w - c0 : MI_RS_TT;                   // the tile's source columns (the grid leaves no empty tile)
  if (ox0 + lane < dst_w)
    for (uint32_t cl = wave; cl < nc; cl += 4) {
      const uint32_t oy = flip_c ? s.w - 1 - (c0 + cl) : c0 + cl;                  // < s.w, the intermediate's rows per image
      uint2 p; p.x = tile[0][lane * MI_RS_TP + cl]; p.y = tile[1][lane * MI_RS_TP + cl];
      inter[((size_t)img * s.w + oy) * pitch + ox0 + lane] = p;
    }
}

// alpha: the picture has four channels (premultiplied in the intermediate); slots = deep slot of the first image.
template <int DC> __global__ void __launch_bounds__(64) resample_v16_kernel(const uint2 *inter, const uint32_t src_h, const uint32_t pitch, const uint32_t *bounds, const int32_t *taps,
                                                                            const uint32_t dst_w, const uint32_t dst_h, const int alpha, uint16_t *slots) {
  RowGroup4 g;
  if (!row_group4(dst_w, dst_h, g)) return;
  const uint32_t x0 = g.x0, oy = g.y, img = g.img;
  const uint32_t ymin = bounds[2 * oy], cnt = bounds[2 * oy + 1];
  const uint2 *col = inter + ((size_t)img * src_h + ymin) * pitch + x0;            // 32-byte aligned: pitch and x0 are multiples of 4 pixels; the row's padding is read and not used
  const int32_t *k_ = taps + oy;
  int64_t acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int c = 0; c < 4; c++) acc[p][c] = (int64_t)1 << (MI_RS16_BITS - 1);
  for (uint32_t j = 0; j < cnt; j++, col += pitch, k_ += dst_h) {
    const uint4 q0 = ((const uint4 *)col)[0], q1 = ((const uint4 *)col)[1];
    const int32_t k = *k_;
    uint2 v[4];
    v[0].x = q0.x; v[0].y = q0.y; v[1].x = q0.z; v[1].y = q0.w; v[2].x = q1.x; v[2].y = q1.y; v[3].x = q1.z; v[3].y = q1.w;
#pragma unroll
    for (int p = 0; p < 4; p++) rs16_mac(acc[p], v[p], k, alpha != 0);
  }
  uint2 px[4];
#pragma unroll
  for (int p = 0; p < 4; p++) {
    uint32_t r = rs16_clip(acc[p][0]), gg = rs16_clip(acc[p][1]), b = rs16_clip(acc[p][2]), a = 65535u;
    if (alpha) {
      a = rs16_clip(acc[p][3]);
      if (a != 0 && a != 65535u) {                                                 // un-premultiply: integer division, clipped (65535 * 65535 < 2^32)
        r = 65535u * r / a; gg = 65535u * gg / a; b = 65535u * b / a;
        r = r > 65535u ? 65535u : r; gg = gg > 65535u ? 65535u : gg; b = b > 65535u ? 65535u : b;
      }
    }
    px[p].x = r | (gg << 16); px[p].y = b | (a << 16);
  }
  slot16_store4<DC>(slot_ptr<DC>(slots, dst_w, dst_h, g), px, g.n);
}

}  // namespace mi
