// dev_resample.h -- resize on input: a picture of any size in HBM -> a batch's input slot, resampled with an integer filter whose pixels are specified
// exactly (Pillow's 8-bit Image.resize).  Two separable passes, horizontal first, one launch per pass for all images of a call.
//   resample_h_kernel   source (IngestSrc addressing: HWC or CHW, any byte strides) -> intermediate of dst_w x src_h pixels, a pixel one dword
//                       r | g << 8 | b << 16 | a << 24, rows `pitch` pixels apart (pitch = dst_w rounded up to 4: the vertical pass loads 16 bytes).
//                       4-channel sources are premultiplied on load.  One workgroup = 64 output columns x 4 rows (a wavefront per row, a lane per
//                       column: a wavefront stores one contiguous 256-byte run of an intermediate row).  The source span of the tile is staged in LDS
//                       MI_RS_CHUNK pixels at a time with the threads running along the row, and every lane adds the taps that fall into the chunk:
//                       the tap count has no bound (257 -> 2 Lanczos: 773), the LDS tile has.  Sums are 32-bit and wrap, so their order is free.
//                       Orientations 2..4 are addressing in the staging loop: the column index and / or the row are counted from the far end.
//   resample_t_kernel   the first pass of a source that is turned by orientation 5..8: the oriented picture's x axis is the source's y axis, so
//                       the pass filters down the source's columns and writes the intermediate the other kernels know -- dst_w wide, a row per source column.
//   resample_v_kernel   intermediate -> slot, in the row groups of dev_slot.h (16 accumulators per thread): each tap is one contiguous 1 KiB run of an
//                       intermediate row; bounds and taps are uniform in a workgroup (scalar loads).  Un-premultiplies 4-channel pictures.  No LDS.
// Tables come from the host (mi_avif.hip: resample_axis), per axis: bounds[2 i] = first sample, bounds[2 i + 1] = taps of output sample i, and the taps in
// 22-bit fixed point, tap-major (tap j of output i at taps[j * n_out + i]: adjacent lanes read adjacent words).  An axis that keeps its length gets the
// one-tap identity table (2^22: 2^21 + s * 2^22 >> 22 = s), so its pass moves the samples unchanged.
//
// resample_t_kernel.  A workgroup of four wavefronts owns a tile of MI_RS_TT source columns x MI_RS_TT output samples along the oriented x axis: grid
// (ceil(dst_w / 64), ceil(s.w / 64), images).  Lanes run along the source's x, so a tap is one contiguous run of a source row (resample_v_kernel's access
// pattern; never a lane per row).  A wavefront takes 16 of the tile's output samples, four at a time: it walks the union of their tap ranges once (first
// samples and ends both grow with the output sample), loads a pixel per lane and row, and adds it to those of the four sums whose range holds the row --
// 16 accumulators per thread; bounds, taps and the range tests are wave-uniform (scalar).  The clipped pixels go into LDS as tile[output][column], a barrier,
// and come out transposed: a wavefront reads tile[lane][column] and stores 64 adjacent pixels of the intermediate row of that column, the 256-byte runs
// resample_h_kernel writes.  The flips of 6, 7 and 8 are index reversals on either side of the tile: the source row of a tap is counted from the bottom
// (6, 7), the intermediate row of a column from the far end (7, 8).
// LDS layout: rows of MI_RS_TP = 65 dwords (one dword of padding), 16640 bytes.  Banks of ds_read_b32 / ds_write_b32 are (dword address) mod 32 and a wave64
// access is served in its two halves of 32 lanes (MI355X: 64 banks of 4 bytes; 4-byte accesses see them mod 32).
//   write (row-wise): a half wave writes 32 adjacent dwords of one row -- 32 banks, no conflict, whatever the pitch.
//   read (transposed): lane l of a half wave reads dword l * P + column.  With the plain pitch P = 64 all 32 lanes meet on bank (column mod 32): 32-way.  With
//     P = 65 the banks are (l + column) mod 32 for 32 consecutive l: 32 lanes, 32 banks, no conflict (one pixel a lane, row = lane: any odd pitch would do).
// No scratch (profiles/resize_orient.md has the compiler's report).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_slot.h"
#include "dev_ingest.h"                   // IngestSrc

namespace mi {

#define MI_RS_BITS 22                     /* fractional bits of a tap */
#define MI_RS_TW 64                       /* output columns of a horizontal tile = lanes */
#define MI_RS_TH 4                        /* rows of a horizontal tile = wavefronts */
#define MI_RS_CHUNK 512                   /* source pixels of a row staged at once: 4 x 512 dwords = 8 KiB of LDS */
#define MI_RS_TT 64                       /* side of a turning tile: source columns = lanes, output samples = lanes of the transposed store */
#define MI_RS_TP 65                       /* dwords from row to row of the turning tile in LDS (see above) */

__device__ __forceinline__ uint32_t rs_clip8(const uint32_t acc) {
  const int v = (int)acc >> MI_RS_BITS;                                            // arithmetic shift of the wrapped sum
  return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}
// c * a / 255 rounded, as Pillow's MULDIV255
__device__ __forceinline__ uint32_t rs_premul(const uint32_t c, const uint32_t a) { const uint32_t t = c * a + 128; return ((t >> 8) + t) >> 8; }

// pixel x of a source row as r | g << 8 | b << 16 | a << 24 (3 channels: alpha 255; 4 channels: colour premultiplied); px / ch: bytes from pixel to pixel / channel to channel
__device__ __forceinline__ uint32_t rs_load_px(const uint8_t *row, const uint32_t x, const size_t px, const size_t ch, const int channels) {
  const uint8_t *q = row + (size_t)x * px;
  const uint32_t r = q[0], g = q[ch], b = q[2 * ch];
  if (channels != 4) return r | (g << 8) | (b << 16) | 0xFF000000u;
  const uint32_t a = q[3 * ch];
  return rs_premul(r, a) | (rs_premul(g, a) << 8) | (rs_premul(b, a) << 16) | (a << 24);
}

// grid: (ceil(dst_w / 64), ceil(s.h / 4), images); block 256.  s.w x s.h is the SOURCE extent; o = 1..4: intermediate row y is source row y (1, 2) or
// s.h - 1 - y (3, 4), sample x of it source column x (1, 4) or s.w - 1 - x (2, 3).
__global__ void __launch_bounds__(64 * MI_RS_TH) resample_h_kernel(const IngestSrc s, const int o, const uint32_t *bounds, const int32_t *taps, const uint32_t dst_w, const uint32_t pitch, uint32_t *inter) {
  __shared__ uint32_t tile[MI_RS_TH * MI_RS_CHUNK];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t ox0 = blockIdx.x * MI_RS_TW, ox = ox0 + lane, y0 = blockIdx.y * MI_RS_TH, y = y0 + wave, img = blockIdx.z;
  const bool live = ox < dst_w && y < s.h;
  const int xmin = ox < dst_w ? (int)bounds[2 * ox] : 0, cnt = live ? (int)bounds[2 * ox + 1] : 0;
  // the tile's span of the source row: first samples and ends both grow with the column
  const uint32_t last = ox0 + MI_RS_TW - 1 < dst_w ? ox0 + MI_RS_TW - 1 : dst_w - 1;
  const uint32_t lo = bounds[2 * ox0], hi = bounds[2 * last] + bounds[2 * last + 1];
  const uint32_t rows = s.h - y0 < MI_RS_TH ? s.h - y0 : MI_RS_TH;
  const size_t px = s.layout == 0 ? (size_t)s.inner_stride : 1, ch = s.layout == 0 ? 1 : (size_t)s.inner_stride;
  const uint8_t *const image = s.base + (size_t)img * s.image_stride;
  const bool alpha = s.channels == 4, flip_r = o == 3 || o == 4, flip_c = o == 2 || o == 3;
  uint32_t acc[4] = { 1u << (MI_RS_BITS - 1), 1u << (MI_RS_BITS - 1), 1u << (MI_RS_BITS - 1), 1u << (MI_RS_BITS - 1) };
  for (uint32_t c0 = lo; c0 < hi; c0 += MI_RS_CHUNK) {                             // uniform in the workgroup
    const uint32_t len = hi - c0 < MI_RS_CHUNK ? hi - c0 : MI_RS_CHUNK;
    for (uint32_t r = 0; r < rows; r++) {
      const uint8_t *const row = image + (size_t)(flip_r ? s.h - 1 - (y0 + r) : y0 + r) * s.row_stride;
      for (uint32_t i = threadIdx.x; i < len; i += 64 * MI_RS_TH) tile[r * MI_RS_CHUNK + i] = rs_load_px(row, flip_c ? s.w - 1 - (c0 + i) : c0 + i, px, ch, s.channels);
    }
    __syncthreads();
    // this lane's taps inside the chunk: j0 <= j < j1
    const int j0 = (int)c0 > xmin ? (int)c0 - xmin : 0, j1 = xmin + cnt < (int)(c0 + len) ? cnt : (int)(c0 + len) - xmin;
    const int at = (int)(wave * MI_RS_CHUNK) + xmin - (int)c0;                     // of tap 0 in the tile: 0 <= at + j < the row's len for j0 <= j < j1
    for (int j = j0; j < j1; j++) {
      const uint32_t v = tile[at + j], k = (uint32_t)taps[(size_t)j * dst_w + ox];
      acc[0] += (v & 255u) * k; acc[1] += ((v >> 8) & 255u) * k; acc[2] += ((v >> 16) & 255u) * k;
      if (alpha) acc[3] += (v >> 24) * k;
    }
    __syncthreads();                                                               // before the next chunk overwrites the tile
  }
  if (live) inter[((size_t)img * s.h + y) * pitch + ox] = rs_clip8(acc[0]) | (rs_clip8(acc[1]) << 8) | (rs_clip8(acc[2]) << 16) | (alpha ? rs_clip8(acc[3]) << 24 : 0xFF000000u);
}

// grid: (ceil(dst_w / 64), ceil(s.w / 64), images); block 256.  s.w x s.h is the SOURCE extent, o = 5..8; the tables are those of the axis s.h -> dst_w.
// Intermediate row c (7, 8: s.w - 1 - c) is source column c; its sample x sums source rows bounds[2 x] + j (6, 7: counted from the bottom).
__global__ void __launch_bounds__(256) resample_t_kernel(const IngestSrc s, const int o, const uint32_t *bounds, const int32_t *taps, const uint32_t dst_w, const uint32_t pitch, uint32_t *inter) {
  __shared__ uint32_t tile[MI_RS_TT * MI_RS_TP];
  const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));     // uniform: bounds, taps and range tests stay scalar
  const uint32_t ox0 = blockIdx.x * MI_RS_TT, c0 = blockIdx.y * MI_RS_TT, img = blockIdx.z;
  const bool flip_r = o == 6 || o == 7, flip_c = o == 7 || o == 8, alpha = s.channels == 4;
  const uint32_t c = c0 + lane;
  const bool has = c < s.w;
  const size_t px = s.layout == 0 ? (size_t)s.inner_stride : 1, ch = s.layout == 0 ? 1 : (size_t)s.inner_stride;
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
    uint32_t acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int k = 0; k < 4; k++) acc[q][k] = 1u << (MI_RS_BITS - 1);
    for (uint32_t t = xmin[0]; t < hi; t++) {                                      // rows of the oriented x axis: 0 <= t < s.h (the tables' input extent)
      const uint8_t *const row = image + (size_t)(flip_r ? s.h - 1 - t : t) * s.row_stride;
      const uint32_t v = has ? rs_load_px(row, c, px, ch, s.channels) : 0;
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t j = t - xmin[q];                                            // wraps to a large number below the range
        if (j < cnt[q]) {
          const uint32_t k = (uint32_t)taps[(size_t)j * dst_w + oxg + q];
          acc[q][0] += (v & 255u) * k; acc[q][1] += ((v >> 8) & 255u) * k; acc[q][2] += ((v >> 16) & 255u) * k;
          if (alpha) acc[q][3] += (v >> 24) * k;
        }
      }
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; q++)
      if (q < n) tile[(o0 + q) * MI_RS_TP + lane] = rs_clip8(acc[q][0]) | (rs_clip8(acc[q][1]) << 8) | (rs_clip8(acc[q][2]) << 16) | (alpha ? rs_clip8(acc[q][3]) << 24 : 0xFF000000u);
  }
  __syncthreads();
  const uint32_t nc = s.w - c0 < MI_RS_TT ? s.w - c0 : MI_RS_TT;                   // the tile's source columns (the grid leaves no empty tile)
  if (ox0 + lane < dst_w)
    for (uint32_t cl = wave; cl < nc; cl += 4) {
      const uint32_t oy = flip_c ? s.w - 1 - (c0 + cl) : c0 + cl;                  // < s.w, the intermediate's rows per image
      inter[((size_t)img * s.w + oy) * pitch + ox0 + lane] = tile[lane * MI_RS_TP + cl];
    }
}

// alpha: the picture has four channels (premultiplied in the intermediate); slots = slot of the first image.
template <int DC> __global__ void __launch_bounds__(64) resample_v_kernel(const uint32_t *inter, const uint32_t src_h, const uint32_t pitch, const uint32_t *bounds, const int32_t *taps,
                                                                          const uint32_t dst_w, const uint32_t dst_h, const int alpha, uint8_t *slots) {
  RowGroup4 g;
  if (!row_group4(dst_w, dst_h, g)) return;
  const uint32_t x0 = g.x0, oy = g.y, img = g.img;
  const uint32_t ymin = bounds[2 * oy], cnt = bounds[2 * oy + 1];
  const uint32_t *col = inter + ((size_t)img * src_h + ymin) * pitch + x0;         // 16-byte aligned: pitch and x0 are multiples of 4; the row's padding is read and not used
  const int32_t *k_ = taps + oy;
  uint32_t acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int c = 0; c < 4; c++) acc[p][c] = 1u << (MI_RS_BITS - 1);
  for (uint32_t j = 0; j < cnt; j++, col += pitch, k_ += dst_h) {
    const uint4 q = *(const uint4 *)col;
    const uint32_t k = (uint32_t)*k_, v[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
    for (int p = 0; p < 4; p++) {
      acc[p][0] += (v[p] & 255u) * k; acc[p][1] += ((v[p] >> 8) & 255u) * k; acc[p][2] += ((v[p] >> 16) & 255u) * k;
      if (alpha) acc[p][3] += (v[p] >> 24) * k;
    }
  }
  uint32_t px[4];
#pragma unroll
  for (int p = 0; p < 4; p++) {
    uint32_t r = rs_clip8(acc[p][0]), g = rs_clip8(acc[p][1]), b = rs_clip8(acc[p][2]), a = 255;
    if (alpha) {
      a = rs_clip8(acc[p][3]);
      if (a != 0 && a != 255) {                                                    // un-premultiply (Pillow's rgba2rgbA): integer division, clipped
        r = 255 * r / a; g = 255 * g / a; b = 255 * b / a;
        r = r > 255 ? 255 : r; g = g > 255 ? 255 : g; b = b > 255 ? 255 : b;
      }
    }
    px[p] = r | (g << 8) | (b << 16) | (a << 24);
  }
  slot_store4<DC>(slot_ptr<DC>(slots, dst_w, dst_h, g), px, g.n);
}

}  // namespace mi
