// dev_jpeg.h -- the device half of the JPEG input side: quantised coefficients (jpeg_reader.h) -> RGBA8 in HBM, two kernels (the second in the row groups of dev_slot.h).
// A JPEG decoder's pixels are not normative; these are libjpeg's in its default configuration (what Pillow and most tools produce), all integer:
//   jpeg_idct_kernel  dequantise + the "islow" 8x8 inverse DCT (CONST_BITS 13, PASS1_BITS 2: column pass descaled by 11 bits, row pass by 18, round half
//                     up, +128, clamp) -> one uint8 plane per component over the MCU-padded block grid
//   jpeg_colour_kernel<DC>  "fancy" (triangle) chroma upsampling 2x1 / 2x2 with edge samples replicated, then YCbCr -> RGB in 16.16 fixed point
//                     (or a copy for grey / RGB files), alpha 255; DC 3 stores packed RGB8 (3-channel batches)
//   jpeg_ycc_kernel<DC>     the same upsampling and no colour arithmetic: (Y, Cb, Cr) as the file holds them, for slots of input kind MI_INPUT_YCBCR
// libjpeg computes the IDCT in 64-bit long; here products and sums are uint32_t (wrapping) and only the descale shifts see them as int32_t: identical
// whenever libjpeg's values fit 32 bits, which they do for every encoder-made file, and some defined value for hostile coefficients.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_slot.h"

namespace mi {

struct JpegDevGeom {
  uint32_t w, h, ncomp, color;            // color: JPEG_GREY / JPEG_YCBCR / JPEG_RGB
  uint32_t nblocks;
  uint32_t first_block[3];                // of each component in the coefficient array; nblocks for a component the file does not have
  uint32_t bw[3], bh[3], cw[3], ch[3];    // block grid and picture-carrying extent of each plane (plane stride = 8 * bw)
  uint32_t hr, vr;                        // luma samples per chroma sample: 1x1, 2x1 or 2x2
  unsigned long long plane_off[3];        // byte offset of each plane in the plane buffer (64 * first_block)
};

#define MI_JPEG_IDCT_BLOCKS 32            /* 8x8 blocks per workgroup: 8 lanes each, 256 threads */
#define MI_JPEG_OUT_STRIDE 36             /* uint2 per row of the store-order staging: 36 = 4 mod 16 spreads the 8 rows of a 32-lane write group over the bank pairs */

// one 8-point pass of the islow IDCT over in[0..7]; out[k] = (x + 2^(shift-1)) >> shift, arithmetic
__device__ __forceinline__ void jpeg_idct8(const uint32_t in[8], const int shift, int32_t out[8]) {
  uint32_t z2 = in[2], z3 = in[6];
  uint32_t z1 = (z2 + z3) * 4433u;                               // FIX(0.541196100)
  const uint32_t e2 = z1 - z3 * 15137u;                          // -FIX(1.847759065)
  const uint32_t e3 = z1 + z2 * 6270u;                           // FIX(0.765366865)
  z2 = in[0]; z3 = in[4];
  const uint32_t e0 = (z2 + z3) << 13, e1 = (z2 - z3) << 13;
  const uint32_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  uint32_t t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
  z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
  uint32_t z4 = t1 + t3;
  const uint32_t z5 = (z3 + z4) * 9633u;                         // FIX(1.175875602)
  t0 *= 2446u; t1 *= 16819u; t2 *= 25172u; t3 *= 12299u;
  z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
  z3 = z3 * (uint32_t)-16069 + z5; z4 = z4 * (uint32_t)-3196 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  const uint32_t r = 1u << (shift - 1);
  out[0] = (int32_t)(t10 + t3 + r) >> shift; out[7] = (int32_t)(t10 - t3 + r) >> shift;
  out[1] = (int32_t)(t11 + t2 + r) >> shift; out[6] = (int32_t)(t11 - t2 + r) >> shift;
  out[2] = (int32_t)(t12 + t1 + r) >> shift; out[5] = (int32_t)(t12 - t1 + r) >> shift;
  out[3] = (int32_t)(t13 + t0 + r) >> shift; out[4] = (int32_t)(t13 - t0 + r) >> shift;
}

__device__ __forceinline__ uint32_t jpeg_clamp255(int v) { return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
__device__ __forceinline__ int jpeg_comp_of(const JpegDevGeom &g, uint32_t b) { return b >= g.first_block[2] ? 2 : b >= g.first_block[1] ? 1 : 0; }

// coef: nblocks x 64 int16 in natural order; quant: 3 x 64 uint16.  Lane (block, i) of a workgroup's 32 blocks: loads row i (16 bytes: a wavefront reads
// 1 KiB contiguous), is column i in the column pass and row i in the row pass; the block lives in LDS in between, rows 9 words apart (conflict-free for
// the row-wise writes and the column-wise reads alike).  The packed rows then change lanes once more so that a wavefront stores two 256-byte runs of a
// plane row where the workgroup's blocks are neighbours in the grid.
__global__ void __launch_bounds__(256) jpeg_idct_kernel(const int16_t *coef, const uint16_t *quant, const JpegDevGeom g, uint8_t *planes) {
  __shared__ int32_t ws[MI_JPEG_IDCT_BLOCKS * 72];
  __shared__ uint2 outs[8 * MI_JPEG_OUT_STRIDE];
  const uint32_t t = threadIdx.x, lb = t >> 3, i = t & 7;
  const uint32_t b = blockIdx.x * MI_JPEG_IDCT_BLOCKS + lb;
  uint32_t x[8]; int32_t o[8];
  if (b < g.nblocks) {
    const uint4 cv = *(const uint4 *)(coef + (size_t)b * 64 + i * 8);
    const uint4 qv = *(const uint4 *)(quant + jpeg_comp_of(g, b) * 64 + i * 8);
    const uint32_t cw[4] = { cv.x, cv.y, cv.z, cv.w }, qw[4] = { qv.x, qv.y, qv.z, qv.w };
    for (int j = 0; j < 4; j++) {
      x[2 * j] = (uint32_t)(int32_t)(int16_t)(cw[j] & 0xFFFFu) * (qw[j] & 0xFFFFu);
      x[2 * j + 1] = (uint32_t)(int32_t)(int16_t)(cw[j] >> 16) * (qw[j] >> 16);
    }
  } else for (int j = 0; j < 8; j++) x[j] = 0;
  for (int j = 0; j < 8; j++) ws[(lb * 8 + i) * 9 + j] = (int32_t)x[j];
  __syncthreads();
  for (int k = 0; k < 8; k++) x[k] = (uint32_t)ws[(lb * 8 + k) * 9 + i];
  jpeg_idct8(x, 11, o);
  for (int k = 0; k < 8; k++) ws[(lb * 8 + k) * 9 + i] = o[k];
  __syncthreads();
  for (int j = 0; j < 8; j++) x[j] = (uint32_t)ws[(lb * 8 + i) * 9 + j];
  jpeg_idct8(x, 18, o);
  uint2 px;
  px.x = jpeg_clamp255(o[0] + 128) | (jpeg_clamp255(o[1] + 128) << 8) | (jpeg_clamp255(o[2] + 128) << 16) | (jpeg_clamp255(o[3] + 128) << 24);
  px.y = jpeg_clamp255(o[4] + 128) | (jpeg_clamp255(o[5] + 128) << 8) | (jpeg_clamp255(o[6] + 128) << 16) | (jpeg_clamp255(o[7] + 128) << 24);
  outs[i * MI_JPEG_OUT_STRIDE + lb] = px;
  __syncthreads();
  const uint32_t row = t >> 5, sb = t & 31, b2 = blockIdx.x * MI_JPEG_IDCT_BLOCKS + sb;
  if (b2 < g.nblocks) {
    const int c = jpeg_comp_of(g, b2);
    const uint32_t local = b2 - g.first_block[c], by = local / g.bw[c], bx = local - by * g.bw[c];
    *(uint2 *)(planes + g.plane_off[c] + ((size_t)by * 8 + row) * ((size_t)g.bw[c] * 8) + (size_t)bx * 8) = outs[row * MI_JPEG_OUT_STRIDE + sb];
  }
}

// four horizontally adjacent samples x0..x0+3 of row y of a chroma plane brought to luma resolution (libjpeg's h2v1 / h2v2 fancy upsampling: weights 3:1
// towards the nearer sample in each direction, neighbours outside the plane's cw x ch extent replaced by the nearest one inside; plain replication in
// both directions when the plane is one or two samples wide, as libjpeg does).  The one implementation of the upsampling: the JPEG kernels below and
// planes_ingest_kernel (dev_planes.h) call it.  PS = bytes from one sample of the plane to the next (1; 2 for interleaved (Cb, Cr) pairs).  PADDED: every
// row holds whole aligned dwords past cw (the MCU-padded planes of jpeg_idct_kernel), so a plane at luma resolution is read as one dword; otherwise a
// dword where the address allows it and n = 4, bytes for the n (1..4) samples that exist else (out[k] for k >= n is 0 then).
template <int PS, bool PADDED> __device__ __forceinline__ void jpeg_chroma4(const uint8_t *plane, const size_t stride, const uint32_t cw, const uint32_t ch, const uint32_t hr,
                                                                            const uint32_t vr, const uint32_t x0, const uint32_t y, const uint32_t n, int out[4]) {
  if (hr == 1) {
    const uint8_t *q = plane + (size_t)y * stride + (size_t)x0 * PS;
    if (PS == 1 && (PADDED || (n == 4 && ((uintptr_t)q & 3) == 0))) {
      const uint32_t v = *(const uint32_t *)q;
      out[0] = v & 255; out[1] = (v >> 8) & 255; out[2] = (v >> 16) & 255; out[3] = v >> 24;
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) out[k] = k < n ? q[(size_t)k * PS] : 0;
    }
    return;
  }
  const uint32_t yn = vr == 2 ? y >> 1 : y;
  if (cw <= 2) {                                                 // libjpeg takes the triangle filter only for planes wider than two samples and replicates otherwise
    const uint8_t *row = plane + (size_t)yn * stride;
    const uint32_t i0 = x0 >> 1, i1 = i0 + 1 < cw ? i0 + 1 : cw - 1;
    out[0] = out[1] = row[(size_t)i0 * PS]; out[2] = out[3] = row[(size_t)i1 * PS];
    return;
  }
  const uint32_t yf = vr == 2 ? ((y & 1) ? (yn + 1 < ch ? yn + 1 : ch - 1) : (yn > 0 ? yn - 1 : 0)) : yn;
  const uint8_t *near = plane + (size_t)yn * stride, *far = plane + (size_t)yf * stride;
  const uint32_t i0 = x0 >> 1;
  int s[4];
  for (int k = 0; k < 4; k++) {
    uint32_t i = i0 + k; i = i > 0 ? i - 1 : 0; i = i < cw ? i : cw - 1;
    s[k] = vr == 2 ? 3 * near[(size_t)i * PS] + far[(size_t)i * PS] : near[(size_t)i * PS];
  }
  if (vr == 2) {
    out[0] = (3 * s[1] + s[0] + 8) >> 4; out[1] = (3 * s[1] + s[2] + 7) >> 4;
    out[2] = (3 * s[2] + s[1] + 8) >> 4; out[3] = (3 * s[2] + s[3] + 7) >> 4;
  } else {
    out[0] = (3 * s[1] + s[0] + 1) >> 2; out[1] = (3 * s[1] + s[2] + 2) >> 2;
    out[2] = (3 * s[2] + s[1] + 1) >> 2; out[3] = (3 * s[2] + s[3] + 2) >> 2;
  }
}

// the component samples of pixels x0..x0+3 of row y at luma resolution: c0 from plane 0, c1 / c2 the upsampled planes 1 / 2 of a three-component file
// (a one-component file leaves them as they are).  What the colour kernels and jpeg_ycc_kernel start from.
__device__ __forceinline__ void jpeg_samples4(const uint8_t *planes, const JpegDevGeom &g, const uint32_t x0, const uint32_t y, int c0[4], int c1[4], int c2[4]) {
  const uint32_t yv = *(const uint32_t *)(planes + g.plane_off[0] + (size_t)y * ((size_t)g.bw[0] * 8) + x0);
  c0[0] = (int)(yv & 255); c0[1] = (int)((yv >> 8) & 255); c0[2] = (int)((yv >> 16) & 255); c0[3] = (int)(yv >> 24);
  if (g.ncomp == 3) {
    jpeg_chroma4<1, true>(planes + g.plane_off[1], (size_t)g.bw[1] * 8, g.cw[1], g.ch[1], g.hr, g.vr, x0, y, 4, c1);
    jpeg_chroma4<1, true>(planes + g.plane_off[2], (size_t)g.bw[2] * 8, g.cw[2], g.ch[2], g.hr, g.vr, x0, y, 4, c2);
  }
}

// planes -> RGBA8 (DC 4) or RGB8 (DC 3) rows of stride_px pixels at a device pointer (a batch slot: stride_px = w), in the row groups of dev_slot.h over
// g.w x g.h, one image per launch.  Alpha is 255.  The one implementation of the colour arithmetic.
template <int DC> __global__ void __launch_bounds__(64) jpeg_colour_kernel(const uint8_t *planes, const JpegDevGeom g, uint8_t *out, const size_t stride_px) {
  RowGroup4 grp;
  if (!row_group4(g.w, g.h, grp)) return;
  int c0[4], c1[4], c2[4];
  jpeg_samples4(planes, g, grp.x0, grp.y, c0, c1, c2);
  uint32_t px[4];
  if (g.ncomp == 3) {
    for (int k = 0; k < 4; k++) {
      uint32_t r, gg, b;
      if (g.color == 1) {                                        // YCbCr: 1.40200, 0.34414, 0.71414, 1.77200 in 16.16
        const int cb = c1[k] - 128, cr = c2[k] - 128;
        r = jpeg_clamp255(c0[k] + ((91881 * cr + 32768) >> 16));
        gg = jpeg_clamp255(c0[k] + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        b = jpeg_clamp255(c0[k] + ((116130 * cb + 32768) >> 16));
      } else { r = (uint32_t)c0[k]; gg = (uint32_t)c1[k]; b = (uint32_t)c2[k]; }
      px[k] = r | (gg << 8) | (b << 16) | 0xFF000000u;
    }
  } else for (int k = 0; k < 4; k++) px[k] = (uint32_t)c0[k] * 0x010101u | 0xFF000000u;
  slot_store4<DC>(group_ptr<DC>(out, 0, stride_px, grp), px, grp.n);
}
// planes -> the file's own samples, no colour arithmetic: (Y, Cb, Cr, 255) of a three-component YCbCr file (chroma upsampled as above), (Y, 128, 128, 255)
// of a grey one, into a slot of DC channels (DC 3: without the fourth byte).  Thread shape and store as for the colour kernel.
template <int DC> __global__ void __launch_bounds__(64) jpeg_ycc_kernel(const uint8_t *planes, const JpegDevGeom g, uint8_t *out, const size_t stride_px) {
  RowGroup4 grp;
  if (!row_group4(g.w, g.h, grp)) return;
  int c0[4], c1[4] = { 128, 128, 128, 128 }, c2[4] = { 128, 128, 128, 128 };
  jpeg_samples4(planes, g, grp.x0, grp.y, c0, c1, c2);
  uint32_t px[4];
  for (int k = 0; k < 4; k++) px[k] = (uint32_t)c0[k] | ((uint32_t)c1[k] << 8) | ((uint32_t)c2[k] << 16) | 0xFF000000u;
  slot_store4<DC>(group_ptr<DC>(out, 0, stride_px, grp), px, grp.n);
}

}  // namespace mi
