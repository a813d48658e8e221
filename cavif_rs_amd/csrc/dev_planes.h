// dev_planes.h -- YCbCr planes that already live in HBM (what a hardware JPEG / video decoder delivers: Y plus subsampled Cb, Cr, planar or with Cb and Cr
// interleaved, NV12-style) -> the packed (Y, Cb, Cr[, 255]) bytes of a batch's input slot of kind MI_INPUT_YCBCR.
//   planes_ingest_kernel  in the row groups of dev_slot.h, a group being four adjacent luma pixels.  Luma: one dword where the address allows it, bytes
//                         otherwise and for a last partial group.  Chroma: brought to
//                         luma resolution by jpeg_chroma4 (dev_jpeg.h: libjpeg's h2v1 / h2v2 triangle filter, edges replicated, planes of one or two
//                         samples' width replicated; samples centred between the luma samples they cover, as in JPEG), which reads its four neighbours
//                         per row with byte loads.  A wavefront's chroma reads cover 130 adjacent bytes of at most two rows per plane (260 interleaved),
//                         each byte wanted by up to four lanes and by the wavefronts of the row above or below: they are served by the vector L1 and L2,
//                         not staged in LDS (measured: profiles/ycc_input.md).  No LDS, no scratch.
// Deep planes (uint16 samples of 8..16 bits, full or narrow range: P010 / P016 with interleaved (Cb, Cr) pairs, or planar) -> the packed
// (Y, Cb, Cr[, 65535]) uint16 samples of a deep slot of kind MI_INPUT_YCBCR16, in the canonical form of include/mi_avif.h (full range, M = 65535, chroma
// centred on 32768).
//   planes_ingest16_kernel  the same row groups.  Luma: deep_load_run (8 bytes per group in the widest form the address allows), halfwords for a last
//                         partial group.  Chroma: ycc16_chroma4, jpeg_chroma4's filter on canonical samples -- every neighbour goes through the sample map
//                         first, then the 3:1 weights (a sum stays below 16 * 65535).  The map's divisor (2^bits - 1, 219 s, 224 s) is a per-call
//                         constant: the host passes its multiply-high reciprocal (SampleMap16), the kernel holds no division.  No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_slot.h"
#include "dev_jpeg.h"                     // jpeg_chroma4

namespace mi {

struct PlanesSrc {
  const uint8_t *y, *cb, *cr;                                   // cr == cb + 1 and cpitch == 2 for interleaved pairs
  unsigned long long y_row, c_row, y_image, c_image;            // byte strides
  uint32_t w, h, cw, ch, hsub, vsub;                            // cw x ch = ceil(w / hsub) x ceil(h / vsub)
  int cpitch;                                                   // bytes from one chroma sample of a plane to the next: 1 | 2
};

// slots = slot of the first image
template <int DC> __global__ void __launch_bounds__(64) planes_ingest_kernel(const PlanesSrc s, uint8_t *slots) {
  RowGroup4 g;
  if (!row_group4(s.w, s.h, g)) return;
  const uint32_t x0 = g.x0, y = g.y, img = g.img, n = g.n;
  const uint32_t yv = plane_load4(s.y + (size_t)img * s.y_image + (size_t)y * s.y_row + x0, n);
  const uint8_t *cb = s.cb + (size_t)img * s.c_image, *cr = s.cr + (size_t)img * s.c_image;
  int c1[4], c2[4];
  if (s.cpitch == 2) {
    jpeg_chroma4<2, false>(cb, (size_t)s.c_row, s.cw, s.ch, s.hsub, s.vsub, x0, y, n, c1);
    jpeg_chroma4<2, false>(cr, (size_t)s.c_row, s.cw, s.ch, s.hsub, s.vsub, x0, y, n, c2);
  } else {
    jpeg_chroma4<1, false>(cb, (size_t)s.c_row, s.cw, s.ch, s.hsub, s.vsub, x0, y, n, c1);
    jpeg_chroma4<1, false>(cr, (size_t)s.c_row, s.cw, s.ch, s.hsub, s.vsub, x0, y, n, c2);
  }
  uint32_t px[4];
#pragma unroll
  for (int k = 0; k < 4; k++) px[k] = ((yv >> (8 * k)) & 255u) | ((uint32_t)c1[k] << 8) | ((uint32_t)c2[k] << 16) | 0xFF000000u;
  slot_store4<DC>(slot_ptr<DC>(slots, s.w, s.h, g), px, n);
}

// ---------------------------------------------------------------- deep planes
// W = clamp(floor((65535 v + bias) / d), 0, 65535) for a sample v already reduced to its bits: the maps of include/mi_avif.h with the factor 2 taken out of
// dividend and divisor (d is odd or the halved rounding term is exact) and, for chroma, the centre 32768 folded into bias.  The dividend is below 2^32 for every
// v wherever it is not negative, and floor(n / d) == umulhi(n, magic) >> shift for every such n (magic = floor(2^(32 + shift) / d) + 1, shift = floor(log2 d):
// make_sample_map16 in host_input.h; tests/helpers/ycc16_cases.py runs every value of every bit count through it).
struct SampleMap16 { uint32_t magic; int32_t bias; uint32_t shift; };
struct Planes16Src {
  const uint8_t *y, *cb, *cr;                                   // cr unused for interleaved pairs (pairs != 0): cb points at (Cb, Cr) uint16 pairs
  unsigned long long y_row, c_row, y_image, c_image;            // byte strides, even
  uint32_t w, h, cw, ch, hsub, vsub;                            // cw x ch = ceil(w / hsub) x ceil(h / vsub)
  int pairs;
  uint32_t down, mask;                                          // a sample reduced to its bits: (v >> down) & mask
  SampleMap16 ym, cm;
};
__device__ __forceinline__ uint32_t sample_map16(const uint32_t raw, const uint32_t down, const uint32_t mask, const SampleMap16 &m) {
  const uint32_t mv = 65535u * ((raw >> down) & mask);
  const bool below = m.bias < 0 && mv < (uint32_t)(-m.bias);   // a negative dividend: the quotient is below 0 and clamps to it
  const uint32_t q = __umulhi(mv + (uint32_t)m.bias, m.magic) >> m.shift;
  return below ? 0u : q < 65535u ? q : 65535u;
}

template <bool PAIRS> __device__ __forceinline__ uint32_t ycc16_pair(const uint8_t *cb_row, const uint8_t *cr_row, const uint32_t i) {      // Cb | Cr << 16 of chroma column i
  if (PAIRS) {
    const uint8_t *q = cb_row + (size_t)i * 4;
    return ((uintptr_t)q & 3) == 0 ? *(const uint32_t *)q : (uint32_t)((const uint16_t *)q)[0] | ((uint32_t)((const uint16_t *)q)[1] << 16);
  }
  return (uint32_t)((const uint16_t *)cb_row)[i] | ((uint32_t)((const uint16_t *)cr_row)[i] << 16);
}
// Cb and Cr of pixels x0..x0+3 of row y at luma resolution, in canonical samples: jpeg_chroma4 (dev_jpeg.h) for uint16 planes, both components at once so that
// an interleaved pair is one dword where its address allows it.  Every sample read goes through the sample map before the filter.  PAIRS: cb points at
// (Cb, Cr) pairs, else cb and cr are planes of their own; strides in bytes.  At 4:4:4 a sample that does not exist (k >= n) is not read: its pair counts as 0.
template <bool PAIRS> __device__ __forceinline__ void ycc16_chroma4(const Planes16Src &s, const uint8_t *cb, const uint8_t *cr, const uint32_t x0, const uint32_t y,
                                                                    const uint32_t n, uint32_t c1[4], uint32_t c2[4]) {
  const size_t stride = (size_t)s.c_row;
  const uint32_t cw = s.cw, ch = s.ch, vr = s.vsub;
  const uint32_t yn = vr == 2 ? y >> 1 : y;
  const uint8_t *nb = cb + (size_t)yn * stride, *nr = cr + (size_t)yn * stride;
  uint32_t p[4] = { 0, 0, 0, 0 };                                // the pairs the group starts from: its own (4:4:4, replicated planes) or its four neighbour columns
  if (s.hsub == 1) {
    if (n == 4) {
      if (PAIRS) deep_load_run<4>(nb + (size_t)x0 * 4, p);
      else {
        uint32_t d[2], e[2];
        deep_load_run<2>(nb + (size_t)x0 * 2, d); deep_load_run<2>(nr + (size_t)x0 * 2, e);
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = deep_half(d, k) | (deep_half(e, k) << 16);
      }
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) if (k < n) p[k] = ycc16_pair<PAIRS>(nb, nr, x0 + k);
    }
  } else if (cw <= 2) {                                          // planes of one or two samples' width are replicated, as libjpeg does
    const uint32_t i0 = x0 >> 1, i1 = i0 + 1 < cw ? i0 + 1 : cw - 1;
    p[0] = p[1] = ycc16_pair<PAIRS>(nb, nr, i0); p[2] = p[3] = ycc16_pair<PAIRS>(nb, nr, i1);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      uint32_t i = (x0 >> 1) + k; i = i > 0 ? i - 1 : 0; i = i < cw ? i : cw - 1;
      p[k] = ycc16_pair<PAIRS>(nb, nr, i);
    }
  }
  uint32_t a[4], b[4];
#pragma unroll
  for (int k = 0; k < 4; k++) { a[k] = sample_map16(p[k] & 0xFFFFu, s.down, s.mask, s.cm); b[k] = sample_map16(p[k] >> 16, s.down, s.mask, s.cm); }
  if (s.hsub == 1 || cw <= 2) {
#pragma unroll
    for (int k = 0; k < 4; k++) { c1[k] = a[k]; c2[k] = b[k]; }
    return;
  }
  if (vr == 2) {
    const uint32_t yf = (y & 1) ? (yn + 1 < ch ? yn + 1 : ch - 1) : (yn > 0 ? yn - 1 : 0);
    const uint8_t *fb = cb + (size_t)yf * stride, *fr = cr + (size_t)yf * stride;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      uint32_t i = (x0 >> 1) + k; i = i > 0 ? i - 1 : 0; i = i < cw ? i : cw - 1;
      const uint32_t f = ycc16_pair<PAIRS>(fb, fr, i);
      a[k] = 3 * a[k] + sample_map16(f & 0xFFFFu, s.down, s.mask, s.cm); b[k] = 3 * b[k] + sample_map16(f >> 16, s.down, s.mask, s.cm);
    }
    c1[0] = (3 * a[1] + a[0] + 8) >> 4; c1[1] = (3 * a[1] + a[2] + 7) >> 4; c1[2] = (3 * a[2] + a[1] + 8) >> 4; c1[3] = (3 * a[2] + a[3] + 7) >> 4;
    c2[0] = (3 * b[1] + b[0] + 8) >> 4; c2[1] = (3 * b[1] + b[2] + 7) >> 4; c2[2] = (3 * b[2] + b[1] + 8) >> 4; c2[3] = (3 * b[2] + b[3] + 7) >> 4;
  } else {
    c1[0] = (3 * a[1] + a[0] + 1) >> 2; c1[1] = (3 * a[1] + a[2] + 2) >> 2; c1[2] = (3 * a[2] + a[1] + 1) >> 2; c1[3] = (3 * a[2] + a[3] + 2) >> 2;
    c2[0] = (3 * b[1] + b[0] + 1) >> 2; c2[1] = (3 * b[1] + b[2] + 2) >> 2; c2[2] = (3 * b[2] + b[1] + 1) >> 2; c2[3] = (3 * b[2] + b[3] + 2) >> 2;
  }
}

// slots = deep slot of the first image
template <int DC> __global__ void __launch_bounds__(64) planes_ingest16_kernel(const Planes16Src s, uint16_t *slots) {
  RowGroup4 g;
  if (!row_group4(s.w, s.h, g)) return;
  const uint32_t x0 = g.x0, y = g.y, img = g.img, n = g.n;
  const uint8_t *yp = s.y + (size_t)img * s.y_image + (size_t)y * s.y_row + (size_t)x0 * 2;
  uint32_t yv[2] = { 0, 0 };
  if (n == 4) deep_load_run<2>(yp, yv);
  else {
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) if (k < n) yv[k >> 1] |= (uint32_t)((const uint16_t *)yp)[k] << (16 * (k & 1));
  }
  const uint8_t *cb = s.cb + (size_t)img * s.c_image, *cr = s.cr + (size_t)img * s.c_image;
  uint32_t c1[4], c2[4];
  if (s.pairs) ycc16_chroma4<true>(s, cb, cb, x0, y, n, c1, c2);
  else ycc16_chroma4<false>(s, cb, cr, x0, y, n, c1, c2);
  uint2 px[4];
#pragma unroll
  for (int k = 0; k < 4; k++) { px[k].x = sample_map16(deep_half(yv, k), s.down, s.mask, s.ym) | (c1[k] << 16); px[k].y = c2[k] | 0xFFFF0000u; }
  slot16_store4<DC>(slot_ptr<DC>(slots, s.w, s.h, g), px, n);
}

}  // namespace mi
