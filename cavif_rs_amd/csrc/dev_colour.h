// dev_colour.h -- colour-managed input: the colour channels of batch slots converted IN PLACE to sRGB by a transform the host baked
// (icc_reader.h: three input curves, a 3 x 3 matrix, the sRGB output curve).  Alpha is never read into the arithmetic and is stored back as it was.
//   colour_convert_kernel<DC>     8-bit slots (MI_INPUT_RGB), DC = channels of the slot
//   colour_convert16_kernel<DC>   deep slots (MI_INPUT_RGB16)
// Both work in the row groups of dev_slot.h, read with slot_load4 / slot16_load4 and written back with slot_store4 / slot16_store4, MI_COLOUR_ROWS rows per
// workgroup (grid y counts groups of rows), so that the table fill of the 8-bit kernel is paid once per MI_COLOUR_ROWS * 256 pixels.  No scratch in either.
//
// The arithmetic is integers only.  With the tables of icc_reader.h (lin8, lin16, matrix, U, out16), floor division and >> on negative numbers rounding
// towards minus infinity:
//   linear light of a byte v of channel c:      x_c = lin8[c][v]
//   linear light of a 16-bit sample s:          p = 4096 s, i = floor(p / 65535), f = p - 65535 i   (s = 0: entry 0; s = 65535: entry 4096, f = 0)
//                                               x_c = floor((lin16[c][i] (65535 - f) + lin16[c][i + 1] f + 32767) / 65535)
//   the matrix, for output channel i:           y_i = clamp((sum_j matrix[i][j] x_j + 2^29) >> 30, 0, 2^24)        (64-bit products and sums, half up)
//   a byte out:                                 the number of k in 1..255 with U[k] <= y_i                          (eight steps of a binary search; U ascends)
//   a 16-bit sample out:                        i = y >> 11, f = y & 2047,  (out16[i] (2048 - f) + out16[i + 1] f + 1024) >> 11
// icc_reader.h refuses coefficients of 64 and above (display profiles stay below 4): |matrix| < 2^36 and x <= 2^24, so a sum of three products stays below 2^62.
// The 8-bit tables (3 x 256 + 256 dwords = 4 KiB) are copied into LDS by every workgroup.  The 16-bit tables (3 x 4098 dwords + 8194 halfwords = 64 KiB) stay
// in global memory: they fit the L2 many times over, and in LDS they would leave two workgroups of one wavefront per CU (DESIGN.md 5h has the numbers).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_slot.h"

namespace mi {

constexpr int MI_COLOUR_ROWS = 8;
constexpr int MI_COLOUR_LIN16 = 4098, MI_COLOUR_OUT16 = 8194;   // entries per table: CT_LIN16_SEG + 2, CT_OUT16_SEG + 2

// what a launch gets: pointers into the transform's device copy (16-byte aligned) and the matrix by value
struct ColourDev {
  const uint32_t *tab8;                                        // lin8 R, G, B (256 each), then U (256): 1024 dwords
  const uint32_t *lin16;                                       // 3 x MI_COLOUR_LIN16
  const uint16_t *out16;                                       // MI_COLOUR_OUT16
  long long m[9];
};

__device__ __forceinline__ uint32_t colour_mix(const long long *m, const uint32_t x0, const uint32_t x1, const uint32_t x2) {
  const long long s = (m[0] * (long long)x0 + m[1] * (long long)x1 + m[2] * (long long)x2 + (1ll << 29)) >> 30;
  return s < 0 ? 0u : s > (1ll << 24) ? (1u << 24) : (uint32_t)s;
}
__device__ __forceinline__ uint32_t colour_level8(const uint32_t *U, const uint32_t y) {
  uint32_t lo = 0;
#pragma unroll
  for (uint32_t step = 128; step; step >>= 1) if (U[lo + step] <= y) lo += step;
  return lo;
}

// grid: grid_by_four over w x ceil(h / MI_COLOUR_ROWS); slots = slot of the first image
template <int DC> __global__ void __launch_bounds__(64) colour_convert_kernel(const ColourDev t, uint8_t *slots, const uint32_t w, const uint32_t h) {
  __shared__ uint32_t tab[1024];
#pragma unroll
  for (int k = 0; k < 4; k++) ((uint4 *)tab)[threadIdx.x + 64 * k] = ((const uint4 *)t.tab8)[threadIdx.x + 64 * k];
  __syncthreads();
  const uint32_t *const U = tab + 768;
  for (uint32_t r = 0; r < (uint32_t)MI_COLOUR_ROWS; r++) {
    RowGroup4 g;
    if (!row_group4(w, h, blockIdx.y * MI_COLOUR_ROWS + r, g)) break;
    const uint32_t n = g.n;
    uint8_t *p = slot_ptr<DC>(slots, w, h, g);
    uint32_t px[4];
    slot_load4<DC>(p, px, n);
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) if (k < n) {
      const uint32_t l0 = tab[px[k] & 255u], l1 = tab[256 + ((px[k] >> 8) & 255u)], l2 = tab[512 + ((px[k] >> 16) & 255u)];
      const uint32_t o0 = colour_level8(U, colour_mix(t.m, l0, l1, l2)), o1 = colour_level8(U, colour_mix(t.m + 3, l0, l1, l2)), o2 = colour_level8(U, colour_mix(t.m + 6, l0, l1, l2));
      px[k] = (px[k] & 0xFF000000u) | o0 | (o1 << 8) | (o2 << 16);
    }
    slot_store4<DC>(p, px, n);
  }
}

__device__ __forceinline__ uint32_t colour_lin16(const uint32_t *lin, const uint32_t s) {
  const uint32_t p = s * 4096u, i = p / 65535u, f = p - i * 65535u;
  return (uint32_t)(((unsigned long long)lin[i] * (65535u - f) + (unsigned long long)lin[i + 1] * f + 32767u) / 65535u);
}
__device__ __forceinline__ uint32_t colour_level16(const uint16_t *out, const uint32_t y) {
  const uint32_t i = y >> 11, f = y & 2047u;
  return ((uint32_t)out[i] * (2048u - f) + (uint32_t)out[i + 1] * f + 1024u) >> 11;
}

// grid: as above; slots = deep slot of the first image
template <int DC> __global__ void __launch_bounds__(64) colour_convert16_kernel(const ColourDev t, uint16_t *slots, const uint32_t w, const uint32_t h) {
#ifdef MI_COLOUR16_LDS                                          /* probe builds only (tools/colour_input_rate.py): the three input tables, 48 KiB, in LDS */
  __shared__ uint32_t lds_lin[3 * MI_COLOUR_LIN16];
  for (uint32_t k = threadIdx.x; k < 3u * MI_COLOUR_LIN16 / 2; k += 64) ((uint2 *)lds_lin)[k] = ((const uint2 *)t.lin16)[k];
  __syncthreads();
  const uint32_t *const lin16 = lds_lin;
#else
  const uint32_t *const lin16 = t.lin16;
#endif
  for (uint32_t r = 0; r < (uint32_t)MI_COLOUR_ROWS; r++) {
    RowGroup4 g;
    if (!row_group4(w, h, blockIdx.y * MI_COLOUR_ROWS + r, g)) break;
    const uint32_t n = g.n;
    uint16_t *p = slot_ptr<DC>(slots, w, h, g);
    uint2 px[4];
    slot16_load4<DC>(p, px, n);
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) if (k < n) {
      const uint32_t l0 = colour_lin16(lin16, px[k].x & 0xFFFFu), l1 = colour_lin16(lin16 + MI_COLOUR_LIN16, px[k].x >> 16), l2 = colour_lin16(lin16 + 2 * MI_COLOUR_LIN16, px[k].y & 0xFFFFu);
      const uint32_t o0 = colour_level16(t.out16, colour_mix(t.m, l0, l1, l2)), o1 = colour_level16(t.out16, colour_mix(t.m + 3, l0, l1, l2)), o2 = colour_level16(t.out16, colour_mix(t.m + 6, l0, l1, l2));
      px[k].x = o0 | (o1 << 16); px[k].y = (px[k].y & 0xFFFF0000u) | o2;
    }
    slot16_store4<DC>(p, px, n);
  }
}

}  // namespace mi
