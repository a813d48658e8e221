// dev_ingest.h -- pictures that already live in HBM -> the packed layout of a batch's input slot (w*h*channels bytes, rows packed, images back to back).
//   IngestSrc       a strided picture in device memory: what ingest_kernel, ingest16_kernel (dev_deep.h), resample_h_kernel (dev_resample.h) and orient_kernel (dev_orient.h) read
//   ingest_load4    four adjacent pixels of such a picture's row, in the widest loads its addresses allow: ingest_kernel's and orient_kernel's (dev_orient.h) read
//   ingest_kernel   uint8 HWC or CHW pictures with arbitrary byte strides (torch views: crops, permuted tensors, padded rows) -> slot, in the row groups of
//                   dev_slot.h: a wavefront reads one contiguous run of an interleaved row (1 KiB for packed RGBA) or one 256-byte run per plane.  No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_slot.h"

namespace mi {

struct IngestSrc {
  const uint8_t *base;
  unsigned long long image_stride, row_stride, inner_stride;    // bytes; inner: from pixel to pixel (HWC) or from plane to plane (CHW)
  uint32_t w, h;
  int layout, channels;                                         // 0 = HWC, 1 = CHW; 3 | 4 (3 into an RGBA slot: alpha 255)
};

// Pixels x0 .. x0 + n - 1 (n = 1..4) of a source row that starts at `row`, as slot_store4 takes them (3 channels: alpha 255; px[k] for k >= n is not to be used).
// Wide loads where the source is packed and aligned for them (slot_load4; one dword per plane), byte loads otherwise and for a last partial group: decided per
// thread from its own addresses.
__device__ __forceinline__ void ingest_load4(const IngestSrc &s, const uint8_t *row, const uint32_t x0, const uint32_t n, uint32_t px[4]) {
  const uint32_t opaque = s.channels == 4 ? 0u : 0xFF000000u;
  px[0] = px[1] = px[2] = px[3] = 0;
  if (s.layout == 0) {
    const uint8_t *p = row + (size_t)x0 * s.inner_stride;
    const bool packed = s.inner_stride == (unsigned long long)s.channels;
    if (packed && s.channels == 4 && ((uintptr_t)p & 3) == 0) slot_load4<4>(p, px, n);
    else if (packed && s.channels == 3) slot_load4<3>(p, px, n);
    else {
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) if (k < n) {
        const uint8_t *q = p + (size_t)k * s.inner_stride;
        px[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | (s.channels == 4 ? (uint32_t)q[3] << 24 : 0u);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) px[k] |= opaque;
  } else {
    uint32_t v[4] = { 0, 0, 0, 0xFFFFFFFFu };                   // four samples of each plane, sample k in byte k
#pragma unroll
    for (int c = 0; c < 4; c++) if (c < s.channels) v[c] = plane_load4(row + (size_t)c * s.inner_stride + x0, n);
#pragma unroll
    for (int k = 0; k < 4; k++) px[k] = ((v[0] >> (8 * k)) & 255u) | (((v[1] >> (8 * k)) & 255u) << 8) | (((v[2] >> (8 * k)) & 255u) << 16) | ((v[3] >> (8 * k)) << 24);
  }
}

// dst = slot of the first image
template <int DC> __global__ void __launch_bounds__(64) ingest_kernel(const IngestSrc s, uint8_t *slots) {
  RowGroup4 g;
  if (!row_group4(s.w, s.h, g)) return;
  uint32_t px[4];
  ingest_load4(s, s.base + (size_t)g.img * s.image_stride + (size_t)g.y * s.row_stride, g.x0, g.n, px);
  slot_store4<DC>(slot_ptr<DC>(slots, s.w, s.h, g), px, g.n);
}

}  // namespace mi
