// dev_planes.h -- YCbCr planes that already live in HBM (what a hardware JPEG / video decoder delivers: Y plus subsampled Cb, Cr, planar or with Cb and Cr
// interleaved, NV12-style) -> the packed (Y, Cb, Cr[, 255]) bytes of a batch's input slot of kind MI_INPUT_YCBCR.
//   planes_ingest_kernel  in the row groups of dev_slot.h, a group being four adjacent luma pixels.  Luma: one dword where the address allows it, bytes
//                         otherwise and for a last partial group.  Chroma: brought to
//                         luma resolution by jpeg_chroma4 (dev_jpeg.h: libjpeg's h2v1 / h2v2 triangle filter, edges replicated, planes of one or two
//                         samples' width replicated; samples centred between the luma samples they cover, as in JPEG), which reads its four neighbours
//                         per row with byte loads.  A wavefront's chroma reads cover 130 adjacent bytes of at most two rows per plane (260 interleaved),
//                         each byte wanted by up to four lanes and by the wavefronts of the row above or below: they are served by the vector L1 and L2,
//                         not staged in LDS (measured: profiles/ycc_input.md).  No LDS, no scratch.
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

}  // namespace mi
