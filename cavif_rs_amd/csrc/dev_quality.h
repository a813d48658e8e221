// dev_quality.h -- quality metrics of a finished encode: per frame and plane the exact sum of squared errors and a fixed-point SSIM sum between
// the source planes (FrameDev::src) and the final reconstruction (lrp when the frame runs loop restoration, else fin), over the visible w x h samples only.
//   quality_kernel      one launch for every frame and plane of a batch, driven by the frame descriptors the encode left on the device: grid
//                       (64 x 64 tiles of a padded plane, 3 planes, frames), block 256.  A workgroup takes one tile plus a halo of one 4 x 4 cell on the right
//                       and below (17 x 17 cells).  Pass 1: a thread loads a cell from both planes with one 8-byte load per row and plane (cell i of the tile
//                       in row-major order goes to thread i, so a wavefront reads runs of 17 adjacent cells) and leaves the five sums S, R, SS, RR, SR of its
//                       samples in LDS; samples outside w x h count as zero in both planes, so a partial cell at the picture's edge still gives its squared
//                       errors and a cell outside gives nothing.  Pass 2: a thread owns the cell (tid & 15, tid >> 4) and the 8 x 8 window whose top-left
//                       cell that is (windows step by 4 samples: 2 x 2 cells, the right and lower ones may be halo).  sse = SS + RR - 2 SR of the own cell;
//                       the window's quotient is taken in double from four exact integer factors and rounded to 2^-30 fixed point at once.
//                       Only integers are ever added across threads: DPP wave sums, four partials per quantity in LDS, then one 64-bit atomicAdd per
//                       quantity and workgroup into the (frame, plane) record.  The result does not depend on the order of anything.
// Loads stay inside the padded plane: a cell is read only when its first sample is inside w x h, columns come in fours and the stride is a multiple of 64.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_common.h"

namespace mi {

#define MI_Q_TILE 64                      /* samples of a tile edge */
#define MI_Q_CELLS 17                     /* 4 x 4 cells of a tile edge, halo included */
#define MI_Q_ONE 1073741824.0             /* 2^30: the fixed-point scale of one window's SSIM */

// one per (frame, plane), at records[3 * frame + plane]; zeroed before the launch
struct QualityRec { unsigned long long sse; unsigned long long ssim_sum /* two's complement */; unsigned long long ssim_windows; };

__global__ void __launch_bounds__(256) quality_kernel(const FrameDev *frames, QualityRec *records) {
  __shared__ uint32_t cell[5][MI_Q_CELLS * MI_Q_CELLS];
  __shared__ long long part[3][4];
  const FrameDev *f = frames + blockIdx.z;
  const int plane = blockIdx.y, tiles_x = f->pw / MI_Q_TILE;
  if (plane >= f->np || (int)blockIdx.x >= tiles_x * (f->ph / MI_Q_TILE) || frame_idle(f)) return;     // uniform in the workgroup
  const int w = f->w, h = f->h, stride = f->stride;
  const int x_tile = ((int)blockIdx.x % tiles_x) * MI_Q_TILE, y_tile = ((int)blockIdx.x / tiles_x) * MI_Q_TILE;
  if (x_tile >= w || y_tile >= h) return;                                                               // a tile of padding only
  const uint16_t *const src = f->src[plane], *const rec = f->enable_restoration ? f->lrp[plane] : f->fin[plane];
  const int tid = (int)threadIdx.x;
  // ---- pass 1: the cells' sums
  for (int i = tid; i < MI_Q_CELLS * MI_Q_CELLS; i += 256) {
    const int x0 = x_tile + (i % MI_Q_CELLS) * 4, y0 = y_tile + (i / MI_Q_CELLS) * 4;
    uint32_t S = 0, R = 0, SS = 0, RR = 0, SR = 0;
    if (x0 < w && y0 < h) {
      const int rows = h - y0 < 4 ? h - y0 : 4, cols = w - x0 < 4 ? w - x0 : 4;
      for (int j = 0; j < rows; j++) {
        const size_t at = (size_t)(y0 + j) * stride + x0;                                               // 8-byte aligned: planes are 256-byte aligned, x0 and the stride multiples of 4
        const uint2 a = *(const uint2 *)(src + at), b = *(const uint2 *)(rec + at);
        const uint32_t s4[4] = { a.x & 0xFFFFu, a.x >> 16, a.y & 0xFFFFu, a.y >> 16 }, r4[4] = { b.x & 0xFFFFu, b.x >> 16, b.y & 0xFFFFu, b.y >> 16 };
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t s = k < cols ? s4[k] : 0u, r = k < cols ? r4[k] : 0u;
          S += s; R += r; SS += s * s; RR += r * r; SR += s * r;
        }
      }
    }
    cell[0][i] = S; cell[1][i] = R; cell[2][i] = SS; cell[3][i] = RR; cell[4][i] = SR;
  }
  __syncthreads();
  // ---- pass 2: the own cell's squared errors, the own window's SSIM
  const int cx = tid & 15, cy = tid >> 4, at = cy * MI_Q_CELLS + cx;
  const long long sse = (long long)(cell[2][at] + cell[3][at] - 2u * cell[4][at]);
  long long ssim = 0; int windows = 0;
  if (x_tile + cx * 4 + 8 <= w && y_tile + cy * 4 + 8 <= h) {
    long long v[5];
#pragma unroll
    for (int k = 0; k < 5; k++) v[k] = (long long)cell[k][at] + cell[k][at + 1] + cell[k][at + MI_Q_CELLS] + cell[k][at + MI_Q_CELLS + 1];
    const long long S = v[0], R = v[1], SS = v[2], RR = v[3], SR = v[4];
    const long long c1 = f->bd == 8 ? 26634 : 428658, c2 = f->bd == 8 ? 239708 : 3857925;            // 4096 (0.01 peak)^2, 4096 (0.03 peak)^2
    const long long fa = 2 * S * R + c1, fb = 128 * SR - 2 * S * R + c2, fc = S * S + R * R + c1, fd = 64 * SS - S * S + 64 * RR - R * R + c2;
    const double n = (double)fa * (double)fb, m = (double)fc * (double)fd;                              // every factor is below 2^53: the conversions are exact
    const double q = n / m;
    ssim = (long long)__builtin_floor(q * MI_Q_ONE + 0.5);
    windows = 1;
  }
  // ---- integers only from here: wave sums, one partial per wave and quantity, one atomic per quantity
  const long long wave_sse = wave_sum_i64(sse), wave_ssim = wave_sum_i64(ssim);
  const int wave_windows = wave_sum_i32(windows);
  if (LANE == 0) { part[0][tid >> 6] = wave_sse; part[1][tid >> 6] = wave_ssim; part[2][tid >> 6] = wave_windows; }
  __syncthreads();
  if (tid == 0) {
    QualityRec *out = records + 3 * blockIdx.z + plane;
    atomicAdd(&out->sse, (unsigned long long)(part[0][0] + part[0][1] + part[0][2] + part[0][3]));
    atomicAdd(&out->ssim_sum, (unsigned long long)(part[1][0] + part[1][1] + part[1][2] + part[1][3]));
    atomicAdd(&out->ssim_windows, (unsigned long long)(part[2][0] + part[2][1] + part[2][2] + part[2][3]));
  }
}

}  // namespace mi
