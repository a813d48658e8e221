// dev_orient.h -- EXIF orientation on input: pictures of sw x sh pixels in device memory -> slots of w x h, turned and mirrored as tag 0x0112 asks.
// S[row][column] the source, D[y][x] the slot:
//   o   D[y][x] =              slot is          o   D[y][x] =              slot is
//   1   S[y][x]                sw x sh          5   S[x][y]                sh x sw
//   2   S[y][sw-1-x]           sw x sh          6   S[sh-1-x][y]           sh x sw
//   3   S[sh-1-y][sw-1-x]      sw x sh          7   S[sh-1-x][sw-1-y]      sh x sw
//   4   S[sh-1-y][x]           sw x sh          8   S[x][sw-1-y]           sh x sw
// (Pillow's ImageOps.exif_transpose; tests/test_orient_reference.py).  A pure permutation of pixels: the slot's bytes are specified exactly.
//   orient_kernel<DC, T>   T = uint8_t: sources described by an IngestSrc (HWC / CHW, any strides, 3 or 4 channels; 3 into an RGBA slot: alpha 255) -> 8-bit slots;
//                          T = uint16_t: packed 16-bit pictures (HWC, the deep slot's samples; 3 into an RGBA slot: A = 65535) -> deep slots.  Orientations 2..8;
//                          orientation 1 is the plain upload of the source's kind and never comes here.
// One path for all seven.  A workgroup of 256 threads owns a tile of MI_ORIENT_TILE x MI_ORIENT_TILE slot pixels, the tiles lie on the slot's grid: grid
// (ceil(w / 64), ceil(h / 64), images).  The tile's pixels are a rectangle of the source.  Load: the row groups of dev_slot.h over that rectangle -- a thread reads
// four adjacent pixels of a source row (ingest_load4 / slot16_load4: one 16-byte load where the source is packed RGBA and aligned for it), 16 threads a row of the
// rectangle, a wavefront four rows -- into LDS, one dword per pixel.  Barrier.  Store: the same row groups over the tile -- a thread gathers the four adjacent slot
// pixels of its group from LDS and writes them with slot_store4 / slot16_store4, a wavefront four slot rows of 256 bytes (RGBA).  Neither the global reads nor
// the global writes have adjacent lanes a row stride apart, whichever way the picture is turned; the tiles lie on the slot's grid so that the stores are the
// aligned ones (a mirrored source rectangle starts where sw leaves it, and its loads take the width their addresses allow, per thread).
//
// LDS layout.  Pixel (r, c) of the rectangle, r its source row and c its source column, lies at dword
//     orient_lds_at(r, c) = r * 64 + ((c + 2 * (r >> 2) + (r & 3)) & 63)
// -- rows of 64 dwords, no padding, each row rotated by 2 * (r >> 2) + (r & 3).  Banks of ds_read_b32 / ds_write_b32 are (dword address) mod 32, a wave64 access
// is served in its two halves of 32 lanes (MI355X: 64 banks of 4 bytes; 4-byte accesses see them mod 32).
//   transposed read (5..8): a half wave is 16 groups j = 0..15 of two adjacent slot rows; for its k-th pixel a lane reads r = 4 j + k (or B - 4 j - k, mirrored)
//     and c = c0 or c0 + 1.  With a plain pitch P the banks are (4 j + k) P + c: 4 j P mod 32 takes 8 values whatever P is, so four pixels a lane make any pitch
//     2-way (an odd pitch is conflict-free only for one pixel a lane, r = lane).  The rotation's 2 * (r >> 2) = 2 j (or const - 2 j) gives the 16 groups the 16
//     even banks, (r & 3) is the same for all of them, and the second slot row takes the odd ones: 32 lanes, 32 banks, no conflict.
//   row-wise accesses (the load's writes; the reads of 2..4): 16 lanes of a row at c = 4 j + k cover 8 banks twice, the half wave's other row is rotated by one
//     more or one less and takes 8 other banks: 2-way.  On ds_write_b32 that is free (its 4 cycles are the transfer of address and data, the array needs 2 + 2).
// Deep pixels are 8 bytes: two such planes of dwords ({ r | g << 16 }, { b | a << 16 }), each accessed as above, so the same rotation serves.  (One plane of 8-byte
// pixels read with ds_read_b64 would be conflict-free as well -- banks mod 64 dwords = 32 pixels -- but ds_write_b64 is served in groups of 16 lanes over 32 banks =
// 16 pixels, where a row group's stride of four pixels is 4-way.)  LDS: 16 KiB (8-bit), 32 KiB (deep); no scratch (profiles/orient_input.md has the compiler's report).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_slot.h"
#include "dev_ingest.h"

namespace mi {

constexpr uint32_t MI_ORIENT_TILE = 64, MI_ORIENT_THREADS = 256;

__device__ __forceinline__ uint32_t orient_lds_at(const uint32_t r, const uint32_t c) { return r * MI_ORIENT_TILE + ((c + 2 * (r >> 2) + (r & 3)) & (MI_ORIENT_TILE - 1)); }

// s: the source pictures (s.w x s.h = sw x sh; T = uint16_t: packed HWC, strides in bytes); o = 2..8; slots = slot (deep slot) of the first image, of the oriented size
template <int DC, class T> __global__ void __launch_bounds__(MI_ORIENT_THREADS) orient_kernel(const IngestSrc s, const int o, T *slots) {
  constexpr bool DEEP = sizeof(T) == 2;
  constexpr uint32_t TILE = MI_ORIENT_TILE;
  __shared__ uint32_t tile[(DEEP ? 2 : 1) * TILE * TILE];
  const bool turn = o >= 5, flip_r = o == 3 || o == 4 || o == 6 || o == 7, flip_c = o == 2 || o == 3 || o == 7 || o == 8;
  const uint32_t w = turn ? s.h : s.w, h = turn ? s.w : s.h;               // the slot
  const uint32_t x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE, img = blockIdx.z;
  const uint32_t nx = w - x0 < TILE ? w - x0 : TILE, ny = h - y0 < TILE ? h - y0 : TILE;      // the tile: nx x ny slot pixels (the grid leaves no empty tile)
  // its source rectangle: nr rows from r0 on, nc columns from c0 on
  const uint32_t nr = turn ? nx : ny, nc = turn ? ny : nx;
  const uint32_t r0 = flip_r ? s.h - (turn ? x0 : y0) - nr : (turn ? x0 : y0), c0 = flip_c ? s.w - (turn ? y0 : x0) - nc : (turn ? y0 : x0);
  const uint32_t g4 = (threadIdx.x & 15) * 4, line = threadIdx.x >> 4;    // this thread's group of four pixels in a line of 64, and its line of every 16

  const uint8_t *const image = s.base + (size_t)img * s.image_stride;
#pragma unroll
  for (uint32_t r = line; r < TILE; r += MI_ORIENT_THREADS / 16) {
    if (r >= nr || g4 >= nc) continue;
    const uint32_t n = nc - g4 < 4 ? nc - g4 : 4;
    const uint8_t *const row = image + (size_t)(r0 + r) * s.row_stride;
    if (DEEP) {
      uint2 px[4];
      const uint16_t *const p = (const uint16_t *)(row + (size_t)(c0 + g4) * s.inner_stride);
      if (s.channels == 4) slot16_load4<4>(p, px, n); else slot16_load4<3>(p, px, n);
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) if (k < n) { tile[orient_lds_at(r, g4 + k)] = px[k].x; tile[TILE * TILE + orient_lds_at(r, g4 + k)] = s.channels == 4 ? px[k].y : px[k].y | 0xFFFF0000u; }
    } else {
      uint32_t px[4];
      ingest_load4(s, row, c0 + g4, n, px);
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) if (k < n) tile[orient_lds_at(r, g4 + k)] = px[k];
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t y = line; y < TILE; y += MI_ORIENT_THREADS / 16) {
    if (y >= ny || g4 >= nx) continue;
    const uint32_t n = nx - g4 < 4 ? nx - g4 : 4;
    uint32_t lo[4] = { 0, 0, 0, 0 }, hi[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) if (k < n) {
      const uint32_t x = g4 + k, u = turn ? x : y, v = turn ? y : x;       // u picks the source row, v the source column
      const uint32_t at = orient_lds_at(flip_r ? nr - 1 - u : u, flip_c ? nc - 1 - v : v);
      lo[k] = tile[at];
      if (DEEP) hi[k] = tile[TILE * TILE + at];
    }
    T *const dst = slots + (((size_t)img * h + y0 + y) * w + x0 + g4) * DC;
    if constexpr (DEEP) {
      uint2 px[4];
#pragma unroll
      for (int k = 0; k < 4; k++) { px[k].x = lo[k]; px[k].y = hi[k]; }
      slot16_store4<DC>(dst, px, n);
    } else slot_store4<DC>(dst, lo, n);
  }
}

}  // namespace mi
