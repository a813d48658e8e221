// dev_png.h -- the device half of the PNG input side: inflated scanlines (png_reader.h: png_read_scanlines) -> RGBA8 / RGB8 in a batch's input slot, two kernels.
//   png_unfilter_kernel  the five scanline filters, in place.  Byte i of row y needs a = row[y][i - bpp], b = row[y - 1][i], c = row[y - 1][i - bpp]: a 2-D
//                        recurrence (Average and Paeth), run as a skewed wavefront.  One workgroup = one pass of one image (the grid runs over the pass
//                        descriptors of all images of a call), one wavefront = a band of 64 rows, one lane = one row; at step t lane r handles the whole
//                        pixel (bpp bytes) t - r, so a is the lane's own previous output, b the previous output of the lane above (one cross-lane move per
//                        dword) and c the lane's previous b.  The filter type is per lane: all five predictors are computed and one is selected.
//                        Bands run as a pipeline: a wavefront works in skewed tiles of MI_PNG_CHUNK columns, tile (band j, chunk c) in time slot 2j + c, a
//                        workgroup barrier between slots.  Row 0 of a band takes b from the last row of the band above, which that band finished one slot
//                        earlier: the tile's 64 boundary pixels are read back from the scanline buffer (the workgroup's own stores, ordered by the barrier)
//                        one per lane at the start of the tile and handed to lane 0 step by step with v_readlane.  Pictures taller than the workgroup's
//                        rows loop over groups of bands inside the same workgroup the same way.  No waiting on another workgroup.
//                        Lane = row would make every global access of the recurrence touch 64 cache lines (measured: 9.9 ms for 32 1080p RGB files, bound
//                        by the address path), so the bytes pass through an LDS tile per wavefront: four (two) pixels of each of the 64 rows are fetched
//                        with the lanes running along the rows, one sub-tile ahead of the steps that use them, and go back the same way.
//   png_expand_kernel    unfiltered scanlines -> slot: every colour type and bit depth, MSB-first sub-byte samples, gray scaled s * 255 / max, the high
//                        byte of 16-bit samples, the tRNS colour key compared on all 16 bits, palette + tRNS through a 256-entry table, Adam7 (the output
//                        pixel picks its pass from (x & 7, y & 7): png_pass_row).  The arithmetic is png_expand_rgba's (png_reader.h).  In the row groups
//                        of dev_slot.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_slot.h"

namespace mi {

#define MI_PNG_WAVES 16                   /* bands a workgroup runs at once: 1024 rows */
#define MI_PNG_CHUNK 64                   /* columns (pixels) of a skewed tile = steps between two workgroup barriers */

struct PngPassDev { unsigned long long off; uint32_t rows, rowbytes, bpp, pad; };      // off: of the pass's first filter byte in the scanline buffer
struct PngImageDev {
  unsigned long long pass_off[7];         // of each Adam7 pass ([0] alone for a non-interlaced file); unused for passes without pixels
  unsigned long long palette_off;         // 256 x uint32 r | g << 8 | b << 16 | a << 24 (colour type 3)
  uint32_t pass_rowbytes[7];
  uint32_t depth, ctype, interlace, has_key;
  uint32_t key[3], pad;
};

// byte q of a pixel kept in two dwords
__device__ __forceinline__ int png_byte(const uint32_t p[2], const int q) { return (int)((p[q >> 2] >> (8 * (q & 3))) & 255u); }

template <int BPP> __device__ __forceinline__ void png_load_pixel(const uint8_t *p, uint32_t out[2]) {
  out[0] = 0; out[1] = 0;
#pragma unroll
  for (int q = 0; q < BPP; q++) out[q >> 2] |= (uint32_t)p[q] << (8 * (q & 3));
}

// A wavefront's staging in LDS: four (two, for pixels wider than four bytes) pixels of each of its 64 rows, a pixel in a 4- or 8-byte slot, rows 5
// dwords apart (odd: the lanes' per-step dword accesses fall on 32 different banks).  Lane = row would make every global access touch 64 cache lines, so the bytes go
// through this tile instead: a sub-tile's bytes are fetched and written back with the lanes running along the rows.
#define MI_PNG_PITCH 20
#define MI_PNG_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

template <int BPP> __device__ void png_unfilter_pass(uint8_t *data, const uint32_t rows, const uint32_t rowbytes, const uint32_t nwaves, uint32_t *wg_tiles) {
  constexpr int T = BPP > 4 ? 2 : 4;                                               // pixels of a sub-tile
  constexpr int SLOT = BPP > 4 ? 8 : 4;                                            // LDS bytes of a pixel
  constexpr int SEG = T * BPP;                                                     // bytes of one row in a sub-tile: 4, 8, 12 or 16
  constexpr int G = SEG <= 4 ? 4 : SEG <= 8 ? 8 : 16;                              // lanes that run along a row; 64 / G rows per access
  constexpr int RPI = 64 / G;
  const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));     // uniform: what hangs on it stays in scalar registers
  uint32_t *const tile32 = wg_tiles + wave * (64 * MI_PNG_PITCH / 4);
  uint8_t *const tile8 = (uint8_t *)tile32;
  const uint32_t W = rowbytes / BPP;                                               // pixels (filter units) of a row
  const uint32_t nchunks = (W + 63 + MI_PNG_CHUNK - 1) / MI_PNG_CHUNK;             // the last lane of a band ends 63 columns after the first
  const uint32_t nbands = (rows + 63) / 64;
  const size_t stride = (size_t)rowbytes + 1;
  // this lane in the accesses that run along the rows: byte cb of the segment of row it * RPI + crow, it = 0 .. G - 1
  // Its address is the band's first pixel (uniform) plus a 32-bit offset (a band is at most 64 rows of 512 KiB), its pixel x0 + cdx - it * RPI.
  const uint32_t cb = lane % G, crow = lane / G, cpx = cb / BPP;
  const uint32_t clds = crow * MI_PNG_PITCH + cpx * SLOT + cb % BPP;
  const uint32_t kstride = rowbytes + 1 - BPP, kstep = RPI * kstride;              // one row down and one pixel back; from one access to the next
  const uint32_t coff = crow * kstride + cb;
  const int cdx = (int)cpx - (int)crow;
  const bool cuse = cb < (uint32_t)SEG;
  for (uint32_t g0 = 0; g0 < nbands; g0 += nwaves) {
    const uint32_t gb = nbands - g0 < nwaves ? nbands - g0 : nwaves;                // bands of this group
    const uint32_t band = g0 + wave, y = band * 64 + lane;
    const bool row_ok = wave < gb && y < rows;
    const int ft = row_ok ? (int)data[(size_t)y * stride] : 0;
    const uint32_t band_rows = wave < gb ? (rows - band * 64 < 64 ? rows - band * 64 : 64) : 0;
    uint8_t *const band0 = data + (size_t)(wave < gb ? band * 64 : 0) * stride + 1;  // the first pixel of the band's first row
    const uint8_t *const above = data + (size_t)(band > 0 && wave < gb ? band * 64 - 1 : 0) * stride + 1;     // the row over the band's first
    uint32_t out[2] = { 0, 0 }, cc[2] = { 0, 0 };                                  // the lane's previous output (a), its previous b (c)
    const uint32_t nslots = 2 * (gb - 1) + nchunks;
    for (uint32_t slot = 0; slot < nslots; slot++) {
      const int c = (int)slot - 2 * (int)wave;
      if (wave < gb && c >= 0 && c < (int)nchunks) {                               // wave-uniform
        uint32_t bd[2] = { 0, 0 };
        { const uint32_t bx = (uint32_t)c * MI_PNG_CHUNK + lane; if (band > 0 && bx < W) png_load_pixel<BPP>(above + (size_t)bx * BPP, bd); }
        uint32_t nxt[G];
        // the bytes of sub-tile u: row r holds pixels x0 - r .. x0 - r + T - 1, x0 = 64 c + T u
        auto fetch = [&](const int u) {
          const int x0 = c * MI_PNG_CHUNK + u * T;
          uint32_t vo = coff + (uint32_t)x0 * BPP;
          const int xl = x0 + cdx;
#pragma unroll
          for (int it = 0; it < G; it++, vo += kstep) {
            nxt[it] = 0;
            if (cuse && (int)crow < (int)band_rows - it * RPI && (uint32_t)(xl - it * RPI) < W) nxt[it] = band0[vo];
          }
        };
        fetch(0);
#pragma unroll 1
        for (int u = 0; u < MI_PNG_CHUNK / T; u++) {
          if (cuse) {
#pragma unroll
            for (int it = 0; it < G; it++) tile8[it * RPI * MI_PNG_PITCH + clds] = (uint8_t)nxt[it];
          }
          MI_PNG_WAVE_SYNC();
          if (u + 1 < MI_PNG_CHUNK / T) fetch(u + 1);                              // in flight while this sub-tile's steps run
#pragma unroll
          for (int j = 0; j < T; j++) {
            const int s = u * T + j, x = c * MI_PNG_CHUNK + s - (int)lane;         // the lane's pixel at step s
            uint32_t raw[2], b[2];
            raw[0] = tile32[lane * (MI_PNG_PITCH / 4) + j * (SLOT / 4)];
            raw[1] = BPP > 4 ? tile32[lane * (MI_PNG_PITCH / 4) + j * (SLOT / 4) + 1] : 0u;
            // b: the previous output of the lane above; for the band's first row, the boundary pixel of this step
            b[0] = (uint32_t)__shfl((int)out[0], (int)((lane + 63) & 63));
            b[1] = BPP > 4 ? (uint32_t)__shfl((int)out[1], (int)((lane + 63) & 63)) : 0u;
            const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)bd[0], s), e1 = BPP > 4 ? (uint32_t)__builtin_amdgcn_readlane((int)bd[1], s) : 0u;
            if (lane == 0) { b[0] = e0; b[1] = e1; }
            uint32_t o[2] = { 0, 0 };
#pragma unroll
            for (int q = 0; q < BPP; q++) {
              const int av = png_byte(out, q), bv = png_byte(b, q), cv = png_byte(cc, q);
              const int p = av + bv - cv;
              const int pa = p > av ? p - av : av - p, pb = p > bv ? p - bv : bv - p, pc = p > cv ? p - cv : cv - p;
              const int paeth = (pa <= pb && pa <= pc) ? av : (pb <= pc ? bv : cv);
              const int add = ft == 1 ? av : ft == 2 ? bv : ft == 3 ? (av + bv) >> 1 : ft == 4 ? paeth : 0;
              o[q >> 2] |= (uint32_t)((png_byte(raw, q) + add) & 255) << (8 * (q & 3));
            }
            if (row_ok && x >= 0 && x < (int)W) {
              out[0] = o[0]; out[1] = o[1]; cc[0] = b[0]; cc[1] = b[1];
              tile32[lane * (MI_PNG_PITCH / 4) + j * (SLOT / 4)] = o[0];
              if (BPP > 4) tile32[lane * (MI_PNG_PITCH / 4) + j * (SLOT / 4) + 1] = o[1];
            }
          }
          MI_PNG_WAVE_SYNC();
          {                                                                        // the sub-tile goes back, the lanes along the rows again
            const int x0 = c * MI_PNG_CHUNK + u * T;
            uint32_t vo = coff + (uint32_t)x0 * BPP;
            const int xl = x0 + cdx;
#pragma unroll
            for (int it = 0; it < G; it++, vo += kstep) {
              if (cuse && (int)crow < (int)band_rows - it * RPI && (uint32_t)(xl - it * RPI) < W) band0[vo] = tile8[it * RPI * MI_PNG_PITCH + clds];
            }
          }
          MI_PNG_WAVE_SYNC();                                                      // before the next sub-tile's bytes overwrite the tile
        }
      }
      __syncthreads();                                                             // the band below reads this tile's last row in the next slot
    }
  }
}

// grid: one workgroup per pass descriptor; block: 64 * min(MI_PNG_WAVES, bands of the tallest pass)
__global__ void __launch_bounds__(64 * MI_PNG_WAVES) png_unfilter_kernel(uint8_t *buf, const PngPassDev *passes) {
  const PngPassDev d = passes[blockIdx.x];
  uint8_t *data = buf + d.off;
  const uint32_t nwaves = blockDim.x >> 6;
  __shared__ uint32_t tiles[MI_PNG_WAVES * 64 * MI_PNG_PITCH / 4];                 // 20 KiB: a 64-row staging tile per wavefront
  switch (d.bpp) {                                                                 // workgroup-uniform
    case 1: png_unfilter_pass<1>(data, d.rows, d.rowbytes, nwaves, tiles); break;
    case 2: png_unfilter_pass<2>(data, d.rows, d.rowbytes, nwaves, tiles); break;
    case 3: png_unfilter_pass<3>(data, d.rows, d.rowbytes, nwaves, tiles); break;
    case 4: png_unfilter_pass<4>(data, d.rows, d.rowbytes, nwaves, tiles); break;
    case 6: png_unfilter_pass<6>(data, d.rows, d.rowbytes, nwaves, tiles); break;
    default: png_unfilter_pass<8>(data, d.rows, d.rowbytes, nwaves, tiles); break;
  }
}

// the first sample byte of the row that holds pixel (x, y) in its Adam7 pass (the only pass of a non-interlaced file), and in xx the pixel's column within that pass
__device__ __forceinline__ const uint8_t *png_pass_row(const uint8_t *buf, const PngImageDev &im, const uint32_t x, const uint32_t y, uint32_t &xx) {
  uint32_t p = 0, yy = y;
  xx = x;
  if (im.interlace) {
    p = (y & 1) ? 6 : (x & 1) ? 5 : (y & 2) ? 4 : (x & 2) ? 3 : (y & 4) ? 2 : (x & 4) ? 1 : 0;
    // per pass: x0 = 0 4 0 2 0 1 0, y0 = 0 0 4 0 2 0 1, dx = 8 8 4 4 2 2 1, dy = 8 8 8 4 4 2 2 (a nibble each)
    xx = (x - ((0x0102040u >> (4 * p)) & 15u)) >> ((0x0112233u >> (4 * p)) & 15u);
    yy = (y - ((0x1020400u >> (4 * p)) & 15u)) >> ((0x1122333u >> (4 * p)) & 15u);
  }
  return buf + im.pass_off[p] + (size_t)yy * ((size_t)im.pass_rowbytes[p] + 1) + 1;
}

// pixel (x, y) of the picture as r | g << 8 | b << 16 | a << 24
__device__ __forceinline__ uint32_t png_pixel(const uint8_t *buf, const PngImageDev &im, const uint32_t x, const uint32_t y) {
  uint32_t xx;
  const uint8_t *row = png_pass_row(buf, im, x, y, xx);
  const uint32_t depth = im.depth, ctype = im.ctype;
  const uint32_t channels = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : 4;
  const uint32_t mx = (1u << (depth > 8 ? 8 : depth)) - 1;
  uint32_t s[4] = { 0, 0, 0, 0 }, key16[4] = { 0, 0, 0, 0 };
#pragma unroll
  for (uint32_t c = 0; c < 4; c++) if (c < channels) {
    const size_t bit = ((size_t)xx * channels + c) * depth;
    const uint32_t v = row[bit >> 3];
    if (depth == 8) s[c] = v;
    else if (depth == 16) { s[c] = v; key16[c] = (v << 8) | row[(bit >> 3) + 1]; }
    else s[c] = (v >> (8 - depth - (uint32_t)(bit & 7))) & mx;
  }
  uint32_t r, g, b, a = 255;
  if (ctype == 3) return ((const uint32_t *)(buf + im.palette_off))[s[0]];
  if (ctype == 0 || ctype == 4) {
    r = g = b = depth < 8 ? s[0] * 255 / mx : s[0];
    if (ctype == 4) a = s[1];
    else if (im.has_key && (depth == 16 ? key16[0] : s[0]) == im.key[0]) a = 0;
  } else {
    r = s[0]; g = s[1]; b = s[2];
    if (ctype == 6) a = s[3];
    else if (im.has_key) {
      bool eq = true;
#pragma unroll
      for (int c = 0; c < 3; c++) eq = eq && ((depth == 16 ? key16[c] : s[c]) == im.key[c]);
      if (eq) a = 0;
    }
  }
  return r | (g << 8) | (b << 16) | (a << 24);
}

// slots = slot of the first image
template <int DC> __global__ void __launch_bounds__(64) png_expand_kernel(const uint8_t *buf, const PngImageDev *imgs, const uint32_t w, const uint32_t h, uint8_t *slots) {
  RowGroup4 g;
  if (!row_group4(w, h, g)) return;
  const PngImageDev &im = imgs[g.img];
  uint32_t px[4] = { 0, 0, 0, 0 };
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) if (k < g.n) px[k] = png_pixel(buf, im, g.x0 + k, g.y);
  slot_store4<DC>(slot_ptr<DC>(slots, w, h, g), px, g.n);
}

}  // namespace mi
