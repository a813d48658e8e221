// dev_predict.h -- AV1 intra prediction (spec 7.11.2), one wavefront per block, edges and the
// predicted block staged in that wave's LDS region.  Square blocks, 4:4:4 / 4:0:0.
// Mirrors rav1e src/predict.rs in function (that file is not in /root/reference; the arithmetic is
// the normative AV1 prediction process).
#pragma once
#include "dev_common.h"

#define EDGE_OFF 16
#define EDGE_LEN(N) (EDGE_OFF + 2 * (N) + 16)

__device__ __forceinline__ const uint8_t *sm_weights_dev(int log2w) {
  // Sm_Weights_Tx_4x4 .. 64x64 in one array: the table of size n starts at n - 4
  static __device__ const uint8_t sw[124] = { 255, 149, 85, 64,
                                              255, 197, 146, 105, 73, 50, 37, 32,
                                              255, 225, 196, 170, 145, 123, 102, 84, 68, 54, 43, 33, 26, 20, 17, 16,
                                              255, 240, 225, 210, 196, 182, 169, 157, 145, 133, 122, 111, 101, 92, 83, 74,
                                              66, 59, 52, 45, 39, 34, 29, 25, 21, 17, 14, 12, 10, 9, 8, 8,
                                              255, 248, 240, 233, 225, 218, 210, 203, 196, 189, 182, 176, 169, 163, 156, 150,
                                              144, 138, 133, 127, 121, 116, 111, 106, 101, 96, 91, 86, 82, 77, 73, 69,
                                              65, 61, 57, 54, 50, 47, 44, 41, 38, 35, 32, 29, 27, 25, 22, 20,
                                              18, 16, 15, 13, 12, 10, 9, 8, 7, 6, 6, 5, 5, 4, 4, 4 };
  const int l = ((log2w >= 2) & (log2w <= 5)) ? log2w : 6;
  return sw + ((1 << l) - 4);
}
// The three lookups below are straight-line code on packed immediates.  Their arguments are uniform per 16-lane row, not per wave (the SATD stage predicts four angles
// per wave): as a `switch` / `if` ladder each became a divergent decision tree, walked once per distinct value among the wave's rows (profiles/k1_lookups.md).
//
// Dr_Intra_Derivative (spec 7.11.2.4).  The 27 angles that have one are a = 3 k + r with k = a / 3 distinct for each (1..29 without 11 and 26) and r a function
// of k: eight low bits of the value per k in four words, the two high bits (k = 1..4 only) and r (3: no such angle) in two-bit tables.  Every other a gives 0.
__device__ __forceinline__ int dr_deriv_dev(int a) {
  const int aa = (unsigned)a < 90u ? a : 0;
  const int k = (aa * 43) >> 7;                                      // aa / 3 for 0..89
  const unsigned long long w01 = k < 8 ? 0x97b2d7117423ff00ULL : 0x4047505a00667484ULL, w23 = k < 24 ? 0x171b1f23282d3339ULL : 0x000003070b000f13ULL;
  const unsigned long long w = k < 16 ? w01 : w23;
  const int v = lut8(w, k & 7) | ((int)((0x16cULL >> (2 * k)) & 3) << 8);
  const int r = (int)((0xf035554000eaaa03ULL >> (2 * k)) & 3);
  return aa - 3 * k == r ? v : 0;
}
// Edge filter strength (spec 7.11.2.9): the block classes w + h <= 8, 12, 16, 24, 32 and above; per class and filter type the smallest |delta| of strength 1, 2 and 3
// (255: never; a strength that a class skips has the next one's threshold), eight bits per class.
__device__ __forceinline__ int edge_strength_dev(int w, int h, int ft, int delta) {
  const int d = imin_(iabs_(delta), 254), blk = w + h;
  const int c = (blk > 8) + (blk > 12) + (blk > 16) + (blk > 24) + (blk > 32);
  const unsigned long long t1 = ft == 0 ? 0x010108282838ULL : 0x010104141428ULL, t2 = ft == 0 ? 0x010410ffffffULL : 0x010104303040ULL;
  const unsigned long long t3 = ft == 0 ? 0x012020ffffffULL : 0x010104ffffffULL;
  return (d >= lut8(t1, c)) + (d >= lut8(t2, c)) + (d >= lut8(t3, c));
}
__device__ __forceinline__ int edge_upsample_sel_dev(int w, int h, int ft, int delta) {
  const int d = iabs_(delta), blk = w + h;
  return (int)((d > 0) & (d < 40) & (blk <= (ft == 0 ? 16 : 8)));
}
// dx and dy of a directional prediction of angle pa (spec 7.11.2.4 steps 5-7: dx below 180 degrees, dy above 90; 0 where the prediction does not use one).
// dr_deriv_dev is 0 for every argument that is not a derivative's angle, a negative one included, which stands for the conditions.
__device__ __forceinline__ void dr_dxdy_dev(int pa, int *dx, int *dy) {
  *dx = dr_deriv_dev(pa < 90 ? pa : 180 - pa);
  *dy = dr_deriv_dev(pa < 180 ? pa - 90 : 270 - pa);
}
// The same for an angle the compiler knows to be wave-uniform (readlane / readfirstlane): one scalar load and a few scalar instructions, no vector register.
// Entry pa / 3 is dx | dy << 10 | (pa % 3) << 20 for the angles with a dx or dy (they lie at least 3 apart: no two share an entry), 3 << 20 for the rest.
static __device__ const uint32_t dr_dxdy_tab[91] = {
    0x300000, 0x0003ff, 0x000223, 0x000174, 0x200111, 0x2000d7, 0x2000b2, 0x200097, 0x200084, 0x200074, 0x200066, 0x300000, 0x00005a,
    0x000050, 0x000047, 0x000040, 0x000039, 0x000033, 0x00002d, 0x100028, 0x100023, 0x10001f, 0x10001b, 0x100017, 0x100013, 0x10000f,
    0x300000, 0x00000b, 0x000007, 0x000003, 0x300000, 0x0ffc03, 0x088c07, 0x05d00b, 0x24440f, 0x235c13, 0x22c817, 0x225c1b, 0x22101f,
    0x21d023, 0x219828, 0x300000, 0x01682d, 0x014033, 0x011c39, 0x010040, 0x00e447, 0x00cc50, 0x00b45a, 0x10a066, 0x108c74, 0x107c84,
    0x106c97, 0x105cb2, 0x104cd7, 0x103d11, 0x300000, 0x002d74, 0x001e23, 0x000fff, 0x300000, 0x000c00, 0x001c00, 0x002c00, 0x203c00,
    0x204c00, 0x205c00, 0x206c00, 0x207c00, 0x208c00, 0x20a000, 0x300000, 0x00b400, 0x00cc00, 0x00e400, 0x010000, 0x011c00, 0x014000,
    0x016800, 0x119800, 0x11d000, 0x121000, 0x125c00, 0x12c800, 0x135c00, 0x144400, 0x300000, 0x05d000, 0x088c00, 0x0ffc00, 0x300000 };
__device__ __forceinline__ void dr_dxdy_uni(int pa, int *dx, int *dy) {
  const int p = (unsigned)pa <= 270u ? pa : 0, k = (p * 683) >> 11;               // p / 3 for 0..270
  const uint32_t e = dr_dxdy_tab[k];
  const bool has = p - 3 * k == (int)(e >> 20);
  *dx = has ? (int)(e & 1023) : 0; *dy = has ? (int)((e >> 10) & 1023) : 0;
}

// Raw (unfiltered) edges of the block at pixel (x,y) of `plane`: above[-1..2n-1], left[-1..2n-1]. (spec 7.11.2 steps 1-4)
// In three steps, so that the head of a block search can send these loads off with its other loads (tile_search.h head_stage_*):
//   edge_addr   pure: where sample i of the above edge and of the left edge of a w x h block comes from (sample offsets into the plane); i = w + h is the
//               corner, every i beyond it the block's own first sample.  Every sample comes from one unconditional load per edge (addresses selected, not the loads): with no row above the
//               left neighbour's sample, with no neighbour at all the block's own first sample
//   (the loads: rec[ia], rec[il])
//   edge_value  the values spec 7.11.2 puts where there is no neighbour at all
struct EdgeAddr { int ia, il; };
__device__ __forceinline__ EdgeAddr edge_addr(int rs, int mi_rows, int mi_cols, int x, int y, int w, int h, int have_left, int have_above, int have_ar, int have_bl, int i) {
  const int max_x = mi_cols * 4 - 1, max_y = mi_rows * 4 - 1;
  const int lim_a = imin_(max_x, x + (have_ar ? 2 * w : w) - 1), lim_l = imin_(max_y, y + (have_bl ? 2 * h : h) - 1);
  const bool corner = i == w + h;
  EdgeAddr e;
  if (have_above) e.ia = (y - 1) * rs + (corner ? (have_left ? x - 1 : x) : imin_(lim_a, x + i));
  else e.ia = y * rs + (have_left ? x - 1 : x);
  if (have_left) e.il = imin_(lim_l, y + i) * rs + x - 1;
  else e.il = (have_above ? y - 1 : y) * rs + x;
  if (i > w + h) e.ia = e.il = y * rs + x;                       // a lane with no sample to fetch
  return e;
}
__device__ __forceinline__ void edge_value(int bd, int have_left, int have_above, bool corner, uint16_t *a, uint16_t *l) {
  if (!have_above && !have_left) { *a = (uint16_t)(corner ? (1 << (bd - 1)) : (1 << (bd - 1)) - 1); *l = (uint16_t)((1 << (bd - 1)) + 1); }
}
__device__ inline void load_edges(const LDS FrameDev *f, int plane, int x, int y, int n, int have_left, int have_above,
                                  int have_ar, int have_bl, LDS uint16_t *above /* +EDGE_OFF */, LDS uint16_t *left) {
  const int bd = f->bd, rs = f->stride, mi_rows = f->mi_rows, mi_cols = f->mi_cols;
  const uint16_t *rec = f->rec[plane];
  const int tot = 2 * n;                                        // index tot is the corner
  for (int i = LANE; i <= tot; i += 64) {
    const bool corner = i == tot;
    const EdgeAddr e = edge_addr(rs, mi_rows, mi_cols, x, y, n, n, have_left, have_above, have_ar, have_bl, i);
    uint16_t a = rec[e.ia], l = rec[e.il];
    edge_value(bd, have_left, have_above, corner, &a, &l);
    if (corner) { above[-1] = a; left[-1] = a; }
    else { above[i] = a; left[i] = l; }
  }
  WAVE_SYNC();
}

__device__ inline void edge_filter_dev(LDS uint16_t *buf, int sz, int strength, LDS uint16_t *tmp) {
  if (!strength) return;
  for (int i = LANE; i < sz; i += 64) tmp[i] = buf[i - 1];
  WAVE_SYNC();
  for (int i = 1 + LANE; i < sz; i += 64) {
    int s = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const int k = iclamp_(i - 2 + j, 0, sz - 1);
      const int kw = strength == 1 ? (j == 0 || j == 4 ? 0 : (j == 2 ? 8 : 4)) : (strength == 2 ? (j == 0 || j == 4 ? 0 : (j == 2 ? 6 : 5)) : (j == 0 || j == 4 ? 2 : 4));
      s += kw * tmp[k];
    }
    buf[i - 1] = (uint16_t)((s + 8) >> 4);
  }
  WAVE_SYNC();
}
__device__ inline void edge_upsample_dev(LDS uint16_t *buf, int num_px, int bd, LDS uint16_t *tmp) {
  // dup[0] = buf[-1]; dup[i+2] = buf[i] (i=-1..num_px-1); dup[num_px+2] = buf[num_px-1]
  for (int i = LANE; i < num_px + 3; i += 64) {
    uint16_t v;
    if (i == 0) v = buf[-1]; else if (i == num_px + 2) v = buf[num_px - 1]; else v = buf[i - 2];
    tmp[i] = v;
  }
  WAVE_SYNC();
  const int mx = (1 << bd) - 1;
  if (LANE == 0) buf[-2] = tmp[0];
  for (int i = LANE; i < num_px; i += 64) {
    int s = -(int)tmp[i] + 9 * (int)tmp[i + 1] + 9 * (int)tmp[i + 2] - (int)tmp[i + 3];
    s = iclamp_(round2_(s, 4), 0, mx);
    buf[2 * i - 1] = (uint16_t)s;
    buf[2 * i] = tmp[i + 2];
  }
  WAVE_SYNC();
}

// Predict an n x n block into pred[n*n] from raw edges. wa/wl are working copies (modified by filters).
__device__ inline void predict_block(const LDS FrameDev *f, int x, int y, int log2w, int have_left, int have_above,
                                     int mode, int angle_delta, int ftype, const LDS uint16_t *ra, const LDS uint16_t *rl,
                                     LDS uint16_t *wa, LDS uint16_t *wl, LDS uint16_t *tmp, LDS uint16_t *pred) {
  const int n = 1 << log2w, bd = f->bd, nn = n * n;
  const int max_x = f->mi_cols * 4 - 1, max_y = f->mi_rows * 4 - 1;
  if (mode == PAETH_PRED) {
    const int tl = ra[-1];
    for (int idx = LANE; idx < nn; idx += 64) {
      const int i = idx >> log2w, j = idx & (n - 1);
      const int base = ra[j] + rl[i] - tl;
      const int pl = iabs_(base - rl[i]), pt = iabs_(base - ra[j]), ptl = iabs_(base - tl);
      pred[idx] = (pl <= pt && pl <= ptl) ? rl[i] : (pt <= ptl ? ra[j] : (uint16_t)tl);
    }
  } else if (mode == DC_PRED) {
    int v;
    if (have_left || have_above) {
      int s = 0;
      for (int k = LANE; k < n; k += 64) s += (have_above ? ra[k] : 0) + (have_left ? rl[k] : 0);
      s = wave_sum_i32(s);
      if (have_left && have_above) v = (s + n) / (2 * n);
      else v = (s + (n >> 1)) >> log2w;
    } else v = 1 << (bd - 1);
    for (int idx = LANE; idx < nn; idx += 64) pred[idx] = (uint16_t)v;
  } else if (mode == SMOOTH_PRED || mode == SMOOTH_V_PRED || mode == SMOOTH_H_PRED) {
    const uint8_t *sw = sm_weights_dev(log2w);
    const int bl = rl[n - 1], tr = ra[n - 1];
    for (int idx = LANE; idx < nn; idx += 64) {
      const int i = idx >> log2w, j = idx & (n - 1);
      int p;
      if (mode == SMOOTH_PRED) p = round2_(sw[i] * ra[j] + (256 - sw[i]) * bl + sw[j] * rl[i] + (256 - sw[j]) * tr, 9);
      else if (mode == SMOOTH_V_PRED) p = round2_(sw[i] * ra[j] + (256 - sw[i]) * bl, 8);
      else p = round2_(sw[j] * rl[i] + (256 - sw[j]) * tr, 8);
      pred[idx] = (uint16_t)p;
    }
  } else {
    const int pa = mode_angle_of(mode) + angle_delta * 3;
    // working copies of the edges
    for (int i = LANE; i < 2 * n + 1; i += 64) { wa[i - 1] = ra[i - 1]; wl[i - 1] = rl[i - 1]; }
    WAVE_SYNC();
    int up_a = 0, up_l = 0;
    if (pa != 90 && pa != 180) {
      if (pa > 90 && pa < 180 && 2 * n >= 24) {
        if (LANE == 0) { const int v = round2_(wl[0] * 5 + wa[-1] * 6 + wa[0] * 5, 4); wa[-1] = (uint16_t)v; wl[-1] = (uint16_t)v; }
        WAVE_SYNC();
      }
      if (have_above) {
        const int st = edge_strength_dev(n, n, ftype, pa - 90);
        const int num = imin_(n, max_x - x + 1) + (pa < 90 ? n : 0) + 1;
        edge_filter_dev(wa, num, st, tmp);
      }
      if (have_left) {
        const int st = edge_strength_dev(n, n, ftype, pa - 180);
        const int num = imin_(n, max_y - y + 1) + (pa > 180 ? n : 0) + 1;
        edge_filter_dev(wl, num, st, tmp);
      }
    }
    up_a = edge_upsample_sel_dev(n, n, ftype, pa - 90);
    if (up_a) edge_upsample_dev(wa, n + (pa < 90 ? n : 0), bd, tmp);
    up_l = edge_upsample_sel_dev(n, n, ftype, pa - 180);
    if (up_l) edge_upsample_dev(wl, n + (pa > 180 ? n : 0), bd, tmp);
    int dx, dy;
    dr_dxdy_dev(pa, &dx, &dy);
    for (int idx = LANE; idx < nn; idx += 64) {
      const int i = idx >> log2w, j = idx & (n - 1);
      int v;
      if (pa < 90) {
        const int max_base = (2 * n - 1) << up_a;
        const int id = (i + 1) * dx, base = (id >> (6 - up_a)) + (j << up_a), sh = ((id << up_a) >> 1) & 0x1F;
        v = base < max_base ? round2_(wa[base] * (32 - sh) + wa[base + 1] * sh, 5) : wa[max_base];
      } else if (pa > 90 && pa < 180) {
        int id = (j << 6) - (i + 1) * dx, base = id >> (6 - up_a);
        if (base >= -(1 << up_a)) { const int sh = ((id << up_a) >> 1) & 0x1F; v = round2_(wa[base] * (32 - sh) + wa[base + 1] * sh, 5); }
        else { id = (i << 6) - (j + 1) * dy; base = id >> (6 - up_l); const int sh = ((id << up_l) >> 1) & 0x1F; v = round2_(wl[base] * (32 - sh) + wl[base + 1] * sh, 5); }
      } else if (pa > 180) {
        const int id = (j + 1) * dy, base = (id >> (6 - up_l)) + (i << up_l), sh = ((id << up_l) >> 1) & 0x1F;
        v = round2_(wl[base] * (32 - sh) + wl[base + 1] * sh, 5);
      } else if (pa == 90) v = wa[j];
      else v = wl[i];
      pred[idx] = (uint16_t)v;
    }
  }
  WAVE_SYNC();
}

// spec 7.11.5 (4:4:4): pred holds the DC prediction on entry; luma reconstruction read from f->rec[0].
__device__ inline void predict_cfl_dev(const LDS FrameDev *f, int x, int y, int log2w, int alpha, const LDS uint16_t *dcp, LDS uint16_t *out) {
  const int n = 1 << log2w, nn = n * n, mx = (1 << f->bd) - 1, rs = f->stride;
  const uint16_t *luma = f->rec[0] + y * rs + x;
  int s = 0;
  for (int idx = LANE; idx < nn; idx += 64) s += luma[(idx >> log2w) * rs + (idx & (n - 1))] << 3;
  s = wave_sum_i32(s);
  const int avg = round2_(s, 2 * log2w);
  for (int idx = LANE; idx < nn; idx += 64) {
    const int l = (luma[(idx >> log2w) * rs + (idx & (n - 1))] << 3) - avg;
    const int v = alpha * l;
    const int sc = v >= 0 ? round2_(v, 6) : -round2_(-v, 6);
    out[idx] = (uint16_t)iclamp_(dcp[idx] + sc, 0, mx);
  }
  WAVE_SYNC();
}
