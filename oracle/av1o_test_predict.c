/* oracle/av1o_test_predict.c -- tests only: the oracle's intra prediction (av1o_predict_intra_wh), chroma from luma (av1o_predict_cfl_wh) and the search's
 * block distortions (the SATD and SSE of av1o_search.c) on caller-supplied planes and blocks, so that tests/helpers/predict_ref.py can be pinned by something
 * other than the kernels it judges (tests/test_predict_kernels.py).  TEST INFRASTRUCTURE (see av1o.h). */
#include "av1o_int.h"

/* par = { w, h, bit depth, x, y, log2 width, log2 height, have_left, have_above, have_above_rt, have_below_lft, mode, angle_delta, filter_type, cfl, alpha }.
 * luma / plane: padded planes (pw x ph, pitch pw) as Av1oFrame lays them out; the edges are read from `plane`.  With cfl != 0 the block is the DC prediction of
 * `plane` plus the scaled luma of `luma` (mode and angle_delta are ignored).  dst: the block, pitch 1 << log2 width.  Returns 0, or -1 for a block that does
 * not lie in the picture or that claims a neighbour the planes do not have. */
int av1o_test_predict(const int *par, const uint16_t *luma, const uint16_t *plane, uint16_t *dst) {
  static __thread Av1oFrame f;
  memset(&f, 0, sizeof(f));
  f.w = par[0]; f.h = par[1]; f.bd = par[2]; f.np = 3;
  if (f.w < 1 || f.h < 1 || (f.bd != 8 && f.bd != 10)) return -1;
  f.mi_cols = 2 * ((f.w + 7) >> 3); f.mi_rows = 2 * ((f.h + 7) >> 3); f.sb_cols = (f.mi_cols + 15) >> 4; f.sb_rows = (f.mi_rows + 15) >> 4;
  f.pw = f.sb_cols * 64; f.ph = f.sb_rows * 64; f.stride = f.pw; f.mi_stride = f.pw / 4; f.mi_h = f.ph / 4;
  f.rec[0] = (uint16_t *)luma; f.rec[1] = (uint16_t *)plane; f.rec[2] = (uint16_t *)plane;
  const int x = par[3], y = par[4], wl = par[5], hl = par[6], have_left = par[7], have_above = par[8], have_ar = par[9], have_bl = par[10];
  if (wl < 2 || wl > 6 || hl < 2 || hl > 6 || x < 0 || y < 0 || x >= f.mi_cols * MI || y >= f.mi_rows * MI || x + (1 << wl) > f.pw || y + (1 << hl) > f.ph) return -1;
  if ((have_above && y == 0) || (have_left && x == 0) || (have_ar && !have_above) || (have_bl && !have_left)) return -1;
  const int cfl = par[14];
  av1o_predict_intra_wh(&f, NULL, 1, x, y, wl, hl, have_left, have_above, have_ar, have_bl, cfl ? DC_PRED : par[11], cfl ? 0 : par[12], par[13], dst, 1 << wl);
  if (cfl) av1o_predict_cfl_wh(&f, 1, x, y, wl, hl, par[15], dst, 1 << wl);
  return 0;
}

/* what: 0 = the search's SATD of a w x h block (both blocks with pitch w), 1 = its SSE */
int64_t av1o_test_distortion(const uint16_t *src, const uint16_t *pred, int w, int h, int what) {
  return what == 0 ? av1o_satd_block_wh(src, w, pred, w, w, h) : av1o_sse_block_wh(src, w, pred, w, w, h);
}

/* The psychovisual luma distortion (av1o_psy_dist_luma) of the n x n reconstruction `rec` against the source block `src` (both with pitch n), the block at the
 * origin of a 64 x 64 picture whose activity is computed as for any frame.  sv / act: the variance and the activity scale of the block's cells in raster order
 * (one 4x4 cell for n = 4, 8x8 cells otherwise), as the tile search is handed them.  Returns the distortion, or -1 for a size it is not written for. */
int64_t av1o_test_psy_dist(const uint16_t *src, const uint16_t *rec, int n, int bd, uint32_t *sv, uint32_t *act) {
  static __thread Av1oFrame f;
  static __thread uint16_t plane[64 * 64];
  if ((n != 4 && n != 8 && n != 16 && n != 32 && n != 64) || (bd != 8 && bd != 10)) return -1;
  memset(&f, 0, sizeof(f));
  f.w = f.h = 64; f.bd = bd; f.np = 1; f.mi_cols = f.mi_rows = 16; f.sb_cols = f.sb_rows = 1; f.pw = f.ph = f.stride = 64; f.mi_stride = f.mi_h = 16;
  memset(plane, 0, sizeof(plane));
  for (int i = 0; i < n; i++) memcpy(plane + i * 64, src + i * n, (size_t)n * 2);
  f.src[0] = plane;
  av1o_activity(&f);
  const int64_t d = av1o_psy_dist_luma(&f, rec, n, 0, 0, n);
  if (n == 4) { sv[0] = f.svar4[0]; act[0] = f.act[0]; }
  else for (int cy = 0; cy < n / 8; cy++) for (int cx = 0; cx < n / 8; cx++) { sv[cy * (n / 8) + cx] = f.svar8[cy * 8 + cx]; act[cy * (n / 8) + cx] = f.act[cy * 8 + cx]; }
  free(f.act); free(f.svar8); free(f.svar4);
  return d;
}
