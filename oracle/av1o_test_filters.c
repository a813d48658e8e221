/* oracle/av1o_test_filters.c -- tests only: the oracle's frame-level filter stages (av1o_deblock_search / av1o_deblock_frame, av1o_cdef_search_and_apply,
 * av1o_lr_search_and_apply) on a caller-supplied frame, so that tests/helpers/loopfilter_ref.py can be pinned by something other than the kernels it judges
 * (tests/test_loopfilter_kernels.py).  TEST INFRASTRUCTURE (see av1o.h). */
#include "av1o_int.h"

/* par = { w, h, bit depth, planes, tune_psnr, fast_deblock, enable_cdef, enable_restoration, sgr_full, ac_q[3], stages }; stages: 1 = deblock (level search on
 * rec, then the filter at the picked levels, in place), 2 = CDEF (rec -> fin), 4 = restoration (fin inside a stripe, rec across its boundaries -> lrp).
 * Planes are padded (pw x ph, pitch pw), maps mi_stride x mi_h, as Av1oFrame lays them out; m_skip holds the skip flag only.
 * Out: tally [3][2][64] and lf_level [4] (stage 1), cdef_idx [sb_rows * sb_cols] (2), lr_type / lr_set [np][units], lr_xqd [np][units][2] (4), and the
 * activity scale and variance per 8x8 cell.  Returns 0, or -1 for parameters the stages are not written for. */
int av1o_test_loop_filters(const int *par, int64_t rdmult, uint16_t *const src[3], uint16_t *const rec[3], uint16_t *const fin[3], uint16_t *const lrp[3],
                           const uint8_t *m_txsize, const uint8_t *m_bsize, const uint8_t *m_skip, int64_t *tally, int *lf_level, int8_t *cdef_idx,
                           uint32_t *act, uint32_t *svar8, uint8_t *lr_type, uint8_t *lr_set, int8_t *lr_xqd) {
  static __thread Av1oFrame f;
  memset(&f, 0, sizeof(f));
  f.w = par[0]; f.h = par[1]; f.bd = par[2]; f.np = par[3];
  if (f.w < 1 || f.h < 1 || (f.bd != 8 && f.bd != 10) || (f.np != 1 && f.np != 3)) return -1;
  f.cfg.width = f.w; f.cfg.height = f.h; f.cfg.bit_depth = f.bd; f.cfg.mono = f.np == 1;
  f.cfg.tune_psnr = par[4]; f.cfg.fast_deblock = par[5]; f.cfg.cdef = par[6]; f.cfg.lrf = par[7]; f.cfg.sgr_full = par[8];
  f.enable_cdef = par[6]; f.enable_restoration = par[7];
  for (int p = 0; p < 3; p++) { f.ac_q[p] = par[9 + p]; f.rdmult[p] = rdmult; }
  const int stages = par[12];
  f.mi_cols = 2 * ((f.w + 7) >> 3); f.mi_rows = 2 * ((f.h + 7) >> 3); f.sb_cols = (f.mi_cols + 15) >> 4; f.sb_rows = (f.mi_rows + 15) >> 4;
  f.pw = f.sb_cols * 64; f.ph = f.sb_rows * 64; f.stride = f.pw; f.mi_stride = f.pw / 4; f.mi_h = f.ph / 4;
  const size_t npx = (size_t)f.pw * f.ph, ncell = (size_t)(f.pw / 8) * (f.ph / 8);
  for (int p = 0; p < f.np; p++) { f.src[p] = src[p]; f.rec[p] = rec[p]; }
  f.m_txsize = (uint8_t *)m_txsize; f.m_bsize = (uint8_t *)m_bsize; f.m_skip = (uint8_t *)m_skip;
  f.cdef_idx = cdef_idx;
  av1o_activity(&f);
  memcpy(act, f.act, ncell * sizeof(uint32_t)); memcpy(svar8, f.svar8, ncell * sizeof(uint32_t));
  if (stages & 1) {
    int64_t t[3][2][64];
    memset(t, 0, sizeof(t));
    if (!f.cfg.fast_deblock) av1o_deblock_search(&f, t);
    memcpy(tally, t, sizeof(t));
    av1o_deblock_frame(&f);
    for (int i = 0; i < 4; i++) lf_level[i] = f.lf_level[i];
  }
  if (stages & 2) {
    for (int p = 0; p < f.np; p++) { memcpy(fin[p], rec[p], npx * 2); f.rec[p] = fin[p]; }
    av1o_cdef_search_and_apply(&f);                       /* keeps copies of the deblocked planes in f.dbk */
    for (int p = 0; p < f.np; p++) { free(f.dbk[p]); f.dbk[p] = NULL; }
  }
  if (stages & 4) {
    for (int p = 0; p < f.np; p++) { memcpy(lrp[p], fin[p], npx * 2); f.rec[p] = lrp[p]; f.dbk[p] = rec[p]; }
    av1o_lr_search_and_apply(&f);
    const int nu = f.lr_unit_cols * f.lr_unit_rows;
    for (int p = 0; p < f.np; p++) {
      memcpy(lr_type + p * nu, f.lr_type[p], (size_t)nu); memcpy(lr_set + p * nu, f.lr_set[p], (size_t)nu); memcpy(lr_xqd + p * nu * 2, f.lr_xqd[p], (size_t)nu * 2);
      free(f.lr_type[p]); free(f.lr_set[p]); free(f.lr_xqd[p]);
    }
  }
  free(f.act); free(f.svar8); free(f.svar4);
  return 0;
}
