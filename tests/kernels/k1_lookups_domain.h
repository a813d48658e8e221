// k1_lookups_domain.h -- TEST INFRASTRUCTURE: the whole domain of the tile search's branch-free lookups as one numbered list of arguments, shared by the
// stand-alone CPU program (k1_lookups_main.cpp: the new forms against restatements of the earlier switch / if forms, exhaustively) and the GPU harness
// (k1_lookups_harness.hip: the new forms, one argument per lane).  Consecutive numbers differ in the argument that the earlier forms branched on, so the
// lanes of a 16-lane row, and the rows of a wave, all hold different arguments.
#pragma once
#include "../../cavif_rs_amd/csrc/dev_predict.h"

#ifdef __HIPCC__
#define K1L_FN __host__ __device__ inline
#else
#define K1L_FN inline
#endif

enum { K1L_DERIV = 0, K1L_STRENGTH, K1L_UPSAMPLE, K1L_DXDY_ROW, K1L_DXDY_ANGLE, K1L_DXDY_UNI_ROW, K1L_DXDY_UNI_ANGLE, K1L_TXSYM, K1L_SMW, K1L_OPS };
// DERIV: angles -10..280.  STRENGTH / UPSAMPLE: (w, h) in {4, 8, 16, 32, 64}^2 x filter type 0 / 1 x delta -135..135.  DXDY_ROW: the row's (dx, dy) for every
// directional mode x angle delta -3..3; DXDY_ANGLE: for every angle -10..280; DXDY_UNI_*: the same two lists through the table form for wave-uniform angles (dr_dxdy_uni;
// with one angle per lane its scalar load becomes a vector load of the same table).  TXSYM: tx set 0..2 x transform type 0..15.  SMW: every entry of the five smooth
// weight tables.
enum { K1L_N_DERIV = 291, K1L_N_EDGE = 25 * 2 * 271, K1L_N_ROW = 8 * 7, K1L_N_TXSYM = 3 * 16, K1L_N_SMW = 4 + 8 + 16 + 32 + 64,
       K1L_TOTAL = K1L_N_DERIV + 2 * K1L_N_EDGE + 2 * (K1L_N_ROW + K1L_N_DERIV) + K1L_N_TXSYM + K1L_N_SMW };

struct K1LArg { int op, a[4]; };

K1L_FN K1LArg k1l_arg(int i) {
  K1LArg q = { K1L_OPS, { 0, 0, 0, 0 } };
  if (i < 0) return q;
  if (i < K1L_N_DERIV) { q.op = K1L_DERIV; q.a[0] = i - 10; return q; }
  i -= K1L_N_DERIV;
  for (int op = K1L_STRENGTH; op <= K1L_UPSAMPLE; op++) {
    if (i < K1L_N_EDGE) {
      const int d = i % 271, r = i / 271, ft = r & 1, s = r >> 1;       // delta fastest, then the filter type, then the shape
      q.op = op; q.a[0] = 4 << (s / 5); q.a[1] = 4 << (s % 5); q.a[2] = ft; q.a[3] = d - 135;
      return q;
    }
    i -= K1L_N_EDGE;
  }
  for (int op = K1L_DXDY_ROW; op <= K1L_DXDY_UNI_ROW; op += 2) {
    if (i < K1L_N_ROW) { q.op = op; q.a[0] = 1 + i / 7; q.a[1] = i % 7 - 3; return q; }               // mode V_PRED .. D67_PRED, delta
    i -= K1L_N_ROW;
    if (i < K1L_N_DERIV) { q.op = op + 1; q.a[0] = i - 10; return q; }
    i -= K1L_N_DERIV;
  }
  if (i < K1L_N_TXSYM) { q.op = K1L_TXSYM; q.a[0] = i / 16; q.a[1] = i % 16; return q; }
  i -= K1L_N_TXSYM;
  if (i < K1L_N_SMW) {
    int l = 2;
    while (i >= (1 << l)) { i -= 1 << l; l++; }
    q.op = K1L_SMW; q.a[0] = l; q.a[1] = i;
  }
  return q;
}

// the product's functions on one argument (dx and dy of a row packed as dx | dy << 16)
__device__ inline int k1l_new(const K1LArg &q) {
  int dx, dy;
  switch (q.op) {
    case K1L_DERIV: return dr_deriv_dev(q.a[0]);
    case K1L_STRENGTH: return edge_strength_dev(q.a[0], q.a[1], q.a[2], q.a[3]);
    case K1L_UPSAMPLE: return edge_upsample_sel_dev(q.a[0], q.a[1], q.a[2], q.a[3]);
    case K1L_DXDY_ROW: dr_dxdy_dev(mode_angle_of(q.a[0]) + 3 * q.a[1], &dx, &dy); return dx | (dy << 16);
    case K1L_DXDY_ANGLE: dr_dxdy_dev(q.a[0], &dx, &dy); return dx | (dy << 16);
    case K1L_DXDY_UNI_ROW: dr_dxdy_uni(mode_angle_of(q.a[0]) + 3 * q.a[1], &dx, &dy); return dx | (dy << 16);
    case K1L_DXDY_UNI_ANGLE: dr_dxdy_uni(q.a[0], &dx, &dy); return dx | (dy << 16);
    case K1L_TXSYM: return txtype_to_sym(q.a[0], q.a[1]);
    case K1L_SMW: return sm_weights_dev(q.a[0])[q.a[1]];
    default: return -1;
  }
}
