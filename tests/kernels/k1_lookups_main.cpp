// k1_lookups_main.cpp -- TEST INFRASTRUCTURE: a stand-alone host program (g++ with the SIMT emulator's macros, tests/emu/include) that compares the tile search's
// branch-free lookups (dev_predict.h, dev_common.h) with restatements of the switch / if forms they replaced, over every argument of k1_lookups_domain.h.
// Prints one line per mismatch (at most 20) and "checked N mismatches M"; exit status 0 when M == 0.  With a file name it also writes the restatements' values,
// one 32-bit integer per argument in the domain's order: what tests/test_k1_lookups.py compares the GPU harness's output with.
#include <cstdio>
#include <vector>
#include "k1_lookups_domain.h"

namespace old_form {
int dr_deriv(int a) {
  switch (a) {
    case 3: return 1023; case 6: return 547; case 9: return 372; case 14: return 273; case 17: return 215;
    case 20: return 178; case 23: return 151; case 26: return 132; case 29: return 116; case 32: return 102;
    case 36: return 90; case 39: return 80; case 42: return 71; case 45: return 64; case 48: return 57;
    case 51: return 51; case 54: return 45; case 58: return 40; case 61: return 35; case 64: return 31;
    case 67: return 27; case 70: return 23; case 73: return 19; case 76: return 15; case 81: return 11;
    case 84: return 7; case 87: return 3; default: return 0;
  }
}
int edge_strength(int w, int h, int ft, int delta) {
  const int d = delta < 0 ? -delta : delta, blk = w + h; int s = 0;
  if (ft == 0) {
    if (blk <= 8) { if (d >= 56) s = 1; }
    else if (blk <= 12) { if (d >= 40) s = 1; }
    else if (blk <= 16) { if (d >= 40) s = 1; }
    else if (blk <= 24) { if (d >= 8) s = 1; if (d >= 16) s = 2; if (d >= 32) s = 3; }
    else if (blk <= 32) { if (d >= 1) s = 1; if (d >= 4) s = 2; if (d >= 32) s = 3; }
    else { if (d >= 1) s = 3; }
  } else {
    if (blk <= 8) { if (d >= 40) s = 1; if (d >= 64) s = 2; }
    else if (blk <= 16) { if (d >= 20) s = 1; if (d >= 48) s = 2; }
    else if (blk <= 24) { if (d >= 4) s = 3; }
    else { if (d >= 1) s = 3; }
  }
  return s;
}
int edge_upsample_sel(int w, int h, int ft, int delta) {
  const int d = delta < 0 ? -delta : delta, blk = w + h;
  if (d <= 0 || d >= 40) return 0;
  return ft == 0 ? (blk <= 16) : (blk <= 8);
}
int dxdy(int pa) {
  int dx = 0, dy = 0;
  if (pa < 90) dx = dr_deriv(pa); else if (pa > 90 && pa < 180) dx = dr_deriv(180 - pa);
  if (pa > 90 && pa < 180) dy = dr_deriv(pa - 90); else if (pa > 180) dy = dr_deriv(270 - pa);
  return dx | (dy << 16);
}
int mode_angle(int m) { static const int t[9] = { 0, 90, 180, 45, 135, 113, 157, 203, 67 }; return t[m]; }
int sym_to_txtype(int set, int s) {
  static const int set1[7] = { IDTX, DCT_DCT, V_DCT, H_DCT, ADST_ADST, ADST_DCT, DCT_ADST }, set2[5] = { IDTX, DCT_DCT, ADST_ADST, ADST_DCT, DCT_ADST };
  return set == 0 ? DCT_DCT : (set == 1 ? set1[s] : set2[s]);
}
int txtype_to_sym(int set, int t) {
  const int n = set == 0 ? 1 : (set == 1 ? 7 : 5);
  for (int i = 0; i < n; i++) if (sym_to_txtype(set, i) == t) return i;
  return -1;
}
int sm_weight(int log2w, int i) {
  static const uint8_t w4[4] = { 255, 149, 85, 64 };
  static const uint8_t w8[8] = { 255, 197, 146, 105, 73, 50, 37, 32 };
  static const uint8_t w16[16] = { 255, 225, 196, 170, 145, 123, 102, 84, 68, 54, 43, 33, 26, 20, 17, 16 };
  static const uint8_t w32[32] = { 255, 240, 225, 210, 196, 182, 169, 157, 145, 133, 122, 111, 101, 92, 83, 74,
                                   66, 59, 52, 45, 39, 34, 29, 25, 21, 17, 14, 12, 10, 9, 8, 8 };
  static const uint8_t w64[64] = { 255, 248, 240, 233, 225, 218, 210, 203, 196, 189, 182, 176, 169, 163, 156, 150,
                                   144, 138, 133, 127, 121, 116, 111, 106, 101, 96, 91, 86, 82, 77, 73, 69,
                                   65, 61, 57, 54, 50, 47, 44, 41, 38, 35, 32, 29, 27, 25, 22, 20,
                                   18, 16, 15, 13, 12, 10, 9, 8, 7, 6, 6, 5, 5, 4, 4, 4 };
  switch (log2w) { case 2: return w4[i]; case 3: return w8[i]; case 4: return w16[i]; case 5: return w32[i]; default: return w64[i]; }
}
int eval(const K1LArg &q) {
  switch (q.op) {
    case K1L_DERIV: return dr_deriv(q.a[0]);
    case K1L_STRENGTH: return edge_strength(q.a[0], q.a[1], q.a[2], q.a[3]);
    case K1L_UPSAMPLE: return edge_upsample_sel(q.a[0], q.a[1], q.a[2], q.a[3]);
    case K1L_DXDY_ROW: case K1L_DXDY_UNI_ROW: return dxdy(mode_angle(q.a[0]) + 3 * q.a[1]);
    case K1L_DXDY_ANGLE: case K1L_DXDY_UNI_ANGLE: return dxdy(q.a[0]);
    case K1L_TXSYM: return txtype_to_sym(q.a[0], q.a[1]);
    case K1L_SMW: return sm_weight(q.a[0], q.a[1]);
    default: return -2;
  }
}
}

int main(int argc, char **argv) {
  std::vector<int32_t> want((size_t)K1L_TOTAL);
  int bad = 0, per_op[K1L_OPS] = { 0 };
  for (int i = 0; i < K1L_TOTAL; i++) {
    const K1LArg q = k1l_arg(i);
    if (q.op >= K1L_OPS) { printf("argument %d has no operation\n", i); return 2; }
    per_op[q.op]++;
    const int o = old_form::eval(q), n = k1l_new(q);
    want[(size_t)i] = o;
    if (o != n && bad++ < 20) printf("mismatch: op %d (%d, %d, %d, %d): was %d, is %d\n", q.op, q.a[0], q.a[1], q.a[2], q.a[3], o, n);
  }
  if (k1l_arg(-1).op != K1L_OPS || k1l_arg(K1L_TOTAL).op != K1L_OPS) { printf("the domain does not end at %d\n", K1L_TOTAL); return 2; }
  printf("per operation:");
  for (int op = 0; op < K1L_OPS; op++) printf(" %d", per_op[op]);
  printf("\nchecked %d mismatches %d\n", K1L_TOTAL, bad);
  if (argc > 1) {
    FILE *f = fopen(argv[1], "wb");
    if (!f || fwrite(want.data(), sizeof(int32_t), want.size(), f) != want.size() || fclose(f) != 0) { perror(argv[1]); return 2; }
  }
  return bad ? 1 : 0;
}
