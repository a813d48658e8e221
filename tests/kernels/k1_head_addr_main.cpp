// k1_head_addr_main.cpp -- TEST INFRASTRUCTURE: a stand-alone host program (g++ with the SIMT emulator's macros, tests/emu/include) for the address step of the tile
// search's split staging helpers: txb_ctx_addr (dev_rate.h) and edge_addr (dev_predict.h) against restatements of the helpers they replaced (txb_ctx_dev / txb_ctx_wh,
// load_edges / load_edges_wh as they stood when each of them loaded for itself).  A tile of 3 x 3 superblocks, placed at the frame's origin or one superblock in, in frames
// that end with the tile, beyond it, or inside its last superblock; every block shape of both classes at every aligned position, every availability the search can
// pass, every lane of a wave.  Each address must equal the one the earlier helper loaded from, or -- where the earlier helper loaded nothing -- be the block's own
// cell / first sample; and every address must lie inside the map / plane.  Prints "checked N mismatches M out of bounds B"; exit status 0 when M == B == 0.
#include <cstdio>
#include "../../cavif_rs_amd/csrc/dev_predict.h"
#include "../../cavif_rs_amd/csrc/dev_rate.h"

namespace old_form {
struct Ctx { bool loads; int ia, il; bool ha, hl; };
// txb_ctx_wh (txb_ctx_dev: w4 == h4): lanes below max(w4, h4) load, both neighbours unconditionally, the block's own cell where there is none
Ctx txb_ctx(int ms, int mi_rows, int mi_cols, int row_start, int col_start, int r4, int c4, int w4, int h4, int k) {
  Ctx o = { false, 0, 0, false, false };
  if (k < (w4 > h4 ? w4 : h4)) {
    o.loads = true;
    o.ha = k < w4 && r4 - 1 >= row_start && c4 + k < mi_cols; o.hl = k < h4 && c4 - 1 >= col_start && r4 + k < mi_rows;
    o.ia = o.ha ? (r4 - 1) * ms + c4 + k : r4 * ms + c4; o.il = o.hl ? (r4 + k) * ms + c4 - 1 : r4 * ms + c4;
  }
  return o;
}
struct Edge { bool loads; int ia, il; };
// load_edges_wh (load_edges: w == h): lanes 0 .. w + h load, lane w + h the corner
Edge edge(int rs, int mi_rows, int mi_cols, int x, int y, int w, int h, int have_left, int have_above, int have_ar, int have_bl, int i) {
  Edge o = { false, 0, 0 };
  const int tot = w + h, max_x = mi_cols * 4 - 1, max_y = mi_rows * 4 - 1;
  const int na = x + (have_ar ? 2 * w : w) - 1, nl = y + (have_bl ? 2 * h : h) - 1;
  const int lim_a = max_x < na ? max_x : na, lim_l = max_y < nl ? max_y : nl;
  if (i <= tot) {
    const bool corner = i == tot;
    o.loads = true;
    if (have_above) o.ia = (y - 1) * rs + (corner ? (have_left ? x - 1 : x) : (lim_a < x + i ? lim_a : x + i));
    else o.ia = y * rs + (have_left ? x - 1 : x);
    if (have_left) o.il = (lim_l < y + i ? lim_l : y + i) * rs + x - 1;
    else o.il = (have_above ? y - 1 : y) * rs + x;
  }
  return o;
}
}  // namespace old_form

int main() {
  long checked = 0, bad = 0, oob = 0;
  static const int shapes[][2] = { { 1, 1 }, { 2, 2 }, { 4, 4 }, { 8, 8 }, { 16, 16 }, { 2, 1 }, { 1, 2 } };          // (w4, h4): 4x4 .. 64x64, 8x4, 4x8
  auto report = [&](const char *what, int a, int b, int r, int c, int w4, int h4, int k) {
    if (bad++ < 20) printf("%s: got %d, earlier form %d at r %d c %d block %dx%d lane %d\n", what, a, b, r, c, w4 * 4, h4 * 4, k);
  };
  for (int origin = 0; origin <= 16; origin += 16)
    for (int fr = 0; fr < 3; fr++)
      for (int fc = 0; fc < 3; fc++) {
        const int row_start = origin, col_start = origin, tile_rows = 48, tile_cols = 48;
        // the frame ends with the tile, one superblock beyond it, or 3 / 5 cells inside its last superblock (the tile is cut to the frame then)
        const int mi_rows = row_start + (fr == 0 ? tile_rows : fr == 1 ? tile_rows + 16 : tile_rows - 3), mi_cols = col_start + (fc == 0 ? tile_cols : fc == 1 ? tile_cols + 16 : tile_cols - 5);
        const int row_end = row_start + tile_rows < mi_rows ? row_start + tile_rows : mi_rows, col_end = col_start + tile_cols < mi_cols ? col_start + tile_cols : mi_cols;
        const int ms = ((mi_cols + 15) & ~15) + 16, rs = ms * 4, plane_rows = ((mi_rows + 15) & ~15) * 4;
        for (const auto &sh : shapes) {
          const int w4 = sh[0], h4 = sh[1], w = w4 * 4, h = h4 * 4;
          for (int r = row_start; r < row_end; r += h4)
            for (int c = col_start; c < col_end; c += w4) {
              // ---- the transform contexts' cells ----
              for (int k = 0; k < 64; k++) {
                const TxbCtxAddr a = txb_ctx_addr(ms, mi_rows, mi_cols, row_start, col_start, r, c, w4, h4, k);
                const old_form::Ctx o = old_form::txb_ctx(ms, mi_rows, mi_cols, row_start, col_start, r, c, w4, h4, k);
                const int own = r * ms + c;
                checked += 2;
                if (o.loads) {
                  if (a.ia != o.ia) report("ctx above", a.ia, o.ia, r, c, w4, h4, k);
                  if (a.il != o.il) report("ctx left", a.il, o.il, r, c, w4, h4, k);
                  if (a.ha != o.ha || a.hl != o.hl) report("ctx flags", a.ha * 2 + a.hl, o.ha * 2 + o.hl, r, c, w4, h4, k);
                } else {
                  if (a.ia != own || a.il != own || a.ha || a.hl) report("ctx idle lane", a.ia, own, r, c, w4, h4, k);
                }
                for (int v : { a.ia, a.il }) if (v < 0 || v / ms >= mi_rows || v % ms >= mi_cols) oob++;
              }
              // ---- the raw edges' samples ----
              const int x = c * 4, y = r * 4, have_above = r > row_start, have_left = c > col_start;
              const int can_ar = have_above && c + w4 < col_end, can_bl = have_left && r + h4 < row_end;
              for (int have_ar = 0; have_ar <= can_ar; have_ar++)
                for (int have_bl = 0; have_bl <= can_bl; have_bl++)
                  for (int i = 0; i < 192; i++) {
                    const EdgeAddr e = edge_addr(rs, mi_rows, mi_cols, x, y, w, h, have_left, have_above, have_ar, have_bl, i);
                    const old_form::Edge o = old_form::edge(rs, mi_rows, mi_cols, x, y, w, h, have_left, have_above, have_ar, have_bl, i);
                    const int own = y * rs + x;
                    checked += 2;
                    if (o.loads) {
                      if (e.ia != o.ia) report("edge above", e.ia, o.ia, r, c, w4, h4, i);
                      if (e.il != o.il) report("edge left", e.il, o.il, r, c, w4, h4, i);
                    } else if (e.ia != own || e.il != own) report("edge idle lane", e.ia, own, r, c, w4, h4, i);
                    for (int v : { e.ia, e.il }) if (v < 0 || v / rs >= plane_rows || v % rs >= mi_cols * 4) oob++;
                  }
            }
        }
      }
  printf("checked %ld mismatches %ld out of bounds %ld\n", checked, bad, oob);
  return bad || oob ? 1 : 0;
}
