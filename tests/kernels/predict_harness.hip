// predict_harness.hip -- TEST INFRASTRUCTURE: the tile search's intra prediction and distortion stages (cavif_rs_amd/csrc/tile_search.h with dev_predict.h,
// dev_group.h, dev_rect.h and dev_blk64.h, unchanged; nothing of K1 itself is instantiated) on blocks given by the test.
// The block runner gives every case one wavefront: it stages a FrameDev head in LDS (geometry as plan_geometry / fill_dev of host_frames.h give it), fills the
// wave's LDS arena with a seeded pattern, calls the functions with the argument shapes try_block / try_block_rect use (raw edges at +EDGE_OFF, working copies of
// EDGE_LEN(64), one GroupPredBuf per 16-lane row) and copies the whole arena back, so that the test sees the defined output and everything around it.
// The planes and the distortion samples sit between guard zones in device memory; the functions only read them.  A second entry point runs the small
// __device__ functions on rows of arguments, one thread per row.
// Built twice by tests/helpers/predict_harness.py: hipcc for gfx950 with the product's flags, g++ with the SIMT emulator (tests/emu/).
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "../../cavif_rs_amd/csrc/tile_search.h"

#define PH_GUARD 256                 /* bytes of sentinel in front of and behind every device buffer */
#define PH_SENT 0xA7
enum { PH_WAVE = 0, PH_RECT = 1, PH_GDIR4 = 2, PH_GDIR8 = 3, PH_GNON4 = 4, PH_GNON8 = 5, PH_CFL = 6, PH_SATD = 7, PH_SATD_WH = 8, PH_SATD_G4 = 9, PH_SATD_G8 = 10, PH_SSE = 11, PH_PSY = 12, PH_OPS = 13 };

// the wave's LDS arena in uint16 units (mirrored by tests/helpers/predict_harness.py): 32 guard entries in front of, between and behind the buffers
enum { A_G = 32, A_EDGE = EDGE_LEN(64), A_RA = A_G, A_RL = A_RA + A_EDGE + A_G, A_WA = A_RL + A_EDGE + A_G, A_WL = A_WA + A_EDGE + A_G, A_TMP = A_WL + A_EDGE + A_G,
       A_TMP_LEN = 2 * 64 + 16, A_PRED = A_TMP + A_TMP_LEN + A_G, A_SRC = A_PRED + 4096 + A_G, A_GP = A_SRC + 4096 + A_G, A_GP_LEN = 4 * (int)(sizeof(GroupPredBuf) / 2),
       A_AUX = A_GP + A_GP_LEN + A_G, A_AUX_LEN = 2 * 2 * 64 /* 64 cells' variance and activity, 32 bits each */, A_LEN = A_AUX + A_AUX_LEN + A_G };
#define PH_HEAD 1024                 /* bytes of LDS in front of the arena: the FrameDev head */
static_assert(FRAMEDEV_K1_BYTES <= PH_HEAD, "the FrameDev head outgrew its LDS slot");
static_assert(sizeof(GroupPredBuf) == 192 * 2, "GroupPredBuf layout (tests/helpers/predict_harness.py)");

// mirrored field by field by tests/helpers/predict_harness.py (ctypes)
struct PhCase {
  int op, bd, w, h;                  // the picture: w x h samples (the mi grid and the padded planes follow from it)
  int plane_off, luma_off;           // first sample of the plane the edges are read from (rec[1]) and of the luma plane (rec[0]) in `planes`
  int x, y, wl, hl;                  // the block
  int have_left, have_above, have_ar, have_bl;
  int ftype, alpha;
  int mode[4], delta[4];             // PH_WAVE / PH_RECT / PH_CFL: [0]; PH_GDIR: mode[g] = the row's prediction angle; PH_GNON: mode[g] (< 0: the row idles)
  int data_off, aux_off;             // distortion: first sample in `data` (src, then the prediction(s)); PH_PSY: first word in `aux` (the cells' variances, then their activities)
};

__device__ __forceinline__ uint16_t ph_fill(unsigned seed, int i) { return (uint16_t)(((unsigned)i * 2654435761u + seed * 40503u) >> 13); }

__global__ __launch_bounds__(64) void ph_block_kernel(const PhCase *cases, const uint16_t *planes, const uint16_t *data, const int *aux, uint16_t *dump, long long *res, unsigned seed) {
  extern __shared__ __align__(16) uint8_t smem[];
  const PhCase c = cases[blockIdx.x];
  LDS FrameDev *f = (LDS FrameDev *)smem;
  LDS uint16_t *ar = (LDS uint16_t *)(smem + PH_HEAD);
  for (int i = LANE; i < PH_HEAD / 4; i += 64) ((LDS int *)smem)[i] = 0;
  for (int i = LANE; i < A_LEN; i += 64) ar[i] = ph_fill(seed, i);
  WAVE_SYNC();
  if (LANE == 0) {
    f->w = c.w; f->h = c.h; f->bd = c.bd; f->np = 3;
    f->mi_cols = 2 * ((c.w + 7) >> 3); f->mi_rows = 2 * ((c.h + 7) >> 3); f->sb_cols = (f->mi_cols + 15) >> 4; f->sb_rows = (f->mi_rows + 15) >> 4;
    f->pw = f->sb_cols * 64; f->ph = f->sb_rows * 64; f->stride = f->pw; f->mi_stride = f->pw / 4; f->mi_h = f->ph / 4;
    f->rec[0] = const_cast<uint16_t *>(planes) + c.luma_off; f->rec[1] = const_cast<uint16_t *>(planes) + c.plane_off; f->rec[2] = f->rec[1];
  }
  WAVE_SYNC();
  LDS uint16_t *ra = ar + A_RA + EDGE_OFF, *rl = ar + A_RL + EDGE_OFF, *wa = ar + A_WA + EDGE_OFF, *wl = ar + A_WL + EDGE_OFF, *tmp = ar + A_TMP;
  LDS uint16_t *pred = ar + A_PRED, *src = ar + A_SRC;
  LDS GroupPredBuf *gp = (LDS GroupPredBuf *)(ar + A_GP);
  const int bw = 1 << c.wl, bh = 1 << c.hl, g = GROUP_ID;
  long long r = 0;
  switch (c.op) {
    case PH_WAVE:
      load_edges(f, 1, c.x, c.y, bw, c.have_left, c.have_above, c.have_ar, c.have_bl, ra, rl);
      predict_block(f, c.x, c.y, c.wl, c.have_left, c.have_above, c.mode[0], c.delta[0], c.ftype, ra, rl, wa, wl, tmp, pred);
      break;
    case PH_RECT:
      load_edges_wh(f, 1, c.x, c.y, bw, bh, c.have_left, c.have_above, c.have_ar, c.have_bl, ra, rl);
      predict_block_wh(f, c.x, c.y, c.wl, c.hl, c.have_left, c.have_above, c.mode[0], c.delta[0], c.ftype, ra, rl, wa, wl, tmp, pred);
      break;
    case PH_GDIR4: case PH_GDIR8:
      load_edges(f, 1, c.x, c.y, bw, c.have_left, c.have_above, c.have_ar, c.have_bl, ra, rl);
      if (c.op == PH_GDIR4) predict_dir_group<4>(f, c.x, c.y, c.have_left, c.have_above, c.mode[g], c.ftype, ra, rl, &gp[g]);
      else predict_dir_group<8>(f, c.x, c.y, c.have_left, c.have_above, c.mode[g], c.ftype, ra, rl, &gp[g]);
      break;
    case PH_GNON4: case PH_GNON8:
      load_edges(f, 1, c.x, c.y, bw, c.have_left, c.have_above, c.have_ar, c.have_bl, ra, rl);
      if (c.op == PH_GNON4) predict_nondir_group<4>(c.mode[g], c.have_left, c.have_above, c.bd, ra, rl, gp[g].pred);
      else predict_nondir_group<8>(c.mode[g], c.have_left, c.have_above, c.bd, ra, rl, gp[g].pred);
      break;
    case PH_CFL:                                   // the DC prediction of the chroma plane into src (try_block's dcp), then chroma from luma into pred
      load_edges(f, 1, c.x, c.y, bw, c.have_left, c.have_above, c.have_ar, c.have_bl, ra, rl);
      predict_block(f, c.x, c.y, c.wl, c.have_left, c.have_above, DC_PRED, 0, c.ftype, ra, rl, wa, wl, tmp, src);
      predict_cfl_dev(f, c.x, c.y, c.wl, c.alpha, src, pred);
      break;
    case PH_SATD: case PH_SATD_WH: case PH_SSE: {
      const int nn = bw * bh;
      for (int i = LANE; i < nn; i += 64) { src[i] = data[c.data_off + i]; pred[i] = data[c.data_off + nn + i]; }
      WAVE_SYNC();
      r = c.op == PH_SATD ? satd_dev(src, pred, bw) : (c.op == PH_SATD_WH ? satd_wh(src, pred, bw, bh) : sse_dev(src, pred, nn));
      if (LANE == 0) res[blockIdx.x * 4] = r;
      break;
    }
    case PH_SATD_G4: case PH_SATD_G8: {            // one source block, one prediction per 16-lane row
      const int nn = bw * bh;
      for (int i = LANE; i < nn; i += 64) src[i] = data[c.data_off + i];
      for (int i = LANE; i < 4 * nn; i += 64) gp[i / nn].pred[i % nn] = data[c.data_off + nn + i];
      WAVE_SYNC();
      r = c.op == PH_SATD_G4 ? satd_group<4>(src, gp[g].pred) : satd_group<8>(src, gp[g].pred);
      if (GROUP_LANE == 0) res[blockIdx.x * 4 + g] = r;
      break;
    }
    case PH_PSY: {                                 // the cells' source variances and activities as try_block stages them (psv, pact)
      const int nn = bw * bh, ncell = bw == 4 ? 1 : (bw >> 3) * (bw >> 3);
      LDS int *sv = (LDS int *)(ar + A_AUX), *act = sv + 64;
      for (int i = LANE; i < nn; i += 64) { src[i] = data[c.data_off + i]; pred[i] = data[c.data_off + nn + i]; }
      for (int i = LANE; i < ncell; i += 64) { sv[i] = aux[c.aux_off + i]; act[i] = aux[c.aux_off + ncell + i]; }
      WAVE_SYNC();
      switch (c.wl) {
        case 2: r = psy_dist_wave<4>(src, pred, sv, act, c.bd); break;
        case 3: r = psy_dist_wave<8>(src, pred, sv, act, c.bd); break;
        case 4: r = psy_dist_wave<16>(src, pred, sv, act, c.bd); break;
        case 5: r = psy_dist_wave<32>(src, pred, sv, act, c.bd); break;
        default: r = psy_dist_wave<64>(src, pred, sv, act, c.bd); break;
      }
      if (LANE == 0) res[blockIdx.x * 4] = r;
      break;
    }
    default: break;
  }
  WAVE_SYNC();
  for (int i = LANE; i < A_LEN; i += 64) dump[(size_t)blockIdx.x * A_LEN + i] = ar[i];
}

namespace {
struct Buf { uint8_t *dev; void *host; size_t bytes; bool back; };
struct Pool {
  std::vector<Buf> bufs; bool ok = true;
  template <typename T> T *put(T *host, size_t count, bool back = true) {
    if (!host || !ok) return nullptr;
    const size_t bytes = count * sizeof(T);
    uint8_t *d = nullptr;
    if (hipMalloc(&d, bytes + 2 * PH_GUARD) != hipSuccess) { ok = false; return nullptr; }
    bufs.push_back({ d, (void *)host, bytes, back });
    if (hipMemset(d, PH_SENT, bytes + 2 * PH_GUARD) != hipSuccess || hipMemcpy(d + PH_GUARD, host, bytes, hipMemcpyHostToDevice) != hipSuccess) ok = false;
    return (T *)(d + PH_GUARD);
  }
  // copies the buffers back and counts their changed guard bytes; a buffer that is not copied back must still hold what it was given
  int collect() {
    int damage = 0;
    std::vector<uint8_t> g(2 * PH_GUARD), now;
    for (const Buf &b : bufs) {
      if (b.back) { if (hipMemcpy(b.host, b.dev + PH_GUARD, b.bytes, hipMemcpyDeviceToHost) != hipSuccess) ok = false; }
      else {
        now.resize(b.bytes);
        if (hipMemcpy(now.data(), b.dev + PH_GUARD, b.bytes, hipMemcpyDeviceToHost) != hipSuccess) ok = false;
        damage += std::memcmp(now.data(), b.host, b.bytes) != 0;
      }
      if (hipMemcpy(g.data(), b.dev, PH_GUARD, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(g.data() + PH_GUARD, b.dev + PH_GUARD + b.bytes, PH_GUARD, hipMemcpyDeviceToHost) != hipSuccess) ok = false;
      for (uint8_t v : g) damage += v != PH_SENT;
    }
    return damage;
  }
  ~Pool() { for (const Buf &b : bufs) (void)hipFree(b.dev); }
};
bool ph_angle_ok(int pa) {
  static const int base[8] = { 45, 67, 90, 113, 135, 157, 180, 203 };
  for (int b : base) for (int d = -3; d <= 3; d++) if (pa == b + 3 * d) return true;
  return false;
}
// only arguments the functions are written for reach the device, and nothing they read lies outside the buffers
bool ph_case_ok(const PhCase &c, size_t nplanes, size_t ndata, size_t naux) {
  if (c.op < 0 || c.op >= PH_OPS || (c.bd != 8 && c.bd != 10) || c.wl < 2 || c.wl > 6 || c.hl < 2 || c.hl > 6) return false;
  const int bw = 1 << c.wl, bh = 1 << c.hl, nn = bw * bh;
  if (c.op >= PH_SATD) {
    const size_t need = (size_t)nn * (c.op == PH_SATD_G4 || c.op == PH_SATD_G8 ? 5 : 2);
    if (c.data_off < 0 || (size_t)c.data_off + need > ndata) return false;
    if (c.op == PH_PSY) { const size_t nc = c.wl == 2 ? 1 : (size_t)(bw >> 3) * (bw >> 3); return c.wl == c.hl && c.aux_off >= 0 && (size_t)c.aux_off + 2 * nc <= naux; }
    if (c.op == PH_SATD) return c.wl == c.hl;
    if (c.op == PH_SATD_WH) return (c.wl == 3 && c.hl == 2) || (c.wl == 2 && c.hl == 3);
    if (c.op == PH_SATD_G4) return c.wl == 2 && c.hl == 2;
    if (c.op == PH_SATD_G8) return c.wl == 3 && c.hl == 3;
    return true;
  }
  if (c.w < 1 || c.h < 1 || c.w > 256 || c.h > 256) return false;
  const int mi_cols = 2 * ((c.w + 7) >> 3), mi_rows = 2 * ((c.h + 7) >> 3), pw = ((mi_cols + 15) >> 4) * 64, ph = ((mi_rows + 15) >> 4) * 64;
  const size_t npx = (size_t)pw * ph;
  if (c.plane_off < 0 || c.luma_off < 0 || (size_t)c.plane_off + npx > nplanes || (size_t)c.luma_off + npx > nplanes) return false;
  if (c.x < 0 || c.y < 0 || (c.x & 3) || (c.y & 3) || c.x > mi_cols * 4 - 1 || c.y > mi_rows * 4 - 1 || c.x + bw > pw || c.y + bh > ph) return false;
  for (int v : { c.have_left, c.have_above, c.have_ar, c.have_bl, c.ftype }) if (v != 0 && v != 1) return false;
  if ((c.have_above && c.y == 0) || (c.have_left && c.x == 0) || (c.have_ar && !c.have_above) || (c.have_bl && !c.have_left)) return false;
  if (c.op == PH_RECT) { if (!((c.wl == 3 && c.hl == 2) || (c.wl == 2 && c.hl == 3))) return false; }
  else if (c.wl != c.hl) return false;
  if ((c.op == PH_GDIR4 || c.op == PH_GNON4) && c.wl != 2) return false;
  if ((c.op == PH_GDIR8 || c.op == PH_GNON8) && c.wl != 3) return false;
  if (c.op == PH_WAVE || c.op == PH_RECT) {
    if (c.mode[0] < 0 || c.mode[0] > 12 || c.delta[0] < -3 || c.delta[0] > 3) return false;
    if ((c.mode[0] == 0 || c.mode[0] > 8) && c.delta[0] != 0) return false;
  }
  if (c.op == PH_GDIR4 || c.op == PH_GDIR8) for (int g = 0; g < 4; g++) if (!ph_angle_ok(c.mode[g])) return false;
  if (c.op == PH_GNON4 || c.op == PH_GNON8) for (int g = 0; g < 4; g++) if (!(c.mode[g] == -1 || c.mode[g] == 0 || (c.mode[g] >= 9 && c.mode[g] <= 12))) return false;
  if (c.op == PH_CFL && (c.alpha < -16 || c.alpha > 16)) return false;
  return true;
}
}

extern "C" int ph_arena_len(void) { return A_LEN; }

// Runs all cases in one launch (one wavefront each).  dump: ncases x ph_arena_len() samples, res: ncases x 4.  Returns 0, -1 for arguments the functions are
// not written for (nothing is launched then), -10 for a HIP error, -20 when a guard zone or a read-only buffer changed.
extern "C" int ph_run(const PhCase *cases, int ncases, const uint16_t *planes, long long nplanes, const uint16_t *data, long long ndata, const int *aux, long long naux, uint16_t *dump, long long *res, unsigned seed) {
  if (ncases <= 0 || ncases > (1 << 16) || nplanes < 1 || ndata < 1 || naux < 1 || !cases || !planes || !data || !aux || !dump || !res) return -1;
  for (int k = 0; k < ncases; k++) if (!ph_case_ok(cases[k], (size_t)nplanes, (size_t)ndata, (size_t)naux)) return -1;
  for (long long i = 0; i < nplanes; i++) if (planes[i] > 1023) return -1;
  for (long long i = 0; i < ndata; i++) if (data[i] > 1023) return -1;
  for (long long i = 0; i < naux; i++) if (aux[i] < 0) return -1;
  Pool pool;
  std::memset(dump, 0, (size_t)ncases * A_LEN * 2);
  std::memset(res, 0, (size_t)ncases * 4 * sizeof(long long));
  const PhCase *d_cases = pool.put(const_cast<PhCase *>(cases), (size_t)ncases, false);
  const uint16_t *d_planes = pool.put(const_cast<uint16_t *>(planes), (size_t)nplanes, false);
  const uint16_t *d_data = pool.put(const_cast<uint16_t *>(data), (size_t)ndata, false);
  const int *d_aux = pool.put(const_cast<int *>(aux), (size_t)naux, false);
  uint16_t *d_dump = pool.put(dump, (size_t)ncases * A_LEN);
  long long *d_res = pool.put(res, (size_t)ncases * 4);
  if (!pool.ok) return -10;
  hipLaunchKernelGGL(ph_block_kernel, dim3(ncases), dim3(64), PH_HEAD + A_LEN * 2, 0, d_cases, d_planes, d_data, d_aux, d_dump, d_res, seed);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -10;
  const int damage = pool.collect();
  if (!pool.ok) return -10;
  return damage ? -20 : 0;
}

// ---------------------------------------------------------------- the table runner: one thread per row of 8 arguments -> 1 result
enum { PT_STRENGTH = 0, PT_UPSAMPLE = 1, PT_DERIV = 2, PT_SM_WEIGHT = 3, PT_MODE_ANGLE = 4, PT_DECODED = 5, PT_OPS = 6 };
#define PT_IN 8
__global__ __launch_bounds__(64) void ph_table_kernel(int op, const int *in, int *out, int nrows) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nrows) return;
  const int *a = in + (size_t)row * PT_IN;
  int v = 0;
  if (op == PT_STRENGTH) v = edge_strength_dev(a[0], a[1], a[2], a[3]);            // w, h, filter type, delta
  else if (op == PT_UPSAMPLE) v = edge_upsample_sel_dev(a[0], a[1], a[2], a[3]);
  else if (op == PT_DERIV) v = dr_deriv_dev(a[0]);
  else if (op == PT_SM_WEIGHT) v = sm_weights_dev(a[0])[a[1]];                      // log2 size, index
  else if (op == PT_MODE_ANGLE) v = mode_angle_of(a[0]);
  else if (op == PT_DECODED) v = decoded_before(a[0], a[1], a[2], a[3], a[4]);     // cur_r, cur_c, shape, pr, pc
  out[row] = v;
}

extern "C" int ph_table(int op, const int *in, int *out, int nrows) {
  if (nrows <= 0 || nrows > (1 << 22) || op < 0 || op >= PT_OPS) return -1;
  for (int r = 0; r < nrows; r++) {
    const int *a = in + (size_t)r * PT_IN;
    if (op == PT_SM_WEIGHT && (a[0] < 2 || a[0] > 6 || a[1] < 0 || a[1] >= (1 << a[0]))) return -1;
    if (op == PT_MODE_ANGLE && (a[0] < 1 || a[0] > 8)) return -1;
    if (op == PT_DECODED) { for (int i = 0; i < 5; i++) if (a[i] < 0 || a[i] > 4096) return -1; if (a[2] > 2) return -1; }
  }
  Pool pool;
  std::vector<int> zeros((size_t)nrows, 0);
  const int *d_in = pool.put(const_cast<int *>(in), (size_t)nrows * PT_IN, false);
  int *d_out = pool.put(zeros.data(), (size_t)nrows);
  if (!pool.ok) return -10;
  hipLaunchKernelGGL(ph_table_kernel, dim3((nrows + 63) / 64), dim3(64), 0, 0, op, d_in, d_out, nrows);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -10;
  const int damage = pool.collect();
  if (!pool.ok) return -10;
  if (damage) return -20;
  std::memcpy(out, zeros.data(), zeros.size() * sizeof(int));
  return 0;
}
