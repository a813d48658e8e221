// host_frames.h -- the host side of the frame chain, shared by every entry point of mi_avif.hip: the per-device tables, the plan of one AV1 frame and its
// arena, the launch helpers of the kernels, the tile search's work queue, and FrameSet: a set of frames on one device, ready to run.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstddef>
#include <mutex>
#include <vector>
#include <algorithm>
#include "host_av1.h"
#include "tile_search.h"
#include "tile_entropy.h"
#include "loopfilter.h"
#include "restoration.h"

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { fprintf(stderr, "mi_avif: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return MI_ENCODING_ERROR; } } while (0)

namespace mi {

// move-only owner of one hipMalloc (DevBuf) or hipHostMalloc (PinBuf) buffer of `count` T's; freed by the destructor or the next alloc
template <class T, bool PINNED> struct HipBuf {
  T *p = nullptr;
  HipBuf() = default;
  HipBuf(HipBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
  HipBuf &operator=(HipBuf &&o) noexcept { std::swap(p, o.p); return *this; }
  ~HipBuf() { reset(); }
  void reset() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; }
  hipError_t alloc(size_t count) {
    reset();
    const hipError_t e = PINNED ? hipHostMalloc(&p, count * sizeof(T)) : hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess) p = nullptr;
    return e;
  }
  T *get() const { return p; }
};
template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using PinBuf = HipBuf<T, true>;

__global__ void pack_tiles_kernel(const FrameDev *frames, const TileJob *jobs, int njobs, const uint32_t *offsets, uint8_t *packed) {
  const int job = blockIdx.x;
  if (job >= njobs) return;
  const TileJob tj = jobs[job];
  const FrameDev *f = frames + tj.frame;
  const int ti = tj.tile_row * f->tile_cols + tj.tile_col;
  const uint32_t len = f->tile_len[ti];
  const uint8_t *src = f->tile_out + (size_t)ti * f->tile_out_cap;
  uint8_t *dst = packed + offsets[job];
  for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) dst[i] = src[i];
}

// ---- two-pass pricing (mi_av1_config.rdo_passes = 2): the rate table of the CDFs a tile ended its first pass with ----
__device__ inline uint32_t neg_log2_q9_dev(uint32_t p) {      // host_av1.h neg_log2_q9, integer only: (15 - log2 p) * 512
  if (p < 1u) p = 1u;
  const int msb = 31 - __clz(p);
  unsigned long long x = (unsigned long long)p << (31 - msb);
  uint32_t frac = 0;
  for (int i = 0; i < 9; i++) { x = (x * x) >> 31; frac <<= 1; if (x >> 32) { frac |= 1; x >>= 1; } }
  return (uint32_t)(15 * 512 - (msb * 512 + (int)frac));
}
// grid (tiles, frames): tile t of the frame; also switches the frame over to its second pass (tile_cost set, cdf_out cleared) -- by the
// block of tile 0, after a grid-wide ... no: by a separate tiny launch (pass_flip_kernel), the frames are read by every block here
__global__ __launch_bounds__(256) void cdf_cost_kernel(const FrameDev *frames) {
  const FrameDev *f = frames + blockIdx.y;
  const int tile = blockIdx.x;
  if (tile >= f->tile_cols * f->tile_rows || f->cdf_out == nullptr || frame_idle(f)) return;
  const uint16_t *cdf = f->cdf_out + (size_t)tile * CDF_TOTAL;
  uint16_t *cost = f->tile_cost_buf + (size_t)tile * CDF_TOTAL;
  for (int i = threadIdx.x; i < CDF_TOTAL; i += 256) cost[i] = 0;
  __syncthreads();
#define MI_ROW_(o, st, n, k) for (int i = threadIdx.x; i < (n) * (k); i += 256) { const int r = i / (k), s = i - r * (k); const uint16_t *row = cdf + (o) + r * (st); \
    cost[(o) + r * (st) + s] = (uint16_t)neg_log2_q9_dev((s > 0 ? (uint32_t)row[s - 1] : 32768u) - (uint32_t)row[s]); }
  MI_COST_ROWS(MI_ROW_)
#undef MI_ROW_
}
__global__ void pass_flip_kernel(FrameDev *frames, int nframes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nframes && frames[i].cdf_out != nullptr) { frames[i].tile_cost = frames[i].tile_cost_buf; frames[i].cdf_out = nullptr; }
}

// ---- per-device read-only tables ----
struct DeviceTables { uint16_t *cost[4] = { 0, 0, 0, 0 }; uint16_t *cdf0[4] = { 0, 0, 0, 0 }; bool ready = false; };
static std::mutex g_tab_mu;
#define MI_MAX_DEVICES 64
static DeviceTables g_tabs[MI_MAX_DEVICES];
// First launch of anything from this library makes the runtime load the gfx950 code object (~2 MB, 0.1-0.2 s): ensure_tables
// does it once per device with an empty kernel, so callers can overlap it with their allocations (mi_ravif_encode_stream does).
__global__ void module_warm_kernel() {}
static int ensure_tables(int dev) {
  std::lock_guard<std::mutex> lk(g_tab_mu);
  if (dev < 0 || dev >= MI_MAX_DEVICES) { fprintf(stderr, "mi_avif: HIP ordinal %d outside the supported 0..%d\n", dev, MI_MAX_DEVICES - 1); return MI_INVALID_ARGUMENT; }
  DeviceTables &t = g_tabs[dev];
  if (t.ready) return MI_OK;
  for (int q = 0; q < 4; q++) {
    const std::vector<uint16_t> cost = build_cost_table(q);
    HIP_OK(hipMalloc(&t.cost[q], CDF_TOTAL * 2)); HIP_OK(hipMalloc(&t.cdf0[q], CDF_TOTAL * 2));
    HIP_OK(hipMemcpy(t.cost[q], cost.data(), CDF_TOTAL * 2, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(t.cdf0[q], av1_default_cdfs + (size_t)q * CDF_TOTAL, CDF_TOTAL * 2, hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(module_warm_kernel, dim3(1), dim3(64), 0, 0);
  HIP_OK(hipDeviceSynchronize());
  t.ready = true;
  return MI_OK;
}

// ---- one AV1 frame (colour image or alpha plane) inside a batch ----
struct FramePlan {
  mi_av1_config cfg{}; int np = 3, image = 0; bool is_alpha = false;
  int mi_cols = 0, mi_rows = 0, sb_cols = 0, sb_rows = 0, pw = 0, ph = 0, mi_stride = 0, mi_h = 0, ntiles = 0, maxbs = 2;
  QuantSel q{}; Tiling tiles; FrameHeaderInfo hdr{};
  FrameDev dev{};
  size_t arena_bytes = 0; uint8_t *arena = nullptr;
  std::vector<uint8_t> obu;
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static int lr_units_host(uint32_t size) { const int n = ((int)size + 32) / 64; return n < 1 ? 1 : n; }
static size_t zeroed_bytes(const FramePlan &p) { return align_up((size_t)p.mi_stride * p.mi_h, 256) + align_up(6 * 65 * sizeof(long long), 256) + ((size_t)p.sb_rows * p.tiles.cols + (size_t)p.sb_rows * p.sb_cols + 1) * sizeof(int); }   // decoded flags, deblock tallies, K1's per-row counters and per-superblock root masks
static void plan_geometry(FramePlan &p) {
  const mi_av1_config &c = p.cfg;
  p.np = c.chroma == 1 ? 1 : 3;
  p.mi_cols = 2 * ((c.width + 7) >> 3); p.mi_rows = 2 * ((c.height + 7) >> 3);
  p.sb_cols = (p.mi_cols + 15) >> 4; p.sb_rows = (p.mi_rows + 15) >> 4;
  p.pw = p.sb_cols * 64; p.ph = p.sb_rows * 64; p.mi_stride = p.pw / 4; p.mi_h = p.ph / 4;
  int part_max = c.part_max, part_min = c.part_min;
  if (part_min > part_max) part_min = part_max;
  p.cfg.part_max = (uint8_t)part_max; p.cfg.part_min = (uint8_t)part_min;
  p.maxbs = part_max <= 16 ? 2 : 4;                   // the search's two block-size classes (tile_search.h k1_maxn): up to 16x16, up to 64x64
  p.q = select_quantizers(c.quantizer, c.bit_depth, p.np);
  p.tiles = plan_tiles((int)c.width, (int)c.height, p.sb_cols, p.sb_rows, c.min_tile_size, c.threads, c.tiles_override);
  p.ntiles = p.tiles.cols * p.tiles.rows;
}

// carve the frame's arena; returns bytes needed (dry run when base == nullptr)
static size_t carve(FramePlan &p, uint8_t *base, uint32_t tile_cap) {
  size_t off = 0;
  auto take = [&](size_t bytes) { uint8_t *ptr = base ? base + off : nullptr; off = align_up(off + bytes, 256); return ptr; };
  const size_t npx = (size_t)p.pw * p.ph, nmi = (size_t)p.mi_stride * p.mi_h;
  FrameDev &d = p.dev;
  for (int i = 0; i < p.np; i++) {
    d.src[i] = (uint16_t *)take(npx * 2); d.rec[i] = (uint16_t *)take(npx * 2); d.fin[i] = (uint16_t *)take(npx * 2);
    d.coef[i] = (int32_t *)take(npx * 4);
    d.m_lvl[i] = take(nmi); d.m_dc[i] = take(nmi); d.m_eob[i] = (uint16_t *)take(nmi * 2);
  }
  d.m_bsize = take(nmi); d.m_skip = take(nmi); d.m_ymode = take(nmi); d.m_uvmode = take(nmi); d.m_txtype = take(nmi);
  d.m_cfl_sign = take(nmi); d.m_cfl_au = take(nmi); d.m_cfl_av = take(nmi); d.m_txsize = take(nmi);
  // state the kernels expect zeroed before every encode, in one block (one memset): decoded flags + deblock tallies
  d.m_decoded = take(zeroed_bytes(p)); d.lf_tally = (long long *)(d.m_decoded + align_up(nmi, 256));
  d.sb_prog = (int *)(d.m_decoded + align_up(nmi, 256) + align_up(6 * 65 * sizeof(long long), 256));
  d.zero_words = (int)((zeroed_bytes(p) + 3) / 4);
  d.lf_out = (int *)take(64);                              // 4 deblock levels, segment count, 8 segment indices
  d.seg = (const SegTab *)take(sizeof(SegTab));
  d.m_angle_y = (int8_t *)take(nmi); d.m_angle_uv = (int8_t *)take(nmi);
  d.cdef_idx = (int8_t *)take((size_t)p.sb_cols * p.sb_rows);
  { const size_t ncell = (size_t)(p.pw / 8) * (p.ph / 8); d.act = (const uint32_t *)take(ncell * 4); d.svar8 = (const uint32_t *)take(ncell * 4); d.svar4 = (const uint32_t *)take(nmi * 4); }
  {
    const size_t nlr = (size_t)lr_units_host(p.cfg.width) * lr_units_host(p.cfg.height) * p.np;
    for (int i = 0; i < 3; i++) d.lrp[i] = (i < p.np && p.cfg.lrf) ? (uint16_t *)take(npx * 2) : nullptr;
    d.lr_type = take(nlr); d.lr_set = take(nlr); d.lr_xqd = (int8_t *)take(nlr * 2);
    d.lr_cand = p.cfg.lrf ? take(nlr * 16 * sizeof(LrCand)) : nullptr;
  }
  d.tile_out = take((size_t)p.ntiles * tile_cap);
  d.tile_len = (uint32_t *)take((size_t)p.ntiles * 4);
  d.tile_clk = (unsigned long long *)take((size_t)p.ntiles * 32);
  d.tile_cost = nullptr; d.cdf_out = nullptr; d.tile_cost_buf = nullptr;
  if (p.cfg.rdo_passes == 2) { d.cdf_out = (uint16_t *)take((size_t)p.ntiles * CDF_TOTAL * 2); d.tile_cost_buf = (uint16_t *)take((size_t)p.ntiles * CDF_TOTAL * 2); }
  d.prof_out = nullptr;
  d.tile_out_cap = tile_cap;
  return off;
}

static uint32_t tile_capacity(const FramePlan &p) {
  int tw = 0, th = 0;
  for (int i = 0; i < p.tiles.cols; i++) tw = std::max(tw, p.tiles.col_start[i + 1] - p.tiles.col_start[i]);
  for (int i = 0; i < p.tiles.rows; i++) th = std::max(th, p.tiles.row_start[i + 1] - p.tiles.row_start[i]);
  const size_t px = (size_t)tw * th * 4096;
  return (uint32_t)align_up(px * p.np * 2 + 4096, 256);
}

static void fill_dev(FramePlan &p, const DeviceTables &tab) {
  FrameDev &d = p.dev; const mi_av1_config &c = p.cfg;
  d.w = c.width; d.h = c.height; d.bd = c.bit_depth; d.np = p.np;
  d.mi_cols = p.mi_cols; d.mi_rows = p.mi_rows; d.sb_cols = p.sb_cols; d.sb_rows = p.sb_rows;
  d.pw = p.pw; d.ph = p.ph; d.stride = p.pw; d.mi_stride = p.mi_stride; d.mi_h = p.mi_h;
  d.base_q_idx = p.q.base_q_idx; d.qctx = p.q.qctx; d.rdmult = p.q.rdmult;
  d.seg_n = 0;
  for (int i = 0; i < 3; i++) { d.seg_ddc[i] = i < p.np ? p.q.dc_qi[i] - p.q.base_q_idx : 0; d.seg_dac[i] = i < p.np ? p.q.ac_qi[i] - p.q.base_q_idx : 0; }
  for (int i = 0; i < 3; i++) { d.dc_q[i] = p.q.dc_q[i]; d.ac_q[i] = p.q.ac_q[i]; d.wq[i] = p.q.wq[i]; d.dc_recip[i] = 0xFFFFFFFFu / (uint32_t)std::max(1, p.q.dc_q[i]); d.ac_recip[i] = 0xFFFFFFFFu / (uint32_t)std::max(1, p.q.ac_q[i]); }
  d.part_min = c.part_min; d.part_max = c.part_max; d.complex_modes = c.complex_pred_modes; d.fine_directional = c.fine_directional_intra;
  d.bottomup = c.encode_bottomup;
  d.tx_mode_select = c.rdo_tx_decision || c.inter_tx_split;    // rav1e FrameInvariants.tx_mode_select (recall)
  d.rdo_tx = c.rdo_tx_decision; d.reduced_tx_set = c.reduced_tx_set; d.enable_cdef = c.cdef; d.fast_deblock = c.fast_deblock;
  d.enable_restoration = c.lrf; d.sgr_full = c.sgr_full; d.tune_psnr = c.tune_psnr;
  { const uint32_t cdf[3] = { 9413, 22581, 32768 }; uint32_t lo = 0; for (int i = 0; i < 3; i++) { d.lr_cost[i] = neg_log2_q9(cdf[i] - lo); lo = cdf[i]; } }   // libaom default_switchable_restore_cdf
  d.tile_cols = p.tiles.cols; d.tile_rows = p.tiles.rows; d.tile_cols_log2 = p.tiles.cols_log2; d.tile_rows_log2 = p.tiles.rows_log2;
  for (int i = 0; i <= p.tiles.cols; i++) d.tile_col_start[i] = p.tiles.col_start[i];
  for (int i = 0; i <= p.tiles.rows; i++) d.tile_row_start[i] = p.tiles.row_start[i];
  d.cost = tab.cost[p.q.qctx]; d.cdf0 = tab.cdf0[p.q.qctx];
#if MI_DEBUG_HOOKS
  d.dbg = getenv("MI_DEBUG_LEVEL") ? atoi(getenv("MI_DEBUG_LEVEL")) : 0;
#else
  d.dbg = 0;
#endif
  // fast_deblock: the q formula; otherwise K2a searches the levels on the device and the host reads them back for the header
  const int lvl = c.fast_deblock ? deblock_level_from_q(p.q.ac_q[0], c.bit_depth) : 0;
  d.lf_level[0] = d.lf_level[1] = d.lf_level[2] = d.lf_level[3] = lvl; d.lf_sharp = 0;
  static const int strengths[8] = { 0, 1 * 4 + 0, 2 * 4 + 1, 3 * 4 + 1, 5 * 4 + 2, 7 * 4 + 3, 10 * 4 + 3, 13 * 4 + 3 };   // rav1e's fixed list
  d.cdef_damping = 3; d.cdef_bits = 3;
  for (int i = 0; i < 8; i++) { d.cdef_y[i] = strengths[i]; d.cdef_uv[i] = strengths[i]; }
  FrameHeaderInfo &h = p.hdr;
  h.cfg = c; h.np = p.np; h.sb_cols = p.sb_cols; h.sb_rows = p.sb_rows; h.q = p.q; h.tiles = p.tiles;
  for (int i = 0; i < 4; i++) h.lf_level[i] = d.lf_level[i];
  h.seg_n = 0; for (int i = 0; i < 8; i++) h.seg_qidx[i] = p.q.base_q_idx;
  h.lf_sharp = 0; h.enable_cdef = c.cdef; h.cdef_damping = 3; h.cdef_bits = 3; h.enable_restoration = c.lrf; h.tx_mode_select = d.tx_mode_select;
  for (int i = 0; i < 8; i++) { h.cdef_y[i] = strengths[i]; h.cdef_uv[i] = strengths[i]; }
}

// ---- K1 launch: the tile search as a work queue of superblocks (tile_search.h) ----
// Persistent workgroups: as many as the device holds at once for this instantiation (asked from the runtime, not assumed), capped by the number of items.
template <int MAXBS, int NW, bool BU, int TS> static hipError_t launch_search_t(const FrameDev *d_frames, const TileJob *d_jobs, const SbItem *d_items, int nitems, int *d_next, uint8_t *d_snap_pool, int *grid_out, int device, hipStream_t s) {
  const size_t lds = k1_lds_bytes<MAXBS, NW>();
  static int resident[MI_MAX_DEVICES];                    // per instantiation and device; 0 = not asked yet
  if (resident[device] == 0) {
    hipError_t e = hipFuncSetAttribute((const void *)tile_search_kernel<MAXBS, NW, BU, TS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    int per_cu = 0, cus = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)tile_search_kernel<MAXBS, NW, BU, TS>, 64 * NW, lds);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return e;
    resident[device] = std::max(1, per_cu) * std::max(1, cus);
  }
  const int grid = std::min(nitems, resident[device]);
  if (grid_out) { *grid_out = grid; return hipSuccess; }   // dry run: the caller sizes the snapshot pool
  hipLaunchKernelGGL((tile_search_kernel<MAXBS, NW, BU, TS>), dim3(grid), dim3(64 * NW), lds, s, d_frames, d_jobs, d_items, nitems, d_next, d_snap_pool, 0);   // 0: persistent workgroups (tile_search.h ipw)
  return hipGetLastError();
}
static size_t k1_snap_bytes(int maxbs) { return MI_K1_POOL_BYTES(maxbs); }
// every frame of a launch comes from one encoder configuration, so the partition order (top-down / bottom-up) is per launch; the
// jobs must all belong to frames of the same block-size class (one instantiation per class).  grid_out != nullptr: only report the grid.
// `tools`: the tool set the kernels are instantiated for (tile_search.h Tools): bit 0 = the full candidate set of speed <= 1 (complex_pred_modes), bit 1 = the switches of
// ravif's speed 4 as constants -- instantiated where speed 4 runs (blocks up to 16x16, top-down); any other combination of switches runs the general kernels
static hipError_t launch_search(int maxbs, bool bottomup, int tools, const FrameDev *d_frames, const TileJob *d_jobs, const SbItem *d_items, int nitems, int *d_next, uint8_t *d_snap_pool, int *grid_out, int device, hipStream_t s) {
  if (nitems <= 0) { if (grid_out) *grid_out = 0; return hipSuccess; }
#define MI_LAUNCH_(MB, BU_, TS_) launch_search_t<MB, 4, BU_, TS_>(d_frames, d_jobs, d_items, nitems, d_next, d_snap_pool, grid_out, device, s)
#ifdef MI_FAST_BUILD                                     // experiment builds only (tools/build_variant.sh): the headline configuration's instantiation and nothing else
  return MI_LAUNCH_(2, false, 2);
#else
  const bool full = (tools & 1) != 0;
  if (maxbs <= 2 && !bottomup && tools == 2) return MI_LAUNCH_(2, false, 2);
  if (maxbs <= 2) return bottomup ? (full ? MI_LAUNCH_(2, true, 1) : MI_LAUNCH_(2, true, 0)) : (full ? MI_LAUNCH_(2, false, 1) : MI_LAUNCH_(2, false, 0));
  return bottomup ? (full ? MI_LAUNCH_(4, true, 1) : MI_LAUNCH_(4, true, 0)) : (full ? MI_LAUNCH_(4, false, 1) : MI_LAUNCH_(4, false, 0));
#endif
#undef MI_LAUNCH_
}
// K4, one instantiation per block-size class like K1 (jobs + first_job .. first_job + njobs of the grouped job list); the jobs must all belong to frames of the same class
template <int MAXBS, int NA> static hipError_t launch_entropy_t(const FrameDev *d_frames, const TileJob *d_jobs, int njobs, uint16_t *d_precarry, uint32_t pre_cap, uint32_t *d_recbuf, uint32_t rec_cap, hipStream_t s) {
  hipLaunchKernelGGL((tile_entropy_kernel<MAXBS, NA>), dim3(njobs), dim3(MI_K4_THREADS_OF(NA)), sizeof(EntropyLds<(MAXBS <= 2 ? 16 : 32)>), s, d_frames, d_jobs, njobs, d_precarry, pre_cap, d_recbuf, rec_cap);
  return hipGetLastError();
}
static hipError_t launch_entropy(int maxbs, const FrameDev *d_frames, const TileJob *d_jobs, int njobs, uint16_t *d_precarry, uint32_t pre_cap, uint32_t *d_recbuf, uint32_t rec_cap, hipStream_t s) {
  if (njobs <= 0) return hipSuccess;
#define MI_LAUNCH_(MB, NA_) launch_entropy_t<MB, NA_>(d_frames, d_jobs, njobs, d_precarry, pre_cap, d_recbuf, rec_cap, s)
#ifdef MI_FAST_BUILD                                     // experiment builds only (tools/build_variant.sh): the headline configuration's instantiation and nothing else
  return MI_LAUNCH_(2, MI_K4_ADAPTERS);
#else
  // a launch that leaves wave slots free (fewer than 512 tiles: 6 waves each still fit the device in one round) runs four adapter waves per tile
  const bool sparse = njobs < 512;
  if (maxbs <= 2) return sparse ? MI_LAUNCH_(2, MI_K4_ADAPTERS_SPARSE) : MI_LAUNCH_(2, MI_K4_ADAPTERS);
  return sparse ? MI_LAUNCH_(4, MI_K4_ADAPTERS_SPARSE) : MI_LAUNCH_(4, MI_K4_ADAPTERS);
#endif
#undef MI_LAUNCH_
}

// The work list of a set of tile jobs (grouped by block-size class, class_begin[2..5]) and the device objects a queue launch needs: the items, the claim
// counters (self-resetting: the last workgroup to leave a launch zeroes its pair), one snapshot area per persistent workgroup.
struct SearchQueue {
  std::vector<SbItem> items; int q_begin[6] = { 0, 0, 0, 0, 0, 0 };
  DevBuf<SbItem> d_items; PinBuf<SbItem> h_items; size_t items_cap = 0; DevBuf<int> d_next; DevBuf<uint8_t> d_snap; size_t snap_bytes = 0;
};
// The frame-level stages between the tile search and the entropy coder: K2a deblock level search -> level pick -> K2 deblock
// (vertical, horizontal edges) -> K3 CDEF -> K5 restoration.  ev_cdef (may be null) is recorded in front of CDEF.
static hipError_t launch_loop_filters(FrameDev *d_frames, int nframes, int max_mi_cells, int max_sb, int max_lr_units, hipStream_t s, hipEvent_t ev_cdef) {
  hipLaunchKernelGGL(deblock_tally_kernel, dim3((max_mi_cells + MI_DBK_CHUNK - 1) / MI_DBK_CHUNK, 6, nframes), dim3(256), 0, s, d_frames, nframes);
  hipLaunchKernelGGL(deblock_pick_kernel, dim3((nframes + 63) / 64), dim3(64), 0, s, d_frames, nframes);
  for (int pass = 0; pass < 2; pass++)
    hipLaunchKernelGGL(deblock_kernel, dim3((max_mi_cells + MI_DBK_CHUNK - 1) / MI_DBK_CHUNK, 3, nframes), dim3(256), 0, s, d_frames, nframes, pass);
  if (ev_cdef) { hipError_t e = hipEventRecord(ev_cdef, s); if (e != hipSuccess) return e; }
  hipLaunchKernelGGL(cdef_kernel, dim3(max_sb, nframes), dim3(256), 0, s, d_frames, 1);
  if (max_lr_units > 0) {
    hipLaunchKernelGGL(lr_search_kernel, dim3(max_lr_units, 3, nframes), dim3(256), 0, s, d_frames);
    hipLaunchKernelGGL(lr_kernel, dim3(max_lr_units, 3, nframes), dim3(256), 0, s, d_frames);
  }
  return hipGetLastError();
}

// Builds the launch's work list -- per block-size class, the superblocks of the class's tiles in (2 * row + column, job) order; jobs are indexed inside
// their class segment of d_jobs -- and enqueues one queue launch per class on `s`.
// the launches over a work list that is already on the device (the second pass of a two-pass encode reuses the first one's)
// every frame of a launch comes from one encoder configuration: which walker and which candidate set the kernels are instantiated for
// bit 0: bottom-up walker; bits 1..: the kernels' tool set (tile_search.h Tools).  The walker and the candidate set follow from the speed alone, the same for every frame of a
// launch; rdo_tx_decision also depends on the frame's quantiser (av1encoder.rs:576: `speed <= 4 && !high_quality`), and a launch holds the colour and the alpha frames of
// its pictures, each with its own quality: the kernels with the speed-4 switches as constants run only when EVERY frame of the launch has them.
static int search_mode(const std::vector<FramePlan> &frames) {
  if (frames.empty()) return 0;
  const mi_av1_config &c0 = frames[0].cfg;
  bool speed4_switches = true;
  for (const FramePlan &p : frames) {
    const mi_av1_config &c = p.cfg;
    speed4_switches = speed4_switches && !c.complex_pred_modes && c.rdo_tx_decision && c.reduced_tx_set && c.fine_directional_intra && !c.tune_psnr;   // (tx_mode_select follows from rdo_tx_decision)
  }
  return (c0.encode_bottomup != 0 ? 1 : 0) | (c0.complex_pred_modes != 0 ? 2 : 0) | (speed4_switches ? 4 : 0);
}
// The walker and the candidate set are template parameters of the launch (taken from frames[0]): every frame must agree on them.  They follow from the speed alone, which a
// batch shares, but mi_av1_config lets a caller override the resolved tweaks per call -- a mixed launch would run the wrong candidate set for some frames, silently.
static bool search_mode_consistent(const std::vector<FramePlan> &frames) {
  for (const FramePlan &p : frames)
    if ((p.cfg.encode_bottomup != 0) != (frames[0].cfg.encode_bottomup != 0) || (p.cfg.complex_pred_modes != 0) != (frames[0].cfg.complex_pred_modes != 0)) return false;
  return true;
}
static int search_launch(SearchQueue &q, int mode /* search_mode() */, const int class_begin[6], const FrameDev *d_frames, const TileJob *d_jobs, int device, hipStream_t s) {
  for (int cls = 2; cls <= 4; cls++)
    HIP_OK(launch_search(cls, (mode & 1) != 0, mode >> 1, d_frames, d_jobs + class_begin[cls], q.d_items.get() + q.q_begin[cls], q.q_begin[cls + 1] - q.q_begin[cls], q.d_next.get() + 2 * cls, q.d_snap.get(), nullptr, device, s));
  return MI_OK;
}
// the queue's device objects hold `nitems` work items and `snap_need` bytes of area snapshots (grown, never shrunk).  hipFree / hipMalloc wait for the device:
// a batch object reserves its worst case when it is made (search_reserve), so that an encode whose image count grows does not stall behind the other slots' kernels
static int queue_fit(SearchQueue &q, size_t nitems, size_t snap_need, hipStream_t s) {
  if (nitems > q.items_cap) { q.items_cap = nitems + nitems / 8; HIP_OK(q.d_items.alloc(q.items_cap)); HIP_OK(q.h_items.alloc(q.items_cap)); }
  if (!q.d_next.get()) { HIP_OK(q.d_next.alloc(16)); HIP_OK(hipMemsetAsync(q.d_next.get(), 0, 16 * sizeof(int), s)); }   // once: every launch leaves its pair zeroed
  if (snap_need > q.snap_bytes) { q.snap_bytes = snap_need; HIP_OK(q.d_snap.alloc(snap_need)); }
  return MI_OK;
}
// what the queue of a launch over `frames` needs at most: its work items and the bytes of area snapshots (host only: the grids are asked from the runtime, nothing is launched)
static int search_demand(const std::vector<FramePlan> &frames, int device, hipStream_t s, size_t &items, size_t &snap_need) {
  size_t per_class[5] = { 0, 0, 0, 0, 0 };
  items = snap_need = 0;
  for (const FramePlan &p : frames) { per_class[std::max(p.maxbs, 2)] += (size_t)p.sb_rows * p.sb_cols; items += (size_t)p.sb_rows * p.sb_cols; }
  const int mode = search_mode(frames);
  for (int cls = 2; cls <= 4; cls++) for (int tools : { mode >> 1, (mode >> 1) & ~2 }) {        // a run with fewer frames may run the other instantiation (search_mode)
    int grid = 0;
    HIP_OK(launch_search(cls, (mode & 1) != 0, tools, nullptr, nullptr, nullptr, (int)per_class[cls], nullptr, nullptr, &grid, device, s));
    snap_need = std::max(snap_need, (size_t)grid * k1_snap_bytes(cls));
  }
  return MI_OK;
}
static int search_reserve(SearchQueue &q, const std::vector<FramePlan> &frames, int device, hipStream_t s) {
  size_t items = 0, snap_need = 0;
  if (int st = search_demand(frames, device, s, items, snap_need)) return st;
  return queue_fit(q, items, snap_need, s);
}
static int search_enqueue(SearchQueue &q, const std::vector<FramePlan> &frames, const std::vector<TileJob> &jobs, const int class_begin[6], const FrameDev *d_frames, const TileJob *d_jobs, int device, hipStream_t s) {
  q.items.clear();
  size_t snap_need = 0;
  if (!search_mode_consistent(frames)) return MI_INVALID_ARGUMENT;
  const int mode = search_mode(frames);
  for (int cls = 2; cls <= 4; cls++) {
    q.q_begin[cls] = (int)q.items.size();
    // Synchronisation grain and list order.  Blocks up to 16x16 (classes below 4): per root block (tile_search.h root_wait / root_publish), where a superblock can start
    // ~0.75 of a superblock time after its left neighbour and ~1.125 after the one above; the list is ordered by 3 * row + 2 * column -- any a * row + b * column
    // with a > b > 0 lists a superblock after its left and its above-right neighbour, and 1.5 columns per row is the closest of the small ratios to what the roots
    // allow.  Until round 5 a full batch used whole-superblock flags and 2 * row + column: K1 106.6 -> 103.0 ms on 32 x 1080p, 121.1 -> 110.6 ms with 16 tiles per
    // image, where the longest tile's chain and not the device's throughput bounds the launch (profiles/r05zr_k1_sync_grain_and_order.txt).  64x64 superblocks
    // are their own roots: whole-superblock flags, two columns per row.
    const bool fine = cls < 4;
    const int key_a = fine ? 3 : 2, key_b = fine ? 2 : 1;
    std::vector<std::vector<SbItem>> by_key;
    for (int j = class_begin[cls]; j < class_begin[cls + 1]; j++) {
      const TileJob &tj = jobs[j]; const FramePlan &p = frames[tj.frame];
      const int rows = std::min(p.tiles.row_start[tj.tile_row + 1], p.sb_rows) - p.tiles.row_start[tj.tile_row];
      const int cols = std::min(p.tiles.col_start[tj.tile_col + 1], p.sb_cols) - p.tiles.col_start[tj.tile_col];
      if ((int)by_key.size() < key_a * rows + key_b * cols) by_key.resize(key_a * rows + key_b * cols);
      for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) by_key[key_a * r + key_b * c].push_back(SbItem{ (uint32_t)(j - class_begin[cls]), (uint16_t)r, (uint16_t)c });
    }
    for (auto &v : by_key) q.items.insert(q.items.end(), v.begin(), v.end());
    const int nitems = (int)q.items.size() - q.q_begin[cls];
    int grid = 0;
    HIP_OK(launch_search(cls, (mode & 1) != 0, mode >> 1, nullptr, nullptr, nullptr, nitems, nullptr, nullptr, &grid, device, s));
    if (fine) for (int i = q.q_begin[cls]; i < (int)q.items.size(); i++) q.items[i].job |= 0x80000000u;
    snap_need = std::max(snap_need, (size_t)grid * k1_snap_bytes(cls));
  }
  q.q_begin[5] = (int)q.items.size();
  if (int st = queue_fit(q, q.items.size(), snap_need, s)) return st;
  memcpy(q.h_items.get(), q.items.data(), q.items.size() * sizeof(SbItem));
  HIP_OK(hipMemcpyAsync(q.d_items.get(), q.h_items.get(), q.items.size() * sizeof(SbItem), hipMemcpyHostToDevice, s));
  return search_launch(q, mode, class_begin, d_frames, d_jobs, device, s);
}

#define MI_FRAME_RECORD_BYTES 32          /* reserved per (frame, plane) behind the frames' arenas (FrameSet::d_records) */
// ---- a set of frames on one device, ready to run: what mi_batch and mi_av1_encode_planes share ----
// reserve() once for the worst case, then per encode: fill `frames` (plan_geometry), place(), write the source planes, stage(), enqueue_chain(),
// enqueue_readback(), wait for the stream, check_lengths(), assemble().
struct FrameSet {
  int device = 0;
  std::vector<FramePlan> frames; std::vector<TileJob> jobs; int class_begin[6] = { 0, 0, 0, 0, 0, 0 };   // jobs grouped by block-size class (one K1 / K4 instantiation per class)
  DevBuf<uint8_t> d_arena; size_t arena_bytes = 0, aux_bytes = 0;       // aux: pre-carry units + symbol records
  DevBuf<FrameDev> d_frames; DevBuf<TileJob> d_jobs; DevBuf<uint16_t> d_precarry; uint32_t pre_cap = 0, pre_run = 0;   // pre-carry units per tile job: reserved (the worst case's largest tile), of the placed frames (theirs)
  DevBuf<uint32_t> d_recbuf; uint32_t rec_cap = 0;                      // K4's symbol records: three rotating superblock buffers per tile
  DevBuf<unsigned long long> d_prof;                                    // profiling builds: per tile job (K4) / per persistent workgroup (K1)
  PinBuf<FrameDev> h_frames; PinBuf<TileJob> h_jobs; PinBuf<uint32_t> h_lens; PinBuf<int> h_lf;   // pinned: H2D sources; tile lengths, deblock levels + segment indices (13 per frame)
  SearchQueue queue;
  size_t tiles_cap = 0, payload_worst = 0, frames_cap = 0;              // reserved: tile jobs, the sum of their output capacities, frames
  uint8_t *d_records = nullptr; size_t records_cap = 0;                 // MI_FRAME_RECORD_BYTES per (frame, plane) of the worst case, behind the frames' arenas: what a stage outside
                                                                        // the chain reports per plane (the quality metrics, dev_quality.h); never touched by an encode
  int max_mi_cells = 0, max_sb = 0, max_lr = 0, max_cells = 0, max_tiles = 1;   // launch maxima of the placed frames

  // What a set of planned frames asks of the objects reserve() makes: the one count behind reserve(), which sizes them, and fits(), which holds a set against them
  struct Demand { size_t arena = 0, tiles = 0, payload = 0, items = 0, snap = 0; uint32_t max_cap = 0; int max_np = 1; };
  static int demand(std::vector<FramePlan> &set, int dev, hipStream_t s, Demand &d) {
    d = Demand();
    for (auto &p : set) {
      const uint32_t cap = tile_capacity(p);
      d.arena += align_up(carve(p, nullptr, cap), 4096); d.tiles += (size_t)p.ntiles; d.max_cap = std::max(d.max_cap, cap); d.max_np = std::max(d.max_np, p.np);
      d.payload += (size_t)p.ntiles * cap;
    }
    return search_demand(set, dev, s, d.items, d.snap);
  }
  // allocates everything for the worst case `worst` (geometry planned): no (device-synchronising) reallocation inside an encode
  int reserve(std::vector<FramePlan> worst, int dev, hipStream_t s) {
    device = dev;
    Demand d;
    if (int st = demand(worst, dev, s, d)) return st;
    size_t total = d.arena; const uint32_t max_cap = d.max_cap;
    tiles_cap = d.tiles; payload_worst = d.payload; frames_cap = worst.size();
    pre_cap = pre_run = max_cap; rec_cap = MI_K4_SB_RECORDS(d.max_np);
    const size_t records_off = total;
    records_cap = worst.size() * 3; total += align_up(records_cap * MI_FRAME_RECORD_BYTES, 4096);
    arena_bytes = total; aux_bytes = tiles_cap * (size_t)max_cap * 2 + tiles_cap * 3 * (size_t)rec_cap * 4;
    const size_t prof_words = std::max<size_t>(tiles_cap, 2048) * 128;
    HIP_OK(d_arena.alloc(total));
    d_records = d_arena.get() + records_off;
    HIP_OK(d_frames.alloc(worst.size()));
    HIP_OK(d_jobs.alloc(tiles_cap));
    HIP_OK(d_precarry.alloc(tiles_cap * (size_t)max_cap));
    HIP_OK(d_recbuf.alloc(tiles_cap * 3 * (size_t)rec_cap));
    HIP_OK(d_prof.alloc(prof_words)); HIP_OK(hipMemset(d_prof.get(), 0, prof_words * 8));
    HIP_OK(h_lens.alloc(tiles_cap));
    HIP_OK(h_lf.alloc(worst.size() * 13));
    HIP_OK(h_frames.alloc(worst.size()));
    HIP_OK(h_jobs.alloc(tiles_cap));
    return queue_fit(queue, d.items, d.snap, s);
  }
  // `set` (geometry planned) runs in what reserve() made: the frames' arenas stay in front of the records, and every quantity reserve() sized for its worst case
  // holds the set's -- frames, tile jobs, payload capacities, the jobs' pre-carry units (one stride for all jobs: the largest tile capacity) and symbol records,
  // the queue's items and snapshots.  Allocates and launches nothing
  bool fits(std::vector<FramePlan> set, hipStream_t s) const {
    Demand d;
    if (set.empty() || demand(set, device, s, d) != MI_OK) return false;
    const size_t records_off = arena_bytes - align_up(records_cap * MI_FRAME_RECORD_BYTES, 4096);
    return set.size() <= frames_cap && d.arena <= records_off && d.tiles <= tiles_cap && d.payload <= payload_worst && d.tiles * (size_t)d.max_cap <= tiles_cap * (size_t)pre_cap &&
           MI_K4_SB_RECORDS(d.max_np) <= rec_cap && d.items <= queue.items_cap && d.snap <= queue.snap_bytes;
  }
  // carves the arena for `frames`, fills their descriptors, builds the grouped job list (tile_base indexes it) and the launch maxima; host only
  void place() {
    const DeviceTables &tab = g_tabs[device];
    size_t off = 0;
    for (auto &p : frames) { p.arena = d_arena.get() + off; p.arena_bytes = carve(p, p.arena, tile_capacity(p)); off += align_up(p.arena_bytes, 4096); fill_dev(p, tab); }
    jobs.clear();
    for (int cls = 2; cls <= 4; cls++) {
      class_begin[cls] = (int)jobs.size();
      for (size_t k = 0; k < frames.size(); k++) {
        FramePlan &p = frames[k];
        if (std::max(p.maxbs, 2) != cls) continue;
        p.dev.tile_base = (int)jobs.size();
        p.dev.prof_out = d_prof.get();
        for (int tr = 0; tr < p.tiles.rows; tr++) for (int tc = 0; tc < p.tiles.cols; tc++) jobs.push_back(TileJob{ (int)k, tr, tc });
      }
    }
    class_begin[5] = (int)jobs.size();
    max_mi_cells = max_sb = max_lr = max_cells = 0; max_tiles = 1; pre_run = 0;
    for (const FramePlan &p : frames) {
      pre_run = std::max(pre_run, p.dev.tile_out_cap);
      max_mi_cells = std::max(max_mi_cells, p.mi_cols * p.mi_rows * 4); max_sb = std::max(max_sb, p.sb_cols * p.sb_rows);
      max_cells = std::max(max_cells, (p.pw / 8) * (p.ph / 8)); max_tiles = std::max(max_tiles, p.ntiles);
      if (p.cfg.lrf) max_lr = std::max(max_lr, lr_units_host(p.cfg.width) * lr_units_host(p.cfg.height));
    }
  }
  // frame descriptors and tile jobs to the device, through the pinned mirrors: the copies never block the host
  int stage(hipStream_t s) {
    for (size_t k = 0; k < frames.size(); k++) h_frames.get()[k] = frames[k].dev;
    memcpy(h_jobs.get(), jobs.data(), sizeof(TileJob) * jobs.size());
    HIP_OK(hipMemcpyAsync(d_frames.get(), h_frames.get(), sizeof(FrameDev) * frames.size(), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(d_jobs.get(), h_jobs.get(), sizeof(TileJob) * jobs.size(), hipMemcpyHostToDevice, s));
    return MI_OK;
  }
  // activity mask (Tune::Psychovisual) -> K1 tile search -> K2a/K2 deblock (level search + filter), K3 CDEF, K5 restoration -> K4 entropy coding.
  // A two-pass encode (rdo_passes = 2) runs the chain twice: between the passes every tile's final CDFs become its rate table, the frames switch
  // over to them, and the activity kernel clears the per-encode state again.  ev (may be null): ev[1] is recorded in front of the tile search,
  // ev[2] behind it, ev[3] in front of CDEF, ev[4] in front of the entropy coder; they time the last pass.
  int enqueue_chain(hipStream_t s, hipEvent_t *ev) {
    const int nframes = (int)frames.size();
    const int passes = frames[0].cfg.rdo_passes == 2 ? 2 : 1;
    for (int pass = 0; pass < passes; pass++) {
      if (pass == 1) {
        hipLaunchKernelGGL(cdf_cost_kernel, dim3(max_tiles, nframes), dim3(256), 0, s, d_frames.get());
        hipLaunchKernelGGL(pass_flip_kernel, dim3((nframes + 63) / 64), dim3(64), 0, s, d_frames.get(), nframes);
      }
      hipLaunchKernelGGL(activity_kernel, dim3((max_cells + 255) / 256, nframes), dim3(256), 0, s, d_frames.get());
      hipLaunchKernelGGL(segment_kernel, dim3(nframes), dim3(256), 0, s, d_frames.get());
      if (ev) HIP_OK(hipEventRecord(ev[1], s));
      if (pass == 0) { if (int st = search_enqueue(queue, frames, jobs, class_begin, d_frames.get(), d_jobs.get(), device, s)) return st; }
      else if (int st = search_launch(queue, search_mode(frames), class_begin, d_frames.get(), d_jobs.get(), device, s)) return st;
      if (ev) HIP_OK(hipEventRecord(ev[2], s));
      HIP_OK(launch_loop_filters(d_frames.get(), nframes, max_mi_cells, max_sb, max_lr, s, ev ? ev[3] : nullptr));
      if (ev) HIP_OK(hipEventRecord(ev[4], s));
      for (int cls = 2; cls <= 4; cls++)
        HIP_OK(launch_entropy(cls, d_frames.get(), d_jobs.get() + class_begin[cls], class_begin[cls + 1] - class_begin[cls], d_precarry.get() + (size_t)class_begin[cls] * (size_t)pre_run, pre_run,
                              d_recbuf.get() + (size_t)class_begin[cls] * 3 * (size_t)rec_cap, rec_cap, s));
    }
    HIP_OK(hipGetLastError());
    return MI_OK;
  }
  // tile lengths (indexed like `jobs`) and the 13 ints of every frame's lf_out into the pinned mirrors
  int enqueue_readback(hipStream_t s) {
    for (size_t k = 0; k < frames.size(); k++) {
      const FramePlan &p = frames[k];
      HIP_OK(hipMemcpyAsync(h_lens.get() + p.dev.tile_base, p.dev.tile_len, (size_t)p.ntiles * 4, hipMemcpyDeviceToHost, s));
      HIP_OK(hipMemcpyAsync(h_lf.get() + 13 * k, p.dev.lf_out, 13 * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    return MI_OK;
  }
  // after the readback has arrived: K4 reports a tile that did not fit (or whose search gave up) as length 0xFFFFFFFF
  int check_lengths() const {
    for (size_t j = 0; j < jobs.size(); j++)
      if (h_lens.get()[j] == 0xFFFFFFFFu) { fprintf(stderr, "mi_avif: tile %d overflowed its output buffer (or its frame's tile search gave up waiting for a neighbour)\n", (int)j); return MI_ENCODING_ERROR; }
    return MI_OK;
  }
  // frame k's OBUs from its tile payloads (host pointers; tile t has length h_lens[tile_base + t]) and the levels the device picked
  void assemble(size_t k, const std::vector<const uint8_t *> &tile_data) {
    FramePlan &p = frames[k];
    std::vector<std::pair<const uint8_t *, size_t>> tl;
    for (int t = 0; t < p.ntiles; t++) tl.push_back({ tile_data[t], (size_t)h_lens.get()[p.dev.tile_base + t] });
    static_assert(offsetof(FrameHeaderInfo, seg_n) == offsetof(FrameHeaderInfo, lf_level) + 4 * sizeof(int) && offsetof(FrameHeaderInfo, seg_qidx) == offsetof(FrameHeaderInfo, seg_n) + sizeof(int),
                  "FrameDev::lf_out reports 13 ints: lf_level[4], seg_n, seg_qidx[8]");
    memcpy((char *)&p.hdr + offsetof(FrameHeaderInfo, lf_level), h_lf.get() + 13 * k, 13 * sizeof(int));
    p.obu = assemble_obus(p.hdr, tl);
  }
};
}  // namespace mi
