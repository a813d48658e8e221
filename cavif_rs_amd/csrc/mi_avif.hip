// mi_avif.hip -- the entry points of include/mi_avif.h: the batch object (pixels and staging, K0 front end, pack + D2H, AVIF containers, timing), its
// pool, the JPEG decode contexts, the stream worker and the level-1 plane encoder.  The frame chain they all run (plans, arena, K1 tile search, K2 deblock,
// K3 CDEF, K5 restoration, K4 tile entropy coding, readback) is host_frames.h.  One HIP stream per batch, no hidden device syncs
// other than the two points where the host needs device results (alpha flags, tile lengths).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <condition_variable>
#include <memory>
#include <thread>
#include <atomic>
#include <future>
#include <chrono>
#include <exception>
#include <algorithm>
#include "host_av1.h"
#include "png_reader.h"
#include "jpeg_reader.h"
#include "dev_jpeg.h"
#include "dev_png.h"
#include "dev_planes.h"
#include "dev_resample.h"
#include "dev_quality.h"
#include "dev_decoded.h"
#include "dev_deep.h"
#include "host_frames.h"

// The product library reads no environment variables; probe builds (tools/) get MI_AVIF_TIMING=1 (-DMI_TUNING_KNOBS: host-side timeline on stderr)
// and MI_DEBUG_LEVEL (-DMI_DEBUG_HOOKS=1: bisect levels of the tile search).
// the streaming form's rotation: resident batch objects per image shape, and the first run's share of a full run
#ifndef MI_STREAM_SLOTS_DEFAULT
#define MI_STREAM_SLOTS_DEFAULT 2          /* 256 x 1080p files end to end: 1.32 s with two, 1.48 with three, 1.51 with four (profiles/r05zk_e2e_knobs.txt, matrix 5) */
#endif
#define MI_STREAM_FIRST_RUN_NUM 1         /* a worker's first run as a share of a full one: a whole run (a half run started the GPU ~0.03 s earlier and cost two runs of 16 images, */
#define MI_STREAM_FIRST_RUN_DEN 1         /* 0.09 s of tile search each against 0.10 for 32: worker phase 1.24 -> 1.20 s on 256 files, profiles/r05zk_e2e_knobs.txt matrix 6) */
static inline bool mi_timing_enabled() {
#ifdef MI_TUNING_KNOBS
  static const bool on = getenv("MI_AVIF_TIMING") != nullptr; return on;
#else
  return false;
#endif
}

using namespace mi;

// ================================================================ batch object
struct mi_batch {
  mi_ravif_encoder enc{}; int n = 0; uint32_t w = 0, h = 0; int channels = 3, device = 0, depth = 10;
  std::vector<uint8_t> exif;                                       // the batch's own copy of enc.exif (the caller's buffer need not outlive mi_batch_create)
  hipStream_t stream = nullptr;
  int cap = 0;                                                     // images the batch was created for (n = images of the current run <= cap)
  DevBuf<uint8_t> d_pixels; size_t pixel_bytes = 0;               // cap * w*h*channels
  std::mutex staging_mu; PinBuf<uint8_t> h_pixels;                                        // pinned staging of the same size: the H2D source (async, no pageable copies); made by the first mi_batch_input (a batch fed
                                                                   // JPEG coefficients, PNG scanlines or device pixels alone never pins it: pinning and unpinning 265 MB costs ~0.1 s)
  DevBuf<int> d_alpha_flags; PinBuf<int> h_alpha; std::vector<int> alpha_flags;      // h_alpha: pinned D2H target
  DevBuf<uint8_t> d_clean, d_clean_tmp; DevBuf<unsigned long long> d_alpha_acc;       // dirty-alpha cleaner (RGBA, UnassociatedClean)
  FrameSet fs;                                                     // frames: colour frames [0..n), alpha frames after
  DevBuf<uint32_t> d_offsets; DevBuf<uint8_t> d_packed; PinBuf<uint8_t> h_packed; size_t packed_cap = 0, packed_max = 0;   // the tile payloads, compacted (pinned twin: one D2H)
  std::vector<std::vector<uint8_t>> files; std::vector<size_t> color_sz, alpha_sz;
  hipEvent_t ev[8]{}; double stage_ms[8]{};
  bool in_flight = false;
  // device-resident input (made on the first use): the event a producer's stream is joined through, and the JPEG staging -- quantisation tables + coefficients
  // of the images uploaded since the stream last drained, pinned and on the device, and one image's component planes
  hipEvent_t ev_src = nullptr;
  PinBuf<uint8_t> h_jpeg; DevBuf<uint8_t> d_jpeg, d_jpeg_planes; size_t h_jpeg_cap = 0, d_jpeg_cap = 0, d_jpeg_planes_cap = 0, jpeg_used = 0;
  // PNG staging: descriptors + palettes + inflated scanlines of the mi_batch_upload_png calls since the stream last drained, pinned and on the device (unfiltered there in place)
  PinBuf<uint8_t> h_png; DevBuf<uint8_t> d_png; size_t h_png_cap = 0, d_png_cap = 0, png_used = 0;
  // resize on input: the per-axis tables (bounds + taps) of the mi_batch_resize_* calls since the stream last drained, pinned and on the device, the last call's
  // kept for the next one of the same sizes and filter; one device scratch for a decoded JPEG / PNG source and the intermediate of the two passes
  PinBuf<uint8_t> h_rs; DevBuf<uint8_t> d_rs, d_rs_scratch; size_t h_rs_cap = 0, d_rs_cap = 0, rs_used = 0, d_rs_scratch_cap = 0;
  uint32_t rs_key[5] = { 0, 0, 0, 0, 0 }; size_t rs_key_at = 0;     // src_w, src_h, dst_w, dst_h, filter + 1 of the tables at rs_key_at (0 in [4]: none)
  // quality metrics (mi_batch_measure): `encoded` = the planes of a completed encode of the current image count are on the device, `measured` = h_quality holds
  // that encode's records.  The records live at the end of the arena (FrameSet::d_records); their pinned D2H target is made by the first measure.
  bool encoded = false, measured = false;
  PinBuf<QualityRec> h_quality; size_t h_quality_bytes = 0;
  // decoded pixels (mi_batch_decode): one image of w*h*4 bytes on the device, made by the first call that decodes into host memory
  DevBuf<uint8_t> d_decoded; size_t d_decoded_cap = 0;
  // what the bytes of each input slot mean (MI_INPUT_RGB / MI_INPUT_YCBCR): host state, set by whichever call last filled the slot, kept across encodes and
  // mi_batch_set_count like the slot's contents
  std::vector<uint8_t> kinds;
  // deep input: the slots of kind MI_INPUT_RGB16, cap * w*h*channels uint16 samples laid out like d_pixels; made by the first call that needs
  // them (under staging_mu), never by a batch that sees no 16-bit source
  DevBuf<uint16_t> d_pixels16; size_t deep_bytes = 0;
};
static void batch_tag(mi_batch *b, int first, int count, int kind) { std::fill(b->kinds.begin() + first, b->kinds.begin() + first + count, (uint8_t)kind); }
// MI_INPUT_YCBCR needs the YCbCr colour model (the planes are the slot's bytes) and, in a 4-channel batch, an alpha mode that leaves opaque pixels alone
static bool batch_takes_ycbcr(const mi_batch *b) { return b->enc.color_model != 1 && !(b->channels == 4 && b->enc.alpha_mode == 2); }
// MI_INPUT_RGB16: the dirty-alpha cleaner and the premultiply branch are defined on 8-bit samples, so a 4-channel batch takes a deep source with an alpha channel
// under UnassociatedDirty alone and an opaque one (A = 65535: the cleaner skips it as it skips MI_INPUT_YCBCR) under both unassociated modes; a 3-channel batch takes 3 channels
static bool batch_takes_deep(const mi_batch *b, int src_channels) {
  if (src_channels != 3 && src_channels != 4) return false;
  if (b->channels == 3) return src_channels == 3;
  return src_channels == 4 ? b->enc.alpha_mode == 0 : b->enc.alpha_mode != 2;
}
// the deep slots, made on first use; nullptr = could not be allocated
static uint16_t *batch_deep(mi_batch *b) {
  std::lock_guard<std::mutex> lk(b->staging_mu);
  if (!b->d_pixels16.get()) {
    (void)hipSetDevice(b->device);
    if (b->d_pixels16.alloc(b->pixel_bytes) != hipSuccess) return nullptr;
    b->deep_bytes = b->pixel_bytes * sizeof(uint16_t);
  }
  return b->d_pixels16.get();
}
static_assert(sizeof(QualityRec) <= MI_FRAME_RECORD_BYTES, "FrameSet reserves MI_FRAME_RECORD_BYTES per (frame, plane)");

static void batch_plan(mi_batch *b) {
  // (re)build frame plans: colour for every image [0, n), then (RGBA input) one alpha frame per image [n, 2n) -- whether an alpha
  // frame is used is decided on the device (FrameDev::active)
  b->fs.frames.clear();
  const int quantizer = quality_to_quantizer(b->enc.quality), aquant = quality_to_quantizer(b->enc.alpha_quality);
  auto make = [&](int image, bool alpha) {
    FramePlan p; p.image = image; p.is_alpha = alpha;
    mi_av1_config &c = p.cfg;
    c.width = b->w; c.height = b->h; c.bit_depth = (uint8_t)b->depth; c.quantizer = (uint8_t)(alpha ? aquant : quantizer);
    c.chroma = alpha ? 1 : 0; c.pixel_range = 1; c.threads = b->enc.threads; c.device = b->device; c.tiles_override = b->enc.tiles_override; c.rdo_passes = (uint8_t)(b->enc.rdo_passes == 2 ? 2 : 1);
    c.has_color_desc = alpha ? 0 : 1; c.primaries = 1; c.transfer = 13; c.matrix = b->enc.color_model == 1 ? 0 : 6;
    tweaks_from_preset(b->enc.speed, c.quantizer, &c);
    plan_geometry(p);
    return p;
  };
  for (int i = 0; i < b->n; i++) b->fs.frames.push_back(make(i, false));
  if (b->channels == 4) for (int i = 0; i < b->n; i++) b->fs.frames.push_back(make(i, true));
}

// allocate for the worst case: every image has an alpha frame when channels == 4
static int batch_alloc(mi_batch *b) {
  batch_plan(b);
  if (int st = b->fs.reserve(b->fs.frames, b->device, b->stream)) return st;
  HIP_OK(b->d_offsets.alloc(b->fs.tiles_cap));
  // Packed payloads: the worst case is the sum of the tile capacities (raw size, hundreds of MB of pinned memory per batch), the
  // usual case a few per cent of it: start at 1/16 and let mi_batch_wait grow the pair when a run needs more.
  b->packed_max = std::min<size_t>(b->fs.payload_worst, (size_t)1 << 31);
  b->packed_cap = std::min(b->packed_max, align_up(std::max<size_t>(b->fs.payload_worst / 16, (size_t)1 << 20), 4096));
  HIP_OK(b->d_packed.alloc(b->packed_cap));
  HIP_OK(b->h_packed.alloc(b->packed_cap));
  HIP_OK(b->h_alpha.alloc(b->cap));
  return MI_OK;
}

extern "C" {

const char *mi_version(void) { return "mi_avif 0.1 (gfx950)"; }
int mi_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
void mi_free(void *p) { free(p); }
int mi_quality_to_quantizer(float q) { return quality_to_quantizer(q); }
int mi_av1_tweaks_from_preset(uint8_t speed, uint8_t quantizer, mi_av1_config *cfg) { if (!cfg) return MI_INVALID_ARGUMENT; return tweaks_from_preset(speed, quantizer, cfg); }
void mi_rgb_to_ycbcr(const uint8_t rgb[3], int depth, uint16_t out[3]) { rgb_to_ycbcr_host(rgb, depth, out); }

void mi_ravif_encoder_default(mi_ravif_encoder *e) {     // Encoder::new, ravif/src/av1encoder.rs:88-102
  memset(e, 0, sizeof(*e));
  e->quality = 80.f; e->alpha_quality = 80.f; e->speed = 5; e->color_model = 0; e->depth = 0; e->alpha_mode = 1; e->threads = 0; e->device = 0;
}

size_t mi_avif_serialize(const uint8_t *color, size_t color_len, const uint8_t *alpha, size_t alpha_len, uint32_t w, uint32_t h,
                         uint8_t depth, uint8_t matrix, int premultiplied, const uint8_t *exif, size_t exif_len, uint8_t **out) {
  std::vector<uint8_t> v = avif_container(color, color_len, alpha, alpha_len, w, h, depth, matrix, premultiplied != 0, exif, exif_len);
  *out = (uint8_t *)malloc(v.size()); memcpy(*out, v.data(), v.size());
  return v.size();
}

// The filters address samples inside a plane with 32-bit offsets (row * stride + column): a padded plane must stay below 2^31 samples.  That is 60 x the largest picture
// any AV1 level allows (level 6.x: 35.6 MPix); beyond it the entry points answer MI_INVALID_ARGUMENT instead of filtering the wrong samples.
static bool mi_plane_too_large(uint32_t w, uint32_t h) {
  const uint64_t pw = ((uint64_t)w + 63) & ~63ull, ph = ((uint64_t)h + 63) & ~63ull;
  return (pw + 64) * (ph + 64) >= (1ull << 31);
}
mi_batch *mi_batch_create(const mi_ravif_encoder *e, int n_images, uint32_t w, uint32_t h, int channels) {
  if (!e || n_images < 1 || w < 1 || h < 1 || w > 65536 || h > 65536 || (channels != 3 && channels != 4) || e->alpha_mode > 2) return nullptr;
  if (mi_plane_too_large(w, h)) return nullptr;
  if (e->speed < 1 || e->speed > 10 || !(e->quality >= 1.f && e->quality <= 100.f) || !(e->alpha_quality >= 1.f && e->alpha_quality <= 100.f)) return nullptr;
  if (mi_device_count() <= e->device) { fprintf(stderr, "mi_avif: no HIP device %d (the HIP path is mandatory; there is no CPU fallback)\n", e->device); return nullptr; }
  if (hipSetDevice(e->device) != hipSuccess) return nullptr;
  const bool timing = mi_timing_enabled();
  const auto t0 = std::chrono::steady_clock::now();
  auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3; };
  mi_batch *b = new mi_batch();
  b->enc = *e; b->n = b->cap = n_images; b->w = w; b->h = h; b->channels = channels; b->device = e->device; b->depth = e->depth == 8 ? 8 : 10;
  if (e->exif && e->exif_len) b->exif.assign(e->exif, e->exif + e->exif_len);
  b->enc.exif = b->exif.empty() ? nullptr : b->exif.data(); b->enc.exif_len = b->exif.size();
  b->alpha_flags.assign(n_images, 0);
  b->kinds.assign(n_images, MI_INPUT_RGB);
  b->pixel_bytes = (size_t)n_images * w * h * channels;
  bool ok = hipStreamCreate(&b->stream) == hipSuccess && b->d_pixels.alloc(b->pixel_bytes) == hipSuccess &&
            b->d_alpha_flags.alloc(n_images) == hipSuccess;
  if (ok && channels == 4 && e->alpha_mode == 1)
    ok = b->d_clean.alloc(b->pixel_bytes) == hipSuccess && b->d_clean_tmp.alloc((size_t)w * h * 4) == hipSuccess && b->d_alpha_acc.alloc((size_t)4 * n_images) == hipSuccess;
  if (ok && channels == 4 && e->alpha_mode == 2) ok = b->d_clean.alloc(b->pixel_bytes) == hipSuccess;   // premultiplied pixels
  for (int i = 0; i < 8 && ok; i++) ok = hipEventCreate(&b->ev[i]) == hipSuccess;
  const double t_px = since();
  if (ok) ok = batch_alloc(b) == MI_OK;
  const double t_arena = since();
  if (ok) ok = ensure_tables(e->device) == MI_OK;              // last: a caller may be warming the device up on another thread meanwhile
  if (timing) fprintf(stderr, "[mi_avif] batch_create %d x %ux%u: pixels + pinned staging %.1f ms, arena (%.2f GB) %.1f ms, tables %.1f ms\n", n_images, w, h, t_px, b->fs.arena_bytes / 1e9, t_arena - t_px, since() - t_arena);
  if (!ok) { mi_batch_destroy(b); return nullptr; }
  b->files.resize(n_images); b->color_sz.assign(n_images, 0); b->alpha_sz.assign(n_images, 0);
  return b;
}

// The batch owns a pinned host staging area laid out like its HBM input slot; H2D always starts from there.
uint8_t *mi_batch_input(mi_batch *b, int index) {
  if (!b || index < 0 || index >= b->cap) return nullptr;
  {                                                           // made once, by whichever thread asks first (callers may fill different slots from different threads)
    std::lock_guard<std::mutex> lk(b->staging_mu);
    if (!b->h_pixels.get()) { (void)hipSetDevice(b->device); if (b->h_pixels.alloc(b->pixel_bytes) != hipSuccess) return nullptr; }
  }
  return b->h_pixels.get() + (size_t)index * b->w * b->h * b->channels;
}
int mi_batch_set_count(mi_batch *b, int n_images) {
  if (!b || b->in_flight || n_images < 1 || n_images > b->cap) return MI_INVALID_ARGUMENT;
  b->n = n_images; b->alpha_flags.assign(n_images, 0);
  b->encoded = b->measured = false;
  return MI_OK;
}
// enqueue the H2D of images [first, first + count) from the pinned staging on the batch's stream; returns at once
int mi_batch_upload_async(mi_batch *b, int first, int count) {
  if (!b || first < 0 || count < 1 || first + count > b->cap || !mi_batch_input(b, first)) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  const size_t img = (size_t)b->w * b->h * b->channels;
  HIP_OK(hipMemcpyAsync(b->d_pixels.get() + first * img, b->h_pixels.get() + first * img, count * img, hipMemcpyHostToDevice, b->stream));
  batch_tag(b, first, count, MI_INPUT_RGB);
  return MI_OK;
}
int mi_batch_set_input_kind(mi_batch *b, int first, int count, int kind) {
  if (!b || b->in_flight || first < 0 || count < 1 || first > b->cap - count || (kind != MI_INPUT_RGB && kind != MI_INPUT_YCBCR && kind != MI_INPUT_RGB16)) return MI_INVALID_ARGUMENT;
  if (kind == MI_INPUT_YCBCR && !batch_takes_ycbcr(b)) return MI_INVALID_ARGUMENT;
  // kind 2 tags what a HIP caller wrote through mi_batch_device_input16, the call that makes the deep slots: a batch without them has nothing to tag (and the
  // set call allocates nothing); the slot may hold any alpha
  if (kind == MI_INPUT_RGB16) {
    if (!batch_takes_deep(b, b->channels)) return MI_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lk(b->staging_mu);
    if (!b->d_pixels16.get()) return MI_INVALID_ARGUMENT;
  }
  batch_tag(b, first, count, kind);
  return MI_OK;
}
int mi_batch_input_kind(mi_batch *b, int index, int *kind) {
  if (!b || !kind || index < 0 || index >= b->cap) return MI_INVALID_ARGUMENT;
  *kind = b->kinds[index];
  return MI_OK;
}
int mi_batch_upload(mi_batch *b, int index, const uint8_t *pixels, size_t stride_px) {
  if (!b || index < 0 || index >= b->cap || !pixels) return MI_INVALID_ARGUMENT;
  const size_t row = (size_t)b->w * b->channels;
  uint8_t *dst = mi_batch_input(b, index);
  if (!dst) return MI_ENCODING_ERROR;
  for (uint32_t y = 0; y < b->h; y++) memcpy(dst + y * row, pixels + (size_t)y * stride_px * b->channels, row);
  if (int st = mi_batch_upload_async(b, index, 1)) return st;
  HIP_OK(hipStreamSynchronize(b->stream));
  return MI_OK;
}

// debug/profiling: per-tile [K1 start, K1 end, K4 start, K4 end] ticks of the last encode; out must hold 4*num_tiles values
int mi_batch_tile_clocks(mi_batch *b, unsigned long long *out) {
  if (!b || !out) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  for (auto &p : b->fs.frames) HIP_OK(hipMemcpy(out + (size_t)p.dev.tile_base * 4, p.dev.tile_clk, (size_t)p.ntiles * 32, hipMemcpyDeviceToHost));
  return MI_OK;
}
// profiling builds (MI_PROFILE=1): K1 phase cycle counters, 64 values per tile job of the last encode
int mi_batch_phase_profile(mi_batch *b, unsigned long long *out) {
  if (!b || !out || !b->fs.d_prof.get()) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  HIP_OK(hipMemcpy(out, b->fs.d_prof.get(), std::max<size_t>(b->fs.jobs.size(), 2048) * 128 * 8, hipMemcpyDeviceToHost));     // rows: tile jobs (K4) or persistent workgroups (K1: up to the resident grid); unused rows are zero
  return MI_OK;
}
int mi_batch_num_tiles(const mi_batch *b) { return b ? (int)b->fs.jobs.size() : 0; }
double mi_batch_stage_ms(const mi_batch *b, int stage) { return (b && stage >= 0 && stage < 8) ? b->stage_ms[stage] : 0.0; }

// Enqueues the GPU part of the hot path (K0..K4 + tile-length readback) on the batch's stream and returns.
int mi_batch_encode_async(mi_batch *b) {
  if (!b) return MI_INVALID_ARGUMENT;
  if (b->in_flight) return MI_INVALID_ARGUMENT;
  b->encoded = b->measured = false;
  (void)hipSetDevice(b->device);
  hipStream_t s = b->stream;
  uint8_t *const d_pixels = b->d_pixels.get(), *const d_clean = b->d_clean.get(), *const d_clean_tmp = b->d_clean_tmp.get();
  int *const d_alpha_flags = b->d_alpha_flags.get(); unsigned long long *const d_alpha_acc = b->d_alpha_acc.get();
  // ---- plan colour frames and, for RGBA input, an alpha frame per image (idle on the device unless the front end flags the image)
  batch_plan(b);
  b->fs.place();
  // ---- K0 front end: RGBA8 -> planes (+ alpha plane into a staging slot at the end of the colour frame's fin[] planes)
  HIP_OK(hipEventRecord(b->ev[0], s));
  HIP_OK(hipMemsetAsync(d_alpha_flags, 0, sizeof(int) * b->n, s));
  const FrontConsts fc = front_consts(b->depth);
  FrontParams fp{ fc.sy_r, fc.sy_g, fc.sy_b, fc.scale, fc.kcb, fc.kcr, fc.shift, b->depth, b->enc.color_model, b->channels, 0 };
  const uint8_t *front_src = d_pixels;
  if (d_clean && b->enc.alpha_mode == 2) {                  // convert_alpha_8bit: Premultiplied (av1encoder.rs:282-296)
    const size_t npx = (size_t)b->n * b->w * b->h;
    hipLaunchKernelGGL(premultiply_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s, d_pixels, d_clean, npx);
    HIP_OK(hipGetLastError());
    front_src = d_clean;
  } else if (d_clean) {                                     // convert_alpha_8bit: UnassociatedClean (av1encoder.rs:277-281)
    HIP_OK(hipMemsetAsync(d_alpha_acc, 0, sizeof(unsigned long long) * 4 * b->n, s));
    const dim3 g((b->w + 255) / 256, b->h), blk(256);
    for (int i = 0; i < b->n; i++) {
      if (b->kinds[i] != MI_INPUT_RGB) continue;                // opaque (YCbCr, or a deep image with A = 65535): the passes would be copies; the front end reads the slot itself
      const uint8_t *in = d_pixels + (size_t)i * b->w * b->h * 4; uint8_t *outp = d_clean + (size_t)i * b->w * b->h * 4;
      hipLaunchKernelGGL(alpha_scan_kernel, g, blk, 0, s, in, (int)b->w, (int)b->h, d_alpha_acc + 4 * i);
      hipLaunchKernelGGL(alpha_rewrite_kernel, g, blk, 0, s, in, d_clean_tmp, (int)b->w, (int)b->h, d_alpha_acc + 4 * i, 0);
      hipLaunchKernelGGL(alpha_rewrite_kernel, g, blk, 0, s, (const uint8_t *)d_clean_tmp, outp, (int)b->w, (int)b->h, d_alpha_acc + 4 * i, 1);
    }
    HIP_OK(hipGetLastError());
    front_src = d_clean;
  }
  for (int i = 0; i < b->n; i++) {
    FramePlan &p = b->fs.frames[i];
    uint16_t *alpha_stage = b->channels == 4 ? p.dev.fin[0] : nullptr;      // fin[0] is free until CDEF runs
    if (b->kinds[i] == MI_INPUT_RGB16) {                        // its deep slot, through the 16-bit front end
      const uint16_t *deep = b->d_pixels16.get();
      if (!deep) return MI_INVALID_ARGUMENT;
      deep += (size_t)i * b->w * b->h * b->channels;
      const FrontDeepParams dp{ b->depth, b->enc.color_model };
      if (b->channels == 4) hipLaunchKernelGGL((frontend_deep_kernel<4>), dim3((p.pw + 255) / 256, p.ph), dim3(256), 0, s, deep, (int)b->w, (int)b->h, dp,
                                               p.dev.src[0], p.dev.src[1], p.dev.src[2], alpha_stage, p.pw, p.ph, d_alpha_flags + i);
      else hipLaunchKernelGGL((frontend_deep_kernel<3>), dim3((p.pw + 255) / 256, p.ph), dim3(256), 0, s, deep, (int)b->w, (int)b->h, dp,
                              p.dev.src[0], p.dev.src[1], p.dev.src[2], alpha_stage, p.pw, p.ph, d_alpha_flags + i);
      continue;
    }
    fp.ycc = b->kinds[i] == MI_INPUT_YCBCR;
    hipLaunchKernelGGL(frontend_kernel, dim3((p.pw + 255) / 256, p.ph), dim3(256), 0, s,
                       (fp.ycc ? d_pixels : front_src) + (size_t)i * b->w * b->h * b->channels, (int)b->w, (int)b->h, (int)b->w, fp,
                       p.dev.src[0], p.dev.src[1], p.dev.src[2], alpha_stage, p.pw, p.ph, d_alpha_flags + i);
  }
  HIP_OK(hipGetLastError());
  if (b->channels == 4) {
    HIP_OK(hipMemcpyAsync(b->h_alpha.get(), d_alpha_flags, sizeof(int) * b->n, hipMemcpyDeviceToHost, s));    // read in mi_batch_wait
    for (size_t k = b->n; k < b->fs.frames.size(); k++) {
      FramePlan &a = b->fs.frames[k], &col = b->fs.frames[a.image];
      a.dev.active = d_alpha_flags + a.image;
      HIP_OK(hipMemcpyAsync(a.dev.src[0], col.dev.fin[0], (size_t)a.pw * a.ph * 2, hipMemcpyDeviceToDevice, s));
    }
  }
  // ---- frame descriptors + tile jobs -> the stage chain (K1 .. K4) -> tile lengths and the levels the device picked (read in mi_batch_wait)
  if (int st = b->fs.stage(s)) return st;
  if (int st = b->fs.enqueue_chain(s, b->ev)) return st;
  HIP_OK(hipEventRecord(b->ev[5], s));
  if (int st = b->fs.enqueue_readback(s)) return st;
  b->in_flight = true;
  return MI_OK;
}

// Waits for the enqueued work, compacts + downloads the tile payloads (one D2H) and assembles OBUs and containers.
int mi_batch_wait(mi_batch *b) {
  if (!b || !b->in_flight) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  hipStream_t s = b->stream;
  b->in_flight = false;
  const int njobs = (int)b->fs.jobs.size();
  std::vector<uint32_t> offsets(njobs);
  HIP_OK(hipStreamSynchronize(s));
  b->jpeg_used = 0; b->png_used = 0; b->rs_used = 0;          // every JPEG / PNG upload and every resize table of the run has left the pinned staging (the last call's
                                                              // tables stay on the device until the next ones are written: rs_key)
  if (b->channels == 4) for (int i = 0; i < b->n; i++) b->alpha_flags[i] = b->h_alpha.get()[i];
  auto idle = [&](const FramePlan &p) { return p.is_alpha && !b->alpha_flags[p.image]; };
  if (int st = b->fs.check_lengths()) return st;
  size_t total = 0;
  for (int j = 0; j < njobs; j++) { offsets[j] = (uint32_t)total; total += b->fs.h_lens.get()[j]; }
  if (total > b->packed_max) return MI_ENCODING_ERROR;
  if (total > b->packed_cap) {                                 // rare (near-lossless settings): grow the packed pair, keep it
    b->d_packed.reset(); b->h_packed.reset();
    b->packed_cap = std::min(b->packed_max, align_up(total + total / 2, 4096));
    HIP_OK(b->d_packed.alloc(b->packed_cap));
    HIP_OK(b->h_packed.alloc(b->packed_cap));
  }
  HIP_OK(hipMemcpyAsync(b->d_offsets.get(), offsets.data(), (size_t)njobs * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(pack_tiles_kernel, dim3(njobs), dim3(256), 0, s, b->fs.d_frames.get(), b->fs.d_jobs.get(), njobs, b->d_offsets.get(), b->d_packed.get());
  HIP_OK(hipMemcpyAsync(b->h_packed.get(), b->d_packed.get(), total, hipMemcpyDeviceToHost, s));
  HIP_OK(hipEventRecord(b->ev[6], s));
  HIP_OK(hipStreamSynchronize(s));
  // ---- host assembly
  for (size_t k = 0; k < b->fs.frames.size(); k++) {
    FramePlan &p = b->fs.frames[k];
    if (idle(p)) { p.obu.clear(); continue; }
    std::vector<const uint8_t *> tiles;
    for (int t = 0; t < p.ntiles; t++) tiles.push_back(b->h_packed.get() + offsets[p.dev.tile_base + t]);
    b->fs.assemble(k, tiles);
  }
  for (int i = 0; i < b->n; i++) {
    const FramePlan *alpha = nullptr;
    if (b->channels == 4 && b->alpha_flags[i]) alpha = &b->fs.frames[b->n + i];
    const FramePlan &col = b->fs.frames[i];
    b->files[i] = avif_container(col.obu.data(), col.obu.size(), alpha ? alpha->obu.data() : nullptr, alpha ? alpha->obu.size() : 0,
                                 b->w, b->h, b->depth, col.cfg.matrix, b->enc.alpha_mode == 2, b->enc.exif, b->enc.exif_len);
    b->color_sz[i] = col.obu.size(); b->alpha_sz[i] = alpha ? alpha->obu.size() : 0;
  }
  HIP_OK(hipEventRecord(b->ev[7], s));
  HIP_OK(hipEventSynchronize(b->ev[7]));
  for (int i = 0; i < 7; i++) { float ms = 0; (void)hipEventElapsedTime(&ms, b->ev[i], b->ev[i + 1]); b->stage_ms[i] = ms; }
  b->encoded = true;
  return MI_OK;
}

int mi_batch_encode(mi_batch *b) {
  const int st = mi_batch_encode_async(b);
  return st ? st : mi_batch_wait(b);
}

int mi_batch_get(mi_batch *b, int index, mi_encoded_image *out) {
  if (!b || !out || index < 0 || index >= b->n || b->files[index].empty()) return MI_INVALID_ARGUMENT;
  const std::vector<uint8_t> &f = b->files[index];
  out->avif_file = (uint8_t *)malloc(f.size()); memcpy(out->avif_file, f.data(), f.size());
  out->avif_len = f.size(); out->color_byte_size = b->color_sz[index]; out->alpha_byte_size = b->alpha_sz[index];
  return MI_OK;
}

int mi_batch_get_recon(mi_batch *b, int index, int alpha, uint16_t *planes[3]) {
  if (!b || index < 0 || index >= b->n) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  const FramePlan *p = nullptr;
  if (!alpha) p = &b->fs.frames[index]; else if (b->channels == 4 && b->alpha_flags[index]) p = &b->fs.frames[b->n + index];
  if (!p) return MI_INVALID_ARGUMENT;
  for (int i = 0; i < 3; i++) planes[i] = nullptr;
  for (int i = 0; i < p->np; i++) {
    planes[i] = (uint16_t *)malloc((size_t)b->w * b->h * 2);
    HIP_OK(hipMemcpy2D(planes[i], (size_t)b->w * 2, p->cfg.lrf ? p->dev.lrp[i] : p->dev.fin[i], (size_t)p->pw * 2, (size_t)b->w * 2, b->h, hipMemcpyDeviceToHost));
  }
  return MI_OK;
}

int mi_batch_get_source(mi_batch *b, int index, int alpha, uint16_t *planes[3]) {
  if (!b || !planes || index < 0 || index >= b->n || !b->encoded) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  const FramePlan *p = nullptr;
  if (!alpha) p = &b->fs.frames[index]; else if (b->channels == 4 && b->alpha_flags[index]) p = &b->fs.frames[b->n + index];
  if (!p) return MI_INVALID_ARGUMENT;
  for (int i = 0; i < 3; i++) planes[i] = nullptr;
  for (int i = 0; i < p->np; i++) {
    planes[i] = (uint16_t *)malloc((size_t)b->w * b->h * 2);
    HIP_OK(hipMemcpy2D(planes[i], (size_t)b->w * 2, p->dev.src[i], (size_t)p->pw * 2, (size_t)b->w * 2, b->h, hipMemcpyDeviceToHost));
  }
  return MI_OK;
}

// ---- quality metrics of the last completed encode (dev_quality.h) ----
// One launch over the frame descriptors the encode staged (still on the device: nothing after mi_batch_wait writes them or the planes until the next encode),
// the records zeroed in front of it and copied to the pinned mirror behind it, one sync.
int mi_batch_measure(mi_batch *b) {
  if (!b || b->in_flight || !b->encoded) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  hipStream_t s = b->stream;
  const size_t nrec = b->fs.frames.size() * 3;
  if (nrec == 0 || nrec > b->fs.records_cap) return MI_INVALID_ARGUMENT;
  if (!b->h_quality.get()) { HIP_OK(b->h_quality.alloc(b->fs.records_cap)); b->h_quality_bytes = b->fs.records_cap * sizeof(QualityRec); }
  b->measured = false;
  QualityRec *const d_rec = (QualityRec *)b->fs.d_records;
  unsigned tiles = 0;
  for (const FramePlan &p : b->fs.frames) tiles = std::max(tiles, (unsigned)((p.pw / MI_Q_TILE) * (p.ph / MI_Q_TILE)));
  HIP_OK(hipMemsetAsync(d_rec, 0, nrec * sizeof(QualityRec), s));
  hipLaunchKernelGGL(quality_kernel, dim3(tiles, 3, (unsigned)b->fs.frames.size()), dim3(256), 0, s, (const FrameDev *)b->fs.d_frames.get(), d_rec);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(b->h_quality.get(), d_rec, nrec * sizeof(QualityRec), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  b->measured = true;
  return MI_OK;
}
int mi_batch_get_quality(mi_batch *b, int index, mi_image_quality *out) {
  if (!b || !out || index < 0 || index >= b->n || !b->encoded || !b->measured) return MI_INVALID_ARGUMENT;
  memset(out, 0, sizeof(*out));
  out->width = b->w; out->height = b->h; out->depth = (uint8_t)b->depth; out->color_planes = (uint8_t)b->fs.frames[index].np;
  out->has_alpha = (b->channels == 4 && b->alpha_flags[index]) ? 1 : 0;
  auto put = [&](mi_plane_quality &q, size_t frame, int plane) {
    const QualityRec &r = b->h_quality.get()[3 * frame + plane];
    q.sse = r.sse; q.ssim_sum = (int64_t)r.ssim_sum; q.ssim_windows = r.ssim_windows;
  };
  for (int p = 0; p < out->color_planes; p++) put(out->color[p], (size_t)index, p);
  if (out->has_alpha) put(out->alpha, (size_t)b->n + index, 0);
  return MI_OK;
}
double mi_quality_psnr_db(const mi_image_quality *q) {
  if (!q) return NAN;
  double sse = 0; for (int p = 0; p < q->color_planes && p < 3; p++) sse += (double)q->color[p].sse;
  if (sse == 0) return INFINITY;
  const double peak = (double)((1 << q->depth) - 1), n = (double)q->color_planes * q->width * q->height;
  return 10.0 * log10(peak * peak * n / sse);
}
double mi_quality_ssim_db(const mi_image_quality *q) {
  if (!q || q->color[0].ssim_windows == 0) return NAN;
  const double mean = (double)q->color[0].ssim_sum / MI_Q_ONE / (double)q->color[0].ssim_windows;
  return mean >= 1.0 ? INFINITY : -10.0 * log10(1.0 - mean);
}

void mi_batch_destroy(mi_batch *b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  const hipStream_t stream = b->stream;
  hipEvent_t ev[8]; memcpy(ev, b->ev, sizeof(ev));
  const hipEvent_t ev_src = b->ev_src;
  delete b;                                                        // the buffers first: hipFree waits for the device, so an abandoned run has let go of the events and the stream
  for (int i = 0; i < 8; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
  if (ev_src) (void)hipEventDestroy(ev_src);
  if (stream) (void)hipStreamDestroy(stream);
}

// ---- batch objects behind the one-call entry points are pooled ----
// Creating a batch (hipMalloc of the arena, pinned staging: ~0.2 s for 32 x 1080p) and destroying it cost more than encoding a
// small image, and a caller of ravif::Encoder::encode_rgba calls it in a loop with the same settings.  mi_ravif_encode_rgba/_rgb,
// _batch and _stream therefore take their batch objects from a process-wide pool keyed by (device, capacity, shape, settings) and
// hand them back afterwards; mi_release_cached() (or process exit) frees them.  Explicit mi_batch_create objects are not pooled.
struct PoolKey {
  int device, cap, channels; uint32_t w, h; float quality, alpha_quality; uint8_t speed, color_model, depth, alpha_mode; int32_t threads, tiles_override, rdo_passes;
  bool operator==(const PoolKey &o) const {
    return device == o.device && cap == o.cap && channels == o.channels && w == o.w && h == o.h && quality == o.quality && alpha_quality == o.alpha_quality &&
           speed == o.speed && color_model == o.color_model && depth == o.depth && alpha_mode == o.alpha_mode && threads == o.threads && tiles_override == o.tiles_override && rdo_passes == o.rdo_passes;
  }
};
static PoolKey pool_key(const mi_ravif_encoder *e, int cap, uint32_t w, uint32_t h, int channels) {
  return PoolKey{ e->device, cap, channels, w, h, e->quality, e->alpha_quality, e->speed, e->color_model, e->depth, e->alpha_mode, e->threads, e->tiles_override, e->rdo_passes == 2 ? 2 : 1 };
}
static std::mutex g_pool_mu;
static std::vector<std::pair<PoolKey, mi_batch *>> g_pool;          // oldest first; never destroyed at process exit (the runtime may be gone by then)
static size_t batch_footprint(const mi_batch *b) { return b->fs.arena_bytes + b->fs.aux_bytes + 3 * b->pixel_bytes + b->packed_cap + b->h_jpeg_cap + b->d_jpeg_cap + b->d_jpeg_planes_cap + b->h_png_cap + b->d_png_cap + b->h_rs_cap + b->d_rs_cap + b->d_rs_scratch_cap + b->h_quality_bytes + b->d_decoded_cap + b->deep_bytes; }     // (the quality records themselves are part of the arena)
static constexpr size_t MI_POOL_MAX_ITEMS = 8, MI_POOL_MAX_BYTES = (size_t)32 << 30;     // what the one-call entry points may keep between calls (mi_release_cached() frees it)

static mi_batch *pool_acquire(const mi_ravif_encoder *e, int cap, uint32_t w, uint32_t h, int channels) {
  const PoolKey key = pool_key(e, cap, w, h, channels);
  mi_batch *b = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); i++) if (g_pool[i].first == key) { b = g_pool[i].second; g_pool.erase(g_pool.begin() + i); break; }
  }
  if (!b) return mi_batch_create(e, cap, w, h, channels);
  b->exif.clear();
  if (e->exif && e->exif_len) b->exif.assign(e->exif, e->exif + e->exif_len);
  b->enc.exif = b->exif.empty() ? nullptr : b->exif.data(); b->enc.exif_len = b->exif.size();
  b->n = b->cap; b->alpha_flags.assign(b->cap, 0);
  b->encoded = b->measured = false;
  return b;
}
static void pool_release(mi_batch *b) {
  if (!b) return;
  if (b->in_flight) { mi_batch_destroy(b); return; }
  const PoolKey key = pool_key(&b->enc, b->cap, b->w, b->h, b->channels);
  std::vector<mi_batch *> evict;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool.push_back({ key, b });
    size_t bytes = 0; for (auto &x : g_pool) bytes += batch_footprint(x.second);
    while (g_pool.size() > MI_POOL_MAX_ITEMS || (bytes > MI_POOL_MAX_BYTES && g_pool.size() > 1)) { bytes -= batch_footprint(g_pool.front().second); evict.push_back(g_pool.front().second); g_pool.erase(g_pool.begin()); }
  }
  for (mi_batch *x : evict) mi_batch_destroy(x);
}

// ---- JPEG input: decode contexts ----
// mi_jpeg_decode_rgba is called from many loader threads at once (the command line runs a few dozen).  Each call borrows a context -- its own stream, pinned
// staging and device buffers, all grown on demand and never shrunk -- from a per-device free list and hands it back: no hipMalloc per call in the steady
// state.  At most MI_JPEG_CTX_MAX contexts exist per device: a caller that finds them all busy waits for one (the device part of a decode is a fraction of
// the call, the Huffman decoding before it needs no context), because allocating and freeing pinned and device memory per call stalls every other stream of
// the process (measured: profiles/jpeg_input.md).  mi_release_cached() frees the idle ones.
struct JpegCtx {
  int device = 0; hipStream_t stream = nullptr;
  PinBuf<uint8_t> h_in, h_rgba; DevBuf<uint8_t> d_in, d_planes, d_rgba;
  size_t h_in_cap = 0, d_in_cap = 0, d_planes_cap = 0, d_rgba_cap = 0, h_rgba_cap = 0;
};
static constexpr int MI_JPEG_CTX_MAX = 8;
static std::mutex g_jpeg_mu;
static std::condition_variable g_jpeg_cv;
static std::vector<JpegCtx *> g_jpeg_free;                    // never destroyed at process exit (the runtime may be gone by then)
static std::vector<int> g_jpeg_live;                          // contexts in existence per device, idle or borrowed
static void jpeg_ctx_destroy(JpegCtx *c) {
  (void)hipSetDevice(c->device);
  const hipStream_t stream = c->stream;
  delete c;                                                   // the buffers first, then the stream
  if (stream) (void)hipStreamDestroy(stream);
}
static JpegCtx *jpeg_ctx_acquire(int device) {
  {
    std::unique_lock<std::mutex> lk(g_jpeg_mu);
    if ((size_t)device >= g_jpeg_live.size()) g_jpeg_live.resize((size_t)device + 1, 0);
    for (;;) {
      for (size_t i = g_jpeg_free.size(); i-- > 0;) if (g_jpeg_free[i]->device == device) { JpegCtx *c = g_jpeg_free[i]; g_jpeg_free.erase(g_jpeg_free.begin() + i); return c; }
      if (g_jpeg_live[device] < MI_JPEG_CTX_MAX) { g_jpeg_live[device]++; break; }
      g_jpeg_cv.wait(lk);
    }
  }
  JpegCtx *c = new JpegCtx; c->device = device;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    { std::lock_guard<std::mutex> lk(g_jpeg_mu); g_jpeg_live[device]--; }
    g_jpeg_cv.notify_one();
    return nullptr;
  }
  return c;
}
static void jpeg_ctx_release(JpegCtx *c) {
  { std::lock_guard<std::mutex> lk(g_jpeg_mu); g_jpeg_free.push_back(c); }
  g_jpeg_cv.notify_one();
}
// the buffer holds at least `need` bytes afterwards (the context is idle whenever this runs: every public call ends with a stream sync)
static const auto staging_grow = [](auto &buf /* DevBuf or PinBuf */, size_t &cap, size_t need) {
  if (need <= cap) return true;
  need = (need + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
  cap = 0;
  if (buf.alloc(need) != hipSuccess) return false;
  cap = need; return true;
};

void mi_release_cached(void) {
  std::vector<std::pair<PoolKey, mi_batch *>> all;
  { std::lock_guard<std::mutex> lk(g_pool_mu); all.swap(g_pool); }
  for (auto &x : all) mi_batch_destroy(x.second);
  std::vector<JpegCtx *> ctxs;
  { std::lock_guard<std::mutex> lk(g_jpeg_mu); ctxs.swap(g_jpeg_free); for (JpegCtx *c : ctxs) g_jpeg_live[c->device]--; }
  g_jpeg_cv.notify_all();
  for (JpegCtx *c : ctxs) jpeg_ctx_destroy(c);
}

static int encode_one(const mi_ravif_encoder *e, const uint8_t *px, int channels, uint32_t w, uint32_t h, size_t stride_px, mi_encoded_image *out) {
  if (!e || !px || !out || w < 1 || h < 1) return MI_INVALID_ARGUMENT;
  mi_batch *b = pool_acquire(e, 1, w, h, channels);
  if (!b) return mi_device_count() > e->device ? MI_INVALID_ARGUMENT : MI_NO_DEVICE;
  int st = mi_batch_upload(b, 0, px, stride_px);
  if (st == MI_OK) st = mi_batch_encode(b);
  if (st == MI_OK) st = mi_batch_get(b, 0, out);
  pool_release(b);
  return st;
}
int mi_ravif_encode_rgba(const mi_ravif_encoder *e, const uint8_t *rgba, uint32_t w, uint32_t h, size_t stride_px, mi_encoded_image *out) { return encode_one(e, rgba, 4, w, h, stride_px, out); }

// PNG -> RGBA8 (cavif's load_rgba, src/main.rs:265-283); host code, no GPU involved
int mi_png_decode_rgba(const uint8_t *data, size_t len, uint8_t **rgba, uint32_t *w, uint32_t *h) {
  if (!data || !rgba || !w || !h) return MI_INVALID_ARGUMENT;
  try {                                                       // nothing may unwind through the C ABI
    std::vector<uint8_t> px;
    const int st = png_decode_rgba(data, len, px, *w, *h);
    if (st) return st;
    *rgba = (uint8_t *)malloc(px.size());
    if (!*rgba) return MI_ENCODING_ERROR;
    memcpy(*rgba, px.data(), px.size());
    return MI_OK;
  } catch (const std::exception &) { return MI_ENCODING_ERROR; }
}

// The seam of the JPEG path: coefficients of one parsed file -> RGBA8 (channels 4) or RGB8 (channels 3) rows of stride_px pixels at a DEVICE pointer, on
// `stream`.  h_in (pinned) and d_in hold jpeg_in_bytes(jc), d_planes jpeg_plane_bytes(jc): quantisation tables + coefficients are copied to h_in, then one
// H2D and the two kernels of dev_jpeg.h, no sync (probe builds with MI_AVIF_TIMING sync between the steps to time them).  Its own function so that d_out
// can be memory that is consumed on the device (a batch's HBM input slot: mi_batch_upload_jpeg) or a buffer that goes back to the host
// (mi_jpeg_decode_rgba).  The caller has made the device current and keeps h_in untouched until the stream has passed the copy.
static size_t jpeg_in_bytes(const JpegCoeffs &jc) { return 3 * 64 * sizeof(uint16_t) + jc.nblocks * 64 * sizeof(int16_t); }
static size_t jpeg_plane_bytes(const JpegCoeffs &jc) { return jc.nblocks * 64; }
static int jpeg_decode_to_device(const JpegCoeffs &jc, uint8_t *h_in, uint8_t *d_in, uint8_t *d_planes, uint8_t *d_out, int channels, size_t stride_px, hipStream_t stream, double *step_ms, bool ycc = false) {
  JpegDevGeom g; memset(&g, 0, sizeof(g));
  g.w = jc.w; g.h = jc.h; g.ncomp = (uint32_t)jc.ncomp; g.color = (uint32_t)jc.color; g.nblocks = (uint32_t)jc.nblocks;
  for (int c = 0; c < 3; c++) {
    g.first_block[c] = g.nblocks;
    if (c >= jc.ncomp) continue;
    const JpegComp &k = jc.comp[c];
    g.first_block[c] = (uint32_t)k.first_block; g.plane_off[c] = (unsigned long long)k.first_block * 64;
    g.bw[c] = k.bw; g.bh[c] = k.bh; g.cw[c] = k.cw; g.ch[c] = k.ch;
  }
  g.hr = jc.ncomp == 3 ? (uint32_t)(jc.comp[0].h / jc.comp[1].h) : 1; g.vr = jc.ncomp == 3 ? (uint32_t)(jc.comp[0].v / jc.comp[1].v) : 1;
  const size_t quant_bytes = 3 * 64 * sizeof(uint16_t), in_bytes = jpeg_in_bytes(jc);
  const auto t0 = std::chrono::steady_clock::now();
  memset(h_in, 0, quant_bytes);
  for (int c = 0; c < jc.ncomp; c++) memcpy(h_in + c * 64 * sizeof(uint16_t), jc.comp[c].quant, 64 * sizeof(uint16_t));
  memcpy(h_in + quant_bytes, jc.coef.data(), jc.nblocks * 64 * sizeof(int16_t));
  auto lap = [&](int i) { if (step_ms) { (void)hipStreamSynchronize(stream); step_ms[i] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); } };
  HIP_OK(hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, stream));
  lap(0);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((jc.nblocks + MI_JPEG_IDCT_BLOCKS - 1) / MI_JPEG_IDCT_BLOCKS)), dim3(256), 0, stream,
                     (const int16_t *)(d_in + quant_bytes), (const uint16_t *)d_in, g, d_planes);
  const dim3 grid(((jc.w + 3) / 4 + 63) / 64, jc.h);
  if (channels == 4) {
    const int vec16 = (stride_px % 4 == 0 && ((uintptr_t)d_out & 15) == 0) ? 1 : 0;
    if (ycc) hipLaunchKernelGGL((jpeg_ycc_kernel<4>), grid, dim3(64), 0, stream, (const uint8_t *)d_planes, g, d_out, stride_px, vec16);
    else hipLaunchKernelGGL(jpeg_rgba_kernel, grid, dim3(64), 0, stream, (const uint8_t *)d_planes, g, d_out, stride_px, vec16);
  } else {
    const int vec4 = (stride_px % 4 == 0 && ((uintptr_t)d_out & 3) == 0) ? 1 : 0;        // a row is 3 * stride_px bytes
    if (ycc) hipLaunchKernelGGL((jpeg_ycc_kernel<3>), grid, dim3(64), 0, stream, (const uint8_t *)d_planes, g, d_out, stride_px, vec4);
    else hipLaunchKernelGGL(jpeg_rgb_kernel, grid, dim3(64), 0, stream, (const uint8_t *)d_planes, g, d_out, stride_px, vec4);
  }
  HIP_OK(hipGetLastError());
  lap(1);
  return MI_OK;
}

static int jpeg_decode_with(JpegCtx &ctx, const JpegCoeffs &jc, uint8_t *dst, double *step_ms) {
  const size_t out_bytes = (size_t)jc.w * jc.h * 4;
  if (!staging_grow(ctx.d_rgba, ctx.d_rgba_cap, out_bytes) || !staging_grow(ctx.h_rgba, ctx.h_rgba_cap, out_bytes)) return MI_ENCODING_ERROR;
  if (!staging_grow(ctx.h_in, ctx.h_in_cap, jpeg_in_bytes(jc)) || !staging_grow(ctx.d_in, ctx.d_in_cap, jpeg_in_bytes(jc)) || !staging_grow(ctx.d_planes, ctx.d_planes_cap, jpeg_plane_bytes(jc))) return MI_ENCODING_ERROR;
  const int st = jpeg_decode_to_device(jc, ctx.h_in.get(), ctx.d_in.get(), ctx.d_planes.get(), ctx.d_rgba.get(), 4, jc.w, ctx.stream, step_ms);
  if (st) { (void)hipStreamSynchronize(ctx.stream); return st; }
  const auto t0 = std::chrono::steady_clock::now();
  HIP_OK(hipMemcpyAsync(ctx.h_rgba.get(), ctx.d_rgba.get(), out_bytes, hipMemcpyDeviceToHost, ctx.stream));
  HIP_OK(hipStreamSynchronize(ctx.stream));
  if (step_ms) step_ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  memcpy(dst, ctx.h_rgba.get(), out_bytes);
  if (step_ms) step_ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - step_ms[2];
  return MI_OK;
}

// JPEG -> RGBA8 (load_image::load_data + load_rgba, src/main.rs:255-283, for JPEG bytes): Huffman decoding on the host, everything after it on the device
int mi_jpeg_decode_rgba(const uint8_t *data, size_t len, int device, uint8_t **rgba, uint32_t *w, uint32_t *h) {
  if (!data || !rgba || !w || !h) return MI_INVALID_ARGUMENT;
  try {                                                       // nothing may unwind through the C ABI
    const bool timing = mi_timing_enabled();
    const auto t0 = std::chrono::steady_clock::now();
    JpegCoeffs jc;
    int st = jpeg_read_coeffs(data, len, jc);                 // header and stream errors come first: they need no device
    if (st) return st;
    const double parse_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (device < 0) return MI_INVALID_ARGUMENT;
    if (mi_device_count() <= device) return MI_NO_DEVICE;     // no CPU fallback
    if (hipSetDevice(device) != hipSuccess) return MI_NO_DEVICE;
    uint8_t *px = (uint8_t *)malloc((size_t)jc.w * jc.h * 4);
    if (!px) return MI_ENCODING_ERROR;
    JpegCtx *ctx = jpeg_ctx_acquire(device);
    if (!ctx) { free(px); return MI_ENCODING_ERROR; }
    double step_ms[4] = { 0, 0, 0, 0 };
    st = jpeg_decode_with(*ctx, jc, px, timing ? step_ms : nullptr);
    jpeg_ctx_release(ctx);
    if (st) { free(px); return st; }
    if (timing) fprintf(stderr, "[jpeg] %ux%u %zu bytes: parse+entropy %.3f ms, staging+H2D %.3f ms, kernels %.3f ms, D2H %.3f ms, copy-out %.3f ms\n", jc.w, jc.h, len, parse_ms,
                        step_ms[0], step_ms[1] - step_ms[0], step_ms[2], step_ms[3]);
    *rgba = px; *w = jc.w; *h = jc.h;
    return MI_OK;
  } catch (const std::exception &) { return MI_ENCODING_ERROR; }
}

// load_rgba (src/main.rs:255-283) for the formats this library reads, told apart by their first bytes as load_image does
int mi_image_decode_rgba(const uint8_t *data, size_t len, int device, uint8_t **rgba, uint32_t *w, uint32_t *h) {
  if (!data || !rgba || !w || !h) return MI_INVALID_ARGUMENT;
  static const uint8_t png_sig[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
  if (len >= 8 && !memcmp(data, png_sig, 8)) return mi_png_decode_rgba(data, len, rgba, w, h);
  if (len >= 2 && data[0] == 0xFF && data[1] == 0xD8) return mi_jpeg_decode_rgba(data, len, device, rgba, w, h);
  return MI_UNSUPPORTED;
}

// ---- device-resident input: a picture reaches a batch's HBM input slot without ever being host pixels ----
struct mi_jpeg_coeffs { JpegCoeffs jc; };

// jpeg_read_coeffs behind a handle: host work only, the statuses mi_jpeg_decode_rgba gives for the same bytes
int mi_jpeg_parse(const uint8_t *data, size_t len, mi_jpeg_coeffs **out, uint32_t *w, uint32_t *h) {
  if (!data || !out || !w || !h) return MI_INVALID_ARGUMENT;
  *out = nullptr;
  try {                                                       // nothing may unwind through the C ABI
    std::unique_ptr<mi_jpeg_coeffs> c(new mi_jpeg_coeffs);
    if (const int st = jpeg_read_coeffs(data, len, c->jc)) return st;
    *w = c->jc.w; *h = c->jc.h;
    *out = c.release();
    return MI_OK;
  } catch (const std::exception &) { return MI_ENCODING_ERROR; }
}
void mi_jpeg_coeffs_free(mi_jpeg_coeffs *c) { delete c; }

uint8_t *mi_batch_device_input(mi_batch *b, int index) {
  if (!b || index < 0 || index >= b->cap) return nullptr;
  return b->d_pixels.get() + (size_t)index * b->w * b->h * b->channels;
}
int mi_batch_read_input(mi_batch *b, int index, uint8_t *dst) {
  if (!b || !dst || index < 0 || index >= b->cap) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  HIP_OK(hipStreamSynchronize(b->stream));
  HIP_OK(hipMemcpy(dst, mi_batch_device_input(b, index), (size_t)b->w * b->h * b->channels, hipMemcpyDeviceToHost));
  return MI_OK;
}

// images [first, first + count) from pictures in the memory of the batch's device: one ingest_kernel launch on the batch's stream, after whatever
// src->after_stream holds at this moment.  Strides of 0 mean packed; a row must not be shorter than its packed pixels (torch views -- crops, permuted
// tensors, padded rows -- all satisfy that).
int mi_batch_upload_device(mi_batch *b, int first, int count, const mi_device_pixels *src) {
  if (!b || !src || !src->dev || b->in_flight || first < 0 || count < 1 || first > b->cap - count) return MI_INVALID_ARGUMENT;
  if ((src->layout != 0 && src->layout != 1) || (src->channels != 3 && src->channels != 4) || src->channels > b->channels) return MI_INVALID_ARGUMENT;   // alpha is never dropped
  IngestSrc s;
  s.base = (const uint8_t *)src->dev; s.w = b->w; s.h = b->h; s.layout = src->layout; s.channels = src->channels;
  const size_t packed_row = (size_t)b->w * (s.layout == 0 ? s.channels : 1);
  s.row_stride = src->row_stride ? src->row_stride : packed_row;
  s.inner_stride = src->pixel_or_plane_stride ? src->pixel_or_plane_stride : s.layout == 0 ? (size_t)s.channels : s.row_stride * b->h;
  s.image_stride = src->image_stride ? src->image_stride : s.layout == 0 ? s.row_stride * b->h : s.inner_stride * s.channels;
  if (s.row_stride < packed_row || s.inner_stride < (s.layout == 0 ? (size_t)s.channels : (size_t)b->w)) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  if (src->after_stream) {
    if (!b->ev_src) HIP_OK(hipEventCreateWithFlags(&b->ev_src, hipEventDisableTiming));
    HIP_OK(hipEventRecord(b->ev_src, (hipStream_t)src->after_stream));
    HIP_OK(hipStreamWaitEvent(b->stream, b->ev_src, 0));
  }
  const dim3 grid(((b->w + 3) / 4 + 63) / 64, b->h, (unsigned)count);
  uint8_t *const slots = mi_batch_device_input(b, first);
  if (b->channels == 4) hipLaunchKernelGGL((ingest_kernel<4>), grid, dim3(64), 0, b->stream, s, slots);
  else hipLaunchKernelGGL((ingest_kernel<3>), grid, dim3(64), 0, b->stream, s, slots);
  HIP_OK(hipGetLastError());
  batch_tag(b, first, count, MI_INPUT_RGB);
  return MI_OK;
}
// images [first, first + count) from 8-bit YCbCr planes in the memory of the batch's device: one planes_ingest_kernel launch on the batch's stream, after
// whatever src->after_stream holds at this moment; the slots are tagged MI_INPUT_YCBCR.  Strides of 0 mean packed.
int mi_batch_upload_device_ycbcr(mi_batch *b, int first, int count, const mi_device_planes *src) {
  if (!b || !src || !src->y || !src->cb || b->in_flight || first < 0 || count < 1 || first > b->cap - count || !batch_takes_ycbcr(b)) return MI_INVALID_ARGUMENT;
  if (!((src->hsub == 1 && src->vsub == 1) || (src->hsub == 2 && (src->vsub == 1 || src->vsub == 2)))) return MI_INVALID_ARGUMENT;
  PlanesSrc s;
  s.w = b->w; s.h = b->h; s.hsub = (uint32_t)src->hsub; s.vsub = (uint32_t)src->vsub;
  s.cw = (b->w + s.hsub - 1) / s.hsub; s.ch = (b->h + s.vsub - 1) / s.vsub;
  s.cpitch = src->cr ? 1 : 2;
  s.y = (const uint8_t *)src->y; s.cb = (const uint8_t *)src->cb; s.cr = src->cr ? (const uint8_t *)src->cr : s.cb + 1;
  const size_t packed_c = (size_t)s.cw * s.cpitch;
  s.y_row = src->y_row_stride ? src->y_row_stride : b->w; s.c_row = src->c_row_stride ? src->c_row_stride : packed_c;
  s.y_image = src->y_image_stride ? src->y_image_stride : s.y_row * b->h; s.c_image = src->c_image_stride ? src->c_image_stride : s.c_row * s.ch;
  if (s.y_row < b->w || s.c_row < packed_c) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  if (src->after_stream) {
    if (!b->ev_src) HIP_OK(hipEventCreateWithFlags(&b->ev_src, hipEventDisableTiming));
    HIP_OK(hipEventRecord(b->ev_src, (hipStream_t)src->after_stream));
    HIP_OK(hipStreamWaitEvent(b->stream, b->ev_src, 0));
  }
  const dim3 grid(((b->w + 3) / 4 + 63) / 64, b->h, (unsigned)count);
  uint8_t *const slots = mi_batch_device_input(b, first);
  if (b->channels == 4) hipLaunchKernelGGL((planes_ingest_kernel<4>), grid, dim3(64), 0, b->stream, s, slots);
  else hipLaunchKernelGGL((planes_ingest_kernel<3>), grid, dim3(64), 0, b->stream, s, slots);
  HIP_OK(hipGetLastError());
  batch_tag(b, first, count, MI_INPUT_YCBCR);
  return MI_OK;
}

// ---- deep input: 16-bit sources into the deep slots (dev_deep.h) ----
uint16_t *mi_batch_device_input16(mi_batch *b, int index) {
  if (!b || index < 0 || index >= b->cap) return nullptr;
  uint16_t *const deep = batch_deep(b);
  return deep ? deep + (size_t)index * b->w * b->h * b->channels : nullptr;
}
int mi_batch_read_input16(mi_batch *b, int index, uint16_t *dst) {
  if (!b || !dst || index < 0 || index >= b->cap) return MI_INVALID_ARGUMENT;
  const uint16_t *const src = mi_batch_device_input16(b, index);
  if (!src) return MI_ENCODING_ERROR;
  (void)hipSetDevice(b->device);
  HIP_OK(hipStreamSynchronize(b->stream));
  HIP_OK(hipMemcpy(dst, src, (size_t)b->w * b->h * b->channels * sizeof(uint16_t), hipMemcpyDeviceToHost));
  return MI_OK;
}
size_t mi_batch_footprint(const mi_batch *b) { return b ? batch_footprint(b) : 0; }

// images [first, first + count) from uint16 pictures in the memory of the batch's device: one ingest16_kernel launch on the batch's stream, after whatever
// src->after_stream holds at this moment; the slots are tagged MI_INPUT_RGB16.  Every check comes before the deep slots are made: a refused call allocates nothing.
int mi_batch_upload_device16(mi_batch *b, int first, int count, const mi_device_pixels16 *src) {
  if (!b || !src || !src->dev || b->in_flight || first < 0 || count < 1 || first > b->cap - count) return MI_INVALID_ARGUMENT;
  if ((src->layout != 0 && src->layout != 1) || !batch_takes_deep(b, src->channels)) return MI_INVALID_ARGUMENT;   // alpha is never dropped; the alpha rules of the kind
  if (src->bits < 8 || src->bits > 16 || (src->msb_aligned != 0 && src->msb_aligned != 1)) return MI_INVALID_ARGUMENT;
  if (((uintptr_t)src->dev | src->row_stride | src->pixel_or_plane_stride | src->image_stride) & 1) return MI_INVALID_ARGUMENT;   // uint16 samples
  Ingest16Src s;
  s.base = (const uint8_t *)src->dev; s.w = b->w; s.h = b->h; s.layout = src->layout; s.channels = src->channels; s.bits = src->bits; s.msb_aligned = src->msb_aligned;
  const size_t packed_row = (size_t)b->w * (s.layout == 0 ? s.channels : 1) * 2;
  s.row_stride = src->row_stride ? src->row_stride : packed_row;
  s.inner_stride = src->pixel_or_plane_stride ? src->pixel_or_plane_stride : s.layout == 0 ? (size_t)s.channels * 2 : s.row_stride * b->h;
  s.image_stride = src->image_stride ? src->image_stride : s.layout == 0 ? s.row_stride * b->h : s.inner_stride * s.channels;
  if (s.row_stride < packed_row || s.inner_stride < (s.layout == 0 ? (size_t)s.channels * 2 : (size_t)b->w * 2)) return MI_INVALID_ARGUMENT;
  uint16_t *const slots = mi_batch_device_input16(b, first);
  if (!slots) return MI_ENCODING_ERROR;
  (void)hipSetDevice(b->device);
  if (src->after_stream) {
    if (!b->ev_src) HIP_OK(hipEventCreateWithFlags(&b->ev_src, hipEventDisableTiming));
    HIP_OK(hipEventRecord(b->ev_src, (hipStream_t)src->after_stream));
    HIP_OK(hipStreamWaitEvent(b->stream, b->ev_src, 0));
  }
  const dim3 grid(((b->w + 3) / 4 + 63) / 64, b->h, (unsigned)count);
  if (b->channels == 4) hipLaunchKernelGGL((ingest16_kernel<4>), grid, dim3(64), 0, b->stream, s, slots);
  else hipLaunchKernelGGL((ingest16_kernel<3>), grid, dim3(64), 0, b->stream, s, slots);
  HIP_OK(hipGetLastError());
  batch_tag(b, first, count, MI_INPUT_RGB16);
  return MI_OK;
}
// one image of full-scale uint16 host pixels into the deep slot of `index`: a 2-D copy on the batch's stream (3 channels into a 4-channel batch: through a host
// copy that carries A = 65535), then the stream is waited for.  No pinned staging of its own.
int mi_batch_upload16(mi_batch *b, int index, const uint16_t *pixels, size_t stride_px, int channels) {
  if (!b || !pixels || b->in_flight || index < 0 || index >= b->cap || !batch_takes_deep(b, channels)) return MI_INVALID_ARGUMENT;
  if (stride_px == 0) stride_px = b->w;
  if (stride_px < b->w) return MI_INVALID_ARGUMENT;
  uint16_t *const slot = mi_batch_device_input16(b, index);
  if (!slot) return MI_ENCODING_ERROR;
  (void)hipSetDevice(b->device);
  const size_t row = (size_t)b->w * b->channels * sizeof(uint16_t);
  try {                                                       // nothing may unwind through the C ABI
    std::vector<uint16_t> wide;
    if (channels != b->channels) {
      wide.resize((size_t)b->w * b->h * 4);
      for (uint32_t y = 0; y < b->h; y++) for (uint32_t x = 0; x < b->w; x++) {
        const uint16_t *q = pixels + ((size_t)y * stride_px + x) * 3; uint16_t *o = wide.data() + ((size_t)y * b->w + x) * 4;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = 65535;
      }
      HIP_OK(hipMemcpyAsync(slot, wide.data(), row * b->h, hipMemcpyHostToDevice, b->stream));
    } else HIP_OK(hipMemcpy2DAsync(slot, row, pixels, stride_px * channels * sizeof(uint16_t), row, b->h, hipMemcpyHostToDevice, b->stream));
    HIP_OK(hipStreamSynchronize(b->stream));
  } catch (const std::exception &) { return MI_ENCODING_ERROR; }
  batch_tag(b, index, 1, MI_INPUT_RGB16);
  return MI_OK;
}

// ---- decoded pixels of the last completed encode (dev_decoded.h) ----
int mi_batch_uses_alpha(mi_batch *b, int index, int *uses_alpha) {
  if (!b || !uses_alpha || b->in_flight || !b->encoded || index < 0 || index >= b->n) return MI_INVALID_ARGUMENT;
  *uses_alpha = (b->channels == 4 && b->alpha_flags[index]) ? 1 : 0;
  return MI_OK;
}
// One decoded_kernel launch over the frame descriptors the encode staged (still on the device, like the planes: nothing after mi_batch_wait writes them until
// the next encode), after whatever dst->after_stream holds at this moment, then the batch's stream is waited for.  Strides of 0 mean packed.
int mi_batch_decode_device(mi_batch *b, int first, int count, int which, const mi_device_target *dst) {
  if (!b || !dst || !dst->dev || b->in_flight || !b->encoded || first < 0 || count < 1 || first > b->n - count) return MI_INVALID_ARGUMENT;
  if ((which != MI_DECODED_RECON && which != MI_DECODED_SOURCE) || (dst->layout != 0 && dst->layout != 1) || (dst->channels != 3 && dst->channels != 4)) return MI_INVALID_ARGUMENT;
  if ((size_t)b->n * (b->channels == 4 ? 2 : 1) != b->fs.frames.size()) return MI_INVALID_ARGUMENT;
  if (dst->channels == 3 && b->channels == 4)
    for (int i = first; i < first + count; i++) if (b->alpha_flags[i]) return MI_INVALID_ARGUMENT;      // alpha is never dropped
  DecodedDst d;
  d.base = (uint8_t *)dst->dev; d.layout = dst->layout; d.channels = dst->channels; d.first = first; d.n = b->n; d.alpha_frames = b->channels == 4; d.source = which == MI_DECODED_SOURCE;
  const size_t packed_row = (size_t)b->w * (d.layout == 0 ? d.channels : 1);
  d.row_stride = dst->row_stride ? dst->row_stride : packed_row;
  d.inner_stride = dst->pixel_or_plane_stride ? dst->pixel_or_plane_stride : d.layout == 0 ? (size_t)d.channels : d.row_stride * b->h;
  d.image_stride = dst->image_stride ? dst->image_stride : d.layout == 0 ? d.row_stride * b->h : d.inner_stride * d.channels;
  if (d.row_stride < packed_row || d.inner_stride < (d.layout == 0 ? (size_t)d.channels : (size_t)b->w)) return MI_INVALID_ARGUMENT;
  if (d.layout == 0 && d.row_stride < (size_t)(b->w - 1) * d.inner_stride + d.channels) return MI_INVALID_ARGUMENT;     // a written row must end before the next one starts
  (void)hipSetDevice(b->device);
  if (dst->after_stream) {
    if (!b->ev_src) HIP_OK(hipEventCreateWithFlags(&b->ev_src, hipEventDisableTiming));
    HIP_OK(hipEventRecord(b->ev_src, (hipStream_t)dst->after_stream));
    HIP_OK(hipStreamWaitEvent(b->stream, b->ev_src, 0));
  }
  const dim3 grid(((b->w + 3) / 4 + 63) / 64, b->h, (unsigned)count);
  const FrameDev *const frames = b->fs.d_frames.get();
  const bool rgb_model = b->fs.frames[first].cfg.matrix == 0;
  if (b->depth == 8) {
    if (rgb_model) hipLaunchKernelGGL((decoded_kernel<8, 1>), grid, dim3(64), 0, b->stream, frames, d);
    else hipLaunchKernelGGL((decoded_kernel<8, 0>), grid, dim3(64), 0, b->stream, frames, d);
  } else {
    if (rgb_model) hipLaunchKernelGGL((decoded_kernel<10, 1>), grid, dim3(64), 0, b->stream, frames, d);
    else hipLaunchKernelGGL((decoded_kernel<10, 0>), grid, dim3(64), 0, b->stream, frames, d);
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(b->stream));
  return MI_OK;
}
// One image into host memory: the same launch into the batch's own one-image scratch (never the input slot), one D2H.
int mi_batch_decode(mi_batch *b, int index, int which, int channels, uint8_t *dst) {
  if (!b || !dst || b->in_flight || !b->encoded || index < 0 || index >= b->n || (channels != 3 && channels != 4)) return MI_INVALID_ARGUMENT;
  if ((which != MI_DECODED_RECON && which != MI_DECODED_SOURCE) || (channels == 3 && b->channels == 4 && b->alpha_flags[index])) return MI_INVALID_ARGUMENT;   // before the scratch exists: a refused call allocates nothing
  (void)hipSetDevice(b->device);
  if (!staging_grow(b->d_decoded, b->d_decoded_cap, (size_t)b->w * b->h * 4)) return MI_ENCODING_ERROR;
  mi_device_target t;
  memset(&t, 0, sizeof(t));
  t.dev = b->d_decoded.get(); t.layout = 0; t.channels = channels;
  if (const int st = mi_batch_decode_device(b, index, 1, which, &t)) return st;
  HIP_OK(hipMemcpy(dst, b->d_decoded.get(), (size_t)b->w * b->h * channels, hipMemcpyDeviceToHost));
  return MI_OK;
}

// One parsed JPEG into the slot of image `index`: tables + coefficients into the batch's own pinned staging, one H2D and the two kernels of
// jpeg_decode_to_device on the batch's stream, no sync.  The staging keeps the images uploaded since the stream last drained (room for
// MI_BATCH_JPEG_STAGED of the first one's size; when the next one does not fit, the stream -- which carries nothing but such uploads then -- is waited
// for and the staging starts over); the plane buffer is one image's, stream order serialises its users.
static constexpr size_t MI_BATCH_JPEG_STAGED = 4;
// (the staging half, shared with mi_batch_resize_jpeg: rows of stride_px pixels at any device pointer)
static int batch_jpeg_decode(mi_batch *b, const JpegCoeffs &jc, uint8_t *d_out, int channels, size_t stride_px, bool ycc = false) {
  const size_t need = align_up(jpeg_in_bytes(jc), 256);
  if (b->jpeg_used + need > b->h_jpeg_cap) {
    HIP_OK(hipStreamSynchronize(b->stream));
    b->jpeg_used = 0;
    if (!staging_grow(b->h_jpeg, b->h_jpeg_cap, MI_BATCH_JPEG_STAGED * need) || !staging_grow(b->d_jpeg, b->d_jpeg_cap, MI_BATCH_JPEG_STAGED * need)) return MI_ENCODING_ERROR;
  }
  if (jpeg_plane_bytes(jc) > b->d_jpeg_planes_cap) {
    HIP_OK(hipStreamSynchronize(b->stream));                  // an earlier image's kernels may still read the buffer that is replaced
    if (!staging_grow(b->d_jpeg_planes, b->d_jpeg_planes_cap, jpeg_plane_bytes(jc))) return MI_ENCODING_ERROR;
  }
  const size_t at = b->jpeg_used; b->jpeg_used += need;
  return jpeg_decode_to_device(jc, b->h_jpeg.get() + at, b->d_jpeg.get() + at, b->d_jpeg_planes.get(), d_out, channels, stride_px, b->stream, nullptr, ycc);
}
int mi_batch_upload_jpeg(mi_batch *b, int index, const mi_jpeg_coeffs *c) {
  if (!b || !c || b->in_flight || index < 0 || index >= b->cap) return MI_INVALID_ARGUMENT;
  const JpegCoeffs &jc = c->jc;
  if (jc.w != b->w || jc.h != b->h) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  if (int st = batch_jpeg_decode(b, jc, mi_batch_device_input(b, index), b->channels, b->w)) return st;
  batch_tag(b, index, 1, MI_INPUT_RGB);
  return MI_OK;
}
// the same staging, copy and IDCT, then jpeg_ycc_kernel instead of a colour kernel: the slot holds the file's own (Y, Cb, Cr) and is tagged MI_INPUT_YCBCR
int mi_batch_upload_jpeg_ycbcr(mi_batch *b, int index, const mi_jpeg_coeffs *c) {
  if (!b || !c || b->in_flight || index < 0 || index >= b->cap) return MI_INVALID_ARGUMENT;
  const JpegCoeffs &jc = c->jc;
  if (jc.w != b->w || jc.h != b->h || !batch_takes_ycbcr(b)) return MI_INVALID_ARGUMENT;
  if (jc.color == JPEG_RGB) return MI_UNSUPPORTED;
  (void)hipSetDevice(b->device);
  if (int st = batch_jpeg_decode(b, jc, mi_batch_device_input(b, index), b->channels, b->w, true)) return st;
  batch_tag(b, index, 1, MI_INPUT_YCBCR);
  return MI_OK;
}
int mi_jpeg_coeffs_info(const mi_jpeg_coeffs *c, int *color, int *hsub, int *vsub) {
  if (!c) return MI_INVALID_ARGUMENT;
  const JpegCoeffs &jc = c->jc;
  if (color) *color = jc.color == JPEG_GREY ? 0 : jc.color == JPEG_YCBCR ? 1 : 2;
  if (hsub) *hsub = jc.ncomp == 3 ? jc.comp[0].h / jc.comp[1].h : 1;
  if (vsub) *vsub = jc.ncomp == 3 ? jc.comp[0].v / jc.comp[1].v : 1;
  return MI_OK;
}

// ---- PNG input: the host half behind a handle, the device half on the batch's stream ----
struct mi_png_scanlines { PngScanlines sl; };

// png_read_scanlines behind a handle: host work only (chunk walk, inflate, filter-byte and palette-index checks), the statuses of mi_png_decode_rgba
int mi_png_parse(const uint8_t *data, size_t len, mi_png_scanlines **out, uint32_t *w, uint32_t *h, int *has_alpha) {
  if (!data || !out || !w || !h) return MI_INVALID_ARGUMENT;
  *out = nullptr;
  try {                                                       // nothing may unwind through the C ABI
    std::unique_ptr<mi_png_scanlines> p(new mi_png_scanlines);
    if (const int st = png_read_scanlines(data, len, p->sl)) return st;
    *w = p->sl.w; *h = p->sl.h;
    if (has_alpha) *has_alpha = p->sl.has_alpha() ? 1 : 0;
    *out = p.release();
    return MI_OK;
  } catch (const std::exception &) { return MI_ENCODING_ERROR; }
}
void mi_png_scanlines_free(mi_png_scanlines *p) { delete p; }

// what one call stages: pass descriptors of the passes that have a filtered row, one image descriptor per image, then per image its palette (colour type 3)
// and its scanlines, 16-byte aligned; 16 spare bytes at the end
static size_t png_call_bytes(int count, const mi_png_scanlines *const *png) {
  size_t n = align_up((size_t)count * 7 * sizeof(PngPassDev), 16) + align_up((size_t)count * sizeof(PngImageDev), 16);
  for (int i = 0; i < count; i++) n += (png[i]->sl.ctype == 3 ? 1024 : 0) + align_up(png[i]->sl.raw.size(), 16);
  return align_up(n + 16, 256);
}

// room for `bytes` of PNG staging, pinned and on the device, made ahead of the first mi_batch_upload_png (the stream worker does this on the thread that creates the batch
// object, beside the loaders: on the worker's own thread the 35 - 55 ms of a first call's allocation delay the first run); idle batches only, false = could not
static bool batch_reserve_png(mi_batch *b, size_t bytes) {
  if (!b || b->in_flight || b->png_used) return false;
  if (bytes <= b->h_png_cap && bytes <= b->d_png_cap) return true;
  (void)hipSetDevice(b->device);
  if (hipStreamSynchronize(b->stream) != hipSuccess) return false;
  return staging_grow(b->h_png, b->h_png_cap, bytes) && staging_grow(b->d_png, b->d_png_cap, bytes);
}

// images [first, first + count) from parsed PNG files of the batch's size: descriptors, palettes and scanlines into the batch's pinned staging, one H2D, then
// png_unfilter_kernel (one workgroup per pass that has a filtered row, all images in one launch) and png_expand_kernel on the batch's stream, no sync.
// The staging keeps the calls since the stream last drained; when the next one does not fit, the stream is waited for and the staging starts over, grown to the call.
// (the body, shared with mi_batch_resize_png: `count` checked files of w x h into packed pictures of `channels` channels, back to back from `slots` on)
static int batch_png_expand(mi_batch *b, int count, const mi_png_scanlines *const *png, uint32_t w, uint32_t h, int channels, void *slots, bool deep = false) {
  const size_t need = png_call_bytes(count, png);
  if (b->png_used + need > b->h_png_cap || b->png_used + need > b->d_png_cap) {
    HIP_OK(hipStreamSynchronize(b->stream));                  // earlier calls' copies and kernels may still use the buffers that start over or are replaced
    b->png_used = 0;
    if (!staging_grow(b->h_png, b->h_png_cap, need) || !staging_grow(b->d_png, b->d_png_cap, need)) return MI_ENCODING_ERROR;
  }
  const size_t at = b->png_used; b->png_used += need;
  uint8_t *const hb = b->h_png.get() + at;
  PngPassDev *passes = (PngPassDev *)hb;
  const size_t img_at = align_up((size_t)count * 7 * sizeof(PngPassDev), 16);
  PngImageDev *imgs = (PngImageDev *)(hb + img_at);
  size_t pos = img_at + align_up((size_t)count * sizeof(PngImageDev), 16);
  uint32_t npass = 0, max_rows = 0;
  for (int i = 0; i < count; i++) {
    const PngScanlines &sl = png[i]->sl;
    PngImageDev &im = imgs[i]; memset(&im, 0, sizeof(im));
    im.depth = (uint32_t)sl.depth; im.ctype = (uint32_t)sl.ctype; im.interlace = (uint32_t)sl.interlace; im.has_key = sl.has_key ? 1 : 0;
    for (int c = 0; c < 3; c++) im.key[c] = sl.key[c];
    if (sl.ctype == 3) { im.palette_off = at + pos; memcpy(hb + pos, sl.palette, 1024); pos += 1024; }
    memcpy(hb + pos, sl.raw.data(), sl.raw.size());
    for (int p = 0; p < sl.npass; p++) {
      const PngPass &ps = sl.pass[p];
      // the Adam7 pass this is: dx, dy and x0 tell (a non-interlaced file has the one pass 0)
      const int id = !sl.interlace ? 0 : ps.dy == 8 ? (ps.dx == 4 ? 2 : ps.x0 ? 1 : 0) : ps.dy == 4 ? (ps.dx == 4 ? 3 : 4) : ps.dx == 2 ? 5 : 6;
      im.pass_off[id] = at + pos + ps.off; im.pass_rowbytes[id] = ps.rowbytes;
      bool filtered = false;
      for (uint32_t y = 0; y < ps.rows && !filtered; y++) filtered = sl.raw[ps.off + (size_t)y * (ps.rowbytes + 1)] != 0;
      if (!filtered) continue;                                // nothing to undo
      passes[npass++] = PngPassDev{ at + pos + ps.off, ps.rows, ps.rowbytes, (uint32_t)sl.bpp, 0 };
      max_rows = std::max(max_rows, ps.rows);
    }
    pos += align_up(sl.raw.size(), 16);
  }
  uint8_t *const db = b->d_png.get();
  HIP_OK(hipMemcpyAsync(db + at, hb, pos, hipMemcpyHostToDevice, b->stream));
  if (npass) {
    const unsigned waves = std::min<unsigned>(MI_PNG_WAVES, (max_rows + 63) / 64);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(npass), dim3(64 * waves), 0, b->stream, db, (const PngPassDev *)(db + at));
  }
  const dim3 grid(((w + 3) / 4 + 63) / 64, h, (unsigned)count);
  if (deep) {                                                 // files of bit depth 16 into deep slots: both bytes of every sample
    if (channels == 4) hipLaunchKernelGGL((png_expand16_kernel<4>), grid, dim3(64), 0, b->stream, (const uint8_t *)db, (const PngImageDev *)(db + at + img_at), w, h, (uint16_t *)slots);
    else hipLaunchKernelGGL((png_expand16_kernel<3>), grid, dim3(64), 0, b->stream, (const uint8_t *)db, (const PngImageDev *)(db + at + img_at), w, h, (uint16_t *)slots);
  } else if (channels == 4) hipLaunchKernelGGL((png_expand_kernel<4>), grid, dim3(64), 0, b->stream, (const uint8_t *)db, (const PngImageDev *)(db + at + img_at), w, h, (uint8_t *)slots);
  else hipLaunchKernelGGL((png_expand_kernel<3>), grid, dim3(64), 0, b->stream, (const uint8_t *)db, (const PngImageDev *)(db + at + img_at), w, h, (uint8_t *)slots);
  HIP_OK(hipGetLastError());
  return MI_OK;
}
int mi_batch_upload_png(mi_batch *b, int first, int count, const mi_png_scanlines *const *png) {
  if (!b || !png || b->in_flight || first < 0 || count < 1 || first > b->cap - count) return MI_INVALID_ARGUMENT;
  for (int i = 0; i < count; i++) {
    if (!png[i] || png[i]->sl.w != b->w || png[i]->sl.h != b->h) return MI_INVALID_ARGUMENT;
    if (b->channels == 3 && png[i]->sl.has_alpha()) return MI_INVALID_ARGUMENT;      // alpha is never dropped
  }
  (void)hipSetDevice(b->device);
  if (int st = batch_png_expand(b, count, png, b->w, b->h, b->channels, mi_batch_device_input(b, first))) return st;
  batch_tag(b, first, count, MI_INPUT_RGB);
  return MI_OK;
}

// mi_batch_upload_png for 16-bit masters: a handle of bit depth 16 is unfiltered as above and expanded by png_expand16_kernel into its deep slot (kind
// MI_INPUT_RGB16), every other handle goes exactly the way mi_batch_upload_png sends it (kind MI_INPUT_RGB).  Neighbours that go the same way share one call's
// staging, copy and launches.  Every handle is checked before anything is staged or allocated.
static bool png_goes_deep(const mi_png_scanlines *p) { return p->sl.depth == 16 && p->sl.ctype != 3; }
int mi_png_scanlines_info(const mi_png_scanlines *p, int *color_type, int *bit_depth) {
  if (!p) return MI_INVALID_ARGUMENT;
  if (color_type) *color_type = p->sl.ctype;
  if (bit_depth) *bit_depth = p->sl.depth;
  return MI_OK;
}
int mi_batch_upload_png_deep(mi_batch *b, int first, int count, const mi_png_scanlines *const *png) {
  if (!b || !png || b->in_flight || first < 0 || count < 1 || first > b->cap - count) return MI_INVALID_ARGUMENT;
  bool any_deep = false;
  for (int i = 0; i < count; i++) {
    if (!png[i] || png[i]->sl.w != b->w || png[i]->sl.h != b->h) return MI_INVALID_ARGUMENT;
    if (b->channels == 3 && png[i]->sl.has_alpha()) return MI_INVALID_ARGUMENT;      // alpha is never dropped
    if (png_goes_deep(png[i])) { any_deep = true; if (!batch_takes_deep(b, png[i]->sl.has_alpha() ? 4 : 3)) return MI_INVALID_ARGUMENT; }
  }
  if (any_deep && !batch_deep(b)) return MI_ENCODING_ERROR;
  (void)hipSetDevice(b->device);
  for (int i = 0; i < count;) {
    const bool deep = png_goes_deep(png[i]);
    int j = i + 1;
    while (j < count && png_goes_deep(png[j]) == deep) j++;
    void *const slots = deep ? (void *)mi_batch_device_input16(b, first + i) : (void *)mi_batch_device_input(b, first + i);
    if (int st = batch_png_expand(b, j - i, png + i, b->w, b->h, b->channels, slots, deep)) return st;
    batch_tag(b, first + i, j - i, deep ? MI_INPUT_RGB16 : MI_INPUT_RGB);
    i = j;
  }
  return MI_OK;
}

// ---- resize on input: a source of any size is resampled on the batch's stream into the slot (kernels: dev_resample.h) ----
// The filters and the coefficients of one axis, as Pillow computes them for 8-bit pictures (Image.resize, reducing_gap=None): all in double, in this order.
static double resample_filter(int filter, double x) {
  switch (filter) {
    case MI_RESAMPLE_BOX: return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
    case MI_RESAMPLE_BILINEAR: if (x < 0.0) x = -x; return x < 1.0 ? 1.0 - x : 0.0;
    case MI_RESAMPLE_BICUBIC: {
      const double a = -0.5;
      if (x < 0.0) x = -x;
      if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
      if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
      return 0.0;
    }
    default: {
      if (!(-3.0 <= x && x < 3.0)) return 0.0;
      auto sinc = [](double v) { if (v == 0.0) return 1.0; v = v * 3.14159265358979323846; return sin(v) / v; };
      return sinc(x) * sinc(x / 3);
    }
  }
}
static size_t resample_ksize(uint32_t in, uint32_t out, int filter) {
  if (in == out) return 1;
  static const double supports[4] = { 0.5, 1.0, 2.0, 3.0 };
  const double scale = (double)in / out;
  return (size_t)ceil(supports[filter] * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}
static size_t resample_axis_bytes(uint32_t in, uint32_t out, int filter) { return align_up((size_t)out * 8, 16) + align_up(resample_ksize(in, out, filter) * out * 4, 16); }
// bounds[2 i] = first sample, bounds[2 i + 1] = taps of output sample i; tap j of output i at taps[j * out + i], 22 fractional bits (unused ones 0).
// An axis that keeps its length: the identity (its pass is skipped: the kernel moves the samples unchanged).
static void resample_axis(uint32_t in, uint32_t out, int filter, uint32_t *bounds, int32_t *taps) {
  const size_t ksize = resample_ksize(in, out, filter);
  if (in == out) { for (uint32_t i = 0; i < out; i++) { bounds[2 * i] = i; bounds[2 * i + 1] = 1; taps[i] = 1 << MI_RS_BITS; } return; }
  static const double supports[4] = { 0.5, 1.0, 2.0, 3.0 };
  const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale, support = supports[filter] * fs;
  std::vector<double> k(ksize);
  memset(taps, 0, ksize * out * sizeof(int32_t));
  for (uint32_t i = 0; i < out; i++) {
    const double centre = (i + 0.5) * scale;
    int xmin = (int)(centre - support + 0.5), xmax = (int)(centre + support + 0.5);
    if (xmin < 0) xmin = 0;
    if (xmax > (int)in) xmax = (int)in;
    const int n = xmax - xmin;
    double sum = 0.0;
    for (int j = 0; j < n; j++) { k[j] = resample_filter(filter, (j + xmin - centre + 0.5) / fs); sum += k[j]; }
    for (int j = 0; j < n; j++) {
      const double v = sum != 0.0 ? k[j] / sum : k[j];
      taps[(size_t)j * out + i] = v < 0 ? (int)(-0.5 + v * (1 << MI_RS_BITS)) : (int)(0.5 + v * (1 << MI_RS_BITS));
    }
    bounds[2 * i] = (uint32_t)xmin; bounds[2 * i + 1] = (uint32_t)n;
  }
}

// the scratch holds `bytes` afterwards; an earlier call's kernels may still use the buffer that is replaced, so the stream is waited for first
static int batch_reserve_scratch(mi_batch *b, size_t bytes) {
  if (bytes <= b->d_rs_scratch_cap) return MI_OK;
  HIP_OK(hipStreamSynchronize(b->stream));
  return staging_grow(b->d_rs_scratch, b->d_rs_scratch_cap, bytes) ? MI_OK : MI_ENCODING_ERROR;
}

// The two passes: `count` pictures of s.w x s.h described by s -> slots [first, first + count).  The tables go into the batch's pinned staging and over in
// one H2D (a call with the sizes and the filter of the one before it finds them on the device); the intermediate lies `inter_at` bytes into the scratch,
// which the caller has reserved up to inter_at + resample_inter_bytes().  Stream order serialises the users of the scratch.  No sync.
static size_t resample_inter_bytes(int count, uint32_t src_h, uint32_t dst_w) { return (size_t)count * src_h * align_up(dst_w, 4) * 4; }
static int batch_resample(mi_batch *b, int first, int count, const IngestSrc &s, int filter, size_t inter_at) {
  const uint32_t key[5] = { s.w, s.h, b->w, b->h, (uint32_t)filter + 1 };
  const size_t h_bytes = resample_axis_bytes(s.w, b->w, filter), need = align_up(h_bytes + resample_axis_bytes(s.h, b->h, filter), 256);
  size_t at = b->rs_key_at;
  if (memcmp(key, b->rs_key, sizeof(key)) != 0) {
    if (b->rs_used + need > b->h_rs_cap || b->rs_used + need > b->d_rs_cap) {
      HIP_OK(hipStreamSynchronize(b->stream));                // earlier calls' copies and kernels may still use the buffers that start over or are replaced
      b->rs_used = 0; b->rs_key[4] = 0;
      if (!staging_grow(b->h_rs, b->h_rs_cap, need) || !staging_grow(b->d_rs, b->d_rs_cap, need)) return MI_ENCODING_ERROR;
    }
    at = b->rs_used; b->rs_used += need;
    uint8_t *const hb = b->h_rs.get() + at;
    resample_axis(s.w, b->w, filter, (uint32_t *)hb, (int32_t *)(hb + align_up((size_t)b->w * 8, 16)));
    resample_axis(s.h, b->h, filter, (uint32_t *)(hb + h_bytes), (int32_t *)(hb + h_bytes + align_up((size_t)b->h * 8, 16)));
    HIP_OK(hipMemcpyAsync(b->d_rs.get() + at, hb, need, hipMemcpyHostToDevice, b->stream));
    memcpy(b->rs_key, key, sizeof(key)); b->rs_key_at = at;
  }
  const uint8_t *const db = b->d_rs.get() + at;
  const uint32_t *const hbounds = (const uint32_t *)db, *const vbounds = (const uint32_t *)(db + h_bytes);
  const int32_t *const htaps = (const int32_t *)(db + align_up((size_t)b->w * 8, 16)), *const vtaps = (const int32_t *)(db + h_bytes + align_up((size_t)b->h * 8, 16));
  const uint32_t pitch = (uint32_t)align_up(b->w, 4);
  uint32_t *const inter = (uint32_t *)(b->d_rs_scratch.get() + inter_at);
  hipLaunchKernelGGL(resample_h_kernel, dim3((b->w + MI_RS_TW - 1) / MI_RS_TW, (s.h + MI_RS_TH - 1) / MI_RS_TH, (unsigned)count), dim3(64 * MI_RS_TH), 0, b->stream,
                     s, hbounds, htaps, b->w, pitch, inter);
  const dim3 grid(((b->w + 3) / 4 + 63) / 64, b->h, (unsigned)count);
  uint8_t *const slots = mi_batch_device_input(b, first);
  const int alpha = s.channels == 4 ? 1 : 0;
  if (b->channels == 4) hipLaunchKernelGGL((resample_v_kernel<4>), grid, dim3(64), 0, b->stream, (const uint32_t *)inter, s.h, pitch, vbounds, vtaps, b->w, b->h, alpha, slots);
  else hipLaunchKernelGGL((resample_v_kernel<3>), grid, dim3(64), 0, b->stream, (const uint32_t *)inter, s.h, pitch, vbounds, vtaps, b->w, b->h, alpha, slots);
  HIP_OK(hipGetLastError());
  batch_tag(b, first, count, MI_INPUT_RGB);
  return MI_OK;
}
static bool resample_filter_known(int filter) { return filter >= MI_RESAMPLE_BOX && filter <= MI_RESAMPLE_LANCZOS3; }
static bool resample_extent_ok(uint32_t w, uint32_t h) { return w >= 1 && h >= 1 && w <= 65536 && h <= 65536; }     // what a batch may have (the grids and the tables count on it)

// images [first, first + count) from pictures of src_w x src_h in the memory of the batch's device; of the batch's own size: mi_batch_upload_device
int mi_batch_resize_device(mi_batch *b, int first, int count, const mi_device_pixels *src, uint32_t src_w, uint32_t src_h, int filter) {
  if (!b || !src || !src->dev || b->in_flight || first < 0 || count < 1 || first > b->cap - count || !resample_filter_known(filter) || !resample_extent_ok(src_w, src_h)) return MI_INVALID_ARGUMENT;
  if ((src->layout != 0 && src->layout != 1) || (src->channels != 3 && src->channels != 4) || src->channels > b->channels) return MI_INVALID_ARGUMENT;   // alpha is never dropped
  if (src_w == b->w && src_h == b->h) return mi_batch_upload_device(b, first, count, src);
  IngestSrc s;
  s.base = (const uint8_t *)src->dev; s.w = src_w; s.h = src_h; s.layout = src->layout; s.channels = src->channels;
  const size_t packed_row = (size_t)src_w * (s.layout == 0 ? s.channels : 1);
  s.row_stride = src->row_stride ? src->row_stride : packed_row;
  s.inner_stride = src->pixel_or_plane_stride ? src->pixel_or_plane_stride : s.layout == 0 ? (size_t)s.channels : s.row_stride * src_h;
  s.image_stride = src->image_stride ? src->image_stride : s.layout == 0 ? s.row_stride * src_h : s.inner_stride * s.channels;
  if (s.row_stride < packed_row || s.inner_stride < (s.layout == 0 ? (size_t)s.channels : (size_t)src_w)) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  if (int st = batch_reserve_scratch(b, resample_inter_bytes(count, src_h, b->w))) return st;
  if (src->after_stream) {
    if (!b->ev_src) HIP_OK(hipEventCreateWithFlags(&b->ev_src, hipEventDisableTiming));
    HIP_OK(hipEventRecord(b->ev_src, (hipStream_t)src->after_stream));
    HIP_OK(hipStreamWaitEvent(b->stream, b->ev_src, 0));
  }
  return batch_resample(b, first, count, s, filter, 0);
}

// a decoded source at the start of the scratch, packed, `channels` channels: what the two forms below resample
static IngestSrc resample_scratch_source(const mi_batch *b, uint32_t w, uint32_t h, int channels) {
  IngestSrc s;
  s.base = b->d_rs_scratch.get(); s.w = w; s.h = h; s.layout = 0; s.channels = channels;
  s.inner_stride = (size_t)channels; s.row_stride = (size_t)w * channels; s.image_stride = s.row_stride * h;
  return s;
}

// one parsed JPEG of any size into slot `index`: decoded into the scratch as RGB (mi_batch_upload_jpeg's kernels), then the two passes; of the batch's own size: mi_batch_upload_jpeg
int mi_batch_resize_jpeg(mi_batch *b, int index, const mi_jpeg_coeffs *c, int filter) {
  if (!b || !c || b->in_flight || index < 0 || index >= b->cap || !resample_filter_known(filter)) return MI_INVALID_ARGUMENT;
  const JpegCoeffs &jc = c->jc;
  if (jc.w == b->w && jc.h == b->h) return mi_batch_upload_jpeg(b, index, c);
  if (!resample_extent_ok(jc.w, jc.h)) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  const size_t inter_at = align_up((size_t)jc.w * jc.h * 3, 256);
  if (int st = batch_reserve_scratch(b, inter_at + resample_inter_bytes(1, jc.h, b->w))) return st;
  if (int st = batch_jpeg_decode(b, jc, b->d_rs_scratch.get(), 3, jc.w)) return st;
  return batch_resample(b, index, 1, resample_scratch_source(b, jc.w, jc.h, 3), filter, inter_at);
}

// one parsed PNG of any size into slot `index`: unfiltered and expanded into the scratch (RGBA when the file has alpha or tRNS, else RGB), then the two passes; of
// the batch's own size: mi_batch_upload_png
int mi_batch_resize_png(mi_batch *b, int index, const mi_png_scanlines *p, int filter) {
  if (!b || !p || b->in_flight || index < 0 || index >= b->cap || !resample_filter_known(filter)) return MI_INVALID_ARGUMENT;
  const int channels = p->sl.has_alpha() ? 4 : 3;
  if (channels > b->channels) return MI_INVALID_ARGUMENT;     // alpha is never dropped
  if (p->sl.w == b->w && p->sl.h == b->h) return mi_batch_upload_png(b, index, 1, &p);
  if (!resample_extent_ok(p->sl.w, p->sl.h)) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  const size_t inter_at = align_up((size_t)p->sl.w * p->sl.h * channels, 256);
  if (int st = batch_reserve_scratch(b, inter_at + resample_inter_bytes(1, p->sl.h, b->w))) return st;
  if (int st = batch_png_expand(b, 1, &p, p->sl.w, p->sl.h, channels, b->d_rs_scratch.get())) return st;
  return batch_resample(b, index, 1, resample_scratch_source(b, p->sl.w, p->sl.h, channels), filter, inter_at);
}

// ravif::Encoder::encode_rgba / encode_rgb for a picture in the memory of device e->device (channels 4 / 3 as src->channels says)
int mi_ravif_encode_device(const mi_ravif_encoder *e, const mi_device_pixels *src, uint32_t w, uint32_t h, mi_encoded_image *out) {
  if (!e || !src || !src->dev || !out || w < 1 || h < 1 || (src->channels != 3 && src->channels != 4)) return MI_INVALID_ARGUMENT;
  mi_batch *b = pool_acquire(e, 1, w, h, src->channels);
  if (!b) return mi_device_count() > e->device ? MI_INVALID_ARGUMENT : MI_NO_DEVICE;
  int st = mi_batch_upload_device(b, 0, 1, src);
  if (st == MI_OK) st = mi_batch_encode(b);
  if (st == MI_OK) st = mi_batch_get(b, 0, out);
  pool_release(b);
  return st;
}
// the same for a uint16 picture in the memory of device e->device (mi_batch_upload_device16)
int mi_ravif_encode_device16(const mi_ravif_encoder *e, const mi_device_pixels16 *src, uint32_t w, uint32_t h, mi_encoded_image *out) {
  if (!e || !src || !src->dev || !out || w < 1 || h < 1 || (src->channels != 3 && src->channels != 4)) return MI_INVALID_ARGUMENT;
  mi_batch *b = pool_acquire(e, 1, w, h, src->channels);
  if (!b) return mi_device_count() > e->device ? MI_INVALID_ARGUMENT : MI_NO_DEVICE;
  int st = mi_batch_upload_device16(b, 0, 1, src);
  if (st == MI_OK) st = mi_batch_encode(b);
  if (st == MI_OK) st = mi_batch_get(b, 0, out);
  pool_release(b);
  return st;
}
// the same for YCbCr planes in the memory of device e->device: the file of a 3-channel batch fed through mi_batch_upload_device_ycbcr
int mi_ravif_encode_device_ycbcr(const mi_ravif_encoder *e, const mi_device_planes *src, uint32_t w, uint32_t h, mi_encoded_image *out) {
  if (!e || !src || !src->y || !src->cb || !out || w < 1 || h < 1) return MI_INVALID_ARGUMENT;
  mi_batch *b = pool_acquire(e, 1, w, h, 3);
  if (!b) return mi_device_count() > e->device ? MI_INVALID_ARGUMENT : MI_NO_DEVICE;
  int st = mi_batch_upload_device_ycbcr(b, 0, 1, src);
  if (st == MI_OK) st = mi_batch_encode(b);
  if (st == MI_OK) st = mi_batch_get(b, 0, out);
  pool_release(b);
  return st;
}
// the same for a picture of src_w x src_h that is resampled to w x h on the way in
int mi_ravif_encode_device_resized(const mi_ravif_encoder *e, const mi_device_pixels *src, uint32_t src_w, uint32_t src_h, uint32_t w, uint32_t h, int filter, mi_encoded_image *out) {
  if (!e || !src || !src->dev || !out || w < 1 || h < 1 || (src->channels != 3 && src->channels != 4)) return MI_INVALID_ARGUMENT;
  mi_batch *b = pool_acquire(e, 1, w, h, src->channels);
  if (!b) return mi_device_count() > e->device ? MI_INVALID_ARGUMENT : MI_NO_DEVICE;
  int st = mi_batch_resize_device(b, 0, 1, src, src_w, src_h, filter);
  if (st == MI_OK) st = mi_batch_encode(b);
  if (st == MI_OK) st = mi_batch_get(b, 0, out);
  pool_release(b);
  return st;
}

// The reference's files.into_par_iter() (src/main.rs:223) over the GPUs of one node: images are independent, so a host
// thread per device pulls runs of equally-shaped images from a shared cursor and pushes each run through one resident
// batch (no collective, no cross-device traffic).  status[i] receives the per-image result; returns the first failure.
// Streaming form of the fan-out: image i is obtained through `fetch(user, i, &desc)` when a worker is about to stage it (the
// call may block until the pixels exist -- e.g. until a loader thread has decoded the file), so loading, upload, encoding and
// assembly of consecutive runs overlap.  fetch returns MI_OK or a status that becomes the image's status.  An image is host pixels (kind 0) or the
// coefficients of a parsed JPEG (kind 1; kind 3: the same, kept as the file's own YCbCr) or the scanlines of a parsed PNG (kind 2; kind 4: the same, a file of bit depth 16 through its deep slot), whose pixels come into being in the batch's HBM input slot; mi_ravif_encode_stream is this
// with kind 0 throughout.
int mi_ravif_encode_sources(const mi_ravif_encoder *e, size_t n, mi_fetch_source_fn fetch, mi_release_fn release, void *user, mi_encoded_image *out, int *status, const int *devices, int ndev) {
  if (!e || !fetch || (n && !out)) return MI_INVALID_ARGUMENT;
  const int have = mi_device_count();
  std::vector<int> devs;
  if (devices && ndev > 0) devs.assign(devices, devices + ndev); else for (int d = 0; d < have; d++) devs.push_back(d);
  for (int d : devs) if (d < 0 || d >= have) { fprintf(stderr, "mi_avif: no HIP device %d (no CPU fallback)\n", d); return MI_NO_DEVICE; }
  if (devs.empty()) { fprintf(stderr, "mi_avif: no HIP device (no CPU fallback)\n"); return MI_NO_DEVICE; }
  std::vector<int> st(n, MI_OK);
  for (size_t i = 0; i < n; i++) { out[i].avif_file = nullptr; out[i].avif_len = out[i].color_byte_size = out[i].alpha_byte_size = 0; }
  std::atomic<size_t> cursor{ 0 };
  // A run holds at most 32 images, and no more than an even share of the job when it is small (64 files on 8 GPUs: 8 each, not 32 + 32 + nothing).
  const size_t max_run = std::min<size_t>(32, std::max<size_t>(1, (n + devs.size() - 1) / devs.size()));
  const bool timing = mi_timing_enabled();
  const auto t0 = std::chrono::steady_clock::now();
  auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3; };
  // Per device: two resident batch objects (from the pool) per image shape (MI_STREAM_SLOTS_DEFAULT).  While one batch encodes, the host fills the next one's
  // pinned staging and enqueues its H2D + encode, so uploads, tile search, entropy coding and the host-side assembly of consecutive runs overlap
  // (the same rotation bench.py drives).  Memory is bounded: a batch object holds as many images of its shape as fit MI_SLOT_BYTES (one 12 MP RGBA
  // image needs ~1.5 GB: such a shape gets runs of a few images, not 32), and before a new object is made the worker gives back the objects of the
  // shapes it has not used for the longest time until the total stays under its budget (a share of the device's free memory at the start).
  constexpr size_t MI_SLOT_BYTES = (size_t)8 << 30;
  auto est_bytes = [](uint32_t w, uint32_t h, int ch, size_t images) { return images * (size_t)w * h * (ch == 4 ? 110 : 82) + ((size_t)32 << 20); };   // arena + records + staging per pixel (measured on the planner)
  // what a batch object adds at its first JPEG image: MI_BATCH_JPEG_STAGED images' coefficients (at most three full planes of int16) pinned and on the device, one image's planes
  auto est_jpeg_bytes = [](uint32_t w, uint32_t h) { return ((size_t)w + 15) * ((size_t)h + 15) * (2 * MI_BATCH_JPEG_STAGED * 6 + 3) + ((size_t)3 << 20); };
  auto worker = [&](int dev) {
    mi_ravif_encoder enc = *e; enc.device = dev;
    std::future<int> warm = std::async(std::launch::async, [dev]() { return hipSetDevice(dev) == hipSuccess ? ensure_tables(dev) : (int)MI_ENCODING_ERROR; });
    size_t budget = (size_t)48 << 30;
    { size_t fr = 0, tot = 0; if (hipSetDevice(dev) == hipSuccess && hipMemGetInfo(&fr, &tot) == hipSuccess && fr) budget = fr / 10 * 6; }
    { int sharing = 0; for (int d2 : devs) sharing += d2 == dev; budget /= (size_t)std::max(1, sharing); }      // workers on the same ordinal (devices = [0, 0]) split what is free
    static constexpr int NSLOT_MAX = 4;
    const int NSLOT = MI_STREAM_SLOTS_DEFAULT;
    struct Slot { mi_batch *b = nullptr; std::future<mi_batch *> making; std::vector<size_t> idx; bool busy = false, jpeg = false, deep = false; size_t bytes = 0, png_bytes = 0; };
    struct Shape { uint32_t w, h; int ch; size_t cap; Slot slot[NSLOT_MAX]; int next = 0; size_t runs = 0, last_use = 0; };
    std::vector<std::unique_ptr<Shape>> shapes;
    size_t live_bytes = 0, tick = 0;
    auto collect = [&](Slot &sl) {
      if (!sl.busy) return;
      const int rc = mi_batch_wait(sl.b);
      if (timing) fprintf(stderr, "[mi_avif %8.1f ms] dev %d: run of %zu done (on the device: front end %.1f, tile search %.1f, deblock %.1f, cdef + restoration %.1f, entropy %.1f, pack + D2H %.1f ms)\n", since(), dev, sl.idx.size(),
                          mi_batch_stage_ms(sl.b, 0), mi_batch_stage_ms(sl.b, 1), mi_batch_stage_ms(sl.b, 2), mi_batch_stage_ms(sl.b, 3), mi_batch_stage_ms(sl.b, 4), mi_batch_stage_ms(sl.b, 5));
      for (size_t k = 0; k < sl.idx.size(); k++) st[sl.idx[k]] = rc == MI_OK ? mi_batch_get(sl.b, (int)k, &out[sl.idx[k]]) : rc;
      sl.busy = false;
    };
    auto drop = [&](Slot &sl) {                                 // finish the slot's run and give its object back to the device
      collect(sl);
      if (sl.making.valid()) sl.b = sl.making.get();
      if (sl.b) mi_batch_destroy(sl.b);
      sl.b = nullptr; live_bytes -= std::min(live_bytes, sl.bytes); sl.bytes = 0; sl.jpeg = false; sl.deep = false; sl.png_bytes = 0;
    };
    auto make_room = [&](Shape *keep, size_t need) {
      while (live_bytes + need > budget) {
        Shape *victim = nullptr;
        for (auto &c : shapes) if (c.get() != keep && (!victim || c->last_use < victim->last_use)) { bool any = false; for (Slot &sl : c->slot) any |= sl.b || sl.making.valid(); if (any) victim = c.get(); }
        if (!victim) break;
        for (Slot &sl : victim->slot) drop(sl);
      }
    };
    auto ensure_slot = [&](Shape *sh, int j, bool host_staging, size_t png_staging) {
      Slot &sl = sh->slot[j];
      if (sl.b || sl.making.valid()) return;
      const size_t need = est_bytes(sh->w, sh->h, sh->ch, sh->cap);
      make_room(sh, need);
      sl.bytes = need; live_bytes += need;
      const mi_ravif_encoder ec = enc; const uint32_t w = sh->w, h = sh->h; const int ch = sh->ch; const int c = (int)sh->cap;
      // the pinned pixel staging with it when host pixels are coming (a run of JPEG / PNG sources never pins it)
      // and the PNG staging when scanlines are coming (png_staging: the bytes a full run is expected to need; a call that needs more grows it)
      sl.making = std::async(std::launch::async, [ec, c, w, h, ch, host_staging, png_staging]() {
        mi_batch *nb = pool_acquire(&ec, c, w, h, ch);
        if (nb && host_staging) (void)mi_batch_input(nb, 0);
        if (nb && png_staging) (void)batch_reserve_png(nb, png_staging);
        return nb;
      });
    };
    auto shape_for = [&](const mi_image_desc &x) {
      for (auto &c : shapes) if (c->w == x.width && c->h == x.height && c->ch == x.channels) return c.get();
      const size_t per = est_bytes(x.width, x.height, x.channels, 1);
      const size_t cap = std::max<size_t>(1, std::min(max_run, MI_SLOT_BYTES / per));
      shapes.emplace_back(new Shape{ x.width, x.height, x.channels, cap, {}, 0, 0, 0 });
      return shapes.back().get();
    };
    // one run (<= the shape's capacity) through the shape's next slot
    auto submit = [&](Shape *sh, const std::vector<mi_image_source> &d, const std::vector<size_t> &run, size_t i0, bool more) {
      const mi_image_desc &d0 = d[run[0]].desc;
      sh->last_use = ++tick; sh->runs++;
      const int j = sh->next; sh->next = (j + 1) % NSLOT;
      Slot &sl = sh->slot[j];
      collect(sl);                                           // the slot's previous run, if any
      bool any_host = false; for (size_t k : run) any_host |= d[k].kind == 0;
      size_t png_run = 0; { std::vector<const mi_png_scanlines *> all; for (size_t k : run) if (d[k].kind == 2 || d[k].kind == 4) all.push_back(d[k].png); if (!all.empty()) png_run = png_call_bytes((int)all.size(), all.data()); }
      ensure_slot(sh, j, any_host, png_run);
      if (sl.making.valid()) sl.b = sl.making.get();
      if (!sl.b) { live_bytes -= std::min(live_bytes, sl.bytes); sl.bytes = 0; sl.jpeg = false; sl.deep = false; sl.png_bytes = 0; }      // the object could not be made: nothing of it is resident
      int rc = sl.b ? mi_batch_set_count(sl.b, (int)run.size()) : MI_ENCODING_ERROR;
      if (timing) fprintf(stderr, "[mi_avif %8.1f ms] dev %d: slot %d ready\n", since(), dev, j);
      if (rc == MI_OK) {
        // host images: pinned staging, then one H2D per stretch of neighbours (never across a JPEG or PNG image's slot: the staging there is stale).  JPEG images:
        // coefficients to the batch's own staging, decoded into the slot on the batch's stream.  PNG images: a stretch of neighbours goes up in one
        // mi_batch_upload_png call (one H2D, one launch per kernel); what the batch's PNG staging holds, pinned and on the device, joins the worker's budget.
        const size_t row = (size_t)d0.width * d0.channels;
        size_t host_from = 0;
        auto upload_host = [&](size_t end) { if (rc == MI_OK && end > host_from) rc = mi_batch_upload_async(sl.b, (int)host_from, (int)(end - host_from)); };
        std::vector<const mi_png_scanlines *> pngs; size_t png_from = 0; int png_kind = 2;       // a stretch holds one kind: 2 goes through mi_batch_upload_png, 4 through _png_deep
        auto upload_png = [&]() {
          if (rc == MI_OK && !pngs.empty()) {
            const size_t extra = 2 * (png_call_bytes((int)pngs.size(), pngs.data()) + ((size_t)1 << 20));
            if (extra > sl.png_bytes) { sl.bytes += extra - sl.png_bytes; live_bytes += extra - sl.png_bytes; sl.png_bytes = extra; }
            if (png_kind == 4 && !sl.deep) { sl.deep = true; const size_t deep = sh->cap * (size_t)sh->w * sh->h * sh->ch * 2; sl.bytes += deep; live_bytes += deep; }   // the deep slots join the worker's budget
            rc = png_kind == 4 ? mi_batch_upload_png_deep(sl.b, (int)png_from, (int)pngs.size(), pngs.data()) : mi_batch_upload_png(sl.b, (int)png_from, (int)pngs.size(), pngs.data());
          }
          pngs.clear();
        };
        for (size_t k = 0; k < run.size() && rc == MI_OK; k++) {
          const mi_image_source &src = d[run[k]];
          if (src.kind == 2 || src.kind == 4) {
            upload_host(k); host_from = k + 1;
            if (!pngs.empty() && png_kind != src.kind) upload_png();
            if (pngs.empty()) { png_from = k; png_kind = src.kind; }
            pngs.push_back(src.png);
            continue;
          }
          upload_png();
          if (src.kind == 1 || src.kind == 3) {
            upload_host(k); host_from = k + 1;
            if (!sl.jpeg) { sl.jpeg = true; const size_t extra = est_jpeg_bytes(sh->w, sh->h); sl.bytes += extra; live_bytes += extra; }
            if (rc == MI_OK) rc = src.kind == 3 ? mi_batch_upload_jpeg_ycbcr(sl.b, (int)k, src.jpeg) : mi_batch_upload_jpeg(sl.b, (int)k, src.jpeg);
            continue;
          }
          const mi_image_desc &x = src.desc;
          uint8_t *dst = mi_batch_input(sl.b, (int)k);
          if (!dst) { rc = MI_ENCODING_ERROR; break; }
          const size_t sp = x.stride_px ? x.stride_px : x.width;
          if (sp == x.width) memcpy(dst, x.pixels, row * d0.height);
          else for (uint32_t y = 0; y < d0.height; y++) memcpy(dst + y * row, x.pixels + (size_t)y * sp * d0.channels, row);
        }
        upload_png();
        upload_host(run.size());
        if (timing) fprintf(stderr, "[mi_avif %8.1f ms] dev %d: slot %d staged, uploads enqueued\n", since(), dev, j);
      }
      if (release) for (size_t k : run) release(user, i0 + k);   // staged (or failed): the caller's pixels are no longer read
      if (rc == MI_OK) rc = mi_batch_encode_async(sl.b);
      if (timing) fprintf(stderr, "[mi_avif %8.1f ms] dev %d: run of %zu enqueued on slot %d\n", since(), dev, run.size(), j);
      if (rc != MI_OK) { for (size_t k : run) st[i0 + k] = rc; return; }
      sl.idx.clear(); for (size_t k : run) sl.idx.push_back(i0 + k);
      sl.busy = true;
      // a shape that keeps coming gets its next slot made while the GPU works on this run (not earlier: hipMalloc / hipHostMalloc on another
      // thread hold runtime locks that stall this thread's copies and launches; not for a shape seen once: a directory of differently sized files)
      if (more && sh->runs >= 2) ensure_slot(sh, sh->next, any_host, png_run);
    };
    size_t claims = 0;
    for (;;) {
      // every claim is a full run, the first one included (MI_STREAM_FIRST_RUN_NUM / _DEN)
      const size_t first_run = std::max<size_t>(1, max_run * MI_STREAM_FIRST_RUN_NUM / MI_STREAM_FIRST_RUN_DEN);
      const size_t want = claims++ == 0 ? first_run : max_run;
      const size_t i0 = cursor.fetch_add(want);                // claim the index range [i0, i1)
      if (i0 >= n) break;
      const size_t i1 = std::min(n, i0 + want);
      std::vector<mi_image_source> d(i1 - i0);
      // images are staged in arrival order: a run is handed over as soon as the next image has another shape or the run is full
      std::vector<size_t> run; Shape *run_shape = nullptr;
      auto flush = [&](bool more) { if (!run.empty()) { submit(run_shape, d, run, i0, more); run.clear(); } };
      for (size_t i = i0; i < i1; i++) {
        const int rc = fetch(user, i, &d[i - i0]);
        const mi_image_source &src = d[i - i0];
        const mi_image_desc &x = src.desc;
        if (rc != MI_OK) { st[i] = rc; continue; }
        const bool have = src.kind == 0 ? x.pixels != nullptr : (src.kind == 1 || src.kind == 3) ? src.jpeg && src.jpeg->jc.w == x.width && src.jpeg->jc.h == x.height :
                          (src.kind == 2 || src.kind == 4) && src.png && src.png->sl.w == x.width && src.png->sl.h == x.height && !(x.channels == 3 && src.png->sl.has_alpha());
        if (!have || !x.width || !x.height || (x.channels != 3 && x.channels != 4)) { st[i] = MI_INVALID_ARGUMENT; if (release) release(user, i); continue; }
        // a kind-3 source that its upload call would refuse fails alone, not with its run
        if (src.kind == 3 && (src.jpeg->jc.color == JPEG_RGB || e->color_model == 1 || (x.channels == 4 && e->alpha_mode == 2))) {
          st[i] = src.jpeg->jc.color == JPEG_RGB && e->color_model != 1 && !(x.channels == 4 && e->alpha_mode == 2) ? MI_UNSUPPORTED : MI_INVALID_ARGUMENT;
          if (release) release(user, i);
          continue;
        }
        // so does a kind-4 source of bit depth 16 under an alpha mode that takes no deep image of its channels (batch_takes_deep)
        if (src.kind == 4 && png_goes_deep(src.png) && x.channels == 4 && (src.png->sl.has_alpha() ? e->alpha_mode != 0 : e->alpha_mode == 2)) {
          st[i] = MI_INVALID_ARGUMENT;
          if (release) release(user, i);
          continue;
        }
        Shape *sh = shape_for(x);
        if (sh != run_shape || run.size() >= sh->cap) flush(true);
        run_shape = sh; run.push_back(i - i0);
        if (run.size() == 1) ensure_slot(sh, sh->next, src.kind == 0, src.kind == 2 || src.kind == 4 ? sh->cap * png_call_bytes(1, &src.png) : 0);   // made in the background while the rest of the run arrives
      }
      if (timing) fprintf(stderr, "[mi_avif %8.1f ms] dev %d: images %zu..%zu fetched\n", since(), dev, i0, i1);
      flush(cursor.load() < n);
    }
    for (auto &c : shapes) for (Slot &sl : c->slot) {
      collect(sl);
      if (sl.making.valid()) sl.b = sl.making.get();
      pool_release(sl.b);                                      // back to the pool: the next call (or nobody, at process exit) gets them
      sl.b = nullptr;
    }
    warm.get();
    if (timing) fprintf(stderr, "[mi_avif %8.1f ms] dev %d: worker done\n", since(), dev);
  };
  std::vector<std::thread> th;
  for (int d : devs) th.emplace_back(worker, d);
  for (auto &t : th) t.join();
  int first = MI_OK;
  for (size_t i = 0; i < n; i++) { if (status) status[i] = st[i]; if (first == MI_OK && st[i] != MI_OK) first = st[i]; }
  return first;
}
// the host-pixel form: every source is kind 0
struct StreamAdapter { mi_fetch_fn fetch; mi_release_fn release; void *user; };
static int fetch_host_source(void *user, size_t i, mi_image_source *src) { const StreamAdapter *a = (const StreamAdapter *)user; src->kind = 0; src->jpeg = nullptr; src->png = nullptr; return a->fetch(a->user, i, &src->desc); }
static void release_host_source(void *user, size_t i) { const StreamAdapter *a = (const StreamAdapter *)user; a->release(a->user, i); }
int mi_ravif_encode_stream(const mi_ravif_encoder *e, size_t n, mi_fetch_fn fetch, mi_release_fn release, void *user, mi_encoded_image *out, int *status, const int *devices, int ndev) {
  if (!e || !fetch || (n && !out)) return MI_INVALID_ARGUMENT;
  StreamAdapter a{ fetch, release, user };
  return mi_ravif_encode_sources(e, n, fetch_host_source, release ? release_host_source : nullptr, &a, out, status, devices, ndev);
}
// The reference's files.into_par_iter() (src/main.rs:223) over the GPUs of one node with every image already in host memory.
static int fetch_from_array(void *user, size_t i, mi_image_desc *d) { *d = ((const mi_image_desc *)user)[i]; return MI_OK; }
int mi_ravif_encode_batch(const mi_ravif_encoder *e, size_t n, const mi_image_desc *in, mi_encoded_image *out, int *status, const int *devices, int ndev) {
  if (!e || (n && (!in || !out))) return MI_INVALID_ARGUMENT;
  return mi_ravif_encode_stream(e, n, fetch_from_array, nullptr, (void *)in, out, status, devices, ndev);
}
int mi_ravif_encode_rgb(const mi_ravif_encoder *e, const uint8_t *rgb, uint32_t w, uint32_t h, size_t stride_px, mi_encoded_image *out) { return encode_one(e, rgb, 3, w, h, stride_px, out); }

// level 1: caller-supplied planes (encode_to_av1). Planes go straight into the frame's src[] (edge-replicated on the host).
int mi_av1_encode_planes(const mi_av1_config *cfg, const void *const planes[3], const size_t stride_bytes[3], uint8_t **out_obu, size_t *out_len, uint16_t *recon[3]) {
  if (!cfg || !planes || !planes[0] || !stride_bytes || !out_obu || !out_len || (cfg->bit_depth != 8 && cfg->bit_depth != 10)) return MI_INVALID_ARGUMENT;
  // rav1e rejects these with InvalidWidth / InvalidHeight (the sequence header carries at most 16 bits per dimension)
  if (cfg->width < 1 || cfg->height < 1 || cfg->width > 65536 || cfg->height > 65536 || mi_plane_too_large(cfg->width, cfg->height)) return MI_INVALID_ARGUMENT;
  auto pow2_4_64 = [](int v) { return v == 4 || v == 8 || v == 16 || v == 32 || v == 64; };
  if (!pow2_4_64(cfg->part_min) || !pow2_4_64(cfg->part_max) || cfg->part_min > cfg->part_max || cfg->chroma > 1) return MI_INVALID_ARGUMENT;
  if (mi_device_count() <= cfg->device) { fprintf(stderr, "mi_avif: no HIP device %d (no CPU fallback)\n", cfg->device); return MI_NO_DEVICE; }
  HIP_OK(hipSetDevice(cfg->device));
  if (int st = ensure_tables(cfg->device)) return st;
  // the stream and, through the frame set, every device allocation live for this call: all return paths release them (the set first)
  struct Stream { hipStream_t s = nullptr; ~Stream() { if (s) (void)hipStreamDestroy(s); } } stream;
  FrameSet fs;
  fs.frames.resize(1); fs.frames[0].cfg = *cfg; plan_geometry(fs.frames[0]);
  FramePlan &p = fs.frames[0];
  for (int i = 0; i < p.np; i++) if (!planes[i]) return MI_TOO_FEW_PIXELS;
  HIP_OK(hipStreamCreate(&stream.s));
  hipStream_t s = stream.s;
  if (int st = fs.reserve(fs.frames, cfg->device, s)) return st;
  fs.place();
  const size_t npx = (size_t)p.pw * p.ph;
  std::vector<uint16_t> host(npx);
  for (int i = 0; i < p.np; i++) {
    for (int y = 0; y < p.ph; y++) {
      const uint8_t *row = (const uint8_t *)planes[i] + (size_t)std::min<int>(y, cfg->height - 1) * stride_bytes[i];
      for (int x = 0; x < p.pw; x++) { const int sx = std::min<int>(x, cfg->width - 1); host[(size_t)y * p.pw + x] = cfg->bit_depth == 8 ? row[sx] : ((const uint16_t *)row)[sx]; }
    }
    HIP_OK(hipMemcpy(p.dev.src[i], host.data(), npx * 2, hipMemcpyHostToDevice));
  }
  if (int st = fs.stage(s)) return st;
  if (int st = fs.enqueue_chain(s, nullptr)) return st;
  if (int st = fs.enqueue_readback(s)) return st;
  HIP_OK(hipStreamSynchronize(s));
  if (int st = fs.check_lengths()) return st;
  std::vector<std::vector<uint8_t>> td(p.ntiles); std::vector<const uint8_t *> tiles;
  for (int j = 0; j < p.ntiles; j++) {
    td[j].resize(fs.h_lens.get()[j]);
    HIP_OK(hipMemcpy(td[j].data(), p.dev.tile_out + (size_t)j * p.dev.tile_out_cap, td[j].size(), hipMemcpyDeviceToHost));
    tiles.push_back(td[j].data());
  }
  fs.assemble(0, tiles);
  const std::vector<uint8_t> &obu = p.obu;
  uint16_t *rec_out[3] = { nullptr, nullptr, nullptr };
  if (recon) for (int i = 0; i < p.np; i++) {
    rec_out[i] = (uint16_t *)malloc((size_t)cfg->width * cfg->height * 2);
    const hipError_t e = rec_out[i] ? hipMemcpy2D(rec_out[i], (size_t)cfg->width * 2, p.cfg.lrf ? p.dev.lrp[i] : p.dev.fin[i], (size_t)p.pw * 2, (size_t)cfg->width * 2, cfg->height, hipMemcpyDeviceToHost) : hipErrorOutOfMemory;
    if (e != hipSuccess) { for (int k = 0; k <= i; k++) free(rec_out[k]); return MI_ENCODING_ERROR; }
  }
  *out_obu = (uint8_t *)malloc(obu.size());
  if (!*out_obu) { for (int k = 0; k < 3; k++) free(rec_out[k]); return MI_ENCODING_ERROR; }
  memcpy(*out_obu, obu.data(), obu.size()); *out_len = obu.size();
  if (recon) for (int i = 0; i < 3; i++) recon[i] = rec_out[i];
  return MI_OK;
}

static int raw_planes(const mi_ravif_encoder *e, uint32_t w, uint32_t h, const void *yuv, const void *alpha, int depth, uint8_t range, uint8_t matrix, mi_encoded_image *out) {
  if (!e || !yuv || !out || w < 1 || h < 1) return MI_INVALID_ARGUMENT;
  const size_t n = (size_t)w * h, bps = depth == 8 ? 1 : 2;
  std::vector<uint8_t> pl[3]; for (auto &v : pl) v.resize(n * bps);
  for (size_t i = 0; i < n; i++) for (int c = 0; c < 3; c++) {
    if (depth == 8) pl[c][i] = ((const uint8_t *)yuv)[i * 3 + c]; else ((uint16_t *)pl[c].data())[i] = ((const uint16_t *)yuv)[i * 3 + c];
  }
  mi_av1_config c{}; c.width = w; c.height = h; c.bit_depth = (uint8_t)depth; c.quantizer = (uint8_t)quality_to_quantizer(e->quality);
  c.chroma = 0; c.pixel_range = range; c.threads = e->threads; c.has_color_desc = 1; c.primaries = 1; c.transfer = 13; c.matrix = matrix; c.device = e->device; c.tiles_override = e->tiles_override; c.rdo_passes = (uint8_t)(e->rdo_passes == 2 ? 2 : 1);
  if (int st = tweaks_from_preset(e->speed, c.quantizer, &c)) return st;
  const void *pp[3] = { pl[0].data(), pl[1].data(), pl[2].data() }; const size_t sb[3] = { w * bps, w * bps, w * bps };
  uint8_t *cobu = nullptr, *aobu = nullptr; size_t clen = 0, alen = 0;
  if (int st = mi_av1_encode_planes(&c, pp, sb, &cobu, &clen, nullptr)) return st;
  if (alpha) {
    mi_av1_config a = c; a.quantizer = (uint8_t)quality_to_quantizer(e->alpha_quality); a.chroma = 1; a.pixel_range = 1; a.has_color_desc = 0;
    tweaks_from_preset(e->speed, a.quantizer, &a);
    const void *ap[3] = { alpha, nullptr, nullptr };
    if (int st = mi_av1_encode_planes(&a, ap, sb, &aobu, &alen, nullptr)) { free(cobu); return st; }
  }
  out->avif_len = mi_avif_serialize(cobu, clen, aobu, alen, w, h, (uint8_t)depth, matrix, e->alpha_mode == 2, e->exif, e->exif_len, &out->avif_file);
  out->color_byte_size = clen; out->alpha_byte_size = alen;
  free(cobu); free(aobu);
  return MI_OK;
}
int mi_ravif_encode_raw_planes_8(const mi_ravif_encoder *e, uint32_t w, uint32_t h, const uint8_t *yuv, const uint8_t *alpha, uint8_t range, uint8_t matrix, mi_encoded_image *out) { return raw_planes(e, w, h, yuv, alpha, 8, range, matrix, out); }
int mi_ravif_encode_raw_planes_10(const mi_ravif_encoder *e, uint32_t w, uint32_t h, const uint16_t *yuv, const uint16_t *alpha, uint8_t range, uint8_t matrix, mi_encoded_image *out) { return raw_planes(e, w, h, yuv, alpha, 10, range, matrix, out); }

}  // extern "C"
