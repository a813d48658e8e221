// mi_avif.hip -- the entry points of include/mi_avif.h: the batch's lifecycle and its encode (K0 front end, pack + D2H, AVIF containers, timing), its
// pool, the one-call entry points and the level-1 plane encoder.  Every call through which pixels reach a slot or leave it (host, device,
// JPEG, PNG, 16-bit, resize, colour management, orientation, decoded output) is host_input.h, included below the pool; the stream fan-out (source kinds, per-device worker, mi_ravif_encode_sources /
// _stream / _batch) is host_stream.h, included below the one-call entry points.  The frame chain they all run (plans, arena, K1 tile search, K2 deblock,
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
#include "dev_resample16.h"
#include "icc_reader.h"
#include "dev_colour.h"
#include "dev_orient.h"
#include "dev_float.h"
#include "dev_decoded16.h"
#include "host_frames.h"

// The product library reads no environment variables; probe builds (tools/) get MI_AVIF_TIMING=1 (-DMI_TUNING_KNOBS: host-side timeline on stderr)
// and MI_DEBUG_LEVEL (-DMI_DEBUG_HOOKS=1: bisect levels of the tile search).
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
  mi_ravif_encoder enc{}; int n = 0; uint32_t w = 0, h = 0; int channels = 3, device = 0, depth = 10;     // w x h: the reference size, what the batch was created for
  // the layout: per slot its width, height and the sample offset of its first sample in the slot arrays (8-bit, deep, pinned staging, cleaned pixels
  // alike).  Uniform: cap slots of w x h at i * w * h * channels.  Mixed (mi_batch_set_sizes): the n pictures of the run back to back, the slots behind them empty
  std::vector<uint32_t> slot_w, slot_h; std::vector<size_t> slot_at; bool mixed = false; size_t run_px = 0;       // run_px: the pixels of the run's n pictures
  std::vector<uint8_t> exif;                                       // the batch's own copy of enc.exif (the caller's buffer need not outlive mi_batch_create)
  hipStream_t stream = nullptr;
  int cap = 0;                                                     // images the batch was created for (n = images of the current run <= cap)
  DevBuf<uint8_t> d_pixels; size_t pixel_bytes = 0;               // cap * w*h*channels
  std::mutex staging_mu; PinBuf<uint8_t> h_pixels;                                        // pinned staging of the same size and layout: the H2D source (async, no pageable copies); made by the first mi_batch_input (a batch fed
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
  uint32_t rs_key[6] = { 0, 0, 0, 0, 0, 0 }; size_t rs_key_at = 0;  // oriented src_w, src_h, dst_w, dst_h, filter + 1, fractional bits of the tables at rs_key_at (0 in [4]: none)
  // quality metrics (mi_batch_measure): `encoded` = the planes of a completed encode of the current image count are on the device, `measured` = h_quality holds
  // that encode's records.  The records live at the end of the arena (FrameSet::d_records); their pinned D2H target is made by the first measure.
  bool encoded = false, measured = false;
  PinBuf<QualityRec> h_quality; size_t h_quality_bytes = 0;
  // decoded pixels (mi_batch_decode): one image of w*h*4 bytes on the device, made by the first call that decodes into host memory
  DevBuf<uint8_t> d_decoded; size_t d_decoded_cap = 0;
  // what the samples of each input slot mean (MI_INPUT_RGB / _YCBCR in the 8-bit slots, MI_INPUT_RGB16 / _YCBCR16 in the deep ones): host state, set by
  // whichever call last filled the slot, kept across encodes and mi_batch_set_count like the slot's contents
  std::vector<uint8_t> kinds;
  // deep input: the slots of kinds MI_INPUT_RGB16 and MI_INPUT_YCBCR16, cap * w*h*channels uint16 samples laid out like d_pixels; made by the first call that needs
  // them (under staging_mu), never by a batch that sees no 16-bit source
  DevBuf<uint16_t> d_pixels16; size_t deep_bytes = 0;
};
static_assert(sizeof(QualityRec) <= MI_FRAME_RECORD_BYTES, "FrameSet reserves MI_FRAME_RECORD_BYTES per (frame, plane)");

// ---- the layout's accessors: nothing below reads b->w / b->h for a slot ----
static uint32_t slot_w(const mi_batch *b, int i) { return b->slot_w[i]; }
static uint32_t slot_h(const mi_batch *b, int i) { return b->slot_h[i]; }
static size_t slot_px(const mi_batch *b, int i) { return (size_t)b->slot_w[i] * b->slot_h[i]; }
static size_t slot_samples(const mi_batch *b, int i) { return slot_px(b, i) * b->channels; }
static size_t slot_at(const mi_batch *b, int i) { return b->slot_at[i]; }
static int batch_slots(const mi_batch *b) { return b->mixed ? b->n : b->cap; }                   // the slots that can be addressed
// slots [first, first + count) have one size (the calls that describe their pictures with one size ask this)
static bool slots_one_size(const mi_batch *b, int first, int count) {
  for (int i = first + 1; i < first + count; i++) if (b->slot_w[i] != b->slot_w[first] || b->slot_h[i] != b->slot_h[first]) return false;
  return true;
}
static void batch_layout_uniform(mi_batch *b) {
  b->mixed = false;
  b->slot_w.assign(b->cap, b->w); b->slot_h.assign(b->cap, b->h); b->slot_at.resize(b->cap);
  for (int i = 0; i < b->cap; i++) b->slot_at[i] = (size_t)i * b->w * b->h * b->channels;
  b->run_px = (size_t)b->n * b->w * b->h;
}


// The filters address samples inside a plane with 32-bit offsets (row * stride + column): a padded plane must stay below 2^31 samples.  That is 60 x the largest picture
// any AV1 level allows (level 6.x: 35.6 MPix); beyond it the entry points answer MI_INVALID_ARGUMENT instead of filtering the wrong samples.
static bool mi_plane_too_large(uint32_t w, uint32_t h) {
  const uint64_t pw = ((uint64_t)w + 63) & ~63ull, ph = ((uint64_t)h + 63) & ~63ull;
  return (pw + 64) * (ph + 64) >= (1ull << 31);
}

// frame plans of n pictures of the given sizes: colour for every image [0, n), then (RGBA input) one alpha frame per image [n, 2n) -- whether an alpha
// frame is used is decided on the device (FrameDev::active)
static std::vector<FramePlan> batch_plans(const mi_batch *b, int n, const uint32_t *ws, const uint32_t *hs) {
  std::vector<FramePlan> frames;
  const int quantizer = quality_to_quantizer(b->enc.quality), aquant = quality_to_quantizer(b->enc.alpha_quality);
  auto make = [&](int image, bool alpha) {
    FramePlan p; p.image = image; p.is_alpha = alpha;
    mi_av1_config &c = p.cfg;
    c.width = ws[image]; c.height = hs[image]; c.bit_depth = (uint8_t)b->depth; c.quantizer = (uint8_t)(alpha ? aquant : quantizer);
    c.chroma = alpha ? 1 : 0; c.pixel_range = 1; c.threads = b->enc.threads; c.device = b->device; c.tiles_override = b->enc.tiles_override; c.rdo_passes = (uint8_t)(b->enc.rdo_passes == 2 ? 2 : 1);
    c.has_color_desc = alpha ? 0 : 1; c.primaries = 1; c.transfer = 13; c.matrix = b->enc.color_model == 1 ? 0 : 6;
    tweaks_from_preset(b->enc.speed, c.quantizer, &c);
    plan_geometry(p);
    return p;
  };
  for (int i = 0; i < n; i++) frames.push_back(make(i, false));
  if (b->channels == 4) for (int i = 0; i < n; i++) frames.push_back(make(i, true));
  return frames;
}
static void batch_plan(mi_batch *b) { b->fs.frames = batch_plans(b, b->n, b->slot_w.data(), b->slot_h.data()); }      // (re)build the plans of the run's pictures

// The status mi_batch_set_sizes gives a layout (mi_batch_fits hands it out as it is): host arithmetic over the plans, nothing is allocated, launched or changed
static int batch_layout_status(const mi_batch *b, int n, const uint32_t *ws, const uint32_t *hs) {
  if (!b || !ws || !hs || n < 1) return MI_INVALID_ARGUMENT;
  for (int i = 0; i < n; i++) if (ws[i] < 1 || hs[i] < 1 || ws[i] > 65536 || hs[i] > 65536 || mi_plane_too_large(ws[i], hs[i])) return MI_INVALID_ARGUMENT;
  if (n > b->cap) return MI_UNSUPPORTED;
  size_t px = 0;
  for (int i = 0; i < n; i++) px += (size_t)ws[i] * hs[i];
  if (px > (size_t)b->cap * b->w * b->h) return MI_UNSUPPORTED;                                  // the slot arrays
  if (b->channels == 4 && b->enc.alpha_mode == 1)                                              // the cleaner's one-image scratch
    for (int i = 0; i < n; i++) if ((size_t)ws[i] * hs[i] > (size_t)b->w * b->h) return MI_UNSUPPORTED;
  try { return b->fs.fits(batch_plans(b, n, ws, hs), b->stream) ? MI_OK : MI_UNSUPPORTED; } catch (const std::exception &) { return MI_ENCODING_ERROR; }
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
  batch_layout_uniform(b);
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

int mi_batch_set_count(mi_batch *b, int n_images) {
  if (!b || b->in_flight || n_images < 1 || n_images > b->cap) return MI_INVALID_ARGUMENT;
  b->n = n_images; b->alpha_flags.assign(n_images, 0);
  b->encoded = b->measured = false;
  if (b->mixed) std::fill(b->kinds.begin(), b->kinds.end(), (uint8_t)MI_INPUT_RGB);              // back from a mixed layout: the slots moved, their contents are unspecified
  batch_layout_uniform(b);
  return MI_OK;
}

// ---- mixed-size layouts: the run's pictures differ in size and share what the batch reserved for cap pictures of w x h ----
int mi_batch_fits(const mi_batch *b, int n_images, const uint32_t *widths, const uint32_t *heights) { return batch_layout_status(b, n_images, widths, heights); }
int mi_batch_set_sizes(mi_batch *b, int n_images, const uint32_t *widths, const uint32_t *heights) {
  if (b && b->in_flight) return MI_INVALID_ARGUMENT;
  if (const int st = batch_layout_status(b, n_images, widths, heights)) return st;
  b->n = n_images; b->alpha_flags.assign(n_images, 0);
  b->encoded = b->measured = false;
  std::fill(b->kinds.begin(), b->kinds.end(), (uint8_t)MI_INPUT_RGB);
  b->mixed = true; b->run_px = 0;
  b->slot_w.assign(b->cap, 0); b->slot_h.assign(b->cap, 0); b->slot_at.assign(b->cap, 0);
  for (int i = 0; i < n_images; i++) { b->slot_w[i] = widths[i]; b->slot_h[i] = heights[i]; b->slot_at[i] = b->run_px * b->channels; b->run_px += (size_t)widths[i] * heights[i]; }
  return MI_OK;
}
int mi_batch_image_size(const mi_batch *b, int index, uint32_t *w, uint32_t *h) {
  if (!b || !w || !h || index < 0 || index >= batch_slots(b)) return MI_INVALID_ARGUMENT;
  *w = slot_w(b, index); *h = slot_h(b, index);
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
    const size_t npx = b->run_px;
    hipLaunchKernelGGL(premultiply_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s, d_pixels, d_clean, npx);
    HIP_OK(hipGetLastError());
    front_src = d_clean;
  } else if (d_clean) {                                     // convert_alpha_8bit: UnassociatedClean (av1encoder.rs:277-281)
    HIP_OK(hipMemsetAsync(d_alpha_acc, 0, sizeof(unsigned long long) * 4 * b->n, s));
    const dim3 blk(256);
    for (int i = 0; i < b->n; i++) {
      if (b->kinds[i] != MI_INPUT_RGB) continue;                // opaque (YCbCr, or a deep image with A = 65535): the passes would be copies; the front end reads the slot itself
      const int w = (int)slot_w(b, i), h = (int)slot_h(b, i);
      const dim3 g((w + 255) / 256, h);
      const uint8_t *in = d_pixels + slot_at(b, i); uint8_t *outp = d_clean + slot_at(b, i);
      hipLaunchKernelGGL(alpha_scan_kernel, g, blk, 0, s, in, w, h, d_alpha_acc + 4 * i);
      hipLaunchKernelGGL(alpha_rewrite_kernel, g, blk, 0, s, in, d_clean_tmp, w, h, d_alpha_acc + 4 * i, 0);
      hipLaunchKernelGGL(alpha_rewrite_kernel, g, blk, 0, s, (const uint8_t *)d_clean_tmp, outp, w, h, d_alpha_acc + 4 * i, 1);
    }
    HIP_OK(hipGetLastError());
    front_src = d_clean;
  }
  for (int i = 0; i < b->n; i++) {
    FramePlan &p = b->fs.frames[i];
    const int w = (int)slot_w(b, i), h = (int)slot_h(b, i);
    uint16_t *alpha_stage = b->channels == 4 ? p.dev.fin[0] : nullptr;      // fin[0] is free until CDEF runs
    if (b->kinds[i] == MI_INPUT_RGB16 || b->kinds[i] == MI_INPUT_YCBCR16) {   // its deep slot, through the 16-bit front end (kind 3: canonical YCbCr, no matrix)
      const uint16_t *deep = b->d_pixels16.get();
      if (!deep) return MI_INVALID_ARGUMENT;
      deep += slot_at(b, i);
      const FrontDeepParams dp{ b->depth, b->enc.color_model, b->kinds[i] == MI_INPUT_YCBCR16 };
      if (b->channels == 4) hipLaunchKernelGGL((frontend_deep_kernel<4>), dim3((p.pw + 255) / 256, p.ph), dim3(256), 0, s, deep, w, h, dp,
                                               p.dev.src[0], p.dev.src[1], p.dev.src[2], alpha_stage, p.pw, p.ph, d_alpha_flags + i);
      else hipLaunchKernelGGL((frontend_deep_kernel<3>), dim3((p.pw + 255) / 256, p.ph), dim3(256), 0, s, deep, w, h, dp,
                              p.dev.src[0], p.dev.src[1], p.dev.src[2], alpha_stage, p.pw, p.ph, d_alpha_flags + i);
      continue;
    }
    fp.ycc = b->kinds[i] == MI_INPUT_YCBCR;
    hipLaunchKernelGGL(frontend_kernel, dim3((p.pw + 255) / 256, p.ph), dim3(256), 0, s,
                       (fp.ycc ? d_pixels : front_src) + slot_at(b, i), w, h, w, fp,
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
                                 slot_w(b, i), slot_h(b, i), b->depth, col.cfg.matrix, b->enc.alpha_mode == 2, b->enc.exif, b->enc.exif_len);
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
  const size_t w = slot_w(b, index), h = slot_h(b, index);
  for (int i = 0; i < p->np; i++) {
    planes[i] = (uint16_t *)malloc(w * h * 2);
    HIP_OK(hipMemcpy2D(planes[i], w * 2, p->cfg.lrf ? p->dev.lrp[i] : p->dev.fin[i], (size_t)p->pw * 2, w * 2, h, hipMemcpyDeviceToHost));
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
  const size_t w = slot_w(b, index), h = slot_h(b, index);
  for (int i = 0; i < p->np; i++) {
    planes[i] = (uint16_t *)malloc(w * h * 2);
    HIP_OK(hipMemcpy2D(planes[i], w * 2, p->dev.src[i], (size_t)p->pw * 2, w * 2, h, hipMemcpyDeviceToHost));
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
  out->width = slot_w(b, index); out->height = slot_h(b, index); out->depth = (uint8_t)b->depth; out->color_planes = (uint8_t)b->fs.frames[index].np;
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
  (void)mi_batch_set_count(b, b->cap);                          // every image, the uniform layout
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

}  // extern "C"

#include "host_input.h"

extern "C" {

void mi_release_cached(void) {
  std::vector<std::pair<PoolKey, mi_batch *>> all;
  { std::lock_guard<std::mutex> lk(g_pool_mu); all.swap(g_pool); }
  for (auto &x : all) mi_batch_destroy(x.second);
  jpeg_ctx_release_cached();
}
size_t mi_batch_footprint(const mi_batch *b) { return b ? batch_footprint(b) : 0; }

// ---- the one-call entry points: a pooled batch of one image of w x h, filled by `fill`, encoded, its file handed out ----
static const auto encode_pooled = [](const mi_ravif_encoder *e, uint32_t w, uint32_t h, int channels, mi_encoded_image *out, auto fill) -> int {
  if (!e || !out || w < 1 || h < 1) return MI_INVALID_ARGUMENT;
  mi_batch *b = pool_acquire(e, 1, w, h, channels);
  if (!b) return mi_device_count() > e->device ? MI_INVALID_ARGUMENT : MI_NO_DEVICE;
  int st = fill(b);
  if (st == MI_OK) st = mi_batch_encode(b);
  if (st == MI_OK) st = mi_batch_get(b, 0, out);
  pool_release(b);
  return st;
};
static int encode_one(const mi_ravif_encoder *e, const uint8_t *px, int channels, uint32_t w, uint32_t h, size_t stride_px, mi_encoded_image *out) {
  if (!px) return MI_INVALID_ARGUMENT;
  return encode_pooled(e, w, h, channels, out, [&](mi_batch *b) { return mi_batch_upload(b, 0, px, stride_px); });
}
int mi_ravif_encode_rgba(const mi_ravif_encoder *e, const uint8_t *rgba, uint32_t w, uint32_t h, size_t stride_px, mi_encoded_image *out) { return encode_one(e, rgba, 4, w, h, stride_px, out); }
int mi_ravif_encode_rgb(const mi_ravif_encoder *e, const uint8_t *rgb, uint32_t w, uint32_t h, size_t stride_px, mi_encoded_image *out) { return encode_one(e, rgb, 3, w, h, stride_px, out); }
// ravif::Encoder::encode_rgba / encode_rgb for a picture in the memory of device e->device (channels 4 / 3 as src->channels says)
int mi_ravif_encode_device(const mi_ravif_encoder *e, const mi_device_pixels *src, uint32_t w, uint32_t h, mi_encoded_image *out) {
  if (!src || !src->dev || (src->channels != 3 && src->channels != 4)) return MI_INVALID_ARGUMENT;
  return encode_pooled(e, w, h, src->channels, out, [&](mi_batch *b) { return mi_batch_upload_device(b, 0, 1, src); });
}
// the same for a uint16 picture in the memory of device e->device (mi_batch_upload_device16)
int mi_ravif_encode_device16(const mi_ravif_encoder *e, const mi_device_pixels16 *src, uint32_t w, uint32_t h, mi_encoded_image *out) {
  if (!src || !src->dev || (src->channels != 3 && src->channels != 4)) return MI_INVALID_ARGUMENT;
  return encode_pooled(e, w, h, src->channels, out, [&](mi_batch *b) { return mi_batch_upload_device16(b, 0, 1, src); });
}
// the same for a binary16 or binary32 picture in the memory of device e->device (mi_batch_upload_device_float)
int mi_ravif_encode_device_float(const mi_ravif_encoder *e, const mi_device_pixels_float *src, uint32_t w, uint32_t h, mi_encoded_image *out) {
  if (!src || !src->dev || (src->channels != 3 && src->channels != 4)) return MI_INVALID_ARGUMENT;
  return encode_pooled(e, w, h, src->channels, out, [&](mi_batch *b) { return mi_batch_upload_device_float(b, 0, 1, src); });
}
// the same for YCbCr planes in the memory of device e->device: the file of a 3-channel batch fed through mi_batch_upload_device_ycbcr
int mi_ravif_encode_device_ycbcr(const mi_ravif_encoder *e, const mi_device_planes *src, uint32_t w, uint32_t h, mi_encoded_image *out) {
  if (!src || !src->y || !src->cb) return MI_INVALID_ARGUMENT;
  return encode_pooled(e, w, h, 3, out, [&](mi_batch *b) { return mi_batch_upload_device_ycbcr(b, 0, 1, src); });
}
// the same for uint16 planes (P010 / P016, planar 10- to 16-bit): mi_batch_upload_device_ycbcr16
int mi_ravif_encode_device_ycbcr16(const mi_ravif_encoder *e, const mi_device_planes16 *src, uint32_t w, uint32_t h, mi_encoded_image *out) {
  if (!src || !src->y || !src->cb) return MI_INVALID_ARGUMENT;
  return encode_pooled(e, w, h, 3, out, [&](mi_batch *b) { return mi_batch_upload_device_ycbcr16(b, 0, 1, src); });
}
// the same for a picture of src_w x src_h that is resampled to w x h on the way in
int mi_ravif_encode_device_resized(const mi_ravif_encoder *e, const mi_device_pixels *src, uint32_t src_w, uint32_t src_h, uint32_t w, uint32_t h, int filter, mi_encoded_image *out) {
  if (!src || !src->dev || (src->channels != 3 && src->channels != 4)) return MI_INVALID_ARGUMENT;
  return encode_pooled(e, w, h, src->channels, out, [&](mi_batch *b) { return mi_batch_resize_device(b, 0, 1, src, src_w, src_h, filter); });
}
// the same for a uint16 picture: resampled at 16 bits into the deep slot (mi_batch_resize_device16)
int mi_ravif_encode_device16_resized(const mi_ravif_encoder *e, const mi_device_pixels16 *src, uint32_t src_w, uint32_t src_h, uint32_t w, uint32_t h, int filter, mi_encoded_image *out) {
  if (!src || !src->dev || (src->channels != 3 && src->channels != 4)) return MI_INVALID_ARGUMENT;
  return encode_pooled(e, w, h, src->channels, out, [&](mi_batch *b) { return mi_batch_resize_device16(b, 0, 1, src, src_w, src_h, filter); });
}

}  // extern "C"

#include "host_stream.h"

extern "C" {

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
