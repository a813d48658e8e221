// host_input.h -- the input half of mi_avif.hip, the one translation unit every build names: the rules every slot-filling call shares and the calls through
// which pixels reach a batch slot or leave it -- host pixels, pictures and planes in device memory, JPEG coefficients, PNG scanlines, 16-bit sources, resize
// on input, colour management, orientation, decoded output.  Included there below struct mi_batch, the batch's lifecycle, its encode and its pool, so that the kernels keep the order of their
// first launch site and the code object stays the one the sources gave before the split; the one-call entry points, the stream worker and the plane encoder follow it.
#pragma once

static void batch_tag(mi_batch *b, int first, int count, int kind) { std::fill(b->kinds.begin() + first, b->kinds.begin() + first + count, (uint8_t)kind); }
// The rules of the input kinds, each over (settings, channels of the batch) and over a batch: the stream worker asks the first form before a batch exists.
// MI_INPUT_YCBCR needs the YCbCr colour model (the planes are the slot's bytes) and, in a 4-channel batch, an alpha mode that leaves opaque pixels alone
static bool batch_takes_ycbcr(const mi_ravif_encoder &e, int channels) { return e.color_model != 1 && !(channels == 4 && e.alpha_mode == 2); }
static bool batch_takes_ycbcr(const mi_batch *b) { return batch_takes_ycbcr(b->enc, b->channels); }
// MI_INPUT_RGB16: the dirty-alpha cleaner and the premultiply branch are defined on 8-bit samples, so a 4-channel batch takes a deep source with an alpha channel
// under UnassociatedDirty alone and an opaque one (A = 65535: the cleaner skips it as it skips MI_INPUT_YCBCR) under both unassociated modes; a 3-channel batch takes 3 channels
static bool batch_takes_deep(const mi_ravif_encoder &e, int channels, int src_channels) {
  if (src_channels != 3 && src_channels != 4) return false;
  if (channels == 3) return src_channels == 3;
  return src_channels == 4 ? e.alpha_mode == 0 : e.alpha_mode != 2;
}
static bool batch_takes_deep(const mi_batch *b, int src_channels) { return batch_takes_deep(b->enc, b->channels, src_channels); }
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

// the buffer holds at least `need` bytes afterwards (whoever calls has made sure that nothing on the device still uses the buffer that is replaced)
static const auto staging_grow = [](auto &buf /* DevBuf or PinBuf */, size_t &cap, size_t need) {
  if (need <= cap) return true;
  need = (need + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
  cap = 0;
  if (buf.alloc(need) != hipSuccess) return false;
  cap = need; return true;
};

// ---- the rules the slot-filling calls share ----
// images [first, first + count) are slots of the batch, and the one-index form (what a call that may run beside an encode in flight asks); the same of a batch
// with no encode in flight (what every call that fills slots on the stream asks), and its one-index form; the same against the images of a completed encode
static bool batch_has_slots(const mi_batch *b, int first, int count) { return b && first >= 0 && count >= 1 && first <= batch_slots(b) - count; }
static bool batch_has_slot(const mi_batch *b, int index) { return batch_has_slots(b, index, 1); }
static bool batch_range_ok(const mi_batch *b, int first, int count) { return batch_has_slots(b, first, count) && !b->in_flight; }
static bool batch_index_ok(const mi_batch *b, int index) { return batch_range_ok(b, index, 1); }
static bool batch_encoded_ok(const mi_batch *b, int first, int count) { return b && !b->in_flight && b->encoded && first >= 0 && count >= 1 && first <= b->n - count; }

// the same for the calls that take a range and describe its pictures with one size: every slot of the range has it (w x h on return)
static bool batch_range_sized(const mi_batch *b, int first, int count, uint32_t &w, uint32_t &h) {
  if (!batch_range_ok(b, first, count) || !slots_one_size(b, first, count)) return false;
  w = slot_w(b, first); h = slot_h(b, first);
  return true;
}
// the bytes of slots [first, first + count): they lie back to back
static size_t batch_range_samples(const mi_batch *b, int first, int count) { return slot_at(b, first + count - 1) + slot_samples(b, first + count - 1) - slot_at(b, first); }

// fn(from, to) for every maximal stretch [from, to) of neighbours in [0, n) whose key(k) is equal, in index order; the first status that is not MI_OK ends the walk and is returned
template <class Key, class Fn> static int for_each_group(size_t n, Key key, Fn fn) {
  for (size_t k = 0, k1; k < n; k = k1) {
    for (k1 = k + 1; k1 < n && key(k1) == key(k);) k1++;
    if (const int rc = fn(k, k1)) return rc;
  }
  return MI_OK;
}

// the batch's stream waits for whatever `after_stream` (a producer's or a consumer's hipStream_t, or null) holds at this moment; the event is made on first use
static int batch_join(mi_batch *b, void *after_stream) {
  if (!after_stream) return MI_OK;
  if (!b->ev_src) HIP_OK(hipEventCreateWithFlags(&b->ev_src, hipEventDisableTiming));
  HIP_OK(hipEventRecord(b->ev_src, (hipStream_t)after_stream));
  HIP_OK(hipStreamWaitEvent(b->stream, b->ev_src, 0));
  return MI_OK;
}

// the grid of the kernels that work in row groups (dev_slot.h: one thread per four pixels of a row, workgroups of 64), a grid row per picture row and a grid
// plane per image
static dim3 grid_by_four(uint32_t w, uint32_t h, int count) { return dim3(((w + 3) / 4 + 63) / 64, h, (unsigned)count); }
// such a kernel template, `kernel`<3> or <4> by `channels`, on a stream / on the batch's stream.  A macro because a template of kernels has no name to pass:
// `stream` and `channels` are evaluated twice, the kernel's arguments once per branch -- pass plain variables
#define LAUNCH_BY_CHANNELS_ON(stream, channels, w, h, count, kernel, ...) do { \
    if ((channels) == 4) hipLaunchKernelGGL((kernel<4>), grid_by_four(w, h, count), dim3(64), 0, stream, __VA_ARGS__); \
    else hipLaunchKernelGGL((kernel<3>), grid_by_four(w, h, count), dim3(64), 0, stream, __VA_ARGS__); \
  } while (0)
#define LAUNCH_BY_CHANNELS(b, channels, w, h, count, kernel, ...) LAUNCH_BY_CHANNELS_ON((b)->stream, channels, w, h, count, kernel, __VA_ARGS__)

// Strided pictures in device memory (mi_device_pixels, mi_device_pixels16, mi_device_target -> IngestSrc, Ingest16Src, DecodedDst): pointer, layout, channels
// and the three byte strides of `src` for pictures of w x h samples of `sample_bytes` go into `d`.  A stride of 0 means packed -- HWC: pixels back to back, rows
// back to back; CHW: rows back to back, planes back to back -- and images back to back.  false = refused: a row shorter than its packed samples, pixels closer
// than their channels or planes closer than a row, and for a target that is written (`writable`) interleaved rows that would reach into the next one.
template <class Desc, class Dev> static bool strided_resolve(const Desc &src, uint32_t w, uint32_t h, size_t sample_bytes, bool writable, Dev &d) {
  const bool hwc = src.layout == 0;
  const size_t pixel = (size_t)src.channels * sample_bytes, packed_row = (size_t)w * (hwc ? pixel : sample_bytes);
  d.base = (decltype(d.base))src.dev; d.layout = src.layout; d.channels = src.channels;
  d.row_stride = src.row_stride ? src.row_stride : packed_row;
  d.inner_stride = src.pixel_or_plane_stride ? src.pixel_or_plane_stride : hwc ? pixel : d.row_stride * h;
  d.image_stride = src.image_stride ? src.image_stride : hwc ? d.row_stride * h : d.inner_stride * src.channels;
  if (d.row_stride < packed_row || d.inner_stride < (hwc ? pixel : (size_t)w * sample_bytes)) return false;
  return !(writable && hwc && d.row_stride < (size_t)(w - 1) * d.inner_stride + pixel);       // a written row must end before the next one starts
}

// the slot of image `index` in device memory: uint8_t the 8-bit slots, uint16_t the deep ones (made by the first call: nullptr = could not be allocated)
template <class T> static T *batch_slot(mi_batch *b, int index) {
  if (!batch_has_slot(b, index)) return nullptr;
  const size_t at = slot_at(b, index);
  if constexpr (sizeof(T) == 1) return b->d_pixels.get() + at;
  else { uint16_t *const deep = batch_deep(b); return deep ? deep + at : nullptr; }
}
// its samples into host memory, after everything the batch's stream holds
template <class T> static int batch_read_slot(mi_batch *b, int index, T *dst) {
  if (!batch_has_slot(b, index) || !dst) return MI_INVALID_ARGUMENT;
  const T *const src = batch_slot<T>(b, index);
  if (!src) return MI_ENCODING_ERROR;                         // the deep slots could not be made (the 8-bit ones exist since mi_batch_create)
  (void)hipSetDevice(b->device);
  HIP_OK(hipStreamSynchronize(b->stream));
  HIP_OK(hipMemcpy(dst, src, slot_samples(b, index) * sizeof(T), hipMemcpyDeviceToHost));
  return MI_OK;
}

extern "C" {

// The batch owns a pinned host staging area laid out like its HBM input slot; H2D always starts from there.
uint8_t *mi_batch_input(mi_batch *b, int index) {
  if (!batch_has_slot(b, index)) return nullptr;
  {                                                           // made once, by whichever thread asks first (callers may fill different slots from different threads)
    std::lock_guard<std::mutex> lk(b->staging_mu);
    if (!b->h_pixels.get()) { (void)hipSetDevice(b->device); if (b->h_pixels.alloc(b->pixel_bytes) != hipSuccess) return nullptr; }
  }
  return b->h_pixels.get() + slot_at(b, index);
}
// enqueue the H2D of images [first, first + count) from the pinned staging on the batch's stream; returns at once
int mi_batch_upload_async(mi_batch *b, int first, int count) {
  if (!batch_has_slots(b, first, count) || !mi_batch_input(b, first)) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  HIP_OK(hipMemcpyAsync(b->d_pixels.get() + slot_at(b, first), b->h_pixels.get() + slot_at(b, first), batch_range_samples(b, first, count), hipMemcpyHostToDevice, b->stream));
  batch_tag(b, first, count, MI_INPUT_RGB);
  return MI_OK;
}
int mi_batch_set_input_kind(mi_batch *b, int first, int count, int kind) {
  if (!batch_range_ok(b, first, count) || kind < MI_INPUT_RGB || kind > MI_INPUT_YCBCR16) return MI_INVALID_ARGUMENT;
  if ((kind == MI_INPUT_YCBCR || kind == MI_INPUT_YCBCR16) && !batch_takes_ycbcr(b)) return MI_INVALID_ARGUMENT;
  // kinds 2 and 3 tag what a HIP caller wrote through mi_batch_device_input16, the call that makes the deep slots: a batch without them has nothing to tag (and
  // the set call allocates nothing); a slot of kind 2 may hold any alpha, one of kind 3 is opaque whatever its fourth sample holds
  if (kind == MI_INPUT_RGB16 || kind == MI_INPUT_YCBCR16) {
    if (kind == MI_INPUT_RGB16 && !batch_takes_deep(b, b->channels)) return MI_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lk(b->staging_mu);
    if (!b->d_pixels16.get()) return MI_INVALID_ARGUMENT;
  }
  batch_tag(b, first, count, kind);
  return MI_OK;
}
int mi_batch_input_kind(mi_batch *b, int index, int *kind) {
  if (!batch_has_slot(b, index) || !kind) return MI_INVALID_ARGUMENT;
  *kind = b->kinds[index];
  return MI_OK;
}
int mi_batch_upload(mi_batch *b, int index, const uint8_t *pixels, size_t stride_px) {
  if (!batch_has_slot(b, index) || !pixels) return MI_INVALID_ARGUMENT;
  const size_t row = (size_t)slot_w(b, index) * b->channels;
  uint8_t *dst = mi_batch_input(b, index);
  if (!dst) return MI_ENCODING_ERROR;
  for (uint32_t y = 0; y < slot_h(b, index); y++) memcpy(dst + y * row, pixels + (size_t)y * stride_px * b->channels, row);
  if (int st = mi_batch_upload_async(b, index, 1)) return st;
  HIP_OK(hipStreamSynchronize(b->stream));
  return MI_OK;
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
// the idle contexts go (mi_release_cached)
static void jpeg_ctx_release_cached() {
  std::vector<JpegCtx *> ctxs;
  { std::lock_guard<std::mutex> lk(g_jpeg_mu); ctxs.swap(g_jpeg_free); for (JpegCtx *c : ctxs) g_jpeg_live[c->device]--; }
  g_jpeg_cv.notify_all();
  for (JpegCtx *c : ctxs) jpeg_ctx_destroy(c);
}

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
  if (ycc) LAUNCH_BY_CHANNELS_ON(stream, channels, jc.w, jc.h, 1, jpeg_ycc_kernel, (const uint8_t *)d_planes, g, d_out, stride_px);
  else LAUNCH_BY_CHANNELS_ON(stream, channels, jc.w, jc.h, 1, jpeg_colour_kernel, (const uint8_t *)d_planes, g, d_out, stride_px);
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

uint8_t *mi_batch_device_input(mi_batch *b, int index) { return batch_slot<uint8_t>(b, index); }
int mi_batch_read_input(mi_batch *b, int index, uint8_t *dst) { return batch_read_slot(b, index, dst); }

// images [first, first + count) from pictures in the memory of the batch's device: one ingest_kernel launch on the batch's stream, after whatever
// src->after_stream holds at this moment.  Strides of 0 mean packed; a row must not be shorter than its packed pixels (torch views -- crops, permuted
// tensors, padded rows -- all satisfy that).
// (what it and mi_batch_resize_device ask of a source of w x h and make of it; false = refused)
static bool batch_device_source(const mi_batch *b, const mi_device_pixels *src, uint32_t w, uint32_t h, IngestSrc &s) {
  if (!src || !src->dev || (src->layout != 0 && src->layout != 1) || (src->channels != 3 && src->channels != 4) || src->channels > b->channels) return false;   // alpha is never dropped
  s.w = w; s.h = h;
  return strided_resolve(*src, w, h, 1, false, s);
}
int mi_batch_upload_device(mi_batch *b, int first, int count, const mi_device_pixels *src) {
  IngestSrc s; uint32_t w, h;
  if (!batch_range_sized(b, first, count, w, h) || !batch_device_source(b, src, w, h, s)) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  if (int st = batch_join(b, src->after_stream)) return st;
  uint8_t *const slots = mi_batch_device_input(b, first);
  LAUNCH_BY_CHANNELS(b, b->channels, w, h, count, ingest_kernel, s, slots);
  HIP_OK(hipGetLastError());
  batch_tag(b, first, count, MI_INPUT_RGB);
  return MI_OK;
}
// images [first, first + count) from 8-bit YCbCr planes in the memory of the batch's device: one planes_ingest_kernel launch on the batch's stream, after
// whatever src->after_stream holds at this moment; the slots are tagged MI_INPUT_YCBCR.  Strides of 0 mean packed.
int mi_batch_upload_device_ycbcr(mi_batch *b, int first, int count, const mi_device_planes *src) {
  uint32_t w, h;
  if (!batch_range_sized(b, first, count, w, h) || !src || !src->y || !src->cb || !batch_takes_ycbcr(b)) return MI_INVALID_ARGUMENT;
  if (!((src->hsub == 1 && src->vsub == 1) || (src->hsub == 2 && (src->vsub == 1 || src->vsub == 2)))) return MI_INVALID_ARGUMENT;
  PlanesSrc s;
  s.w = w; s.h = h; s.hsub = (uint32_t)src->hsub; s.vsub = (uint32_t)src->vsub;
  s.cw = (w + s.hsub - 1) / s.hsub; s.ch = (h + s.vsub - 1) / s.vsub;
  s.cpitch = src->cr ? 1 : 2;
  s.y = (const uint8_t *)src->y; s.cb = (const uint8_t *)src->cb; s.cr = src->cr ? (const uint8_t *)src->cr : s.cb + 1;
  const size_t packed_c = (size_t)s.cw * s.cpitch;
  s.y_row = src->y_row_stride ? src->y_row_stride : w; s.c_row = src->c_row_stride ? src->c_row_stride : packed_c;
  s.y_image = src->y_image_stride ? src->y_image_stride : s.y_row * h; s.c_image = src->c_image_stride ? src->c_image_stride : s.c_row * s.ch;
  if (s.y_row < w || s.c_row < packed_c) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  if (int st = batch_join(b, src->after_stream)) return st;
  uint8_t *const slots = mi_batch_device_input(b, first);
  LAUNCH_BY_CHANNELS(b, b->channels, w, h, count, planes_ingest_kernel, s, slots);
  HIP_OK(hipGetLastError());
  batch_tag(b, first, count, MI_INPUT_YCBCR);
  return MI_OK;
}

// ---- deep input: 16-bit sources into the deep slots (dev_deep.h) ----
uint16_t *mi_batch_device_input16(mi_batch *b, int index) { return batch_slot<uint16_t>(b, index); }
int mi_batch_read_input16(mi_batch *b, int index, uint16_t *dst) { return batch_read_slot(b, index, dst); }

// (what mi_batch_upload_device16 and mi_batch_resize_device16 ask of a uint16 source of w x h and make of it; false = refused)
static bool batch_device_source16(const mi_batch *b, const mi_device_pixels16 *src, uint32_t w, uint32_t h, Ingest16Src &s) {
  if (!src || !src->dev) return false;
  if ((src->layout != 0 && src->layout != 1) || !batch_takes_deep(b, src->channels)) return false;   // alpha is never dropped; the alpha rules of the kind
  if (src->bits < 8 || src->bits > 16 || (src->msb_aligned != 0 && src->msb_aligned != 1)) return false;
  if (((uintptr_t)src->dev | src->row_stride | src->pixel_or_plane_stride | src->image_stride) & 1) return false;   // uint16 samples
  s.w = w; s.h = h; s.bits = src->bits; s.msb_aligned = src->msb_aligned;
  return strided_resolve(*src, w, h, 2, false, s);
}
// images [first, first + count) from uint16 pictures in the memory of the batch's device: one ingest16_kernel launch on the batch's stream, after whatever
// src->after_stream holds at this moment; the slots are tagged MI_INPUT_RGB16.  Every check comes before the deep slots are made: a refused call allocates nothing.
int mi_batch_upload_device16(mi_batch *b, int first, int count, const mi_device_pixels16 *src) {
  uint32_t w, h;
  Ingest16Src s;
  if (!batch_range_sized(b, first, count, w, h) || !batch_device_source16(b, src, w, h, s)) return MI_INVALID_ARGUMENT;
  uint16_t *const slots = mi_batch_device_input16(b, first);
  if (!slots) return MI_ENCODING_ERROR;
  (void)hipSetDevice(b->device);
  if (int st = batch_join(b, src->after_stream)) return st;
  LAUNCH_BY_CHANNELS(b, b->channels, w, h, count, ingest16_kernel, s, slots);
  HIP_OK(hipGetLastError());
  batch_tag(b, first, count, MI_INPUT_RGB16);
  return MI_OK;
}
// one image of full-scale uint16 host pixels into the deep slot of `index`: a 2-D copy on the batch's stream (3 channels into a 4-channel batch: through a host
// copy that carries A = 65535), then the stream is waited for.  No pinned staging of its own.
int mi_batch_upload16(mi_batch *b, int index, const uint16_t *pixels, size_t stride_px, int channels) {
  if (!batch_index_ok(b, index) || !pixels || !batch_takes_deep(b, channels)) return MI_INVALID_ARGUMENT;
  const uint32_t w = slot_w(b, index), h = slot_h(b, index);
  if (stride_px == 0) stride_px = w;
  if (stride_px < w) return MI_INVALID_ARGUMENT;
  uint16_t *const slot = mi_batch_device_input16(b, index);
  if (!slot) return MI_ENCODING_ERROR;
  (void)hipSetDevice(b->device);
  const size_t row = (size_t)w * b->channels * sizeof(uint16_t);
  try {                                                       // nothing may unwind through the C ABI
    std::vector<uint16_t> wide;
    if (channels != b->channels) {
      wide.resize((size_t)w * h * 4);
      for (uint32_t y = 0; y < h; y++) for (uint32_t x = 0; x < w; x++) {
        const uint16_t *q = pixels + ((size_t)y * stride_px + x) * 3; uint16_t *o = wide.data() + ((size_t)y * w + x) * 4;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = 65535;
      }
      HIP_OK(hipMemcpyAsync(slot, wide.data(), row * h, hipMemcpyHostToDevice, b->stream));
    } else HIP_OK(hipMemcpy2DAsync(slot, row, pixels, stride_px * channels * sizeof(uint16_t), row, h, hipMemcpyHostToDevice, b->stream));
    HIP_OK(hipStreamSynchronize(b->stream));
  } catch (const std::exception &) { return MI_ENCODING_ERROR; }
  batch_tag(b, index, 1, MI_INPUT_RGB16);
  return MI_OK;
}

// ---- float sources (dev_float.h) ----
static size_t sample_bytes_of(int sample) { return sample == MI_SAMPLE_F32 ? 4 : 2; }
static bool full_scale_ok(float full_scale) { return std::isfinite(full_scale) && full_scale > 0.0f; }
// images [first, first + count) from binary16 or binary32 pictures in the memory of the batch's device: one ingest_float_kernel launch on the batch's stream,
// after whatever src->after_stream holds at this moment; the slots are tagged MI_INPUT_RGB16.  mi_batch_upload_device16's rules (the alpha rules of deep input
// among them), the strides counted in the sample's size.  Every check comes before the deep slots are made: a refused call allocates nothing.
int mi_batch_upload_device_float(mi_batch *b, int first, int count, const mi_device_pixels_float *src) {
  uint32_t w, h;
  IngestFloatSrc s;
  if (!batch_range_sized(b, first, count, w, h) || !src || !src->dev) return MI_INVALID_ARGUMENT;
  if ((src->layout != 0 && src->layout != 1) || !batch_takes_deep(b, src->channels)) return MI_INVALID_ARGUMENT;   // alpha is never dropped; the alpha rules of the kind
  if ((src->sample != MI_SAMPLE_F16 && src->sample != MI_SAMPLE_F32) || !full_scale_ok(src->full_scale)) return MI_INVALID_ARGUMENT;
  const size_t sb = sample_bytes_of(src->sample);
  if (((uintptr_t)src->dev | src->row_stride | src->pixel_or_plane_stride | src->image_stride) & (sb - 1)) return MI_INVALID_ARGUMENT;   // whole samples
  s.w = w; s.h = h; s.sample = src->sample; s.full_scale = src->full_scale;
  if (!strided_resolve(*src, w, h, sb, false, s)) return MI_INVALID_ARGUMENT;
  uint16_t *const slots = mi_batch_device_input16(b, first);
  if (!slots) return MI_ENCODING_ERROR;
  (void)hipSetDevice(b->device);
  if (int st = batch_join(b, src->after_stream)) return st;
  LAUNCH_BY_CHANNELS(b, b->channels, w, h, count, ingest_float_kernel, s, slots);
  HIP_OK(hipGetLastError());
  batch_tag(b, first, count, MI_INPUT_RGB16);
  return MI_OK;
}

// ---- deep YCbCr planes (dev_planes.h) ----
// the multiply-high form of one sample map of include/mi_avif.h for planes_ingest16_kernel: W = clamp(floor((65535 v + bias) / d), 0, 65535), where
// full range has d = P = 2^bits - 1 and the rounding term (P - 1) / 2, narrow range d = 219 s (luma) | 224 s (chroma), s = 2^(bits - 8), and the rounding term
// floor(d / 2); the dividend starts at -65535 * (0 | 2^(bits-1) | 16 s | 128 s) and chroma adds the centre, 32768 d.  |bias| stays below 2^29.
static SampleMap16 make_sample_map16(int bits, bool chroma, bool narrow) {
  const long long M = 65535, P = (1ll << bits) - 1, s = 1ll << (bits - 8);
  const long long d = narrow ? (chroma ? 224 : 219) * s : P;
  const long long zero = narrow ? (chroma ? 128 : 16) * s : chroma ? 1ll << (bits - 1) : 0;
  const long long bias = -M * zero + (narrow ? d / 2 : (P - 1) / 2) + (chroma ? 32768 * d : 0);
  uint32_t shift = 0;
  while ((2ll << shift) <= d) shift++;                          // floor(log2 d); d is no power of two, so the magic number fits 32 bits
  return SampleMap16{ (uint32_t)(((1ull << (32 + shift)) / (unsigned long long)d) + 1), (int32_t)bias, shift };
}
// images [first, first + count) from uint16 YCbCr planes in the memory of the batch's device: one planes_ingest16_kernel launch on the batch's stream, after
// whatever src->after_stream holds at this moment; the slots are tagged MI_INPUT_YCBCR16.  Strides of 0 mean packed.  Every check comes before the deep slots
// are made: a refused call allocates nothing.
int mi_batch_upload_device_ycbcr16(mi_batch *b, int first, int count, const mi_device_planes16 *src) {
  uint32_t w, h;
  if (!batch_range_sized(b, first, count, w, h) || !src || !src->y || !src->cb || !batch_takes_ycbcr(b)) return MI_INVALID_ARGUMENT;
  if (!((src->hsub == 1 && src->vsub == 1) || (src->hsub == 2 && (src->vsub == 1 || src->vsub == 2)))) return MI_INVALID_ARGUMENT;
  if (src->bits < 8 || src->bits > 16 || (src->msb_aligned != 0 && src->msb_aligned != 1) || (src->narrow_range != 0 && src->narrow_range != 1)) return MI_INVALID_ARGUMENT;
  if (((uintptr_t)src->y | (uintptr_t)src->cb | (uintptr_t)src->cr | src->y_row_stride | src->c_row_stride | src->y_image_stride | src->c_image_stride) & 1) return MI_INVALID_ARGUMENT;   // uint16 samples
  Planes16Src s;
  s.w = w; s.h = h; s.hsub = (uint32_t)src->hsub; s.vsub = (uint32_t)src->vsub;
  s.cw = (w + s.hsub - 1) / s.hsub; s.ch = (h + s.vsub - 1) / s.vsub;
  s.pairs = src->cr ? 0 : 1;
  s.y = (const uint8_t *)src->y; s.cb = (const uint8_t *)src->cb; s.cr = src->cr ? (const uint8_t *)src->cr : s.cb;
  const size_t packed_y = (size_t)w * 2, packed_c = (size_t)s.cw * (s.pairs ? 4 : 2);
  s.y_row = src->y_row_stride ? src->y_row_stride : packed_y; s.c_row = src->c_row_stride ? src->c_row_stride : packed_c;
  s.y_image = src->y_image_stride ? src->y_image_stride : s.y_row * h; s.c_image = src->c_image_stride ? src->c_image_stride : s.c_row * s.ch;
  if (s.y_row < packed_y || s.c_row < packed_c) return MI_INVALID_ARGUMENT;
  s.down = src->msb_aligned ? (uint32_t)(16 - src->bits) : 0u; s.mask = (1u << src->bits) - 1u;
  s.ym = make_sample_map16(src->bits, false, src->narrow_range != 0); s.cm = make_sample_map16(src->bits, true, src->narrow_range != 0);
  uint16_t *const slots = mi_batch_device_input16(b, first);
  if (!slots) return MI_ENCODING_ERROR;
  (void)hipSetDevice(b->device);
  if (int st = batch_join(b, src->after_stream)) return st;
  LAUNCH_BY_CHANNELS(b, b->channels, w, h, count, planes_ingest16_kernel, s, slots);
  HIP_OK(hipGetLastError());
  batch_tag(b, first, count, MI_INPUT_YCBCR16);
  return MI_OK;
}

// ---- decoded pixels of the last completed encode (dev_decoded.h) ----
int mi_batch_uses_alpha(mi_batch *b, int index, int *uses_alpha) {
  if (!batch_encoded_ok(b, index, 1) || !uses_alpha) return MI_INVALID_ARGUMENT;
  *uses_alpha = (b->channels == 4 && b->alpha_flags[index]) ? 1 : 0;
  return MI_OK;
}
// One decoded_kernel launch over the frame descriptors the encode staged (still on the device, like the planes: nothing after mi_batch_wait writes them until
// the next encode), after whatever dst->after_stream holds at this moment, then the batch's stream is waited for.  Strides of 0 mean packed.
int mi_batch_decode_device(mi_batch *b, int first, int count, int which, const mi_device_target *dst) {
  if (!batch_encoded_ok(b, first, count) || !slots_one_size(b, first, count) || !dst || !dst->dev) return MI_INVALID_ARGUMENT;
  const uint32_t w = slot_w(b, first), h = slot_h(b, first);
  if ((which != MI_DECODED_RECON && which != MI_DECODED_SOURCE) || (dst->layout != 0 && dst->layout != 1) || (dst->channels != 3 && dst->channels != 4)) return MI_INVALID_ARGUMENT;
  if ((size_t)b->n * (b->channels == 4 ? 2 : 1) != b->fs.frames.size()) return MI_INVALID_ARGUMENT;
  if (dst->channels == 3 && b->channels == 4)
    for (int i = first; i < first + count; i++) if (b->alpha_flags[i]) return MI_INVALID_ARGUMENT;      // alpha is never dropped
  DecodedDst d;
  d.first = first; d.n = b->n; d.alpha_frames = b->channels == 4; d.source = which == MI_DECODED_SOURCE;
  if (!strided_resolve(*dst, w, h, 1, true, d)) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  if (int st = batch_join(b, dst->after_stream)) return st;
  const dim3 grid = grid_by_four(w, h, count);
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
  if (!batch_encoded_ok(b, index, 1) || !dst || (channels != 3 && channels != 4)) return MI_INVALID_ARGUMENT;
  if ((which != MI_DECODED_RECON && which != MI_DECODED_SOURCE) || (channels == 3 && b->channels == 4 && b->alpha_flags[index])) return MI_INVALID_ARGUMENT;   // before the scratch exists: a refused call allocates nothing
  (void)hipSetDevice(b->device);
  if (!staging_grow(b->d_decoded, b->d_decoded_cap, slot_px(b, index) * 4)) return MI_ENCODING_ERROR;     // (one image: follows the largest picture asked for)
  mi_device_target t;
  memset(&t, 0, sizeof(t));
  t.dev = b->d_decoded.get(); t.layout = 0; t.channels = channels;
  if (const int st = mi_batch_decode_device(b, index, 1, which, &t)) return st;
  HIP_OK(hipMemcpy(dst, b->d_decoded.get(), slot_px(b, index) * channels, hipMemcpyDeviceToHost));
  return MI_OK;
}

// ---- full-depth decoded pixels (dev_decoded16.h) ----
// mi_batch_decode_device with uint16, binary16 or binary32 samples: its state rule, one-size rule, alpha rule and stride rules, the packed extents counted in
// the sample's size; one decoded_deep_kernel launch, then the batch's stream is waited for.
int mi_batch_decode_device_deep(mi_batch *b, int first, int count, int which, const mi_device_target_deep *dst) {
  if (!batch_encoded_ok(b, first, count) || !slots_one_size(b, first, count) || !dst || !dst->dev) return MI_INVALID_ARGUMENT;
  const uint32_t w = slot_w(b, first), h = slot_h(b, first);
  if ((which != MI_DECODED_RECON && which != MI_DECODED_SOURCE) || (dst->layout != 0 && dst->layout != 1) || (dst->channels != 3 && dst->channels != 4)) return MI_INVALID_ARGUMENT;
  if (dst->sample != MI_SAMPLE_U16 && dst->sample != MI_SAMPLE_F16 && dst->sample != MI_SAMPLE_F32) return MI_INVALID_ARGUMENT;
  if (dst->sample != MI_SAMPLE_U16 && !full_scale_ok(dst->full_scale)) return MI_INVALID_ARGUMENT;
  const size_t sb = sample_bytes_of(dst->sample);
  if (((uintptr_t)dst->dev | dst->row_stride | dst->pixel_or_plane_stride | dst->image_stride) & (sb - 1)) return MI_INVALID_ARGUMENT;   // whole samples
  if ((size_t)b->n * (b->channels == 4 ? 2 : 1) != b->fs.frames.size()) return MI_INVALID_ARGUMENT;
  if (dst->channels == 3 && b->channels == 4)
    for (int i = first; i < first + count; i++) if (b->alpha_flags[i]) return MI_INVALID_ARGUMENT;      // alpha is never dropped
  DecodedDeepDst d;
  d.first = first; d.n = b->n; d.alpha_frames = b->channels == 4; d.source = which == MI_DECODED_SOURCE;
  d.sample = dst->sample; d.full_scale = dst->sample == MI_SAMPLE_U16 ? 1.0f : dst->full_scale;
  if (!strided_resolve(*dst, w, h, sb, true, d)) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  if (int st = batch_join(b, dst->after_stream)) return st;
  const dim3 grid = grid_by_four(w, h, count);
  const FrameDev *const frames = b->fs.d_frames.get();
  const bool rgb_model = b->fs.frames[first].cfg.matrix == 0;
  if (b->depth == 8) {
    if (rgb_model) hipLaunchKernelGGL((decoded_deep_kernel<8, 1>), grid, dim3(64), 0, b->stream, frames, d);
    else hipLaunchKernelGGL((decoded_deep_kernel<8, 0>), grid, dim3(64), 0, b->stream, frames, d);
  } else {
    if (rgb_model) hipLaunchKernelGGL((decoded_deep_kernel<10, 1>), grid, dim3(64), 0, b->stream, frames, d);
    else hipLaunchKernelGGL((decoded_deep_kernel<10, 0>), grid, dim3(64), 0, b->stream, frames, d);
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(b->stream));
  return MI_OK;
}
// One image into host memory (rows packed): the same launch into the batch's one-image decode scratch, grown to the sample size asked for, one D2H.
int mi_batch_decode_deep(mi_batch *b, int index, int which, int channels, int sample, float full_scale, void *dst) {
  if (!batch_encoded_ok(b, index, 1) || !dst || (channels != 3 && channels != 4)) return MI_INVALID_ARGUMENT;
  if ((which != MI_DECODED_RECON && which != MI_DECODED_SOURCE) || (channels == 3 && b->channels == 4 && b->alpha_flags[index])) return MI_INVALID_ARGUMENT;
  if (sample != MI_SAMPLE_U16 && sample != MI_SAMPLE_F16 && sample != MI_SAMPLE_F32) return MI_INVALID_ARGUMENT;
  if (sample != MI_SAMPLE_U16 && !full_scale_ok(full_scale)) return MI_INVALID_ARGUMENT;                // before the scratch grows: a refused call allocates nothing
  (void)hipSetDevice(b->device);
  const size_t sb = sample_bytes_of(sample);
  if (!staging_grow(b->d_decoded, b->d_decoded_cap, slot_px(b, index) * 4 * sb)) return MI_ENCODING_ERROR;
  mi_device_target_deep t;
  memset(&t, 0, sizeof(t));
  t.dev = b->d_decoded.get(); t.layout = 0; t.channels = channels; t.sample = sample; t.full_scale = full_scale;
  if (const int st = mi_batch_decode_device_deep(b, index, 1, which, &t)) return st;
  HIP_OK(hipMemcpy(dst, b->d_decoded.get(), slot_px(b, index) * channels * sb, hipMemcpyDeviceToHost));
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
// (the two calls below: ycc = jpeg_ycc_kernel instead of a colour kernel -- the slot holds the file's own (Y, Cb, Cr) and is tagged MI_INPUT_YCBCR)
static int batch_upload_jpeg(mi_batch *b, int index, const mi_jpeg_coeffs *c, bool ycc) {
  if (!batch_index_ok(b, index) || !c) return MI_INVALID_ARGUMENT;
  const JpegCoeffs &jc = c->jc;
  if (jc.w != slot_w(b, index) || jc.h != slot_h(b, index) || (ycc && !batch_takes_ycbcr(b))) return MI_INVALID_ARGUMENT;
  if (ycc && jc.color == JPEG_RGB) return MI_UNSUPPORTED;
  (void)hipSetDevice(b->device);
  if (int st = batch_jpeg_decode(b, jc, mi_batch_device_input(b, index), b->channels, slot_w(b, index), ycc)) return st;
  batch_tag(b, index, 1, ycc ? MI_INPUT_YCBCR : MI_INPUT_RGB);
  return MI_OK;
}
int mi_batch_upload_jpeg(mi_batch *b, int index, const mi_jpeg_coeffs *c) { return batch_upload_jpeg(b, index, c, false); }
int mi_batch_upload_jpeg_ycbcr(mi_batch *b, int index, const mi_jpeg_coeffs *c) { return batch_upload_jpeg(b, index, c, true); }
int mi_jpeg_coeffs_info(const mi_jpeg_coeffs *c, int *color, int *hsub, int *vsub) {
  if (!c) return MI_INVALID_ARGUMENT;
  const JpegCoeffs &jc = c->jc;
  if (color) *color = jc.color == JPEG_GREY ? 0 : jc.color == JPEG_YCBCR ? 1 : 2;
  if (hsub) *hsub = jc.ncomp == 3 ? jc.comp[0].h / jc.comp[1].h : 1;
  if (vsub) *vsub = jc.ncomp == 3 ? jc.comp[0].v / jc.comp[1].v : 1;
  return MI_OK;
}

// ---- PNG input: the host half behind a handle, the device half on the batch's stream ----
struct mi_png_scanlines { PngScanlines sl; std::mutex colour_mu; };
// the file's colour description, resolved on first use (png_resolve_colour inflates the iCCP chunk then): a handle may be asked from several threads
static const PngScanlines &png_handle_colour(const mi_png_scanlines *p) {
  mi_png_scanlines *const q = const_cast<mi_png_scanlines *>(p);
  std::lock_guard<std::mutex> lk(q->colour_mu);
  png_resolve_colour(q->sl);
  return q->sl;
}

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
// (the body, shared with mi_batch_resize_png: `count` checked files, each of its own size, into packed pictures of `channels` channels, back to back from `slots` on: one
// staging, one copy and one unfilter launch for the call -- its grid runs over per-image pass descriptors -- and one expand launch per stretch of equal-sized neighbours)
static int batch_png_expand(mi_batch *b, int count, const mi_png_scanlines *const *png, int channels, void *slots, bool deep = false) {
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
  const uint8_t *const cdb = db; const PngImageDev *const imgs_dev = (const PngImageDev *)(db + at + img_at);
  size_t out_at = 0;                                            // samples from `slots` to the stretch's first picture
  const int rc = for_each_group((size_t)count, [&](size_t k) { return ((uint64_t)png[k]->sl.w << 32) | png[k]->sl.h; }, [&](size_t from, size_t to) -> int {
    const uint32_t w = png[from]->sl.w, h = png[from]->sl.h; const int n = (int)(to - from);
    const PngImageDev *const stretch = imgs_dev + from;
    if (deep) { uint16_t *const out = (uint16_t *)slots + out_at; LAUNCH_BY_CHANNELS(b, channels, w, h, n, png_expand16_kernel, cdb, stretch, w, h, out); }      // files of bit depth 16 into deep slots: both bytes of every sample
    else { uint8_t *const out = (uint8_t *)slots + out_at; LAUNCH_BY_CHANNELS(b, channels, w, h, n, png_expand_kernel, cdb, stretch, w, h, out); }
    out_at += (size_t)n * w * h * channels;
    return MI_OK;
  });
  if (rc != MI_OK) return rc;
  HIP_OK(hipGetLastError());
  return MI_OK;
}
int mi_png_scanlines_info(const mi_png_scanlines *p, int *color_type, int *bit_depth) {
  if (!p) return MI_INVALID_ARGUMENT;
  if (color_type) *color_type = p->sl.ctype;
  if (bit_depth) *bit_depth = p->sl.depth;
  return MI_OK;
}

// mi_batch_upload_png and, for 16-bit masters, mi_batch_upload_png_deep (deep_handles): there a handle of bit depth 16 is unfiltered as above and expanded by
// png_expand16_kernel into its deep slot (kind MI_INPUT_RGB16); every other handle, and every handle of the plain call, goes into its 8-bit slot (kind
// MI_INPUT_RGB).  Neighbours that go the same way share one call's staging, copy and launches.  Every handle is checked before anything is staged or allocated.
static bool png_goes_deep(const mi_png_scanlines *p) { return p->sl.depth == 16 && p->sl.ctype != 3; }
static int batch_upload_png(mi_batch *b, int first, int count, const mi_png_scanlines *const *png, bool deep_handles) {
  if (!batch_range_ok(b, first, count) || !png) return MI_INVALID_ARGUMENT;
  auto goes_deep = [&](const mi_png_scanlines *p) { return deep_handles && png_goes_deep(p); };
  bool any_deep = false;
  for (int i = 0; i < count; i++) {
    if (!png[i] || png[i]->sl.w != slot_w(b, first + i) || png[i]->sl.h != slot_h(b, first + i)) return MI_INVALID_ARGUMENT;
    if (b->channels == 3 && png[i]->sl.has_alpha()) return MI_INVALID_ARGUMENT;      // alpha is never dropped
    if (goes_deep(png[i])) { any_deep = true; if (!batch_takes_deep(b, png[i]->sl.has_alpha() ? 4 : 3)) return MI_INVALID_ARGUMENT; }
  }
  if (any_deep && !batch_deep(b)) return MI_ENCODING_ERROR;
  (void)hipSetDevice(b->device);
  for (int i = 0; i < count;) {                                 // stretches of neighbours that go the same way; in a mixed layout a stretch may hold several sizes
    const bool deep = goes_deep(png[i]);
    int j = i + 1;
    while (j < count && goes_deep(png[j]) == deep) j++;
    void *const slots = deep ? (void *)mi_batch_device_input16(b, first + i) : (void *)mi_batch_device_input(b, first + i);
    if (int st = batch_png_expand(b, j - i, png + i, b->channels, slots, deep)) return st;
    batch_tag(b, first + i, j - i, deep ? MI_INPUT_RGB16 : MI_INPUT_RGB);
    i = j;
  }
  return MI_OK;
}
int mi_batch_upload_png(mi_batch *b, int first, int count, const mi_png_scanlines *const *png) { return batch_upload_png(b, first, count, png, false); }
int mi_batch_upload_png_deep(mi_batch *b, int first, int count, const mi_png_scanlines *const *png) { return batch_upload_png(b, first, count, png, true); }

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
// bounds[2 i] = first sample, bounds[2 i + 1] = taps of output sample i; tap j of output i at taps[j * out + i], `bits` fractional bits (MI_RS_BITS for the
// 8-bit kernels, MI_RS16_BITS for the deep ones; unused taps 0).  Bounds and the normalised double coefficients do not depend on `bits`.
// An axis that keeps its length: the identity (its pass is skipped: the kernel moves the samples unchanged).
static void resample_axis(uint32_t in, uint32_t out, int filter, int bits, uint32_t *bounds, int32_t *taps) {
  const size_t ksize = resample_ksize(in, out, filter);
  const int one = 1 << bits;
  if (in == out) { for (uint32_t i = 0; i < out; i++) { bounds[2 * i] = i; bounds[2 * i + 1] = 1; taps[i] = one; } return; }
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
      taps[(size_t)j * out + i] = v < 0 ? (int)(-0.5 + v * one) : (int)(0.5 + v * one);
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

// The two passes: `count` pictures of s.w x s.h described by s, turned by `o` (1..8, DESIGN.md 5l: the oriented picture is resampled from where the source lies,
// no turned copy) -> slots [first, first + count), tagged `kind`.  The tables go into the batch's pinned staging and over in one H2D (a call with the oriented
// size, the slots' size and the filter of the one before it finds them on the device); the intermediate lies `inter_at` bytes into the scratch, which the caller
// has reserved up to inter_at + resample_inter_bytes() of the ORIENTED height.  Stream order serialises the users of the scratch.  No sync.
static size_t resample_inter_bytes(int count, uint32_t src_h, uint32_t dst_w) { return (size_t)count * src_h * align_up(dst_w, 4) * 4; }
// (the tables of both axes with `bits` fractional bits, on the device when the stream gets there: horizontal bounds, taps, vertical bounds, taps.  The key holds
// the bit count, so an 8-bit call and a deep call of one shape never share a table)
struct ResampleTables { const uint32_t *hbounds, *vbounds; const int32_t *htaps, *vtaps; };
static int batch_resample_tables(mi_batch *b, uint32_t ow, uint32_t oh, uint32_t dw, uint32_t dh, int filter, int bits, ResampleTables &t) {
  const uint32_t key[6] = { ow, oh, dw, dh, (uint32_t)filter + 1, (uint32_t)bits };
  const size_t h_bytes = resample_axis_bytes(ow, dw, filter), need = align_up(h_bytes + resample_axis_bytes(oh, dh, filter), 256);
  size_t at = b->rs_key_at;
  if (memcmp(key, b->rs_key, sizeof(key)) != 0) {
    if (b->rs_used + need > b->h_rs_cap || b->rs_used + need > b->d_rs_cap) {
      HIP_OK(hipStreamSynchronize(b->stream));                // earlier calls' copies and kernels may still use the buffers that start over or are replaced
      b->rs_used = 0; b->rs_key[4] = 0;
      if (!staging_grow(b->h_rs, b->h_rs_cap, need) || !staging_grow(b->d_rs, b->d_rs_cap, need)) return MI_ENCODING_ERROR;
    }
    at = b->rs_used; b->rs_used += need;
    uint8_t *const hb = b->h_rs.get() + at;
    resample_axis(ow, dw, filter, bits, (uint32_t *)hb, (int32_t *)(hb + align_up((size_t)dw * 8, 16)));
    resample_axis(oh, dh, filter, bits, (uint32_t *)(hb + h_bytes), (int32_t *)(hb + h_bytes + align_up((size_t)dh * 8, 16)));
    HIP_OK(hipMemcpyAsync(b->d_rs.get() + at, hb, need, hipMemcpyHostToDevice, b->stream));
    memcpy(b->rs_key, key, sizeof(key)); b->rs_key_at = at;
  }
  const uint8_t *const db = b->d_rs.get() + at;
  t.hbounds = (const uint32_t *)db; t.vbounds = (const uint32_t *)(db + h_bytes);
  t.htaps = (const int32_t *)(db + align_up((size_t)dw * 8, 16)); t.vtaps = (const int32_t *)(db + h_bytes + align_up((size_t)dh * 8, 16));
  return MI_OK;
}
static int batch_resample(mi_batch *b, int first, int count, const IngestSrc &s, int filter, size_t inter_at, int o = 1, int kind = MI_INPUT_RGB) {
  const uint32_t dw = slot_w(b, first), dh = slot_h(b, first);    // the slots' size (one for the range: the callers have checked)
  uint32_t ow, oh;
  oriented_size(s.w, s.h, o, &ow, &oh);                           // 5..8: the source's height feeds the horizontal axis, its width the vertical one
  ResampleTables t;
  if (int st = batch_resample_tables(b, ow, oh, dw, dh, filter, MI_RS_BITS, t)) return st;
  const uint32_t pitch = (uint32_t)align_up(dw, 4);
  uint32_t *const inter = (uint32_t *)(b->d_rs_scratch.get() + inter_at);
  if (orientation_turns(o))
    hipLaunchKernelGGL(resample_t_kernel, dim3((dw + MI_RS_TT - 1) / MI_RS_TT, (s.w + MI_RS_TT - 1) / MI_RS_TT, (unsigned)count), dim3(256), 0, b->stream,
                       s, o, t.hbounds, t.htaps, dw, pitch, inter);
  else
    hipLaunchKernelGGL(resample_h_kernel, dim3((dw + MI_RS_TW - 1) / MI_RS_TW, (s.h + MI_RS_TH - 1) / MI_RS_TH, (unsigned)count), dim3(64 * MI_RS_TH), 0, b->stream,
                       s, o, t.hbounds, t.htaps, dw, pitch, inter);
  uint8_t *const slots = mi_batch_device_input(b, first);
  const int alpha = s.channels == 4 ? 1 : 0;
  LAUNCH_BY_CHANNELS(b, b->channels, dw, dh, count, resample_v_kernel, (const uint32_t *)inter, oh, pitch, t.vbounds, t.vtaps, dw, dh, alpha, slots);
  HIP_OK(hipGetLastError());
  batch_tag(b, first, count, kind);
  return MI_OK;
}
// The deep form (kernels: dev_resample16.h): uint16 pictures described by s -> deep slots [first, first + count), tagged MI_INPUT_RGB16.  The same
// tables with MI_RS16_BITS fractional bits, the same grids; the intermediate holds 8 bytes a pixel (resample_inter16_bytes() of the ORIENTED height, reserved
// by the caller `inter_at` bytes into the scratch, a multiple of 32).  The deep slots exist (the callers have made them).  No sync.
static size_t resample_inter16_bytes(int count, uint32_t src_h, uint32_t dst_w) { return (size_t)count * src_h * align_up(dst_w, 4) * 8; }
static int batch_resample16(mi_batch *b, int first, int count, const Ingest16Src &s, int filter, size_t inter_at, int o = 1) {
  const uint32_t dw = slot_w(b, first), dh = slot_h(b, first);
  uint32_t ow, oh;
  oriented_size(s.w, s.h, o, &ow, &oh);
  uint16_t *const slots = mi_batch_device_input16(b, first);
  if (!slots) return MI_ENCODING_ERROR;
  ResampleTables t;
  if (int st = batch_resample_tables(b, ow, oh, dw, dh, filter, MI_RS16_BITS, t)) return st;
  const uint32_t pitch = (uint32_t)align_up(dw, 4);
  uint2 *const inter = (uint2 *)(b->d_rs_scratch.get() + inter_at);
  if (orientation_turns(o))
    hipLaunchKernelGGL(resample_t16_kernel, dim3((dw + MI_RS_TT - 1) / MI_RS_TT, (s.w + MI_RS_TT - 1) / MI_RS_TT, (unsigned)count), dim3(256), 0, b->stream,
                       s, o, t.hbounds, t.htaps, dw, pitch, inter);
  else
    hipLaunchKernelGGL(resample_h16_kernel, dim3((dw + MI_RS_TW - 1) / MI_RS_TW, (s.h + MI_RS_TH - 1) / MI_RS_TH, (unsigned)count), dim3(64 * MI_RS_TH), 0, b->stream,
                       s, o, t.hbounds, t.htaps, dw, pitch, inter);
  const int alpha = s.channels == 4 ? 1 : 0;
  LAUNCH_BY_CHANNELS(b, b->channels, dw, dh, count, resample_v16_kernel, (const uint2 *)inter, oh, pitch, t.vbounds, t.vtaps, dw, dh, alpha, slots);
  HIP_OK(hipGetLastError());
  batch_tag(b, first, count, MI_INPUT_RGB16);
  return MI_OK;
}
static bool resample_filter_known(int filter) { return filter >= MI_RESAMPLE_BOX && filter <= MI_RESAMPLE_LANCZOS3; }
static bool resample_extent_ok(uint32_t w, uint32_t h) { return w >= 1 && h >= 1 && w <= 65536 && h <= 65536; }     // what a batch may have (the grids and the tables count on it)

// images [first, first + count) from pictures of src_w x src_h in the memory of the batch's device; of the batch's own size: mi_batch_upload_device
int mi_batch_resize_device(mi_batch *b, int first, int count, const mi_device_pixels *src, uint32_t src_w, uint32_t src_h, int filter) {
  IngestSrc s; uint32_t w, h;
  if (!batch_range_sized(b, first, count, w, h) || !resample_filter_known(filter) || !resample_extent_ok(src_w, src_h) || !batch_device_source(b, src, src_w, src_h, s)) return MI_INVALID_ARGUMENT;
  if (src_w == w && src_h == h) return mi_batch_upload_device(b, first, count, src);
  (void)hipSetDevice(b->device);
  if (int st = batch_reserve_scratch(b, resample_inter_bytes(count, src_h, w))) return st;
  if (int st = batch_join(b, src->after_stream)) return st;
  return batch_resample(b, first, count, s, filter, 0);
}
// the same for uint16 pictures, resampled at 16 bits into the deep slots: the refusals of mi_batch_upload_device16 and of mi_batch_resize_device,
// all before the deep slots are made (a refused call allocates nothing); of the batch's own size: mi_batch_upload_device16.  No orientation.
int mi_batch_resize_device16(mi_batch *b, int first, int count, const mi_device_pixels16 *src, uint32_t src_w, uint32_t src_h, int filter) {
  Ingest16Src s; uint32_t w, h;
  if (!batch_range_sized(b, first, count, w, h) || !resample_filter_known(filter) || !resample_extent_ok(src_w, src_h) || !batch_device_source16(b, src, src_w, src_h, s)) return MI_INVALID_ARGUMENT;
  if (src_w == w && src_h == h) return mi_batch_upload_device16(b, first, count, src);
  if (!batch_deep(b)) return MI_ENCODING_ERROR;
  (void)hipSetDevice(b->device);
  if (int st = batch_reserve_scratch(b, resample_inter16_bytes(count, src_h, w))) return st;
  if (int st = batch_join(b, src->after_stream)) return st;
  return batch_resample16(b, first, count, s, filter, 0);
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
  if (!batch_index_ok(b, index) || !c || !resample_filter_known(filter)) return MI_INVALID_ARGUMENT;
  const JpegCoeffs &jc = c->jc;
  if (jc.w == slot_w(b, index) && jc.h == slot_h(b, index)) return mi_batch_upload_jpeg(b, index, c);
  if (!resample_extent_ok(jc.w, jc.h)) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  const size_t inter_at = align_up((size_t)jc.w * jc.h * 3, 256);
  if (int st = batch_reserve_scratch(b, inter_at + resample_inter_bytes(1, jc.h, slot_w(b, index)))) return st;
  if (int st = batch_jpeg_decode(b, jc, b->d_rs_scratch.get(), 3, jc.w)) return st;
  return batch_resample(b, index, 1, resample_scratch_source(b, jc.w, jc.h, 3), filter, inter_at);
}

// one parsed PNG of any size into slot `index`: unfiltered and expanded into the scratch (RGBA when the file has alpha or tRNS, else RGB), then the two passes; of
// the batch's own size: mi_batch_upload_png
int mi_batch_resize_png(mi_batch *b, int index, const mi_png_scanlines *p, int filter) {
  if (!batch_index_ok(b, index) || !p || !resample_filter_known(filter)) return MI_INVALID_ARGUMENT;
  const int channels = p->sl.has_alpha() ? 4 : 3;
  if (channels > b->channels) return MI_INVALID_ARGUMENT;     // alpha is never dropped
  if (p->sl.w == slot_w(b, index) && p->sl.h == slot_h(b, index)) return mi_batch_upload_png(b, index, 1, &p);
  if (!resample_extent_ok(p->sl.w, p->sl.h)) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  const size_t inter_at = align_up((size_t)p->sl.w * p->sl.h * channels, 256);
  if (int st = batch_reserve_scratch(b, inter_at + resample_inter_bytes(1, p->sl.h, slot_w(b, index)))) return st;
  if (int st = batch_png_expand(b, 1, &p, channels, b->d_rs_scratch.get())) return st;
  return batch_resample(b, index, 1, resample_scratch_source(b, p->sl.w, p->sl.h, channels), filter, inter_at);
}

// ---- colour-managed input: a file's colour description baked into a transform to sRGB, applied to slots in place (icc_reader.h, dev_colour.h) ----
// A transform is host state, baked once; the first conversion on a device leaves a copy of its tables there (70 KB), which goes with the transform.
struct mi_colour_transform {
  ColourTables t;
  std::mutex mu;
  struct DevCopy { int device; uint8_t *base; };
  std::vector<DevCopy> copies;
};
static constexpr size_t MI_COLOUR_TAB8_BYTES = 1024 * sizeof(uint32_t), MI_COLOUR_LIN16_BYTES = 3 * MI_COLOUR_LIN16 * sizeof(uint32_t), MI_COLOUR_OUT16_BYTES = MI_COLOUR_OUT16 * sizeof(uint16_t);
static_assert(MI_COLOUR_LIN16 == CT_LIN16_SEG + 2 && MI_COLOUR_OUT16 == CT_OUT16_SEG + 2, "dev_colour.h and icc_reader.h speak about the same tables");
// the tables on `device` (copied there by the first call that asks, blocking); false = could not be allocated
static bool colour_on_device(mi_colour_transform *t, int device, ColourDev &d) {
  std::lock_guard<std::mutex> lk(t->mu);
  uint8_t *base = nullptr;
  for (const auto &c : t->copies) if (c.device == device) base = c.base;
  if (!base) {
    std::vector<uint8_t> host(MI_COLOUR_TAB8_BYTES + MI_COLOUR_LIN16_BYTES + MI_COLOUR_OUT16_BYTES);
    memcpy(host.data(), t->t.lin8.data(), 768 * sizeof(uint32_t));
    memcpy(host.data() + 768 * sizeof(uint32_t), t->t.thresholds.data(), 256 * sizeof(uint32_t));
    memcpy(host.data() + MI_COLOUR_TAB8_BYTES, t->t.lin16.data(), MI_COLOUR_LIN16_BYTES);
    memcpy(host.data() + MI_COLOUR_TAB8_BYTES + MI_COLOUR_LIN16_BYTES, t->t.out16.data(), MI_COLOUR_OUT16_BYTES);
    if (hipMalloc((void **)&base, host.size()) != hipSuccess) return false;
    if (hipMemcpy(base, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(base); return false; }
    t->copies.push_back({ device, base });
  }
  d.tab8 = (const uint32_t *)base; d.lin16 = (const uint32_t *)(base + MI_COLOUR_TAB8_BYTES); d.out16 = (const uint16_t *)(base + MI_COLOUR_TAB8_BYTES + MI_COLOUR_LIN16_BYTES);
  for (int i = 0; i < 9; i++) d.m[i] = (long long)t->t.matrix[i];
  return true;
}
static int colour_transform_make(int st, std::unique_ptr<mi_colour_transform> &t, mi_colour_transform **out) {
  if (st) return st;
  *out = t.release();
  return MI_OK;
}
// (for the stream workers: the transform of a description, or nullptr when it cannot be converted -- an unsupported or malformed profile, degenerate chromaticities)
static mi_colour_transform *colour_transform_from_description(const ColourDescription &d) {
  try {
    std::unique_ptr<mi_colour_transform> t(new mi_colour_transform);
    return colour_tables_from_description(d, t->t) == 0 ? t.release() : nullptr;
  } catch (const std::exception &) { return nullptr; }
}
int mi_colour_transform_from_icc(const uint8_t *icc, size_t len, mi_colour_transform **out) {
  if (!out) return MI_INVALID_ARGUMENT;
  *out = nullptr;
  if (!icc) return MI_INVALID_ARGUMENT;
  try {                                                       // nothing may unwind through the C ABI
    std::unique_ptr<mi_colour_transform> t(new mi_colour_transform);
    return colour_transform_make(colour_tables_from_icc(icc, len, t->t), t, out);
  } catch (const std::exception &) { return MI_ENCODING_ERROR; }
}
int mi_colour_transform_from_png(double file_gamma, const double *chrm8_or_null, mi_colour_transform **out) {
  if (!out) return MI_INVALID_ARGUMENT;
  *out = nullptr;
  try {
    std::unique_ptr<mi_colour_transform> t(new mi_colour_transform);
    return colour_transform_make(file_gamma == 0.0 && !chrm8_or_null ? MI_OK : colour_tables_from_png(file_gamma, chrm8_or_null, t->t), t, out);   // 0 and no cHRM: no description at all
  } catch (const std::exception &) { return MI_ENCODING_ERROR; }
}
// (the device copies go first: hipFree waits for whatever the device still runs with them)
void mi_colour_transform_free(mi_colour_transform *t) {
  if (!t) return;
  for (const auto &c : t->copies) { (void)hipSetDevice(c.device); (void)hipFree(c.base); }
  delete t;
}
// what the two calls above would answer, without the tables: the profile is parsed and the matrix made, no curve is evaluated
int mi_colour_probe_icc(const uint8_t *icc, size_t len, int *is_identity) {
  if (!icc) return MI_INVALID_ARGUMENT;
  try {
    ColourTables t;
    const int st = colour_tables_from_icc(icc, len, t, false);
    if (!st && is_identity) *is_identity = t.identity ? 1 : 0;
    return st;
  } catch (const std::exception &) { return MI_ENCODING_ERROR; }
}
int mi_colour_probe_png(double file_gamma, const double *chrm8_or_null, int *is_identity) {
  try {
    ColourTables t;
    const int st = file_gamma == 0.0 && !chrm8_or_null ? MI_OK : colour_tables_from_png(file_gamma, chrm8_or_null, t, false);
    if (!st && is_identity) *is_identity = t.identity ? 1 : 0;
    return st;
  } catch (const std::exception &) { return MI_ENCODING_ERROR; }
}
int mi_colour_transform_is_identity(const mi_colour_transform *t) { return t && t->t.identity ? 1 : 0; }
size_t mi_colour_transform_table(const mi_colour_transform *t, int which, const void **data) {
  if (!t || !data || t->t.identity) return 0;
  switch (which) {
    case 0: *data = t->t.matrix; return 9;
    case 1: *data = t->t.lin8.data(); return t->t.lin8.size();
    case 2: *data = t->t.thresholds.data(); return t->t.thresholds.size();
    case 3: *data = t->t.lin16.data(); return t->t.lin16.size();
    case 4: *data = t->t.out16.data(); return t->t.out16.size();
    default: return 0;
  }
}
int mi_png_scanlines_colour(const mi_png_scanlines *p, int *what, const uint8_t **icc, size_t *icc_len, double *file_gamma, double chrm8[8]) {
  if (!p || !what) return MI_INVALID_ARGUMENT;
  try { (void)png_handle_colour(p); } catch (const std::exception &) { return MI_ENCODING_ERROR; }      // nothing may unwind through the C ABI
  const PngScanlines &sl = p->sl;
  *what = sl.colour;
  if (icc) *icc = sl.colour == 1 && !sl.icc_oversize ? sl.icc.data() : nullptr;
  if (icc_len) *icc_len = sl.colour == 1 && !sl.icc_oversize ? sl.icc.size() : 0;
  if (file_gamma) *file_gamma = sl.colour == 3 ? sl.file_gamma : 0.0;
  if (chrm8) for (int i = 0; i < 8; i++) chrm8[i] = sl.colour == 3 && sl.has_chrm ? sl.chrm[i] : 0.0;
  return sl.colour == 1 && sl.icc_oversize ? MI_UNSUPPORTED : MI_OK;
}
int mi_jpeg_coeffs_icc(const mi_jpeg_coeffs *c, const uint8_t **icc, size_t *len) {
  if (!c || !icc || !len) return MI_INVALID_ARGUMENT;
  *icc = c->jc.icc.empty() ? nullptr : c->jc.icc.data(); *len = c->jc.icc.size();
  return MI_OK;
}

// The colour channels of slots [first, first + count) through `t`, in place, on the batch's stream (after the uploads that filled them): one launch per run of
// slots of one kind and size, all images of a run in grid z.  Every check comes first; a refused call and the identity transform launch and allocate nothing.
int mi_batch_convert_colour(mi_batch *b, int first, int count, mi_colour_transform *t) {
  if (!batch_range_ok(b, first, count) || !t) return MI_INVALID_ARGUMENT;
  for (int i = first; i < first + count; i++) if (b->kinds[i] != MI_INPUT_RGB && b->kinds[i] != MI_INPUT_RGB16) return MI_INVALID_ARGUMENT;
  if (t->t.identity) return MI_OK;
  (void)hipSetDevice(b->device);
  ColourDev d;
  if (!colour_on_device(t, b->device, d)) return MI_ENCODING_ERROR;
  for (int i = first; i < first + count;) {
    const int kind = b->kinds[i];
    const uint32_t w = slot_w(b, i), h = slot_h(b, i), row_groups = (h + MI_COLOUR_ROWS - 1) / MI_COLOUR_ROWS;    // a workgroup runs down MI_COLOUR_ROWS rows
    int j = i + 1;
    while (j < first + count && b->kinds[j] == kind && slot_w(b, j) == w && slot_h(b, j) == h) j++;
    if (kind == MI_INPUT_RGB) {
      uint8_t *const slots = mi_batch_device_input(b, i);
      LAUNCH_BY_CHANNELS(b, b->channels, w, row_groups, j - i, colour_convert_kernel, d, slots, w, h);
    } else {
      uint16_t *const slots = mi_batch_device_input16(b, i);
      if (!slots) return MI_ENCODING_ERROR;
      LAUNCH_BY_CHANNELS(b, b->channels, w, row_groups, j - i, colour_convert16_kernel, d, slots, w, h);
    }
    i = j;
  }
  HIP_OK(hipGetLastError());
  return MI_OK;
}

// ---- EXIF orientation on input: the file's tag 0x0112 read on the host (exif_reader.h), the picture turned on its way into the slot (dev_orient.h) ----
int mi_exif_orientation(const uint8_t *exif, size_t len, int *orientation) {
  if (!exif || !orientation) return MI_INVALID_ARGUMENT;
  *orientation = exif_orientation(exif, len);
  return MI_OK;
}
int mi_jpeg_coeffs_orientation(const mi_jpeg_coeffs *c, int *orientation) {
  if (!c || !orientation) return MI_INVALID_ARGUMENT;
  *orientation = c->jc.orientation;
  return MI_OK;
}
int mi_png_scanlines_orientation(const mi_png_scanlines *p, int *orientation) {
  if (!p || !orientation) return MI_INVALID_ARGUMENT;
  *orientation = p->sl.orientation;
  return MI_OK;
}
void mi_oriented_size(uint32_t w, uint32_t h, int orientation, uint32_t *ow, uint32_t *oh) { oriented_size(w, h, orientation, ow, oh); }

}  // extern "C"

// a source of sw x sh turned by `orientation` (1..8) has the size of slot `index`
static bool batch_oriented_fits(const mi_batch *b, int index, uint32_t sw, uint32_t sh, int orientation) {
  uint32_t ow, oh;
  oriented_size(sw, sh, orientation, &ow, &oh);
  return ow == slot_w(b, index) && oh == slot_h(b, index);
}
// one orient_kernel launch on the batch's stream: `count` pictures described by s (8-bit; deep: packed uint16 samples) into slots (deep slots) [first, first + count); o = 2..8
static int batch_orient(mi_batch *b, int first, int count, const IngestSrc &s, int o, bool deep) {
  const dim3 grid((slot_w(b, first) + MI_ORIENT_TILE - 1) / MI_ORIENT_TILE, (slot_h(b, first) + MI_ORIENT_TILE - 1) / MI_ORIENT_TILE, (unsigned)count), block(MI_ORIENT_THREADS);     // the slots' size (one for the range)
  if (deep) {
    uint16_t *const slots = mi_batch_device_input16(b, first);
    if (!slots) return MI_ENCODING_ERROR;
    if (b->channels == 4) hipLaunchKernelGGL((orient_kernel<4, uint16_t>), grid, block, 0, b->stream, s, o, slots);
    else hipLaunchKernelGGL((orient_kernel<3, uint16_t>), grid, block, 0, b->stream, s, o, slots);
  } else {
    uint8_t *const slots = mi_batch_device_input(b, first);
    if (b->channels == 4) hipLaunchKernelGGL((orient_kernel<4, uint8_t>), grid, block, 0, b->stream, s, o, slots);
    else hipLaunchKernelGGL((orient_kernel<3, uint8_t>), grid, block, 0, b->stream, s, o, slots);
  }
  HIP_OK(hipGetLastError());
  return MI_OK;
}
// a decoded source at the start of the scratch, packed, `channels` channels of `sample_bytes`: what the two handle forms below turn
static IngestSrc orient_scratch_source(const mi_batch *b, uint32_t w, uint32_t h, int channels, size_t sample_bytes) {
  IngestSrc s = resample_scratch_source(b, w, h, channels);
  s.inner_stride *= sample_bytes; s.row_stride *= sample_bytes; s.image_stride *= sample_bytes;
  return s;
}

extern "C" {

// images [first, first + count) from pictures in the memory of the batch's device, of the batch's size (orientations 1..4) or of h x w (5..8): one orient_kernel
// launch on the batch's stream, after whatever src->after_stream holds at this moment; orientation 1: mi_batch_upload_device
int mi_batch_orient_device(mi_batch *b, int first, int count, const mi_device_pixels *src, int orientation) {
  uint32_t w, h;
  if (!batch_range_sized(b, first, count, w, h) || orientation < 1 || orientation > 8) return MI_INVALID_ARGUMENT;
  if (orientation == 1) return mi_batch_upload_device(b, first, count, src);
  const bool turn = orientation_turns(orientation);
  IngestSrc s;
  if (!batch_device_source(b, src, turn ? h : w, turn ? w : h, s)) return MI_INVALID_ARGUMENT;
  (void)hipSetDevice(b->device);
  if (int st = batch_join(b, src->after_stream)) return st;
  if (int st = batch_orient(b, first, count, s, orientation, false)) return st;
  batch_tag(b, first, count, MI_INPUT_RGB);
  return MI_OK;
}

// one parsed JPEG into slot `index`, turned by `orientation` (0: as the file's Exif segment says): decoded into the scratch as three channels (mi_batch_upload_jpeg's
// kernels; ycbcr: jpeg_ycc_kernel, the slot is tagged MI_INPUT_YCBCR), then orient_kernel; orientation 1: mi_batch_upload_jpeg / _jpeg_ycbcr.  Every check comes first.
int mi_batch_upload_jpeg_oriented(mi_batch *b, int index, const mi_jpeg_coeffs *c, int orientation, int ycbcr) {
  if (!batch_index_ok(b, index) || !c || orientation < 0 || orientation > 8) return MI_INVALID_ARGUMENT;
  const JpegCoeffs &jc = c->jc;
  const int o = orientation ? orientation : jc.orientation;
  const bool ycc = ycbcr != 0;
  if (!batch_oriented_fits(b, index, jc.w, jc.h, o) || (ycc && !batch_takes_ycbcr(b))) return MI_INVALID_ARGUMENT;
  if (o == 1) return batch_upload_jpeg(b, index, c, ycc);
  if (ycc && jc.color == JPEG_RGB) return MI_UNSUPPORTED;
  (void)hipSetDevice(b->device);
  if (int st = batch_reserve_scratch(b, (size_t)jc.w * jc.h * 3)) return st;
  if (int st = batch_jpeg_decode(b, jc, b->d_rs_scratch.get(), 3, jc.w, ycc)) return st;
  if (int st = batch_orient(b, index, 1, orient_scratch_source(b, jc.w, jc.h, 3, 1), o, false)) return st;
  batch_tag(b, index, 1, ycc ? MI_INPUT_YCBCR : MI_INPUT_RGB);
  return MI_OK;
}

// one parsed PNG into slot `index`, turned by `orientation` (0: as the file's eXIf chunk says): unfiltered and expanded into the scratch (RGBA when the file has alpha
// or tRNS, else RGB; deep: a file of bit depth 16 as uint16 samples, on its way to the deep slot, kind MI_INPUT_RGB16), then orient_kernel; orientation 1:
// mi_batch_upload_png / _png_deep.  Every check comes first: a refused call allocates nothing.
int mi_batch_upload_png_oriented(mi_batch *b, int index, const mi_png_scanlines *p, int orientation, int deep) {
  if (!batch_index_ok(b, index) || !p || orientation < 0 || orientation > 8) return MI_INVALID_ARGUMENT;
  const PngScanlines &sl = p->sl;
  const int o = orientation ? orientation : sl.orientation, channels = sl.has_alpha() ? 4 : 3;
  const bool goes_deep = deep && png_goes_deep(p);
  if (!batch_oriented_fits(b, index, sl.w, sl.h, o) || channels > b->channels) return MI_INVALID_ARGUMENT;      // alpha is never dropped
  if (goes_deep && !batch_takes_deep(b, channels)) return MI_INVALID_ARGUMENT;
  if (o == 1) return batch_upload_png(b, index, 1, &p, deep != 0);
  if (goes_deep && !batch_deep(b)) return MI_ENCODING_ERROR;
  (void)hipSetDevice(b->device);
  const size_t sample_bytes = goes_deep ? 2 : 1;
  if (int st = batch_reserve_scratch(b, (size_t)sl.w * sl.h * channels * sample_bytes)) return st;
  if (int st = batch_png_expand(b, 1, &p, channels, b->d_rs_scratch.get(), goes_deep)) return st;
  if (int st = batch_orient(b, index, 1, orient_scratch_source(b, sl.w, sl.h, channels, sample_bytes), o, goes_deep)) return st;
  batch_tag(b, index, 1, goes_deep ? MI_INPUT_RGB16 : MI_INPUT_RGB);
  return MI_OK;
}

// ---- resize on input of a turned source: orientation and resampling in one go, from where the source lies -- no turned copy, the scratch of the plain
// resize call.  Orientation 1 (given or the file's) is the plain mi_batch_resize_* call (ycbcr: the same two passes over the file's own triples); an oriented source
// that already has the slot's size is the _oriented upload of its kind: neither takes the premultiply round trip.  Every check comes first: a refused call
// allocates nothing.  These four fill 8-bit slots: a 16-bit PNG is taken through its high bytes, as mi_batch_resize_png takes it; mi_batch_resize_png_deep and
// mi_batch_resize_device16 resample 16-bit sources into the deep slots. ----
int mi_batch_resize_device_oriented(mi_batch *b, int first, int count, const mi_device_pixels *src, uint32_t src_w, uint32_t src_h, int filter, int orientation) {
  IngestSrc s; uint32_t w, h, ow, oh;
  if (!batch_range_sized(b, first, count, w, h) || !resample_filter_known(filter) || orientation < 1 || orientation > 8 || !resample_extent_ok(src_w, src_h) ||
      !batch_device_source(b, src, src_w, src_h, s)) return MI_INVALID_ARGUMENT;
  if (orientation == 1) return mi_batch_resize_device(b, first, count, src, src_w, src_h, filter);
  oriented_size(src_w, src_h, orientation, &ow, &oh);
  if (ow == w && oh == h) return mi_batch_orient_device(b, first, count, src, orientation);
  (void)hipSetDevice(b->device);
  if (int st = batch_reserve_scratch(b, resample_inter_bytes(count, oh, w))) return st;
  if (int st = batch_join(b, src->after_stream)) return st;
  return batch_resample(b, first, count, s, filter, 0, orientation);
}

// one parsed JPEG of any size into slot `index`, turned by `orientation` (0: as the file's Exif segment says) and resampled: decoded into the scratch as three
// channels (ycbcr: jpeg_ycc_kernel -- the file's own (Y, Cb', Cr') triples are resampled channel by channel and the slot is tagged MI_INPUT_YCBCR), then the two passes
int mi_batch_resize_jpeg_oriented(mi_batch *b, int index, const mi_jpeg_coeffs *c, int filter, int orientation, int ycbcr) {
  if (!batch_index_ok(b, index) || !c || !resample_filter_known(filter) || orientation < 0 || orientation > 8) return MI_INVALID_ARGUMENT;
  const JpegCoeffs &jc = c->jc;
  const int o = orientation ? orientation : jc.orientation;
  const bool ycc = ycbcr != 0;
  if (ycc && !batch_takes_ycbcr(b)) return MI_INVALID_ARGUMENT;
  if (batch_oriented_fits(b, index, jc.w, jc.h, o)) return mi_batch_upload_jpeg_oriented(b, index, c, o, ycbcr);
  if (!resample_extent_ok(jc.w, jc.h)) return MI_INVALID_ARGUMENT;
  if (ycc && jc.color == JPEG_RGB) return MI_UNSUPPORTED;
  if (o == 1 && !ycc) return mi_batch_resize_jpeg(b, index, c, filter);
  uint32_t ow, oh;
  oriented_size(jc.w, jc.h, o, &ow, &oh);
  (void)hipSetDevice(b->device);
  const size_t inter_at = align_up((size_t)jc.w * jc.h * 3, 256);
  if (int st = batch_reserve_scratch(b, inter_at + resample_inter_bytes(1, oh, slot_w(b, index)))) return st;
  if (int st = batch_jpeg_decode(b, jc, b->d_rs_scratch.get(), 3, jc.w, ycc)) return st;
  return batch_resample(b, index, 1, resample_scratch_source(b, jc.w, jc.h, 3), filter, inter_at, o, ycc ? MI_INPUT_YCBCR : MI_INPUT_RGB);
}

// one parsed PNG of any size into slot `index`, turned by `orientation` (0: as the file's eXIf chunk says) and resampled: unfiltered and expanded into the scratch
// (RGBA when the file has alpha or tRNS, else RGB; a file of bit depth 16 through its high bytes), then the two passes
int mi_batch_resize_png_oriented(mi_batch *b, int index, const mi_png_scanlines *p, int filter, int orientation) {
  if (!batch_index_ok(b, index) || !p || !resample_filter_known(filter) || orientation < 0 || orientation > 8) return MI_INVALID_ARGUMENT;
  const PngScanlines &sl = p->sl;
  const int o = orientation ? orientation : sl.orientation, channels = sl.has_alpha() ? 4 : 3;
  if (channels > b->channels) return MI_INVALID_ARGUMENT;     // alpha is never dropped
  if (batch_oriented_fits(b, index, sl.w, sl.h, o)) return mi_batch_upload_png_oriented(b, index, p, o, 0);
  if (!resample_extent_ok(sl.w, sl.h)) return MI_INVALID_ARGUMENT;
  if (o == 1) return mi_batch_resize_png(b, index, p, filter);
  uint32_t ow, oh;
  oriented_size(sl.w, sl.h, o, &ow, &oh);
  (void)hipSetDevice(b->device);
  const size_t inter_at = align_up((size_t)sl.w * sl.h * channels, 256);
  if (int st = batch_reserve_scratch(b, inter_at + resample_inter_bytes(1, oh, slot_w(b, index)))) return st;
  if (int st = batch_png_expand(b, 1, &p, channels, b->d_rs_scratch.get())) return st;
  return batch_resample(b, index, 1, resample_scratch_source(b, sl.w, sl.h, channels), filter, inter_at, o);
}

// the deep form: a file that png_goes_deep accepts is expanded as uint16 samples into the scratch and resampled at 16 bits into its deep slot (kind
// MI_INPUT_RGB16), the flips and turns as above; every other file goes exactly as mi_batch_resize_png_oriented sends it (its bytes, kind MI_INPUT_RGB).  An oriented
// source of the slot's size is mi_batch_upload_png_oriented(.., 1).  The alpha rules of deep input (batch_takes_deep); every check comes first.
int mi_batch_resize_png_deep(mi_batch *b, int index, const mi_png_scanlines *p, int filter, int orientation) {
  if (!batch_index_ok(b, index) || !p || !resample_filter_known(filter) || orientation < 0 || orientation > 8) return MI_INVALID_ARGUMENT;
  if (!png_goes_deep(p)) return mi_batch_resize_png_oriented(b, index, p, filter, orientation);
  const PngScanlines &sl = p->sl;
  const int o = orientation ? orientation : sl.orientation, channels = sl.has_alpha() ? 4 : 3;
  if (channels > b->channels || !batch_takes_deep(b, channels)) return MI_INVALID_ARGUMENT;     // alpha is never dropped; the alpha rules of the kind
  if (batch_oriented_fits(b, index, sl.w, sl.h, o)) return mi_batch_upload_png_oriented(b, index, p, o, 1);
  if (!resample_extent_ok(sl.w, sl.h)) return MI_INVALID_ARGUMENT;
  if (!batch_deep(b)) return MI_ENCODING_ERROR;
  uint32_t ow, oh;
  oriented_size(sl.w, sl.h, o, &ow, &oh);
  (void)hipSetDevice(b->device);
  const size_t inter_at = align_up((size_t)sl.w * sl.h * channels * 2, 256);
  if (int st = batch_reserve_scratch(b, inter_at + resample_inter16_bytes(1, oh, slot_w(b, index)))) return st;
  if (int st = batch_png_expand(b, 1, &p, channels, b->d_rs_scratch.get(), true)) return st;
  Ingest16Src s;
  static_cast<IngestSrc &>(s) = orient_scratch_source(b, sl.w, sl.h, channels, 2);
  s.bits = 16; s.msb_aligned = 0;
  return batch_resample16(b, index, 1, s, filter, inter_at, o);
}

// the size of a picture of sw x sh scaled down, never up, to fit a box (an extent of 0: no bound on that axis), aspect ratio kept: the bound axis takes the
// box's extent, the free one is rounded half up (at least 1, never past the box).  Exact 64-bit integers.
void mi_fit_size(uint32_t sw, uint32_t sh, uint32_t box_w, uint32_t box_h, uint32_t *w, uint32_t *h) {
  const uint64_t W = sw, H = sh, bw = box_w, bh = box_h;
  uint64_t fw = W, fh = H;
  // (2 a b + c) / (2 c) for 32-bit a, b, c without leaving 64 bits: the quotient of a b / c, one more when twice the remainder reaches c; at least 1
  auto half_up = [](uint64_t a, uint64_t b, uint64_t c) { const uint64_t p = a * b, q = p / c + (2 * (p % c) >= c ? 1 : 0); return q ? q : (uint64_t)1; };
  if (W && H && !((bw == 0 || W <= bw) && (bh == 0 || H <= bh))) {
    if (bh == 0 || (bw != 0 && bw * H <= bh * W)) { fw = bw; fh = half_up(H, bw, W); }
    else { fh = bh; fw = half_up(W, bh, H); }
  }
  if (w) *w = (uint32_t)fw;
  if (h) *h = (uint32_t)fh;
}

}  // extern "C"
