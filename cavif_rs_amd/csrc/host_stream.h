// host_stream.h -- the stream fan-out of mi_avif.hip: the source kinds as a table, what one call's workers share (StreamCall), the per-device worker
// (StreamWorker: resident batch objects per image shape -- or, with mixed_runs, one rotation per channel count for pictures of any size --, their byte budget and eviction, the staging of a run) and the three entry points over them,
// mi_ravif_encode_sources / _stream / _batch.  Included there below host_input.h, the pool and the one-call entry points; host code only, no kernel is launched here.
#pragma once

// the rotation: resident batch objects per image shape, and the first run's share of a full run
#ifndef MI_STREAM_SLOTS_DEFAULT
#define MI_STREAM_SLOTS_DEFAULT 2          /* 256 x 1080p files end to end: 1.32 s with two, 1.48 with three, 1.51 with four (profiles/r05zk_e2e_knobs.txt, matrix 5) */
#endif
#define MI_STREAM_FIRST_RUN_NUM 1         /* a worker's first run as a share of a full one: a whole run (a half run started the GPU ~0.03 s earlier and cost two runs of 16 images, */
#define MI_STREAM_FIRST_RUN_DEN 1         /* 0.09 s of tile search each against 0.10 for 32: worker phase 1.24 -> 1.20 s on 256 files, profiles/r05zk_e2e_knobs.txt matrix 6) */

// ---- the kinds of source (MI_SOURCE_*), as data: the handle a kind carries, the upload call it takes, and whether the file's own colour description is
// applied after the upload (the managed kinds); MI_SOURCE_ORIENTED is a modifier on them, below.  A new kind is a row here, a case in StreamWorker::stage and, where its upload call refuses more, a line in source_refusal.
enum SourceHandle : uint8_t { HANDLE_NONE, HANDLE_JPEG, HANDLE_PNG };
enum UploadRoute : uint8_t { ROUTE_HOST, ROUTE_JPEG, ROUTE_JPEG_YCBCR, ROUTE_PNG, ROUTE_PNG_DEEP };   // pinned copy + mi_batch_upload_async, mi_batch_upload_jpeg, _jpeg_ycbcr, _png, _png_deep
struct SourceKind { SourceHandle handle; UploadRoute route; bool managed; };
static constexpr SourceKind SOURCE_KINDS[] = {
  { HANDLE_NONE, ROUTE_HOST, false },             // MI_SOURCE_HOST
  { HANDLE_JPEG, ROUTE_JPEG, false },             // MI_SOURCE_JPEG
  { HANDLE_PNG, ROUTE_PNG, false },               // MI_SOURCE_PNG
  { HANDLE_JPEG, ROUTE_JPEG_YCBCR, false },       // MI_SOURCE_JPEG_YCBCR
  { HANDLE_PNG, ROUTE_PNG_DEEP, false },          // MI_SOURCE_PNG_DEEP
  { HANDLE_JPEG, ROUTE_JPEG, true },              // MI_SOURCE_JPEG_MANAGED
  { HANDLE_PNG, ROUTE_PNG, true },                // MI_SOURCE_PNG_MANAGED
  { HANDLE_PNG, ROUTE_PNG_DEEP, true },           // MI_SOURCE_PNG_DEEP_MANAGED
};
static_assert(sizeof(SOURCE_KINDS) / sizeof(SOURCE_KINDS[0]) == 8 && MI_SOURCE_HOST == 0 && MI_SOURCE_JPEG == 1 && MI_SOURCE_PNG == 2 && MI_SOURCE_JPEG_YCBCR == 3 && MI_SOURCE_PNG_DEEP == 4 &&
              MI_SOURCE_JPEG_MANAGED == 5 && MI_SOURCE_PNG_MANAGED == 6 && MI_SOURCE_PNG_DEEP_MANAGED == 7, "one row per MI_SOURCE_*, in the enum's order");
// One modifier on the kinds that carry a handle, not eight more rows: MI_SOURCE_ORIENTED (0x100) ORed into kinds 1..7 -- the picture is turned as its file says on its
// way into the slot (the _oriented upload of its route), and desc names the oriented picture.  The row is found by kind & 0xFF.
// A second one, MI_SOURCE_RESIZED (0x200) on kinds 1, 2, 3, 5 and 6: desc names the OUTPUT picture -- the slot --, the file has any size and is resampled
// on its way in with mi_image_source.resize_filter (the _oriented resize call of its route; with MI_SOURCE_ORIENTED it is turned as its file asks first).
static bool source_oriented(int kind) { return (kind & MI_SOURCE_ORIENTED) != 0; }
// A third one, MI_SOURCE_RESIZED_DEEP (0x400) on kinds 4 and 7 alone: desc and resize_filter as under MI_SOURCE_RESIZED; a 16-bit file is resampled at 16
// bits into its deep slot (mi_batch_resize_png_deep), every other file as under MI_SOURCE_RESIZED on kind 2.  Never together with MI_SOURCE_RESIZED.
static bool source_resized(int kind) { return (kind & MI_SOURCE_RESIZED) != 0; }
static bool source_resized_deep(int kind) { return (kind & MI_SOURCE_RESIZED_DEEP) != 0; }
static bool source_any_resize(int kind) { return (kind & (MI_SOURCE_RESIZED | MI_SOURCE_RESIZED_DEEP)) != 0; }
static const SourceKind *source_kind(int kind) {                 // nullptr: no such kind (8..255, any other bit, a flag on host pixels, MI_SOURCE_RESIZED on the deep kinds, MI_SOURCE_RESIZED_DEEP on any other, both flags)
  const int row = kind & 0xFF;
  if (kind < 0 || (kind & ~(0xFF | MI_SOURCE_ORIENTED | MI_SOURCE_RESIZED | MI_SOURCE_RESIZED_DEEP)) != 0 || row >= 8) return nullptr;
  if ((source_oriented(kind) || source_any_resize(kind)) && row == MI_SOURCE_HOST) return nullptr;
  if (source_resized(kind) && SOURCE_KINDS[row].route == ROUTE_PNG_DEEP) return nullptr;      // the deep kinds resize under their own flag
  if (source_resized_deep(kind) && (SOURCE_KINDS[row].route != ROUTE_PNG_DEEP || source_resized(kind))) return nullptr;
  return &SOURCE_KINDS[row];
}
// the colour description of a managed source (icc_reader.h: the kind travels beside the bytes; a view into the source's handle)
static ColourDescription source_colour_description(const mi_image_source &src) {
  if (source_kind(src.kind)->handle == HANDLE_JPEG) return colour_description_of_icc(src.jpeg->jc.icc.data(), src.jpeg->jc.icc.size());
  const PngScanlines &sl = png_handle_colour(src.png);
  return colour_description_of_png(sl.colour, sl.icc_oversize, sl.icc.data(), sl.icc.size(), sl.file_gamma, sl.has_chrm, sl.chrm);
}
// MI_OK, or the status of a fetched source that names nothing usable or that its upload call would refuse: it fails alone, not with its run
static int source_refusal(const mi_ravif_encoder &e, const mi_image_source &src) {
  const mi_image_desc &x = src.desc;
  const SourceKind *const kind = source_kind(src.kind);
  if (!kind) return MI_INVALID_ARGUMENT;
  // the size desc names is the file's, or with MI_SOURCE_ORIENTED that of the file turned as it asks
  // (a resized source's file has any size the resize calls take: desc names the output, and the filter must be one of MI_RESAMPLE_*)
  const bool resized = source_any_resize(src.kind);
  if (resized && !resample_filter_known(src.resize_filter)) return MI_INVALID_ARGUMENT;
  auto fits = [&](uint32_t w, uint32_t h, int orientation) {
    if (resized) return resample_extent_ok(w, h);
    uint32_t ow, oh; oriented_size(w, h, source_oriented(src.kind) ? orientation : 1, &ow, &oh); return ow == x.width && oh == x.height;
  };
  const bool have = kind->handle == HANDLE_NONE ? x.pixels != nullptr : kind->handle == HANDLE_JPEG ? src.jpeg && fits(src.jpeg->jc.w, src.jpeg->jc.h, src.jpeg->jc.orientation) :
                    src.png && fits(src.png->sl.w, src.png->sl.h, src.png->sl.orientation) && !(x.channels == 3 && src.png->sl.has_alpha());
  if (!have || !x.width || !x.height || (x.channels != 3 && x.channels != 4)) return MI_INVALID_ARGUMENT;
  if (resized && !resample_extent_ok(x.width, x.height)) return MI_INVALID_ARGUMENT;
  if (kind->route == ROUTE_JPEG_YCBCR && !batch_takes_ycbcr(e, x.channels)) return MI_INVALID_ARGUMENT;      // the batch's rule first, then the file's colour, as in mi_batch_upload_jpeg_ycbcr
  if (kind->route == ROUTE_JPEG_YCBCR && src.jpeg->jc.color == JPEG_RGB) return MI_UNSUPPORTED;
  if (kind->route == ROUTE_PNG_DEEP && png_goes_deep(src.png) && !batch_takes_deep(e, x.channels, src.png->sl.has_alpha() ? 4 : 3)) return MI_INVALID_ARGUMENT;
  return MI_OK;
}

// ---- what the workers of one mi_ravif_encode_sources call share ----
struct StreamCall {
  const mi_ravif_encoder *e; size_t n; mi_fetch_source_fn fetch; mi_release_fn release; void *user; mi_encoded_image *out;
  size_t max_run; std::vector<int> devs;
  std::vector<int> st;                                           // per image; each index is written by the one worker that claimed it
  std::atomic<size_t> cursor{ 0 };                               // the next unclaimed image
  const bool timing = mi_timing_enabled(); const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double since() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3; }
};

// ---- the worker of one device ----
// Two resident batch objects (from the pool) per image shape (MI_STREAM_SLOTS_DEFAULT).  While one batch encodes, the host fills the next one's
// pinned staging and enqueues its H2D + encode, so uploads, tile search, entropy coding and the host-side assembly of consecutive runs overlap
// (the same rotation bench.py drives).  Memory is bounded: a batch object holds as many images of its shape as fit MI_SLOT_BYTES (one 12 MP RGBA
// image needs ~1.5 GB: such a shape gets runs of a few images, not 32), and before a new object is made the worker gives back the objects of the
// shapes it has not used for the longest time until the total stays under its budget (a share of the device's free memory at the start).
static constexpr size_t MI_SLOT_BYTES = (size_t)8 << 30;
static constexpr int NSLOT_MAX = 4, NSLOT = MI_STREAM_SLOTS_DEFAULT;
static size_t est_bytes(uint32_t w, uint32_t h, int ch, size_t images) { return images * (size_t)w * h * (ch == 4 ? 110 : 82) + ((size_t)32 << 20); }   // arena + records + staging per pixel (measured on the planner)
// what a batch object adds at its first JPEG image: MI_BATCH_JPEG_STAGED images' coefficients (at most three full planes of int16) pinned and on the device, one image's planes
static size_t est_jpeg_bytes(uint32_t w, uint32_t h) { return ((size_t)w + 15) * ((size_t)h + 15) * (2 * MI_BATCH_JPEG_STAGED * 6 + 3) + ((size_t)3 << 20); }
struct Slot { mi_batch *b = nullptr; std::future<mi_batch *> making; std::vector<size_t> idx; bool busy = false, deep = false; size_t bytes = 0, jpeg_bytes = 0, png_bytes = 0, scratch_bytes = 0; };
struct Shape { uint32_t w, h; int ch; size_t cap; Slot slot[NSLOT_MAX]; int next = 0; size_t runs = 0, last_use = 0; bool mixed = false; };
// mixed runs (mi_ravif_encoder.mixed_runs == 1): one rotation per channel count whose objects are made for `cap` pictures of this reference size and
// hold runs of pictures of any sizes that fit what such an object reserves (mi_batch_fits); the bench's own batch, under MI_SLOT_BYTES for both channel counts
static constexpr uint32_t MI_MIXED_REF_W = 1920, MI_MIXED_REF_H = 1080;
struct Baked { ColourKey key; mi_colour_transform *t; };
using Sources = std::vector<mi_image_source>;                    // the fetched sources of one claim
using Run = std::vector<size_t>;                                 // indices into them: neighbours of one shape (or, in a mixed run, of sizes that fit one object together), staged together

struct StreamWorker {
  StreamCall &call; const int dev; mi_ravif_encoder enc; size_t budget = (size_t)48 << 30;
  std::vector<std::unique_ptr<Shape>> shapes;
  // the transforms of the managed sources, by the bytes of their colour description (hash, then compare): a thousand photos of one phone bake one transform.
  // nullptr = unsupported or malformed.  They live until the worker's last run has been collected.
  std::vector<Baked> baked;
  size_t live_bytes = 0, tick = 0;

  StreamWorker(StreamCall &c, int device) : call(c), dev(device), enc(*c.e) { enc.device = dev; }
  mi_colour_transform *transform_for(const mi_image_source &src) {
    const ColourDescription desc = source_colour_description(src);
    if (desc.kind == 0) return nullptr;
    uint8_t scratch[80]; const uint8_t *p = nullptr; size_t n = 0;
    colour_description_bytes(desc, scratch, p, n);
    const uint64_t hash = colour_hash(p, n);
    for (const Baked &c : baked) if (colour_key_matches(c.key, desc.kind, hash, p, n)) return c.t;
    baked.push_back(Baked{ colour_key_make(desc.kind, hash, p, n), nullptr });
    baked.back().t = colour_transform_from_description(colour_description_of_key(baked.back().key));
    return baked.back().t;
  }
  void charge(Slot &sl, size_t extra) { sl.bytes += extra; live_bytes += extra; }      // what a slot's object holds on the device and pinned counts against the worker's budget
  void reset_accounting(Slot &sl) { live_bytes -= std::min(live_bytes, sl.bytes); sl.bytes = 0; sl.jpeg_bytes = 0; sl.deep = false; sl.png_bytes = 0; sl.scratch_bytes = 0; }
  // finish the slot's run, if any (its files and statuses go to the caller), and take an object that is being made: sl.b is the slot's object afterwards, or null
  void settle(Slot &sl) {
    if (sl.busy) {
      const int rc = mi_batch_wait(sl.b);
      if (call.timing) fprintf(stderr, "[mi_avif %8.1f ms] dev %d: run of %zu done (on the device: front end %.1f, tile search %.1f, deblock %.1f, cdef + restoration %.1f, entropy %.1f, pack + D2H %.1f ms)\n", call.since(), dev, sl.idx.size(),
                               mi_batch_stage_ms(sl.b, 0), mi_batch_stage_ms(sl.b, 1), mi_batch_stage_ms(sl.b, 2), mi_batch_stage_ms(sl.b, 3), mi_batch_stage_ms(sl.b, 4), mi_batch_stage_ms(sl.b, 5));
      for (size_t k = 0; k < sl.idx.size(); k++) call.st[sl.idx[k]] = rc == MI_OK ? mi_batch_get(sl.b, (int)k, &call.out[sl.idx[k]]) : rc;
      sl.busy = false;
    }
    if (sl.making.valid()) sl.b = sl.making.get();
  }
  void drop(Slot &sl) {                                          // settle the slot and give its object back to the device
    settle(sl);
    if (sl.b) mi_batch_destroy(sl.b);
    sl.b = nullptr; reset_accounting(sl);
  }
  // room for `need` more bytes under the budget: the objects of the shape used longest ago go first, never those of `keep`
  void make_room(const Shape *keep, size_t need) {
    while (live_bytes + need > budget) {
      Shape *victim = nullptr;
      for (auto &c : shapes) if (c.get() != keep && (!victim || c->last_use < victim->last_use)) { bool any = false; for (Slot &sl : c->slot) any |= sl.b || sl.making.valid(); if (any) victim = c.get(); }
      if (!victim) break;
      for (Slot &sl : victim->slot) drop(sl);
    }
  }
  // slot j of the shape has an object or one being made on another thread afterwards: with the pinned pixel staging when host pixels are coming (a run of JPEG / PNG
  // sources never pins it) and the PNG staging when scanlines are coming (png_staging: the bytes a full run is expected to need; a call that needs more grows it)
  void ensure_slot(Shape &sh, int j, bool host_staging, size_t png_staging) {
    Slot &sl = sh.slot[j];
    if (sl.b || sl.making.valid()) return;
    const size_t need = est_bytes(sh.w, sh.h, sh.ch, sh.cap);
    make_room(&sh, need);
    sl.bytes = need; live_bytes += need;
    const mi_ravif_encoder ec = enc; const uint32_t w = sh.w, h = sh.h; const int ch = sh.ch; const int c = (int)sh.cap;
    sl.making = std::async(std::launch::async, [ec, c, w, h, ch, host_staging, png_staging]() {
      mi_batch *nb = pool_acquire(&ec, c, w, h, ch);
      if (nb && host_staging) (void)mi_batch_input(nb, 0);
      if (nb && png_staging) (void)batch_reserve_png(nb, png_staging);
      return nb;
    });
  }
  Shape &shape_for(const mi_image_desc &x) {
    for (auto &c : shapes) if (!c->mixed && c->w == x.width && c->h == x.height && c->ch == x.channels) return *c;
    const size_t per = est_bytes(x.width, x.height, x.channels, 1);
    const size_t cap = std::max<size_t>(1, std::min(call.max_run, MI_SLOT_BYTES / per));
    shapes.emplace_back(new Shape{ x.width, x.height, x.channels, cap, {}, 0, 0, 0 });
    return *shapes.back();
  }
  // the rotation of mixed objects for `channels`, made on first use
  Shape &mixed_shape_for(int channels) {
    for (auto &c : shapes) if (c->mixed && c->ch == channels) return *c;
    const size_t per = est_bytes(MI_MIXED_REF_W, MI_MIXED_REF_H, channels, 1);
    const size_t cap = std::max<size_t>(1, std::min(call.max_run, MI_SLOT_BYTES / per));
    shapes.emplace_back(new Shape{ MI_MIXED_REF_W, MI_MIXED_REF_H, channels, cap, {}, 0, 0, 0 });
    shapes.back()->mixed = true;
    return *shapes.back();
  }
  // an object of the mixed rotation to ask mi_batch_fits of (all of a rotation's objects reserve the same; the call reads what mi_batch_create fixed, so an object with a
  // run in flight serves): the first one that exists, else the next slot's, made now and waited for.  nullptr: it could not be made
  mi_batch *mixed_probe(Shape &sh, bool host_staging, size_t png_staging) {
    for (Slot &sl : sh.slot) if (sl.b) return sl.b;
    Slot &sl = sh.slot[sh.next];
    ensure_slot(sh, sh.next, host_staging, png_staging);
    if (sl.making.valid()) sl.b = sl.making.get();
    if (!sl.b) reset_accounting(sl);
    return sl.b;
  }
  // The uploads of a run into the slot's object, enqueued on its stream in index order, one stretch of neighbours that take the same upload call at a time (a host
  // stretch never reaches across a JPEG or PNG image's slot: the pinned staging there is stale); then the conversions of the managed sources.
  int stage(const Shape &sh, Slot &sl, const Sources &d, const Run &run) {
    auto source = [&](size_t k) -> const mi_image_source & { return d[run[k]]; };
    // (an oriented source's picture is decoded into the batch's scratch first: one picture of the slot's size, two bytes a sample on the deep route, joins the worker's budget)
    auto charge_bytes = [&](size_t need) { if (need > sl.scratch_bytes) { charge(sl, need - sl.scratch_bytes); sl.scratch_bytes = need; } };
    auto charge_scratch = [&](bool deep_route, const mi_image_desc &x) { charge_bytes((size_t)x.width * x.height * 4 * (deep_route ? 2 : 1) + ((size_t)1 << 20)); };
    // (a resized source: the decoded file of fw x fh and the intermediate of the two passes, at most max(fw, fh) rows of the slot's width -- the slot is charged what its largest source needs)
    auto charge_resize = [&](uint32_t fw, uint32_t fh, const mi_image_desc &x) { charge_bytes((size_t)fw * fh * 4 + resample_inter_bytes(1, std::max(fw, fh), x.width) + ((size_t)2 << 20)); };
    // (the deep form: two bytes a sample of the decoded file, eight a pixel of the intermediate)
    auto charge_resize16 = [&](uint32_t fw, uint32_t fh, const mi_image_desc &x) { charge_bytes((size_t)fw * fh * 8 + resample_inter16_bytes(1, std::max(fw, fh), x.width) + ((size_t)2 << 20)); };
    // (the JPEG staging follows the largest file: the shape's size, or a resized source's own)
    auto charge_jpeg = [&](uint32_t fw, uint32_t fh) { const size_t need = est_jpeg_bytes(fw, fh); if (need > sl.jpeg_bytes) { charge(sl, need - sl.jpeg_bytes); sl.jpeg_bytes = need; } };
    const int rc = for_each_group(run.size(), [&](size_t k) { return (int)source_kind(source(k).kind)->route | (source(k).kind & (MI_SOURCE_ORIENTED | MI_SOURCE_RESIZED | MI_SOURCE_RESIZED_DEEP)); }, [&](size_t from, size_t to) -> int {
      const UploadRoute route = source_kind(source(from).kind)->route;
      const bool oriented = source_oriented(source(from).kind), resized = source_resized(source(from).kind);
      switch (route) {
      case ROUTE_HOST: {                                         // every image into the pinned staging, then one H2D
        for (size_t k = from; k < to; k++) {                      // (a slot has its source's size: the shape's, or in a mixed run the one mi_batch_set_sizes gave it)
          const mi_image_desc &x = source(k).desc;
          const size_t row = (size_t)x.width * sh.ch;
          uint8_t *dst = mi_batch_input(sl.b, (int)k);
          if (!dst) return MI_ENCODING_ERROR;
          const size_t sp = x.stride_px ? x.stride_px : x.width;
          if (sp == x.width) memcpy(dst, x.pixels, row * x.height);
          else for (uint32_t y = 0; y < x.height; y++) memcpy(dst + y * row, x.pixels + (size_t)y * sp * sh.ch, row);
        }
        return mi_batch_upload_async(sl.b, (int)from, (int)(to - from));
      }
      case ROUTE_JPEG: case ROUTE_JPEG_YCBCR:                    // coefficients to the batch's own staging, decoded into the slot on the batch's stream
        charge_jpeg(sh.w, sh.h);
        for (size_t k = from; k < to; k++) {
          if (resized) {                                         // any size: turned as the file asks (orientation 0) or not at all (1), resampled into the slot
            const JpegCoeffs &jc = source(k).jpeg->jc;
            charge_jpeg(jc.w, jc.h); charge_resize(jc.w, jc.h, source(k).desc);
            if (const int st = mi_batch_resize_jpeg_oriented(sl.b, (int)k, source(k).jpeg, source(k).resize_filter, oriented ? 0 : 1, route == ROUTE_JPEG_YCBCR)) return st;
            continue;
          }
          if (oriented) charge_scratch(false, source(k).desc);
          if (const int st = oriented ? mi_batch_upload_jpeg_oriented(sl.b, (int)k, source(k).jpeg, 0, route == ROUTE_JPEG_YCBCR) :
                             route == ROUTE_JPEG_YCBCR ? mi_batch_upload_jpeg_ycbcr(sl.b, (int)k, source(k).jpeg) : mi_batch_upload_jpeg(sl.b, (int)k, source(k).jpeg)) return st;
        }
        return MI_OK;
      case ROUTE_PNG: case ROUTE_PNG_DEEP: {                     // one call (one H2D, one launch per kernel); what the batch's PNG staging holds, pinned and on the device, joins the worker's budget
        std::vector<const mi_png_scanlines *> pngs;
        for (size_t k = from; k < to; k++) pngs.push_back(source(k).png);
        const size_t extra = 2 * (png_call_bytes((int)pngs.size(), pngs.data()) + ((size_t)1 << 20));
        if (extra > sl.png_bytes) { charge(sl, extra - sl.png_bytes); sl.png_bytes = extra; }
        if (route == ROUTE_PNG_DEEP && !sl.deep) { sl.deep = true; charge(sl, sh.cap * (size_t)sh.w * sh.h * sh.ch * 2); }   // the deep slots join the worker's budget
        if (source_resized_deep(source(from).kind)) {            // one file a call: a 16-bit file at 16 bits into its deep slot, any other as under MI_SOURCE_RESIZED
          for (size_t k = from; k < to; k++) {
            charge_resize16(source(k).png->sl.w, source(k).png->sl.h, source(k).desc);
            if (const int st = mi_batch_resize_png_deep(sl.b, (int)k, source(k).png, source(k).resize_filter, oriented ? 0 : 1)) return st;
          }
          return MI_OK;
        }
        if (resized) {                                           // one file a call, as above (never the deep route: source_kind)
          for (size_t k = from; k < to; k++) {
            charge_resize(source(k).png->sl.w, source(k).png->sl.h, source(k).desc);
            if (const int st = mi_batch_resize_png_oriented(sl.b, (int)k, source(k).png, source(k).resize_filter, oriented ? 0 : 1)) return st;
          }
          return MI_OK;
        }
        if (oriented) {                                          // one file a call: each goes through the scratch
          for (size_t k = from; k < to; k++) charge_scratch(route == ROUTE_PNG_DEEP, source(k).desc);
          for (size_t k = from; k < to; k++) if (const int st = mi_batch_upload_png_oriented(sl.b, (int)k, source(k).png, 0, route == ROUTE_PNG_DEEP)) return st;
          return MI_OK;
        }
        return route == ROUTE_PNG_DEEP ? mi_batch_upload_png_deep(sl.b, (int)from, (int)pngs.size(), pngs.data()) : mi_batch_upload_png(sl.b, (int)from, (int)pngs.size(), pngs.data());
      }
      }
      return MI_INVALID_ARGUMENT;
    });
    if (rc != MI_OK) return rc;
    // the managed sources, after their uploads on the same stream: neighbours that share a transform share a call
    std::vector<mi_colour_transform *> ts(run.size(), nullptr);                // one look-up (one hash of the description) per managed source
    try { for (size_t k = 0; k < run.size(); k++) if (source_kind(source(k).kind)->managed) ts[k] = transform_for(source(k)); } catch (const std::exception &) { return MI_ENCODING_ERROR; }
    return for_each_group(run.size(), [&](size_t k) { return ts[k]; }, [&](size_t from, size_t to) { return ts[from] ? mi_batch_convert_colour(sl.b, (int)from, (int)(to - from), ts[from]) : (int)MI_OK; });
  }
  // one run (<= the shape's capacity) through the shape's next slot; `more`: the call has images left after this claim
  void submit(Shape &sh, const Sources &d, const Run &run, size_t i0, bool more) {
    sh.last_use = ++tick; sh.runs++;
    const int j = sh.next; sh.next = (j + 1) % NSLOT;
    Slot &sl = sh.slot[j];
    bool any_host = false; std::vector<const mi_png_scanlines *> pngs;
    for (size_t k : run) { const SourceKind &kind = *source_kind(d[k].kind); any_host |= kind.route == ROUTE_HOST; if (kind.handle == HANDLE_PNG) pngs.push_back(d[k].png); }
    const size_t png_run = pngs.empty() ? 0 : png_call_bytes((int)pngs.size(), pngs.data());
    ensure_slot(sh, j, any_host, png_run);                       // (nothing to do for a slot that has an object, with a run in flight or not)
    settle(sl);                                                  // the slot's previous run, if any
    if (!sl.b) reset_accounting(sl);                             // the object could not be made: nothing of it is resident
    int rc = MI_ENCODING_ERROR;
    if (sl.b && sh.mixed) {                                      // the run's own sizes, laid into what the object reserved (run() has asked mi_batch_fits)
      std::vector<uint32_t> ws, hs;
      for (size_t k : run) { ws.push_back(d[k].desc.width); hs.push_back(d[k].desc.height); }
      rc = mi_batch_set_sizes(sl.b, (int)run.size(), ws.data(), hs.data());
    } else if (sl.b) rc = mi_batch_set_count(sl.b, (int)run.size());
    if (call.timing) fprintf(stderr, "[mi_avif %8.1f ms] dev %d: slot %d ready\n", call.since(), dev, j);
    if (rc == MI_OK) {
      rc = stage(sh, sl, d, run);
      if (call.timing) fprintf(stderr, "[mi_avif %8.1f ms] dev %d: slot %d staged, uploads enqueued\n", call.since(), dev, j);
    }
    if (call.release) for (size_t k : run) call.release(call.user, i0 + k);   // staged (or failed): the caller's pixels are no longer read
    if (rc == MI_OK) rc = mi_batch_encode_async(sl.b);
    if (call.timing) fprintf(stderr, "[mi_avif %8.1f ms] dev %d: run of %zu enqueued on slot %d\n", call.since(), dev, run.size(), j);
    if (rc != MI_OK) { for (size_t k : run) call.st[i0 + k] = rc; return; }
    sl.idx.clear(); for (size_t k : run) sl.idx.push_back(i0 + k);
    sl.busy = true;
    // a shape that keeps coming gets its next slot made while the GPU works on this run (not earlier: hipMalloc / hipHostMalloc on another
    // thread hold runtime locks that stall this thread's copies and launches; not for a shape seen once: a directory of differently sized files)
    if (more && sh.runs >= 2) ensure_slot(sh, sh.next, any_host, png_run);
  }
  // Claims index ranges from the shared cursor until none is left.  Images are staged in arrival order: a run is handed over as soon as the next image has
  // another shape or the run is full.  fetch may block until the image exists; a source that is refused fails alone.
  void run() {
    std::future<int> warm = std::async(std::launch::async, [dev = dev]() { return hipSetDevice(dev) == hipSuccess ? ensure_tables(dev) : (int)MI_ENCODING_ERROR; });
    { size_t fr = 0, tot = 0; if (hipSetDevice(dev) == hipSuccess && hipMemGetInfo(&fr, &tot) == hipSuccess && fr) budget = fr / 10 * 6; }
    { int sharing = 0; for (int d2 : call.devs) sharing += d2 == dev; budget /= (size_t)std::max(1, sharing); }      // workers on the same ordinal (devices = [0, 0]) split what is free
    for (size_t claims = 0;; claims++) {
      // every claim is a full run, the first one included (MI_STREAM_FIRST_RUN_NUM / _DEN)
      const size_t first_run = std::max<size_t>(1, call.max_run * MI_STREAM_FIRST_RUN_NUM / MI_STREAM_FIRST_RUN_DEN);
      const size_t want = claims == 0 ? first_run : call.max_run;
      const size_t i0 = call.cursor.fetch_add(want);             // claim the index range [i0, i1)
      if (i0 >= call.n) break;
      const size_t i1 = std::min(call.n, i0 + want);
      Sources d(i1 - i0);
      Run run; Shape *run_shape = nullptr;
      std::vector<uint32_t> run_w, run_h;                        // a mixed run's sizes so far
      auto flush = [&](bool more) { if (!run.empty()) { submit(*run_shape, d, run, i0, more); run.clear(); run_w.clear(); run_h.clear(); } };
      for (size_t i = i0; i < i1; i++) {
        mi_image_source &src = d[i - i0];
        src.resize_filter = -1;                                  // no filter: a caller that sets MI_SOURCE_RESIZED says which (one that does not know the field cannot ask for a resize)
        if (const int rc = call.fetch(call.user, i, &src)) { call.st[i] = rc; continue; }
        if (const int why = source_refusal(*call.e, src)) { call.st[i] = why; if (call.release) call.release(call.user, i); continue; }
        const SourceKind &kind = *source_kind(src.kind);
        if (enc.mixed_runs == 1) {
          // a mixed run grows in arrival order while the object's reserve takes the sizes so far; a picture that does not fit it alone goes the per-shape way below
          Shape &mx = mixed_shape_for(src.desc.channels);
          const mi_batch *probe = mixed_probe(mx, kind.route == ROUTE_HOST, kind.handle == HANDLE_PNG ? mx.cap * png_call_bytes(1, &src.png) : 0);
          if (probe && mi_batch_fits(probe, 1, &src.desc.width, &src.desc.height) == MI_OK) {
            if (&mx != run_shape || run.size() >= mx.cap) flush(true);
            run_w.push_back(src.desc.width); run_h.push_back(src.desc.height);
            if (run_w.size() > 1 && mi_batch_fits(probe, (int)run_w.size(), run_w.data(), run_h.data()) != MI_OK) {
              flush(true);
              run_w.push_back(src.desc.width); run_h.push_back(src.desc.height);
            }
            run_shape = &mx; run.push_back(i - i0);
            continue;
          }
        }
        Shape &sh = shape_for(src.desc);
        if (&sh != run_shape || run.size() >= sh.cap) flush(true);
        run_shape = &sh; run.push_back(i - i0);
        if (run.size() == 1) ensure_slot(sh, sh.next, kind.route == ROUTE_HOST, kind.handle == HANDLE_PNG ? sh.cap * png_call_bytes(1, &src.png) : 0);   // made in the background while the rest of the run arrives
      }
      if (call.timing) fprintf(stderr, "[mi_avif %8.1f ms] dev %d: images %zu..%zu fetched\n", call.since(), dev, i0, i1);
      flush(call.cursor.load() < call.n);
    }
    for (auto &c : shapes) for (Slot &sl : c->slot) {
      settle(sl);
      pool_release(sl.b);                                        // back to the pool: the next call (or nobody, at process exit) gets them
      sl.b = nullptr;
    }
    for (const Baked &c : baked) mi_colour_transform_free(c.t);
    warm.get();
    if (call.timing) fprintf(stderr, "[mi_avif %8.1f ms] dev %d: worker done\n", call.since(), dev);
  }
};

extern "C" {

// The reference's files.into_par_iter() (src/main.rs:223) over the GPUs of one node: images are independent, so a host
// thread per device pulls runs of equally-shaped images from a shared cursor and pushes each run through one resident
// batch (no collective, no cross-device traffic).  status[i] receives the per-image result; returns the first failure.
// Streaming form of the fan-out: image i is obtained through `fetch(user, i, &src)` when a worker is about to stage it (the
// call may block until the pixels exist -- e.g. until a loader thread has decoded the file), so loading, upload, encoding and
// assembly of consecutive runs overlap.  fetch returns MI_OK or a status that becomes the image's status.  An image is host pixels or the
// coefficients of a parsed JPEG or the scanlines of a parsed PNG (SOURCE_KINDS above), whose pixels come into being in the batch's HBM input slot;
// mi_ravif_encode_stream is this with MI_SOURCE_HOST throughout.
int mi_ravif_encode_sources(const mi_ravif_encoder *e, size_t n, mi_fetch_source_fn fetch, mi_release_fn release, void *user, mi_encoded_image *out, int *status, const int *devices, int ndev) {
  if (!e || !fetch || (n && !out)) return MI_INVALID_ARGUMENT;
  const int have = mi_device_count();
  std::vector<int> devs;
  if (devices && ndev > 0) devs.assign(devices, devices + ndev); else for (int d = 0; d < have; d++) devs.push_back(d);
  for (int d : devs) if (d < 0 || d >= have) { fprintf(stderr, "mi_avif: no HIP device %d (no CPU fallback)\n", d); return MI_NO_DEVICE; }
  if (devs.empty()) { fprintf(stderr, "mi_avif: no HIP device (no CPU fallback)\n"); return MI_NO_DEVICE; }
  for (size_t i = 0; i < n; i++) { out[i].avif_file = nullptr; out[i].avif_len = out[i].color_byte_size = out[i].alpha_byte_size = 0; }
  // A run holds at most 32 images, and no more than an even share of the job when it is small (64 files on 8 GPUs: 8 each, not 32 + 32 + nothing).
  const size_t max_run = std::min<size_t>(32, std::max<size_t>(1, (n + devs.size() - 1) / devs.size()));
  StreamCall call{ e, n, fetch, release, user, out, max_run, devs, std::vector<int>(n, MI_OK) };
  std::vector<std::thread> th;
  for (int d : call.devs) th.emplace_back([&call, d]() { StreamWorker(call, d).run(); });
  for (auto &t : th) t.join();
  int first = MI_OK;
  for (size_t i = 0; i < n; i++) { if (status) status[i] = call.st[i]; if (first == MI_OK && call.st[i] != MI_OK) first = call.st[i]; }
  return first;
}
// the host-pixel form: every source is MI_SOURCE_HOST
struct StreamAdapter { mi_fetch_fn fetch; mi_release_fn release; void *user; };
static int fetch_host_source(void *user, size_t i, mi_image_source *src) { const StreamAdapter *a = (const StreamAdapter *)user; src->kind = MI_SOURCE_HOST; src->jpeg = nullptr; src->png = nullptr; src->resize_filter = 0; return a->fetch(a->user, i, &src->desc); }
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

}  // extern "C"
