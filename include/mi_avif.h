/* mi_avif.h -- C ABI of the MI355X-native AV1 still-picture encode path (libmi_avif.so).
 *
 * Drop-in boundary for the one hot path cavif-rs delegates to rav1e.  The reference has no FFI here: the
 * path sits behind rav1e's Rust API, used in ravif/src/av1encoder.rs:749-771 (encode_to_av1) and configured
 * at :662-708 (rav1e_config).  Each entry point below names the reference interface it stands in for; the
 * Rust binding a ravif maintainer would add is shown in INTEGRATION.md.
 *
 * Threading: every function is re-entrant and thread-safe (no global mutable state beyond per-device
 * read-only tables built on first use); each call/batch owns its HIP stream.  All pointers are plain host
 * pointers unless a name says `dev`.  Buffers returned through `uint8_t**` / mi_encoded_image are owned by
 * the caller and released with mi_free().
 *
 * Status codes mirror ravif::Error (ravif/src/error.rs:7-25) plus the builder asserts (:117,146,159,188).
 */
#ifndef MI_AVIF_H
#define MI_AVIF_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { MI_OK = 0, MI_TOO_FEW_PIXELS = 1, MI_UNSUPPORTED = 2, MI_ENCODING_ERROR = 3, MI_INVALID_ARGUMENT = 4, MI_NO_DEVICE = 5 };

/* ---- level 1: one AV1 frame; mirrors Av1EncodeConfig (:649-660) + SpeedTweaks (:533-552) ---- */
typedef struct mi_av1_config {
  uint32_t width, height;
  uint8_t bit_depth;        /* 8 | 10 */
  uint8_t quantizer;        /* rav1e quantizer 0..255 */
  uint8_t speed;            /* 1..10 (informational once the tweaks below are filled) */
  uint8_t chroma;           /* 0 = Cs444, 1 = Cs400 */
  uint8_t pixel_range;      /* 0 = Limited, 1 = Full */
  int32_t threads;          /* bounds the tile target min(threads, w*h / min_tile_size^2) (:665-668).  <= 0 = unspecified: the
                               reference then takes rayon::current_num_threads() (:666), i.e. the host's core count; a GPU has no
                               such number, so the target is left uncapped (1080p speed 4 -> 31, i.e. 32 tiles).  Pass the
                               host's core count to get the reference's tile split: the Rust binding of INTEGRATION.md and the
                               cavif_mi command line do (no -j = this host's logical cores). */
  int8_t has_color_desc; uint8_t matrix, transfer, primaries;
  /* resolved SpeedTweaks (mi_av1_tweaks_from_preset fills them; callers may override) */
  uint8_t part_min, part_max, complex_pred_modes, sgr_full, encode_bottomup, rdo_tx_decision,
          reduced_tx_set, fine_directional_intra, fast_deblock, lrf, cdef, inter_tx_split, tx_domain_rate;
  int8_t tx_domain_distortion;
  uint16_t min_tile_size;
  int32_t tiles_override;   /* >0 forces the tile target (tests) */
  int32_t device;           /* HIP ordinal */
  uint8_t tune_psnr;        /* 0 = Tune::Psychovisual, what ravif always sets (:694); 1 = Tune::Psnr (plain SSE; ablation only) */
  uint8_t rdo_passes;       /* exactly 2 selects two-pass pricing, ANY other value means one pass (the struct grew by this field: a caller that fills it field by field
                               without zeroing must not switch modes by accident -- zero-initialise the struct, or start from mi_av1_tweaks_from_preset).
                               One pass: the tile search prices against the table of the frame's initial CDFs.  2 (an extension, not in ravif): the
                               whole encode runs twice and the second search prices every tile against the CDFs that tile ended the first
                               pass with -- a step towards rav1e's adaptive pricing that keeps tiles and superblock rows independent */
} mi_av1_config;

/* SpeedTweaks::from_my_preset (ravif/src/av1encoder.rs:554-606) */
int mi_av1_tweaks_from_preset(uint8_t speed, uint8_t quantizer, mi_av1_config *cfg);
/* quality_to_quantizer (ravif/src/av1encoder.rs:526-530) */
int mi_quality_to_quantizer(float quality);
/* rgb_to_ycbcr + casts (ravif/src/av1encoder.rs:504-524), host evaluation of the same f32 FMA chain (known-answer tests) */
void mi_rgb_to_ycbcr(const uint8_t rgb[3], int depth, uint16_t out[3]);

/* encode_to_av1 (ravif/src/av1encoder.rs:749-771): planes are host pointers to 8-bit (uint8) or 10-bit (uint16)
 * samples, Y/U/V or a single plane for Cs400.  Returns the concatenated KEY-frame OBUs (TD + sequence header +
 * frame).  recon (optional, may be NULL) receives malloc'd uint16 planes of the final reconstruction. */
int mi_av1_encode_planes(const mi_av1_config *cfg, const void *const planes[3], const size_t stride_bytes[3],
                         uint8_t **out_obu, size_t *out_len, uint16_t *recon[3]);

/* ---- level 2: ravif::Encoder (:67-86) and EncodedImage (:54-61) ---- */
typedef struct mi_ravif_encoder {
  float quality, alpha_quality;   /* with_quality :116, with_alpha_quality :145 */
  uint8_t speed;                  /* with_speed :158 */
  uint8_t color_model;            /* 0 YCbCr, 1 RGB (with_internal_color_model :174) */
  uint8_t depth;                  /* 8, 10, 0 = Auto (== 10, :266,:339) */
  uint8_t alpha_mode;             /* 0 UnassociatedDirty, 1 UnassociatedClean, 2 Premultiplied (:197) */
  int32_t threads;                /* with_num_threads :187; <=0 = None */
  const uint8_t *exif; size_t exif_len;   /* with_exif :208; copied by mi_batch_create / every encode call, need not outlive it */
  int32_t device;
  int32_t tiles_override;
  int32_t rdo_passes;             /* extension: see mi_av1_config.rdo_passes (exactly 2 = two passes; anything else = one pass, ravif's behaviour).  The struct must be
                                     zero-initialised or come from mi_ravif_encoder_default: both structs have grown at the tail and may grow again */
  int32_t mixed_runs;             /* extension, read by mi_ravif_encode_sources / _stream / _batch alone: exactly 1 lets a run hold pictures of different sizes (one
                                     rotation of batch objects per channel count, made for 32 x 1920 x 1080 at most and filled through mi_batch_set_sizes below, instead
                                     of one per shape); ANY other value keeps runs of one shape.  The files are the same either way.  It means nothing to a batch and is no
                                     part of the pool's key */
} mi_ravif_encoder;

typedef struct mi_encoded_image { uint8_t *avif_file; size_t avif_len, color_byte_size, alpha_byte_size; } mi_encoded_image;

void mi_ravif_encoder_default(mi_ravif_encoder *e);                      /* Encoder::new (:88-102) */
int  mi_ravif_encode_rgba(const mi_ravif_encoder *e, const uint8_t *rgba, uint32_t w, uint32_t h, size_t stride_px, mi_encoded_image *out);  /* :243 */
int  mi_ravif_encode_rgb (const mi_ravif_encoder *e, const uint8_t *rgb,  uint32_t w, uint32_t h, size_t stride_px, mi_encoded_image *out);  /* :318 */
/* encode_raw_planes_8_bit / _10_bit (:366,:390): interleaved [Y,U,V] triples + optional alpha plane */
int  mi_ravif_encode_raw_planes_8 (const mi_ravif_encoder *e, uint32_t w, uint32_t h, const uint8_t  *yuv, const uint8_t  *alpha, uint8_t range, uint8_t matrix, mi_encoded_image *out);
int  mi_ravif_encode_raw_planes_10(const mi_ravif_encoder *e, uint32_t w, uint32_t h, const uint16_t *yuv, const uint16_t *alpha, uint8_t range, uint8_t matrix, mi_encoded_image *out);

/* ---- many images, all GPUs of the node: the reference's files.into_par_iter() (src/main.rs:223) ----
 * One host thread per device pulls runs of equally-shaped images and pushes each run through a resident batch; images are
 * independent (no collective).  devices == NULL / ndev <= 0: every visible device.  status (nullable) gets one code per image;
 * the return value is the first failure.  out[i].avif_file is malloc'd (mi_free). */
typedef struct mi_image_desc { const uint8_t *pixels; uint32_t width, height; size_t stride_px /* 0 = width */; int channels /* 3 RGB8 | 4 RGBA8 */; } mi_image_desc;
int  mi_ravif_encode_batch(const mi_ravif_encoder *e, size_t n, const mi_image_desc *in, mi_encoded_image *out, int *status, const int *devices, int ndev);
/* streaming form: image i is pulled through `fetch` right before it is staged (the callback may block until a loader has produced
 * the pixels), so file loading overlaps the GPU work -- what rayon's work stealing gives the reference when load and encode sit in
 * one par_iter body (src/main.rs:179-223).  fetch returns MI_OK or the image's status.  `release` (nullable) is called once per
 * successfully fetched image as soon as its pixels have been copied into the pinned staging: the caller may free them and let its
 * loaders run further ahead (bounded host memory for any number of files).  Without it the pixels must stay valid until the call
 * returns.  Indices are fetched in increasing order per device thread; both callbacks may be called from several threads. */
typedef int (*mi_fetch_fn)(void *user, size_t index, mi_image_desc *desc);
typedef void (*mi_release_fn)(void *user, size_t index);
int  mi_ravif_encode_stream(const mi_ravif_encoder *e, size_t n, mi_fetch_fn fetch, mi_release_fn release, void *user, mi_encoded_image *out, int *status, const int *devices, int ndev);

/* The same fan-out over sources that need not be host pixels; the kinds are named MI_SOURCE_* below.  MI_SOURCE_JPEG (kind 1): the coefficients of a parsed
 * JPEG file (mi_jpeg_parse below); desc.width / height /
 * channels name the batch slot the picture is decoded into on the device (width and height must be the file's; channels 4 gives the pixels
 * mi_jpeg_decode_rgba gives, 3 the same without alpha), desc.pixels is unused.  Images are grouped into runs by (width, height, channels), so a JPEG and a
 * PNG picture of one size share a run.  `release` is called once the pixels (MI_SOURCE_HOST, kind 0) or the coefficients (kind 1) are in pinned staging: the handle may
 * be freed then.  MI_SOURCE_PNG (kind 2): the scanlines of a parsed PNG file (mi_png_parse below), unfiltered and expanded on the device; desc as for kind 1 (channels 3 only
 * for files without an alpha channel and without tRNS, else the image is MI_INVALID_ARGUMENT), release once the scanlines are in pinned staging.
 * MI_SOURCE_JPEG_YCBCR (kind 3): a parsed JPEG file as for kind 1, uploaded through mi_batch_upload_jpeg_ycbcr: the frame is coded from the file's own (Y, Cb, Cr) without the detour over
 * RGB.  A file whose colour is RGB gets MI_UNSUPPORTED, and an encoder with the RGB colour model or (channels 4) the premultiplied alpha mode
 * MI_INVALID_ARGUMENT, for that image alone.  Runs are grouped by (width, height, channels) as before, so kinds 0 to 3 mix in one run.
 * MI_SOURCE_PNG_DEEP (kind 4): a parsed PNG file as for kind 2, uploaded through mi_batch_upload_png_deep (below): a file of bit depth 16 is coded from all 16 bits of its samples, any
 * other file exactly as kind 2.  A 16-bit file that the alpha rules of deep input refuse (4 channels: alpha or tRNS unless alpha_mode is 0; any under
 * alpha_mode 2) gets MI_INVALID_ARGUMENT, for that image alone.
 * MI_SOURCE_JPEG_MANAGED (kind 5), MI_SOURCE_PNG_MANAGED (6), MI_SOURCE_PNG_DEEP_MANAGED (7): as kinds 1, 2 and 4 (fields, refusals, release), with the file's own
 * colour description -- a JPEG's APP2 profile; a PNG's iCCP profile, else gAMA with an optional cHRM -- applied to the slot after the upload
 * (mi_batch_convert_colour below).  A file that says nothing or sRGB, and a file whose profile is unsupported or malformed, is encoded unmanaged with status MI_OK.
 * A worker bakes one transform per distinct description (cached by the description's bytes: hash, then compare); neighbours of a run that share it share a launch.
 * MI_SOURCE_ORIENTED (0x100), ORed into kinds 1 to 7: the picture is turned as its file's EXIF orientation asks on its way into the slot (the _oriented upload of
 * its kind below; for the managed kinds the conversion follows as before: a permutation of pixels and a map of each pixel commute).  desc.width / height then name the
 * ORIENTED picture -- mi_oriented_size of the file's size and mi_jpeg_coeffs_orientation / mi_png_scanlines_orientation -- and runs are grouped by that shape; a source
 * whose oriented size differs from them is MI_INVALID_ARGUMENT, for that image alone.  So is a kind of 8..255, any other bit, and the flag on kind 0.
 * MI_SOURCE_RESIZED (0x200), ORed into kinds 1, 2, 3, 5 and 6: desc.width / height name the OUTPUT picture, which is the slot; the file may have any size
 * (extents 1..65536) and is resampled on its way in with the filter in mi_image_source.resize_filter (the mi_batch_resize_*_oriented call of its route below; the pixels
 * are specified exactly).  With MI_SOURCE_ORIENTED the file is turned as it asks and then resampled.  The managed kinds convert after the resize, in the slot, as they
 * convert after an upload: the resampling is done on the file's own sample values, not in linear light.  Runs are grouped by desc as before, so by the output shape.
 * MI_INVALID_ARGUMENT, for that image alone: the flag on kind 0 or on kinds 4 and 7 (they resize under MI_SOURCE_RESIZED_DEEP), a filter that is none of MI_RESAMPLE_*
 * (the library sets the field to -1 before it calls fetch, so a caller that sets the flag has to set the filter), a file extent outside 1..65536, a PNG with alpha
 * or tRNS into channels 3.
 * MI_SOURCE_RESIZED_DEEP (0x400), ORed into kinds 4 and 7 alone, optionally with MI_SOURCE_ORIENTED: desc and resize_filter are read as under
 * MI_SOURCE_RESIZED; a file of bit depth 16 is resampled at 16 bits into its deep slot (mi_batch_resize_png_deep below: the pixels are specified exactly), every other
 * file goes as under MI_SOURCE_RESIZED on kind 2.  Kind 7 converts after the resize, in the deep slot.  MI_INVALID_ARGUMENT, for that image alone: the flag on any
 * other kind, the flag together with MI_SOURCE_RESIZED, a filter that is none of MI_RESAMPLE_*, a file extent outside 1..65536, the alpha refusals of kind 4.
 * mi_ravif_encode_stream is this call with MI_SOURCE_HOST throughout.  Pictures in device memory are not a kind here (a pointer belongs to one
 * device, the shared cursor hands images to any): they enter through mi_ravif_encode_device and mi_batch_upload_device. */
enum { MI_SOURCE_HOST = 0, MI_SOURCE_JPEG = 1, MI_SOURCE_PNG = 2, MI_SOURCE_JPEG_YCBCR = 3, MI_SOURCE_PNG_DEEP = 4,
       MI_SOURCE_JPEG_MANAGED = 5, MI_SOURCE_PNG_MANAGED = 6, MI_SOURCE_PNG_DEEP_MANAGED = 7,
       MI_SOURCE_ORIENTED = 0x100 /* a modifier, ORed into kinds 1 to 7 */,
       MI_SOURCE_RESIZED = 0x200 /* a second modifier, ORed into kinds 1, 2, 3, 5 and 6: desc names the output size, resize_filter the filter */,
       MI_SOURCE_RESIZED_DEEP = 0x400 /* the same for kinds 4 and 7: a 16-bit file is resampled at 16 bits into its deep slot */ };
typedef struct mi_jpeg_coeffs mi_jpeg_coeffs;   /* opaque: one parsed file, host memory only */
typedef struct mi_png_scanlines mi_png_scanlines;      /* opaque: one inflated file, host memory only */
typedef struct mi_image_source {
  int kind;                   /* MI_SOURCE_HOST host pixels (desc), MI_SOURCE_JPEG JPEG coefficients (jpeg; desc.width/height/channels say the slot), MI_SOURCE_PNG PNG
                                 scanlines (png; desc likewise), MI_SOURCE_JPEG_YCBCR JPEG coefficients kept as the file's own YCbCr (jpeg; desc as for kind 1;
                                 mi_batch_upload_jpeg_ycbcr below), MI_SOURCE_PNG_DEEP PNG scanlines, 16-bit files through their deep slot (png; desc as for
                                 kind 2; mi_batch_upload_png_deep below) */
  mi_image_desc desc;
  const mi_jpeg_coeffs *jpeg;
  const mi_png_scanlines *png; /* kinds 2, 4, 6 and 7 only (the struct grew by this field at its tail: never read for kinds 0 and 1) */
  int resize_filter;           /* one of MI_RESAMPLE_* (below); read only when kind carries MI_SOURCE_RESIZED or MI_SOURCE_RESIZED_DEEP (the struct grew by this field at its tail: a fetch callback
                                  that never sets the flag need not know it) */
} mi_image_source;
typedef int (*mi_fetch_source_fn)(void *user, size_t index, mi_image_source *src);
int  mi_ravif_encode_sources(const mi_ravif_encoder *e, size_t n, mi_fetch_source_fn fetch, mi_release_fn release, void *user, mi_encoded_image *out,
                             int *status, const int *devices, int ndev);

/* A picture in the memory of a HIP device: uint8 samples, interleaved (HWC) or planar (CHW), any byte strides that do not make rows overlap their own
 * pixels (row_stride >= the packed row, pixel stride >= channels, plane stride >= width): crops, permuted views and padded rows of a tensor all fit.
 * 3 channels into an RGBA batch get alpha 255 (as load_rgba gives RGB files); 4 channels into an RGB batch are MI_INVALID_ARGUMENT. */
typedef struct mi_device_pixels {
  const void *dev;
  int layout;        /* 0 = HWC, 1 = CHW */
  int channels;      /* 3 | 4 */
  size_t row_stride, pixel_or_plane_stride, image_stride;   /* bytes; 0 = packed */
  void *after_stream; /* hipStream_t the pixels were produced on, or NULL = already complete */
} mi_device_pixels;
/* ravif::Encoder::encode_rgb / encode_rgba (by src->channels) of a w x h picture in the memory of device e->device.  The pointer must belong to that
 * device (not detected).  Blocking, through the pooled batch objects like mi_ravif_encode_rgba. */
int  mi_ravif_encode_device(const mi_ravif_encoder *e, const mi_device_pixels *src, uint32_t w, uint32_t h, mi_encoded_image *out);
/* 8-bit YCbCr planes in the memory of a HIP device, BT.601 full range (JFIF's matrix: the one the colour frames signal): what rocJPEG / rocDecode deliver.
 * Chroma is subsampled by (hsub, vsub) luma samples per chroma sample and has ceil(w / hsub) x ceil(h / vsub) samples, sited at the centre of the luma
 * samples it covers (JPEG's siting, not MPEG-2's co-sited columns).  See mi_batch_upload_device_ycbcr below for the exact bytes. */
typedef struct mi_device_planes {
  const void *y, *cb, *cr;   /* cr == NULL: cb points at interleaved (Cb, Cr) byte pairs (NV12-style) */
  int hsub, vsub;            /* luma samples per chroma sample: (1,1), (2,1) or (2,2); anything else MI_INVALID_ARGUMENT */
  size_t y_row_stride, c_row_stride, y_image_stride, c_image_stride;   /* bytes; 0 = packed; same for Cb and Cr */
  void *after_stream;        /* hipStream_t the planes were produced on, or NULL = already complete */
} mi_device_planes;
/* mi_ravif_encode_device for such planes: the file of a 3-channel batch of one image fed through mi_batch_upload_device_ycbcr.  Blocking, pooled. */
int  mi_ravif_encode_device_ycbcr(const mi_ravif_encoder *e, const mi_device_planes *src, uint32_t w, uint32_t h, mi_encoded_image *out);
/* The same for a picture of src_w x src_h that is resampled to w x h on the device on the way in (mi_batch_resize_device below: `filter` is one of
 * MI_RESAMPLE_*, the pixels are specified exactly).  Blocking, pooled by (w, h, channels) like mi_ravif_encode_device. */
int  mi_ravif_encode_device_resized(const mi_ravif_encoder *e, const mi_device_pixels *src, uint32_t src_w, uint32_t src_h, uint32_t w, uint32_t h, int filter,
                                    mi_encoded_image *out);

/* The one-call entry points above (mi_ravif_encode_rgba / _rgb / _device / _batch / _stream / _sources) keep their device arenas and pinned staging in
 * a process-wide pool keyed by (device, shape, settings), so a loop of calls with the same settings pays the allocation once
 * (what a long-lived rav1e thread pool is to the reference).  At most 12 objects / 96 GB are retained; this frees them now, and the idle JPEG
 * decode contexts (at most 8 exist per device) with them. */
void mi_release_cached(void);

/* PNG -> RGBA8 as cavif's load_rgba does (src/main.rs:265-283: RGB gets alpha 255, 16-bit samples keep their high byte, gray is
 * replicated); all colour types, bit depths, tRNS and Adam7.  Host code over zlib.  *rgba is malloc'd (mi_free), w*h*4 bytes. */
int  mi_png_decode_rgba(const uint8_t *data, size_t len, uint8_t **rgba, uint32_t *w, uint32_t *h);
/* The host half of a PNG decode on its own: chunk walk, inflate and every check that can fail (filter bytes, palette indices) into a handle that holds the
 * inflated scanlines.  Never touches a device; the status for any bytes is the one mi_png_decode_rgba gives.  *has_alpha (nullable): the file has an alpha
 * channel or a tRNS chunk.  The handle feeds mi_batch_upload_png and mi_ravif_encode_sources (kind 2) any number of times, from any thread, and is released
 * with mi_png_scanlines_free (NULL is fine). */
int  mi_png_parse(const uint8_t *data, size_t len, mi_png_scanlines **out, uint32_t *w, uint32_t *h, int *has_alpha);
void mi_png_scanlines_free(mi_png_scanlines *p);
/* JPEG -> RGBA8, the other format cavif's loader takes (load_image::load_data, src/main.rs:258; load_rgba :265-283: alpha 255, gray replicated).
 * Baseline / extended sequential and progressive Huffman files, 8 bit, one component or three at 4:4:4 / 4:2:2 / 4:2:0; arithmetic coding, lossless,
 * hierarchical, 12-bit, four-component files and other sampling ratios are MI_UNSUPPORTED, broken or incomplete streams MI_ENCODING_ERROR.  Huffman
 * decoding runs on the host, dequantisation + IDCT + chroma upsampling + YCbCr->RGB on HIP device `device`; the pixels are libjpeg's (integer "islow"
 * IDCT, "fancy" upsampling), embedded ICC profiles and EXIF orientation are ignored (this call still hands out the sensor's rows: orientation is applied by the
 * oriented uploads below and by nothing else).  Data errors are reported before the device is looked at, then
 * MI_NO_DEVICE when there is no such device: no CPU fallback.  *rgba is malloc'd (mi_free), w*h*4 bytes.  Calls from many threads share a pool of at most 8
 * decode contexts per device (stream + staging; a call that finds all of them busy waits for one) that mi_release_cached() frees. */
int  mi_jpeg_decode_rgba(const uint8_t *data, size_t len, int device, uint8_t **rgba, uint32_t *w, uint32_t *h);
/* The host half of mi_jpeg_decode_rgba on its own: parse + Huffman decoding into a handle (quantised coefficients and tables, host memory).  Never touches a
 * device; the statuses are the ones mi_jpeg_decode_rgba gives for the same bytes' data errors.  The handle feeds mi_batch_upload_jpeg and
 * mi_ravif_encode_sources any number of times, from any thread, and is released with mi_jpeg_coeffs_free (NULL is fine). */
int  mi_jpeg_parse(const uint8_t *data, size_t len, mi_jpeg_coeffs **out, uint32_t *w, uint32_t *h);
void mi_jpeg_coeffs_free(mi_jpeg_coeffs *c);
/* load_rgba (src/main.rs:255-283) over both: the first bytes decide -- PNG -> mi_png_decode_rgba (host, `device` unused), FF D8 -> mi_jpeg_decode_rgba,
 * anything else MI_UNSUPPORTED. */
int  mi_image_decode_rgba(const uint8_t *data, size_t len, int device, uint8_t **rgba, uint32_t *w, uint32_t *h);

/* ---- batch: the data-parallel path (src/main.rs:223 files.into_par_iter()); images resident in HBM ---- */
typedef struct mi_batch mi_batch;
/* n images of w x h, channels 3 (RGB8) or 4 (RGBA8) on HIP device `e->device` */
mi_batch *mi_batch_create(const mi_ravif_encoder *e, int n_images, uint32_t w, uint32_t h, int channels);
int  mi_batch_upload(mi_batch *b, int index, const uint8_t *pixels, size_t stride_px);   /* copy into the pinned staging + H2D into the batch's HBM input slot (blocking) */
/* zero-copy form: fill the batch's PINNED host staging of image `index` (w*h*channels bytes, rows packed) in place, then enqueue
 * the H2D of a range of images on the batch's stream (returns at once; ordered before the next mi_batch_encode[_async]).
 * The staging is pinned by the first mi_batch_input / mi_batch_upload of a batch, not by mi_batch_create (a batch fed through the device-resident calls
 * below never pins it): that first call takes the time of pinning n * w * h * channels bytes, makes the batch's device the calling thread's current HIP
 * device like the other mi_batch_* calls, and returns NULL (mi_batch_upload[_async]: MI_ENCODING_ERROR / MI_INVALID_ARGUMENT) when the memory cannot be
 * pinned.  It may come from several threads at once. */
uint8_t *mi_batch_input(mi_batch *b, int index);
int  mi_batch_upload_async(mi_batch *b, int first, int count);
/* device-resident input: the picture reaches the slot without ever being host pixels.
 * mi_batch_device_input: the HBM input slot of image `index` (w*h*channels bytes, rows packed): a HIP caller may write it directly, ordered before the
 * next encode by its own means.  mi_batch_read_input: D2H of that slot into dst (w*h*channels bytes), blocking; tests and debugging, like mi_batch_get_recon.
 * mi_batch_upload_device: images [first, first+count) from memory of the batch's own device (documented, not detected), image k at
 * dev + k * image_stride; enqueued on the batch's stream -- after the work src->after_stream holds at the time of the call, if given -- and returns
 * at once: the source must stay valid until the next mi_batch_wait.
 * mi_batch_upload_jpeg: one parsed JPEG of the batch's width and height (else MI_INVALID_ARGUMENT) into slot `index`: coefficients into pinned staging
 * the batch owns, H2D, dequantisation + IDCT + upsampling + colour on the batch's stream, no sync; the handle may be freed when the call returns.
 * mi_batch_upload_png: images [first, first+count) from parsed PNG files of the batch's width and height (else MI_INVALID_ARGUMENT; so is a file with an
 * alpha channel or tRNS into a 3-channel batch: alpha is never dropped): scanlines into pinned staging the batch owns, one H2D, the scanline filters undone and
 * the samples expanded to the slot's pixels -- those of mi_png_decode_rgba -- on the batch's stream, one launch per kernel for the whole call, no sync; the
 * handles may be freed when the call returns.
 * The upload calls return MI_INVALID_ARGUMENT between mi_batch_encode_async and mi_batch_wait. */
/* ---- input kinds: what the bytes of a slot mean.  MI_INPUT_RGB: (R, G, B[, A]), converted by the front end (BT.601 full range, rgb_to_ycbcr).
 * MI_INPUT_YCBCR: (Y, Cb, Cr) in a 3-channel batch, (Y, Cb, Cr, 255) in a 4-channel one, BT.601 full range already.  With (Y, C1, C2) the slot bytes of a
 * pixel the planes of the colour frame are, without any matrix,
 *   8 bit:   p0 = Y, p1 = C1, p2 = C2
 *   10 bit:  p0 = floor((2046 Y + 255) / 510),  p_k = clamp(512 + floor((2046 (C_k - 128) + 255) / 510), 0, 1023)      (floor towards -inf)
 * i.e. the scale 1023/255 about the centres (128 -> 512), rounded half up: the convention of rgb_to_ycbcr at depth 10 and the one mi_batch_decode's q() inverts
 * (bit replication would map neutral chroma 128 to 514).  Samples past the picture replicate its edge as for RGB.  Such an image is opaque: its fourth byte
 * is not read, it never gets an alpha frame (mi_batch_uses_alpha 0), and the clean alpha mode leaves it as it is.  mi_batch_get_source, mi_batch_measure and
 * mi_batch_decode* (MI_DECODED_SOURCE: through the exact inverse) then speak about the YCbCr the source held.
 * The kind is host state per slot, set by whichever call last filled the slot: every upload / resize call above and below tags its slots MI_INPUT_RGB, the
 * three *_ycbcr calls tag theirs MI_INPUT_YCBCR; it survives encodes and mi_batch_set_count as the slot's contents do.  mi_batch_set_input_kind is for HIP
 * callers that write mi_batch_device_input themselves.  MI_INPUT_YCBCR is refused with MI_INVALID_ARGUMENT (by the set call and the *_ycbcr uploads alike)
 * when the encoder's colour model is RGB (color_model 1) and when the batch has 4 channels and alpha_mode 2 (premultiplied: defined on RGB colours).
 * mi_batch_set_input_kind: MI_INVALID_ARGUMENT as well for a range past the capacity, a kind not 0, 1, 2 or 3 (MI_INPUT_RGB16 and MI_INPUT_YCBCR16: deep
 * input and deep YCbCr planes, below; both refused while the batch has no deep slots), a call between mi_batch_encode_async and mi_batch_wait.
 * mi_batch_upload_jpeg_ycbcr: mi_batch_upload_jpeg (staging, H2D, IDCT, ordering, lifetimes) ending in jpeg_ycc_kernel: the slot's pixels are
 * (Y, Cb', Cr') of a three-component YCbCr file, Cb' Cr' libjpeg's fancy-upsampled chroma -- exactly the triples whose 16.16 conversion mi_batch_upload_jpeg
 * stores -- and (Y, 128, 128) of a grey file.  A file whose colour is RGB (Adobe transform 0, or components named R G B): MI_UNSUPPORTED; a size mismatch, an
 * encode in flight or a refusal of the kind: MI_INVALID_ARGUMENT (checked first).
 * mi_jpeg_coeffs_info: *color 0 grey, 1 YCbCr, 2 RGB; *hsub, *vsub luma samples per chroma sample (1, 1 for grey); any of the three may be NULL.
 * mi_batch_upload_device_ycbcr: images [first, first + count) from mi_device_planes of the batch's own device, image k's planes at y + k * y_image_stride and
 * cb / cr + k * c_image_stride; one launch on the batch's stream, ordered after src->after_stream, returns at once; the source must stay valid until the next
 * mi_batch_wait.  Pixel (x, y) gets Y = y[y][x] and chroma upsampled as libjpeg's h2v1 / h2v2 "fancy" upsampling does, with c[j][i] the chroma sample of row j,
 * column i, indices clamped to the plane (edges replicated), cw = ceil(w / hsub), i = floor(x / 2), j = floor(y / 2):
 *   (1,1)  c[y][x]
 *   (2,1)  cw <= 2: c[y][i];  else x even: (3 c[y][i] + c[y][i-1] + 1) >> 2,  x odd: (3 c[y][i] + c[y][i+1] + 2) >> 2
 *   (2,2)  cw <= 2: c[j][i];  else with v(i) = 3 c[j][i] + c[j'][i], j' = j - 1 for even y and j + 1 for odd y:
 *          x even: (3 v(i) + v(i-1) + 8) >> 4,  x odd: (3 v(i) + v(i+1) + 7) >> 4
 * MI_INVALID_ARGUMENT: null b / src / y / cb, another (hsub, vsub), a row stride below the packed row (w for y; cw, or 2 cw interleaved, for chroma), a
 * range past the capacity, a refusal of the kind, a call between mi_batch_encode_async and mi_batch_wait. */
enum { MI_INPUT_RGB = 0, MI_INPUT_YCBCR = 1, MI_INPUT_RGB16 = 2, MI_INPUT_YCBCR16 = 3 };
int  mi_batch_set_input_kind(mi_batch *b, int first, int count, int kind);
int  mi_batch_input_kind(mi_batch *b, int index, int *kind);
int  mi_batch_upload_jpeg_ycbcr(mi_batch *b, int index, const mi_jpeg_coeffs *c);
int  mi_jpeg_coeffs_info(const mi_jpeg_coeffs *c, int *color, int *hsub, int *vsub);
int  mi_batch_upload_device_ycbcr(mi_batch *b, int first, int count, const mi_device_planes *src);
uint8_t *mi_batch_device_input(mi_batch *b, int index);
int  mi_batch_read_input(mi_batch *b, int index, uint8_t *dst);
int  mi_batch_upload_device(mi_batch *b, int first, int count, const mi_device_pixels *src);
int  mi_batch_upload_jpeg(mi_batch *b, int index, const mi_jpeg_coeffs *c);
int  mi_batch_upload_png(mi_batch *b, int first, int count, const mi_png_scanlines *const *png);
/* ---- deep input: 16-bit sources.  MI_INPUT_RGB16: the image is read from its DEEP slot, a second slot array beside the 8-bit one: w*h*channels
 * uint16 samples per image, rows packed, images back to back, FULL SCALE 0..65535, (R, G, B[, A]).  The array is made by the first call that needs it (any
 * call below but mi_png_scanlines_info and mi_batch_footprint) and never by a batch that sees no 16-bit source; the 8-bit slot of such an image is ignored.
 * mi_batch_set_input_kind(.., 2) tags what a HIP caller wrote through mi_batch_device_input16: on a batch whose deep slots do not exist yet it has nothing to
 * tag, allocates nothing and answers MI_INVALID_ARGUMENT.  Kinds 0, 1 and 2 mix freely in one batch; the kind follows the last call that filled the slot and survives encodes and mi_batch_set_count.
 * The planes of the colour frame are specified exactly, in integers.  M = 65535, bd = the batch's bit depth (8 | 10), peak = 2^bd - 1, half = 2^(bd-1), floor
 * division towards minus infinity:
 *   YCbCr model:  S  = 299 R + 587 G + 114 B
 *                 Y  = floor((2 peak S + 1000 M) / (2000 M))
 *                 Cb = clamp(half + floor((2 peak (1000 B - S) + 1772 M) / (3544 M)), 0, peak)
 *                 Cr = clamp(half + floor((2 peak (1000 R - S) + 1402 M) / (2804 M)), 0, peak)
 *   RGB model (planes G, B, R) and the alpha plane:  p = floor((2 peak v + M) / (2 M))
 * i.e. BT.601 with Kr = 0.299, Kb = 0.114 and the scale peak / M, rounded half up: the constants mi_batch_decode's q() inverts; grey gives chroma exactly half.
 * Samples past the picture replicate its edge.  The image uses alpha when A != 65535 anywhere inside w x h.
 * Alpha rules (the dirty-alpha cleaner and the premultiplied mode are defined on 8-bit samples and are not generalised): a 3-channel batch takes kind 2 under
 * every alpha mode.  In a 4-channel batch a 3-channel deep source is stored with A = 65535 -- opaque, skipped by the cleaner as MI_INPUT_YCBCR is -- and is taken
 * under alpha_mode 0 and 1; a 4-channel deep source and mi_batch_set_input_kind(.., 2) need alpha_mode 0; alpha_mode 2 takes none.  4 channels into a 3-channel
 * batch are refused.  Every refusal is MI_INVALID_ARGUMENT and allocates nothing.
 * mi_batch_device_input16: the deep slot of image `index` in device memory (a HIP caller may write it and then tag it with mi_batch_set_input_kind), NULL when
 * it cannot be made.  mi_batch_read_input16: D2H of that slot (w*h*channels uint16), blocking; tests and debugging.  mi_batch_footprint: the bytes of device
 * and pinned memory the batch holds now (what the pool of the one-call entry points counts).
 * mi_batch_upload_device16: mi_batch_upload_device (after_stream, ordering, lifetimes, stride rules in BYTES) for uint16 samples; the pointer and every stride
 * must be even.  A sample v is first reduced to `bits` (8..16) -- masked to its low bits, or v >> (16 - bits) when msb_aligned -- then widened by bit
 * replication, (v << (16 - bits)) | (v >> (2 bits - 16)): 16 bits pass unchanged, 8 bits give 257 v, and a 10-bit (8-bit) sample comes back from the RGB-model
 * formula above at depth 10 (8) as itself.  One launch for all images of the call.
 * mi_batch_upload16: one image of full-scale host pixels, rows stride_px pixels apart (0 = packed), channels 3 | 4; blocking, on the batch's stream.
 * mi_batch_upload_png_deep: mi_batch_upload_png where a handle whose file has bit depth 16 (colour types 0, 2, 4, 6; Adam7) fills its deep slot with both
 * bytes of every sample -- grey replicated, the tRNS colour key compared on all 16 bits (A = 0, else 65535), a file with an alpha channel or tRNS a 4-channel
 * source under the rules above -- and every other handle goes exactly as mi_batch_upload_png sends it, kind 0.  All handles are checked before any is staged.
 * mi_png_scanlines_info: the file's colour type and bit depth (either pointer may be NULL): bit depth 16 is what goes deep.
 * mi_ravif_encode_device16: mi_ravif_encode_device for such a source. */
typedef struct mi_device_pixels16 {        /* mi_device_pixels for uint16 samples, plus how many bits of a sample count */
  const void *dev;
  int layout;        /* 0 = HWC, 1 = CHW */
  int channels;      /* 3 | 4 */
  size_t row_stride, pixel_or_plane_stride, image_stride;   /* bytes, even; 0 = packed */
  void *after_stream; /* hipStream_t the pixels were produced on, or NULL = already complete */
  int bits;          /* 8..16 significant bits */
  int msb_aligned;   /* 0: they are the low bits of a sample (bits above them are ignored), 1: the high bits */
} mi_device_pixels16;
uint16_t *mi_batch_device_input16(mi_batch *b, int index);
int  mi_batch_read_input16(mi_batch *b, int index, uint16_t *dst);
size_t mi_batch_footprint(const mi_batch *b);
int  mi_batch_upload_device16(mi_batch *b, int first, int count, const mi_device_pixels16 *src);
int  mi_batch_upload16(mi_batch *b, int index, const uint16_t *pixels, size_t stride_px, int channels);
int  mi_batch_upload_png_deep(mi_batch *b, int first, int count, const mi_png_scanlines *const *png);
int  mi_png_scanlines_info(const mi_png_scanlines *p, int *color_type, int *bit_depth);
/* ---- deep YCbCr planes.  MI_INPUT_YCBCR16: the image is read from its deep slot (laid out as for MI_INPUT_RGB16: w*h*channels uint16 samples,
 * rows packed), which holds (Y, Cb, Cr[, 65535]) in a CANONICAL 16-bit form: BT.601 full range, M = 65535, chroma centred on 32768.  Such an image is opaque
 * exactly as MI_INPUT_YCBCR is: its fourth sample is never read, it never gets an alpha frame (mi_batch_uses_alpha 0), the clean alpha mode leaves it alone.
 * The kind is taken where MI_INPUT_YCBCR is: it needs the YCbCr colour model and is refused in a 4-channel batch under alpha_mode 2; every refusal is
 * MI_INVALID_ARGUMENT and allocates nothing.  mi_batch_set_input_kind(.., 3) tags what a HIP caller wrote through mi_batch_device_input16 and, like kind 2,
 * is refused while the batch has no deep slots.  Kinds 0 to 3 mix freely in one batch.  mi_batch_convert_colour refuses a slot of this kind.
 * All maps are exact integers, floor division towards minus infinity.  A source sample is first reduced to its `bits` (8..16) as mi_batch_upload_device16
 * does -- masked to its low bits, or v >> (16 - bits) when msb_aligned -- giving v; P = 2^bits - 1, c = 2^(bits-1), s = 2^(bits-8).  Source to slot sample W:
 *   full range    Y: W = floor((2 M v + P) / (2 P))
 *                 C: W = clamp(32768 + floor((2 M (v - c) + P) / (2 P)), 0, M)
 *   narrow range  Y: W = clamp(floor((2 M (v - 16 s) + 219 s) / (438 s)), 0, M)
 *                 C: W = clamp(32768 + floor((2 M (v - 128 s) + 224 s) / (448 s)), 0, M)
 * Slot sample to plane, bd = the batch's bit depth, peak = 2^bd - 1, half = 2^(bd-1):
 *   p0  = floor((2 peak Y + M) / (2 M))
 *   p_k = clamp(half + floor((2 peak (C_k - 32768) + M) / (2 M)), 0, peak)
 * With bits == bd (8 or 10) a full-range sample reaches its plane as itself, luma and chroma (P010 full range at depth 10 is lossless on the way in); with
 * bits = 8 the planes at depth 10 are those of MI_INPUT_YCBCR; neutral chroma c gives half for every `bits`.  The contract is this two-stage map: for 14 and 15
 * bits into depth 10 it differs from one direct rounding at a few dozen values.  Samples past the picture replicate its edge.
 * Chroma upsampling is done on W, not on source samples: every chroma sample is mapped first, then the formulas of mi_batch_upload_device_ycbcr above apply to
 * the W values unchanged (libjpeg's h2v1 / h2v2 weights and rounding constants, planes of one or two samples' width replicated, edges clamped, centred siting;
 * a sum reaches at most 16 M).  So a SUBSAMPLED 8-bit source sent through this call (bits = 8) does not give the 8-bit call's slot times 257: the rounding
 * happens at 16 bits here.  A 4:4:4 one (no upsampling) gives the 8-bit call's planes and so its file.
 * The files stay tagged matrix 6 (BT.601), full range, as the 8-bit path's are; narrow range is expanded, never signalled.
 * mi_batch_upload_device_ycbcr16: mi_batch_upload_device_ycbcr (after_stream, ordering, lifetimes, image k's planes at y + k * y_image_stride and cb / cr +
 * k * c_image_stride) for uint16 samples; strides in BYTES; one launch for all images of the call; the slots are tagged MI_INPUT_YCBCR16.
 * MI_INVALID_ARGUMENT: null b / src / y / cb, another (hsub, vsub), bits outside 8..16, msb_aligned or narrow_range not 0 or 1, an odd pointer or stride, a
 * row stride below the packed row (2 w for y; 2 cw, or 4 cw interleaved, for chroma), a range past the capacity, a refusal of the kind, a call between
 * mi_batch_encode_async and mi_batch_wait -- all checked before the deep slots are made.  MI_ENCODING_ERROR when the deep slots cannot be allocated.
 * mi_ravif_encode_device_ycbcr16: mi_ravif_encode_device_ycbcr for such planes.  Blocking, pooled. */
typedef struct mi_device_planes16 {      /* mi_device_planes for uint16 samples */
  const void *y, *cb, *cr;               /* cr == NULL: cb points at interleaved (Cb, Cr) uint16 pairs (P010 / P016-style) */
  int hsub, vsub;                        /* (1,1), (2,1), (2,2) */
  size_t y_row_stride, c_row_stride, y_image_stride, c_image_stride;   /* bytes, even; 0 = packed */
  void *after_stream;
  int bits, msb_aligned;                 /* 8..16; P010 = 10, 1 */
  int narrow_range;                      /* 0 full, 1 narrow ("video") range, expanded by the maps above */
} mi_device_planes16;
int  mi_batch_upload_device_ycbcr16(mi_batch *b, int first, int count, const mi_device_planes16 *src);
int  mi_ravif_encode_device_ycbcr16(const mi_ravif_encoder *e, const mi_device_planes16 *src, uint32_t w, uint32_t h, mi_encoded_image *out);
int  mi_ravif_encode_device16(const mi_ravif_encoder *e, const mi_device_pixels16 *src, uint32_t w, uint32_t h, mi_encoded_image *out);
/* ---- colour-managed input (opt-in: without these calls every slot holds the bytes it held before).  Every file this library writes is tagged
 * sRGB; a source that says something else about its colour is converted to sRGB in its slot, on the device, before it is encoded.
 * A transform (mi_colour_transform) is host state, baked once: three input curves, the 3 x 3 matrix inverse(sRGB colorants, D50) * (source colorants, D50) and the
 * sRGB output curve; relative colorimetric, no black-point compensation, each channel clipped to [0, 1] in linear light.  It may be used by any number of
 * batches, on any device, from any thread, and is released with mi_colour_transform_free (NULL is fine) once no conversion that uses it is still queued (the free
 * waits for the device).
 * mi_colour_transform_from_icc: an ICC v2 / v4 RGB matrix/TRC profile (colour space 'RGB ', PCS 'XYZ ', tags rXYZ gXYZ bXYZ rTRC gTRC bTRC; 'curv' with 0, 1 or n
 * entries, 'para' of types 0..4).  MI_UNSUPPORTED: a well-formed profile of another kind (A2B0 tables, CMYK, grey, Lab PCS, device link, abstract, named colours).
 * MI_ENCODING_ERROR: a malformed one (a size field beyond the data, a tag outside the profile, a table larger than its tag, a truncated header, a missing tag,
 * singular colorants).  The parser never reads outside [icc, icc + len).  An ICC transform is never the identity.
 * mi_colour_transform_from_png: a gAMA value (file_gamma, e.g. 0.45455: the input curve is the pure power 1 / file_gamma) with the eight cHRM values (white x y,
 * red x y, green x y, blue x y; the white point Bradford-adapted to D50) or NULL (sRGB's primaries).  The identity: |file_gamma * 2.2 - 1| < 0.05 without cHRM
 * (libpng's significance threshold), and file_gamma 0 without cHRM (a file with an sRGB chunk or no description).  MI_INVALID_ARGUMENT: a gamma that is
 * negative or not finite; MI_ENCODING_ERROR: degenerate chromaticities.
 * mi_colour_probe_icc / mi_colour_probe_png: the status the two calls above would give for the same arguments and, with MI_OK, whether the transform would be the
 * identity (*is_identity, may be NULL), without baking anything: the profile is parsed and the matrix made, no curve is evaluated.  What a loader asks to learn
 * whether a file can be managed.
 * mi_colour_transform_is_identity: 1 for such a transform, else 0.  mi_colour_transform_table: the baked integers (tests and debugging): which 0 the matrix
 * (9 int64, 30 fractional bits, row-major), 1 lin8 (3 x 256 uint32), 2 U (256 uint32), 3 lin16 (3 x 4098 uint32), 4 out16 (8194 uint16); returns the number of
 * entries and points *data at them (valid while the transform lives), 0 for the identity.  The tables are specified in cavif_rs_amd/csrc/icc_reader.h.
 * mi_png_scanlines_colour: what a parsed PNG says, by the PNG specification's priority: *what 1 an iCCP profile (*icc, *icc_len: inflated, valid while the handle
 * lives), 2 an sRGB chunk, 3 gAMA (*file_gamma; chrm8 gets the cHRM values, or eight zeros when the file has none; a cHRM chunk of eight zeros counts as absent), 0 nothing.
 * A broken colour chunk counts as absent.  mi_png_parse keeps the iCCP chunk as it is in the file; the first call here (or the first managed use of the handle)
 * inflates it, so a file that is never asked about its colour does not pay for its profile.  MI_UNSUPPORTED (with *what 1, *icc NULL): a profile that inflates beyond 4 MiB.  Any pointer but p and what may be NULL.
 * mi_jpeg_coeffs_icc: the profile of a parsed JPEG (APP2 "ICC_PROFILE" segments in any order, joined by sequence number), or *icc NULL, *len 0 when the file has
 * none or its segments do not add up (a missing or duplicate number, disagreeing counts).
 * mi_batch_convert_colour: the colour channels of slots [first, first + count) through the transform, IN PLACE, on the batch's stream (ordered after the uploads
 * that filled them, before the next encode).  The launches are asynchronous; the FIRST conversion of a transform on a device first copies the transform's tables
 * there (one hipMalloc and one blocking 70 KB hipMemcpy, which wait for the device), every later one enqueues and returns.  MI_INPUT_RGB slots are converted in the 8-bit slot array, MI_INPUT_RGB16 slots in the deep one; alpha is
 * never touched and the input kind stays.  The arithmetic is integers only and specified in cavif_rs_amd/csrc/dev_colour.h.  The identity transform is a no-op
 * that launches nothing.  MI_INVALID_ARGUMENT: an MI_INPUT_YCBCR slot in the range, a range past the capacity, a null transform, a call between
 * mi_batch_encode_async and mi_batch_wait; a refused call allocates nothing (mi_batch_footprint). */
typedef struct mi_colour_transform mi_colour_transform;
int  mi_colour_transform_from_icc(const uint8_t *icc, size_t len, mi_colour_transform **out);
int  mi_colour_transform_from_png(double file_gamma, const double *chrm8_or_null, mi_colour_transform **out);
void mi_colour_transform_free(mi_colour_transform *t);
int  mi_colour_probe_icc(const uint8_t *icc, size_t len, int *is_identity);
int  mi_colour_probe_png(double file_gamma, const double *chrm8_or_null, int *is_identity);
int  mi_colour_transform_is_identity(const mi_colour_transform *t);
size_t mi_colour_transform_table(const mi_colour_transform *t, int which, const void **data);
int  mi_png_scanlines_colour(const mi_png_scanlines *p, int *what, const uint8_t **icc, size_t *icc_len, double *file_gamma, double chrm8[8]);
int  mi_jpeg_coeffs_icc(const mi_jpeg_coeffs *c, const uint8_t **icc, size_t *len);
int  mi_batch_convert_colour(mi_batch *b, int first, int count, mi_colour_transform *t);
/* ---- EXIF orientation on input (opt-in: without these calls, MI_SOURCE_ORIENTED or their arguments every slot holds the bytes it held before, and a file's
 * orientation is ignored as it always was).  A camera file stores the sensor's rows and says in EXIF tag 0x0112 how to turn them for display; these calls turn the
 * pixels on the device on their way into the slot, so the file that is written needs no irot / imir.  With S[row][column] a source of sw x sh and D[y][x] the slot:
 *   1  D[y][x] = S[y][x]                 slot sw x sh          5  D[y][x] = S[x][y]                 slot sh x sw
 *   2  D[y][x] = S[y][sw-1-x]            slot sw x sh          6  D[y][x] = S[sh-1-x][y]            slot sh x sw
 *   3  D[y][x] = S[sh-1-y][sw-1-x]       slot sw x sh          7  D[y][x] = S[sh-1-x][sw-1-y]       slot sh x sw
 *   4  D[y][x] = S[sh-1-y][x]            slot sw x sh          8  D[y][x] = S[x][sw-1-y]            slot sh x sw
 * (what Pillow's ImageOps.exif_transpose gives): a permutation of pixels, so the slot's bytes are specified exactly.
 * mi_exif_orientation: the orientation of an Exif blob, with or without a leading "Exif\0\0": TIFF header ("II*\0" or "MM\0*"), IFD0's entries only, tag 0x0112 of
 * type SHORT and count 1 with a value of 1..8; anything else -- no tag, another type or count, 0, 9 and above, a truncated blob, an offset or an entry count that
 * leaves the blob -- is 1.  Always MI_OK for non-null pointers: a file's orientation never makes the picture an error.  Never reads outside [exif, exif + len).
 * mi_jpeg_coeffs_orientation: that of the first APP1 segment of a parsed JPEG that starts with "Exif\0\0"; mi_png_scanlines_orientation: that of the first eXIf chunk
 * of a parsed PNG whose CRC holds (before or after IDAT); 1 when the file says nothing.  mi_oriented_size: width and height change places for 5..8 (either pointer may be NULL).
 * mi_batch_orient_device: mi_batch_upload_device (source description, after_stream, ordering, lifetimes) for pictures of the batch's size (orientations 1..4) or of
 * h x w (5..8), turned by `orientation` (1..8): one launch for all images of the call; 3 channels into an RGBA batch get alpha 255; kind MI_INPUT_RGB.
 * mi_batch_upload_jpeg_oriented: one parsed JPEG into slot `index`, turned by `orientation` (1..8, or 0: the file's own); ycbcr != 0: the file's own (Y, Cb, Cr) as
 * mi_batch_upload_jpeg_ycbcr stores them (kind MI_INPUT_YCBCR, that call's refusals), else mi_batch_upload_jpeg's pixels (kind MI_INPUT_RGB).
 * mi_batch_upload_png_oriented: one parsed PNG likewise; deep != 0: a file of bit depth 16 goes into its deep slot as through mi_batch_upload_png_deep (kind
 * MI_INPUT_RGB16, the alpha rules of deep input), every other file as through mi_batch_upload_png.  A file with an alpha channel or tRNS into a 3-channel batch is refused.
 * The two handle calls decode the file into a device scratch of the batch (grown on demand, shared with the resize calls) and turn it into the slot from there, all on
 * the batch's stream, no sync; the handle may be freed when the call returns.  Orientation 1 -- given, or read from the file -- takes the plain upload call of its kind,
 * gives that call's bytes and touches no scratch.  The slot bytes of every other orientation are the plain call's bytes permuted by the map above.
 * MI_INVALID_ARGUMENT: an orientation outside the call's range, a source whose oriented size is not the batch's, a range past the capacity, null pointers, 4 channels
 * into a 3-channel batch, a refusal of the kind, a call between mi_batch_encode_async and mi_batch_wait; a refused call allocates nothing (mi_batch_footprint).
 * MI_ENCODING_ERROR when staging or scratch cannot be allocated.  Orientation together with resize: the mi_batch_resize_*_oriented calls below.  The YCbCr planes of
 * mi_batch_upload_device_ycbcr and mi_batch_upload_device16 are not built; an Exif blob passed through mi_ravif_encoder's exif field is written as it is and should not still carry an orientation other than 1. */
int  mi_exif_orientation(const uint8_t *exif, size_t len, int *orientation);
int  mi_jpeg_coeffs_orientation(const mi_jpeg_coeffs *c, int *orientation);
int  mi_png_scanlines_orientation(const mi_png_scanlines *p, int *orientation);
void mi_oriented_size(uint32_t w, uint32_t h, int orientation, uint32_t *ow, uint32_t *oh);
int  mi_batch_orient_device(mi_batch *b, int first, int count, const mi_device_pixels *src, int orientation);
int  mi_batch_upload_jpeg_oriented(mi_batch *b, int index, const mi_jpeg_coeffs *c, int orientation, int ycbcr);
int  mi_batch_upload_png_oriented(mi_batch *b, int index, const mi_png_scanlines *p, int orientation, int deep);
/* resize on input: the source has any size and is resampled into the slot on the batch's stream, no sync.  The pixels are exactly those of Pillow's
 * Image.resize((w, h), resample=filter, reducing_gap=None) on 8-bit pictures: coefficients in double on the host, 22-bit fixed-point taps, horizontal pass
 * first into an 8-bit intermediate, then the vertical one, a pass whose axis keeps its length skipped; 4-channel sources are premultiplied before the passes and
 * un-premultiplied after them, 3 channels into an RGBA batch get alpha 255 and no premultiplication.  A source of the batch's own size takes the upload call
 * of its kind above and gives that call's bytes.  The tables go through pinned staging the batch owns (one H2D per call), a decoded JPEG / PNG source and the
 * intermediate live in one device scratch of the batch, grown on demand.
 * mi_batch_resize_device: images [first, first+count) from pictures of src_w x src_h, described and ordered (after_stream) as for mi_batch_upload_device.
 * mi_batch_resize_jpeg / _png: one parsed file into slot `index`; a PNG with an alpha channel or tRNS into a 3-channel batch is MI_INVALID_ARGUMENT.
 * MI_INVALID_ARGUMENT as well: an unknown filter, a zero extent (or one above 65536), strides below the packed row, a range past the capacity, a call between
 * mi_batch_encode_async and mi_batch_wait, 4 channels into a 3-channel batch; MI_ENCODING_ERROR when staging or scratch cannot be allocated.  Lifetimes as for
 * the upload calls: the device source until the next mi_batch_wait, the handles until the call returns. */
enum { MI_RESAMPLE_BOX = 0, MI_RESAMPLE_BILINEAR = 1, MI_RESAMPLE_BICUBIC = 2, MI_RESAMPLE_LANCZOS3 = 3 };
int  mi_batch_resize_device(mi_batch *b, int first, int count, const mi_device_pixels *src, uint32_t src_w, uint32_t src_h, int filter);
int  mi_batch_resize_jpeg(mi_batch *b, int index, const mi_jpeg_coeffs *c, int filter);
int  mi_batch_resize_png(mi_batch *b, int index, const mi_png_scanlines *p, int filter);
/* resize on input of a turned source (opt-in): the source is turned by the map of the orientation calls above and resampled into the slot in one go.
 * With O the source turned by `orientation`, the slot receives exactly the bytes the two existing calls give one after the other -- mi_batch_orient_device (or the
 * _oriented upload) into a slot of O's size, then mi_batch_resize_* from there: the horizontal pass along O's x axis first, into the clipped 8-bit intermediate, then
 * the vertical one.  No turned copy is made: orientations 2..4 are addressing in the horizontal pass, 5..8 filter down the source's columns and transpose a tile in
 * LDS, and the scratch a call needs is that of the plain resize call (device sources: the intermediate; handles: the decoded source and the intermediate).
 * mi_batch_resize_device_oriented: mi_batch_resize_device with an orientation of 1..8; src_w x src_h is the size of the source as it lies in memory.
 * mi_batch_resize_jpeg_oriented / _png_oriented: one parsed file into slot `index`, orientation 1..8, or 0: the file's own.  ycbcr != 0: the file's own (Y, Cb, Cr)
 * triples, as mi_batch_upload_jpeg_ycbcr stores them, are resampled channel by channel (what Pillow gives for a YCbCr mode image) and the slot is tagged
 * MI_INPUT_YCBCR; that call's refusals apply (MI_UNSUPPORTED for a file whose colour is RGB).  A PNG of bit depth 16 is taken through its high bytes, as
 * mi_batch_resize_png takes it; mi_batch_resize_png_deep (below) resamples all 16 bits.
 * Orientation 1, given or read from the file, is the plain mi_batch_resize_* call (with ycbcr: the same two passes over the triples); an oriented source that already
 * has the slot's size is the _oriented upload of its kind (orientation 1 as well: the plain upload).  Neither takes the premultiply round trip.
 * MI_INVALID_ARGUMENT: the refusals of the resize calls and of the orient calls -- an unknown filter, an orientation outside the call's range, a zero extent or one
 * above 65536, strides below the packed row, a range past the capacity or of slots of different sizes, 4 channels into a 3-channel batch, a PNG with alpha or tRNS
 * into a 3-channel batch, null pointers, a call between mi_batch_encode_async and mi_batch_wait, with ycbcr an encoder that does not take YCbCr input.
 * MI_ENCODING_ERROR when staging or scratch cannot be allocated.  Every check comes first: a refused call allocates nothing (mi_batch_footprint).
 * mi_fit_size: the size of a picture of sw x sh scaled down, never up, to fit a box, aspect ratio kept, in exact 64-bit integers.  A box extent of 0 is no bound on
 * that axis.  A picture that fits keeps (sw, sh).  Otherwise, if box_h == 0 or (box_w != 0 and box_w * sh <= box_h * sw): w = box_w, h = max(1, (2 sh box_w + sw) /
 * (2 sw)); else h = box_h, w = max(1, (2 sw box_h + sh) / (2 sh)): the free axis is rounded half up and never exceeds the box.  Either pointer may be NULL. */
int  mi_batch_resize_device_oriented(mi_batch *b, int first, int count, const mi_device_pixels *src, uint32_t src_w, uint32_t src_h, int filter, int orientation);   /* orientation 1..8 */
int  mi_batch_resize_jpeg_oriented(mi_batch *b, int index, const mi_jpeg_coeffs *c, int filter, int orientation, int ycbcr);   /* 0 = the file's own */
int  mi_batch_resize_png_oriented(mi_batch *b, int index, const mi_png_scanlines *p, int filter, int orientation);             /* 0 = the file's own */
void mi_fit_size(uint32_t sw, uint32_t sh, uint32_t box_w, uint32_t box_h, uint32_t *w, uint32_t *h);
/* deep resize (opt-in): a 16-bit source of any size is resampled at 16 bits into the DEEP slot, kind MI_INPUT_RGB16.  The structure is that of the
 * 8-bit calls above, in exact integers:
 *   tables   bounds and normalised double coefficients exactly as above (same filters, same support, same first sample and count per output sample); each tap is
 *            rounded to 28 fractional bits, (int)(v * 2^28 +- 0.5), an int32 (the largest |tap| is about 1.25); an axis that keeps its length has the one tap 2^28.
 *   a pass   out = clamp((2^27 + sum k_j * s_j) >> 28, 0, 65535): a signed 64-bit sum that does not wrap (|sum| < 2^46, any order), an arithmetic shift.
 *   order    the horizontal pass first, along the oriented picture's x axis, into a clipped 16-bit intermediate, then the vertical one; a pass whose axis keeps
 *            its length moves the samples unchanged.
 *   alpha    a 4-channel source is premultiplied on load: t = c * a + 32768 (uint32), p = (t + (t >> 16)) >> 16 = floor((2 c a + 65535) / 131070); after the
 *            vertical pass, for a not 0 and not 65535, c = min(65535, 65535 * c / a) in integer division.  3 channels into a 4-channel batch: A = 65535, no
 *            premultiplication.
 *   samples  a device sample is first reduced to `bits` and widened by bit replication, exactly as mi_batch_upload_device16 does; then premultiplied, then filtered.
 * A source that already has the slot's size takes the plain call of its kind (mi_batch_upload_device16, mi_batch_upload_png_deep, mi_batch_upload_png_oriented(.., 1))
 * and gives that call's bytes: no premultiply round trip.  The alpha rules are those of deep input: a 4-channel source needs alpha_mode 0, alpha_mode 2 takes none
 * into a 4-channel batch, 4 channels into a 3-channel batch are refused.
 * mi_batch_resize_device16: images [first, first+count) from uint16 pictures of src_w x src_h, described and ordered as for mi_batch_upload_device16.  The refusals
 * of that call (an odd pointer or stride, bits outside 8..16, msb_aligned not 0 or 1, strides below the packed extent, the alpha rules) and of mi_batch_resize_device.
 * No orientation: turning mi_batch_upload_device16 sources is not built.
 * mi_batch_resize_png_deep: one parsed PNG into slot `index`, turned by `orientation` (1..8, or 0: the file's own) and resampled.  A file of bit depth 16 that is
 * not palette-coded is expanded as uint16 samples into the batch's scratch and resampled from where it lies (orientations 2..4 are addressing, 5..8 filter down the
 * columns and transpose a tile, as in the 8-bit calls): the slot receives the bytes of mi_batch_upload_png_oriented(.., deep = 1) into a slot of the oriented size
 * followed by the plain deep resize from there.  Every other file goes exactly as mi_batch_resize_png_oriented sends it: its bytes, kind MI_INPUT_RGB.
 * The scratch is the batch's one shared scratch: the decoded source (w * h * channels * 2 bytes) and the intermediate (count * oriented height * dst_w rounded up to
 * 4 * 8 bytes).  MI_INVALID_ARGUMENT: every refusal above, an unknown filter, an orientation outside 0..8, a zero extent or one above 65536, a range past the capacity
 * or of slots of different sizes, null pointers, a call between mi_batch_encode_async and mi_batch_wait.  Every check comes first: a refused call allocates nothing
 * (mi_batch_footprint).  MI_ENCODING_ERROR when the deep slots, staging or scratch cannot be allocated.
 * mi_ravif_encode_device16_resized: mi_ravif_encode_device16 for a picture of src_w x src_h resampled to w x h through mi_batch_resize_device16. */
int  mi_batch_resize_device16(mi_batch *b, int first, int count, const mi_device_pixels16 *src, uint32_t src_w, uint32_t src_h, int filter);
int  mi_batch_resize_png_deep(mi_batch *b, int index, const mi_png_scanlines *p, int filter, int orientation);                 /* 1..8, 0 = the file's own */
int  mi_ravif_encode_device16_resized(const mi_ravif_encoder *e, const mi_device_pixels16 *src, uint32_t src_w, uint32_t src_h, uint32_t w, uint32_t h,
                                      int filter, mi_encoded_image *out);
int  mi_batch_set_count(mi_batch *b, int n_images);                                       /* images of the next run (<= the count the batch was created for), each of the batch's w x h */
/* ---- mixed-size layouts: the pictures of a run differ in size.  A batch is made as before, mi_batch_create(e, cap, W, H, channels); everything it
 * reserves for cap pictures of W x H -- the slot arrays, the arena, tile jobs, payload and pre-carry capacity, symbol records, the search queue's items and snapshots,
 * the alpha flags -- is the room a mixed layout may use.  Pictures are coded independently: every file equals, byte for byte, the file its picture gets alone.
 * mi_batch_set_sizes: lays n_images pictures of widths[i] x heights[i] into that room.  Slot i of the 8-bit slot array (and of the deep one, the pinned staging alike)
 * starts at sample offset sum over k < i of w_k * h_k * channels: rows packed, slots back to back, so a stretch of equal-sized slots is laid out exactly like a uniform
 * batch from its first slot on.  Allocates nothing (mi_batch_footprint is unchanged), launches nothing.  Afterwards the contents of all slots are unspecified, every
 * slot's kind is MI_INPUT_RGB, the records of the last encode are gone, and slots [0, n_images) are the batch's slots: an index past them is a range past the capacity.
 * mi_batch_set_count(b, n) returns the batch to n pictures of W x H (contents unspecified when it follows a mixed layout; after a uniform one as before).
 * Wherever a call's contract above says "the batch's width and height" it means the slot's: the size checks of mi_batch_upload_jpeg* / _png*, the destination of the
 * resize calls, the oriented size of the orient calls, the pictures of mi_batch_decode*, mi_batch_get_recon / _get_source and mi_image_quality.width / height.  The
 * calls that take a range and describe its pictures with one size -- mi_batch_upload_device[16], _upload_device_ycbcr[16], _resize_device, _orient_device and
 * _decode_device -- need all slots of the range to have one size, else MI_INVALID_ARGUMENT; mi_batch_upload_png[_deep] takes one handle per slot, each of its slot's
 * size; mi_batch_upload_async and mi_batch_convert_colour work on any range.
 * Statuses.  MI_INVALID_ARGUMENT: null pointers, n_images < 1, a zero extent or one above 65536, a picture whose padded plane reaches 2^31 samples, and (set_sizes
 * only) a call between mi_batch_encode_async and mi_batch_wait.  MI_UNSUPPORTED: a well-formed layout that does not fit what the batch reserved -- n_images > cap,
 * sum of w * h > cap * W * H, or a dry run of the actual frames exceeding any quantity the reserve sized for its worst case: arena bytes (these go by PADDED pixels:
 * each extent rounded up to 64), tile jobs, the sum of payload capacities, jobs x the largest tile capacity against the pre-carry and record buffers, work items and
 * snapshot bytes; in a 4-channel batch under alpha_mode 1 also a picture of more than W * H pixels (the cleaner's one-image scratch).  MI_OK otherwise: a layout that
 * fits encodes, and a picture larger than W x H is taken when everything reserved suffices (one 4K photograph in a batch made for 32 x 1080p).
 * mi_batch_fits: the status mi_batch_set_sizes would give; touches no device and changes nothing, and may be asked while an encode is in flight.
 * mi_batch_image_size: the current size of slot `index` (W, H in a uniform batch); MI_INVALID_ARGUMENT for null pointers and an index that is no slot. */
int  mi_batch_set_sizes(mi_batch *b, int n_images, const uint32_t *widths, const uint32_t *heights);
int  mi_batch_fits(const mi_batch *b, int n_images, const uint32_t *widths, const uint32_t *heights);
int  mi_batch_image_size(const mi_batch *b, int index, uint32_t *w, uint32_t *h);
int  mi_batch_encode(mi_batch *b);                                                        /* the hot path over all resident images */
/* split form: enqueue the GPU work and return; wait = sync + one packed D2H + OBU/container assembly.  Two batches
 * driven alternately overlap one batch's entropy coding / loop filters with the next batch's tile search. */
int  mi_batch_encode_async(mi_batch *b);
int  mi_batch_wait(mi_batch *b);
int  mi_batch_get(mi_batch *b, int index, mi_encoded_image *out);                         /* copies; caller frees avif_file */
int  mi_batch_get_recon(mi_batch *b, int index, int alpha, uint16_t *planes[3]);          /* malloc'd w*h uint16 planes (tests) */
/* ---- quality metrics of the last completed encode, computed on the device from the planes it left there (opt-in: an encode that is never measured does
 * nothing for them).  Per frame -- the colour frame of an image, its alpha frame when the image uses alpha -- and per plane, over the visible w x h samples,
 * between the uint16 source samples the encoder saw (mi_batch_get_source) and the final reconstruction (mi_batch_get_recon), bd = the batch's bit depth:
 *   sse           sum of (s - r)^2, exact.
 *   ssim_windows  ((w - 8) / 4 + 1) * ((h - 8) / 4 + 1) in integer division, 0 when w < 8 or h < 8: the 8 x 8 windows with their top-left corner at
 *                 (4 i, 4 j) that lie wholly inside the picture.
 *   ssim_sum      the sum over those windows of (long long)floor(q * 2^30 + 0.5).  With the window's integer sums S, R, SS, RR, SR of s, r, s^2, r^2, s r and
 *                 c1 = 26634, c2 = 239708 at 8 bit, c1 = 428658, c2 = 3857925 at 10 bit (4096 (0.01 peak)^2, 4096 (0.03 peak)^2, rounded):
 *                 a = 2 S R + c1, b = 128 SR - 2 S R + c2, c = S S + R R + c1, d = 64 SS - S S + 64 RR - R R + c2 as exact int64, each converted to double
 *                 (exact), q = (a * b) / (c * d): three IEEE double operations, no contraction.  Identical planes give ssim_sum == ssim_windows << 30.
 * Being sums of integers the three numbers do not depend on any order of evaluation; they equal a float64 restatement bit for bit.
 * mi_batch_measure: after mi_batch_wait and before the next encode: zeroes the records (they live in the batch's arena), one kernel launch for all frames
 * and planes, one D2H into pinned memory the batch owns, one sync.  MI_INVALID_ARGUMENT when no encode of the current image count has completed or one is
 * in flight.  mi_batch_get_quality: MI_INVALID_ARGUMENT until a measure of the current encode exists.  mi_batch_get_source: mi_batch_get_recon for the source
 * planes (tests and debugging).  The conversions are host arithmetic and not part of the exactness contract: mi_quality_psnr_db = 10 log10(peak^2 N / sum of
 * sse) over the colour planes (N their samples, peak = 2^bd - 1; +inf when the sum is 0); mi_quality_ssim_db = -10 log10(1 - mean) of plane 0 (Y, or G under
 * the RGB colour model) with mean = ssim_sum / 2^30 / ssim_windows, +inf when mean >= 1, NaN when there is no window. */
typedef struct mi_plane_quality { uint64_t sse; int64_t ssim_sum; uint64_t ssim_windows; } mi_plane_quality;
typedef struct mi_image_quality { uint32_t width, height; uint8_t depth, color_planes, has_alpha, pad_;
                                  mi_plane_quality color[3], alpha; } mi_image_quality;
int  mi_batch_measure(mi_batch *b);
int  mi_batch_get_quality(mi_batch *b, int index, mi_image_quality *out);
int  mi_batch_get_source(mi_batch *b, int index, int alpha, uint16_t *planes[3]);
double mi_quality_psnr_db(const mi_image_quality *q);
double mi_quality_ssim_db(const mi_image_quality *q);
/* ---- decoded pixels of the last completed encode: the final reconstruction (MI_DECODED_RECON, the planes of mi_batch_get_recon) or the source planes
 * (MI_DECODED_SOURCE, those of mi_batch_get_source) as 8-bit RGB or RGBA, made on the device by one kernel launch per call (opt-in: an encode that never asks
 * allocates and launches nothing for it).  The pixels are specified exactly.  bd = the batch's bit depth, peak = 2^bd - 1, half = 2^(bd-1),
 * p0 p1 p2 the colour frame's samples at (x, y), a plane 0 of the image's alpha frame there, and for exact integers n, d > 0
 *   q(n, d) = clamp(floor((2 * 255 * n + d * peak) / (2 * d * peak)), 0, 255)          (0 whenever the numerator is negative):
 *   YCbCr model:  cb = p1 - half, cr = p2 - half;  R = q(1000 p0 + 1402 cr, 1000),  G = q(587000 p0 - 202008 cb - 419198 cr, 587000),
 *                 B = q(1000 p0 + 1772 cb, 1000)          (matrix 6, full range: the exact BT.601 inverse)
 *   RGB model:    G = q(p0, 1), B = q(p1, 1), R = q(p2, 1)
 *   alpha:        A = q(a, 1) when the image uses alpha (mi_batch_uses_alpha), else 255.
 * There is no alpha association step: with the premultiplied alpha mode the output holds the stored (premultiplied) colours, with the clean mode the cleaned
 * ones.  Only the visible w x h pixels are read and written; bytes of the destination that its layout does not address are left alone.
 * All three calls are valid after mi_batch_wait and before the next encode or mi_batch_set_count (the state rule of mi_batch_measure), else
 * MI_INVALID_ARGUMENT.  mi_batch_decode_device: images [first, first + count) into memory of the batch's own device (documented, not detected), image k at
 * dev + k * image_stride, strides under mi_device_pixels' rules (0 = packed) and, being written, an interleaved row stride of at least (w - 1) * pixel stride +
 * channels; beyond that, that rows, planes and images of the destination do not overlap one another is the caller's promise (not detected); the launch is ordered after the work dst->after_stream holds at the time of the
 * call, the batch's stream is waited for, and the pixels are in place when the call returns.  mi_batch_decode: one image into host memory (w * h * channels
 * bytes, rows packed) through a one-image device scratch the batch makes on first use; the input slot is never touched.  MI_INVALID_ARGUMENT as well: null
 * pointers, a range outside the images of the run or an empty one, `which` not 0 or 1, channels not 3 or 4, a layout not 0 or 1, strides below the packed
 * extent, and 3 channels when any image of the range uses alpha (alpha is never dropped).  4 channels for an opaque image or a 3-channel batch give A = 255. */
enum { MI_DECODED_RECON = 0, MI_DECODED_SOURCE = 1 };
typedef struct mi_device_target {          /* mi_device_pixels with a writable pointer; same stride rules, 0 = packed */
  void *dev;
  int layout;        /* 0 = HWC, 1 = CHW */
  int channels;      /* 3 | 4 */
  size_t row_stride, pixel_or_plane_stride, image_stride;   /* bytes; 0 = packed */
  void *after_stream; /* hipStream_t whose queued work must finish before dst is written, or NULL */
} mi_device_target;
int  mi_batch_uses_alpha(mi_batch *b, int index, int *uses_alpha);
int  mi_batch_decode_device(mi_batch *b, int first, int count, int which, const mi_device_target *dst);
int  mi_batch_decode(mi_batch *b, int index, int which, int channels, uint8_t *dst);
/* ---- full-depth tensors: binary16 / binary32 sources into the deep slots, and decoded pixels as uint16, binary16 or binary32 samples.  Opt-in:
 * a batch that never asks allocates and launches nothing for it.  Everything is exact; a restatement in float64 and integers gives the same bits.
 * FLOAT SOURCE TO DEEP SLOT SAMPLE W.  v = the source sample; a binary16 sample is converted to binary32 exactly (subnormal halves are values, not zero).
 * full_scale = the binary32 value that means white, finite and > 0 (1.0 for normalised tensors, 255.0 for byte-valued floats).  In this order:
 *   v is NaN                                  W = 0
 *   v <= 0          (-0.0, -inf)              W = 0
 *   v >= full_scale (+inf)                    W = 65535
 *   otherwise       u = ((double)v * 65535.0) / (double)full_scale,  W = (uint16)rint(u), round half to even.
 * The product is exact in binary64 (24 by 16 bits) and the division its one rounding (none when full_scale is 1).  3 channels into a 4-channel batch get
 * A = 65535; a float alpha sample goes through the same map.  The slot is of kind MI_INPUT_RGB16 and is coded by the formulas of deep input above.
 * DEEP DECODED SAMPLE D.  mi_batch_decode's formulas with 65535 in the place of 255: for exact integers n, d > 0
 *   q16(n, d) = clamp(floor((2 * 65535 * n + d * peak) / (2 * d * peak)), 0, 65535)          (0 whenever the numerator is negative)
 * with the same n and d per channel and colour model (R = q16(1000 p0 + 1402 cr, 1000), G = q16(587000 p0 - 202008 cb - 419198 cr, 587000),
 * B = q16(1000 p0 + 1772 cb, 1000); or G, B, R = q16(p, 1)); A = q16(a, 1) when the image uses alpha, else 65535.  No alpha association step, as at 8 bits.
 * TARGET SAMPLE.  MI_SAMPLE_U16: D.  MI_SAMPLE_F32: (float)(((double)D * (double)full_scale) / 65535.0) -- an exact product, one binary64 division, one
 * conversion to binary32 that rounds to nearest even.  MI_SAMPLE_F16: that binary32 value converted to binary16, round to nearest even.
 * mi_batch_upload_device_float: mi_batch_upload_device16 (after_stream, ordering, lifetimes, the one-size rule, stride rules in BYTES, the alpha rules of deep
 * input) for float samples; the slots are tagged MI_INPUT_RGB16; one launch for all images of the call.  MI_INVALID_ARGUMENT: what mi_batch_upload_device16
 * refuses, an unknown `sample`, a full_scale that is not finite or not > 0, a pointer or stride that is no multiple of the sample size, a call between
 * mi_batch_encode_async and mi_batch_wait -- all checked before the deep slots are made: a refused call allocates nothing (mi_batch_footprint).
 * mi_ravif_encode_device_float: mi_ravif_encode_device16 for such a source.  Blocking, pooled.
 * mi_batch_decode_device_deep: mi_batch_decode_device (state rule, one-size rule, alpha never dropped, stride rules, synchronisation) with the packed extents
 * counted in the sample's size; the pointer and every stride are multiples of it; full_scale is read for float samples only.  mi_batch_decode_deep: one image
 * into host memory (w * h * channels samples, rows packed) through the scratch of mi_batch_decode, grown to the sample size asked for. */
enum { MI_SAMPLE_U16 = 1, MI_SAMPLE_F16 = 2, MI_SAMPLE_F32 = 3 };
typedef struct mi_device_pixels_float {    /* mi_device_pixels for binary16 / binary32 samples */
  const void *dev;
  int layout;        /* 0 = HWC, 1 = CHW */
  int channels;      /* 3 | 4 */
  size_t row_stride, pixel_or_plane_stride, image_stride;   /* bytes, multiples of the sample size; 0 = packed */
  void *after_stream; /* hipStream_t the pixels were produced on, or NULL = already complete */
  int sample;        /* MI_SAMPLE_F16 | MI_SAMPLE_F32 */
  float full_scale;  /* the value that means white: finite, > 0 */
} mi_device_pixels_float;
typedef struct mi_device_target_deep {     /* mi_device_target for uint16 / binary16 / binary32 samples */
  void *dev;
  int layout;        /* 0 = HWC, 1 = CHW */
  int channels;      /* 3 | 4 */
  size_t row_stride, pixel_or_plane_stride, image_stride;   /* bytes, multiples of the sample size; 0 = packed */
  void *after_stream; /* hipStream_t whose queued work must finish before dst is written, or NULL */
  int sample;        /* MI_SAMPLE_U16 | MI_SAMPLE_F16 | MI_SAMPLE_F32 */
  float full_scale;  /* floats only: the value white is written as */
} mi_device_target_deep;
int  mi_batch_upload_device_float(mi_batch *b, int first, int count, const mi_device_pixels_float *src);
int  mi_ravif_encode_device_float(const mi_ravif_encoder *e, const mi_device_pixels_float *src, uint32_t w, uint32_t h, mi_encoded_image *out);
int  mi_batch_decode_device_deep(mi_batch *b, int first, int count, int which, const mi_device_target_deep *dst);
int  mi_batch_decode_deep(mi_batch *b, int index, int which, int channels, int sample, float full_scale, void *dst);
/* per-kernel HIP-event time (ms) of the last mi_batch_encode: 0 front-end, 1 tile search, 2 deblock, 3 cdef, 4 entropy, 5 pack+D2H, 6 host assembly */
double mi_batch_stage_ms(const mi_batch *b, int stage);
int  mi_batch_num_tiles(const mi_batch *b);
/* profiling aid: per tile [K1 start, K1 end, K4 start, K4 end] in wall_clock64 ticks (100 MHz) of the last encode */
int  mi_batch_tile_clocks(mi_batch *b, unsigned long long *out);
void mi_batch_destroy(mi_batch *b);

/* AVIF container (avif-serialize Aviffy::to_vec, call site ravif/src/av1encoder.rs:457-473) */
size_t mi_avif_serialize(const uint8_t *color, size_t color_len, const uint8_t *alpha, size_t alpha_len,
                         uint32_t w, uint32_t h, uint8_t depth, uint8_t matrix, int premultiplied,
                         const uint8_t *exif, size_t exif_len, uint8_t **out);
int  mi_device_count(void);
void mi_free(void *p);
const char *mi_version(void);

#ifdef __cplusplus
}
#endif
#endif
