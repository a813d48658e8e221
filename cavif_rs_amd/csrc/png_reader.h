// png_reader.h -- PNG -> RGBA8, the input side of the cavif CLI (reference: load_rgba, src/main.rs:265-283, which maps
// every load_image pixel kind to RGBA8: RGB -> alpha 255, 16-bit -> high byte, gray -> r=g=b).
// Host C++ over zlib's inflate; written from the PNG specification (chunks IHDR / PLTE / tRNS / IDAT / IEND, the five
// scanline filters, Adam7).  The colour chunks before IDAT (iCCP, sRGB, gAMA, cHRM) are kept beside the scanlines for colour-managed input and
// change neither the pixels nor the status of any file; so is the orientation of the eXIf chunk (exif_reader.h).  JPEG bytes get MI_UNSUPPORTED here: the reference's other input format has its own reader
// (jpeg_reader.h + dev_jpeg.h), and mi_image_decode_rgba picks between the two.
#pragma once
#include <algorithm>
#include <zlib.h>
#include <cstdint>
#include <cstring>
#include <vector>
#include "exif_reader.h"

namespace mi {

inline uint32_t png_be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// un-filters `rows` scanlines of `rowbytes` bytes (each preceded by its filter byte) in place; bpp = bytes per complete pixel (>= 1)
inline bool png_unfilter(uint8_t *data, size_t rows, size_t rowbytes, int bpp) {
  std::vector<uint8_t> zero(rowbytes, 0);
  const uint8_t *prev = zero.data();
  for (size_t y = 0; y < rows; y++) {
    uint8_t *line = data + y * (rowbytes + 1);
    const int ft = line[0];
    uint8_t *cur = line + 1;
    for (size_t i = 0; i < rowbytes; i++) {
      const int a = i >= (size_t)bpp ? cur[i - bpp] : 0, b = prev[i], c = i >= (size_t)bpp ? prev[i - bpp] : 0;
      int add;
      switch (ft) {
        case 0: add = 0; break;
        case 1: add = a; break;
        case 2: add = b; break;
        case 3: add = (a + b) >> 1; break;
        case 4: { const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
                  add = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); break; }
        default: return false;
      }
      cur[i] = (uint8_t)(cur[i] + add);
    }
    prev = cur;
  }
  return true;
}

// One file after inflate: the filtered scanlines (filter byte + filtered bytes per row, pass after pass for Adam7) and what it takes to turn them into
// pixels.  The host reader below goes on from here with png_unfilter + png_expand_rgba; the device path (dev_png.h, mi_batch_upload_png) uploads `raw`.
struct PngPass { size_t off; uint32_t rows, rowbytes, pw, x0, y0, dx, dy; };      // off: of the pass's first filter byte in raw; rows x (1 + rowbytes) bytes
struct PngScanlines {
  uint32_t w = 0, h = 0;
  int depth = 0, ctype = 0, interlace = 0, channels = 0, bits_pp = 0, bpp = 0;   // bpp: bytes per complete pixel (>= 1), the filters' distance
  uint32_t palette[256];                                                          // r | g << 8 | b << 16 | a << 24 with tRNS folded in; entries beyond PLTE are opaque black
  bool has_key = false, has_trns = false; uint16_t key[3] = { 0, 0, 0 };          // tRNS colour key of gray (key[0]) and truecolour files, compared on all 16 bits
  int npass = 0; PngPass pass[7];                                                 // the passes that have pixels, in stream order
  std::vector<uint8_t> raw;
  // what the file says about its colour (the chunks before IDAT), by the PNG specification's priority: 1 iCCP (icc, or icc_oversize when it inflates beyond
  // PNG_ICC_MAX), 2 sRGB, 3 gAMA (file_gamma, with cHRM's white x y, red x y, green x y, blue x y when has_chrm; a cHRM chunk of eight zeros counts as absent),
  // 0 none.  Nothing in the pixel path reads it.  The reader keeps the first iCCP chunk's body as it is in the file (iccp_body); `colour` and `icc` are valid
  // after png_resolve_colour, which inflates it: a file that is never asked about its colour never pays for that.
  int colour = 0; std::vector<uint8_t> icc; bool icc_oversize = false; double file_gamma = 0.0; bool has_chrm = false; double chrm[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
  std::vector<uint8_t> iccp_body; bool has_srgb = false, colour_resolved = false;
  int orientation = 1;                                                            // what the file's eXIf chunk says (exif_reader.h), 1 = nothing; nothing in the pixel path reads it
  bool has_alpha() const { return ctype == 4 || ctype == 6 || has_trns; }
};

constexpr size_t PNG_ICC_MAX = (size_t)4 << 20;
// the body of an iCCP chunk (name, 0, compression method 0, zlib stream) -> the profile; false = broken (the chunk then counts as absent); *oversize = inflates beyond PNG_ICC_MAX
inline bool png_inflate_iccp(const uint8_t *body, size_t n, std::vector<uint8_t> &icc, bool *oversize) {
  *oversize = false;
  size_t k = 0;
  while (k < n && k < 80 && body[k]) k++;
  if (k == 0 || k >= 80 || k + 2 > n || body[k] != 0 || body[k + 1] != 0) return false;
  const uint8_t *z = body + k + 2; const size_t zn = n - k - 2;
  if (zn == 0 || zn > 0xFFFFFFFFu) return false;
  z_stream zs; memset(&zs, 0, sizeof(zs));
  if (inflateInit(&zs) != Z_OK) return false;
  zs.next_in = const_cast<uint8_t *>(z); zs.avail_in = (uInt)zn;
  icc.clear();
  uint8_t buf[16384]; int zr = Z_OK;
  while (zr == Z_OK) {
    zs.next_out = buf; zs.avail_out = sizeof(buf);
    zr = inflate(&zs, Z_NO_FLUSH);
    if (zr != Z_OK && zr != Z_STREAM_END) break;
    icc.insert(icc.end(), buf, buf + (sizeof(buf) - zs.avail_out));
    if (icc.size() > PNG_ICC_MAX) { inflateEnd(&zs); icc.clear(); *oversize = true; return true; }
    if (zr == Z_OK && zs.avail_in == 0 && zs.avail_out != 0) break;      // the stream ends before its end marker
  }
  inflateEnd(&zs);
  if (zr != Z_STREAM_END || icc.empty()) { icc.clear(); return false; }
  return true;
}

// the file's colour description by priority (PngScanlines::colour): inflates the kept iCCP body once; a broken profile chunk counts as absent.  Not thread-safe:
// whoever shares a PngScanlines between threads calls it under a lock (mi_png_scanlines does)
inline void png_resolve_colour(PngScanlines &sl) {
  if (sl.colour_resolved) return;
  const bool have_icc = !sl.iccp_body.empty() && png_inflate_iccp(sl.iccp_body.data(), sl.iccp_body.size(), sl.icc, &sl.icc_oversize);
  std::vector<uint8_t>().swap(sl.iccp_body);
  sl.colour = have_icc ? 1 : sl.has_srgb ? 2 : sl.file_gamma > 0.0 ? 3 : 0;
  sl.colour_resolved = true;
}

// Chunk walk, IHDR / PLTE / tRNS checks, size guard and inflate; every filter byte is checked (> 4 is an error), and so is every palette index when
// PLTE is shorter than the index range -- for that the scanlines are unfiltered here and handed on as a filter-0 stream.
// Returns 0 on success, 2 (MI_UNSUPPORTED) for non-PNG / unsupported data, 3 (MI_ENCODING_ERROR) for corrupt streams.
inline int png_read_scanlines(const uint8_t *d, size_t len, PngScanlines &sl) {
  static const uint8_t sig[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
  if (len < 8 + 25 || memcmp(d, sig, 8) != 0) return 2;
  size_t pos = 8;
  uint32_t w = 0, h = 0;
  int depth = 0, ctype = 0, interlace = 0; bool have_ihdr = false, have_exif = false;
  std::vector<uint8_t> idat, plte, trns;
  while (pos + 12 <= len) {
    const uint32_t n = png_be32(d + pos); const uint8_t *type = d + pos + 4, *body = d + pos + 8;
    if (n > len || pos + 12 + (size_t)n > len) return 3;
    if (!memcmp(type, "IHDR", 4)) {
      if (n != 13) return 3;
      w = png_be32(body); h = png_be32(body + 4); depth = body[8]; ctype = body[9]; interlace = body[12];
      sl.w = w; sl.h = h;
      if (body[10] != 0 || body[11] != 0 || interlace > 1 || w == 0 || h == 0 || w > (1u << 16) || h > (1u << 16)) return 2;
      have_ihdr = true;
    } else if (!memcmp(type, "PLTE", 4)) plte.assign(body, body + n);
    else if (!memcmp(type, "tRNS", 4)) trns.assign(body, body + n);
    else if (!memcmp(type, "IDAT", 4)) idat.insert(idat.end(), body, body + n);
    else if (!memcmp(type, "IEND", 4)) break;
    else if (!memcmp(type, "eXIf", 4)) {                       // allowed before and after IDAT; the first one whose CRC holds counts, a broken one counts as absent
      if (have_ihdr && !have_exif && png_be32(body + n) == (uint32_t)crc32_z(0, type, 4 + (size_t)n)) { have_exif = true; sl.orientation = exif_orientation(body, n); }
    } else if (idat.empty()) {                                  // the colour chunks come before IDAT; a broken one counts as absent and never as an error of the picture
      if (!memcmp(type, "iCCP", 4)) { if (sl.iccp_body.empty()) sl.iccp_body.assign(body, body + n); }
      else if (!memcmp(type, "sRGB", 4)) sl.has_srgb = sl.has_srgb || n == 1;
      else if (!memcmp(type, "gAMA", 4)) { if (n == 4 && png_be32(body) != 0) sl.file_gamma = (double)png_be32(body) / 100000.0; }
      else if (!memcmp(type, "cHRM", 4)) { if (n == 32) { for (int i = 0; i < 8; i++) { sl.chrm[i] = (double)png_be32(body + 4 * i) / 100000.0; sl.has_chrm = sl.has_chrm || sl.chrm[i] != 0.0; } } }
    }
    pos += 12 + (size_t)n;
  }
  if (!have_ihdr || idat.empty()) return 3;
  const int channels = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
  if (!channels) return 2;
  if (!(depth == 8 || depth == 16 || ((ctype == 0 || ctype == 3) && (depth == 1 || depth == 2 || depth == 4))) || (ctype == 3 && depth == 16)) return 2;
  if (ctype == 3 && plte.size() < 3) return 3;
  const int bits_pp = channels * depth, bpp = bits_pp >= 8 ? bits_pp / 8 : 1;
  sl.w = w; sl.h = h; sl.depth = depth; sl.ctype = ctype; sl.interlace = interlace; sl.channels = channels; sl.bits_pp = bits_pp; sl.bpp = bpp;
  // pass geometry: one pass for non-interlaced, seven for Adam7
  struct Pass { uint32_t x0, y0, dx, dy; };
  static const Pass adam7[7] = { { 0, 0, 8, 8 }, { 4, 0, 8, 8 }, { 0, 4, 4, 8 }, { 2, 0, 4, 4 }, { 0, 2, 2, 4 }, { 1, 0, 2, 2 }, { 0, 1, 1, 2 } };
  const Pass whole = { 0, 0, 1, 1 };
  size_t total = 0;
  sl.npass = 0;
  for (int p = 0; p < (interlace ? 7 : 1); p++) {
    const Pass &ps = interlace ? adam7[p] : whole;
    if (w <= ps.x0 || h <= ps.y0) continue;
    const uint32_t pw = (w - ps.x0 + ps.dx - 1) / ps.dx, ph = (h - ps.y0 + ps.dy - 1) / ps.dy;
    if (!pw || !ph) continue;
    const size_t rowbytes = ((size_t)pw * bits_pp + 7) / 8;
    sl.pass[sl.npass++] = PngPass{ total, ph, (uint32_t)rowbytes, pw, ps.x0, ps.y0, ps.dx, ps.dy };
    total += (size_t)ph * (1 + rowbytes);
  }
  // a deflate stream expands at most ~1032x: a tiny file that claims a huge canvas is refused before anything is allocated
  if (total > idat.size() * 1040 + 65536) return 3;
  std::vector<uint8_t> &raw = sl.raw;
  raw.assign(total, 0);
  {
    z_stream zs; memset(&zs, 0, sizeof(zs));
    if (inflateInit(&zs) != Z_OK) return 3;
    // zlib counts in uInt: feed and drain in chunks so that streams and canvases beyond 4 GiB work
    size_t in_pos = 0, out_pos = 0; int zr = Z_OK;
    const size_t chunk = (size_t)1 << 30;
    while (zr == Z_OK || zr == Z_BUF_ERROR) {
      if (zs.avail_in == 0 && in_pos < idat.size()) { const size_t k = std::min(chunk, idat.size() - in_pos); zs.next_in = idat.data() + in_pos; zs.avail_in = (uInt)k; in_pos += k; }
      if (zs.avail_out == 0 && out_pos < total) { const size_t k = std::min(chunk, total - out_pos); zs.next_out = raw.data() + out_pos; zs.avail_out = (uInt)k; out_pos += k; }
      const uInt in_before = zs.avail_in, out_before = zs.avail_out;
      zr = inflate(&zs, Z_NO_FLUSH);
      if (zr == Z_BUF_ERROR && in_before == zs.avail_in && out_before == zs.avail_out && (in_pos >= idat.size() || out_pos >= total)) break;   // no progress possible
    }
    const size_t got = out_pos - zs.avail_out;
    inflateEnd(&zs);
    if ((zr != Z_STREAM_END && zr != Z_OK && zr != Z_BUF_ERROR) || got != total) return 3;
  }
  // the filter bytes sit at known offsets
  for (int p = 0; p < sl.npass; p++) {
    const PngPass &ps = sl.pass[p];
    for (uint32_t y = 0; y < ps.rows; y++) if (raw[ps.off + (size_t)y * (ps.rowbytes + 1)] > 4) return 3;
  }
  // palette (tRNS folded in) and colour key
  for (int i = 0; i < 256; i++) sl.palette[i] = 0xFF000000u;
  sl.has_key = sl.has_trns = false; sl.key[0] = sl.key[1] = sl.key[2] = 0;
  if (ctype == 3) {
    const size_t entries = std::min<size_t>(plte.size() / 3, 256);
    for (size_t i = 0; i < entries; i++)
      sl.palette[i] = (uint32_t)plte[i * 3] | ((uint32_t)plte[i * 3 + 1] << 8) | ((uint32_t)plte[i * 3 + 2] << 16) | ((uint32_t)(i < trns.size() ? trns[i] : 255) << 24);
    sl.has_trns = !trns.empty();
    if (entries < ((size_t)1 << depth)) {                      // rare: an index may point beyond PLTE, which only the unfiltered stream can tell
      for (int p = 0; p < sl.npass; p++) {
        const PngPass &ps = sl.pass[p];
        if (!png_unfilter(raw.data() + ps.off, ps.rows, ps.rowbytes, bpp)) return 3;
        const int mx = (1 << depth) - 1;
        for (uint32_t y = 0; y < ps.rows; y++) {
          uint8_t *line = raw.data() + ps.off + (size_t)y * (ps.rowbytes + 1);
          line[0] = 0;
          for (uint32_t xx = 0; xx < ps.pw; xx++) {
            const size_t bit = (size_t)xx * depth;
            const size_t idx = depth == 8 ? line[1 + (bit >> 3)] : (size_t)((line[1 + (bit >> 3)] >> (8 - depth - (bit & 7))) & mx);
            if (idx >= entries) return 3;
          }
        }
      }
    }
  } else if (ctype == 0 && trns.size() >= 2) { sl.has_key = sl.has_trns = true; sl.key[0] = (uint16_t)((trns[0] << 8) | trns[1]); }
  else if (ctype == 2 && trns.size() >= 6) { sl.has_key = sl.has_trns = true; for (int c = 0; c < 3; c++) sl.key[c] = (uint16_t)((trns[2 * c] << 8) | trns[2 * c + 1]); }
  return 0;
}

// unfiltered scanlines -> RGBA8 (w * h * 4 bytes)
inline void png_expand_rgba(const PngScanlines &sl, uint8_t *rgba) {
  const int depth = sl.depth, ctype = sl.ctype, channels = sl.channels;
  const int mx = (1 << (depth > 8 ? 8 : depth)) - 1;
  for (int p = 0; p < sl.npass; p++) {
    const PngPass &ps = sl.pass[p];
    for (uint32_t yy = 0; yy < ps.rows; yy++) {
      const uint8_t *row = sl.raw.data() + ps.off + (size_t)yy * (ps.rowbytes + 1) + 1;
      for (uint32_t xx = 0; xx < ps.pw; xx++) {
        // sample fetch: `depth`-bit big-endian samples, MSB first inside a byte; 16-bit samples keep their high byte
        // (px.map(|c| (c >> 8) as u8), src/main.rs:272-273), sub-byte gray is scaled to 0..255
        int s[4] = { 0, 0, 0, 0 }; int key16[4] = { 0, 0, 0, 0 };
        for (int c = 0; c < channels; c++) {
          const size_t bit = ((size_t)xx * channels + c) * depth;
          if (depth == 8) s[c] = row[bit >> 3];
          else if (depth == 16) { s[c] = row[bit >> 3]; key16[c] = (row[bit >> 3] << 8) | row[(bit >> 3) + 1]; }
          else s[c] = (row[bit >> 3] >> (8 - depth - (bit & 7))) & mx;
        }
        uint8_t r, g, b, a = 255;
        if (ctype == 3) {
          const uint32_t e = sl.palette[s[0]];
          r = (uint8_t)e; g = (uint8_t)(e >> 8); b = (uint8_t)(e >> 16); a = (uint8_t)(e >> 24);
        } else if (ctype == 0 || ctype == 4) {
          const int v = depth < 8 ? s[0] * 255 / mx : s[0];
          r = g = b = (uint8_t)v;
          if (ctype == 4) a = (uint8_t)s[1];
          else if (sl.has_key && (depth == 16 ? key16[0] : s[0]) == sl.key[0]) a = 0;
        } else {
          r = (uint8_t)s[0]; g = (uint8_t)s[1]; b = (uint8_t)s[2];
          if (ctype == 6) a = (uint8_t)s[3];
          else if (sl.has_key) {
            bool eq = true;
            for (int c = 0; c < 3; c++) eq = eq && ((depth == 16 ? key16[c] : s[c]) == sl.key[c]);
            if (eq) a = 0;
          }
        }
        uint8_t *o = rgba + (((size_t)ps.y0 + (size_t)yy * ps.dy) * sl.w + ps.x0 + (size_t)xx * ps.dx) * 4;
        o[0] = r; o[1] = g; o[2] = b; o[3] = a;
      }
    }
  }
}

// Returns 0 on success, 2 (MI_UNSUPPORTED) for non-PNG / unsupported data, 3 (MI_ENCODING_ERROR) for corrupt streams.
inline int png_decode_rgba(const uint8_t *d, size_t len, std::vector<uint8_t> &rgba, uint32_t &w, uint32_t &h) {
  PngScanlines sl;
  if (const int st = png_read_scanlines(d, len, sl)) { w = sl.w; h = sl.h; return st; }
  w = sl.w; h = sl.h;
  for (int p = 0; p < sl.npass; p++) if (!png_unfilter(sl.raw.data() + sl.pass[p].off, sl.pass[p].rows, sl.pass[p].rowbytes, sl.bpp)) return 3;
  rgba.assign((size_t)w * h * 4, 0);
  png_expand_rgba(sl, rgba.data());
  return 0;
}

}  // namespace mi
