// jpeg_reader.h -- JPEG -> quantised DCT coefficients, the host half of the JPEG input side of the cavif CLI (reference: load_image::load_data,
// src/main.rs:258, which accepts JPEG next to PNG).  Only the strictly serial part lives here: marker parsing and Huffman decoding (baseline / extended
// sequential, and progressive with spectral selection + successive approximation).  No pixel arithmetic: dequantisation, the inverse DCT, chroma
// upsampling and the colour transform are the kernels of dev_jpeg.h.  Written from ITU-T T.81 (markers: annex B; Huffman tables: annex C; sequential
// decoding: annex F.2; progressive: annex G.2) and the JFIF / Adobe APP14 conventions; the APP2 segments of an embedded ICC profile (ICC.1 annex B.4) are
// joined and kept for colour-managed input, the orientation of the first APP1 Exif segment (exif_reader.h) for the oriented uploads (5i); both
// change neither the coefficients nor the status of any file.
// Stricter than libjpeg where that is simpler: a stream that ends before every block of every scan is decoded, a file without EOI, a component no scan
// covered and a progressive file whose scans leave a coefficient short of full precision are MI_ENCODING_ERROR -- nothing partial is ever decoded.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "exif_reader.h"

namespace mi {

struct JpegComp {
  int id = 0, h = 1, v = 1, tq = 0;
  uint32_t cw = 0, ch = 0;          // samples that carry picture: ceil(w * h / hmax) x ceil(h * v / vmax)
  uint32_t bw = 0, bh = 0;          // MCU-padded block grid
  size_t first_block = 0;           // of this component in JpegCoeffs::coef (blocks of 64)
  uint16_t quant[64];               // natural order, latched at the component's first scan
  bool have_quant = false;
};

enum { JPEG_GREY = 0, JPEG_YCBCR = 1, JPEG_RGB = 2 };

struct JpegCoeffs {
  uint32_t w = 0, h = 0;
  int ncomp = 0, hmax = 1, vmax = 1, color = JPEG_GREY;
  JpegComp comp[3];
  size_t nblocks = 0;
  std::vector<int16_t> coef;        // nblocks x 64, natural (de-zigzagged) order, component after component, row-major over each block grid
  std::vector<uint8_t> icc;         // the embedded ICC profile (APP2 "ICC_PROFILE\0" segments joined by sequence number), empty = none
  int orientation = 1;              // what the first APP1 "Exif\0\0" segment says (exif_reader.h), 1 = nothing: kept for the oriented uploads, no pixel depends on it
};

// APP2 "ICC_PROFILE\0" + sequence number (1..count) + count + bytes: the segments of one file in any order.  finish() joins them; a missing or duplicate
// number, a zero or disagreeing count mean that the file has no profile.  Never an error of the picture.
struct JpegIccParts {
  struct Part { int seq; const uint8_t *data; size_t len; };
  std::vector<Part> parts; int count = 0; bool broken = false;
  void add(const uint8_t *seg, size_t n) {
    if (n < 14 || memcmp(seg, "ICC_PROFILE\0", 12) != 0) return;
    const int seq = seg[12], cnt = seg[13];
    if (seq == 0 || cnt == 0 || seq > cnt || (count && cnt != count)) { broken = true; return; }
    count = cnt;
    for (const Part &p : parts) if (p.seq == seq) { broken = true; return; }
    parts.push_back(Part{ seq, seg + 14, n - 14 });
  }
  void finish(std::vector<uint8_t> &icc) const {
    icc.clear();
    if (broken || !count || (int)parts.size() != count) return;
    for (int s = 1; s <= count; s++) for (const Part &p : parts) if (p.seq == s) icc.insert(icc.end(), p.data, p.data + p.len);
  }
};

static const uint8_t jpeg_zigzag[64] = { 0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                         35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };

// canonical Huffman table (T.81 annex C) with a 9-bit first-level lookup; longer codes walk maxcode[], at most 16 steps
struct JpegHuff {
  bool defined = false;
  uint8_t vals[256];
  uint16_t fast[512];               // (length << 8) | symbol, 0 = longer than 9 bits or no such code
  int32_t maxcode[18];              // largest code of each length, -1 = none
  int32_t valptr[17], mincode[17];
  bool build(const uint8_t counts[16], const uint8_t *symbols, int nsym) {
    int code = 0, k = 0;
    memset(fast, 0, sizeof(fast));
    memcpy(vals, symbols, (size_t)nsym);
    for (int l = 1; l <= 16; l++) {
      valptr[l] = k; mincode[l] = code;
      for (int i = 0; i < counts[l - 1]; i++, k++, code++) {
        if (code >= (1 << l)) return false;                      // more codes of this length than bits allow
        if (l <= 9) for (int f = 0; f < (1 << (9 - l)); f++) fast[(code << (9 - l)) | f] = (uint16_t)((l << 8) | symbols[k]);
      }
      maxcode[l] = counts[l - 1] ? code - 1 : -1;
      code <<= 1;
    }
    maxcode[17] = 0x7fffffff;
    defined = true;
    return true;
  }
};

// entropy-coded segment reader: removes FF00 stuffing, never reads past a marker or the end of the data.  A request for more bits than the segment
// holds sets `bad` and yields zeros; callers test `bad` once per block, so the work after a failure is bounded by one block.
struct JpegBits {
  const uint8_t *d; size_t pos, len;
  uint64_t acc = 0; int n = 0; bool bad = false;
  JpegBits(const uint8_t *d_, size_t pos_, size_t len_) : d(d_), pos(pos_), len(len_) {}
  void fill() {
    while (n <= 56 && pos < len) {
      const uint8_t b = d[pos];
      if (b == 0xFF) {
        if (pos + 1 >= len || d[pos + 1] != 0) return;           // a marker (or a cut): the segment ends here
        pos += 2;
      } else pos++;
      acc = (acc << 8) | b; n += 8;
    }
  }
  uint32_t peek16() {                                            // the next 16 bits, zero-padded behind the segment's end
    if (n < 16) fill();
    return (uint32_t)(n >= 16 ? acc >> (n - 16) : acc << (16 - n)) & 0xFFFFu;
  }
  void skip(int k) { if (k > n) { bad = true; n = 0; } else n -= k; }
  uint32_t bits(int k) {                                         // k <= 16
    if (k == 0) return 0;
    if (n < k) { fill(); if (n < k) { bad = true; n = 0; return 0; } }
    n -= k;
    return (uint32_t)(acc >> n) & ((1u << k) - 1u);
  }
  int decode(const JpegHuff &t) {
    const uint32_t v = peek16();
    const uint16_t f = t.fast[v >> 7];
    if (f) { skip(f >> 8); return f & 0xFF; }
    for (int l = 10; l <= 16; l++) {
      const int32_t code = (int32_t)(v >> (16 - l));
      if (code <= t.maxcode[l]) {                                // maxcode -1 when the length is unused
        const int32_t idx = t.valptr[l] + code - t.mincode[l];
        if (code < t.mincode[l] || idx < 0 || idx > 255) break;
        skip(l); return t.vals[idx];
      }
    }
    bad = true; return 0;                                        // no code matches these bits
  }
  // drop the rest of the current byte and whatever precedes the next marker; returns the marker byte and steps over it, -1 when there is none
  int next_marker() {
    acc = 0; n = 0;
    while (pos + 1 < len) {
      if (d[pos] == 0xFF && d[pos + 1] != 0 && d[pos + 1] != 0xFF) { const int m = d[pos + 1]; pos += 2; return m; }
      pos++;
    }
    return -1;
  }
};

static inline int jpeg_extend(uint32_t v, int t) { return t == 0 ? 0 : (v >> (t - 1)) ? (int)v : (int)v - (1 << t) + 1; }

// Returns 0 on success, 2 (MI_UNSUPPORTED) for non-JPEG data and the JPEG processes / shapes this reader does not take, 3 (MI_ENCODING_ERROR) for
// broken streams.
inline int jpeg_read_coeffs(const uint8_t *d, size_t len, JpegCoeffs &out) {
  if (len < 2 || d[0] != 0xFF || d[1] != 0xD8) return 2;
  uint16_t qt[4][64]; bool have_qt[4] = { false, false, false, false };
  std::vector<JpegHuff> huff(8);                                 // 0-3 DC, 4-7 AC
  bool jfif = false, adobe = false, have_frame = false, progressive = false, saw_eoi = false, have_exif = false;
  int adobe_transform = 0;
  JpegIccParts icc_parts;
  uint32_t restart_interval = 0;
  int8_t coef_bits[3][64];                                       // progressive: the point transform each coefficient has reached, -1 = not sent yet
  memset(coef_bits, -1, sizeof(coef_bits));
  bool covered[3] = { false, false, false };                     // sequential: the component's scan has been decoded
  size_t pos = 2;
  while (!saw_eoi) {
    // marker: FF, any number of fill FFs, the code
    if (pos >= len || d[pos] != 0xFF) return 3;
    while (pos < len && d[pos] == 0xFF) pos++;
    if (pos >= len) return 3;
    const int m = d[pos++];
    if (m == 0xD9) { saw_eoi = true; break; }
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {    // stand-alone markers have no place between segments, SOI none after the first
      if (m == 0xD8) return 3;
      continue;
    }
    if (m == 0) return 3;
    if (pos + 2 > len) return 3;
    const size_t L = ((size_t)d[pos] << 8) | d[pos + 1];
    if (L < 2 || pos + L > len) return 3;
    const uint8_t *seg = d + pos + 2; const size_t n = L - 2;
    pos += L;
    if (m == 0xE0) { if (n >= 12 && !memcmp(seg, "JFIF\0", 5)) jfif = true; }
    else if (m == 0xEE) { if (n >= 12 && !memcmp(seg, "Adobe", 5)) { adobe = true; adobe_transform = seg[11]; } }
    else if (m == 0xE2) icc_parts.add(seg, n);                   // ICC profile segments: kept for mi_jpeg_coeffs_icc, nothing else reads them
    else if (m == 0xE1) {                                        // the first Exif segment: its orientation is kept, nothing else of it (XMP is APP1 as well: skipped)
      if (!have_exif && n >= 6 && !memcmp(seg, "Exif\0\0", 6)) { have_exif = true; out.orientation = exif_orientation(seg, n); }
    } else if ((m >= 0xE3 && m <= 0xEF) || m == 0xFE) {}         // other APPn, COM: skipped
    else if (m == 0xDB) {                                        // DQT
      for (size_t i = 0; i < n;) {
        const int pq = seg[i] >> 4, tq = seg[i] & 15; i++;
        if (pq > 1 || tq > 3 || i + (pq ? 128 : 64) > n) return 3;
        for (int k = 0; k < 64; k++) qt[tq][jpeg_zigzag[k]] = pq ? (uint16_t)((seg[i + 2 * k] << 8) | seg[i + 2 * k + 1]) : seg[i + k];
        i += pq ? 128 : 64; have_qt[tq] = true;
      }
    } else if (m == 0xC4) {                                      // DHT
      for (size_t i = 0; i < n;) {
        if (i + 17 > n) return 3;
        const int tc = seg[i] >> 4, th = seg[i] & 15;
        if (tc > 1 || th > 3) return 3;
        int total = 0; for (int k = 0; k < 16; k++) total += seg[i + 1 + k];
        if (total > 256 || i + 17 + (size_t)total > n) return 3;
        if (!huff[tc * 4 + th].build(seg + i + 1, seg + i + 17, total)) return 3;
        i += 17 + (size_t)total;
      }
    } else if (m == 0xDD) { if (n != 2) return 3; restart_interval = ((uint32_t)seg[0] << 8) | seg[1]; }
    else if (m == 0xC0 || m == 0xC1 || m == 0xC2) {              // SOF0 / SOF1 / SOF2
      if (have_frame || n < 6) return 3;
      const int prec = seg[0], nc = seg[5];
      out.h = ((uint32_t)seg[1] << 8) | seg[2]; out.w = ((uint32_t)seg[3] << 8) | seg[4];
      if (prec != 8) return prec == 12 ? 2 : 3;
      if (out.h == 0) return 2;                                  // height deferred to a DNL segment
      if (out.w == 0 || n != 6 + 3 * (size_t)nc) return 3;
      if (nc != 1 && nc != 3) return 2;                          // CMYK / YCCK and two-component files
      out.ncomp = nc; progressive = m == 0xC2;
      for (int c = 0; c < nc; c++) {
        JpegComp &k = out.comp[c];
        k.id = seg[6 + 3 * c]; k.h = seg[7 + 3 * c] >> 4; k.v = seg[7 + 3 * c] & 15; k.tq = seg[8 + 3 * c];
        if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4 || k.tq > 3) return 3;
        for (int e = 0; e < c; e++) if (out.comp[e].id == k.id) return 3;
      }
      if (nc == 1) { out.comp[0].h = out.comp[0].v = 1; }       // a single component is never interleaved: its sampling factors mean nothing
      else {
        const JpegComp &y = out.comp[0], &cb = out.comp[1], &cr = out.comp[2];
        if (cb.h != cr.h || cb.v != cr.v || y.h % cb.h || y.v % cb.v) return 2;
        const int rh = y.h / cb.h, rv = y.v / cb.v;
        if (!((rh == 1 && rv == 1) || (rh == 2 && rv == 1) || (rh == 2 && rv == 2))) return 2;          // 4:4:4, 4:2:2, 4:2:0
      }
      out.hmax = out.comp[0].h; out.vmax = out.comp[0].v;
      const uint32_t mw = (out.w + 8 * out.hmax - 1) / (8 * out.hmax), mh = (out.h + 8 * out.vmax - 1) / (8 * out.vmax);
      out.nblocks = 0;
      for (int c = 0; c < nc; c++) {
        JpegComp &k = out.comp[c];
        k.cw = (out.w * k.h + out.hmax - 1) / out.hmax; k.ch = (out.h * k.v + out.vmax - 1) / out.vmax;
        k.bw = mw * k.h; k.bh = mh * k.v;
        k.first_block = out.nblocks; out.nblocks += (size_t)k.bw * k.bh;
      }
      // every block costs at least one bit in its first DC scan: a header whose canvas the data cannot back is refused before anything is allocated
      if (out.nblocks > 8 * len) return 3;
      have_frame = true;
    } else if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF)) return 2;   // lossless, hierarchical, arithmetic
    else if (m == 0xDA) {                                        // SOS + its entropy-coded segment
      if (!have_frame || n < 1) return 3;
      const int ns = seg[0];
      if (ns < 1 || ns > out.ncomp || n != 4 + 2 * (size_t)ns) return 3;
      int sc[3], td[3], ta[3];
      for (int i = 0; i < ns; i++) {
        sc[i] = -1;
        for (int c = 0; c < out.ncomp; c++) if (out.comp[c].id == seg[1 + 2 * i]) sc[i] = c;
        if (sc[i] < 0) return 3;
        for (int e = 0; e < i; e++) if (sc[e] == sc[i]) return 3;
        td[i] = seg[2 + 2 * i] >> 4; ta[i] = seg[2 + 2 * i] & 15;
        if (td[i] > 3 || ta[i] > 3) return 3;
      }
      int Ss = seg[1 + 2 * ns], Se = seg[2 + 2 * ns], Ah = seg[3 + 2 * ns] >> 4, Al = seg[3 + 2 * ns] & 15;
      if (progressive) {
        if (Ss > Se || Se > 63 || Ah > 13 || Al > 13 || (Ss == 0 && Se != 0) || (Ss != 0 && ns != 1) || (Ah != 0 && Al != Ah - 1)) return 3;
        for (int i = 0; i < ns; i++) for (int k = Ss; k <= Se; k++) {
          int8_t &b = coef_bits[sc[i]][k];
          if (Ss != 0 && coef_bits[sc[i]][0] < 0) return 3;      // AC before the component's DC
          if (Ah == 0 ? b >= 0 : b != Ah) return 3;              // a first scan of something sent already, or a refinement out of step
          b = (int8_t)Al;
        }
      } else {
        Ss = 0; Se = 63; Ah = 0; Al = 0;
        for (int i = 0; i < ns; i++) { if (covered[sc[i]]) return 3; covered[sc[i]] = true; }
      }
      for (int i = 0; i < ns; i++) {
        JpegComp &k = out.comp[sc[i]];
        if (!k.have_quant) { if (!have_qt[k.tq]) return 3; memcpy(k.quant, qt[k.tq], sizeof(k.quant)); k.have_quant = true; }
        if (Ss == 0 && Ah == 0 && !huff[td[i]].defined) return 3;
        if (Se > 0 && !huff[4 + ta[i]].defined) return 3;
      }
      if (out.coef.empty()) out.coef.assign(out.nblocks * 64, 0);
      // scan geometry: interleaved scans walk MCUs; a one-component scan walks that component's own blocks, ceil(cw / 8) x ceil(ch / 8) of them
      uint32_t units_x, units_y; int bh[3], bv[3];
      if (ns == 1) { const JpegComp &k = out.comp[sc[0]]; units_x = (k.cw + 7) / 8; units_y = (k.ch + 7) / 8; bh[0] = bv[0] = 1; }
      else {
        units_x = out.comp[0].bw / out.comp[0].h; units_y = out.comp[0].bh / out.comp[0].v;
        int per_mcu = 0;
        for (int i = 0; i < ns; i++) { bh[i] = out.comp[sc[i]].h; bv[i] = out.comp[sc[i]].v; per_mcu += bh[i] * bv[i]; }
        if (per_mcu > 10) return 3;
      }
      JpegBits br(d, pos, len);
      uint32_t pred[3] = { 0, 0, 0 }, eobrun = 0, since_restart = 0;
      for (uint32_t uy = 0; uy < units_y; uy++) for (uint32_t ux = 0; ux < units_x; ux++) {
        if (restart_interval && since_restart == restart_interval) {
          const int rm = br.next_marker();
          if (rm < 0xD0 || rm > 0xD7) return 3;
          pred[0] = pred[1] = pred[2] = 0; eobrun = 0; since_restart = 0;
        }
        since_restart++;
        for (int i = 0; i < ns; i++) {
          const JpegComp &k = out.comp[sc[i]];
          const JpegHuff &hd = huff[td[i]], &ha = huff[4 + ta[i]];
          for (int by = 0; by < bv[i]; by++) for (int bx = 0; bx < bh[i]; bx++) {
            const size_t bi = k.first_block + ((size_t)uy * bv[i] + by) * k.bw + (size_t)ux * bh[i] + bx;
            int16_t *blk = &out.coef[bi * 64];
            if (!progressive) {                                  // T.81 F.2.2
              const int t = br.decode(hd);
              if (t > 11) return 3;
              pred[i] += (uint32_t)jpeg_extend(br.bits(t), t);
              blk[0] = (int16_t)pred[i];
              for (int kk = 1; kk < 64; kk++) {
                const int rs = br.decode(ha), r = rs >> 4, s = rs & 15;
                if (s == 0) { if (r != 15) break; kk += 15; continue; }
                kk += r;
                if (kk > 63) return 3;
                blk[jpeg_zigzag[kk]] = (int16_t)jpeg_extend(br.bits(s), s);
              }
            } else if (Ss == 0) {                                // DC scans, G.1.2.1
              if (Ah == 0) {
                const int t = br.decode(hd);
                if (t > 15) return 3;
                pred[i] += (uint32_t)jpeg_extend(br.bits(t), t);
                blk[0] = (int16_t)(pred[i] << Al);
              } else if (br.bits(1)) blk[0] = (int16_t)(blk[0] | (1 << Al));
            } else if (Ah == 0) {                                // AC first scan, G.1.2.2
              if (eobrun) eobrun--;
              else for (int kk = Ss; kk <= Se; kk++) {
                const int rs = br.decode(ha), r = rs >> 4, s = rs & 15;
                if (s == 0) {
                  if (r == 15) { kk += 15; continue; }
                  eobrun = (1u << r) - 1u; if (r) eobrun += br.bits(r);
                  break;
                }
                kk += r;
                if (kk > Se) return 3;
                blk[jpeg_zigzag[kk]] = (int16_t)((uint32_t)jpeg_extend(br.bits(s), s) << Al);
              }
            } else {                                             // AC refinement, G.1.2.3
              const int p1 = 1 << Al, m1 = -(1 << Al);
              int kk = Ss;
              if (eobrun == 0) {
                for (; kk <= Se; kk++) {
                  const int rs = br.decode(ha); int r = rs >> 4, s = rs & 15;
                  if (s) { if (s != 1) return 3; s = br.bits(1) ? p1 : m1; }
                  else if (r != 15) { eobrun = 1u << r; if (r) eobrun += br.bits(r); break; }
                  for (; kk <= Se; kk++) {                       // step over r zero-history coefficients, correcting the nonzero ones passed on the way
                    int16_t &c = blk[jpeg_zigzag[kk]];
                    if (c != 0) { if (br.bits(1) && (c & p1) == 0) c = (int16_t)(c + (c >= 0 ? p1 : m1)); }
                    else if (--r < 0) break;
                  }
                  if (s) { if (kk > Se) return 3; blk[jpeg_zigzag[kk]] = (int16_t)s; }
                }
              }
              if (eobrun) {
                for (; kk <= Se; kk++) {
                  int16_t &c = blk[jpeg_zigzag[kk]];
                  if (c != 0 && br.bits(1) && (c & p1) == 0) c = (int16_t)(c + (c >= 0 ? p1 : m1));
                }
                eobrun--;
              }
            }
            if (br.bad) return 3;                                // the segment ended inside this block, or its bits match no code
          }
        }
      }
      // the segment is over: whatever precedes the next marker is padding
      br.acc = 0; br.n = 0;
      pos = br.pos;
      while (pos + 1 < len && !(d[pos] == 0xFF && d[pos + 1] != 0 && d[pos + 1] != 0xFF)) pos++;
      if (pos + 1 >= len) return 3;                              // no EOI behind the last scan
    } else if (m == 0xDC) return 2;                              // DNL
    else if (m < 0xC0) return 3;                                 // reserved codes
    // anything else with a length (DAC, DHP, EXP, JPGn): skipped
  }
  if (!have_frame || out.coef.empty()) return 3;
  for (int c = 0; c < out.ncomp; c++) {
    if (progressive) { for (int k = 0; k < 64; k++) if (coef_bits[c][k] != 0) return 3; }                 // a scan is missing: libjpeg would smooth, this reader refuses
    else if (!covered[c]) return 3;
  }
  // libjpeg's rule for three components (jdapimin.c default_decompress_parms): JFIF -> YCbCr; Adobe -> its transform byte; else the component ids
  if (out.ncomp == 1) out.color = JPEG_GREY;
  else if (jfif) out.color = JPEG_YCBCR;
  else if (adobe) out.color = adobe_transform == 0 ? JPEG_RGB : JPEG_YCBCR;
  else out.color = (out.comp[0].id == 'R' && out.comp[1].id == 'G' && out.comp[2].id == 'B') ? JPEG_RGB : JPEG_YCBCR;
  icc_parts.finish(out.icc);
  return 0;
}

}  // namespace mi
