// icc_reader.h -- colour descriptions of input files -> a baked transform to sRGB.  Host C++, written from the ICC specification (ICC.1:2001-04
// for v2, ICC.1:2010 for v4: header, tag table, XYZType, curveType, parametricCurveType), the PNG specification (gAMA, cHRM) and IEC 61966-2-1 (sRGB).
//   icc_parse          an RGB matrix/TRC profile (colour space 'RGB ', PCS 'XYZ ', rXYZ gXYZ bXYZ rTRC gTRC bTRC; 'curv' with 0, 1 or n entries, 'para' of
//                      types 0..4) -> three curves and the colorant matrix.  Every offset, size and count is checked against the profile before it is used: the
//                      parser never reads outside [d, d + len).  A well-formed profile of another kind (A2B0, CMYK, grey, Lab PCS, device link, named colours) is
//                      2 (MI_UNSUPPORTED), a malformed one 3 (MI_ENCODING_ERROR).
//   colour_bake        curves + colorants -> the integer tables dev_colour.h runs on.  The arithmetic of the kernels is specified there; the tables are
//                      specified here, in IEEE doubles with one operation per step and no contraction, so that a restatement in another language gives the
//                      same integers (tests/helpers/colour_ref.py):
//                        q(v)        = floor(clamp(v, 0, 1) * 2^24 + 0.5)                                   linear light, 24 fractional bits
//                        lin8[c][v]  = q(curve_c(v / 255)),  v = 0..255
//                        lin16[c][i] = q(curve_c(i / 4096)), i = 0..4096, and lin16[c][4097] = lin16[c][4096]
//                        matrix[i][j] = floor(M[i][j] * 2^30 + 0.5),  M = inverse(S) * P, S the sRGB colorants (D50), P the source's (D50), columns R G B
//                        U[k]        = ceil(2^24 * eotf((2 k - 1) / 510)), k = 1..255, U[0] = 0: the smallest linear value whose sRGB encoding rounds to level k
//                        out16[i]    = floor(65535 * oetf(i / 8192) + 0.5), i = 0..8192, and out16[8193] = out16[8192]
//                      with eotf(e) = e <= 0.04045 ? e / 12.92 : pow((e + 0.055) / 1.055, 2.4) and oetf(l) = l <= 0.0031308 ? 12.92 l : 1.055 pow(l, 1 / 2.4) - 0.055.
//   S is made from the sRGB primaries (0.64, 0.33), (0.30, 0.60), (0.15, 0.06) and D65 (0.3127, 0.3290), Bradford-adapted to D50 (0.9642, 1, 0.8249): the way a
//   cHRM chunk's primaries are treated, so that cHRM = sRGB's gives the identity matrix to the last bit.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace mi {

constexpr int CT_FRAC = 24, CT_MBITS = 30, CT_LIN16_SEG = 4096, CT_OUT16_SEG = 8192;
constexpr uint32_t CT_ONE = 1u << CT_FRAC;

struct ColourCurve {
  int kind = 0;                         // 0 identity, 1 power, 2 table, 3 parametric
  double gamma = 1.0;                   // kind 1
  std::vector<uint16_t> table;          // kind 2: n >= 2 entries over [0, 1]
  int ftype = 0; double p[7] = { 1, 1, 0, 0, 0, 0, 0 };   // kind 3: g a b c d e f
  double eval(double x) const {
    double y = x;
    if (kind == 1) y = pow(x, gamma);
    else if (kind == 2) {
      const size_t n = table.size();
      const double pos = x * (double)(n - 1);
      size_t i = (size_t)pos;
      if (i > n - 2) i = n - 2;
      const double f = pos - (double)i;
      y = ((double)table[i] + ((double)table[i + 1] - (double)table[i]) * f) / 65535.0;
    } else if (kind == 3) {
      const double g = p[0], a = p[1], b = p[2], c = p[3], d = p[4], e = p[5], f = p[6];
      auto power = [&](double t) { return t > 0.0 ? pow(t, g) : 0.0; };
      switch (ftype) {
        case 0: y = power(x); break;
        case 1: y = a * x + b >= 0.0 ? power(a * x + b) : 0.0; break;
        case 2: y = a * x + b >= 0.0 ? power(a * x + b) + c : c; break;
        case 3: y = x >= d ? power(a * x + b) : c * x; break;
        default: y = x >= d ? power(a * x + b) + e : c * x + f; break;
      }
    }
    if (!(y >= 0.0)) y = 0.0;           // NaN as well
    if (y > 1.0) y = 1.0;
    return y;
  }
};

struct ColourSource { ColourCurve curve[3]; double colorants[3][3]; };   // colorants[row X Y Z][column R G B], D50

// ---- 3 x 3 helpers: plain loops, one rounding per operation
inline void mat3_mul(const double a[3][3], const double b[3][3], double o[3][3]) {
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { double s = 0.0; for (int k = 0; k < 3; k++) s += a[i][k] * b[k][j]; o[i][j] = s; }
}
inline bool mat3_inv(const double m[3][3], double o[3][3]) {
  const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
  const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
  if (!(fabs(det) > 1e-12) || !std::isfinite(det)) return false;
  o[0][0] = c00 / det; o[1][0] = c01 / det; o[2][0] = c02 / det;
  o[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det; o[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det; o[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det;
  o[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det; o[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det; o[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
  return true;
}

// chromaticities (white x y, red x y, green x y, blue x y) -> colorants with the white point Bradford-adapted to D50; false = degenerate
inline bool colorants_from_chromaticities(const double c[8], double out[3][3]) {
  for (int i = 0; i < 8; i++) if (!std::isfinite(c[i]) || c[i] < 0.0 || c[i] > 1.0) return false;
  if (c[1] <= 0.0 || c[3] <= 0.0 || c[5] <= 0.0 || c[7] <= 0.0) return false;
  const double W[3] = { c[0] / c[1], 1.0, (1.0 - c[0] - c[1]) / c[1] };
  double P[3][3], Pi[3][3];
  for (int j = 0; j < 3; j++) { const double x = c[2 + 2 * j], y = c[3 + 2 * j]; P[0][j] = x / y; P[1][j] = 1.0; P[2][j] = (1.0 - x - y) / y; }
  if (!mat3_inv(P, Pi)) return false;
  double S[3];
  for (int i = 0; i < 3; i++) { double s = 0.0; for (int k = 0; k < 3; k++) s += Pi[i][k] * W[k]; S[i] = s; }
  double N[3][3];
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) N[i][j] = P[i][j] * S[j];
  static const double B[3][3] = { { 0.8951, 0.2664, -0.1614 }, { -0.7502, 1.7135, 0.0367 }, { 0.0389, -0.0685, 1.0296 } };
  static const double D50[3] = { 0.9642, 1.0, 0.8249 };
  double Bi[3][3];
  if (!mat3_inv(B, Bi)) return false;
  double cs[3], cd[3];
  for (int i = 0; i < 3; i++) { double s = 0.0, d = 0.0; for (int k = 0; k < 3; k++) { s += B[i][k] * W[k]; d += B[i][k] * D50[k]; } cs[i] = s; cd[i] = d; }
  for (int i = 0; i < 3; i++) if (!(fabs(cs[i]) > 1e-12)) return false;
  double DB[3][3], A[3][3];
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) DB[i][j] = (cd[i] / cs[i]) * B[i][j];
  mat3_mul(Bi, DB, A);
  mat3_mul(A, N, out);
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) if (!std::isfinite(out[i][j])) return false;
  return true;
}
inline const double *srgb_chromaticities() { static const double c[8] = { 0.3127, 0.3290, 0.64, 0.33, 0.30, 0.60, 0.15, 0.06 }; return c; }

// ---- the ICC parser
inline uint32_t icc_be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline double icc_s15f16(const uint8_t *p) { return (double)(int32_t)icc_be32(p) / 65536.0; }
constexpr uint32_t icc_sig(char a, char b, char c, char d) { return ((uint32_t)(uint8_t)a << 24) | ((uint32_t)(uint8_t)b << 16) | ((uint32_t)(uint8_t)c << 8) | (uint8_t)d; }

// one curve tag at d[off, off + size): the caller has checked that the range lies inside the profile
inline int icc_parse_curve(const uint8_t *d, size_t off, size_t size, ColourCurve &cv) {
  if (size < 12) return 3;
  const uint8_t *t = d + off;
  const uint32_t type = icc_be32(t);
  if (type == icc_sig('c', 'u', 'r', 'v')) {
    const uint32_t count = icc_be32(t + 8);
    if (count > (size - 12) / 2) return 3;                    // a table larger than its tag
    if (count == 0) { cv.kind = 0; return 0; }
    if (count == 1) { cv.kind = 1; cv.gamma = (double)(((uint32_t)t[12] << 8) | t[13]) / 256.0; return cv.gamma > 0.0 ? 0 : 3; }
    cv.kind = 2; cv.table.resize(count);
    for (uint32_t i = 0; i < count; i++) cv.table[i] = (uint16_t)(((uint32_t)t[12 + 2 * i] << 8) | t[13 + 2 * i]);
    return 0;
  }
  if (type == icc_sig('p', 'a', 'r', 'a')) {
    const uint32_t ftype = ((uint32_t)t[8] << 8) | t[9];
    if (ftype > 4) return 2;
    static const int nparams[5] = { 1, 3, 4, 5, 7 };
    const int n = nparams[ftype];
    if ((size - 12) / 4 < (size_t)n) return 3;
    double v[7];
    for (int i = 0; i < n; i++) v[i] = icc_s15f16(t + 12 + 4 * i);
    cv.kind = 3; cv.ftype = (int)ftype;
    cv.p[0] = v[0]; cv.p[1] = 1.0; cv.p[2] = cv.p[3] = cv.p[4] = cv.p[5] = cv.p[6] = 0.0;
    if (ftype >= 1) { cv.p[1] = v[1]; cv.p[2] = v[2]; }
    if (ftype == 2) cv.p[3] = v[3];                           // g a b c
    if (ftype >= 3) { cv.p[3] = v[3]; cv.p[4] = v[4]; }       // g a b c d
    if (ftype == 4) { cv.p[5] = v[5]; cv.p[6] = v[6]; }       // g a b c d e f
    return 0;
  }
  return 2;
}

inline int icc_parse(const uint8_t *d, size_t len, ColourSource &src) {
  if (!d || len < 132) return 3;                              // a truncated header
  const uint32_t size = icc_be32(d);
  if (size > len || size < 132) return 3;                     // the size field disagrees with the data (bytes after the profile are padding)
  const size_t n = size;
  if (icc_be32(d + 36) != icc_sig('a', 'c', 's', 'p')) return 3;
  const uint32_t cls = icc_be32(d + 12), space = icc_be32(d + 16), pcs = icc_be32(d + 20);
  const uint32_t count = icc_be32(d + 128);
  if (count > (n - 132) / 12) return 3;
  // every tag lies inside the profile, whether it is used or not
  size_t at[7] = { 0, 0, 0, 0, 0, 0, 0 }, sz[7] = { 0, 0, 0, 0, 0, 0, 0 };
  static const uint32_t want[7] = { icc_sig('r', 'X', 'Y', 'Z'), icc_sig('g', 'X', 'Y', 'Z'), icc_sig('b', 'X', 'Y', 'Z'), icc_sig('r', 'T', 'R', 'C'),
                                    icc_sig('g', 'T', 'R', 'C'), icc_sig('b', 'T', 'R', 'C'), icc_sig('A', '2', 'B', '0') };
  for (uint32_t i = 0; i < count; i++) {
    const uint8_t *e = d + 132 + 12 * (size_t)i;
    const uint32_t sig = icc_be32(e), off = icc_be32(e + 4), tsz = icc_be32(e + 8);
    if (off < 128 || off > n || tsz > n - off) return 3;
    for (int k = 0; k < 7; k++) if (sig == want[k] && !sz[k]) { if (!tsz) return 3; at[k] = off; sz[k] = tsz; }
  }
  if (cls == icc_sig('l', 'i', 'n', 'k') || cls == icc_sig('n', 'm', 'c', 'l') || cls == icc_sig('a', 'b', 's', 't')) return 2;
  if (space != icc_sig('R', 'G', 'B', ' ') || pcs != icc_sig('X', 'Y', 'Z', ' ')) return 2;
  if (sz[6]) return 2;                                        // a LUT profile: the tables win over the matrix in every CMM
  for (int k = 0; k < 6; k++) if (!sz[k]) return 3;           // a required tag is missing
  for (int k = 0; k < 3; k++) {
    if (sz[k] < 20 || icc_be32(d + at[k]) != icc_sig('X', 'Y', 'Z', ' ')) return 3;
    for (int r = 0; r < 3; r++) src.colorants[r][k] = icc_s15f16(d + at[k] + 8 + 4 * r);
  }
  for (int k = 0; k < 3; k++) if (const int st = icc_parse_curve(d, at[3 + k], sz[3 + k], src.curve[k])) return st;
  return 0;
}

// ---- the baked transform
struct ColourTables {
  bool identity = true;
  int64_t matrix[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };          // row-major: out channel i = sum_j matrix[3 i + j] * in channel j
  std::vector<uint32_t> lin8, thresholds, lin16;             // 3 x 256, 256, 3 x (CT_LIN16_SEG + 2)
  std::vector<uint16_t> out16;                                // CT_OUT16_SEG + 2
};

inline double srgb_eotf(double e) { return e <= 0.04045 ? e / 12.92 : pow((e + 0.055) / 1.055, 2.4); }
inline double srgb_oetf(double l) { return l <= 0.0031308 ? 12.92 * l : 1.055 * pow(l, 1.0 / 2.4) - 0.055; }
inline uint32_t colour_q(double v) { if (!(v >= 0.0)) v = 0.0; if (v > 1.0) v = 1.0; return (uint32_t)floor(v * 16777216.0 + 0.5); }

// `exact_matrix`: the colorants are sRGB's own (no cHRM): the matrix is the identity without going through an inverse.  false = singular colorants.
// `tables` false: the matrix alone -- what it takes to learn whether a description can be converted (no curve is evaluated)
inline bool colour_bake(const ColourSource &src, bool exact_matrix, ColourTables &t, bool tables = true) {
  double M[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
  if (!exact_matrix) {
    double S[3][3], Si[3][3];
    if (!colorants_from_chromaticities(srgb_chromaticities(), S) || !mat3_inv(S, Si)) return false;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) if (!std::isfinite(src.colorants[i][j])) return false;
    mat3_mul(Si, src.colorants, M);
  }
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
    if (!(fabs(M[i][j]) < 64.0)) return false;                // nothing a display profile holds (they stay below 4); keeps the 64-bit sums of dev_colour.h below 2^62
    t.matrix[3 * i + j] = (int64_t)floor(M[i][j] * 1073741824.0 + 0.5);
  }
  t.identity = false;
  if (!tables) return true;
  t.lin8.resize(3 * 256); t.lin16.resize(3 * (CT_LIN16_SEG + 2)); t.thresholds.resize(256); t.out16.resize(CT_OUT16_SEG + 2);
  for (int c = 0; c < 3; c++) {
    for (int v = 0; v < 256; v++) t.lin8[c * 256 + v] = colour_q(src.curve[c].eval((double)v / 255.0));
    uint32_t *l = t.lin16.data() + c * (CT_LIN16_SEG + 2);
    for (int i = 0; i <= CT_LIN16_SEG; i++) l[i] = colour_q(src.curve[c].eval((double)i / (double)CT_LIN16_SEG));
    l[CT_LIN16_SEG + 1] = l[CT_LIN16_SEG];
  }
  t.thresholds[0] = 0;
  for (int k = 1; k < 256; k++) t.thresholds[k] = (uint32_t)ceil(16777216.0 * srgb_eotf((double)(2 * k - 1) / 510.0));
  for (int i = 0; i <= CT_OUT16_SEG; i++) t.out16[i] = (uint16_t)floor(65535.0 * srgb_oetf((double)i / (double)CT_OUT16_SEG) + 0.5);
  t.out16[CT_OUT16_SEG + 1] = t.out16[CT_OUT16_SEG];
  t.identity = false;
  return true;
}

// 0, or the status of icc_parse; singular colorants are malformed
inline int colour_tables_from_icc(const uint8_t *d, size_t len, ColourTables &t, bool tables = true) {
  ColourSource src;
  if (const int st = icc_parse(d, len, src)) return st;
  return colour_bake(src, false, t, tables) ? 0 : 3;
}

// gAMA (file_gamma, e.g. 0.45455) with an optional cHRM (white x y, red x y, green x y, blue x y).  Identity: no cHRM and |file_gamma * 2.2 - 1| < 0.05, libpng's
// own significance threshold.  4 (MI_INVALID_ARGUMENT): a gamma that is not a positive finite number; 3: degenerate chromaticities
inline int colour_tables_from_png(double file_gamma, const double *chrm, ColourTables &t, bool tables = true) {
  if (!std::isfinite(file_gamma) || !(file_gamma > 0.0)) return 4;
  if (!chrm && fabs(file_gamma * 2.2 - 1.0) < 0.05) { t.identity = true; return 0; }
  ColourSource src;
  for (int c = 0; c < 3; c++) { src.curve[c].kind = 1; src.curve[c].gamma = 1.0 / file_gamma; }
  if (chrm && !colorants_from_chromaticities(chrm, src.colorants)) return 3;
  return colour_bake(src, !chrm, t, tables) ? 0 : 3;
}

// What a file says about its colour, as the stream workers carry and cache it: the kind travels beside the bytes, so the bytes of a profile -- which come from the
// file and may be anything -- are never read as anything but a profile.  A view: `icc` points into the parsed file's handle.
struct ColourDescription {
  int kind = 0;                                               // 0 nothing that needs a conversion, 1 an ICC profile, 2 gAMA with an optional cHRM
  const uint8_t *icc = nullptr; size_t icc_len = 0;           // kind 1
  double file_gamma = 0.0; bool has_chrm = false; double chrm[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };   // kind 2
};
inline ColourDescription colour_description_of_icc(const uint8_t *icc, size_t len) {
  ColourDescription d;
  if (icc && len) { d.kind = 1; d.icc = icc; d.icc_len = len; }
  return d;
}
// the fields of a parsed PNG (png_reader.h: PngScanlines::colour and what goes with it); an sRGB chunk, no description and a profile beyond the reader's cap: kind 0
inline ColourDescription colour_description_of_png(int colour, bool icc_oversize, const uint8_t *icc, size_t icc_len, double file_gamma, bool has_chrm, const double *chrm) {
  if (colour == 1 && !icc_oversize) return colour_description_of_icc(icc, icc_len);
  ColourDescription d;
  if (colour == 3) { d.kind = 2; d.file_gamma = file_gamma; d.has_chrm = has_chrm; if (has_chrm) for (int i = 0; i < 8; i++) d.chrm[i] = chrm[i]; }
  return d;
}
// 0 and the tables (the identity for kind 0), or 2 / 3 as colour_tables_from_icc and _from_png give them (a gamma that is no positive finite number: 3)
inline int colour_tables_from_description(const ColourDescription &d, ColourTables &t, bool tables = true) {
  if (d.kind == 1) return colour_tables_from_icc(d.icc, d.icc_len, t, tables);
  if (d.kind == 2) { const int st = colour_tables_from_png(d.file_gamma, d.has_chrm ? d.chrm : nullptr, t, tables); return st == 4 ? 3 : st; }
  t.identity = true;
  return 0;
}
// The cache key of a description: its kind beside its bytes (the profile, or the ten doubles of gAMA / cHRM).  A look-up hashes the description where it lies
// (colour_description_bytes points at the profile; the doubles go into `scratch`) and compares on a hash hit; only a miss copies the bytes (colour_key_make).
struct ColourKey { int kind = 0; uint64_t hash = 0; std::vector<uint8_t> bytes; };
inline uint64_t colour_hash(const uint8_t *d, size_t len);
inline void colour_description_bytes(const ColourDescription &d, uint8_t scratch[80], const uint8_t *&p, size_t &n) {
  p = d.icc; n = d.kind == 1 ? d.icc_len : 0;
  if (d.kind != 2) return;
  double v[10] = { d.file_gamma, d.has_chrm ? 1.0 : 0.0, 0, 0, 0, 0, 0, 0, 0, 0 };
  for (int i = 0; i < 8; i++) v[2 + i] = d.has_chrm ? d.chrm[i] : 0.0;
  memcpy(scratch, v, sizeof(v)); p = scratch; n = sizeof(v);
}
inline bool colour_key_matches(const ColourKey &k, int kind, uint64_t hash, const uint8_t *p, size_t n) { return k.kind == kind && k.hash == hash && k.bytes.size() == n && (n == 0 || memcmp(k.bytes.data(), p, n) == 0); }
inline ColourKey colour_key_make(int kind, uint64_t hash, const uint8_t *p, size_t n) { ColourKey k; k.kind = kind; k.hash = hash; if (n) k.bytes.assign(p, p + n); return k; }
// the description an owned key stands for (a view into the key)
inline ColourDescription colour_description_of_key(const ColourKey &k) {
  ColourDescription d; d.kind = k.kind;
  if (k.kind == 1) { d.icc = k.bytes.data(); d.icc_len = k.bytes.size(); }
  else if (k.kind == 2 && k.bytes.size() == 10 * sizeof(double)) { double v[10]; memcpy(v, k.bytes.data(), sizeof(v)); d.file_gamma = v[0]; d.has_chrm = v[1] != 0.0; for (int i = 0; i < 8; i++) d.chrm[i] = v[2 + i]; }
  else d.kind = 0;
  return d;
}

// FNV-1a over a profile's bytes: the key the stream workers cache transforms by (compared byte for byte on a hit)
inline uint64_t colour_hash(const uint8_t *d, size_t len) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < len; i++) { h ^= d[i]; h *= 1099511628211ull; }
  return h;
}

}  // namespace mi
