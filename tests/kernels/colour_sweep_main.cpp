// colour_sweep_main.cpp -- TEST INFRASTRUCTURE: a stand-alone host program over icc_reader.h and the colour chunk / APP2 code of png_reader.h and jpeg_reader.h,
// built by tests/test_icc_reader.py with -fsanitize=address,undefined.  It reads a file of blobs (kind byte, 32-bit little-endian length, bytes; kind 0 an ICC
// profile, 1 a PNG file, 2 a JPEG file), hands each to its reader from a heap copy of its exact length -- one byte read past it is a sanitizer report -- and
// carries whatever colour description comes out through the cache key of the stream workers into a bake.  Exit status 0 = every blob gave one of the three statuses; prints "blobs N ok A unsupported B malformed C".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "icc_reader.h"
#include "png_reader.h"
#include "jpeg_reader.h"

// a description the way a stream worker treats it: hashed where it lies, copied into a cache key, and baked from the key (icc_reader.h); a profile is first
// moved into a heap copy of its exact length
static int bake(mi::ColourDescription d) {
  uint8_t *copy = nullptr;
  if (d.kind == 1) { copy = (uint8_t *)malloc(d.icc_len); memcpy(copy, d.icc, d.icc_len); d.icc = copy; }
  uint8_t scratch[80]; const uint8_t *p = nullptr; size_t n = 0;
  mi::colour_description_bytes(d, scratch, p, n);
  const uint64_t hash = mi::colour_hash(p, n);
  const mi::ColourKey key = mi::colour_key_make(d.kind, hash, p, n);
  free(copy);
  if (!mi::colour_key_matches(key, d.kind, hash, key.bytes.data(), key.bytes.size())) return -2;
  mi::ColourTables t, probe;
  const int st = mi::colour_tables_from_description(mi::colour_description_of_key(key), t);
  if (mi::colour_tables_from_description(mi::colour_description_of_key(key), probe, false) != st || (st == 0 && probe.identity != t.identity)) return -3;   // the table-free probe agrees
  if (st == 0 && !t.identity && (t.lin8.size() != 768 || t.lin16.size() != 3 * 4098 || t.thresholds.size() != 256 || t.out16.size() != 8194)) return -1;
  return st;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: colour_sweep BLOBS\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  size_t blobs = 0, count[4] = { 0, 0, 0, 0 };
  for (;;) {
    uint8_t head[5];
    if (fread(head, 1, 5, f) != 5) break;
    const size_t n = (size_t)head[1] | ((size_t)head[2] << 8) | ((size_t)head[3] << 16) | ((size_t)head[4] << 24);
    uint8_t *d = (uint8_t *)malloc(n ? n : 1);
    if (n && fread(d, 1, n, f) != n) { fprintf(stderr, "short blob\n"); return 2; }
    int st = 0;
    if (head[0] == 0) st = n ? bake(mi::colour_description_of_icc(d, n)) : 3;
    else if (head[0] == 1) {
      mi::PngScanlines sl;
      st = mi::png_read_scanlines(d, n, sl);
      if (st == 0) { mi::png_resolve_colour(sl); st = bake(mi::colour_description_of_png(sl.colour, sl.icc_oversize, sl.icc.data(), sl.icc.size(), sl.file_gamma, sl.has_chrm, sl.chrm)); }
    } else {
      mi::JpegCoeffs jc;
      st = mi::jpeg_read_coeffs(d, n, jc);
      if (st == 0) st = bake(mi::colour_description_of_icc(jc.icc.data(), jc.icc.size()));
    }
    free(d);
    if (st != 0 && st != 2 && st != 3) { fprintf(stderr, "blob %zu (kind %d, %zu bytes): status %d\n", blobs, head[0], n, st); return 1; }
    count[st]++; blobs++;
  }
  fclose(f);
  printf("blobs %zu ok %zu unsupported %zu malformed %zu\n", blobs, count[0], count[2], count[3]);
  return 0;
}
