// exif_sweep_main.cpp -- TEST INFRASTRUCTURE: a stand-alone host program over exif_reader.h and the APP1 / eXIf code of jpeg_reader.h and png_reader.h, built by
// tests/test_exif_reader.py with -fsanitize=address,undefined.  It reads a file of blobs (kind byte, 32-bit little-endian length, bytes; kind 0 an Exif blob, 1 a PNG
// file, 2 a JPEG file).  Of an Exif blob it reads every truncation and every single-byte corruption (each byte xor 0xFF, and set to 0 where that is a change), each
// from a heap copy of its exact length -- one byte read past it is a sanitizer report; a PNG or JPEG file is read as it is (the test writes the truncations and
// corruptions of the spliced segment).  Exit status 0 = every answer was an orientation of 1..8; prints "reads N upright A turned B".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "exif_reader.h"
#include "png_reader.h"
#include "jpeg_reader.h"

static size_t reads = 0, count[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
static bool note(int o, const char *what, size_t blob) {
  if (o < 1 || o > 8) { fprintf(stderr, "blob %zu (%s): orientation %d\n", blob, what, o); return false; }
  count[o]++; reads++;
  return true;
}
// the parser over a heap copy of exactly n bytes
static int read_copy(const uint8_t *d, size_t n) {
  uint8_t *c = (uint8_t *)malloc(n ? n : 1);
  if (n) memcpy(c, d, n);
  const int o = mi::exif_orientation(n ? c : c + 1, n);      // nothing may be read of an empty blob: its pointer is one past the allocation
  free(c);
  return o;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: exif_sweep BLOBS\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  size_t blobs = 0;
  for (;; blobs++) {
    uint8_t head[5];
    if (fread(head, 1, 5, f) != 5) break;
    const size_t n = (size_t)head[1] | ((size_t)head[2] << 8) | ((size_t)head[3] << 16) | ((size_t)head[4] << 24);
    std::vector<uint8_t> d(n);
    if (n && fread(d.data(), 1, n, f) != n) { fprintf(stderr, "short blob\n"); return 2; }
    if (head[0] == 0) {
      if (!note(read_copy(d.data(), n), "whole", blobs)) return 1;
      for (size_t k = 0; k < n; k++) if (!note(read_copy(d.data(), k), "truncated", blobs)) return 1;
      for (size_t k = 0; k < n; k++) {
        const uint8_t keep = d[k];
        d[k] = keep ^ 0xFF;
        if (!note(read_copy(d.data(), n), "corrupted", blobs)) return 1;
        if (keep) { d[k] = 0; if (!note(read_copy(d.data(), n), "zeroed", blobs)) return 1; }
        d[k] = keep;
      }
    } else {
      uint8_t *c = (uint8_t *)malloc(n ? n : 1);
      if (n) memcpy(c, d.data(), n);
      int o = 1;
      if (head[0] == 1) { mi::PngScanlines sl; (void)mi::png_read_scanlines(c, n, sl); o = sl.orientation; }
      else { mi::JpegCoeffs jc; (void)mi::jpeg_read_coeffs(c, n, jc); o = jc.orientation; }
      free(c);
      if (!note(o, head[0] == 1 ? "png" : "jpeg", blobs)) return 1;
    }
  }
  fclose(f);
  printf("reads %zu upright %zu turned %zu\n", reads, count[1], reads - count[1]);
  return 0;
}
