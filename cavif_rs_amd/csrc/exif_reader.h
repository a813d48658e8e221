// exif_reader.h -- the orientation an input file asks for.  Host C++, written from the Exif 2.32 specification (JEITA CP-3451E 4.5: the TIFF
// header, IFD structure, 4.6.4 A: tag 0x0112 Orientation) and TIFF 6.0 section 2 (image file header, IFD entries).
//   exif_orientation   an Exif blob -- as it lies in a JPEG APP1 segment ("Exif\0\0" first) or in a PNG eXIf chunk / an AVIF item (the TIFF header first) --
//                      -> 1..8.  The TIFF header ("II*\0" little-endian, "MM\0*" big-endian) gives the offset of IFD0; IFD0's entries are walked and nothing
//                      else (no IFD1, no sub-IFD): tag 0x0112 of type SHORT (3) and count 1 with a value of 1..8 is the answer.  Anything else is 1: no tag,
//                      another type or count, a value of 0 or above 8, a truncated blob, an offset or an entry count that leaves the blob.  A file's
//                      orientation never makes the picture an error, as with a broken colour chunk.  Every offset and count is checked against the blob
//                      before it is used: the parser never reads outside [p, p + len).
//   oriented_size      the size of the picture after it has been turned: width and height change places for 5..8.
// What the values mean (the map the kernel of dev_orient.h follows) is stated there and in DESIGN.md 5i.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace mi {

inline int exif_orientation(const uint8_t *p, size_t len) {
  if (!p) return 1;
  if (len >= 6 && !memcmp(p, "Exif\0\0", 6)) { p += 6; len -= 6; }
  if (len < 8) return 1;
  const bool le = !memcmp(p, "II*\0", 4);
  if (!le && memcmp(p, "MM\0*", 4) != 0) return 1;
  auto u16 = [&](size_t at) { return le ? (uint32_t)p[at] | ((uint32_t)p[at + 1] << 8) : ((uint32_t)p[at] << 8) | p[at + 1]; };
  auto u32 = [&](size_t at) { return le ? u16(at) | (u16(at + 2) << 16) : (u16(at) << 16) | u16(at + 2); };
  const size_t ifd = u32(4);
  if (ifd > len || len - ifd < 2) return 1;                      // the entry count lies inside the blob
  const size_t entries = u16(ifd);
  if ((len - ifd - 2) / 12 < entries) return 1;                  // and so does every entry
  for (size_t i = 0; i < entries; i++) {
    const size_t at = ifd + 2 + 12 * i;
    if (u16(at) != 0x0112) continue;
    if (u16(at + 2) != 3 || u32(at + 4) != 1) return 1;          // the first entry with the tag decides
    const uint32_t v = u16(at + 8);                              // a SHORT lies in the first two bytes of the value field, in the blob's byte order
    return v >= 1 && v <= 8 ? (int)v : 1;
  }
  return 1;
}

inline bool orientation_turns(int orientation) { return orientation >= 5 && orientation <= 8; }
inline void oriented_size(uint32_t w, uint32_t h, int orientation, uint32_t *ow, uint32_t *oh) {
  const bool turn = orientation_turns(orientation);
  if (ow) *ow = turn ? h : w;
  if (oh) *oh = turn ? w : h;
}

}  // namespace mi
