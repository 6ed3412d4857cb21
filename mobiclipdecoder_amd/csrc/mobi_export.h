// mobi_export.h -- addressing of the I420 export (mobi_batch_export, MOBI_EXPORT_I420): one tiled ring slot (mobi_tile.h) -> one packed
// picture, Y width*height, then U and V (width/2)*(height/2) each, rows without stride padding: the reference's Y[i] / UV[i] (MD.cs:107-108,
// 414-415) restricted to the picture area.
//
// One lane moves 16 bytes.  A picture has 1.5 * height * mbw lanes: first height * mbw luma lanes, then (height/2) * mbw chroma lanes.
//   luma   lane -> one macroblock row of 16 pels: 8 bytes of the TL (or BL) quadrant and 8 of the TR (or BR) quadrant, 64 bytes further;
//          consecutive lanes are consecutive macroblocks of one picture row, so a wave's stores are one contiguous run of the output row.
//   chroma lane -> one 16-byte chunk of a chroma tile = one row of 8 U samples and 8 V samples: 8 bytes to the U plane, 8 to the V plane
//          (a row of U is 8 * mbw bytes: an odd mbw needs no special case).
// Only tiles inside the picture are read; Stride == Width (256x192) and Stride > Width are the same code (the tile grid is Stride / 16 wide).
// __host__ __device__ (MOBI_TILE_FN): the kernel (mobi_export.hip) and the CPU test (tests/test_export.py) compile this same code.
#ifndef MOBI_EXPORT_H
#define MOBI_EXPORT_H
#include <stdint.h>

#include "mobi_tile.h"

// lanes of one picture, and of its luma part
MOBI_TILE_FN uint32_t mobi_export_lanes(uint32_t height, uint32_t mbw) { return (height + height / 2) * mbw; }
MOBI_TILE_FN uint32_t mobi_export_luma_lanes(uint32_t height, uint32_t mbw) { return height * mbw; }
// bytes of one packed picture
MOBI_TILE_FN uint32_t mobi_export_i420_bytes(uint32_t width, uint32_t height) { return width * height + width * height / 2; }

// Lane L of a picture: where it reads in the slot and where it writes in the picture.
//   luma (L < height * mbw): src[0], src[1] = 8-byte pieces (src[1] = src[0] + 64); dst[0] = 16 bytes
//   chroma:                  src[0] = one 16-byte chunk [U 8 | V 8]; dst[0] = 8 bytes of U, dst[1] = 8 bytes of V
// Returns 1 for a luma lane, 0 for a chroma lane.
MOBI_TILE_FN int mobi_export_lane(uint32_t L, uint32_t width, uint32_t height, uint32_t mbw, int lgS, uint32_t src[2], uint32_t dst[2]) {
  const uint32_t luma = height * mbw;
  if (L < luma) {
    const uint32_t row = L / mbw, mbx = L - row * mbw;
    src[0] = mobi_tile_y(mbx, row >> 4, lgS) + ((row & 8u) << 4) + ((row & 7u) << 3); // TL / BL quadrant's row
    src[1] = src[0] + 64u;                                                             // TR / BR
    dst[0] = row * width + (mbx << 4);
    dst[1] = dst[0] + 8u;
    return 1;
  }
  const uint32_t l = L - luma, row = l / mbw, mbx = l - row * mbw; // chroma row 0 .. height/2 - 1
  const uint32_t ysz = height << lgS, cw = width >> 1;
  src[0] = ysz + mobi_tile_c(mbx, row >> 3, lgS) + ((row & 7u) << 4);
  src[1] = src[0] + 8u;
  dst[0] = width * height + row * cw + (mbx << 3);
  dst[1] = dst[0] + cw * (height >> 1);
  return 0;
}

#endif
