// mobi_export_rgb.h -- addressing of the RGB tensor export (mobi_batch_export_device, MOBI_EXPORT_RGB_PLANAR / _PACKED): one tiled ring
// slot (mobi_tile.h) -> one picture of 3 * width * height elements of esize bytes (1: uint8, 2: float16, 4: float32), either planar
// (R plane, G plane, B plane, each height x width: CHW) or packed (height x width x [R G B]: HWC).
//
// One wave = one UNIT = 256 consecutive pixels of the picture in raster order (width and height are multiples of 16, so a picture is a
// whole number of units); lane l = pixels 4l .. 4l + 3 of the unit, which lie in one row (4 | width).  The wave's output is 768 * esize
// bytes: in the planar layout three runs of 256 * esize bytes (one per plane), in the packed layout one run.  The lanes first put their
// elements into a staging image of those bytes in LDS (mobi_rgb_stage_off), then store it as 16-byte chunks, chunk c by lane c mod 64
// (mobi_rgb_chunk_dst): every store instruction of a wave writes runs of >= 256 contiguous bytes in every layout and element size, for
// every width (32, or an odd number of macroblocks, included): a run never ends at a row's end, only at a plane's.
//
// Reads of lane l: 4 luma bytes (one row of a quadrant), the 16-byte chroma chunk [U 8 | V 8] of the chroma row under the pixels and, in
// an odd row not the picture's last, the one of the row below; and where the samples right of the lane's lie in the next macroblock (the
// lane's pixels are the last four of a macroblock row and not of the picture), the next tile's chunk of each such row.  Only tiles inside
// the picture are read (Stride == Width, 256x192, is the same code: the tile grid is Stride / 16 wide).
// __host__ __device__ (MOBI_TILE_FN): the kernel (mobi_export_rgb.hip) and the CPU test (tests/test_export_device.py) compile this code.
#ifndef MOBI_EXPORT_RGB_H
#define MOBI_EXPORT_RGB_H
#include <stdint.h>

#include "mobi_tile.h"

// units of one picture; 16-byte chunks of one unit's output
MOBI_TILE_FN uint32_t mobi_rgb_units(uint32_t width, uint32_t height) { return width * height / 256u; }
MOBI_TILE_FN uint32_t mobi_rgb_chunks(uint32_t esize) { return 48u * esize; }
// bytes of one picture
MOBI_TILE_FN uint32_t mobi_rgb_picture_bytes(uint32_t width, uint32_t height, uint32_t esize) { return 3u * width * height * esize; }

// What lane `lane` of unit `unit` reads.  Offsets: luma inside the tiled Y plane, chroma inside the tiled UV plane (V = U + 8).
struct MobiRgbSrc {
  uint32_t x, y;       // the lane's first pixel (x a multiple of 4)
  uint32_t luma;       // 4 bytes: luma of pixels x .. x + 3
  uint32_t c0, c1;     // 16-byte chunks: the chroma row y / 2 under the pixels, and the row below it (c1 = c0 unless `below`)
  uint32_t n0, n1;     // the next macroblock's chunks of the same rows (= c0, c1 unless `next`)
  uint32_t sel;        // byte of sample a (the one under pixel x) inside the U half: 0, 2, 4, 6
  int odd, lastrow, lastcol, below, next;
};
MOBI_TILE_FN void mobi_rgb_lane(uint32_t unit, uint32_t lane, uint32_t width, uint32_t height, int lgS, MobiRgbSrc *s) {
  const uint32_t p = unit * 256u + lane * 4u, y = p / width, x = p - y * width, cy = y >> 1, cx = x >> 1;
  s->x = x;
  s->y = y;
  s->luma = mobi_ty_row(y, lgS) + mobi_ty_col(x);
  s->odd = (int)(y & 1u);
  s->lastrow = (y | 1u) + 1u >= height; // the odd row of the lane's row pair is the picture's last (mobi_rgb.h, chroma_numerators)
  s->lastcol = x + 4u >= width;
  s->below = s->odd && !s->lastrow;
  s->next = (cx & 7u) == 6u && !s->lastcol; // sample e = cx + 2 starts the next macroblock's chroma row
  s->sel = cx & 7u;
  s->c0 = mobi_tc_row(cy, lgS) + mobi_tc_x(cx & ~7u);
  s->c1 = s->below ? mobi_tc_row(cy + 1u, lgS) + mobi_tc_x(cx & ~7u) : s->c0;
  s->n0 = s->next ? s->c0 + 128u : s->c0;
  s->n1 = s->next ? s->c1 + 128u : s->c1;
}
// byte offset, inside a unit's staging image, of channel ch (0 R, 1 G, 2 B) of pixel t (0 .. 3) of lane l
MOBI_TILE_FN uint32_t mobi_rgb_stage_off(int planar, uint32_t esize, uint32_t l, uint32_t t, uint32_t ch) {
  const uint32_t px = l * 4u + t;
  return (planar ? ch * 256u + px : px * 3u + ch) * esize;
}
// chunk c (bytes 16c .. 16c + 15 of the staging image) -> byte offset inside the picture
MOBI_TILE_FN uint32_t mobi_rgb_chunk_dst(int planar, uint32_t esize, uint32_t width, uint32_t height, uint32_t unit, uint32_t c) {
  if (!planar) return unit * 768u * esize + c * 16u;
  const uint32_t per = 16u * esize, ch = c / per; // chunks per plane run
  return (ch * width * height + unit * 256u) * esize + (c - ch * per) * 16u;
}

#endif
