// mobi_export_tensor.h -- what the RGB tensor export kernels share (mobi_export_rgb.hip, mobi_export_scale.hip, mobi_export_resample.hip
// include it): the picture of an export and its ring slot, the Bitmap's words of 4 pixels of two rows fetched from the tiled planes, the
// store of 1, 2 or 4 words, and the launch over layout x element.  The per-pixel arithmetic is
// mobi_rgb.h's, each kernel's geometry its own header's.
#ifndef MOBI_EXPORT_TENSOR_H
#define MOBI_EXPORT_TENSOR_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mobi_rgb.h"
#include "mobi_tile.h"

namespace mobi_export_tensor {
using namespace mobi_rgb;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Picture p of an export: frame j = p / n_clips (ring slot (slot0 + j) % 6), clip clip0 + c with c = p % n_clips; Y, UV = the tiled planes
// of that slot.
struct Picture {
  const uint8_t *Y, *UV;
  uint32_t c;
};
__device__ __forceinline__ Picture picture(const uint8_t *planes, uint64_t clip_bytes, uint32_t slot_bytes, int height, int lgS, int n_clips, int clip0,
                                           int slot0, uint32_t p) {
  const uint32_t j = p / (uint32_t)n_clips, c = p - j * (uint32_t)n_clips;
  const uint8_t *Y = planes + (size_t)(clip0 + c) * clip_bytes + (size_t)((slot0 + j) % 6u) * slot_bytes;
  return Picture{Y, Y + ((size_t)height << lgS), c};
}

// The Bitmap's words of pixels x0 .. x0 + 3 (x0 a multiple of 4) of the even row y0 (pe) and the row below it (po); x0 + 3 < width and
// y0 + 1 < height.  The lane shape of the Bitmap kernel (mobi_rgb.h, convert_quad), fetched from the tiled planes.
__device__ __forceinline__ void fetch_quad(const uint8_t *Y, const uint8_t *UV, uint32_t x0, uint32_t y0, int width, int height, int lgS, int version,
                                           uint32_t (&pe)[4], uint32_t (&po)[4]) {
  const bool lastcol = x0 + 4u >= (uint32_t)width, lastrow = y0 + 2u >= (uint32_t)height;
  // luma column; chroma: samples a, b under the pixels (two bytes of one tile row) and e right of them (the next tile's for a = 6)
  const uint32_t ycol = mobi_ty_col(x0), ccol = mobi_tc_x(x0 >> 1), ecol = lastcol ? ccol : mobi_tc_x((x0 >> 1) + 2u);
  const uint8_t *yp = Y + mobi_ty_row(y0, lgS) + ycol; // rows y0, y0 + 1 are the two rows of one chunk
  const uint32_t yw0 = *(const uint32_t *)yp, yw1 = *(const uint32_t *)(yp + 8);
  const uint8_t *c0p = UV + mobi_tc_row(y0 >> 1, lgS), *c1p = lastrow ? c0p : UV + mobi_tc_row((y0 >> 1) + 1u, lgS);
  const uint32_t u0w = *(const uint16_t *)(c0p + ccol), v0w = *(const uint16_t *)(c0p + ccol + 8);
  const uint32_t u1w = *(const uint16_t *)(c1p + ccol), v1w = *(const uint16_t *)(c1p + ccol + 8);
  const uint32_t ue0 = c0p[ecol], ve0 = c0p[ecol + 8], ue1 = c1p[ecol], ve1 = c1p[ecol + 8]; // (not looked at in the last column)
  convert_quad(version, yw0, yw1, u0w, ue0, u1w, ue1, v0w, ve0, v1w, ve1, lastrow, lastcol, pe, po);
}

// W words (4 * W bytes, aligned to that) in one store
template <int W>
__device__ __forceinline__ void store_words(uint8_t *d, const uint32_t *w) {
  if (W == 1) *(uint32_t *)d = w[0];
  else if (W == 2) *(u32x2 *)d = u32x2{w[0], w[1]};
  else *(u32x4 *)d = u32x4{w[0], w[1], w[2], w[3]};
}
// The launches of an export of n_frames x n_clips pictures: launch(planar, esize, p0, n) enqueues the kernel of that layout and element
// size (std::integral_constant: template arguments) for pictures p0 .. p0 + n - 1, which go in blockIdx.y: one launch up to 65535 of them
// (more are several launches of that many).  -> the first error, as a hipError_t
template <class L>
int launch_pictures(int planar, int esize, int n_frames, int n_clips, const L &launch) {
  if (esize != 1 && esize != 2 && esize != 4) return (int)hipErrorInvalidValue;
  const uint32_t n_pics = (uint32_t)n_frames * (uint32_t)n_clips;
  using std::integral_constant;
  for (uint32_t p0 = 0; p0 < n_pics; p0 += 65535u) {
    const uint32_t n = n_pics - p0 < 65535u ? n_pics - p0 : 65535u;
    if (planar) {
      if (esize == 1) launch(integral_constant<int, 1>{}, integral_constant<int, 1>{}, p0, n);
      else if (esize == 2) launch(integral_constant<int, 1>{}, integral_constant<int, 2>{}, p0, n);
      else launch(integral_constant<int, 1>{}, integral_constant<int, 4>{}, p0, n);
    } else {
      if (esize == 1) launch(integral_constant<int, 0>{}, integral_constant<int, 1>{}, p0, n);
      else if (esize == 2) launch(integral_constant<int, 0>{}, integral_constant<int, 2>{}, p0, n);
      else launch(integral_constant<int, 0>{}, integral_constant<int, 4>{}, p0, n);
    }
    if (hipError_t e = hipGetLastError()) return (int)e;
  }
  return 0;
}
} // namespace mobi_export_tensor

#endif
