// mobi_sink.h -- the clip sink (mobi_batch_set_sink; the kernel is mobi_sink.hip, the host side mobi_sink.cpp): which clips contribute a
// picture in a frame step, and where every element of that picture goes.  Once, for host and device: mobi_sink_plan and the kernel call
// the same functions, and the CPU test (tests/test_sink.py) compiles this header with the host compiler.
//
// Steps count the frame steps a batch runs after arming, from 0.  Clip c contributes picture t (0 <= t < T) at step start[c] + t * stride.
// Element (c, t, ch, y, x) of the tensor, in ELEMENTS from dst:
//   planar   c * clip_stride + t * frame_stride + ch * chan_stride + y * out_w + x
//   packed   c * clip_stride + t * frame_stride + (y * out_w + x) * 3 + ch                      (chan_stride == 0)
// __host__ __device__ (MOBI_TILE_FN).
#ifndef MOBI_SINK_H
#define MOBI_SINK_H
#include <stddef.h>
#include <stdint.h>

#include "mobi_tile.h"

// what a launch carries beside the per-clip records (which hold the box, the tiling and `start`)
struct MobiSinkSched {
  int64_t step;                                    // the step whose pictures the launch reads
  int32_t stride, n_frames;                        // s, T
  int64_t clip_stride, frame_stride, chan_stride;  // in elements
};

// the picture clip `start` contributes in `step`: t, or -1 for none
MOBI_TILE_FN int32_t mobi_sink_select(int64_t step, uint32_t start, int32_t stride, int32_t n_frames) {
  const int64_t d = step - (int64_t)start;
  if (d < 0 || d > (int64_t)(n_frames - 1) * stride) return -1;
  const uint32_t u = (uint32_t)d, t = u / (uint32_t)stride; // ((T - 1) * stride < 2^31: mobi_sink_check)
  return t * (uint32_t)stride == u ? (int32_t)t : -1;
}
// the first element of picture (c, t)
MOBI_TILE_FN int64_t mobi_sink_picture(const MobiSinkSched *s, uint32_t c, int32_t t) { return (int64_t)c * s->clip_stride + (int64_t)t * s->frame_stride; }
// element (ch, y, x) inside a picture
MOBI_TILE_FN int64_t mobi_sink_element(int planar, int64_t chan_stride, uint32_t ow, uint32_t ch, uint32_t y, uint32_t x) {
  return planar ? (int64_t)ch * chan_stride + (int64_t)y * ow + x : ((int64_t)y * ow + x) * 3 + ch;
}
// elements from a picture's first to one past its last
MOBI_TILE_FN int64_t mobi_sink_picture_span(int planar, int64_t chan_stride, uint32_t ow, uint32_t oh) {
  return planar ? 2 * chan_stride + (int64_t)oh * ow : (int64_t)oh * ow * 3;
}
// a + b * c without leaving int64: false when it would
MOBI_TILE_FN bool mobi_sink_madd(int64_t a, int64_t b, int64_t c, int64_t *out) {
  int64_t p;
  return !__builtin_mul_overflow(b, c, &p) && !__builtin_add_overflow(a, p, out);
}
// Do the pictures of n_clips x n_frames lie inside `cap` elements without touching each other?  The (extent, stride) pairs -- clips, frames,
// and for planar tensors the three channels -- ordered by stride: every stride is at least the span of everything with a smaller stride
// (the innermost thing is a plane of oh x ow elements, packed oh x ow x 3), and the whole span fits.  Every stride a multiple of 4.
// *span_out: the elements from dst the sink may write (one past the last).
MOBI_TILE_FN bool mobi_sink_layout_ok(int planar, uint32_t n_clips, int32_t n_frames, uint32_t ow, uint32_t oh, int64_t clip_stride, int64_t frame_stride,
                                      int64_t chan_stride, uint64_t cap, int64_t *span_out) {
  int64_t ext[3] = {(int64_t)n_clips, (int64_t)n_frames, 3}, str[3] = {clip_stride, frame_stride, chan_stride};
  const int np = planar ? 3 : 2;
  if (!planar && chan_stride != 0) return false;
  for (int i = 0; i < np; i++)
    if (str[i] < 0 || (str[i] & 3)) return false;
  for (int i = 1; i < np; i++) // (three entries: an insertion sort by stride)
    for (int j = i; j > 0 && str[j] < str[j - 1]; j--) {
      const int64_t e = ext[j], s = str[j];
      ext[j] = ext[j - 1]; str[j] = str[j - 1];
      ext[j - 1] = e; str[j - 1] = s;
    }
  int64_t span = (int64_t)oh * ow * (planar ? 1 : 3);
  for (int i = 0; i < np; i++) {
    if (str[i] < span) return false;
    if (!mobi_sink_madd(span, ext[i] - 1, str[i], &span)) return false;
  }
  if ((uint64_t)span > cap) return false;
  if (span_out) *span_out = span;
  return true;
}

#endif
