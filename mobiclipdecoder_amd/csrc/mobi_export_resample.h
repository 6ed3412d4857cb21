// mobi_export_resample.h -- geometry of the resampled RGB export (mobi_batch_export_device_boxes; the kernel is mobi_export_resample.hip):
// a box (x, y, w, h) of the picture PER CLIP, resized to ow x oh, mirrored or not, exactly, in integers.
//
// Per axis (in_n source samples -> out_n outputs) a weight matrix W[o][s] whose rows sum to a denominator d:
//   out_n <= in_n, AREA:    W = mobi_scale_weight (mobi_export_scale.h), d = in_n.  The sources of output o are the run
//                           [floor(o * in_n / out_n), ceil((o + 1) * in_n / out_n)): the first and the last are cut by the output's edges, the
//                           ones between them lie inside it and weigh out_n each.
//   out_n >  in_n, LINEAR:  sample centres aligned, clamped at the BOX's edge: n = (2 o + 1) in_n - out_n, i0 = floor(n / (2 out_n)),
//                           f = n - i0 * 2 out_n; 2 out_n - f goes to source clamp(i0), f to clamp(i0 + 1); d = 2 out_n.  One tap where both
//                           clamp to one source or f = 0, two otherwise.
// Both kinds are therefore a RUN of sources with a first, a middle and a last weight (MobiAxisTap): the kernel gathers over runs and does not
// know the kind.  Runs move right with o, so the sources of outputs [o0, o1) are first(o0) .. end(o1 - 1) (mobi_axis_span), tight.
//   S = sum_t sum_s Wy[oy][t] * Wx[ox][s] * v[y + t][x + s],  D = dx * dy,  q = (S + D / 2) / D  (floor);  S + D / 2 < 2^31 while D <= 2^23.
//
// Work split (mobi_resample_plan, per clip): a workgroup of 256 lanes takes one picture, a BAND of `band_rows` output rows and a STRIP of
// `strip_w` output columns (a multiple of 4), strip_w / 4 * band_rows <= 256: in the end a lane owns 4 consecutive outputs of one row and
// their 12 sums are registers.  The sources of the tile are walked in CHUNKS of chunk_rows x chunk_cols (whole row pairs, whole groups of 4
// columns of the PICTURE) that fit the LDS budget: converted to RGB words [chunk_rows][chunk_cols], summed along x into
// [chunk_rows][3][strip_w] and from there, weighted along y, into the lanes' sums.  Large ratios are more chunks, not more LDS.
// The grid of a call is the largest tiling of its clips; a workgroup past a clip's own tiling leaves (mobi_resample_tile returns false).
// __host__ __device__ (MOBI_TILE_FN): the kernel and the CPU test (tests/test_export_resampled.py) compile this code.
#ifndef MOBI_EXPORT_RESAMPLE_H
#define MOBI_EXPORT_RESAMPLE_H
#include <stddef.h>
#include <stdint.h>

#include "mobi_export_scale.h"

#define MOBI_RESAMPLE_FLIP_X 1u // MOBI_BOX_FLIP_X of include/mobiclip_hip.h

enum { MOBI_AXIS_AREA = 0, MOBI_AXIS_LINEAR = 1 };
MOBI_TILE_FN int mobi_axis_kind(uint32_t out_n, uint32_t in_n) { return out_n > in_n ? MOBI_AXIS_LINEAR : MOBI_AXIS_AREA; }
// d: what a row of W sums to
MOBI_TILE_FN uint32_t mobi_axis_den(uint32_t out_n, uint32_t in_n) { return out_n > in_n ? 2u * out_n : in_n; }

// a / b for a < 2^63, b < 2^32, by a 32-bit division where the dividend allows it (it does for every realistic picture)
MOBI_TILE_FN uint32_t mobi_axis_udiv(uint64_t a, uint32_t b) { return (a >> 32) ? (uint32_t)(a / b) : (uint32_t)a / b; }

// The sources of one output: `count` of them from `first` on (1 <= count, first + count <= in_n); the first weighs wf, the last (count >= 2)
// wl, the ones between them wm.
struct MobiAxisTap { uint32_t first, count, wf, wm, wl; };
MOBI_TILE_FN MobiAxisTap mobi_axis_tap(uint32_t o, uint32_t out_n, uint32_t in_n) {
  MobiAxisTap t;
  if (out_n <= in_n) {
    const uint64_t lo = (uint64_t)o * in_n, hi = lo + in_n;
    t.first = mobi_axis_udiv(lo, out_n);
    const uint32_t end = mobi_axis_udiv(hi + out_n - 1u, out_n);
    t.count = end - t.first;
    t.wf = mobi_scale_weight(o, t.first, out_n, in_n);
    t.wm = out_n;
    t.wl = mobi_scale_weight(o, end - 1u, out_n, in_n);
    return t;
  }
  const uint32_t d = 2u * out_n;
  const int64_t n = (int64_t)(2u * (uint64_t)o + 1u) * in_n - (int64_t)out_n; // > -out_n: i0 >= -1
  t.wm = 0;
  if (n < 0) { // i0 = -1: both taps clamp to source 0
    t.first = 0; t.count = 1; t.wf = d; t.wl = d;
    return t;
  }
  const uint32_t i0 = mobi_axis_udiv((uint64_t)n, d), f = (uint32_t)((uint64_t)n - (uint64_t)i0 * d); // i0 <= in_n - 1
  t.first = i0;
  if (f == 0u || i0 + 1u >= in_n) { t.count = 1; t.wf = d; t.wl = d; }
  else { t.count = 2; t.wf = d - f; t.wl = f; }
  return t;
}
// weight of the run's k-th source (k < count)
MOBI_TILE_FN uint32_t mobi_axis_tap_weight(const MobiAxisTap *t, uint32_t k) { return k == 0u ? t->wf : k + 1u == t->count ? t->wl : t->wm; }
// the sources [*s0, *s1) that have weight in outputs [o0, o1), o0 < o1
MOBI_TILE_FN void mobi_axis_span(uint32_t o0, uint32_t o1, uint32_t out_n, uint32_t in_n, uint32_t *s0, uint32_t *s1) {
  const MobiAxisTap a = mobi_axis_tap(o0, out_n, in_n), b = mobi_axis_tap(o1 - 1u, out_n, in_n);
  *s0 = a.first;
  *s1 = b.first + b.count;
}
// no n consecutive outputs have more sources than this (area: ceil(n in / out) + 1; linear: the first taps move by at most
// ceil((n - 1) in / out), and the last output has two)
MOBI_TILE_FN uint32_t mobi_axis_span_max(uint32_t n, uint32_t out_n, uint32_t in_n) {
  const uint32_t s = mobi_axis_udiv((uint64_t)n * in_n + out_n - 1u, out_n) + (out_n > in_n ? 2u : 1u);
  return s < in_n ? s : in_n;
}

// One clip of a call, as the kernel reads it from device memory (a parameter block of the exporter, mobi_export.cpp): 64 bytes.
struct MobiResampleClip {
  uint32_t x, y, w, h, flags;     // the box inside the picture; MOBI_RESAMPLE_FLIP_X
  uint32_t strip_w, n_strips;     // output columns per workgroup (a multiple of 4), strips per row
  uint32_t band_rows, n_bands;    // output rows per workgroup, bands per picture: strip_w / 4 * band_rows <= 256
  uint32_t chunk_rows, chunk_cols; // source rows (even) and columns (a multiple of 4) converted at a time
  uint32_t half;                  // D / 2
  MobiScaleDiv div;               // by D = dx * dy
  uint32_t start;                 // the clip sink's schedule (mobi_sink.h): the step of the clip's first picture; the exports leave it 0
  uint32_t pad;
};
constexpr uint32_t kMobiResampleLanes = 256u;
constexpr uint32_t kMobiResampleStripMax = 64u;      // output columns of one strip at most
constexpr uint32_t kMobiResampleLdsBytes = 20480u;   // per workgroup at most: 7 workgroups per CU
constexpr uint32_t kMobiResampleTilePixels = 16384u; // source pixels per workgroup aimed at
// D = dx * dy of a box and an output size (64-bit: the caller refuses D > 2^23)
MOBI_TILE_FN uint64_t mobi_resample_den(uint32_t w, uint32_t h, uint32_t ow, uint32_t oh) {
  return (uint64_t)mobi_axis_den(ow, w) * mobi_axis_den(oh, h);
}
// LDS of a workgroup: the column runs of the strip [strip_w] (MobiAxisTap without wm: 16 bytes), the RGB words and the sums along x
MOBI_TILE_FN uint32_t mobi_resample_lds_bytes(const MobiResampleClip *k) {
  return 16u * k->strip_w + k->chunk_rows * (4u * k->chunk_cols + 12u * k->strip_w);
}
// D <= 2^23; ow a multiple of 4
MOBI_TILE_FN MobiResampleClip mobi_resample_plan(uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t flags, uint32_t ow, uint32_t oh) {
  MobiResampleClip k;
  k.x = x; k.y = y; k.w = w; k.h = h; k.flags = flags;
  // strips of equal width, 64 columns at most
  k.n_strips = (ow + kMobiResampleStripMax - 1u) / kMobiResampleStripMax;
  k.strip_w = ((ow + k.n_strips - 1u) / k.n_strips + 3u) & ~3u;
  k.n_strips = (ow + k.strip_w - 1u) / k.strip_w;
  // rows: one lane per 4 outputs, and no more than gives the workgroup its share of source pixels (small outputs of large boxes would
  // otherwise be a handful of workgroups); bands of equal height
  const uint32_t span_w = mobi_axis_span_max(k.strip_w < ow ? k.strip_w : ow, ow, w);
  const uint32_t by_lanes = kMobiResampleLanes / (k.strip_w >> 2);
  const uint64_t src_per_row = (uint64_t)span_w * mobi_axis_span_max(1u, oh, h);
  const uint32_t by_work = (uint32_t)(kMobiResampleTilePixels / src_per_row);
  uint32_t r = by_lanes < by_work ? by_lanes : by_work;
  if (r > oh) r = oh;
  if (r < 1u) r = 1u;
  k.n_bands = (oh + r - 1u) / r;
  k.band_rows = (oh + k.n_bands - 1u) / k.n_bands;
  k.n_bands = (oh + k.band_rows - 1u) / k.band_rows;
  // chunks: the tile's span widened to the picture's groups of 4 columns and row pairs, cut to the budget (at least one row pair)
  const uint32_t budget = kMobiResampleLdsBytes - 16u * k.strip_w, hrow = 12u * k.strip_w;
  const uint32_t cols_max = ((budget / 2u - hrow) / 4u) & ~3u;
  uint32_t cc = (span_w + 6u) & ~3u; // (a span of n columns lies in at most (n + 6) / 4 groups)
  if (cc > cols_max) cc = cols_max;
  k.chunk_cols = cc;
  const uint32_t span_h = mobi_axis_span_max(k.band_rows, oh, h);
  uint32_t cr = (budget / (4u * cc + hrow)) & ~1u, need = (span_h + 2u) & ~1u;
  if (cr > need) cr = need;
  k.chunk_rows = cr;
  const uint64_t D = mobi_resample_den(w, h, ow, oh);
  k.half = (uint32_t)(D / 2u);
  k.div = mobi_scale_div_make((uint32_t)D);
  k.start = k.pad = 0u;
  return k;
}
MOBI_TILE_FN uint32_t mobi_resample_blocks(const MobiResampleClip *k) { return k->n_bands * k->n_strips; }
// workgroup `block` of a picture of this clip: false when the clip's tiling has no such workgroup, else its output rows [*r0, *r1) and
// columns [*c0, *c1) (before the flip)
MOBI_TILE_FN bool mobi_resample_tile(const MobiResampleClip *k, uint32_t ow, uint32_t oh, uint32_t block, uint32_t *r0, uint32_t *r1, uint32_t *c0,
                                     uint32_t *c1) {
  if (block >= k->n_bands * k->n_strips) return false;
  const uint32_t band = block / k->n_strips, strip = block - band * k->n_strips;
  *r0 = band * k->band_rows;
  *r1 = *r0 + k->band_rows < oh ? *r0 + k->band_rows : oh;
  *c0 = strip * k->strip_w;
  *c1 = *c0 + k->strip_w < ow ? *c0 + k->strip_w : ow;
  return true;
}

#endif
