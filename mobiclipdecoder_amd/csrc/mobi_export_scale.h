// mobi_export_scale.h -- geometry of the scaled RGB export (mobi_batch_export_device_scaled; the kernel is mobi_export_scale.hip): a crop
// (cx, cy, cw, ch) of the picture, area-averaged down to ow x oh (ow <= cw, oh <= ch), exactly, in integers.
//
// Weights, per axis (in_n source samples -> out_n outputs, out_n <= in_n): on a line of in_n * out_n units source s is [s * out_n,
// (s + 1) * out_n) and output o is [o * in_n, (o + 1) * in_n); the weight of s in o is the length of their overlap,
//   w(o, s) = max(0, min((s + 1) * out_n, (o + 1) * in_n) - max(s * out_n, o * in_n)).
// A source is no longer than an output, so it meets at most two: o = s * out_n / in_n with w = min(out_n, (o + 1) * in_n - s * out_n),
// and o + 1 with the rest, out_n - w (mobi_scale_tap).  An output's weights sum to in_n, a source's to out_n.
//   S = sum_t sum_s wy(oy, t) * wx(ox, s) * v[cy + t][cx + s],  D = cw * ch,  q = (S + D / 2) / D  (floor; v = one byte of the Bitmap's word)
// S + D / 2 < 2^31 while D <= 2^23: 32-bit accumulators, and an exact division by the per-call constant D (mobi_scale_div).
//
// Work split (mobi_scale_plan): a workgroup takes one picture, one BAND of `band_rows` output rows and one STRIP of `strip_w` output
// columns (a multiple of 4; one strip unless ow > 512), and keeps band_rows x 3 x strip_w 32-bit sums in LDS.  It converts the source
// rows and columns that have weight in them (mobi_scale_span), so a source row two bands share is converted by both.
// __host__ __device__ (MOBI_TILE_FN): the kernel and the CPU test (tests/test_export_scaled.py) compile this code.
#ifndef MOBI_EXPORT_SCALE_H
#define MOBI_EXPORT_SCALE_H
#include <stddef.h>
#include <stdint.h>

#include "mobi_tile.h"

// w(o, s) above
MOBI_TILE_FN uint32_t mobi_scale_weight(uint32_t o, uint32_t s, uint32_t out_n, uint32_t in_n) {
  const uint64_t s0 = (uint64_t)s * out_n, s1 = s0 + out_n, o0 = (uint64_t)o * in_n, o1 = o0 + in_n;
  const uint64_t lo = s0 > o0 ? s0 : o0, hi = s1 < o1 ? s1 : o1;
  return hi > lo ? (uint32_t)(hi - lo) : 0u;
}
// source s: the first output it has weight in, and that weight; the rest, out_n - *w (zero or not), is output *o + 1's
MOBI_TILE_FN void mobi_scale_tap(uint32_t s, uint32_t out_n, uint32_t in_n, uint32_t *o, uint32_t *w) {
  uint32_t q, left; // left = (q + 1) * in_n - s * out_n, in 1 .. in_n
  if (in_n <= 0xFFFFu) { // (s * out_n < in_n^2 fits 32 bits: every realistic picture; the other branch is 64-bit division)
    const uint32_t pos = s * out_n;
    q = pos / in_n;
    left = in_n - (pos - q * in_n);
  } else {
    const uint64_t pos = (uint64_t)s * out_n;
    q = (uint32_t)(pos / in_n);
    left = in_n - (uint32_t)(pos - (uint64_t)q * in_n);
  }
  *o = q;
  *w = left < out_n ? left : out_n;
}
// the sources [*s0, *s1) that have weight in outputs [o0, o1)
MOBI_TILE_FN void mobi_scale_span(uint32_t o0, uint32_t o1, uint32_t out_n, uint32_t in_n, uint32_t *s0, uint32_t *s1) {
  *s0 = (uint32_t)((uint64_t)o0 * in_n / out_n);
  *s1 = (uint32_t)(((uint64_t)o1 * in_n + out_n - 1u) / out_n);
}

// n / d for n < 2^31 by a multiplication: m = ceil(2^sh / d), sh = 31 + ceil(log2 d); 2^sh <= m * d <= 2^sh + 2^(sh - 31), which makes
// floor(m * n / 2^sh) the quotient for every n < 2^31 (Granlund & Montgomery 1994, theorem 4.2).  d >= 1; m < 2^32.
struct MobiScaleDiv { uint32_t m, sh; };
MOBI_TILE_FN MobiScaleDiv mobi_scale_div_make(uint32_t d) {
  uint32_t l = 0;
  while (((uint64_t)1 << l) < d) l++;
  MobiScaleDiv k;
  k.sh = 31u + l;
  k.m = (uint32_t)((((uint64_t)1 << k.sh) + d - 1u) / d);
  return k;
}
MOBI_TILE_FN uint32_t mobi_scale_div(uint32_t n, MobiScaleDiv k) { return (uint32_t)(((uint64_t)n * k.m) >> k.sh); }

// One call's geometry, as the kernel gets it.
struct MobiScalePlan {
  uint32_t cx, cy, cw, ch, ow, oh;
  uint32_t strip_w, n_strips; // output columns per workgroup (a multiple of 4), strips per row
  uint32_t band_rows, n_bands; // output rows per workgroup, bands per picture
  uint32_t half;               // D / 2
  MobiScaleDiv div;            // by D = cw * ch
};
constexpr uint32_t kMobiScaleStripMax = 512u;     // output columns of one strip at most
constexpr uint32_t kMobiScaleLdsBytes = 20480u;   // of sums per workgroup at most (one row of a strip is at most 6 KiB): 7 workgroups per CU
constexpr uint32_t kMobiScaleBandPixels = 16384u; // source pixels per workgroup aimed at: 256 lanes x 8 pixels x 8 turns
MOBI_TILE_FN MobiScalePlan mobi_scale_plan(uint32_t cx, uint32_t cy, uint32_t cw, uint32_t ch, uint32_t ow, uint32_t oh) {
  MobiScalePlan p;
  p.cx = cx; p.cy = cy; p.cw = cw; p.ch = ch; p.ow = ow; p.oh = oh;
  p.strip_w = ow < kMobiScaleStripMax ? ow : kMobiScaleStripMax;
  p.n_strips = (ow + p.strip_w - 1u) / p.strip_w;
  // rows: what fits the LDS budget, and no more than gives the workgroup its share of source pixels (small outputs of large pictures
  // would otherwise be a handful of workgroups)
  const uint32_t by_lds = kMobiScaleLdsBytes / (12u * p.strip_w);
  const uint64_t src_per_row = ((uint64_t)p.strip_w * cw / ow) * ch / oh; // source pixels under one output row of a strip, about
  const uint32_t by_work = (uint32_t)(kMobiScaleBandPixels / (src_per_row ? src_per_row : 1u));
  uint32_t r = by_lds < by_work ? by_lds : by_work;
  if (r > oh) r = oh;
  if (r < 1u) r = 1u;
  p.band_rows = r;
  p.n_bands = (oh + r - 1u) / r;
  p.half = cw * ch / 2u;
  p.div = mobi_scale_div_make(cw * ch);
  return p;
}
MOBI_TILE_FN uint32_t mobi_scale_lds_bytes(const MobiScalePlan *p) { return p->band_rows * 3u * p->strip_w * 4u; }
// workgroup (band, strip): its output rows [*r0, *r1) and columns [*c0, *c1)
MOBI_TILE_FN void mobi_scale_tile(const MobiScalePlan *p, uint32_t band, uint32_t strip, uint32_t *r0, uint32_t *r1, uint32_t *c0, uint32_t *c1) {
  *r0 = band * p->band_rows;
  *r1 = *r0 + p->band_rows < p->oh ? *r0 + p->band_rows : p->oh;
  *c0 = strip * p->strip_w;
  *c1 = *c0 + p->strip_w < p->ow ? *c0 + p->strip_w : p->ow;
}
// bytes of one output picture
MOBI_TILE_FN size_t mobi_scale_picture_bytes(uint32_t ow, uint32_t oh, uint32_t esize) { return (size_t)3u * ow * oh * esize; }

#endif
