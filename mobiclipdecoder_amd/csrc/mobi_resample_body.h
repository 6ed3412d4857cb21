// mobi_resample_body.h -- the workgroup body the resampling kernels share (mobi_export_resample.hip: pictures of the ring, picture after
// picture; mobi_sink.hip: the pictures a frame step contributes to a clip tensor): one tile of one picture of one clip -- the gather, the
// two weighted sums, the exact division, the affine, the flip and the stores.  The geometry is mobi_export_resample.h's, the division
// mobi_export_scale.h's, the per-pixel arithmetic mobi_rgb.h's.  Where the tile's elements go is the caller's: a destination policy.
//
// A workgroup (4 waves) takes one picture, one band of output rows and one strip of output columns of ITS CLIP's tiling: the record is read
// once, from device memory, and everything derived from it -- weights, spans, loop counts -- is uniform over the workgroup.  It gathers:
//   1. a chunk of the source rows and columns that have weight in the tile is converted in the Bitmap kernel's lane shape -- 4 pixels of two
//      rows per lane, fetch_quad (mobi_export_tensor.h) -- into RGB words in LDS;
//   2. a lane per (source row, output column) sums its column run of those words, weighted, into sums along x in LDS (a lane owns its sums:
//      no atomics);
//   3. a lane per 4 consecutive outputs of a row adds its row run of the sums along x, weighted, to 12 sums in registers.
// After the last chunk the lanes divide by the clip's D exactly, apply the affine, mirror their store address when the clip is flipped, and
// store 4 consecutive elements of a row each: a wave writes whole runs of the output rows.  No full-size RGB leaves the workgroup, and
// nothing but the output is written to global memory.  Integer sums: the result does not depend on the order of execution.
#ifndef MOBI_RESAMPLE_BODY_H
#define MOBI_RESAMPLE_BODY_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobi_export_resample.h"
#include "mobi_export_tensor.h"
#include "mobi_exporter.h"

namespace mobi_resample_body {
using namespace mobi_export_tensor;
constexpr uint32_t kLanes = kMobiResampleLanes;

// task tid, tid + 256, ... of a list of rows x n tasks as (row, column): the first one, and the step without a division per task
struct Walk {
  uint32_t row, col, drow, dcol, n;
  __device__ __forceinline__ Walk(uint32_t tid, uint32_t n_) : n(n_) {
    row = tid / n; col = tid - row * n;
    drow = kLanes / n; dcol = kLanes - drow * n;
  }
  __device__ __forceinline__ void next() {
    row += drow; col += dcol;
    if (col >= n) { col -= n; row++; }
  }
};

// Destination policies: where output row R, column col (the first of a lane's 4) of a picture goes.  planar(ch, R, col) is channel ch's
// plane, packed(R, col) the pixel's three elements.
// pictures of oh x ow, the channel planes back to back (the exports: picture p at out + p * picture_bytes)
template <int ESIZE>
struct DenseDst {
  uint8_t *pic;
  uint32_t ow, oh;
  __device__ __forceinline__ uint8_t *planar(int ch, size_t R, size_t col) const { return pic + ((ch * (size_t)oh + R) * ow + col) * ESIZE; }
  __device__ __forceinline__ uint8_t *packed(size_t R, size_t col) const { return pic + (R * ow + col) * 3u * ESIZE; }
};
// the same with the channel planes chan_stride elements apart (the clip sink: mobi_sink.h)
template <int ESIZE>
struct StridedDst {
  uint8_t *pic;
  uint32_t ow;
  int64_t chan_stride;
  __device__ __forceinline__ uint8_t *planar(int ch, size_t R, size_t col) const { return pic + (ch * chan_stride + (int64_t)(R * ow + col)) * ESIZE; }
  __device__ __forceinline__ uint8_t *packed(size_t R, size_t col) const { return pic + (R * ow + col) * 3u * ESIZE; }
};

// The tile [r0, r1) x [c0, c1) (mobi_resample_tile) of clip record k's picture in the tiled planes Y / UV -> dst.  lds: the workgroup's
// dynamic LDS (mobi_resample_lds_bytes of the record at least).  Called by every lane of the workgroup.
template <int PLANAR, int ESIZE, class Dst>
__device__ __forceinline__ void tile(uint32_t *lds, const uint8_t *srcY, const uint8_t *srcUV, const MobiResampleClip &k, uint32_t r0, uint32_t r1, uint32_t c0,
                                     uint32_t c1, int width, int height, int lgS, int version, uint32_t ow, uint32_t oh, const MobiRgbAffine &sb, const Dst &dst) {
  const uint32_t tid = threadIdx.x;
  const uint32_t rows = r1 - r0, sw = c1 - c0, nq = sw >> 2;
  u32x4 *coltap = (u32x4 *)lds;                       // [strip_w] first, count, wf, wl of the strip's outputs
  uint32_t *rgb = lds + 4u * k.strip_w;               // [chunk_rows][chunk_cols] the Bitmap's words
  uint32_t *hs = rgb + k.chunk_rows * k.chunk_cols;   // [chunk_rows][3][strip_w] sums along x

  for (uint32_t i = tid; i < sw; i += kLanes) {
    const MobiAxisTap t = mobi_axis_tap(c0 + i, ow, k.w);
    coltap[i] = u32x4{t.first, t.count, t.wf, t.wl};
  }
  // this lane's outputs: columns c0 + q4 .. + 3 of row r0 + orow (lanes past the tile own nothing)
  const bool owner = tid < rows * nq;
  const uint32_t orow = owner ? tid / nq : 0u, q4 = owner ? (tid - orow * nq) * 4u : 0u;
  const MobiAxisTap rt = mobi_axis_tap(r0 + orow, oh, k.h);
  uint32_t acc[3][4] = {};

  // the source rows and columns with weight in this tile, widened to whole row pairs and groups of 4 columns of the PICTURE (parity and
  // the chroma neighbours are the picture's); what the widening adds is in no run
  uint32_t t0, t1, s0, s1;
  mobi_axis_span(r0, r1, oh, k.h, &t0, &t1);
  mobi_axis_span(c0, c1, ow, k.w, &s0, &s1);
  const uint32_t py0 = (k.y + t0) & ~1u, py1 = (k.y + t1 + 1u) & ~1u;
  const uint32_t px0 = (k.x + s0) & ~3u, px1 = (k.x + s1 + 3u) & ~3u;
  for (uint32_t ra = py0; ra < py1; ra += k.chunk_rows) { // (every loop bound here is uniform over the workgroup)
    const uint32_t rb = ra + k.chunk_rows < py1 ? ra + k.chunk_rows : py1, nrows = rb - ra;
    for (uint32_t ca = px0; ca < px1; ca += k.chunk_cols) {
      const uint32_t cb = ca + k.chunk_cols < px1 ? ca + k.chunk_cols : px1, groups = (cb - ca) >> 2;
      if (ca != px0) __syncthreads(); // (step 2 has read the last column chunk's words; between row chunks the barrier of step 3 stands)
      // 1. rows ra .. rb - 1, columns ca .. cb - 1 -> rgb
      Walk w1(tid, groups);
      for (uint32_t i = tid; i < (nrows >> 1) * groups; i += kLanes, w1.next()) {
        const uint32_t x0 = ca + 4u * w1.col, y0 = ra + 2u * w1.row; // x0 + 3 < width, y0 + 1 < height: both are multiples of 16
        uint32_t pe[4], po[4];
        fetch_quad(srcY, srcUV, x0, y0, width, height, lgS, version, pe, po);
        uint32_t *d = rgb + 2u * w1.row * k.chunk_cols + 4u * w1.col;
        *(u32x4 *)d = u32x4{pe[0], pe[1], pe[2], pe[3]};
        *(u32x4 *)(d + k.chunk_cols) = u32x4{po[0], po[1], po[2], po[3]};
      }
      __syncthreads();
      // 2. (source row, output column): the part of the column's run inside [ca, cb), weighted, into hs (set by the first column chunk)
      Walk w2(tid, sw);
      for (uint32_t i = tid; i < nrows * sw; i += kLanes, w2.next()) {
        const u32x4 t = coltap[w2.col];
        const uint32_t base = k.x + t.x; // the picture column of the run's first source
        const uint32_t ka = base < ca ? ca - base : 0u, kb = cb > base ? (cb - base < t.y ? cb - base : t.y) : 0u;
        const uint32_t *src = rgb + w2.row * k.chunk_cols;
        uint32_t s[3] = {0u, 0u, 0u};
        for (uint32_t kk = ka; kk < kb; kk++) {
          const uint32_t w = kk == 0u ? t.z : kk + 1u == t.y ? t.w : ow, word = src[base + kk - ca]; // (a run of 3 or more is an area run: wm = ow)
#pragma unroll
          for (int ch = 0; ch < 3; ch++) s[ch] += w * ((word >> (16 - 8 * ch)) & 0xFFu); // R = byte 2, G = byte 1, B = byte 0
        }
        uint32_t *h = hs + w2.row * 3u * k.strip_w + w2.col;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) h[ch * k.strip_w] = ca == px0 ? s[ch] : h[ch * k.strip_w] + s[ch];
      }
      if (ca + k.chunk_cols < px1) continue; // (more column chunks of these rows)
      __syncthreads();
      // 3. this lane's outputs: the part of its row run inside [ra, rb), weighted
      if (owner) {
        const uint32_t base = k.y + rt.first;
        const uint32_t ka = base < ra ? ra - base : 0u, kb = rb > base ? (rb - base < rt.count ? rb - base : rt.count) : 0u;
        for (uint32_t kk = ka; kk < kb; kk++) {
          const uint32_t w = kk == 0u ? rt.wf : kk + 1u == rt.count ? rt.wl : oh;
          const uint32_t *h = hs + (base + kk - ra) * 3u * k.strip_w + q4;
#pragma unroll
          for (int ch = 0; ch < 3; ch++) {
            const u32x4 v = *(const u32x4 *)(h + ch * k.strip_w);
#pragma unroll
            for (int t = 0; t < 4; t++) acc[ch][t] += w * v[t];
          }
        }
      }
    }
  }
  if (!owner) return;

  // q = (S + D / 2) / D, the element, and stores of 4 * ESIZE bytes (planar, per channel) or 3 of them (packed) that continue the
  // neighbouring lanes'.  A flipped clip: output column ox holds the q of column ow - 1 - ox, so the 4 go, reversed, to ow - 4 - col.
  const bool flip = (k.flags & MOBI_RESAMPLE_FLIP_X) != 0u;
  constexpr int per = 4 / ESIZE; // elements per 32-bit word
  uint32_t q[3][4];
#pragma unroll
  for (int ch = 0; ch < 3; ch++)
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const uint32_t a = flip ? acc[ch][3 - t] : acc[ch][t];
      q[ch][t] = tensor_element<ESIZE>(mobi_scale_div(a + k.half, k.div), ch, sb.v);
    }
  const size_t R = r0 + orow, col = flip ? ow - 4u - (c0 + q4) : c0 + q4;
  if (PLANAR) {
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      uint32_t w[ESIZE];
#pragma unroll
      for (int n = 0; n < ESIZE; n++) {
        w[n] = 0;
#pragma unroll
        for (int e = 0; e < per; e++) w[n] |= q[ch][n * per + e] << (8 * ESIZE * e);
      }
      store_words<ESIZE>(dst.planar(ch, R, col), w);
    }
  } else {
    uint32_t w[3 * ESIZE];
#pragma unroll
    for (int n = 0; n < 3 * ESIZE; n++) {
      w[n] = 0;
#pragma unroll
      for (int e = 0; e < per; e++) {
        const int kk = n * per + e; // pixel kk / 3, channel kk % 3
        w[n] |= q[kk % 3][kk / 3] << (8 * ESIZE * e);
      }
    }
    uint8_t *d = dst.packed(R, col);
#pragma unroll
    for (int n = 0; n < 3; n++) store_words<ESIZE>(d + 4 * ESIZE * n, w + ESIZE * n);
  }
}
} // namespace mobi_resample_body

#endif
