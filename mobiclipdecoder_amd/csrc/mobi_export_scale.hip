// mobi_export_scale.hip -- mobi_export_scale: a crop of the ring slots of many clips x frames, area-averaged down to RGB tensors of
// out_w x out_h in device memory, every picture of an export in one launch (mobi_batch_export_device_scaled; the weights, the work split
// and the division are mobi_export_scale.h's, the per-pixel arithmetic mobi_rgb.h's).  Templated on layout (planar CHW / packed HWC) x
// element (uint8 / float16 / float32), as mobi_export_rgb is.
//
// A workgroup (4 waves) takes one picture, one band of output rows and one strip of output columns.  It converts the source pixels that
// have weight in them in the Bitmap kernel's lane shape -- 4 pixels of two rows per lane, fetch_quad (mobi_export_tensor.h) -- and adds
// weight * byte into 32-bit sums [row][channel][column] in LDS.  Integer sums commute: the result does not depend on the order of the adds.
// A lane is a group of 4 source columns (its column weights are computed once) and a wave walks the row pairs (the row weights are
// wave-uniform); the two rows of a pair are combined per output row before the column weights are applied.  After a barrier the lanes
// divide by D exactly, apply the affine and store 4 consecutive elements of a row each: a wave writes whole runs of the output rows.
// No full-size RGB leaves the registers, and nothing but the output is written to global memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobi_export_scale.h"
#include "mobi_export_tensor.h"
#include "mobi_exporter.h"

namespace {
using namespace mobi_export_tensor;
constexpr uint32_t kWaves = 4;

__device__ __forceinline__ void lds_add(uint32_t *p, uint32_t v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); // ds_add_u32, no return value
}
} // namespace

// Band blockIdx.x / n_strips and strip blockIdx.x % n_strips of picture p = p0 + blockIdx.y of the export: frame j = p / n_clips (ring slot
// (slot0 + j) % 6), clip clip0 + p % n_clips; it goes to out + p * picture_bytes.  Dynamic LDS: mobi_scale_lds_bytes(&k).
template <int PLANAR, int ESIZE>
__global__ __launch_bounds__(64 * kWaves) void mobi_export_scale(const uint8_t *planes, uint64_t clip_bytes, uint32_t slot_bytes, int width, int height,
                                                                 int lgS, int version, int n_clips, int clip0, int slot0, uint32_t p0, MobiScalePlan k,
                                                                 MobiRgbAffine sb, uint8_t *out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t acc[]; // sums [rows][3][sw]
  const uint32_t p = p0 + blockIdx.y, tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const Picture src = picture(planes, clip_bytes, slot_bytes, height, lgS, n_clips, clip0, slot0, p);
  uint8_t *pic = out + (size_t)p * mobi_scale_picture_bytes(k.ow, k.oh, ESIZE);
  const uint32_t band = blockIdx.x / k.n_strips, strip = blockIdx.x - band * k.n_strips;
  uint32_t r0, r1, c0, c1;
  mobi_scale_tile(&k, band, strip, &r0, &r1, &c0, &c1);
  const uint32_t rows = r1 - r0, sw = c1 - c0;
  for (uint32_t i = tid; i < rows * 3u * sw; i += 64u * kWaves) acc[i] = 0u;
  __syncthreads();

  // the source rows and columns with weight in this tile, widened to whole row pairs and groups of 4 columns of the PICTURE (parity and
  // the chroma neighbours are the picture's); what the widening adds gets weight 0
  uint32_t t0, t1, s0, s1;
  mobi_scale_span(r0, r1, k.oh, k.ch, &t0, &t1);
  mobi_scale_span(c0, c1, k.ow, k.cw, &s0, &s1);
  const uint32_t py0 = (k.cy + t0) & ~1u, py1 = k.cy + t1, pairs = (py1 - py0 + 1u) >> 1;
  const uint32_t px0 = (k.cx + s0) & ~3u, px1 = k.cx + s1, groups = (px1 - px0 + 3u) >> 2;
  for (uint32_t g0 = 0; g0 < groups; g0 += 64u) { // (wave-uniform)
    const bool active = g0 + lane < groups;
    const uint32_t x0 = px0 + 4u * (active ? g0 + lane : 0u); // (a lane past the last group converts the first one and adds nothing)
    // pixel x0 + t: sum column ia and weight wa, and the next column ib with the rest of the weight, wb (0: nothing to add)
    uint32_t ia[4], wa[4], ib[4], wb[4];
#pragma unroll
    for (uint32_t t = 0; t < 4; t++) {
      const uint32_t x = x0 + t;
      const bool in = active && x >= k.cx + s0 && x < px1;
      uint32_t o, w;
      mobi_scale_tap(in ? x - k.cx : s0, k.ow, k.cw, &o, &w);
      const bool a_ok = in && o >= c0, b_ok = in && w < k.ow && o + 1u >= c0 && o + 1u < c1; // (o < c1: x is inside the span)
      ia[t] = a_ok ? o - c0 : 0u;
      wa[t] = a_ok ? w : 0u;
      ib[t] = b_ok ? o + 1u - c0 : 0u;
      wb[t] = b_ok ? k.ow - w : 0u;
    }
    for (uint32_t rp = wave; rp < pairs; rp += kWaves) { // (wave-uniform)
      const uint32_t y0 = py0 + 2u * rp; // even; y0 + 1 < height
      uint32_t pe[4], po[4];
      fetch_quad(src.Y, src.UV, x0, y0, width, height, lgS, version, pe, po);
      // the rows' weights (wave-uniform): row y has a in sum row R and b in R + 1; a row outside the span has none
      auto row_tap = [&](uint32_t y, uint32_t &R, uint32_t &a, uint32_t &b) {
        const bool in = y >= k.cy + t0 && y < py1;
        uint32_t o, w;
        mobi_scale_tap(in ? y - k.cy : t0, k.oh, k.ch, &o, &w);
        R = o;
        a = in ? w : 0u;
        b = in ? k.oh - w : 0u;
        return in;
      };
      uint32_t Re, ae, be, Ro, ao, bo;
      const bool in_e = row_tap(y0, Re, ae, be), in_o = row_tap(y0 + 1u, Ro, ao, bo);
      if (!in_e) Re = Ro;
      if (!in_o) Ro = Re; // (one of the two is inside; Re <= Ro <= Re + 1)
#pragma unroll
      for (uint32_t dr = 0; dr < 3u; dr++) { // the pair has weight in sum rows Re .. Re + 2 at most
        const uint32_t R = Re + dr;
        const uint32_t we = R == Re ? ae : R == Re + 1u ? be : 0u, wo = R == Ro ? ao : R == Ro + 1u ? bo : 0u;
        if ((we | wo) == 0u || R < r0 || R >= r1) continue; // (wave-uniform)
        uint32_t *row = acc + (R - r0) * 3u * sw;
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
          for (int ch = 0; ch < 3; ch++) { // R = byte 2, G = byte 1, B = byte 0
            const uint32_t v = we * ((pe[t] >> (16 - 8 * ch)) & 0xFFu) + wo * ((po[t] >> (16 - 8 * ch)) & 0xFFu);
            if (wa[t]) lds_add(row + ch * sw + ia[t], v * wa[t]);
            if (wb[t]) lds_add(row + ch * sw + ib[t], v * wb[t]);
          }
      }
    }
  }
  __syncthreads();

  // 4 consecutive columns of one row per lane: q = (S + D / 2) / D, the element, and stores of 4 * ESIZE bytes (planar, per channel) or
  // 3 of them (packed) that continue the neighbouring lanes'
  const uint32_t nq = sw >> 2;
  constexpr int per = 4 / ESIZE; // elements per 32-bit word
  for (uint32_t i = tid; i < rows * nq; i += 64u * kWaves) {
    const uint32_t r = i / nq, q4 = (i - r * nq) * 4u;
    uint32_t q[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const u32x4 s = *(const u32x4 *)(acc + (r * 3u + ch) * sw + q4);
#pragma unroll
      for (int t = 0; t < 4; t++) q[ch][t] = tensor_element<ESIZE>(mobi_scale_div(s[t] + k.half, k.div), ch, sb.v);
    }
    const size_t R = r0 + r, col = c0 + q4;
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
        store_words<ESIZE>(pic + ((ch * (size_t)k.oh + R) * k.ow + col) * ESIZE, w);
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
      uint8_t *d = pic + (R * k.ow + col) * 3u * ESIZE;
#pragma unroll
      for (int n = 0; n < 3; n++) store_words<ESIZE>(d + 4 * ESIZE * n, w + ESIZE * n);
    }
  }
}

extern "C" int mobi_launch_export_scale(const MobiExportGeom *g, int version, int planar, int esize, const MobiScalePlan *plan, int n_frames,
                                        int n_clips, int clip0, int slot0, const MobiRgbAffine *sb, uint8_t *out_dev, hipStream_t s) {
  return launch_pictures(planar, esize, n_frames, n_clips, [&](auto pl, auto es, uint32_t p0, uint32_t n) {
    hipLaunchKernelGGL((mobi_export_scale<decltype(pl)::value, decltype(es)::value>), dim3(plan->n_bands * plan->n_strips, n), dim3(64 * kWaves),
                       mobi_scale_lds_bytes(plan), s, g->planes, g->clip_bytes, g->slot_bytes, g->width, g->height, g->lg, version, n_clips, clip0, slot0, p0,
                       *plan, *sb, out_dev);
  });
}
