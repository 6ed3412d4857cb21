// mobi_export_rgb.hip -- mobi_export_rgb: ring slots of many clips x frames -> RGB tensors in device memory, every picture of an export in
// one launch (mobi_batch_export_device; the addressing is mobi_export_rgb.h's, the arithmetic mobi_rgb.h's).  Templated on layout (planar
// CHW / packed HWC) x element (uint8 / float16 / float32).
//
// The values are the Bitmap's: each pixel's 0xAARRGGBB word comes out of convert2 exactly as in mobi_yuv_to_argb, and R, G, B are its
// bytes 2, 1, 0.  uint8 stores them as they are; float32 is (float)v * scale[ch] + bias[ch], a product and a sum rounded one after the
// other (contraction is off: mobi_rgb.h); float16 is that float32 value rounded to nearest-even.
//
// HBM-bound: 1.5 bytes read and 3 * esize written per pixel.  A wave puts its unit's elements into LDS in output order and then stores the
// 768 * esize bytes as 16-byte chunks, lane by lane: runs of 256 bytes or more per store instruction in every layout (mobi_export_rgb.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobi_export_rgb.h"
#include "mobi_export_tensor.h"
#include "mobi_exporter.h"

namespace {
using namespace mobi_export_tensor;

// Element k (0 .. 11) of the lane's four pixels in output order -- planar: channel ch's pixels t = 0 .. 3 (k = t, per plane); packed:
// pixel k / 3, channel k % 3 -- as the bits of one element of ESIZE bytes (mobi_rgb.h, tensor_element).
template <int ESIZE>
__device__ __forceinline__ uint32_t element(const uint32_t (&argb)[4], int t, int ch, const MobiRgbAffine &sb) {
  return tensor_element<ESIZE>((argb[t] >> (16 - 8 * ch)) & 0xFFu, ch, sb.v); // R = byte 2, G = byte 1, B = byte 0
}
} // namespace

// Units kUnitsPerWave * blockIdx.x .. + kUnitsPerWave - 1 of picture p = p0 + blockIdx.y of the export: frame j = p / n_clips (ring slot
// (slot0 + j) % 6), clip clip0 + p % n_clips; it goes to out + p * picture_bytes.  One wave per block.  With one unit per wave the kernel ran
// at the rate the GPU starts workgroups (~1.6 G per second, the Bitmap kernel's rate too, which converts twice the pixels per wave).
constexpr uint32_t kUnitsPerWave = 4;
template <int PLANAR, int ESIZE, bool NT>
__global__ __launch_bounds__(64) void mobi_export_rgb(const uint8_t *planes, uint64_t clip_bytes, uint32_t slot_bytes, int width, int height,
                                                     int lgS, int version, int n_clips, int clip0, int slot0, uint32_t p0, MobiRgbAffine sb,
                                                     uint8_t *out) {
  __shared__ u32x4 stage[48 * ESIZE]; // the unit's output bytes, in output order
  const uint32_t p = p0 + blockIdx.y, lane = threadIdx.x;
  const Picture src = picture(planes, clip_bytes, slot_bytes, height, lgS, n_clips, clip0, slot0, p);
  const uint8_t *Y = src.Y, *UV = src.UV;
  uint8_t *pic = out + (size_t)p * mobi_rgb_picture_bytes((uint32_t)width, (uint32_t)height, ESIZE);
  const uint32_t u0 = blockIdx.x * kUnitsPerWave, units = mobi_rgb_units((uint32_t)width, (uint32_t)height);
  const uint32_t u1 = u0 + kUnitsPerWave < units ? u0 + kUnitsPerWave : units;
  for (uint32_t unit = u0; unit < u1; unit++) { // (wave-uniform)
    MobiRgbSrc s;
    mobi_rgb_lane(unit, lane, (uint32_t)width, (uint32_t)height, lgS, &s);
    const uint32_t yw = *(const uint32_t *)(Y + s.luma);
    const u32x4 k0 = *(const u32x4 *)(UV + s.c0), k1 = *(const u32x4 *)(UV + s.c1);
    const u32x4 m0 = *(const u32x4 *)(UV + s.n0), m1 = *(const u32x4 *)(UV + s.n1); // (the same chunks again unless s.next: a cache hit)
    // samples a, b (byte 0, 1) and e (byte 0) of U and V in both rows; e is the sample two to the right of a, in the next tile for sel 6
    const uint32_t sh = 8u * s.sel;
    auto half = [&](uint32_t lo, uint32_t hi, uint32_t nx, uint32_t &w, uint32_t &e) {
      const uint64_t h = (uint64_t)lo | (uint64_t)hi << 32;
      w = (uint32_t)(h >> sh);
      e = s.sel == 6u ? nx : (uint32_t)(h >> (sh + 16u));
    };
    uint32_t uw0, ue0, vw0, ve0, uw1, ue1, vw1, ve1;
    half(k0.x, k0.y, m0.x, uw0, ue0);
    half(k0.z, k0.w, m0.z, vw0, ve0);
    half(k1.x, k1.y, m1.x, uw1, ue1);
    half(k1.z, k1.w, m1.z, vw1, ve1);
    int ue[4], uo[4], ve[4], vo[4];
    chroma_numerators(uw0, ue0, uw1, ue1, s.lastrow, s.lastcol, ue, uo);
    chroma_numerators(vw0, ve0, vw1, ve1, s.lastrow, s.lastcol, ve, vo);
    const int *un = s.odd ? uo : ue, *vn = s.odd ? vo : ve;
    uint32_t argb[4];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const f32x2 y2 = {(float)((yw >> (16 * k)) & 0xFF), (float)((yw >> (16 * k + 8)) & 0xFF)};
      convert2(version, y2, un[2 * k], un[2 * k + 1], vn[2 * k], vn[2 * k + 1], argb[2 * k], argb[2 * k + 1]);
    }
    // the lane's 12 elements into the staging image, as 32-bit words (4 / ESIZE elements each)
    uint32_t *st = (uint32_t *)stage;
    constexpr int per = 4 / ESIZE;
    if (PLANAR) {
#pragma unroll
      for (int ch = 0; ch < 3; ch++)
#pragma unroll
        for (int w = 0; w < ESIZE; w++) {
          uint32_t word = 0;
#pragma unroll
          for (int i = 0; i < per; i++) word |= element<ESIZE>(argb, w * per + i, ch, sb) << (8 * ESIZE * i);
          st[mobi_rgb_stage_off(1, ESIZE, lane, 0, ch) / 4u + w] = word;
        }
    } else {
#pragma unroll
      for (int w = 0; w < 3 * ESIZE; w++) {
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < per; i++) {
          const int k = w * per + i;
          word |= element<ESIZE>(argb, k / 3, k % 3, sb) << (8 * ESIZE * i);
        }
        st[mobi_rgb_stage_off(0, ESIZE, lane, 0, 0) / 4u + w] = word;
      }
    }
    __syncthreads(); // (one wave per block: a wait for the LDS writes, no barrier)
#pragma unroll
    for (uint32_t k = lane; k < 48u * ESIZE; k += 64u) {
      const u32x4 v = stage[k];
      u32x4 *d = (u32x4 *)(pic + mobi_rgb_chunk_dst(PLANAR, ESIZE, (uint32_t)width, (uint32_t)height, unit, k));
      if (NT) __builtin_nontemporal_store(v, d);
      else *d = v;
    }
    __syncthreads(); // (the next unit writes the staging image again: every lane has read this one)
  }
}

extern "C" int mobi_launch_export_rgb(const MobiExportGeom *g, int version, int planar, int esize, int nontemporal, int n_frames, int n_clips,
                                      int clip0, int slot0, const MobiRgbAffine *sb, uint8_t *out_dev, hipStream_t s) {
  const uint32_t waves = (mobi_rgb_units((uint32_t)g->width, (uint32_t)g->height) + kUnitsPerWave - 1) / kUnitsPerWave;
  return launch_pictures(planar, esize, n_frames, n_clips, [&](auto pl, auto es, uint32_t p0, uint32_t n) {
    constexpr int PLANAR = decltype(pl)::value, ESIZE = decltype(es)::value;
    const auto kernel = nontemporal ? mobi_export_rgb<PLANAR, ESIZE, true> : mobi_export_rgb<PLANAR, ESIZE, false>;
    hipLaunchKernelGGL(kernel, dim3(waves, n), dim3(64), 0, s, g->planes, g->clip_bytes, g->slot_bytes, g->width, g->height, g->lg, version, n_clips, clip0,
                       slot0, p0, *sb, out_dev);
  });
}
