// mobi_export.hip -- mobi_export_i420: ring slots of many clips x frames -> packed I420 pictures in a device staging chunk, in one launch
// (mobi_batch_export; the addressing is mobi_export.h's).  Pure data movement: 1.5 bytes read and 1.5 written per pixel.  The staging
// chunk is read by the copy engine alone, so the stores go past the caches (__builtin_nontemporal_store).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobi_export.h"
#include "mobi_exporter.h"

namespace {
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
} // namespace

// Picture p of the launch (blockIdx.x / blocks_per_pic) is picture q = q0 + p of the export: frame j = q / n_clips (ring slot
// (slot0 + j) % 6), clip clip0 + q % n_clips; it goes to out + p * picture_bytes.
extern "C" __global__ __launch_bounds__(256) void mobi_export_i420(const uint8_t *planes, uint64_t clip_bytes, uint32_t slot_bytes, int width,
                                                                  int height, int mbw, int lgS, uint32_t blocks_per_pic, uint32_t q0,
                                                                  int n_clips, int clip0, int slot0, uint8_t *out) {
  const uint32_t p = blockIdx.x / blocks_per_pic, L = (blockIdx.x - p * blocks_per_pic) * 256u + threadIdx.x;
  if (L >= mobi_export_lanes((uint32_t)height, (uint32_t)mbw)) return;
  const uint32_t q = q0 + p, j = q / (uint32_t)n_clips, c = q - j * (uint32_t)n_clips;
  const uint8_t *slot = planes + (size_t)(clip0 + c) * clip_bytes + (size_t)((slot0 + j) % 6u) * slot_bytes;
  uint8_t *pic = out + (size_t)p * mobi_export_i420_bytes((uint32_t)width, (uint32_t)height);
  uint32_t src[2], dst[2];
  if (mobi_export_lane(L, (uint32_t)width, (uint32_t)height, (uint32_t)mbw, lgS, src, dst)) {
    const u32x2 a = *(const u32x2 *)(slot + src[0]), b = *(const u32x2 *)(slot + src[1]);
    __builtin_nontemporal_store(u32x4{a.x, a.y, b.x, b.y}, (u32x4 *)(pic + dst[0]));
  } else {
    const u32x4 uv = *(const u32x4 *)(slot + src[0]);
    __builtin_nontemporal_store(u32x2{uv.x, uv.y}, (u32x2 *)(pic + dst[0]));
    __builtin_nontemporal_store(u32x2{uv.z, uv.w}, (u32x2 *)(pic + dst[1]));
  }
}

extern "C" int mobi_launch_export_i420(const MobiExportGeom *g, uint32_t q0, int n_pics, int n_clips, int clip0, int slot0, uint8_t *out_dev,
                                       hipStream_t s) {
  if (n_pics <= 0) return 0;
  const uint32_t bpp = (mobi_export_lanes((uint32_t)g->height, (uint32_t)g->mbw) + 255u) / 256u;
  hipLaunchKernelGGL(mobi_export_i420, dim3(bpp * (uint32_t)n_pics), dim3(256), 0, s, g->planes, g->clip_bytes, g->slot_bytes, g->width, g->height,
                     g->mbw, g->lg, bpp, q0, n_clips, clip0, slot0, out_dev);
  return (int)hipGetLastError();
}
