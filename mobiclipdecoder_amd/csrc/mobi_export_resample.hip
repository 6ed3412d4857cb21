// mobi_export_resample.hip -- mobi_export_resample: a box PER CLIP of the ring slots of many clips x frames, resized (area-averaged down,
// linearly interpolated up, per axis) to RGB tensors of out_w x out_h in device memory, mirrored or not, every picture of an export in one
// launch (mobi_batch_export_device_boxes; the weights, the per-clip record and the work split are mobi_export_resample.h's, the division
// mobi_export_scale.h's, the per-pixel arithmetic mobi_rgb.h's).  Templated on layout (planar CHW / packed HWC) x element (uint8 / float16 /
// float32), as mobi_export_scale is.
//
// What a workgroup does with its tile -- gather, weighted sums, division, affine, flip, stores -- is mobi_resample_body.h's, shared with the
// clip sink (mobi_sink.hip); here is which picture a workgroup takes and where that picture lies: picture after picture, dense.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobi_resample_body.h"

namespace {
using namespace mobi_resample_body;
} // namespace

// Workgroup blockIdx.x of the tiling of picture p = p0 + blockIdx.y of the export: frame j = p / n_clips (ring slot (slot0 + j) % 6), clip
// clip0 + p % n_clips, whose record is clips[p % n_clips]; it goes to out + p * picture_bytes.  Dynamic LDS: the largest
// mobi_resample_lds_bytes of the call's clips.
template <int PLANAR, int ESIZE>
__global__ __launch_bounds__(kMobiResampleLanes) void mobi_export_resample(const uint8_t *planes, uint64_t clip_bytes, uint32_t slot_bytes, int width,
                                                                           int height, int lgS, int version, int n_clips, int clip0, int slot0,
                                                                           uint32_t p0, uint32_t ow, uint32_t oh, const MobiResampleClip *__restrict__ clips,
                                                                           MobiRgbAffine sb, uint8_t *out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const uint32_t p = p0 + blockIdx.y;
  const Picture src = picture(planes, clip_bytes, slot_bytes, height, lgS, n_clips, clip0, slot0, p);
  const MobiResampleClip k = clips[src.c];
  uint32_t r0, r1, c0, c1;
  if (!mobi_resample_tile(&k, ow, oh, blockIdx.x, &r0, &r1, &c0, &c1)) return; // (a smaller clip's tiling: the whole workgroup leaves)
  const DenseDst<ESIZE> dst{out + (size_t)p * mobi_scale_picture_bytes(ow, oh, ESIZE), ow, oh};
  tile<PLANAR, ESIZE>(lds, src.Y, src.UV, k, r0, r1, c0, c1, width, height, lgS, version, ow, oh, sb, dst);
}

extern "C" int mobi_launch_export_resample(const MobiExportGeom *g, int version, int planar, int esize, const MobiResampleCall *call, int n_frames,
                                           int n_clips, int clip0, int slot0, const MobiRgbAffine *sb, uint8_t *out_dev, hipStream_t s) {
  return launch_pictures(planar, esize, n_frames, n_clips, [&](auto pl, auto es, uint32_t p0, uint32_t n) {
    hipLaunchKernelGGL((mobi_export_resample<decltype(pl)::value, decltype(es)::value>), dim3(call->blocks, n), dim3(kLanes), call->lds_bytes, s, g->planes,
                       g->clip_bytes, g->slot_bytes, g->width, g->height, g->lg, version, n_clips, clip0, slot0, p0, call->ow, call->oh, call->clips_dev, *sb,
                       out_dev);
  });
}
