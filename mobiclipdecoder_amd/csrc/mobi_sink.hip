// mobi_sink.hip -- mobi_sink: the pictures one frame step contributes to a clip tensor (mobi_batch_set_sink): a box per clip of the step's
// ring slot, resized, mirrored or not, written where picture t of clip c lies in an (N, T, ...) tensor of any of the sink's layouts.
// The schedule is on the device: the per-clip record (mobi_export_resample.h), uploaded once at arming, holds `start`, the launch carries
// the step, the temporal stride, T and the three strides (mobi_sink.h), and a workgroup whose clip contributes nothing in this step leaves
// at once -- no per-step transfer.  What a workgroup does with its tile is mobi_resample_body.h's, the body mobi_export_resample runs:
// the same gather, sums, division, affine, flip and stores of 4 consecutive elements per lane, whole runs of an output row per wave.
// Templated on layout (planar / packed) x element (uint8 / float16 / float32).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobi_resample_body.h"
#include "mobi_sink.h"

namespace {
using namespace mobi_resample_body;
} // namespace

// Workgroup blockIdx.x of the tiling of clip c = clip0 + blockIdx.y (a partial launch -- a repair -- carries its first clip and, in the
// grid, its clip count), whose record is clips[c].  The source is ring slot `slot` of the clip, the step's one picture.  Dynamic LDS: the
// largest mobi_resample_lds_bytes of the batch's clips.
template <int PLANAR, int ESIZE>
__global__ __launch_bounds__(kMobiResampleLanes) void mobi_sink(const uint8_t *planes, uint64_t clip_bytes, uint32_t slot_bytes, int width, int height, int lgS,
                                                                int version, int clip0, int slot, uint32_t ow, uint32_t oh,
                                                                const MobiResampleClip *__restrict__ clips, MobiSinkSched sch, MobiRgbAffine sb, uint8_t *out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const uint32_t c = (uint32_t)clip0 + blockIdx.y;
  const MobiResampleClip k = clips[c];
  const int32_t t = mobi_sink_select(sch.step, k.start, sch.stride, sch.n_frames);
  if (t < 0) return; // (not this clip's step: the whole workgroup leaves)
  uint32_t r0, r1, c0, c1;
  if (!mobi_resample_tile(&k, ow, oh, blockIdx.x, &r0, &r1, &c0, &c1)) return; // (a smaller clip's tiling: the whole workgroup leaves)
  const uint8_t *Y = planes + (size_t)c * clip_bytes + (size_t)slot * slot_bytes;
  const StridedDst<ESIZE> dst{out + mobi_sink_picture(&sch, c, t) * ESIZE, ow, sch.chan_stride};
  tile<PLANAR, ESIZE>(lds, Y, Y + ((size_t)height << lgS), k, r0, r1, c0, c1, width, height, lgS, version, ow, oh, sb, dst);
}

// clips [clip0, clip0 + n_clips) of the batch, one picture each at most; 65535 clips per launch (blockIdx.y)
extern "C" int mobi_launch_sink(const MobiExportGeom *g, int version, int planar, int esize, const MobiResampleCall *call, int slot, int clip0, int n_clips,
                                const MobiSinkSched *sch, const MobiRgbAffine *sb, uint8_t *out_dev, hipStream_t s) {
  return launch_pictures(planar, esize, 1, n_clips, [&](auto pl, auto es, uint32_t p0, uint32_t n) {
    hipLaunchKernelGGL((mobi_sink<decltype(pl)::value, decltype(es)::value>), dim3(call->blocks, n), dim3(kLanes), call->lds_bytes, s, g->planes, g->clip_bytes,
                       g->slot_bytes, g->width, g->height, g->lg, version, clip0 + (int)p0, slot, call->ow, call->oh, call->clips_dev, *sch, *sb, out_dev);
  });
}
