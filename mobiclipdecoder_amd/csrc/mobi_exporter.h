// mobi_exporter.h -- interface between the C-ABI layer (mobi_pictures.cpp) and the export of decoded pictures to host and device memory
// (mobi_export.cpp, mobi_export*.hip; include/mobiclip_hip.h, mobi_batch_export*).  The C entry points check their arguments against the batch
// and hand over what the export needs of it; the export's state (streams, staging chunks, parameter blocks, tickets, the ring-slot guard)
// lives in a MobiExporter.
#ifndef MOBI_EXPORTER_H
#define MOBI_EXPORTER_H
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <functional>

#include "mobi_export_resample.h"
#include "mobi_export_scale.h"
#include "mobi_sink.h"

// the ring of one batch as the export reads it (MobiReconArgs' layout: [clip][slot 0..5][tiled Y | tiled UV])
struct MobiExportGeom {
  const uint8_t *planes;
  uint64_t clip_bytes;
  uint32_t slot_bytes;
  int width, height, stride, mbw, lg;
};

// mobi_export.hip: pictures q0 .. q0 + n_pics - 1 of an export of clips [clip0, clip0 + n_clips) (picture q = frame q / n_clips, ring slot
// (slot0 + that) % 6, clip clip0 + q % n_clips) -> out_dev, packed I420, picture after picture
extern "C" int mobi_launch_export_i420(const MobiExportGeom *g, uint32_t q0, int n_pics, int n_clips, int clip0, int slot0, uint8_t *out_dev,
                                       hipStream_t s);

// mobi_export_rgb.hip: the pictures of an export (n_frames x n_clips, picture q = frame q / n_clips, clip clip0 + q % n_clips) -> out_dev as
// RGB tensors: planar (CHW) or packed (HWC), esize 1 (uint8), 2 (float16) or 4 (float32); sb = scale[3], bias[3] (float only); nontemporal:
// the stores go past the caches
struct MobiRgbAffine { float v[6]; };
extern "C" int mobi_launch_export_rgb(const MobiExportGeom *g, int version, int planar, int esize, int nontemporal, int n_frames, int n_clips,
                                      int clip0, int slot0, const MobiRgbAffine *sb, uint8_t *out_dev, hipStream_t s);

// mobi_export_scale.hip: the same pictures, the crop and output size of `plan` (mobi_export_scale.h), area-averaged: RGB tensors of
// plan->ow x plan->oh
extern "C" int mobi_launch_export_scale(const MobiExportGeom *g, int version, int planar, int esize, const MobiScalePlan *plan, int n_frames,
                                        int n_clips, int clip0, int slot0, const MobiRgbAffine *sb, uint8_t *out_dev, hipStream_t s);

// mobi_export_resample.hip: the same pictures, a box per clip resized to ow x oh (mobi_export_resample.h).  clips_dev = n_clips records in
// DEVICE memory (a parameter block of the exporter); blocks = the largest mobi_resample_blocks, lds_bytes the largest mobi_resample_lds_bytes
// of them
struct MobiResampleCall {
  uint32_t ow, oh, blocks, lds_bytes;
  const MobiResampleClip *clips_dev;
};
extern "C" int mobi_launch_export_resample(const MobiExportGeom *g, int version, int planar, int esize, const MobiResampleCall *call, int n_frames,
                                           int n_clips, int clip0, int slot0, const MobiRgbAffine *sb, uint8_t *out_dev, hipStream_t s);

// mobi_sink.hip: the pictures the step in ring slot `slot` contributes to a clip tensor (mobi_sink.h), of clips [clip0, clip0 + n_clips) of
// the batch.  call->clips_dev = the records of ALL the batch's clips (record c is clip c's, with its `start`), call->blocks and
// call->lds_bytes the largest of them
extern "C" int mobi_launch_sink(const MobiExportGeom *g, int version, int planar, int esize, const MobiResampleCall *call, int slot, int clip0, int n_clips,
                                const MobiSinkSched *sch, const MobiRgbAffine *sb, uint8_t *out_dev, hipStream_t s);

#if !defined(__HIPCC__) || !defined(__HIP_DEVICE_COMPILE__)
struct MobiExporter;
// one export of a checked request (mobi_batch_export).  slot0 = the ring slot of the OLDEST frame (ring index ring_idx); frame j is slot
// (slot0 + j) % 6.  argb(clip0, n, slot, out, stream) launches the Bitmap conversion of n clips of one slot (mobi_launch_argb).
// run(n, f) runs f(0 .. n - 1) on the batch's host threads (ParsePool).
struct MobiExportJob {
  MobiExportGeom g;
  int format, n_frames, clip0, n_clips, slot0;
  void *dst;
  hipStream_t src_stream; // the batch's stream: the export goes behind everything enqueued on it
  std::function<int(int clip0, int n, int slot, uint32_t *out, hipStream_t s)> argb;
  std::function<void(int, const std::function<void(int)> &)> run;
};
MobiExporter *mobi_exporter_new(int device);
void mobi_exporter_delete(MobiExporter *x); // waits for every export outstanding
int mobi_exporter_run(MobiExporter *x, const MobiExportJob &job, uint64_t *ticket_out);
// one export into device memory on the caller's stream (mobi_batch_export_device): `stream` waits for job.src_stream through an event,
// launch(stream) enqueues the kernels, and every ring slot read is armed in the guard with an event recorded on `stream` behind them.  No
// staging, no ticket.  On an error after something was enqueued the call waits for `stream` before it returns.
// params (optional): per-call data the kernels read from device memory.  `bytes` bytes at `host` are copied, before the call returns, into
// the pinned side of a PARAMETER BLOCK (a pinned host buffer, a device buffer and an event; a small pool, mobi_export.cpp) and from there
// to the device on `stream`, in front of launch(), which finds the device address in `dev`; the block is taken again once the event
// recorded behind the launch has completed.  No host wait, and no allocation once the pool has a free block of that size.
struct MobiExportParams {
  const void *host;
  size_t bytes;
  const void *dev; // set for launch()
};
int mobi_exporter_run_device(MobiExporter *x, const MobiExportJob &job, hipStream_t stream, const std::function<int(hipStream_t)> &launch,
                             MobiExportParams *params = nullptr);
int mobi_exporter_wait(MobiExporter *x, uint64_t ticket);
int mobi_exporter_query(MobiExporter *x, uint64_t ticket);
// the ring-slot guard: before a step that writes ring slot `slot` is enqueued on `stream`, it waits for every export that read that slot
// and may still be running -- host exports' packs and device exports on callers' streams alike.  No export outstanding: nothing at all
// (no event, no wait).
int mobi_exporter_guard(MobiExporter *x, int slot, hipStream_t stream);
// is any export outstanding: a ticket not complete yet, or a ring slot some export may still be reading?  (mobi_batch_set_motion)
bool mobi_exporter_busy(MobiExporter *x);
// is [p, p + bytes) inside one block of mobi_host_alloc?
bool mobi_host_registered(const void *p, size_t bytes);
#endif
#endif
