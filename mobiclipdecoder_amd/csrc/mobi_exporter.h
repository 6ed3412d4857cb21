// mobi_exporter.h -- interface between the C-ABI layer (mobi_abi.cpp) and the export of decoded pictures to host memory (mobi_export.cpp,
// mobi_export.hip; include/mobiclip_hip.h, mobi_batch_export).  The C entry points check their arguments against the batch and hand over
// what the export needs of it; the export's state (streams, staging chunks, tickets, the ring-slot guard) lives in a MobiExporter.
#ifndef MOBI_EXPORTER_H
#define MOBI_EXPORTER_H
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <functional>

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
int mobi_exporter_wait(MobiExporter *x, uint64_t ticket);
int mobi_exporter_query(MobiExporter *x, uint64_t ticket);
// the ring-slot guard: before a step that writes ring slot `slot` is enqueued on `stream`, it waits for the last pack that read that slot --
// if one may still be running.  No export outstanding: nothing at all (no event, no wait).
int mobi_exporter_guard(MobiExporter *x, int slot, hipStream_t stream);
// is [p, p + bytes) inside one block of mobi_host_alloc?
bool mobi_host_registered(const void *p, size_t bytes);
#endif
#endif
