// mobi_sink.cpp -- the clip sink's host side (include/mobiclip_hip.h, mobi_batch_set_sink): the checks, arming and disarming, the host-only
// plan, and the launch behind a frame step (mobi_batch::sink_step).  Selection and addresses are mobi_sink.h's, for host and device alike;
// the kernel is mobi_sink.hip, its body mobi_resample_body.h's.
#include "mobi_batch.h"

namespace {
size_t sink_esize(const mobi_sink *s) {
  if (s->format != MOBI_EXPORT_RGB_PLANAR && s->format != MOBI_EXPORT_RGB_PACKED) return 0;
  if (s->dtype == MOBI_DTYPE_U8) return s->scale_bias ? 0 : 1;
  return s->dtype == MOBI_DTYPE_F16 ? 2 : s->dtype == MOBI_DTYPE_F32 ? 4 : 0;
}
// clip c's box {x, y, w, h, flags}: the spec's row, or the whole picture
void sink_box(const mobi_sink *s, int c, uint32_t width, uint32_t height, int64_t bx[5]) {
  if (s->boxes) for (int i = 0; i < 5; i++) bx[i] = s->boxes[5 * (size_t)c + i];
  else { bx[0] = bx[1] = bx[4] = 0; bx[2] = width; bx[3] = height; }
}
bool sink_schedule_ok(const mobi_sink *s, int n_clips) { return s && n_clips >= 1 && s->n_frames >= 1 && s->stride >= 1; }
} // namespace

int mobi_sink_check(const mobi_sink *s, int n_clips, uint32_t width, uint32_t height) {
  if (!sink_schedule_ok(s, n_clips) || !s->dst || width < 1 || height < 1) return MOBI_E_ARG;
  const size_t esize = sink_esize(s);
  if (!esize) return MOBI_E_ARG;
  if (s->out_w < 1 || s->out_h < 1 || (s->out_w & 3)) return MOBI_E_ARG;
  for (int c = 0; c < n_clips; c++) {
    int64_t bx[5];
    sink_box(s, c, width, height, bx);
    if (bx[2] < 1 || bx[3] < 1 || bx[0] < 0 || bx[1] < 0 || bx[0] > (int64_t)width - bx[2] || bx[1] > (int64_t)height - bx[3] || (bx[4] & ~(int64_t)MOBI_BOX_FLIP_X))
      return MOBI_E_ARG;
    if (mobi_resample_den((uint32_t)bx[2], (uint32_t)bx[3], (uint32_t)s->out_w, (uint32_t)s->out_h) > ((uint64_t)1 << 23)) return MOBI_E_ARG; // the sums stay below 2^31
  }
  const int64_t reach = (int64_t)(s->n_frames - 1) * s->stride; // (both below 2^31: no overflow)
  if (reach > INT32_MAX) return MOBI_E_ARG;
  for (int c = 0; c < n_clips && s->start; c++)
    if (s->start[c] < 0 || (int64_t)s->start[c] + reach > INT32_MAX) return MOBI_E_ARG;
  if ((uintptr_t)s->dst & 15) return MOBI_E_ARG;
  if (!mobi_sink_layout_ok(s->format == MOBI_EXPORT_RGB_PLANAR, (uint32_t)n_clips, s->n_frames, (uint32_t)s->out_w, (uint32_t)s->out_h, s->clip_stride, s->frame_stride,
                           s->chan_stride, s->dst_bytes / esize, nullptr))
    return MOBI_E_ARG;
  return MOBI_OK;
}

int mobi_sink_plan(const mobi_sink *s, int n_clips, int64_t step, int32_t *clips_out, int64_t *elem_off_out) {
  if (!sink_schedule_ok(s, n_clips)) return MOBI_E_ARG;
  const MobiSinkSched sch{step, s->stride, s->n_frames, s->clip_stride, s->frame_stride, s->chan_stride};
  int count = 0;
  for (int c = 0; c < n_clips; c++) {
    const int32_t t = mobi_sink_select(step, s->start ? (uint32_t)s->start[c] : 0u, s->stride, s->n_frames);
    if (t < 0) continue;
    if (clips_out) clips_out[count] = c;
    if (elem_off_out) elem_off_out[count] = mobi_sink_picture(&sch, (uint32_t)c, t);
    count++;
  }
  return count;
}

// ---- arming and disarming: with nothing in flight, so that no step is half with and half without (as mobi_batch_set_motion) ----
int mobi_batch_set_sink(mobi_batch *b, const mobi_sink *s) {
  if (!b || b->poisoned || b->async_count || b->gop_count) return MOBI_E_ARG;
  if (!s) {
    if (!b->sink.on) return MOBI_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream)); // (synchronous steps may have left launches behind the caller's last wait: mobi_batch_replay)
    b->sink.on = false;
    b->sink.pending = 0;
    b->sink.dst = nullptr;
    return MOBI_OK;
  }
  const int n = b->n;
  if (int e = mobi_sink_check(s, n, b->g.width, b->g.height)) return e;
  const size_t esize = sink_esize(s);
  const int planar = s->format == MOBI_EXPORT_RGB_PLANAR;
  int64_t span = 0;
  (void)mobi_sink_layout_ok(planar, (uint32_t)n, s->n_frames, (uint32_t)s->out_w, (uint32_t)s->out_h, s->clip_stride, s->frame_stride, s->chan_stride,
                            s->dst_bytes / esize, &span);
  HIP_TRY(hipSetDevice(b->device));
  // dst: device memory of this batch's device, everything the sink may write inside one allocation
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, s->dst) != hipSuccess) { (void)hipGetLastError(); return MOBI_E_ARG; }
  if (at.type != hipMemoryTypeDevice || at.device != b->device) return MOBI_E_ARG;
  hipDeviceptr_t base = nullptr;
  size_t range = 0;
  if (hipMemGetAddressRange(&base, &range, (hipDeviceptr_t)s->dst) != hipSuccess) { (void)hipGetLastError(); return MOBI_E_ARG; }
  if ((uintptr_t)s->dst + (size_t)span * esize > (uintptr_t)base + range) return MOBI_E_ARG;
  // the records: box, tiling and start of every clip
  std::vector<MobiResampleClip> recs((size_t)n);
  std::vector<uint32_t> start((size_t)n);
  MobiResampleCall call{(uint32_t)s->out_w, (uint32_t)s->out_h, 0u, 0u, nullptr};
  int64_t last = 0;
  for (int c = 0; c < n; c++) {
    int64_t bx[5];
    sink_box(s, c, b->g.width, b->g.height, bx);
    recs[c] = mobi_resample_plan((uint32_t)bx[0], (uint32_t)bx[1], (uint32_t)bx[2], (uint32_t)bx[3], (uint32_t)bx[4], call.ow, call.oh);
    recs[c].start = start[c] = s->start ? (uint32_t)s->start[c] : 0u;
    call.blocks = std::max(call.blocks, mobi_resample_blocks(&recs[c]));
    call.lds_bytes = std::max(call.lds_bytes, mobi_resample_lds_bytes(&recs[c]));
    last = std::max(last, (int64_t)start[c] + (int64_t)(s->n_frames - 1) * s->stride);
  }
  HIP_TRY(hipStreamSynchronize(b->stream)); // (a sink being replaced: its last launches read the records about to be overwritten)
  mobi_batch::Sink &k = b->sink;
  if (!k.d_recs)
    if (int e = k.d_recs.alloc((size_t)n)) return e;
  HIP_TRY(hipMemcpy(k.d_recs, recs.data(), recs.size() * sizeof(MobiResampleClip), hipMemcpyHostToDevice));
  call.clips_dev = k.d_recs;
  k.planar = planar;
  k.esize = (int)esize;
  k.sb = MobiRgbAffine{{1.f, 1.f, 1.f, 0.f, 0.f, 0.f}};
  if (s->scale_bias) memcpy(k.sb.v, s->scale_bias, sizeof(k.sb.v));
  k.call = call;
  k.sch = MobiSinkSched{0, s->stride, s->n_frames, s->clip_stride, s->frame_stride, s->chan_stride};
  k.dst = (uint8_t *)s->dst;
  k.start.swap(start);
  k.now = k.counted = -1;
  k.last = last;
  k.pending = (int64_t)n * s->n_frames;
  k.on = true;
  return MOBI_OK;
}
int mobi_batch_sink_pending(const mobi_batch *b) { return b && b->sink.on ? (int)std::min<int64_t>(b->sink.pending, INT32_MAX) : 0; }
long mobi_batch_sink_launches(const mobi_batch *b) { return b ? b->sink_launches : 0; }

// ---- behind a step's reconstruction (mobi_batch::sink_step): the clips of the launch that contribute in the step it wrote ----
int mobi_batch::sink_launch(const MobiReconArgs &a) {
  // the step of ring slot a.ring_base: the one begun last, or (a repair) as many steps earlier as the ring has turned since
  const int64_t step = sink.now - (int64_t)((ring_base - a.ring_base + 6) % 6);
  if (step < 0 || step > sink.last) return MOBI_OK;
  const int c0 = (int)((size_t)(a.planes - (arena + kGuard)) / clip_bytes), c1 = c0 + a.n_clips;
  // no empty launches: the clip range that is selected, narrowed from both ends (the workgroups of clips between that are not leave at once)
  int lo = c1, hi = c0, count = 0;
  for (int c = c0; c < c1; c++)
    if (mobi_sink_select(step, sink.start[c], sink.sch.stride, sink.sch.n_frames) >= 0) { lo = std::min(lo, c); hi = c; count++; }
  if (count) {
    const MobiExportGeom geo{arena + kGuard, clip_bytes, (uint32_t)slot_bytes, (int)g.width, (int)g.height, (int)g.stride, (int)g.mbw, g.lg};
    MobiSinkSched sch = sink.sch;
    sch.step = step;
    if (mobi_launch_sink(&geo, version, sink.planar, sink.esize, &sink.call, a.ring_base, lo, hi - lo + 1, &sch, &sink.sb, sink.dst, stream) != 0) return MOBI_E_DEVICE;
    sink_launches++;
  }
  if (step > sink.counted) { // (the step's first launch covers every clip: a repair comes later)
    sink.counted = step;
    sink.pending -= count;
  }
  return MOBI_OK;
}
