// mobi_pictures.cpp -- what callers take out of a batch's ring: planes, Bitmaps, exports (the pipeline is mobi_export.cpp's), encoder-side analysis
#include "mobi_batch.h"

int mobi_batch_get_planes(mobi_batch *b, int clip, int ring_idx, uint8_t *y_out, uint8_t *uv_out) {
  if (!b || clip < 0 || clip >= b->n || ring_idx < 0 || ring_idx > 5) return MOBI_E_ARG;
  if (ring_idx >= b->frames_started) return MOBI_E_NULLREF;
  HIP_TRY(hipSetDevice(b->device));
  const uint8_t *slot = b->arena + kGuard + (size_t)clip * b->clip_bytes + (size_t)((b->ring_base + 6 - ring_idx) % 6) * b->slot_bytes;
  const size_t ysz = (size_t)b->g.stride * b->g.height;
  // the planes live in HBM as macroblock tiles (mobi_tile.h); callers get the reference's row-major arrays (MD.cs:107-108, 414-415)
  if (!b->d_lin)
    if (int e = b->d_lin.alloc(b->slot_bytes)) return e;
  if (mobi_launch_untile(slot, b->d_lin, b->g.stride, b->g.height, b->stream) != 0) return MOBI_E_DEVICE;
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (y_out) HIP_TRY(hipMemcpy(y_out, b->d_lin, ysz, hipMemcpyDeviceToHost));
  if (uv_out) HIP_TRY(hipMemcpy(uv_out, b->d_lin + ysz, ysz / 2, hipMemcpyDeviceToHost));
  return MOBI_OK;
}
// ---- the Bitmap of DecodeFrame(), MD.cs:260-323 ---------------------------------------------------------
int ensure_argb(mobi_batch *b, int n_clips) {
  const size_t need = (size_t)n_clips * b->g.width * b->g.height * 4;
  if (b->d_argb && b->argb_bytes >= need) return MOBI_OK;
  b->d_argb.free();
  b->argb_bytes = 0;
  if (int e = b->d_argb.alloc(need / 4)) return e;
  b->argb_bytes = need;
  return MOBI_OK;
}
int mobi_batch_convert_argb(mobi_batch *b) {
  if (!b) return MOBI_E_ARG;
  if (b->frames_started < 1) return MOBI_E_NULLREF;
  HIP_TRY(hipSetDevice(b->device));
  if (int e = ensure_argb(b, b->n)) return e;
  MobiReconArgs a = b->args(nullptr, nullptr);
  if (mobi_launch_argb(&a, b->version, 0, b->n, b->d_argb, b->stream) != 0) return MOBI_E_DEVICE;
  b->argb_all_valid = true;
  return MOBI_OK;
}
int mobi_batch_get_argb(mobi_batch *b, int clip, uint32_t *out) {
  if (!b || clip < 0 || clip >= b->n || !out) return MOBI_E_ARG;
  if (b->frames_started < 1) return MOBI_E_NULLREF;
  HIP_TRY(hipSetDevice(b->device));
  const size_t words = (size_t)b->g.width * b->g.height;
  size_t src_clip = (size_t)clip;
  if (!b->argb_all_valid) { // convert just this clip into the front of the buffer
    if (int e = ensure_argb(b, 1)) return e;
    MobiReconArgs a = b->args(nullptr, nullptr);
    if (mobi_launch_argb(&a, b->version, clip, 1, b->d_argb, b->stream) != 0) return MOBI_E_DEVICE;
    src_clip = 0;
  }
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(out, b->d_argb + src_clip * words, words * 4, hipMemcpyDeviceToHost));
  return MOBI_OK;
}
// the Bitmap of the frame at ring index ring_idx (0 = the newest): what DecodeFrame() returned `ring_idx` calls ago -- for callers that decode
// in groups (mobi_batch_decode_gop: frame k of a group of K sits at ring index K - 1 - k) and want every frame's Bitmap, as a converter does
// (MobiConverter/Program.cs:57-71).  (The conversion depends on Version alone, MD.cs:260-323: any frame still in the ring converts the same way.)
int mobi_batch_get_argb_at(mobi_batch *b, int clip, int ring_idx, uint32_t *out) {
  if (!b || clip < 0 || clip >= b->n || !out || ring_idx < 0 || ring_idx > 5) return MOBI_E_ARG;
  if (ring_idx >= b->frames_started) return MOBI_E_NULLREF;
  if (ring_idx == 0) return mobi_batch_get_argb(b, clip, out);
  HIP_TRY(hipSetDevice(b->device));
  const size_t words = (size_t)b->g.width * b->g.height;
  if (int e = ensure_argb(b, 1)) return e;
  b->argb_all_valid = false; // (the front of the buffer is this frame's now)
  MobiReconArgs a = b->args(nullptr, nullptr);
  a.ring_base = (b->ring_base + 6 - ring_idx) % 6;
  if (mobi_launch_argb(&a, b->version, clip, 1, b->d_argb, b->stream) != 0) return MOBI_E_DEVICE;
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(out, b->d_argb, words * 4, hipMemcpyDeviceToHost));
  return MOBI_OK;
}
// ---- what the exports to host and to device memory share ----
namespace {
// clips [clip0, clip0 + n_clips) of the batch?
bool clip_range_ok(const mobi_batch *b, int clip0, int n_clips) { return clip0 >= 0 && n_clips >= 1 && clip0 <= b->n - n_clips; }
// Frames ring_idx .. ring_idx - n_frames + 1 of those clips: MOBI_OK when they can be exported.  Ranges (`fits`: what the caller knows
// about dst), then the state of the batch: poisoned, not decoded yet, still in flight.
int check_export(const mobi_batch *b, int ring_idx, int n_frames, int clip0, int n_clips, bool fits) {
  if (!clip_range_ok(b, clip0, n_clips)) return MOBI_E_ARG;
  if (ring_idx < 0 || ring_idx > 5 || n_frames < 1 || ring_idx - n_frames + 1 < 0) return MOBI_E_ARG;
  if (!fits || b->poisoned) return MOBI_E_ARG;
  if (ring_idx >= b->frames_started) return MOBI_E_NULLREF;
  if (ring_idx - n_frames + 1 < b->async_count) return MOBI_E_ARG; // frames of steps not waited for: mobi_batch_wait may still repair them
  return MOBI_OK;
}
// the job of a checked request (mobi_exporter.h); makes the batch's exporter at its first export
MobiExportJob export_job(mobi_batch *b, int format, int ring_idx, int n_frames, int clip0, int n_clips, void *dst) {
  if (!b->exporter) b->exporter = mobi_exporter_new(b->device);
  MobiExportJob job;
  job.g = MobiExportGeom{b->arena + kGuard, b->clip_bytes, (uint32_t)b->slot_bytes, (int)b->g.width, (int)b->g.height, (int)b->g.stride, (int)b->g.mbw, b->g.lg};
  job.format = format;
  job.n_frames = n_frames;
  job.clip0 = clip0;
  job.n_clips = n_clips;
  job.slot0 = (b->ring_base + 6 - ring_idx) % 6;
  job.dst = dst;
  job.src_stream = b->stream;
  return job;
}
} // namespace
// ---- export of whole batches of pictures to host memory (the converter's decode -> AddFrame loop, MobiConverter/Program.cs:69-76) ----
// The arguments are checked here against the batch; the pipeline, the tickets and the ring-slot guard are mobi_export.cpp's.
int mobi_batch_export(mobi_batch *b, int format, int ring_idx, int n_frames, int clip0, int n_clips, void *dst, size_t dst_bytes, uint64_t *ticket_out) {
  if (!b || !dst || (format != MOBI_EXPORT_I420 && format != MOBI_EXPORT_ARGB)) return MOBI_E_ARG;
  const size_t px = (size_t)b->g.width * b->g.height, pic = format == MOBI_EXPORT_I420 ? px * 3 / 2 : px * 4;
  if (int e = check_export(b, ring_idx, n_frames, clip0, n_clips, dst_bytes >= pic * n_frames * n_clips)) return e;
  HIP_TRY(hipSetDevice(b->device));
  MobiExportJob job = export_job(b, format, ring_idx, n_frames, clip0, n_clips, dst);
  job.argb = [b](int c0, int n, int slot, uint32_t *out, hipStream_t s) {
    MobiReconArgs a = b->args(nullptr, nullptr);
    a.ring_base = slot;
    return mobi_launch_argb(&a, b->version, c0, n, out, s);
  };
  job.run = [b](int n, const std::function<void(int)> &f) { b->pool->run(n, f); };
  uint64_t t = 0;
  if (int e = mobi_exporter_run(b->exporter, job, &t)) return e;
  if (ticket_out) *ticket_out = t;
  return MOBI_OK;
}
// ---- export into device memory, on the caller's stream (torch tensors, the caller's own HIP allocations) ----
// The arguments are checked here; the stream order and the ring-slot guard are mobi_export.cpp's, the RGB kernels mobi_export_rgb.hip's,
// mobi_export_scale.hip's and mobi_export_resample.hip's (what the three share: mobi_export_tensor.h).
namespace {
// element size of an RGB export's dtype; 0: a combination the RGB formats do not have
size_t rgb_esize(int dtype, const float *scale_bias) {
  if (dtype == MOBI_DTYPE_U8) return scale_bias ? 0 : 1;
  return dtype == MOBI_DTYPE_F16 ? 2 : dtype == MOBI_DTYPE_F32 ? 4 : 0;
}
// the same for the entry points that have RGB formats only: 0 for any other format too
size_t rgb_only_esize(int format, int dtype, const float *scale_bias) {
  return format == MOBI_EXPORT_RGB_PLANAR || format == MOBI_EXPORT_RGB_PACKED ? rgb_esize(dtype, scale_bias) : 0;
}
// scale[3], bias[3] of a call; none: the bytes as they are
MobiRgbAffine rgb_affine(const float *scale_bias) {
  MobiRgbAffine sb{{1.f, 1.f, 1.f, 0.f, 0.f, 0.f}};
  if (scale_bias) memcpy(sb.v, scale_bias, sizeof(sb.v));
  return sb;
}
// What every device export checks once its format is known, and the hand-over: pictures of `pic` bytes each, n_frames x n_clips of them
// into dst on `stream`; launch(job, need, stream) enqueues the kernels (need = the bytes the export writes).  params: what the kernels read
// from device memory (mobi_exporter.h), or nothing.
int export_device(mobi_batch *b, int format, size_t pic, int ring_idx, int n_frames, int clip0, int n_clips, void *dst, size_t dst_bytes, void *stream,
                  const std::function<int(const MobiExportJob &, size_t, hipStream_t)> &launch, MobiExportParams *params = nullptr) {
  const size_t need = pic * n_frames * n_clips;
  if (int e = check_export(b, ring_idx, n_frames, clip0, n_clips, dst_bytes >= need && !((uintptr_t)dst & 15))) return e;
  HIP_TRY(hipSetDevice(b->device));
  // dst: device memory of this batch's device, the whole of [dst, dst + need) inside one allocation
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, dst) != hipSuccess) { (void)hipGetLastError(); return MOBI_E_ARG; }
  if (at.type != hipMemoryTypeDevice || at.device != b->device) return MOBI_E_ARG;
  hipDeviceptr_t base = nullptr;
  size_t range = 0;
  if (hipMemGetAddressRange(&base, &range, (hipDeviceptr_t)dst) != hipSuccess) { (void)hipGetLastError(); return MOBI_E_ARG; }
  if ((uintptr_t)dst + need > (uintptr_t)base + range) return MOBI_E_ARG;
  const hipStream_t s = (hipStream_t)stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); return MOBI_E_ARG; }
  if (cap != hipStreamCaptureStatusNone) return MOBI_E_ARG;
  const MobiExportJob job = export_job(b, format, ring_idx, n_frames, clip0, n_clips, dst);
  return mobi_exporter_run_device(b->exporter, job, s, [&](hipStream_t st) { return launch(job, need, st); }, params);
}
} // namespace
int mobi_batch_export_device(mobi_batch *b, int format, int dtype, const float *scale_bias, int ring_idx, int n_frames, int clip0, int n_clips,
                             void *dst, size_t dst_bytes, void *stream) {
  if (!b || !dst) return MOBI_E_ARG;
  size_t esize = 0;
  switch (format) {
  case MOBI_EXPORT_I420:
  case MOBI_EXPORT_ARGB:
    if (dtype != MOBI_DTYPE_U8 || scale_bias) return MOBI_E_ARG;
    break;
  case MOBI_EXPORT_RGB_PLANAR:
  case MOBI_EXPORT_RGB_PACKED:
    if (!(esize = rgb_esize(dtype, scale_bias))) return MOBI_E_ARG;
    break;
  default:
    return MOBI_E_ARG;
  }
  const size_t px = (size_t)b->g.width * b->g.height;
  const size_t pic = format == MOBI_EXPORT_I420 ? px * 3 / 2 : format == MOBI_EXPORT_ARGB ? px * 4 : px * 3 * esize;
  const MobiRgbAffine sb = rgb_affine(scale_bias);
  uint8_t *out = (uint8_t *)dst;
  auto launch = [&](const MobiExportJob &job, size_t need, hipStream_t st) -> int {
    if (format == MOBI_EXPORT_I420) return mobi_launch_export_i420(&job.g, 0, n_frames * n_clips, n_clips, clip0, job.slot0, out, st);
    if (format == MOBI_EXPORT_ARGB) {
      for (int j = 0; j < n_frames; j++) { // the Bitmap kernel converts clips of one slot: one launch per frame
        MobiReconArgs a = b->args(nullptr, nullptr);
        a.ring_base = (job.slot0 + j) % 6;
        if (int e = mobi_launch_argb(&a, b->version, clip0, n_clips, (uint32_t *)(out + (size_t)j * n_clips * pic), st)) return e;
      }
      return 0;
    }
    // A GPU reader comes next.  Output that fits the 256 MiB MALL is read faster from the caches (plain stores: export + a reduction over it
    // 4 - 13 % faster); larger output goes past them (0.3 - 4 % faster): tools/exp_export_device.py --nt, DESIGN.md "Export to device memory"
    int nontemporal = need > ((size_t)256 << 20);
#if defined(MOBI_PROFILING)
    if (const char *e = getenv("MOBI_EXPORT_RGB_NT")) nontemporal = atoi(e); // (A/B: tools/exp_export_device.py)
#endif
    return mobi_launch_export_rgb(&job.g, b->version, format == MOBI_EXPORT_RGB_PLANAR, (int)esize, nontemporal, n_frames, n_clips, clip0,
                                  job.slot0, &sb, out, st);
  };
  return export_device(b, format, pic, ring_idx, n_frames, clip0, n_clips, dst, dst_bytes, stream, launch);
}
// The crop, area-averaged down to out_w x out_h (mobi_export_scale.h): RGB tensors only, one crop per call.
int mobi_batch_export_device_scaled(mobi_batch *b, int format, int dtype, const float *scale_bias, int crop_x, int crop_y, int crop_w, int crop_h,
                                    int out_w, int out_h, int ring_idx, int n_frames, int clip0, int n_clips, void *dst, size_t dst_bytes, void *stream) {
  const size_t esize = rgb_only_esize(format, dtype, scale_bias);
  if (!b || !dst || !esize) return MOBI_E_ARG;
  const int W = (int)b->g.width, H = (int)b->g.height;
  if (crop_w < 1 || crop_h < 1 || crop_x < 0 || crop_y < 0 || crop_x > W - crop_w || crop_y > H - crop_h) return MOBI_E_ARG;
  if (out_w < 1 || out_h < 1 || out_w > crop_w || out_h > crop_h || (out_w & 3)) return MOBI_E_ARG;
  if ((uint64_t)crop_w * (uint64_t)crop_h > ((uint64_t)1 << 23)) return MOBI_E_ARG; // the sums stay below 2^31
  const MobiScalePlan plan = mobi_scale_plan((uint32_t)crop_x, (uint32_t)crop_y, (uint32_t)crop_w, (uint32_t)crop_h, (uint32_t)out_w, (uint32_t)out_h);
  const MobiRgbAffine sb = rgb_affine(scale_bias);
  auto launch = [&](const MobiExportJob &job, size_t, hipStream_t st) -> int {
    return mobi_launch_export_scale(&job.g, b->version, format == MOBI_EXPORT_RGB_PLANAR, (int)esize, &plan, n_frames, n_clips, clip0, job.slot0, &sb,
                                    (uint8_t *)dst, st);
  };
  return export_device(b, format, mobi_scale_picture_bytes((uint32_t)out_w, (uint32_t)out_h, (uint32_t)esize), ring_idx, n_frames, clip0, n_clips, dst,
                       dst_bytes, stream, launch);
}
// A box per clip, resized to out_w x out_h, mirrored or not (mobi_export_resample.h): RGB tensors only.  The boxes are checked and the
// clips' records made here; they reach the kernel through a parameter block of the exporter.
int mobi_batch_export_device_boxes(mobi_batch *b, int format, int dtype, const float *scale_bias, const int32_t *boxes, int out_w, int out_h, int ring_idx,
                                   int n_frames, int clip0, int n_clips, void *dst, size_t dst_bytes, void *stream) {
  const size_t esize = rgb_only_esize(format, dtype, scale_bias);
  if (!b || !dst || !boxes || !esize) return MOBI_E_ARG;
  if (out_w < 1 || out_h < 1 || (out_w & 3)) return MOBI_E_ARG;
  // The boxes are the caller's memory and have to be copied before the call returns, so they are read here, in front of the shared
  // checks of export_device: that is why the clip range, which says how many rows `boxes` has, is looked at here as well as there.
  // Nothing is enqueued and nothing of the batch changes before export_device has accepted the rest.
  if (!clip_range_ok(b, clip0, n_clips)) return MOBI_E_ARG;
  const int W = (int)b->g.width, H = (int)b->g.height;
  std::vector<MobiResampleClip> recs((size_t)n_clips);
  MobiResampleCall call{(uint32_t)out_w, (uint32_t)out_h, 0u, 0u, nullptr};
  for (int c = 0; c < n_clips; c++) {
    const int32_t *bx = boxes + 5 * (size_t)c;
    const int x = bx[0], y = bx[1], w = bx[2], h = bx[3];
    if (w < 1 || h < 1 || x < 0 || y < 0 || x > W - w || y > H - h || (bx[4] & ~MOBI_BOX_FLIP_X)) return MOBI_E_ARG;
    if (mobi_resample_den((uint32_t)w, (uint32_t)h, (uint32_t)out_w, (uint32_t)out_h) > ((uint64_t)1 << 23)) return MOBI_E_ARG; // the sums stay below 2^31
    recs[c] = mobi_resample_plan((uint32_t)x, (uint32_t)y, (uint32_t)w, (uint32_t)h, (uint32_t)bx[4], (uint32_t)out_w, (uint32_t)out_h);
    call.blocks = std::max(call.blocks, mobi_resample_blocks(&recs[c]));
    call.lds_bytes = std::max(call.lds_bytes, mobi_resample_lds_bytes(&recs[c]));
  }
  const MobiRgbAffine sb = rgb_affine(scale_bias);
  MobiExportParams params{recs.data(), recs.size() * sizeof(MobiResampleClip), nullptr};
  auto launch = [&](const MobiExportJob &job, size_t, hipStream_t st) -> int {
    call.clips_dev = (const MobiResampleClip *)params.dev;
    return mobi_launch_export_resample(&job.g, b->version, format == MOBI_EXPORT_RGB_PLANAR, (int)esize, &call, n_frames, n_clips, clip0, job.slot0, &sb,
                                       (uint8_t *)dst, st);
  };
  return export_device(b, format, mobi_scale_picture_bytes((uint32_t)out_w, (uint32_t)out_h, (uint32_t)esize), ring_idx, n_frames, clip0, n_clips, dst,
                       dst_bytes, stream, launch, &params);
}
// ---- the motion ring into device memory (mobi_motion_ring.h): mobi_batch_export_device's checks, stream order and guard, the ring's kernels ----
int mobi_batch_export_motion(mobi_batch *b, int format, int dtype, int block, float scale, int ring_idx, int n_frames, int clip0, int n_clips,
                             void *dst, size_t dst_bytes, void *stream) {
  if (!b || !dst) return MOBI_E_ARG;
  const size_t n_mbs = (size_t)b->g.mbw * b->g.mbh;
  size_t pic = 0, esize = 0;
  float k = 0.f;
  switch (format) {
  case MOBI_MOTION_CELLS:
    if (dtype != MOBI_DTYPE_I16 || block != 2) return MOBI_E_ARG;
    pic = 3 * n_mbs * MOBI_MV_CELLS * sizeof(int16_t);
    break;
  case MOBI_MOTION_MB:
    if (dtype != MOBI_DTYPE_I32 || block != 16) return MOBI_E_ARG;
    pic = MOBI_MB_VALUES * n_mbs * sizeof(int32_t);
    break;
  case MOBI_MOTION_FLOW: {
    esize = dtype == MOBI_DTYPE_F32 ? 4 : dtype == MOBI_DTYPE_F16 ? 2 : 0;
    if (!esize || (block != 2 && block != 4 && block != 8 && block != 16) || !(scale - scale == 0.f)) return MOBI_E_ARG; // (a finite scale)
    const int cells = (block / 2) * (block / 2);
    k = (float)((double)scale / (120.0 * cells));
    pic = 2 * n_mbs * (256 / (size_t)(block * block)) * esize;
    break;
  }
  default:
    return MOBI_E_ARG;
  }
  if (!b->motion_on) return MOBI_E_ARG;
  // (the ranges first, as everywhere: then "this frame has no motion slot", the NULLREF of a picture never produced)
  if (int e = check_export(b, ring_idx, n_frames, clip0, n_clips, dst_bytes >= pic * n_frames * n_clips && !((uintptr_t)dst & 15))) return e;
  if (!b->motion_has(ring_idx)) return MOBI_E_NULLREF;
  auto launch = [&](const MobiExportJob &job, size_t, hipStream_t st) -> int {
    const MobiMotionExport x{{b->d_mcells, b->d_mmbs}, b->g.mbw, b->g.mbh, n_frames, n_clips, clip0, job.slot0};
    if (format == MOBI_MOTION_CELLS) return mobi_launch_motion_cells(&x, (int16_t *)dst, st);
    if (format == MOBI_MOTION_MB) return mobi_launch_motion_mb(&x, (int32_t *)dst, st);
    return mobi_launch_motion_flow(&x, block, (int)esize, k, dst, st);
  };
  return export_device(b, format, pic, ring_idx, n_frames, clip0, n_clips, dst, dst_bytes, stream, launch);
}
int mobi_batch_export_wait(mobi_batch *b, uint64_t ticket) {
  if (!b || !b->exporter) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  return mobi_exporter_wait(b->exporter, ticket);
}
int mobi_batch_export_query(mobi_batch *b, uint64_t ticket) {
  if (!b || !b->exporter) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  return mobi_exporter_query(b->exporter, ticket);
}
// ---- encoder-side analysis: Analyzer.InterPredict2x2 over the ring this batch keeps in HBM (Analyzer.cs:608-693) ----
int mobi_batch_motion_search(mobi_batch *b, const uint8_t *const *src_y, uint32_t *out) {
  if (!b || !src_y || !out) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  const size_t n = (size_t)b->n, px = (size_t)b->g.width * b->g.height, n_mbs = (size_t)b->g.mbw * b->g.mbh;
  if (int e = b->h_stage.reserve(n * px)) return e;
  if (int e = b->d_src.reserve(n * px)) return e;
  if (int e = b->d_search.reserve(n * n_mbs * 64 * 4)) return e;
  for (size_t i = 0; i < n; i++)
    if (!src_y[i]) return MOBI_E_ARG;
  b->pool->run((int)n, [&](int i) { memcpy(b->h_stage.p + (size_t)i * px, src_y[i], px); });
  HIP_TRY(hipMemcpyAsync(b->d_src.p, b->h_stage.p, n * px, hipMemcpyHostToDevice, b->stream));
  MobiReconArgs a = b->args(nullptr, nullptr);
  const int n_past = std::min(5, b->frames_started); // PastFramesY[i] == null ends the loop (:618)
  if (mobi_launch_motion_search(&a, b->d_src.p, (uint32_t *)b->d_search.p, n_past, b->stream) != 0) return MOBI_E_DEVICE;
  HIP_TRY(hipMemcpyAsync(out, b->d_search.p, n * n_mbs * 64 * 4, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return MOBI_OK;
}

// ---- encoder-side forward transforms: MobiEncoder.DCT64 / DCT16 over caller buffers ----
int mobi_forward_dct(int device, int n, const int32_t *in, int32_t *out, size_t n_blocks) {
  if ((n != 8 && n != 4) || (n_blocks && (!in || !out)) || n_blocks > 0xFFFFFFFFu / 64) return MOBI_E_ARG;
  if (n_blocks == 0) return MOBI_OK;
  HIP_TRY(hipSetDevice(device));
  const size_t bytes = n_blocks * (size_t)(n * n) * 4;
  DevArr<int32_t> d_in, d_out;
  if (int e = d_in.alloc(bytes / 4)) return e;
  if (int e = d_out.alloc(bytes / 4)) return e;
  if (hipMemcpy(d_in, in, bytes, hipMemcpyHostToDevice) != hipSuccess || mobi_launch_fwd_dct(n, d_in, d_out, (uint32_t)n_blocks, nullptr) != 0 ||
      hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess)
    return MOBI_E_DEVICE;
  return MOBI_OK;
}

// Batches made of copies (clip c decodes the same stream as clip c mod modulus: bench.py, soak runs): how many clips' newest frame differs
// from their source clip's, compared on the device byte for byte; n_diff_out[c] (optional, n_clips entries) = differing 16-byte words of clip c.
int mobi_batch_compare_clips(mobi_batch *b, int modulus, uint32_t *n_diff_out) {
  if (!b || modulus < 1 || modulus > b->n) return MOBI_E_ARG;
  if (b->frames_started < 1) return MOBI_E_NULLREF;
  HIP_TRY(hipSetDevice(b->device));
  if (int e = b->d_search.reserve((size_t)b->n * 4)) return e;
  HIP_TRY(hipMemsetAsync(b->d_search.p, 0, (size_t)b->n * 4, b->stream));
  MobiReconArgs a = b->args(nullptr, nullptr);
  if (mobi_launch_compare_clips(&a, modulus, (uint32_t *)b->d_search.p, b->stream) != 0) return MOBI_E_DEVICE;
  std::vector<uint32_t> h(b->n);
  HIP_TRY(hipMemcpyAsync(h.data(), b->d_search.p, (size_t)b->n * 4, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  int bad = 0;
  for (int i = 0; i < b->n; i++) bad += h[i] != 0;
  if (n_diff_out) memcpy(n_diff_out, h.data(), (size_t)b->n * 4);
  return bad;
}
