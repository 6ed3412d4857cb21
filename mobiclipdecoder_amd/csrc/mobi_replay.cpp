// mobi_replay.cpp -- pre-parsed replay (mobi_batch_preload / commit / replay / sync: what bench.py times) and the timing entry points.
#include "mobi_batch.h"

// ---- pre-parsed replay -----------------------------------------------------------------------------
int mobi_batch_preload(mobi_batch *b, int clip, const uint8_t *data, size_t len, const uint32_t *frame_off, int n_frames, int *rc_per_frame) {
  if (!b || clip < 0 || clip >= b->n || !data || !frame_off || n_frames < 1) return MOBI_E_ARG;
  for (int f = 0; f < n_frames; f++) // every frame boundary is checked before anything of the clip's staged state is replaced
    if (frame_off[f + 1] > len || frame_off[f] > frame_off[f + 1]) return MOBI_E_ARG;
  if (b->staged.empty()) { b->staged.resize(b->n); b->staged_rc.resize(b->n); }
  b->committed = false;
  b->staged[clip] = std::make_shared<std::vector<ParsedFrame>>(n_frames);
  b->staged_rc[clip] = std::make_shared<std::vector<int>>(n_frames, MOBI_E_ARG); // "not parsed": commit never executes such a frame
  auto &dst = *b->staged[clip];
  auto &rcs = *b->staged_rc[clip];
  MobiStreamParser parser((uint32_t)b->g.width, (uint32_t)b->g.height, b->version); // fresh decoder state for this clip
  int worst = MOBI_OK;
  for (int f = 0; f < n_frames; f++) {
    int32_t off = (int32_t)frame_off[f];
    int rc = parser.parse_frame(data, frame_off[f + 1], &off, dst[f]);
    rcs[f] = rc;
    if (rc_per_frame) rc_per_frame[f] = rc;
    if (rc != MOBI_OK && worst == MOBI_OK) worst = rc;
  }
  return worst;
}
int mobi_batch_preload_clone(mobi_batch *b, int clip, int src_clip) {
  if (!b || b->staged.empty() || clip < 0 || clip >= b->n || src_clip < 0 || src_clip >= b->n || !b->staged[src_clip]) return MOBI_E_ARG;
  b->committed = false;
  b->staged[clip] = b->staged[src_clip];
  b->staged_rc[clip] = b->staged_rc[src_clip];
  return MOBI_OK;
}
int mobi_batch_commit(mobi_batch *b) {
  if (!b || b->staged.empty()) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  const int n = b->n;
  int nf = -1;
  for (int c = 0; c < n; c++) {
    if (!b->staged[c] || b->staged[c]->empty()) return MOBI_E_ARG; // every clip must be loaded or cloned
    if (nf < 0) nf = (int)b->staged[c]->size();
    if ((int)b->staged[c]->size() != nf) return MOBI_E_ARG;
  }
  const int n_mbs = b->g.mbw * b->g.mbh;
  const size_t desc_bytes = align_up((size_t)n * n_mbs * sizeof(MbDesc) + 8 * sizeof(MbDesc), kAlign); // slack: a wave reads up to 8 descriptors at once
  size_t cmd_bytes = 0, n_items = 0;
  b->r_plan.assign(nf, LevelPlan());
  b->r_items_off.assign(nf, 0);
  b->r_desc_off.assign(nf, 0);
  b->r_payload_off.assign(nf, 0);
  std::vector<std::vector<const ParsedFrame *>> per_frame(nf, std::vector<const ParsedFrame *>(n, nullptr));
  for (int f = 0; f < nf; f++) {
    auto &ok = per_frame[f];
    for (int c = 0; c < n; c++)
      if ((*b->staged_rc[c])[f] == MOBI_OK && (int)(*b->staged[c])[f].desc.size() == n_mbs) ok[c] = &(*b->staged[c])[f]; // never a frame no parse filled
    if (step_payload_words(ok) + kPaySlack / 4 >= ((uint64_t)1 << 32)) return MOBI_E_ARG; // 32-bit word offsets (split the batch)
    b->r_desc_off[f] = cmd_bytes;
    b->r_payload_off[f] = cmd_bytes + desc_bytes;
    cmd_bytes += desc_bytes + align_up(step_payload_words(ok) * 4 + kPaySlack, kAlign);
    b->r_plan[f].build(ok, b->g.mbw);
    b->r_items_off[f] = n_items;
    n_items += b->r_plan[f].items.size();
  }
  if (int e = b->r_cmd.reserve(cmd_bytes)) return e;
  if (int e = b->r_items.reserve(n_items * 4 + 16)) return e;
  // upload through a bounded pinned window
  const size_t win = (size_t)64 << 20;
  if (int e = b->h_stage.reserve(win)) return e;
  auto upload = [&](uint8_t *dst, const uint8_t *src, size_t bytes) -> int {
    for (size_t done = 0; done < bytes; done += win) {
      size_t chunk = std::min(win, bytes - done);
      memcpy(b->h_stage.p, src + done, chunk);
      HIP_TRY(hipMemcpyAsync(dst + done, b->h_stage.p, chunk, hipMemcpyHostToDevice, b->stream));
      HIP_TRY(hipStreamSynchronize(b->stream));
    }
    return MOBI_OK;
  };
  std::vector<uint8_t> tmp;
  for (int f = 0; f < nf; f++) {
    const size_t bytes = (f + 1 < nf ? b->r_desc_off[f + 1] : cmd_bytes) - b->r_desc_off[f];
    tmp.assign(bytes, 0);
    step_write(per_frame[f], n_mbs, (MbDesc *)tmp.data(), (uint32_t *)(tmp.data() + desc_bytes));
    if (int e = upload(b->r_cmd.p + b->r_desc_off[f], tmp.data(), bytes)) return e;
    if (!b->r_plan[f].items.empty())
      if (int e = upload(b->r_items.p + b->r_items_off[f] * 4, (const uint8_t *)b->r_plan[f].items.data(), b->r_plan[f].items.size() * 4)) return e;
  }
  b->n_frames_loaded = nf;
  b->committed = true;
  return MOBI_OK;
}
int mobi_batch_replay(mobi_batch *b, int frame_idx) {
  if (!b || !b->committed || frame_idx < 0 || frame_idx >= b->n_frames_loaded) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  if (int e = b->begin_step()) return e;
  MobiReconArgs a = b->args(b->r_cmd.p + b->r_desc_off[frame_idx], b->r_cmd.p + b->r_payload_off[frame_idx]);
  return b->launch_plan(a, b->r_plan[frame_idx], (const uint32_t *)b->r_items.p + b->r_items_off[frame_idx]);
}
int mobi_batch_sync(mobi_batch *b) {
  if (!b) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  if (int e = b->read_faults(b->h_fault.data())) return e;
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->drain_events();
  for (int i = 0; i < b->n; i++)
    if (int e = fault_rc(MOBI_OK, b->h_fault[i])) return e;
  return MOBI_OK;
}
uint64_t mobi_batch_cmd_bytes(const mobi_batch *b, int frame_idx) {
  if (!b || !b->committed || frame_idx < 0 || frame_idx >= b->n_frames_loaded) return 0;
  return b->r_plan[frame_idx].cmd_bytes;
}
int mobi_batch_intra_stats(const mobi_batch *b, int frame_idx, uint64_t *n_intra_mbs, uint64_t *intra_cmd_bytes) {
  if (!b || !b->committed || frame_idx < 0 || frame_idx >= b->n_frames_loaded) return MOBI_E_ARG;
  if (n_intra_mbs) *n_intra_mbs = b->r_plan[frame_idx].n_intra;
  if (intra_cmd_bytes) *intra_cmd_bytes = b->r_plan[frame_idx].intra_cmd_bytes;
  return MOBI_OK;
}
int mobi_batch_time_begin(mobi_batch *b) {
  if (!b) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  b->acc_ms[0] = b->acc_ms[1] = 0;
  b->acc_launches[0] = b->acc_launches[1] = 0;
  HIP_TRY(hipEventRecord(b->ev_begin, b->stream));
  return MOBI_OK;
}
int mobi_batch_time_end(mobi_batch *b, float *ms_out) {
  if (!b || !ms_out) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipEventRecord(b->ev_end, b->stream));
  HIP_TRY(hipEventSynchronize(b->ev_end));
  HIP_TRY(hipEventElapsedTime(ms_out, b->ev_begin, b->ev_end));
  b->drain_events();
  return MOBI_OK;
}
int mobi_batch_set_kernel_timing(mobi_batch *b, int enable) {
  if (!b) return MOBI_E_ARG;
  b->ktiming = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
  return MOBI_OK;
}
int mobi_batch_kernel_ms(mobi_batch *b, float *inter_ms, float *intra_ms, int *inter_launches, int *intra_launches) {
  if (!b) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->drain_events();
  if (inter_ms) *inter_ms = b->acc_ms[0];
  if (intra_ms) *intra_ms = b->acc_ms[1];
  if (inter_launches) *inter_launches = b->acc_launches[0];
  if (intra_launches) *intra_launches = b->acc_launches[1];
  return MOBI_OK;
}
