// mobi_batch.cpp -- the batch itself: create / destroy, the parse mode, clip resets, accessors, the single-stream wrappers, the profiling twin's hooks
#include "mobi_batch.h"

thread_local char g_last_hip_error[256] = "";

// ---- test and profiling hooks: only in the -DMOBI_PROFILING twin of the library (libmobiclip_hip_prof.so); the product library has none
// of them (mobi_debug_write_planes lets any caller overwrite reference frames) ----
#if defined(MOBI_PROFILING)
#pragma GCC visibility push(default)
extern "C" {
// profiling aid, not part of the public header: copy out the MOBI_DEBUG=9 per-wave cycle records
// (uint32 x 4 per macroblock: descriptor, pixels+MC, residual, store drain) of the last inter launch
int mobi_debug_read_prof(mobi_batch *b, uint32_t *out, size_t n_words) {
  if (!b || !b->d_prof) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(out, b->d_prof, n_words * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(b->d_prof, 0, n_words * 4)); // read and clear: the next read sees only the steps in between
  return MOBI_OK;
}

// test aid, not part of the public header: overwrite ring slot `ring_idx` of one clip with planes given in the reference layout
// (Y: Stride * Height, UV: Stride * Height / 2) -- tests/test_unit_vectors.py predicts intra macroblocks from chosen halos this way.
// The caller keeps the padding zero (MD.cs:107: fresh planes are zeroed and nothing ever writes the padding).
int mobi_debug_write_planes(mobi_batch *b, int clip, int ring_idx, const uint8_t *y, const uint8_t *uv) {
  if (!b || clip < 0 || clip >= b->n || ring_idx < 0 || ring_idx > 5 || !y || !uv) return MOBI_E_ARG;
  if (ring_idx >= b->frames_started) return MOBI_E_NULLREF;
  HIP_TRY(hipSetDevice(b->device));
  if (b->exporter && mobi_exporter_guard(b->exporter, (b->ring_base + 6 - ring_idx) % 6, b->stream) != MOBI_OK) return MOBI_E_DEVICE;
  HIP_TRY(hipStreamSynchronize(b->stream));
  const uint32_t ysz = (uint32_t)b->g.stride * (uint32_t)b->g.height;
  std::vector<uint8_t> t(b->slot_bytes);
  for (uint32_t a = 0; a < ysz; a++) t[mobi_ty(a, b->g.lg)] = y[a];
  for (uint32_t a = 0; a < ysz / 2; a++) t[ysz + mobi_tc(a, b->g.lg)] = uv[a];
  uint8_t *slot = b->arena + kGuard + (size_t)clip * b->clip_bytes + (size_t)((b->ring_base + 6 - ring_idx) % 6) * b->slot_bytes;
  HIP_TRY(hipMemcpy(slot, t.data(), t.size(), hipMemcpyHostToDevice));
  b->argb_all_valid = false;
  return MOBI_OK;
}
mobi_batch *mobi_debug_dec_batch(mobi_dec *d) { return d ? d->b : nullptr; }
// test aid, not part of the public header: what the last device-side parse left in HBM.  desc_out: n_clips*n_mbs*8 words,
// items_out: n_clips*n_mbs words, res_out: n_clips*8 words, payload_out: n_clips*pay_cap words (any may be null); returns pay_cap
float mobi_debug_parse_ms(const mobi_batch *b) { return b ? b->last_parse_ms : 0.f; }
float mobi_debug_stage_ms(const mobi_batch *b) { return b ? b->last_stage_ms : 0.f; }
float mobi_debug_hostparse_ms(const mobi_batch *b) { return b ? b->last_hostparse_ms : 0.f; }
float mobi_debug_phase_ms(const mobi_batch *b, int k) { return b && k >= 0 && k < 6 ? b->phase_ms[k] : 0.f; } // host-parsed step: where the call's time went
long long mobi_debug_read_parse(mobi_batch *b, uint32_t *desc_out, uint32_t *items_out, uint32_t *res_out, uint32_t *payload_out, size_t payload_words) {
  if (!b || !b->dp.res.p) return MOBI_E_ARG;
  const DpSet &B = b->dp;
  const size_t n = (size_t)b->n, n_mbs = (size_t)b->g.mbw * b->g.mbh;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (desc_out) HIP_TRY(hipMemcpy(desc_out, B.desc.p, n * n_mbs * sizeof(MbDesc), hipMemcpyDeviceToHost));
  if (items_out) HIP_TRY(hipMemcpy(items_out, B.items.p, n * n_mbs * 4, hipMemcpyDeviceToHost));
  if (res_out) HIP_TRY(hipMemcpy(res_out, B.res.p, n * sizeof(MobiDevResult), hipMemcpyDeviceToHost));
  if (payload_out) HIP_TRY(hipMemcpy(payload_out, B.pay.p, std::min(payload_words * 4, B.pay.cap), hipMemcpyDeviceToHost));
  return (long long)b->last_pay_cap;
}
} // extern "C"
#pragma GCC visibility pop
#endif // MOBI_PROFILING

const char *mobi_build_info(void) { return "libmobiclip_hip 0.6 (gfx950, macroblock-tiled planes; HIP kernels: mobi_recon_inter8, mobi_recon_intra, mobi_recon_step, mobi_recon_intra_cl, mobi_recon_intra_walk, mobi_parse_frames, mobi_parse_frames_ls, mobi_ls_deps, mobi_parse_tail, mobi_gop_prepare, mobi_gop_chain, mobi_gop_fronts, mobi_gop_front_starts, mobi_gop_scatter, mobi_untile, mobi_yuv_to_argb, mobi_export_i420, mobi_export_rgb, mobi_export_scale, mobi_reset_state, mobi_idle_rows, mobi_motion_search_2x2, mobi_fwd_dct8, mobi_fwd_dct4, mobi_txcode8, mobi_txcode4; no CPU reconstruction path)"; }

const char *mobi_error_string(int rc) {
  switch (rc) {
    case MOBI_OK: return "ok";
    case MOBI_E_INDEX: return "index out of range (reference would throw IndexOutOfRange/ArgumentException)";
    case MOBI_E_NULLREF: return "reference frame slot is null";
    case MOBI_E_PARTCODE: return "illegal partition code";
    case MOBI_E_VERSION: return "unsupported codec version";
    case MOBI_E_CLAMP: return "residual left the clamp-table domain";
    case MOBI_E_UNSUPPORTED: return "a walk through Internal[] left a coefficient beyond int16 that need not leave the clamp table's domain (the one input outside the parity domain)";
    case MOBI_E_ARG: return "bad argument";
    case MOBI_E_DEVICE: return g_last_hip_error[0] ? g_last_hip_error : "HIP error";
    default: return "unknown";
  }
}

mobi_batch *mobi_batch_create(int n_clips, uint32_t width, uint32_t height, int version, int device) {
  if (n_clips < 1 || n_clips >= (1 << 19) || width == 0 || height == 0 || (width & 15) || (height & 15) || width > 1024 ||
      (width / 16) * (height / 16) > 8191)
    return nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    snprintf(g_last_hip_error, sizeof(g_last_hip_error), "no usable HIP device (count=%d, requested %d)", ndev, device);
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  auto b = std::make_unique<mobi_batch>();
  b->n = n_clips;
#if defined(MOBI_PROFILING)
  if (const char *dbg = getenv("MOBI_DEBUG")) b->debug = atoi(dbg); // 9: the octet kernel with in-kernel cycle records (tools/exp_prof8.py)
#endif
  b->device = device;
  b->version = version;
  for (int i = 0; i < n_clips; i++) b->parsers.emplace_back(new MobiStreamParser(width, height, version));
  b->g = b->parsers[0]->geom();
  b->slot_bytes = (size_t)b->g.stride * b->g.height * 3 / 2;
  b->clip_bytes = 6 * b->slot_bytes;
  b->cur.resize(n_clips);
  b->reset_pending.assign(n_clips, 0);
  b->frames_base.assign(n_clips, 0);
  b->stream_gen.assign(n_clips, 0);
  b->retired.resize(n_clips);
  b->ended.assign(n_clips, 0);
  b->idle_count.assign(n_clips, 0);
  b->h_fault.assign(n_clips, 0);
  b->on_host.assign(n_clips, 0);
  size_t arena_clips = (size_t)n_clips;
  size_t total = kGuard * 2 + b->clip_bytes * arena_clips;
  if (ensure_stream(b->stream)) return nullptr;
  if (b->arena.alloc(total)) return nullptr;
  if (hipMemsetAsync(b->arena, 0, total, b->stream) != hipSuccess) return nullptr; // padding must read 0 forever (MD.cs:107)
  if (b->d_fault.alloc(n_clips)) return nullptr;
  if (hipMemsetAsync(b->d_fault, 0, sizeof(int) * n_clips, b->stream) != hipSuccess) return nullptr;
  if (hipEventCreate(&b->ev_begin.h) != hipSuccess || hipEventCreate(&b->ev_end.h) != hipSuccess) return nullptr;
  {
    // 64 rows: the 6-bit quantizer field of any descriptor stays inside; the intra kernel's tap table rides behind them
    std::vector<int32_t> tab((size_t)MOBI_SCALE_ROWS * MOBI_SCALE_STRIDE + MOBI_TAP_ENTRIES * 2 + 8, 0) /* + 8: the kernel fetches four entries at a time */;
    for (int q = 0; q < MOBI_SCALE_QMAX; q++) mobi_build_scale_table(q, &tab[(size_t)q * MOBI_SCALE_STRIDE]);
    mobi_build_scale_table(MOBI_SCALE_LITERAL, &tab[(size_t)MOBI_SCALE_LITERAL * MOBI_SCALE_STRIDE]); // the row of ones: literal frames (mobi_parse.cpp)
    if (!mobi_build_intra_taps((int16_t *)&tab[(size_t)MOBI_SCALE_ROWS * MOBI_SCALE_STRIDE], MOBI_TAP_PITCH)) {
      snprintf(g_last_hip_error, sizeof(g_last_hip_error), "intra tap table self-check failed");
      return nullptr;
    }
    if (b->d_scale.alloc(tab.size())) return nullptr;
    if (hipMemcpy(b->d_scale, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  }
  {
    const size_t dbytes = (size_t)n_clips * b->g.mbw * b->g.mbh * 4;
    if (b->d_done.alloc(dbytes / 4)) return nullptr;
    if (hipMemset(b->d_done, 0, dbytes) != hipSuccess) return nullptr;
    if (const char *fs = getenv("MOBI_FUSED_STEP_MBS")) b->fused_mbs = (size_t)strtoull(fs, nullptr, 10);
    // parse threads: measured on a 2 x 64-core host (tools/exp_hostparse.py, 1024 clips: 16 / 32 / 64 / 128 threads parse a P-frame step in
    // 20.0 / 10.3 / 5.5 / 4.3 ms): one per two hardware threads, 64 at most
    const int hw = (int)std::thread::hardware_concurrency();
    int helpers = std::min({n_clips, std::max(hw / 2, std::min(hw, 8)), 64}) - 1;
#if defined(MOBI_PROFILING)
    if (const char *hc = getenv("MOBI_HOST_CHUNK")) b->host_chunk = atoi(hc); // (tools/exp_hostparse.py; 0: no pipeline)
#endif
    if (const char *pt = getenv("MOBI_PARSE_THREADS")) helpers = atoi(pt) - 1;
    b->pool.reset(new ParsePool(std::max(0, std::min(helpers, 255))));
    // Where the parse runs by default: on the host threads up to ~20 resident clips per thread, on the GPU beyond (640x480, r04: 64 threads
    // take a step of 1024 / 1536 / 2048 clips in 9.1 / 13.6 / 18.2 ms, parse to planes; mobi_parse_frames in 13.2 / 10.6 / 10.4 ms)
    b->parse_mode = n_clips >= std::max(640, 20 * (b->pool->size() + 1));
    b->parse_auto = true;
    b->ls_policy = 2; // ... and which device parser is in front is decided step by step (ls_decide)
    if (const char *dp = getenv("MOBI_DEVICE_PARSE")) {
      const int v = atoi(dp); // 3: on the GPU, the lock-step parser in front of every step
      b->parse_mode = v == 3 ? 1 : std::max(0, std::min(2, v));
      b->ls_policy = v == 3 ? 1 : 0;
      b->parse_auto = false;
    }
  }
  if (b->debug == 9) {
    const size_t pbytes = (size_t)n_clips * (b->g.mbw * b->g.mbh) * 16;
    if (b->d_prof.alloc(pbytes / 8)) return nullptr;
    if (hipMemset(b->d_prof, 0, pbytes) != hipSuccess) return nullptr;
  }
  if (hipStreamSynchronize(b->stream) != hipSuccess) return nullptr;
  return b.release();
}

void mobi_batch_destroy(mobi_batch *b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  delete b;
}

// Hybrid mode: how many clips (the last ones of the batch) the host pool parses beside the GPU.  (r05, tools/exp_hybrid.py: no share makes
// a step of up to 4096 clips faster than parse mode 1 -- 14.1 ms against 14.6 .. 16.2 -- because every clip has a wave slot of its own there
// and the parse launch is as long as ONE clip's parse whatever their number; the mode only pays beyond what the chip holds at once.)
static void hybrid_share(mobi_batch *b) {
  b->hybrid_host = std::min(1024, b->n / 5);
  if (const char *hh = getenv("MOBI_HYBRID_HOST_CLIPS")) b->hybrid_host = std::max(0, std::min(b->n - 1, atoi(hh)));
}
// Where the parse runs is settled at a batch's first frame (`first`, as the caller's path counts it).  A mode the caller named (env /
// mobi_batch_set_parse_mode) stays; a batch still on `parse_auto` goes to the GPU if force_device (mobi_batch_submit, mobi_batch_gop_begin: they
// have no host-parsed form), else by the lanes the call offers the parse kernels (mobi_batch_create has the figures: n_clips for mobi_batch_decode,
// n_clips * n_frames for mobi_batch_decode_gop), and with data != nullptr (mobi_batch_decode alone) past the packet guard.  The paths differ
// in these by history, not by design; every difference is kept as it was.
void settle_parse_mode(mobi_batch *b, bool first, size_t lanes, bool force_device, const uint8_t *const *data, const size_t *len, const int32_t *offsets) {
  if (!first) return;
  if (b->parse_auto) {
    b->parse_mode = force_device || lanes >= (size_t)std::max(640, 20 * (b->pool->size() + 1));
    if (data && b->parse_mode) {
      // Chosen by batch size only: a caller that hands over whole files as Data (MOC5 style, Form1.cs:292-302) would make the
      // device path upload up to 4 KB per macroblock per clip and frame (the frame length is unknown before the parse).  Packets
      // of a frame or a few are what the device path is for; anything much larger stays on the host parser.
      const size_t packet_like = (size_t)b->g.mbw * b->g.mbh * 256 + 65536;
      for (int i = 0; i < b->n; i++)
        if (data[i] && offsets[i] >= 0 && (uint64_t)offsets[i] < len[i] && len[i] - (size_t)offsets[i] > packet_like) { b->parse_mode = 0; break; }
    }
    b->parse_auto = false; // the decoder state lives on one side from the first frame on
  }
  if (b->parse_mode == 2) hybrid_share(b); // hybrid: a fixed share of the clips stays with the host parsers (their state lives there)
}

// ---- clip resets (mobi_batch_reset_clips) ----
// The host side of the pending resets, for the step with serial `serial` being handed over: a new parser (the old one stays as retired[c]
// while a step of its stream is in flight) and the routing a new decoder has -- back to the device parsers with clean_run = 0 and
// clean_need = 4, or the hybrid share's fresh host parser.  A call that fails before it hands the step over leaves the list pending and the
// next one comes here again with the same serial: clips that have it already are left alone.
void reset_apply_host(mobi_batch *b, uint64_t serial) {
  const bool in_flight = b->async_count || b->gop_count;
  for (int c : b->reset_list) {
    if (b->stream_gen[c] == serial) continue;
    if (in_flight) b->retired[c] = std::move(b->parsers[c]);
    b->parsers[c].reset(new MobiStreamParser((uint32_t)b->g.width, (uint32_t)b->g.height, b->version));
    b->stream_gen[c] = serial;
    if (!b->host_share.empty()) { // (device-parse modes, after dp_init)
      b->on_host[c] = b->host_share[c];
      b->clean_run[c] = 0;
      b->clean_need[c] = 4;
    }
  }
}
// the step with serial `serial` has been handed over, with the resets pending until now
void reset_commit(mobi_batch *b, uint64_t serial) {
  b->handover = serial;
  for (int c : b->reset_list) b->reset_pending[c] = 0;
  b->reset_list.clear();
}

int mobi_batch_in_flight(const mobi_batch *b) { return b ? b->async_count : 0; }
int mobi_batch_host_clips(const mobi_batch *b) {
  if (!b) return 0;
  if (!b->parse_mode) return b->n;
  int k = 0;
  for (uint8_t h : b->on_host) k += h;
  if (b->n_ended) // a clip whose stream has ended (mobi_batch_set_idle) is nobody's to parse
    for (int c = 0; c < b->n && c < (int)b->on_host.size(); c++) k -= b->on_host[c] && b->ended[c];
  return k;
}
int mobi_batch_lockstep_finished(const mobi_batch *b) { return b ? b->ls_finished : -1; }

// new MobiclipDecoder(Width, Height, Version) for clips of the batch, from the next step handed over on (reset_apply_host, mobi_reset_state).
// Records the list and the frame count's new origin; waits for nothing and enqueues nothing.
int mobi_batch_reset_clips(mobi_batch *b, const int32_t *clips, int count) {
  if (!b || count < 0 || (!clips && count > 0)) return MOBI_E_ARG;
  for (int j = 0; j < count; j++)
    if (clips[j] < 0 || clips[j] >= b->n) return MOBI_E_ARG; // (every index before anything changes)
  if (b->poisoned) return MOBI_E_DEVICE;
  // the frames of groups begun that have not turned the ring yet belong to the stream before
  int later = 0;
  for (int i = 0; i < b->gop_count; i++) {
    const mobi_batch::GopSlot &S = b->gslot[(b->gop_head + i) & 1];
    later += S.H.K - (S.resolved ? S.done : 0);
  }
  for (int j = 0; j < count; j++) {
    const int c = clips[j];
    b->frames_base[c] = b->frames_started + later;
    if (!b->reset_pending[c]) {
      b->reset_pending[c] = 1;
      b->reset_list.push_back(c);
    }
  }
  return MOBI_OK;
}
int mobi_batch_clip_frames(const mobi_batch *b, int32_t *out) {
  if (!b || !out) return MOBI_E_ARG;
  for (int c = 0; c < b->n; c++) out[c] = std::max(0, b->frames_started - b->frames_base[c]);
  if (!b->n_ended) return MOBI_OK;
  // live frames only: the idle slots of the clip's stream that have turned the ring do not count (idle_count is booked at the hand-over,
  // the ring turns in mobi_batch_gop_finish: the idle slots of groups begun that have not turned it yet are still to come)
  std::vector<int32_t> turned(b->idle_count);
  for (int i = 0; i < b->gop_count; i++) {
    const mobi_batch::GopSlot &S = b->gslot[(b->gop_head + i) & 1];
    if (S.H.idle_from.empty()) continue;
    const int done = S.resolved ? S.done : 0;
    for (int c = 0; c < b->n; c++)
      if (!b->stale(S.serial, c)) turned[c] -= S.H.K - std::max(done, (int)S.H.idle_from[c]);
  }
  for (int c = 0; c < b->n; c++)
    if (b->ended[c]) out[c] = std::max(0, out[c] - std::max(0, turned[c]));
  return MOBI_OK;
}

// ---- idle frame slots (mobi_batch_set_idle) ----
int mobi_batch_set_idle(mobi_batch *b, const uint8_t *idle, int n_frames) {
  if (!b) return MOBI_E_ARG;
  if (b->poisoned) return MOBI_E_DEVICE;
  if (!idle) { b->idle_frames = 0; return MOBI_OK; }
  if (n_frames < 1 || n_frames > MOBI_GOP_PARSE_MAX) return MOBI_E_ARG;
  b->idle_mask.assign(idle, idle + (size_t)n_frames * b->n);
  b->idle_frames = n_frames;
  return MOBI_OK;
}
int mobi_batch_clip_idle(const mobi_batch *b, int32_t *out) {
  if (!b || !out) return MOBI_E_ARG;
  for (int c = 0; c < b->n; c++) out[c] = b->idle_count[c];
  return MOBI_OK;
}
int mobi_batch_idle_launches(const mobi_batch *b) { return b ? b->idle_launches : 0; }
// ---- the motion ring (mobi_motion_ring.h): switched on and off with nothing in flight, so that no step is half with and half without ----
int mobi_batch_set_motion(mobi_batch *b, int on) {
  if (!b) return MOBI_E_ARG;
  if (b->poisoned) return MOBI_E_DEVICE;
  if ((on != 0) == b->motion_on) return MOBI_OK; // (a batch that never asked for motion: nothing at all)
  if (b->async_count || b->gop_count || (b->exporter && mobi_exporter_busy(b->exporter))) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream)); // (synchronous steps may have left launches behind the caller's last wait: mobi_batch_replay)
  if (!on) {
    b->motion_on = false;
    b->d_mcells.free();
    b->d_mmbs.free();
    return MOBI_OK;
  }
  const size_t mbs = (size_t)b->n * 6 * b->g.mbw * b->g.mbh;
  if (int e = b->d_mcells.alloc(mbs * MOBI_MV_CELLS)) return e;
  if (int e = b->d_mmbs.alloc(mbs * MOBI_MOTION_MB_WORDS)) { b->d_mcells.free(); return e; }
  b->motion_on = true;
  b->motion_from = b->frames_started;
  return MOBI_OK;
}
long mobi_batch_motion_launches(const mobi_batch *b) { return b ? b->motion_launches : 0; }
size_t mobi_batch_motion_bytes(const mobi_batch *b) { return b ? b->motion_bytes() : 0; }
int idle_check(const mobi_batch *b, int K, std::vector<uint8_t> &from) {
  from.clear();
  if (!b->idle_frames && !b->n_ended) return MOBI_OK; // (a caller that never sets a mask: no per-clip work)
  if (b->idle_frames && b->idle_frames != K) return MOBI_E_ARG;
  const int n = b->n;
  bool any = false;
  from.assign(n, (uint8_t)K);
  for (int c = 0; c < n; c++) {
    int first = K;
    if (b->idle_frames) {
      while (first > 0 && b->idle_mask[(size_t)(first - 1) * n + c]) first--; // the idle suffix ...
      for (int k = 0; k < first; k++)
        if (b->idle_mask[(size_t)k * n + c]) return MOBI_E_ARG; // ... and nothing idle in front of it
    }
    if (first > 0 && b->ended[c] && !b->reset_pending[c]) return MOBI_E_ARG; // a live frame, and the stream has ended
    from[c] = (uint8_t)first;
    any = any || first < K;
  }
  if (!any) from.clear();
  return MOBI_OK;
}
void idle_commit(mobi_batch *b, int K, const std::vector<uint8_t> &from) {
  b->idle_frames = 0;
  if (!b->n_ended && from.empty()) return;
  for (int c : b->reset_list) { // the resets that apply to this hand-over: a new stream
    if (b->ended[c]) { b->ended[c] = 0; b->n_ended--; }
    b->idle_count[c] = 0;
  }
  if (from.empty()) return;
  for (int c = 0; c < b->n; c++) {
    if (from[c] >= K) continue;
    if (!b->ended[c]) { b->ended[c] = 1; b->n_ended++; }
    b->idle_count[c] = from[c] > 0 ? K - from[c] : b->idle_count[c] + K;
  }
}

int mobi_batch_set_parse_mode(mobi_batch *b, int device_parse) {
  if (!b || b->frames_started != 0) return MOBI_E_ARG; // the decoder state lives either in the host parsers or in HBM, not both
  b->parse_mode = device_parse == 2 ? 2 : device_parse != 0;
  b->ls_policy = device_parse == 3 ? 1 : 0;
  b->parse_auto = false;
  return MOBI_OK;
}

uint32_t mobi_batch_quantizer(const mobi_batch *b, int clip) {
  if (!b || clip < 0 || clip >= b->n) return 0;
  if (b->parse_mode) return b->dev_quant.empty() ? 0 : b->dev_quant[clip];
  return b->parsers[clip]->quantizer();
}
uint32_t mobi_batch_yuv_format(const mobi_batch *b, int clip) {
  if (!b || clip < 0 || clip >= b->n) return 0;
  if (b->parse_mode) return b->dev_yuvfmt.empty() ? 0 : b->dev_yuvfmt[clip];
  return b->parsers[clip]->yuv_format();
}
float mobi_batch_last_decode_ms(const mobi_batch *b) { return b ? b->last_decode_ms : 0.f; }
int mobi_batch_stride(const mobi_batch *b) { return b ? b->g.stride : 0; }
int mobi_batch_n_clips(const mobi_batch *b) { return b ? b->n : 0; }

// ---- single stream = batch of one --------------------------------------------------------------------
mobi_dec *mobi_create(uint32_t width, uint32_t height, int version, int device) {
  mobi_batch *b = mobi_batch_create(1, width, height, version, device);
  if (!b) return nullptr;
  // the Bitmap buffer of a single stream (1.2 MB at 640x480) exists from the start: the first mobi_get_argb is then a launch and a copy like
  // every later one, not an allocation (r05: a first call that allocated right after another batch had freed 200 GB was once timed at 5 s)
  if (ensure_argb(b, 1) != MOBI_OK) { mobi_batch_destroy(b); return nullptr; }
  return new mobi_dec{b};
}
void mobi_destroy(mobi_dec *d) {
  if (!d) return;
  mobi_batch_destroy(d->b);
  delete d;
}
int mobi_decode(mobi_dec *d, const uint8_t *data, size_t len, int32_t *offset_inout) {
  if (!d || !data || !offset_inout) return MOBI_E_ARG;
  int rc = MOBI_OK;
  const uint8_t *dp[1] = {data};
  size_t lp[1] = {len};
  int e = mobi_batch_decode(d->b, dp, lp, offset_inout, &rc);
  return e != MOBI_OK ? e : rc;
}
long long mobi_selftest_div239(int device) {
  if (hipSetDevice(device) != hipSuccess) return -1;
  return mobi_launch_div239_check(nullptr);
}
int mobi_get_argb(mobi_dec *d, uint32_t *out) { return d ? mobi_batch_get_argb(d->b, 0, out) : MOBI_E_ARG; }
int mobi_get_planes(mobi_dec *d, int ring_idx, uint8_t *y_out, uint8_t *uv_out) { return d ? mobi_batch_get_planes(d->b, 0, ring_idx, y_out, uv_out) : MOBI_E_ARG; }
int mobi_stride(const mobi_dec *d) { return d ? d->b->g.stride : 0; }
uint32_t mobi_quantizer(const mobi_dec *d) { return d ? mobi_batch_quantizer(d->b, 0) : 0; }
uint32_t mobi_yuv_format(const mobi_dec *d) { return d ? mobi_batch_yuv_format(d->b, 0) : 0; }
uint32_t mobi_width(const mobi_dec *d) { return d ? (uint32_t)d->b->g.width : 0; }
uint32_t mobi_height(const mobi_dec *d) { return d ? (uint32_t)d->b->g.height : 0; }
