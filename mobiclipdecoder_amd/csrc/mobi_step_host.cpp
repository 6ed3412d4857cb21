// mobi_step_host.cpp -- mobi_batch_decode: DecodeFrame() of every clip of a batch; the host-parsed pipeline (device-parsed: mobi_step_device.cpp)
#include "mobi_batch.h"

int mobi_batch_decode(mobi_batch *b, const uint8_t *const *data, const size_t *len, int32_t *offsets, int *rc) {
  if (!b || !data || !len || !offsets || !rc) return MOBI_E_ARG;
  if (b->poisoned) return MOBI_E_DEVICE;
  HIP_TRY(hipSetDevice(b->device));
  struct CallTimer { // wall time of this call, for the end-to-end measurements (tools/exp_dparse.py)
    mobi_batch *b;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~CallTimer() { b->last_decode_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
  } call_timer{b};
  if (b->gop_count) return MOBI_E_ARG; // (groups in flight: mobi_batch_gop_finish first)
  settle_parse_mode(b, b->frames_started == 0, (size_t)b->n, false, data, len, offsets);
  if (b->parse_mode) return decode_device_parse(b, data, len, offsets, rc);
  std::vector<uint8_t> idle; // [clip] 0: an idle slot (mobi_batch_set_idle): the pool skips the clip, its command list is empty; empty: none
  if (int e = idle_check(b, 1, idle)) return e;
  { // clips reset since the last step: a new parser each (parse mode 0 keeps no decoder state on the device)
    const uint64_t serial = b->handover + 1;
    reset_apply_host(b, serial);
    idle_commit(b, 1, idle);
    reset_commit(b, serial);
  }
  const int n = b->n;
  // 1. host: serial VLC parse of one frame per clip -> command lists.  The clips are taken in chunks, three stages deep: in one round of
  // the pool chunk k is parsed, chunk k - 1 is written into the staging buffer, and chunk k - 2 is handed to the copy engine (a step of
  // 1024 clips of 640x480 is 100 MB of commands: as long on the bus as it is in the parsers).  A chunk's place in the payload arena is the
  // sum of the chunks before it, so nothing has to wait for the whole batch; only the launch list does (levels are sorted over all clips).
  // The pipelined path needs the step to fit the buffers as they are (they grow in the classic path below, with headroom): the first frame
  // of a batch, and any frame a quarter larger than every one before it, is staged and uploaded after the parse, as all were before r04.
  std::vector<const ParsedFrame *> ok(n, nullptr);
  bool any_version_error = false;
  const int n_mbs = b->g.mbw * b->g.mbh;
  const size_t desc_bytes = align_up((size_t)n * n_mbs * sizeof(MbDesc) + 8 * sizeof(MbDesc), kAlign); // slack: a wave reads up to 8 descriptors at once
  const size_t buf_cap = std::min(b->h_stage.cap, b->d_cmd.cap);
  const size_t cap_words = buf_cap > desc_bytes + kPaySlack + kAlign ? (buf_cap - desc_bytes - kPaySlack - kAlign) / 4 : 0;
  const int chunk = b->host_chunk;
  const int chunks = chunk > 0 && n >= 2 * chunk ? (n + chunk - 1) / chunk : 1;
  bool piped = chunks > 1 && cap_words > 0;
  int uploaded = 0; // clips [0, uploaded) are staged and on their way
  std::vector<size_t> base(n + 1, 0); // where each clip's payload starts in the step's arena (words)
  uint8_t *hs = b->h_stage.p;
  float parse_ms = 0;
  auto stage_range = [&](int c0, int c1) {
    for (int i = c0; i < c1; i++) step_write_clip(ok[i], base[i], n_mbs, (MbDesc *)hs + (size_t)i * n_mbs, (uint32_t *)(hs + desc_bytes));
  };
  auto stage_clips = [&](int c0, int c1) { // every clip writes its own descriptors and payload (at most 32 writers: more threads than that
    const int groups = std::min(c1 - c0, 32); // on the pinned buffer slow each other down -- measured: 34 ms -> 70-90 ms per step of 2048 clips)
    b->pool->run(groups, [&](int g) { stage_range(c0 + (int)((long)(c1 - c0) * g / groups), c0 + (int)((long)(c1 - c0) * (g + 1) / groups)); });
  };
  std::atomic<int> up_err{0};
  auto upload_clips = [&](int c0, int c1) { // (the copy calls hold their thread for as long as the bus is busy: 2.3 ms per 100 MB, measured)
    if (hipSetDevice(b->device) != hipSuccess) { up_err = 1; return; }
    const size_t d0 = (size_t)c0 * n_mbs * sizeof(MbDesc), d1 = (size_t)c1 * n_mbs * sizeof(MbDesc);
    if (hipMemcpyAsync(b->d_cmd.p + d0, hs + d0, d1 - d0, hipMemcpyHostToDevice, b->stream) != hipSuccess) up_err = 1;
    if (base[c1] > base[c0] &&
        hipMemcpyAsync(b->d_cmd.p + desc_bytes + base[c0] * 4, hs + desc_bytes + base[c0] * 4, (base[c1] - base[c0]) * 4, hipMemcpyHostToDevice, b->stream) != hipSuccess)
      up_err = 1;
  };
  // Round k of the pool: the clips of chunk k are parsed; beside them chunk k - 1 (parsed, its place in the arena known) is staged in
  // eight pieces, and chunk k - 2 (staged) is handed to the copy engine by one thread.
  int staged = 0;        // clips [0, staged) are in the staging buffer
  for (int k = 0; k < chunks + 2; k++) {
    const int c0 = k < chunks ? (int)((long)n * k / chunks) : n, c1 = k < chunks ? (int)((long)n * (k + 1) / chunks) : n;
    const int s0 = staged, s1 = piped && k >= 1 ? (int)((long)n * std::min(k, chunks) / chunks) : staged;         // to stage now: parsed chunks not staged yet
    const int u0 = uploaded, u1 = piped ? staged : uploaded;                                                       // to upload now: staged, not uploaded
    const int n_parse = c1 - c0, n_stage = s1 > s0 ? std::min(8, s1 - s0) : 0, n_up = u1 > u0 ? 1 : 0;
    if (n_parse + n_stage + n_up == 0) continue;
    const auto t0 = std::chrono::steady_clock::now();
    b->pool->run(n_up + n_stage + n_parse, [&](int j) {
      if (j < n_up) { upload_clips(u0, u1); return; }
      j -= n_up;
      if (j < n_stage) { stage_range(s0 + (int)((long)(s1 - s0) * j / n_stage), s0 + (int)((long)(s1 - s0) * (j + 1) / n_stage)); return; }
      const int i = c0 + (j - n_stage);
      if (!idle.empty() && idle[i] == 0) { rc[i] = MOBI_IDLE; return; }
      rc[i] = parse_host(b->parsers[i].get(), data[i], len[i], &offsets[i], b->cur[i]);
    });
    parse_ms += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (up_err) piped = false; // (reported below, once the ring has turned and every clip's rc can say so: the parsers have consumed their frames)
    uploaded = u1;
    staged = s1;
    for (int i = c0; i < c1; i++) {
      if (rc[i] == MOBI_OK) ok[i] = &b->cur[i];
      if (rc[i] == MOBI_E_VERSION) any_version_error = true;
      base[i + 1] = base[i] + (ok[i] ? ok[i]->payload.size() : 0);
    }
    if (any_version_error || base[c1] > cap_words) piped = false; // (what is staged already still goes up if it was asked to; the rest waits for the classic path)
  }
  const auto tp1 = std::chrono::steady_clock::now();
  b->last_hostparse_ms = parse_ms;
  if (any_version_error) { // DecodeFrame() returns before touching the ring (MD.cs:56-61)
    if (uploaded) HIP_TRY(hipStreamSynchronize(b->stream)); // (nothing may still be reading the staging buffer when the next call fills it)
    return MOBI_OK;
  }
  // From here on the parsers have consumed the frame and the ring has turned (the two must stay in step: a parser's reference
  // bookkeeping counts frames).  If the call itself fails below, no clip may report MOBI_OK for a frame that was never reconstructed.
  FailAll fail_all{rc, n, b->stream};
  const int guard_rc = b->begin_step();
  if (up_err) return MOBI_E_DEVICE;
  if (guard_rc) return guard_rc;
  if (base[n] + kPaySlack / 4 >= ((uint64_t)1 << 32)) return MOBI_E_ARG; // MbDesc.payload_off is a 32-bit word offset into the step's arena
  LevelPlan plan;
  plan.build(ok, b->g.mbw);
  const auto tp2 = std::chrono::steady_clock::now();
  // 2. what is not on its way yet: [desc table][payload arena] (all of it, if the step did not go chunk by chunk), and the items
  const size_t pay_bytes = align_up(base[n] * 4 + kPaySlack, kAlign);
  const size_t item_bytes = align_up(plan.items.size() * 4 + 4, kAlign);
  if (int e = b->h_items.reserve(item_bytes)) return e;
  if (int e = b->d_items.reserve(item_bytes)) return e;
  const auto t_stage0 = std::chrono::steady_clock::now();
  if (uploaded < n) {
    if (uploaded) HIP_TRY(hipStreamSynchronize(b->stream)); // the buffers may move: nothing of the chunks that did go may be in flight
    const size_t want = desc_bytes + pay_bytes + pay_bytes / 4;  // (headroom: the next steps of this size go chunk by chunk)
    if (int e = b->h_stage.reserve(want)) return e;
    if (int e = b->d_cmd.reserve(want)) return e;
    hs = b->h_stage.p;
    stage_clips(0, n);
    HIP_TRY(hipMemcpyAsync(b->d_cmd.p, hs, desc_bytes + pay_bytes, hipMemcpyHostToDevice, b->stream));
  }
  if (!plan.items.empty()) {
    memcpy(b->h_items.p, plan.items.data(), plan.items.size() * 4);
    HIP_TRY(hipMemcpyAsync(b->d_items.p, b->h_items.p, plan.items.size() * 4, hipMemcpyHostToDevice, b->stream));
  }
  b->last_stage_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_stage0).count(); // (what was not staged under the parse)
  const auto tp3 = std::chrono::steady_clock::now();
  // 3. device: reconstruction
  MobiReconArgs a = b->args(b->d_cmd.p, b->d_cmd.p + desc_bytes);
  if (int e = b->launch_plan(a, plan, (const uint32_t *)b->d_items.p)) return e;
  if (int e = b->read_faults(b->h_fault.data())) return e;
  const auto tp4 = std::chrono::steady_clock::now();
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (b->last_fused) { // a one-launch step whose intra fours gave up waiting (fault bit 2: a dispatch order this library has never seen, see
    bool gave_up = false; // mobi_recon_step): the same step again as two launches, which need no order -- the step only writes ring slot 0
    for (int i = 0; i < n; i++) gave_up = gave_up || (b->h_fault[i] & 2);
    if (gave_up) {
      if (int e = b->launch_plan(a, plan, (const uint32_t *)b->d_items.p, -1, false)) return e;
      if (int e = b->read_faults(b->h_fault.data())) return e;
      HIP_TRY(hipStreamSynchronize(b->stream));
    }
  }
  {
    const auto tp5 = std::chrono::steady_clock::now();
    auto ms = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) { return std::chrono::duration<float, std::milli>(y - x).count(); };
    b->phase_ms[0] = ms(call_timer.t0, tp1); b->phase_ms[1] = ms(tp1, tp2); b->phase_ms[2] = ms(tp2, tp3); b->phase_ms[3] = ms(tp3, tp4); b->phase_ms[4] = ms(tp4, tp5);
  }
  fail_all.armed = false;
  b->drain_events();
  for (int i = 0; i < n; i++) rc[i] = fault_rc(rc[i], b->h_fault[i]);
  return MOBI_OK;
}
