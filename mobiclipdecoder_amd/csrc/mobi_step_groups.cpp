// mobi_step_groups.cpp -- frame-parallel groups (mobi_gop.h): mobi_batch_gop_begin / mobi_batch_gop_finish and the call that is both, mobi_batch_decode_gop
#include "mobi_batch.h"

// ---- frame-parallel groups (mobi_gop.h) -------------------------------------------------------------------------------------------
// K consecutive frames of every clip in one call: data / len / offsets / rc are [k * n_clips + c].  The frames are parsed SIDE BY SIDE --
// n * K virtual clips for the parse kernels, whose cost per frame falls with the number of lanes they are given -- and
// reconstructed as K steps in order.  begin: gather + upload (and, when nothing else is in flight, the parse); finish: the host parser's
// share and every hand-over, the K reconstruction steps, and the parse of the group begun behind it.
// Everything a group's parse and reconstruction write, sized when the group is BEGUN: a group that does not fit is refused by
// mobi_batch_gop_begin, with nothing enqueued (the parse of a group begun behind another goes out inside that one's mobi_batch_gop_finish:
// an allocation failing there would leave rings and parsers out of step).
static int gop_reserve(mobi_batch *b, mobi_batch::GopSlot &S) {
  const int n = b->n, K = S.K, n_mbs = b->g.mbw * b->g.mbh;
  const size_t nv = (size_t)n * K;
  if (S.max_len > b->dp_len_hint) b->dp_len_hint = S.max_len + S.max_len / 4;
  const size_t cap_words = std::min<size_t>((size_t)n_mbs * 448 + MOBI_WIDE_PARAMS, (size_t)n_mbs * 64 + (8 * b->dp_len_hint + 2) / 3) + 448 + 64; // (dp_parse has the bound's reasons)
  S.cap_words = cap_words;
  if (int e = S.d_desc.reserve(align_up(nv * n_mbs * sizeof(MbDesc) + 8 * sizeof(MbDesc), kAlign))) return e;
  if (int e = S.d_pay.reserve(align_up(nv * cap_words * 4 + kPaySlack, kAlign))) return e;
  if (int e = S.d_items.reserve(nv * n_mbs * 4)) return e;
  if (int e = S.d_res.reserve(nv * sizeof(MobiDevResult))) return e;
  if (int e = S.d_sin.reserve(nv * sizeof(MobiDevState))) return e;
  if (int e = S.d_sout.reserve(nv * sizeof(MobiDevState))) return e;
  if (int e = S.d_sls.reserve(nv * sizeof(MobiDevState))) return e;
  if (int e = S.d_tails.reserve(nv * sizeof(MobiDevTail))) return e;
  if (int e = S.d_fault.reserve(nv * sizeof(int))) return e;
  if (b->g.width < b->g.stride) { // the wavefront-ordered intra items (mobi_launch_gop_sort), for the most a group can hold: sized here, not when the
    // counts are known -- mobi_batch_gop_finish would sit in a hipFree + hipMalloc with the GPU idle whenever a group held more than the last
    if (int e = S.d_sorted.reserve((nv * n_mbs + (size_t)K * (3 * MOBI_SORT_LEVELS + 8)) * 16)) return e;
    if (int e = S.d_hist.reserve((size_t)3 * MOBI_GOP_PARSE_MAX * MOBI_SORT_LEVELS * 4)) return e;
  }
  if (int e = S.h_res.reserve(nv * sizeof(MobiDevResult))) return e;
  if (int e = S.h_fault.reserve(nv * sizeof(int))) return e;
  return MOBI_OK;
}
static int gop_enqueue_parse(mobi_batch *b, mobi_batch::GopSlot &S, hipEvent_t after = nullptr) {
  const int n = b->n, K = S.K;
  const size_t nv = (size_t)n * K;
  S.is_host.assign(b->on_host.begin(), b->on_host.end());
  uint32_t *blen = (uint32_t *)(S.h_stage.p + nv * 8);
  DpStaged st;
  for (size_t v = 0; v < nv; v++) {
    if (S.is_host[v % n] || (int)(v / n) >= S.live_end((int)(v % n))) { blen[v] = MOBI_DP_SKIP; continue; } // the host parser's clip / an idle slot
    blen[v] = S.lens[v];
    st.n_dev++;
    st.n_iframes += S.lens[v] >= 2 && (S.h_stage.p[S.hdr_bytes + S.boff[v] + 1] & 0x80) != 0;
  }
  S.lockstep = ls_decide(b, st);
  const size_t cap_words = S.cap_words; // (gop_reserve, when the group was begun)
  hipStream_t ps = b->stream_p;
  HIP_TRY(hipStreamWaitEvent(ps, S.ev_up, 0));
  // `after`: the reconstruction steps just enqueued for the group in front go FIRST.  A full parse workgroup takes a CU's whole LDS (36 lanes x
  // 8 waves), the octet kernel's workgroups the rest: left to the dispatcher, the parse got in first, the reconstruction the caller is waiting
  // for sat behind it, and by the time mobi_batch_gop_finish returned the GPU had nothing left to do while the host gathered the next group
  // (24576 clips x 6: 147 ms per group against 62 + 50 of kernels).  In this order the host's turn overlaps the parse.
  if (after) HIP_TRY(hipStreamWaitEvent(ps, after, 0));
  HIP_TRY(hipMemcpyAsync(S.d_bits.p, S.h_stage.p, S.hdr_bytes, hipMemcpyHostToDevice, ps)); // offsets and lengths (with the host parser's clips marked)
  MobiGopArgs G;
  memset(&G, 0, sizeof(G));
  MobiDevParseArgs &pa = G.P;
  pa.bits = S.d_bits.p + S.hdr_bytes;
  pa.bit_off = (const uint64_t *)S.d_bits.p;
  pa.bit_len = (const uint32_t *)(S.d_bits.p + nv * 8);
  pa.tables = b->d_ptables;
  pa.state_in = (const MobiDevState *)S.d_sin.p; pa.state_out = (MobiDevState *)S.d_sout.p;
  pa.tail_in = nullptr; pa.tail_out = (MobiDevTail *)S.d_tails.p;
  pa.scale = b->d_scale;
  pa.state_ls = (MobiDevState *)S.d_sls.p;
  pa.lockstep = S.lockstep ? 2 : 0;
  pa.pay_local = 1;
  pa.clip_mod = n;
  pa.skip_tail = 1;
  pa.desc = (MbDesc *)S.d_desc.p;
  pa.payload = (uint32_t *)S.d_pay.p;
  pa.items = (uint32_t *)S.d_items.p;
  pa.res = (MobiDevResult *)S.d_res.p;
  pa.pay_cap = (uint32_t)cap_words;
  pa.n_clips = (int)nv; pa.version = b->version;
  pa.width = b->g.width; pa.height = b->g.height; pa.stride = b->g.stride; pa.lg = b->g.lg; pa.mbw = b->g.mbw; pa.mbh = b->g.mbh;
  const int in = b->ps_cur, out = (b->ps_cur + 1) % 3;
  // clips reset from this group on: a new decoder's state into the entry the group starts from (behind dp_return_list, same stream)
  if (S.n_reset && mobi_launch_reset_state((const int32_t *)(S.d_bits.p + S.reset_off), S.n_reset, n, b->d_pstate[in], b->d_ptail[in], ps) != 0)
    return MOBI_E_DEVICE;
  G.ring_in = b->d_pstate[in]; G.ring_out = b->d_pstate[out];
  G.rtail_in = b->d_ptail[in]; G.rtail_out = b->d_ptail[out];
  G.n = n; G.K = K;
  if (S.n_idle) { // the idle slots' empty rows, in front of the parse kernels (mobi_idle.hip); their clips' chains end at idle_from (mobi_gop.h)
    G.idle_from = S.d_bits.p + S.idle_off + align_up((size_t)S.n_idle * 4, 16);
    MobiIdleArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.clips = (const int32_t *)(S.d_bits.p + S.idle_off); ia.count = S.n_idle;
    ia.idle_from = G.idle_from;
    ia.n = n; ia.K = K; ia.n_mbs = b->g.mbw * b->g.mbh;
    ia.desc = pa.desc; ia.res = pa.res;
    if (mobi_launch_idle_rows(&ia, ps) != 0) return MOBI_E_DEVICE;
    b->idle_launches++;
  }
  if (b->ktiming && !b->ev_p0) { (void)hipEventCreate(&b->ev_p0.h); (void)hipEventCreate(&b->ev_p1.h); }
  const bool ptime = b->ktiming && b->ev_p0 && b->ev_p1;
  if (ptime) (void)hipEventRecord(b->ev_p0, ps);
  if (mobi_launch_gop_prepare(&G, ps) != 0) return MOBI_E_DEVICE;
  if (mobi_launch_parse(&pa, ps) != 0) return MOBI_E_DEVICE;
  if (mobi_launch_gop_chain(&G, ps) != 0) return MOBI_E_DEVICE;
  if (ptime) (void)hipEventRecord(b->ev_p1, ps);
  HIP_TRY(hipMemcpyAsync(S.h_res.p, S.d_res.p, nv * sizeof(MobiDevResult), hipMemcpyDeviceToHost, ps));
  HIP_TRY(hipEventRecord(S.ev_parsed, ps));
  b->ps_cur = out;
  S.ring_in = in;
  S.parse_enqueued = true;
  return MOBI_OK;
}

int mobi_batch_gop_begin(mobi_batch *b, int n_frames, const uint8_t *const *data, const size_t *len, const int32_t *offsets) {
  if (!b || !data || !len || !offsets || n_frames < 1 || n_frames > MOBI_GOP_PARSE_MAX) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  const int n = b->n, K = n_frames, n_mbs = b->g.mbw * b->g.mbh;
  const size_t nv = (size_t)n * K;
  // a batch fed by groups parses on the GPU from its first frame ("mutates the batch configuration ... before the ... checks": kept as it was)
  settle_parse_mode(b, b->frames_started == 0 && b->async_seq == 0 && b->gop_count == 0, 0, true);
  if (b->poisoned) return MOBI_E_DEVICE;
  if (b->parse_mode == 0) return MOBI_E_ARG; // the decoder state of this batch lives in the host parsers (mobi_batch_decode_gop serves those too)
  if (!b->version_known()) return MOBI_E_VERSION;
  if (b->g.mbw > 64 || b->async_count || b->gop_count >= 2 || nv >= ((size_t)1 << 22)) return MOBI_E_ARG;
  std::vector<uint8_t> idle_from; // [c] first idle frame (mobi_batch_set_idle); empty: the group has no idle slot
  if (int e = idle_check(b, K, idle_from)) return e;
  const bool dev_state = b->d_pstate[0] != nullptr;
  if (int e = dp_init(b)) return e;
  if (b->gop_count == 0) b->mark_hybrid_share();
  mobi_batch::GopSlot &S = b->gslot[(b->gop_head + b->gop_count) & 1];
  if (int e = ensure_event(S.ev_up)) return e;
  if (int e = ensure_event(S.ev_parsed)) return e;
  if (int e = ensure_stream(b->stream2)) return e;
  if (int e = ensure_stream(b->stream_p)) return e;
  const auto t_stage0 = std::chrono::steady_clock::now();
  // the staged image: [bit_off u64 x nv][bit_len u32 x nv][bits: every frame 8-byte aligned, 32 zero bytes behind it]
  constexpr size_t kBitPad = 32;
  S.K = K;
  S.boff.resize(nv); S.lens.resize(nv);
  S.offs.assign(offsets, offsets + nv);
  size_t pos = 0, max_len = 0;
  const size_t frame_bound = (size_t)n_mbs * 4096 + 64; // (dp_stage: bytes beyond cannot influence the parse of one frame)
  S.idle_from = idle_from;
  for (size_t v = 0; v < nv; v++) {
    const int64_t o = offsets[v];
    const bool idle = !idle_from.empty() && v / n >= idle_from[v % n]; // nothing of an idle slot is read, gathered or uploaded
    size_t l = (!idle && data[v] && o >= 0 && (uint64_t)o < len[v]) ? len[v] - (size_t)o : 0;
    l = std::min(l, frame_bound);
    max_len = std::max(max_len, l);
    S.boff[v] = pos;
    S.lens[v] = (uint32_t)l;
    pos += align_up(l + kBitPad, 8);
  }
  pos += 64;
  const size_t list_pos = pos, n_reset = dev_state ? b->reset_list.size() : 0; // the clips reset from this group on, behind the bits
  pos += align_up(n_reset * 4, 16);
  std::vector<int32_t> idle_list; // the clips with an idle slot, then idle_from[n]: for mobi_idle_rows, mobi_gop_prepare and mobi_gop_chain
  for (int c = 0; c < n && !idle_from.empty(); c++)
    if (idle_from[c] < K) idle_list.push_back(c);
  const size_t idle_pos = pos;
  if (!idle_list.empty()) pos += align_up(idle_list.size() * 4, 16) + align_up((size_t)n, 16);
  const size_t hdr_bytes = align_up(nv * 12, 16), need = hdr_bytes + pos;
  if (need > S.h_stage.cap)
    if (int e = S.h_stage.reserve(need + need / 4)) return e;
  if (need > S.d_bits.cap)
    if (int e = S.d_bits.reserve(need + need / 4)) return e;
  uint8_t *hs = S.h_stage.p;
  memcpy(hs, S.boff.data(), nv * 8);
  memset(hs + hdr_bytes + list_pos - 64, 0, 64);
  if (n_reset) memcpy(hs + hdr_bytes + list_pos, b->reset_list.data(), n_reset * 4);
  S.reset_off = hdr_bytes + list_pos;
  S.n_reset = (int)n_reset;
  S.idle_off = hdr_bytes + idle_pos;
  S.n_idle = (int)idle_list.size();
  if (S.n_idle) {
    memcpy(hs + S.idle_off, idle_list.data(), idle_list.size() * 4);
    memcpy(hs + S.idle_off + align_up(idle_list.size() * 4, 16), idle_from.data(), (size_t)n);
  }
  S.hdr_bytes = hdr_bytes; S.bytes = need; S.max_len = max_len;
  auto gather = [&](size_t v) {
    uint8_t *dst = hs + hdr_bytes + S.boff[v];
    const size_t l = S.lens[v];
    if (l) memcpy(dst, data[v] + offsets[v], l);
    memset(dst + l, 0, align_up(l + kBitPad, 8) - l);
  };
  // gathered in chunks by the pool while one of its threads hands the chunk before to the copy engine (dp_stage)
  {
    const int chunks = nv >= 2048 ? 8 : 1;
    std::atomic<int> up_err{0};
    auto start_of = [&](size_t v) { return v < nv ? hdr_bytes + (size_t)S.boff[v] : need; };
    for (int k = 0; k <= chunks; k++) {
      const size_t c0 = k < chunks ? nv * k / chunks : nv, c1 = k < chunks ? nv * (k + 1) / chunks : nv;
      const size_t u0 = k >= 1 ? nv * (k - 1) / chunks : 0, u1 = k >= 1 ? nv * k / chunks : 0;
      const int n_up = u1 > u0 ? 1 : 0;
      if (n_up + (c1 - c0) == 0) continue;
      constexpr size_t kRun = 64; // frames per task: one per frame had the pool's threads queue at its counter (122 880 frames of 256x192: 8 ms)
      b->pool->run(n_up + (int)((c1 - c0 + kRun - 1) / kRun), [&](int j) {
        if (j < n_up) {
          const size_t a = start_of(u0), e = start_of(u1);
          if (e > a && (hipSetDevice(b->device) != hipSuccess || hipMemcpyAsync(S.d_bits.p + a, hs + a, e - a, hipMemcpyHostToDevice, b->stream2) != hipSuccess)) up_err = 1;
          return;
        }
        for (size_t v = c0 + (size_t)(j - n_up) * kRun, e = std::min(c1, v + kRun); v < e; v++) gather(v);
      });
    }
    if (up_err) { (void)hipStreamSynchronize(b->stream2); return MOBI_E_DEVICE; }
  }
  HIP_TRY(hipEventRecord(S.ev_up, b->stream2));
  b->last_stage_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_stage0).count();
  S.parse_enqueued = false;
  S.resolved = S.returned = false;
  S.done = 0;
  if (int e = gop_reserve(b, S)) { (void)hipStreamSynchronize(b->stream2); return e; } // (does not fit: refused, nothing of it is in flight)
  // the group is handed over: the pending resets' host side now (the routing its parse is enqueued with, here or in the finish in front)
  S.serial = b->handover + 1;
  reset_apply_host(b, S.serial);
  idle_commit(b, K, idle_from);
  reset_commit(b, S.serial);
  b->gop_count++;
  if (b->gop_count == 1) // nothing in front: the parse may start at once (else mobi_batch_gop_finish of the group in front enqueues it, once it knows whose clips are whose)
    if (int e = gop_enqueue_parse(b, S)) { (void)hipStreamSynchronize(b->stream2); (void)hipStreamSynchronize(b->stream_p); b->gop_count--; return e; }
  return MOBI_OK;
}

// ---- the phases of mobi_batch_gop_finish, in the order it calls them ----
// frames host_from[c] .. K - 1 of the clips `cl`, through the host parser of the group's stream, into gop_frames
static void gop_host_parse(mobi_batch *b, mobi_batch::GopSlot &S, const std::vector<int> &cl) {
  const int n = b->n, K = S.K;
  auto &host_from = S.host_from, &hslot = S.hslot, &hrc = S.hrc; auto &hoff = S.hoff; auto &hq = S.hq, &hy = S.hy; auto &hready = S.hready;
  b->pool->run((int)cl.size(), [&](int j) {
    const int c = cl[j];
    for (int k = host_from[c], ke = S.live_end(c); k < ke; k++) { // (the pool skips the clip's idle frames)
      const size_t v = (size_t)k * n + c;
      int32_t off = 0;
      MobiStreamParser *p = b->parser_at(S.serial, c); // (the group's stream: a reset handed over with the group behind it left it retired)
      hrc[v] = p->parse_frame(S.h_stage.p + S.hdr_bytes + S.boff[v], S.lens[v], &off, b->gop_frames[(size_t)hslot[c] * K + k]);
      hoff[v] = S.offs[v] + off;
      hready[v] = hrc[v] == MOBI_OK && p->device_ready();
      hq[v] = p->quantizer();
      hy[v] = p->yuv_format();
    }
  });
}
// 1. the host parser's clips, all K frames of each, while the GPU parses the others
static void gop_host_share(mobi_batch *b, mobi_batch::GopSlot &S, std::vector<int> &host_clips) {
  const int n = b->n, K = S.K;
  const size_t nv = (size_t)n * K;
  auto &host_from = S.host_from, &hslot = S.hslot, &hrc = S.hrc; auto &hoff = S.hoff; auto &hq = S.hq, &hy = S.hy; auto &hready = S.hready;
  host_from.assign(n, K); // first frame of the group that is the host parser's
  hslot.assign(n, -1);    // its place in gop_frames
  hrc.assign(nv, MOBI_OK);
  hoff.assign(nv, 0);
  hq.assign(nv, 0); hy.assign(nv, 0); // Quantizer / YuvFormat behind a host-parsed frame
  hready.assign(nv, 0);               // a host-parsed frame the device parsers would have finished too (MobiStreamParser::device_ready)
  for (int c = 0; c < n; c++)
    if (S.is_host[c]) { host_from[c] = 0; hslot[c] = (int)host_clips.size(); host_clips.push_back(c); }
  if (b->gop_frames.size() < host_clips.size() * K) b->gop_frames.resize(host_clips.size() * K);
  gop_host_parse(b, S, host_clips);
}
// 2. what the device parsers finished; fb: the clips with a frame they could not finish, the host parser's from that frame on
static int gop_device_results(mobi_batch *b, mobi_batch::GopSlot &S, const std::vector<int> &host_clips, std::vector<int> &fb, std::chrono::steady_clock::time_point q0) {
  const int n = b->n, K = S.K;
  auto &host_from = S.host_from, &hslot = S.hslot;
  HIP_TRY(hipEventSynchronize(S.ev_parsed));
  b->phase_ms[0] = ms_since(q0);
  { const bool ptime = b->ktiming && b->ev_p0 && b->ev_p1; float ms = 0; if (ptime && hipEventElapsedTime(&ms, b->ev_p0, b->ev_p1) == hipSuccess) b->last_parse_ms = ms; }
  const MobiDevResult *res = (const MobiDevResult *)S.h_res.p;
  for (int c = 0; c < n; c++) {
    if (S.is_host[c]) continue;
    for (int k = 0, ke = S.live_end(c); k < ke; k++)
      if (res[(size_t)k * n + c].rc != MOBI_OK) { host_from[c] = k; fb.push_back(c); break; }
  }
  if (!fb.empty()) { // hand-overs: the state the first unfinished frame started from (mobi_gop_chain left the true one in its start slot) and the tail before it
    const size_t rec = sizeof(MobiDevState) + sizeof(MobiDevTail);
    if (int e = S.h_seed.reserve(fb.size() * rec)) return e;
    for (size_t j = 0; j < fb.size(); j++) {
      const int c = fb[j], k = host_from[c];
      const size_t v = (size_t)k * n + c;
      HIP_TRY(hipMemcpyAsync(S.h_seed.p + j * rec, (const MobiDevState *)S.d_sin.p + v, sizeof(MobiDevState), hipMemcpyDeviceToHost, b->stream_p));
      const MobiDevTail *t = k == 0 ? b->d_ptail[S.ring_in] + c : (const MobiDevTail *)S.d_tails.p + (v - n);
      HIP_TRY(hipMemcpyAsync(S.h_seed.p + j * rec + sizeof(MobiDevState), t, sizeof(MobiDevTail), hipMemcpyDeviceToHost, b->stream_p));
    }
    HIP_TRY(hipStreamSynchronize(b->stream_p));
    const size_t base = host_clips.size();
    if (b->gop_frames.size() < (base + fb.size()) * K) b->gop_frames.resize((base + fb.size()) * K);
    for (size_t j = 0; j < fb.size(); j++) {
      const int c = fb[j];
      hslot[c] = (int)(base + j);
      b->parser_at(S.serial, c)->import_state(*(const MobiDevState *)(S.h_seed.p + j * rec), *(const MobiDevTail *)(S.h_seed.p + j * rec + sizeof(MobiDevState)));
    }
    gop_host_parse(b, S, fb);
    for (int c : fb)
      if (!b->stale(S.serial, c)) b->route_to_host(c); // (stale: reset since, the clip's routing is a new decoder's)
    b->fallbacks += fb.size();
  }
  return MOBI_OK;
}
// 3. the host parser's command lists over the rows the parse kernels left, frame by frame
static int gop_overrides(mobi_batch *b, mobi_batch::GopSlot &S, const std::vector<int> &host_clips, const std::vector<int> &fb) {
  const int n = b->n, K = S.K, n_mbs = b->g.mbw * b->g.mbh;
  const size_t nv = (size_t)n * K;
  auto &host_from = S.host_from, &hslot = S.hslot, &hrc = S.hrc, &all_host = S.all_host;
  const size_t desc_b = (size_t)n_mbs * sizeof(MbDesc), item_b = (size_t)n_mbs * 4;
  HIP_TRY(hipStreamWaitEvent(b->stream, S.ev_parsed, 0));
  all_host = host_clips;
  all_host.insert(all_host.end(), fb.begin(), fb.end());
  std::sort(all_host.begin(), all_host.end());
  for (int k = 0; k < K && !all_host.empty(); k++) {
    std::vector<int> cl;
    std::vector<const ParsedFrame *> fr;
    std::vector<int> rcs;
    for (int c : all_host)
      if (host_from[c] <= k && k < S.live_end(c)) { // (an idle frame's rows are mobi_idle_rows')
        const size_t v = (size_t)k * n + c;
        cl.push_back(c);
        rcs.push_back(hrc[v]);
        fr.push_back(hrc[v] == MOBI_OK ? &b->gop_frames[(size_t)hslot[c] * K + k] : nullptr);
      }
    const size_t kn = (size_t)k * n;
    const DpRows rows{S.d_desc.p + kn * desc_b, S.d_pay.p + kn * S.cap_words * 4, S.d_items.p + kn * item_b, (MobiDevResult *)S.d_res.p + kn, S.cap_words};
    if (int e = dp_override(b, cl, nullptr, S.h_over[k], rows, b->stream, fr.data(), rcs.data())) return e;
  }
  HIP_TRY(hipMemsetAsync(S.d_fault.p, 0, nv * sizeof(int), b->stream));
  return MOBI_OK;
}
// 3b. the intra macroblocks of every frame of the group as launch items in wavefront order, built on the device behind the overrides (mobi_gop.h)
// (the wavefront order holds where the halo's linear addresses do not wrap: in a picture as wide as its stride -- 256, 512, 1024 -- the
// first macroblock of a row reads the LAST one of the row above, MD.cs:212-217 with Stride == Width; those keep the raster-order launch)
static int gop_sort(mobi_batch *b, mobi_batch::GopSlot &S) {
  const int n = b->n, K = S.K, n_mbs = b->g.mbw * b->g.mbh;
  auto &host_from = S.host_from, &hslot = S.hslot, &hrc = S.hrc;
  const MobiDevResult *res = (const MobiDevResult *)S.h_res.p;
  S.sorted = b->g.width < b->g.stride;
#if defined(MOBI_PROFILING)
  if (const char *e = getenv("MOBI_GOP_INTRA_SORT")) S.sorted = S.sorted && atoi(e) != 0; // (A/B: 0 = the raster-order launch, mobi_recon_intra_cl)
#endif
  if (S.sorted) {
    MobiGopSortArgs A;
    memset(&A, 0, sizeof(A));
    uint64_t off = 0;
    for (int k = 0; k < K; k++) {
      uint64_t sum = 0;
      for (int c = 0; c < n; c++) {
        const size_t v = (size_t)k * n + c;
        if (k >= S.live_end(c)) continue; // (the sort counts nothing for an idle slot)
        sum += k >= host_from[c] ? (hrc[v] == MOBI_OK ? b->gop_frames[(size_t)hslot[c] * K + k].hdr.n_intra : 0u) : res[v].n_intra;
      }
      S.sorted_items[k] = sum ? (uint32_t)(align_up(sum, 4) + 3 * MOBI_SORT_LEVELS + 4) & ~3u : 0u; // (every wavefront starts on a wave of four: at most three rows of padding each)
      S.sorted_off[k] = off;
      A.sorted_off[k] = off;
      A.sorted_cap[k] = S.sorted_items[k];
      off += S.sorted_items[k];
    }
    if (off) {
      const size_t hist_b = (size_t)K * MOBI_SORT_LEVELS * 4;
      if (int e = S.d_sorted.reserve(off * 16)) return e;
      if (int e = S.d_hist.reserve(3 * hist_b)) return e;
      HIP_TRY(hipMemsetAsync(S.d_hist.p, 0, 2 * hist_b, b->stream));
      A.desc = (const MbDesc *)S.d_desc.p;
      A.items = (const uint32_t *)S.d_items.p;
      A.res = (const MobiDevResult *)S.d_res.p;
      A.hist = (uint32_t *)S.d_hist.p;
      A.cursor = (uint32_t *)(S.d_hist.p + hist_b);
      A.start = (uint32_t *)(S.d_hist.p + 2 * hist_b);
      A.sorted = (uint32_t *)S.d_sorted.p;
      A.n = n; A.K = K; A.n_mbs = n_mbs; A.mbw = b->g.mbw;
      if (mobi_launch_gop_sort(&A, b->stream) != 0) return MOBI_E_DEVICE;
    }
  }
  return MOBI_OK;
}
// 4. the reconstruction steps k0 .. k1 - 1 of this part -- at most six: the ring holds six pictures -- from consecutive command lists
static int gop_recon_part(mobi_batch *b, mobi_batch::GopSlot &S, int k0, int k1) {
  const int n = b->n, K = S.K, n_mbs = b->g.mbw * b->g.mbh;
  auto &host_from = S.host_from, &hslot = S.hslot, &hrc = S.hrc;
  const size_t desc_b = (size_t)n_mbs * sizeof(MbDesc), item_b = (size_t)n_mbs * 4;
  const MobiDevResult *res = (const MobiDevResult *)S.h_res.p;
  for (int k = k0; k < k1; k++) {
    const size_t kn = (size_t)k * n;
    uint32_t Kint = 0;
    for (int c = 0; c < n; c++) {
      const size_t v = kn + c;
      if (k >= S.live_end(c)) continue;
      if (k >= host_from[c]) { if (hrc[v] == MOBI_OK) Kint = std::max(Kint, b->gop_frames[(size_t)hslot[c] * K + k].hdr.n_intra); }
      else Kint = std::max(Kint, res[v].n_intra);
    }
    if (int e = b->begin_step()) return e;
    MobiReconArgs a = b->args(S.d_desc.p + kn * desc_b, S.d_pay.p + kn * S.cap_words * 4);
    a.pay_clip_words = (uint32_t)S.cap_words;
    a.fault = (int *)S.d_fault.p + kn;
    mobi_batch::EvPair ep{nullptr, nullptr, 0};
    if (b->ktiming) { ep.a = b->get_event(); ep.b = b->get_event(); (void)hipEventRecord(ep.a, b->stream); }
    if (mobi_launch_inter(&a, b->stream) != 0) return MOBI_E_DEVICE;
    if (b->ktiming) { (void)hipEventRecord(ep.b, b->stream); b->evs.push_back(ep); }
    const MobiDevResult *d_res_k = (const MobiDevResult *)S.d_res.p + kn;
    if (S.sorted) {
      if (S.sorted_items[k] && mobi_launch_intra(&a, (const uint32_t *)S.d_sorted.p + S.sorted_off[k] * 4, (int)S.sorted_items[k], b->stream) != 0) return MOBI_E_DEVICE;
    } else if (Kint && mobi_launch_intra_cl(&a, (const uint32_t *)(S.d_items.p + kn * item_b), &d_res_k->n_intra, (int)(sizeof(MobiDevResult) / 4), (int)Kint, 0, b->stream) != 0)
      return MOBI_E_DEVICE;
  }
  b->pay_clip_words = (uint32_t)S.cap_words;
  HIP_TRY(hipMemcpyAsync(S.h_fault.p + (size_t)k0 * n * sizeof(int), S.d_fault.p + (size_t)k0 * n * sizeof(int), (size_t)(k1 - k0) * n * sizeof(int), hipMemcpyDeviceToHost, b->stream));
  return MOBI_OK;
}
// 5. clips that go back to the device parsers (dp_return's rule, counted in frames): their state into the entry the next parse reads
static int gop_return_clips(mobi_batch *b, mobi_batch::GopSlot &S) {
  const int n = b->n, K = S.K;
  auto &host_from = S.host_from, &all_host = S.all_host; auto &hready = S.hready;
  std::vector<int> back;
  for (int c : all_host) {
    if (b->host_share[c] || b->stale(S.serial, c)) continue;
    int run = b->clean_run[c]; // consecutive frames the device parsers would have finished too
    for (int k = host_from[c], ke = S.live_end(c); k < ke; k++) run = hready[(size_t)k * n + c] ? run + 1 : 0;
    b->clean_run[c] = (uint16_t)std::min(60000, run);
    if (run >= b->clean_need[c]) back.push_back(c);
  }
  return dp_return_list(b, back, b->ps_cur, S.h_ret, b->stream_p);
}
  // 6. the group begun behind this one: its parse goes out behind the reconstruction steps of this group's LAST part.  Parse and reconstruction
  // do not share the GPU (a full parse workgroup takes a CU's whole LDS), so the parse belongs where only the host is busy: a part's steps
  // are waited for before the call returns, the caller's next move behind the last part is the gather and upload of the group after next
  // (mobi_batch_gop_begin: tens of ms at 131 072 frames) -- with the parse in the queue the GPU works through that; with the parse sent out
  // with the FIRST part (r06 until its last hours) it ran while the host sat in the second part's wait, and the GPU idled through the gather
  // (4096 clips x 32 frames: 3.4 -> 2.9 - 3.2 ms per frame step; groups of one part are the same either way).
static int gop_parse_next(mobi_batch *b, mobi_batch::GopSlot &S, bool last) {
  bool parse_now = last;
#if defined(MOBI_PROFILING)
  static const int parse_first = getenv("MOBI_GOP_PARSE_FIRST") ? atoi(getenv("MOBI_GOP_PARSE_FIRST")) : 0; // (A/B: with the group's first part)
  if (parse_first) parse_now = true;
#endif
  if (b->gop_count == 2 && parse_now) {
    mobi_batch::GopSlot &N = b->gslot[(b->gop_head + 1) & 1];
    if (!N.parse_enqueued) {
      if (int e = ensure_event(S.ev_recon)) return e;
      HIP_TRY(hipEventRecord(S.ev_recon, b->stream));
      if (int e = gop_enqueue_parse(b, N, S.ev_recon)) return e;
    }
  }
  return MOBI_OK;
}
// what the frames k0 .. k1 - 1 came to: rc, Offset, and Quantizer / YuvFormat behind the part's last frame
static void gop_report(mobi_batch *b, mobi_batch::GopSlot &S, int k0, int k1, int32_t *offsets_out, int *rc) {
  const int n = b->n;
  auto &host_from = S.host_from, &hrc = S.hrc; auto &hoff = S.hoff; auto &hq = S.hq, &hy = S.hy;
  const MobiDevResult *res = (const MobiDevResult *)S.h_res.p;
  const int *fault = (const int *)S.h_fault.p;
  if (k0 == 0) b->ls_finished = S.lockstep ? 0 : -1;
  b->lockstep = S.lockstep;
  for (int k = k0; k < k1; k++)
    for (int c = 0; c < n; c++) {
      const size_t v = (size_t)k * n + c, o = (size_t)(k - k0) * n + c; // (the part's results count from its first frame)
      if (k >= S.live_end(c)) { // an idle slot: Offset as handed in
        rc[o] = MOBI_IDLE;
        if (offsets_out) offsets_out[o] = S.offs[v];
        continue;
      }
      if (k >= host_from[c]) {
        rc[o] = hrc[v];
        if (offsets_out) offsets_out[o] = hoff[v];
      } else {
        if (S.lockstep && res[v].pad == MOBI_LS_MAGIC) b->ls_finished++;
        rc[o] = res[v].rc;
        if (offsets_out) offsets_out[o] = S.offs[v] + (int32_t)res[v].consumed;
      }
      rc[o] = fault_rc(rc[o], fault[v]);
      if (k == std::min(k1, S.live_end(c)) - 1) { // (behind the part's last LIVE frame of the clip)
        b->dev_quant[c] = k >= host_from[c] ? hq[v] : res[v].quant;
        b->dev_yuvfmt[c] = k >= host_from[c] ? hy[v] : res[v].yuvfmt;
      }
    }
}

int mobi_batch_gop_finish(mobi_batch *b, int32_t *offsets_out, int *rc) {
  if (!b || !rc) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  if (b->poisoned) return MOBI_E_DEVICE;
  if (b->gop_count == 0) return MOBI_E_ARG;
  mobi_batch::GopSlot &S = b->gslot[b->gop_head & 1];
  const int K = S.K;
  // whatever fails from here on leaves rings, parsers and state ring out of step: the batch is drained and refuses further work
  Poison poison{b};
  if (!S.parse_enqueued)
    if (int e = gop_enqueue_parse(b, S)) return e;
  const auto q0 = std::chrono::steady_clock::now();
  if (!S.resolved) { // the group's first finish: whose frames are whose, for all K of them
    std::vector<int> host_clips, fb;
    gop_host_share(b, S, host_clips);
    if (int e = gop_device_results(b, S, host_clips, fb, q0)) return e;
    b->phase_ms[1] = ms_since(q0);
    if (int e = gop_overrides(b, S, host_clips, fb)) return e;
    if (int e = gop_sort(b, S)) return e;
    S.resolved = true;
    S.done = 0;
  }
  const int k0 = S.done, k1 = std::min(K, k0 + 6);
  const bool last = k1 == K;
  if (int e = gop_recon_part(b, S, k0, k1)) return e;
  b->phase_ms[2] = ms_since(q0);
  // (what the next parse needs to know -- whose clips are whose -- is settled once the group is resolved: the clips that go back are sent with the first part)
  if (!S.returned) {
    S.returned = true;
    if (int e = gop_return_clips(b, S)) return e;
  }
  if (int e = gop_parse_next(b, S, last)) return e;
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->phase_ms[3] = ms_since(q0);
  b->drain_events();
  poison.armed = false;
  gop_report(b, S, k0, k1, offsets_out, rc);
  S.done = k1;
  if (last) {
    b->gop_head ^= 1;
    b->gop_count--;
    S.parse_enqueued = false;
    S.resolved = S.returned = false;
  }
  return MOBI_OK;
}
// frames of the OLDEST group begun that mobi_batch_gop_finish has not reported yet (0: no group is begun); the next finish reports min(6, that)
int mobi_batch_gop_frames_pending(const mobi_batch *b) {
  if (!b || b->gop_count == 0) return 0;
  const mobi_batch::GopSlot &S = b->gslot[b->gop_head & 1];
  return S.K - (S.resolved ? S.done : 0);
}
int mobi_batch_gop_in_flight(const mobi_batch *b) { return b ? b->gop_count : 0; }

int mobi_batch_decode_gop(mobi_batch *b, int n_frames, const uint8_t *const *data, const size_t *len, int32_t *offsets, int *rc) {
  if (!b || !data || !len || !offsets || !rc || n_frames < 1 || n_frames > MOBI_GOP_MAX) return MOBI_E_ARG;
  if (b->poisoned) return MOBI_E_DEVICE;
  if (b->async_count || b->gop_count) return MOBI_E_ARG;
  const int n = b->n;
  if (b->parse_auto) settle_parse_mode(b, b->frames_started == 0, (size_t)n * n_frames, false); // as mobi_batch_decode chooses, with the lanes a group offers counted: n_clips * n_frames
  if (b->parse_mode == 0 || (size_t)n * n_frames >= ((size_t)1 << 22) || !b->version_known()) {
    std::vector<uint8_t> idle_from, mask;
    if (int e = idle_check(b, n_frames, idle_from)) return e; // the group's idle mask: checked as a whole before anything changes, then row by row
    if (b->idle_frames) mask.swap(b->idle_mask);
    b->idle_frames = 0;
    for (int k = 0; k < n_frames; k++) { // the host parser's batch (or a version no parser knows): K calls, the same results
      if (!idle_from.empty() && mobi_batch_set_idle(b, mask.data() + (size_t)k * n, 1) != MOBI_OK) return MOBI_E_DEVICE;
      if (int e = mobi_batch_decode(b, data + (size_t)k * n, len + (size_t)k * n, offsets + (size_t)k * n, rc + (size_t)k * n)) return e;
    }
    return MOBI_OK;
  }
  if (int e = mobi_batch_gop_begin(b, n_frames, data, len, offsets)) return e;
  return mobi_batch_gop_finish(b, offsets, rc);
}
