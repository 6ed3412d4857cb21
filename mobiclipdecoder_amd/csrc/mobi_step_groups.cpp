// mobi_step_groups.cpp -- frame-parallel groups (mobi_gop.h): mobi_batch_gop_begin / mobi_batch_gop_finish and the call that is both, mobi_batch_decode_gop.
// The hand-over itself -- staged image, payload bound, parse arguments, idle rows, seeds, overrides, report -- is the steps' (mobi_step_device.cpp,
// mobi_handover.h) at K frames; what is here is the group's own: the chain of states (d_sin / d_sout / d_sls / d_tails), the sort, the K steps.
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
  const int n = b->n, K = S.H.K, n_mbs = b->g.mbw * b->g.mbh;
  const size_t nv = (size_t)n * K;
  if (int e = S.B.reserve_tables(nv, n, n_mbs, dp_cap_words(b, S.img.max_len))) return e;
  if (int e = S.B.reserve_results(nv)) return e;
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
  return S.B.h_fault.reserve(nv * sizeof(int));
}
static int gop_enqueue_parse(mobi_batch *b, mobi_batch::GopSlot &S, hipEvent_t after = nullptr) {
  const int n = b->n;
  DpSet &B = S.B;
  S.is_host.assign(b->on_host.begin(), b->on_host.end());
  S.img.route(B.h_stage.p, S.is_host.data()); // the routing is known: the host parser's lanes are marked
  S.H.lockstep = ls_decide(b, S.img);
  hipStream_t ps = b->stream_p;
  HIP_TRY(hipStreamWaitEvent(ps, B.ev_up, 0));
  // `after`: the reconstruction steps just enqueued for the group in front go FIRST.  A full parse workgroup takes a CU's whole LDS (36 lanes x
  // 8 waves), the octet kernel's workgroups the rest: left to the dispatcher, the parse got in first, the reconstruction the caller is waiting
  // for sat behind it, and by the time mobi_batch_gop_finish returned the GPU had nothing left to do while the host gathered the next group
  // (24576 clips x 6: 147 ms per group against 62 + 50 of kernels).  In this order the host's turn overlaps the parse.
  if (after) HIP_TRY(hipStreamWaitEvent(ps, after, 0));
  HIP_TRY(hipMemcpyAsync(B.bits.p, B.h_stage.p, S.img.hdr_bytes, hipMemcpyHostToDevice, ps)); // offsets and lengths (with the host parser's clips marked)
  MobiGopArgs G;
  memset(&G, 0, sizeof(G));
  MobiDevParseArgs &pa = G.P;
  dp_parse_args(b, S.img, B, pa);
  pa.state_in = (const MobiDevState *)S.d_sin.p; pa.state_out = (MobiDevState *)S.d_sout.p;
  pa.tail_in = nullptr; pa.tail_out = (MobiDevTail *)S.d_tails.p;
  pa.state_ls = (MobiDevState *)S.d_sls.p;
  pa.lockstep = S.H.lockstep ? 2 : 0;
  pa.clip_mod = n;
  pa.skip_tail = 1;
  const int in = b->ps_cur, out = (b->ps_cur + 1) % 3;
  // clips reset from this group on: a new decoder's state into the entry the group starts from (behind dp_return_list, same stream)
  if (S.img.n_reset && mobi_launch_reset_state((const int32_t *)(B.bits.p + S.img.reset_off), S.img.n_reset, n, b->d_pstate[in], b->d_ptail[in], ps) != 0)
    return MOBI_E_DEVICE;
  G.ring_in = b->d_pstate[in]; G.ring_out = b->d_pstate[out];
  G.rtail_in = b->d_ptail[in]; G.rtail_out = b->d_ptail[out];
  G.n = n; G.K = S.H.K;
  if (S.img.n_idle) G.idle_from = B.bits.p + S.img.idle_from_off;
  if (int e = dp_idle_rows(b, S.img, B, pa, false, ps)) return e;
  b->ptimer.start(b->ktiming, ps);
  if (mobi_launch_gop_prepare(&G, ps) != 0) return MOBI_E_DEVICE;
  if (mobi_launch_parse(&pa, ps) != 0) return MOBI_E_DEVICE;
  if (mobi_launch_gop_chain(&G, ps) != 0) return MOBI_E_DEVICE;
  b->ptimer.stop(b->ktiming, ps);
  HIP_TRY(hipMemcpyAsync(B.h_res.p, B.res.p, S.img.lanes() * sizeof(MobiDevResult), hipMemcpyDeviceToHost, ps));
  HIP_TRY(hipEventRecord(B.ev_parsed, ps));
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
  if (int e = ensure_event(S.B.ev_up)) return e;
  if (int e = ensure_event(S.B.ev_parsed)) return e;
  if (int e = ensure_stream(b->stream2)) return e;
  if (int e = ensure_stream(b->stream_p)) return e;
  const auto t0 = std::chrono::steady_clock::now();
  S.H.K = K;
  S.H.offs.assign(offsets, offsets + nv);
  S.H.idle_from = idle_from;
  const uint8_t *idle = idle_from.empty() ? nullptr : idle_from.data();
  const std::vector<int32_t> none, &resets = dev_state ? b->reset_list : none; // the clips reset from this group on
  S.img.plan(n, K, n_mbs, data, len, offsets, nullptr, idle, resets.size(), true); // (whose clips are whose: gop_enqueue_parse)
  if (int e = S.B.h_stage.grow(S.img.bytes)) return e;
  if (int e = S.B.bits.grow(S.img.bytes)) return e;
  if (int e = dp_stage(b, S.img, S.B, data, offsets, idle, resets.data(), 8, 64, b->stream2, false, t0)) { (void)hipStreamSynchronize(b->stream2); return e; }
  HIP_TRY(hipEventRecord(S.B.ev_up, b->stream2));
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
  const int n = b->n, K = S.H.K;
  auto &host_from = S.H.host_from, &hslot = S.hslot, &hrc = S.H.rc; auto &hoff = S.H.off; auto &hq = S.H.quant, &hy = S.H.yuv; auto &hready = S.hready;
  b->pool->run((int)cl.size(), [&](int j) {
    const int c = cl[j];
    for (int k = host_from[c], ke = S.H.live_end(c); k < ke; k++) { // (the pool skips the clip's idle frames)
      const size_t v = (size_t)k * n + c;
      int32_t off = 0;
      MobiStreamParser *p = b->parser_at(S.serial, c); // (the group's stream: a reset handed over with the group behind it left it retired)
      hrc[v] = p->parse_frame(S.B.h_stage.p + S.img.hdr_bytes + S.img.boff[v], S.img.lens[v], &off, b->gop_frames[(size_t)hslot[c] * K + k]);
      hoff[v] = S.H.offs[v] + off;
      hready[v] = hrc[v] == MOBI_OK && p->device_ready();
      hq[v] = p->quantizer();
      hy[v] = p->yuv_format();
    }
  });
}
// 1. the host parser's clips, all K frames of each, while the GPU parses the others
static void gop_host_share(mobi_batch *b, mobi_batch::GopSlot &S, std::vector<int> &host_clips) {
  const int n = b->n, K = S.H.K;
  const size_t nv = (size_t)n * K;
  auto &host_from = S.H.host_from, &hslot = S.hslot; auto &hready = S.hready;
  S.H.clear(n);
  hslot.assign(n, -1);    // the clip's place in gop_frames
  hready.assign(nv, 0);   // a host-parsed frame the device parsers would have finished too (MobiStreamParser::device_ready)
  for (int c = 0; c < n; c++)
    if (S.is_host[c]) { host_from[c] = 0; hslot[c] = (int)host_clips.size(); host_clips.push_back(c); }
  if (b->gop_frames.size() < host_clips.size() * K) b->gop_frames.resize(host_clips.size() * K);
  gop_host_parse(b, S, host_clips);
}
// 2. what the device parsers finished; fb: the clips with a frame they could not finish, the host parser's from that frame on
static int gop_device_results(mobi_batch *b, mobi_batch::GopSlot &S, const std::vector<int> &host_clips, std::vector<int> &fb, std::chrono::steady_clock::time_point q0) {
  const int n = b->n, K = S.H.K;
  auto &host_from = S.H.host_from, &hslot = S.hslot;
  HIP_TRY(hipEventSynchronize(S.B.ev_parsed));
  b->phase_ms[0] = ms_since(q0);
  b->ptimer.read(b->ktiming, b->last_parse_ms);
  const MobiDevResult *res = S.B.results();
  for (int c = 0; c < n; c++) {
    if (S.is_host[c]) continue;
    for (int k = 0, ke = S.H.live_end(c); k < ke; k++)
      if (res[(size_t)k * n + c].rc != MOBI_OK) { host_from[c] = k; fb.push_back(c); break; }
  }
  if (!fb.empty()) { // hand-overs: the state the first unfinished frame started from (mobi_gop_chain left the true one in its start slot) and the tail before it
    const size_t base = host_clips.size();
    if (b->gop_frames.size() < (base + fb.size()) * K) b->gop_frames.resize((base + fb.size()) * K);
    std::vector<DpSeed> seeds;
    for (size_t j = 0; j < fb.size(); j++) {
      const int c = fb[j], k = host_from[c];
      const size_t v = (size_t)k * n + c;
      hslot[c] = (int)(base + j);
      seeds.push_back({(const MobiDevState *)S.d_sin.p + v, k == 0 ? b->d_ptail[S.ring_in] + c : (const MobiDevTail *)S.d_tails.p + (v - n), b->parser_at(S.serial, c)});
    }
    if (int e = dp_seed_parsers(b, seeds, S.h_seed, b->stream_p)) return e;
    gop_host_parse(b, S, fb);
    for (int c : fb)
      if (!b->stale(S.serial, c)) b->route_to_host(c); // (stale: reset since, the clip's routing is a new decoder's)
    b->fallbacks += fb.size();
  }
  return MOBI_OK;
}
// 3. the host parser's command lists over the rows the parse kernels left, frame by frame
static int gop_overrides(mobi_batch *b, mobi_batch::GopSlot &S, const std::vector<int> &host_clips, const std::vector<int> &fb) {
  const int n = b->n, K = S.H.K;
  const size_t nv = (size_t)n * K;
  auto &host_from = S.H.host_from, &hslot = S.hslot, &hrc = S.H.rc, &all_host = S.all_host;
  HIP_TRY(hipStreamWaitEvent(b->stream, S.B.ev_parsed, 0));
  all_host = host_clips;
  all_host.insert(all_host.end(), fb.begin(), fb.end());
  std::sort(all_host.begin(), all_host.end());
  for (int k = 0; k < K && !all_host.empty(); k++) {
    std::vector<int> cl;
    std::vector<const ParsedFrame *> fr;
    std::vector<int> rcs;
    for (int c : all_host)
      if (host_from[c] <= k && k < S.H.live_end(c)) { // (an idle frame's rows are mobi_idle_rows')
        const size_t v = (size_t)k * n + c;
        cl.push_back(c);
        rcs.push_back(hrc[v]);
        fr.push_back(hrc[v] == MOBI_OK ? &b->gop_frames[(size_t)hslot[c] * K + k] : nullptr);
      }
    if (int e = dp_override(b, cl, nullptr, S.h_over[k], S.B, k, b->stream, fr.data(), rcs.data())) return e;
  }
  HIP_TRY(hipMemsetAsync(S.d_fault.p, 0, nv * sizeof(int), b->stream));
  return MOBI_OK;
}
// 3b. the intra macroblocks of every frame of the group as launch items in wavefront order, built on the device behind the overrides (mobi_gop.h)
// (the wavefront order holds where the halo's linear addresses do not wrap: in a picture as wide as its stride -- 256, 512, 1024 -- the
// first macroblock of a row reads the LAST one of the row above, MD.cs:212-217 with Stride == Width; those keep the raster-order launch)
static int gop_sort(mobi_batch *b, mobi_batch::GopSlot &S) {
  const int n = b->n, K = S.H.K, n_mbs = b->g.mbw * b->g.mbh;
  auto &host_from = S.H.host_from, &hslot = S.hslot, &hrc = S.H.rc;
  const MobiDevResult *res = S.B.results();
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
        if (k >= S.H.live_end(c)) continue; // (the sort counts nothing for an idle slot)
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
      A.desc = (const MbDesc *)S.B.desc.p;
      A.items = (const uint32_t *)S.B.items.p;
      A.res = (const MobiDevResult *)S.B.res.p;
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
// 4. the reconstruction steps k0 .. k1 - 1 of this part, from consecutive command lists: any number of them.  (It is the caller of
// mobi_batch_gop_finish that is limited to six, the pictures the ring holds for it to read; mobi_batch_gop_finish_all runs all the rest.)
static int gop_recon_part(mobi_batch *b, mobi_batch::GopSlot &S, int k0, int k1) {
  const int n = b->n, K = S.H.K;
  auto &host_from = S.H.host_from, &hslot = S.hslot, &hrc = S.H.rc;
  const MobiDevResult *res = S.B.results();
  for (int k = k0; k < k1; k++) {
    const size_t kn = (size_t)k * n;
    uint32_t Kint = 0;
    for (int c = 0; c < n; c++) {
      const size_t v = kn + c;
      if (k >= S.H.live_end(c)) continue;
      if (k >= host_from[c]) { if (hrc[v] == MOBI_OK) Kint = std::max(Kint, b->gop_frames[(size_t)hslot[c] * K + k].hdr.n_intra); }
      else Kint = std::max(Kint, res[v].n_intra);
    }
    if (int e = b->begin_step()) return e;
    const DpSet::Rows rows = S.B.rows(k);
    MobiReconArgs a = b->args(rows.desc, rows.pay);
    a.pay_clip_words = (uint32_t)S.B.cap_words;
    a.fault = (int *)S.d_fault.p + kn;
    mobi_batch::EvPair ep{nullptr, nullptr, 0};
    if (b->ktiming) { ep.a = b->get_event(); ep.b = b->get_event(); (void)hipEventRecord(ep.a, b->stream); }
    if (mobi_launch_inter(&a, b->stream) != 0) return MOBI_E_DEVICE;
    if (b->ktiming) { (void)hipEventRecord(ep.b, b->stream); b->evs.push_back(ep); }
    if (int e = b->motion_step(a)) return e;
    if (S.sorted) {
      if (S.sorted_items[k] && mobi_launch_intra(&a, (const uint32_t *)S.d_sorted.p + S.sorted_off[k] * 4, (int)S.sorted_items[k], b->stream) != 0) return MOBI_E_DEVICE;
    } else if (Kint && mobi_launch_intra_cl(&a, (const uint32_t *)rows.items, &rows.res->n_intra, (int)(sizeof(MobiDevResult) / 4), (int)Kint, 0, b->stream) != 0)
      return MOBI_E_DEVICE;
    if (int e = b->sink_step(a)) return e;
  }
  b->pay_clip_words = (uint32_t)S.B.cap_words;
  HIP_TRY(hipMemcpyAsync(S.B.h_fault.p + (size_t)k0 * n * sizeof(int), S.d_fault.p + (size_t)k0 * n * sizeof(int), (size_t)(k1 - k0) * n * sizeof(int), hipMemcpyDeviceToHost, b->stream));
  return MOBI_OK;
}
// 5. clips that go back to the device parsers (dp_return's rule, counted in frames): their state into the entry the next parse reads
static int gop_return_clips(mobi_batch *b, mobi_batch::GopSlot &S) {
  const int n = b->n;
  auto &host_from = S.H.host_from, &all_host = S.all_host; auto &hready = S.hready;
  std::vector<int> back;
  for (int c : all_host) {
    if (b->host_share[c] || b->stale(S.serial, c)) continue;
    int run = b->clean_run[c]; // consecutive frames the device parsers would have finished too
    for (int k = host_from[c], ke = S.H.live_end(c); k < ke; k++) run = hready[(size_t)k * n + c] ? run + 1 : 0;
    b->clean_run[c] = (uint16_t)std::min(60000, run);
    if (run >= b->clean_need[c]) back.push_back(c);
  }
  return dp_return_list(b, back, b->ps_cur, S.B, b->stream_p);
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
// the oldest group's next part (six frames at most), or with `all` every frame it still has, as ONE part: one wait
static int gop_finish_part(mobi_batch *b, int32_t *offsets_out, int *rc, bool all) {
  if (!b || !rc) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  if (b->poisoned) return MOBI_E_DEVICE;
  if (b->gop_count == 0) return MOBI_E_ARG;
  mobi_batch::GopSlot &S = b->gslot[b->gop_head & 1];
  const int K = S.H.K;
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
  const int k0 = S.done, k1 = all ? K : std::min(K, k0 + 6);
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
  b->lockstep = S.H.lockstep;
  dp_report(b, S.H, S.B, k0, k1, offsets_out, rc);
  S.done = k1;
  if (last) {
    b->gop_head ^= 1;
    b->gop_count--;
    S.parse_enqueued = false;
    S.resolved = S.returned = false;
  }
  return MOBI_OK;
}
int mobi_batch_gop_finish(mobi_batch *b, int32_t *offsets_out, int *rc) { return gop_finish_part(b, offsets_out, rc, false); }
int mobi_batch_gop_finish_all(mobi_batch *b, int32_t *offsets_out, int *rc) { return gop_finish_part(b, offsets_out, rc, true); }
// frames of the OLDEST group begun that mobi_batch_gop_finish has not reported yet (0: no group is begun); the next finish reports min(6, that)
int mobi_batch_gop_frames_pending(const mobi_batch *b) {
  if (!b || b->gop_count == 0) return 0;
  const mobi_batch::GopSlot &S = b->gslot[b->gop_head & 1];
  return S.H.K - (S.resolved ? S.done : 0);
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
