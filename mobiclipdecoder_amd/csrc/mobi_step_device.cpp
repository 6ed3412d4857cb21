// mobi_step_device.cpp -- device-parsed frame steps: behind mobi_batch_decode, mobi_batch_submit / mobi_batch_wait.  A step is a group of one
// frame as far as the hand-over goes, and that part is here once, for the groups (mobi_step_groups.cpp) too: gather and upload of the staged
// image (dp_stage; its layout: mobi_handover.h), the payload bound, the parse arguments and the idle rows (dp_cap_words, dp_parse_args,
// dp_idle_rows), the host parser's seeds, command lists and way back (dp_seed_parsers, dp_override, dp_return_list), the report (dp_report).
#include "mobi_batch.h"

// DecodeFrame() of every clip with the bitstream parse on the GPU: upload Data[Offset..) of every clip, one parse launch
// (one wave per clip) that leaves descriptors, payload and intra lists in HBM, then the usual reconstruction launches.
//
// r05: WHICH side parses never shows in the result.  The device parsers finish the frames that decode without incident.  A frame they
// cannot finish -- every condition under which the reference throws, every walk through Internal[] (MD.cs:3424-3429), every value the
// command list has to escape (mobi_parse.cpp) -- is parsed again by the host parser INSIDE THE SAME CALL, from the decoder state the clip
// had when the frame started (the device keeps a ring of three states per clip: mobi_dparse.h, mobi_state.h), and its command list is
// written over the blank one the parse kernel left.  rc, Offset, Quantizer and the planes are then the host parser's, i.e. the same as
// at any other batch size; the clip stays with the host parser from there on (`on_host`), parsed beside the GPU's clips like the
// host-parsed share of the hybrid mode, which is the same mechanism with the last clips of the batch marked from the start.
//
// first use of the device-side parser: zeroed decoder state (a new MobiclipDecoder), result array, tables -- all of it or none of it
int dp_init(mobi_batch *b) {
  const int n = b->n;
  if (b->d_pstate[0]) return MOBI_OK;
  auto init = [&]() -> int {
    if (int e = b->dp.reserve_results(n)) return e;
    HIP_TRY(hipMemset(b->dp.res.p, 0, sizeof(MobiDevResult) * n));
    std::vector<uint8_t> blob(MOBI_DT_BYTES);
    mobi_dparse_build_tables(b->version, blob.data());
    if (int e = b->d_ptables.alloc(MOBI_DT_BYTES)) return e;
    HIP_TRY(hipMemcpy(b->d_ptables, blob.data(), MOBI_DT_BYTES, hipMemcpyHostToDevice));
    if (int e = b->d_pstate_ls.alloc(n)) return e;
    for (int k = 0; k < 3; k++) {
      if (int e = b->d_ptail[k].alloc(n)) return e;
      HIP_TRY(hipMemset(b->d_ptail[k], 0, sizeof(MobiDevTail) * n));
    }
    for (int k = 2; k >= 0; k--) { // entry 0 last: its presence means "initialised"
      if (int e = b->d_pstate[k].alloc(n)) return e;
      HIP_TRY(hipMemset(b->d_pstate[k], 0, sizeof(MobiDevState) * n));
    }
    return MOBI_OK;
  };
  if (int e = init()) {
    b->dp.res.release(); b->d_ptables.free(); b->d_pstate_ls.free();
    for (int k = 0; k < 3; k++) { b->d_pstate[k].free(); b->d_ptail[k].free(); }
    return e;
  }
  b->dev_quant.assign(n, 0);
  b->dev_yuvfmt.assign(n, 0);
  if ((int)b->on_host.size() != n) b->on_host.assign(n, 0);
  b->host_share.assign(n, 0);
  b->clean_run.assign(n, 0);
  b->clean_need.assign(n, 4);
  return MOBI_OK;
}
// Which device parser is in front of this step (parse mode by default, r05; tools/exp_lsab.sh, tools/exp_dparse.py, 640x480, ms per step,
// mobi_parse_frames against the lock-step parser at its best number of clips per wave):
//   P-frames: 2048 clips 8.8 / 9.2, 4096: 11.2 / 13.7, 8192: 21.2 / 18.5, 16384: 42 / 23.5, 24576: 63 / 26.2
//   I-frames: 1024 clips 23.4 / 11.7, 2048: 30.0 / 11.3, 4096: 30.0 / 16.5, 8192: 54.9 / 23.6
// -- one wave per clip wins while every clip has a wave slot of its own and the frames are P-frames; an I-frame's macroblocks are all of one
// kind, which is what lanes in lock step like.
bool ls_decide(const mobi_batch *b, const StageImage &st) {
  if (b->ls_policy != 2) return b->ls_policy == 1;
  const bool iframe_step = 2 * st.n_iframes > st.n_dev;
  return st.n_dev >= 5120 || (iframe_step && st.n_dev >= 768);
}
// Gather and upload.  With `up`, one thread of the pool sits in the copy calls, which return when the bus is done (8 ms for the 370 MB of a
// step of 24576 clips), while the others gather the next round -- r04: gathering and sending were 12 of the 45 ms of such a step, one after
// the other.  `run` frames per task: one per frame has the pool's threads queue at its counter (122 880 frames of 256x192: 8 ms).
int dp_stage(mobi_batch *b, const StageImage &img, DpSet &B, const uint8_t *const *data, const int32_t *offsets, const uint8_t *idle_from, const int32_t *resets, int chunks, int run,
             hipStream_t up, bool header_too, std::chrono::steady_clock::time_point t0) {
  const int nv = (int)img.lanes();
  uint8_t *hs = B.h_stage.p;
  img.write_header(hs, resets, idle_from);
  if (nv < 2048 || !up) chunks = 1;
  std::atomic<int> up_err{0};
  auto start_of = [&](int v) { return v < nv ? img.hdr_bytes + (size_t)img.boff[v] : img.bytes; }; // (behind the last lane: the lists)
  for (int k = 0; k <= chunks; k++) {
    const int c0 = k < chunks ? (int)((long)nv * k / chunks) : nv, c1 = k < chunks ? (int)((long)nv * (k + 1) / chunks) : nv;
    const int u0 = k >= 1 ? (int)((long)nv * (k - 1) / chunks) : 0, u1 = k >= 1 ? (int)((long)nv * k / chunks) : 0; // gathered in the round before
    const int n_up = up && u1 > u0 ? 1 : 0;
    if (n_up + (c1 - c0) == 0) continue;
    b->pool->run(n_up + (c1 - c0 + run - 1) / run, [&](int j) {
      if (j < n_up) {
        const size_t a = u0 == 0 && header_too ? 0 : start_of(u0), e = start_of(u1);
        if (e > a && (hipSetDevice(b->device) != hipSuccess || hipMemcpyAsync(B.bits.p + a, hs + a, e - a, hipMemcpyHostToDevice, up) != hipSuccess)) up_err = 1;
        return;
      }
      for (int v = c0 + (j - n_up) * run, e = std::min(c1, v + run); v < e; v++) img.gather(hs, (size_t)v, data, offsets);
    });
  }
  b->last_stage_ms = ms_since(t0);
  return up_err ? MOBI_E_DEVICE : MOBI_OK;
}
// A lane's payload can never exceed 448 words per macroblock, nor 64 per macroblock + one level per THREE bits read (a level word stands for
// a token with a level, and the shortest of those -- either table, either version -- has two bits and a sign: mobi_dparse_build_tables;
// tests/test_parse_fallback.py checks the tables for it).  The longest frame of a hand-over varies: the bound follows it upwards in steps
// of a quarter, so that the payload arena -- gigabytes for thousands of clips -- is not freed and allocated again every few frames.
size_t dp_cap_words(mobi_batch *b, size_t max_len) {
  const size_t n_mbs = (size_t)b->g.mbw * b->g.mbh;
  if (max_len > b->dp_len_hint) b->dp_len_hint = max_len + max_len / 4;
  return std::min<size_t>(n_mbs * 448 + MOBI_WIDE_PARAMS, n_mbs * 64 + (8 * b->dp_len_hint + 2) / 3) + 448 + 64;
}
// what every parse launch is told: the image, the tables the set holds, the picture.  The caller adds the decoder state and the parser in front
void dp_parse_args(const mobi_batch *b, const StageImage &img, const DpSet &B, MobiDevParseArgs &pa) {
  memset(&pa, 0, sizeof(pa));
  pa.bits = B.bits.p + img.hdr_bytes;
  pa.bit_off = (const uint64_t *)B.bits.p;
  pa.bit_len = (const uint32_t *)(B.bits.p + img.lanes() * 8);
  pa.tables = b->d_ptables;
  pa.scale = b->d_scale;
  pa.pay_local = 1;
  pa.desc = (MbDesc *)B.desc.p;
  pa.payload = (uint32_t *)B.pay.p;
  pa.items = (uint32_t *)B.items.p;
  pa.res = (MobiDevResult *)B.res.p;
  pa.pay_cap = (uint32_t)B.cap_words;
  pa.n_clips = (int)img.lanes(); pa.version = b->version;
  pa.width = b->g.width; pa.height = b->g.height; pa.stride = b->g.stride; pa.lg = b->g.lg; pa.mbw = b->g.mbw; pa.mbh = b->g.mbh;
}
// the idle slots' empty rows, in front of the parse kernels (mobi_idle.hip).  carry_state (steps): their clips' state goes into the entry the
// next parse reads; groups: their clips' chains end at idle_from (mobi_gop.h)
int dp_idle_rows(mobi_batch *b, const StageImage &img, const DpSet &B, const MobiDevParseArgs &pa, bool carry_state, hipStream_t s) {
  if (!img.n_idle) return MOBI_OK;
  MobiIdleArgs ia;
  memset(&ia, 0, sizeof(ia));
  ia.clips = (const int32_t *)(B.bits.p + img.idle_off); ia.count = img.n_idle;
  if (img.idle_from_off) ia.idle_from = B.bits.p + img.idle_from_off;
  ia.n = img.n; ia.K = img.K; ia.n_mbs = b->g.mbw * b->g.mbh;
  ia.desc = pa.desc; ia.res = pa.res;
  if (carry_state) { ia.state_in = pa.state_in; ia.state_out = pa.state_out; ia.tail_in = pa.tail_in; ia.tail_out = pa.tail_out; }
  if (mobi_launch_idle_rows(&ia, s) != 0) return MOBI_E_DEVICE;
  b->idle_launches++;
  return MOBI_OK;
}
// a step's staged image: planned, room made for it (dev_headroom: asynchronous steps leave room in HBM too), gathered -- and with `up` on its way
static int dp_stage_step(mobi_batch *b, StageImage &img, DpSet &B, const uint8_t *const *data, const size_t *len, const int32_t *offsets, const std::vector<uint8_t> &idle,
                         bool dev_state, bool dev_headroom, hipStream_t up) {
  const auto t0 = std::chrono::steady_clock::now();
  const uint8_t *idle_from = idle.empty() ? nullptr : idle.data();
  const std::vector<int32_t> none, &resets = dev_state ? b->reset_list : none; // (before dp_init there is nothing on the device to reset)
  img.plan(b->n, 1, b->g.mbw * b->g.mbh, data, len, offsets, b->on_host.data(), idle_from, resets.size(), false);
  if (int e = B.h_stage.grow(img.bytes)) return e;
  if (int e = dev_headroom ? B.bits.grow(img.bytes) : B.bits.reserve(img.bytes)) return e;
  return dp_stage(b, img, B, data, offsets, idle_from, resets.data(), 4, 32, up, true, t0);
}
// output tables + the parse launch of a step on stream s.  *state_in: which entry of the state ring the step reads (the state its frames start from).
static int dp_parse(mobi_batch *b, const StageImage &img, DpSet &B, hipStream_t s, bool async, int *state_in) {
  b->last_pay_cap = dp_cap_words(b, img.max_len);
  b->pay_clip_words = (uint32_t)b->last_pay_cap;
  if (int e = B.reserve_tables(b->n, b->n, b->g.mbw * b->g.mbh, b->pay_clip_words)) return e;
  MobiDevParseArgs pa;
  dp_parse_args(b, img, B, pa);
  const int in = b->ps_cur, out = (b->ps_cur + 1) % 3;
  pa.state_in = b->d_pstate[in]; pa.state_out = b->d_pstate[out];
  pa.tail_in = b->d_ptail[in]; pa.tail_out = b->d_ptail[out];
  pa.state_ls = b->d_pstate_ls;
  pa.lockstep = b->lockstep ? (async ? 2 : 1) : 0; // (2: an asynchronous step; the launch has had one shape for both since r05: mobi_launch_parse_ls)
  if (int e = dp_idle_rows(b, img, B, pa, true, s)) return e;
  b->ptimer.start(b->ktiming, s);
  if (mobi_launch_parse(&pa, s) != 0) return MOBI_E_DEVICE;
  b->ptimer.stop(b->ktiming, s);
  b->ps_cur = out;
  *state_in = in;
  return MOBI_OK;
}

// The command lists of host-parsed clips of a device-parsed step (`clips`, ascending; b->cur[c] holds clip c's frame when rc[c] is MOBI_OK):
// staged in pinned memory and copied into the clips' own rows of what the parse kernels leave -- descriptor rows, payload parts, item
// rows, result records of frame `frame` of the set B -- on stream s.  Runs of neighbouring clips (the hybrid mode's share) go as one copy per table.
// frames != nullptr: frames[j] is clips[j]'s parsed frame (nullptr: it failed) and rcs[j] its rc -- both by POSITION in `clips` (the
// frame-parallel path: a clip has K frames); else b->cur[c] and rc[c] by clip.
int dp_override(mobi_batch *b, const std::vector<int> &clips, const int *rc, PinnedBuf &stage, const DpSet &B, int frame, hipStream_t s,
                const ParsedFrame *const *frames, const int *rcs) {
  const int k = (int)clips.size(), n_mbs = b->g.mbw * b->g.mbh;
  if (k == 0) return MOBI_OK;
  auto frame_of = [&](int j) -> const ParsedFrame * { return frames ? frames[j] : (rc[clips[j]] == MOBI_OK ? &b->cur[clips[j]] : nullptr); };
  auto rc_of = [&](int j) { return frames ? rcs[j] : rc[clips[j]]; };
  size_t pitch_w = 0; // payload words per clip in the staging area
  for (int j = 0; j < k; j++)
    if (const ParsedFrame *f = frame_of(j)) pitch_w = std::max(pitch_w, f->payload.size());
  pitch_w = align_up(pitch_w + 4, 4);
  const DpSet::Rows d = B.rows(frame);
  const size_t cap_b = B.cap_words * 4;
  if (pitch_w > B.cap_words) return MOBI_E_DEVICE; // cannot happen: cap_words bounds any clip's payload
  const size_t desc_b = (size_t)n_mbs * sizeof(MbDesc), item_b = (size_t)n_mbs * 4, res_b = sizeof(MobiDevResult), pay_b = pitch_w * 4;
  const size_t o_item = align_up((size_t)k * desc_b, 16), o_res = o_item + align_up((size_t)k * item_b, 16), o_pay = o_res + align_up((size_t)k * res_b, 16);
  if (int e = stage.reserve(o_pay + (size_t)k * pay_b)) return e;
  uint8_t *h = stage.p;
  const int groups = std::min(k, 32);
  b->pool->run(groups, [&](int g) {
    for (int j = (int)((long)k * g / groups), e = (int)((long)k * (g + 1) / groups); j < e; j++) {
      const ParsedFrame *f = frame_of(j);
      MbDesc *dd = (MbDesc *)(h + (size_t)j * desc_b);
      uint32_t *it = (uint32_t *)(h + o_item + (size_t)j * item_b);
      MobiDevResult *rr = (MobiDevResult *)(h + o_res + (size_t)j * res_b);
      memset(rr, 0, sizeof(*rr));
      rr->rc = rc_of(j);
      if (!f) { // a failed clip: descriptors typed "intra" that no launch list references
        for (int m = 0; m < n_mbs; m++) dd[m] = MbDesc{0, MOBI_MB_INTRA, 0, 0, 0, 0, 0, 0};
        continue;
      }
      memcpy(dd, f->desc.data(), desc_b); // (payload_off counts from the clip's own part of the arena, as the parser wrote it)
      if (!f->payload.empty()) memcpy(h + o_pay + (size_t)j * pay_b, f->payload.data(), f->payload.size() * 4);
      if (!f->intra_mbs.empty()) memcpy(it, f->intra_mbs.data(), f->intra_mbs.size() * 4); // level order: a valid order for the waits
      rr->n_intra = f->hdr.n_intra;
      rr->payload_words = f->hdr.payload_words;
      rr->quant = f->hdr.quantizer;
      rr->frame_type = f->hdr.frame_type;
    }
  });
  for (int j0 = 0; j0 < k;) {
    int j1 = j0 + 1;
    while (j1 < k && clips[j1] == clips[j1 - 1] + 1) j1++;
    const size_t c0 = (size_t)clips[j0], run = (size_t)(j1 - j0);
    HIP_TRY(hipMemcpyAsync(d.desc + c0 * desc_b, h + (size_t)j0 * desc_b, run * desc_b, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d.items + c0 * item_b, h + o_item + (size_t)j0 * item_b, run * item_b, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync((uint8_t *)(d.res + c0), h + o_res + (size_t)j0 * res_b, run * res_b, hipMemcpyHostToDevice, s));
    if (run == 1) HIP_TRY(hipMemcpyAsync(d.pay + c0 * cap_b, h + o_pay + (size_t)j0 * pay_b, pay_b, hipMemcpyHostToDevice, s));
    else HIP_TRY(hipMemcpy2DAsync(d.pay + c0 * cap_b, cap_b, h + o_pay + (size_t)j0 * pay_b, pay_b, pay_b, run, hipMemcpyHostToDevice, s));
    j0 = j1;
  }
  return MOBI_OK;
}
// Decoder states the device holds into host parsers -- the state a frame STARTED from, when the host parser takes the frame over: two asynchronous
// copies per seed into pinned memory, ONE wait, the imports on the pool (r05 issued two blocking copies per clip: a step in which every clip of a
// large batch is handed over at once -- a ModsDS batch that cuts to a quantiser below 12 -- sat in tens of thousands of them)
int dp_seed_parsers(mobi_batch *b, const std::vector<DpSeed> &seeds, PinnedBuf &stage, hipStream_t s) {
  if (seeds.empty()) return MOBI_OK;
  const size_t rec = sizeof(MobiDevState) + sizeof(MobiDevTail);
  if (int e = stage.reserve(seeds.size() * rec)) return e;
  for (size_t j = 0; j < seeds.size(); j++) {
    HIP_TRY(hipMemcpyAsync(stage.p + j * rec, seeds[j].state, sizeof(MobiDevState), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(stage.p + j * rec + sizeof(MobiDevState), seeds[j].tail, sizeof(MobiDevTail), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  b->pool->run((int)seeds.size(), [&](int j) {
    seeds[j].parser->import_state(*(const MobiDevState *)(stage.p + (size_t)j * rec), *(const MobiDevTail *)(stage.p + (size_t)j * rec + sizeof(MobiDevState)));
  });
  return MOBI_OK;
}
// (a step's: the clips `cl` from entry `in` of the state ring, into `parser(c)`)
template <class F> static int dp_seed_step(mobi_batch *b, const std::vector<int> &cl, int in, PinnedBuf &stage, F parser) {
  std::vector<DpSeed> seeds;
  for (int c : cl) seeds.push_back({b->d_pstate[in] + c, b->d_ptail[in] + c, parser(c)});
  return dp_seed_parsers(b, seeds, stage, b->stream);
}

// A clip the host parser took over goes BACK to the device parsers once its frames are again the kind they finish: `clean_need`
// consecutive frames without a walk, a token without a level or a value beyond the device parsers' fields (MobiStreamParser::device_ready),
// doubled with every hand-over (4, 8, ... 256: a clip whose every frame needs the host parser -- a ModsDS stream below quantiser 12 -- costs
// a wasted device parse every few hundred frames, a glitch in an otherwise clean stream a handful of host-parsed frames).  The parser's state
// goes into entry `entry` of the state ring -- the one the next step's parse reads -- on stream s, through B.h_ret.
static int dp_return(mobi_batch *b, const std::vector<int> &host_clips, const int *rc, int entry, DpSet &B, hipStream_t s) {
  std::vector<int> back;
  for (int c : host_clips) {
    if (b->host_share[c]) continue;
    if (rc[c] == MOBI_OK && b->parsers[c]->device_ready()) b->clean_run[c]++;
    else b->clean_run[c] = 0;
    if (b->clean_run[c] >= b->clean_need[c]) back.push_back(c);
  }
  return dp_return_list(b, back, entry, B, s);
}
int dp_return_list(mobi_batch *b, const std::vector<int> &back, int entry, DpSet &B, hipStream_t s) {
  if (back.empty()) return MOBI_OK;
  PinnedBuf &stage = B.h_ret;
  const size_t rec = sizeof(MobiDevState) + sizeof(MobiDevTail);
  if (int e = stage.reserve(back.size() * rec)) return e;
  for (size_t k = 0; k < back.size(); k++) {
    const int c = back[k];
    MobiDevState *st = (MobiDevState *)(stage.p + k * rec);
    MobiDevTail *tail = (MobiDevTail *)(stage.p + k * rec + sizeof(MobiDevState));
    b->parsers[c]->export_state(*st, *tail);
    HIP_TRY(hipMemcpyAsync(b->d_pstate[entry] + c, st, sizeof(*st), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b->d_ptail[entry] + c, tail, sizeof(*tail), hipMemcpyHostToDevice, s));
    b->on_host[c] = 0;
    b->clean_run[c] = 0;
    b->returns++;
  }
  return MOBI_OK;
}

int decode_device_parse(mobi_batch *b, const uint8_t *const *data, const size_t *len, int32_t *offsets, int *rc) {
  const int n = b->n;
  if (!b->version_known()) {
    for (int i = 0; i < n; i++) rc[i] = MOBI_E_VERSION;
    return MOBI_OK; // DecodeFrame() returns before touching the ring (MD.cs:56-61)
  }
  if (b->g.mbw > 64 || b->async_count || b->gop_count) return MOBI_E_ARG; // (asynchronous steps / groups in flight: wait for them first)
  std::vector<uint8_t> idle; // [clip] 0: an idle slot (mobi_batch_set_idle); empty: none
  if (int e = idle_check(b, 1, idle)) return e;
  auto is_idle = [&](int i) { return !idle.empty() && idle[i] == 0; };
  const bool dev_state = b->d_pstate[0] != nullptr; // (before dp_init there is nothing on the device to reset)
  if (int e = dp_init(b)) return e;
  b->mark_hybrid_share();
  const uint64_t serial = b->handover + 1;
  reset_apply_host(b, serial);
  std::vector<int> host_clips;
  for (int i = 0; i < n; i++)
    if (b->on_host[i] && !is_idle(i)) host_clips.push_back(i);
  DpSet &B = b->dp;
  StageImage st;
  const auto q0 = std::chrono::steady_clock::now();
  if (int e = dp_stage_step(b, st, B, data, len, offsets, idle, dev_state, false, b->stream)) return e; // gathered and on their way
  b->phase_ms[0] = ms_since(q0);
  b->lockstep = ls_decide(b, st);
  if (st.n_reset && mobi_launch_reset_state((const int32_t *)(B.bits.p + st.reset_off), st.n_reset, n, b->d_pstate[b->ps_cur], b->d_ptail[b->ps_cur], b->stream) != 0)
    return MOBI_E_DEVICE;
  int state_in = 0;
  if (int e = dp_parse(b, st, B, b->stream, false, &state_in)) return e;
  idle_commit(b, 1, idle);
  reset_commit(b, serial);
  b->phase_ms[1] = ms_since(q0);
  const MobiDevResult *res = B.results(), *d_res = (const MobiDevResult *)B.res.p;
  HIP_TRY(hipMemcpyAsync(B.h_res.p, d_res, sizeof(MobiDevResult) * n, hipMemcpyDeviceToHost, b->stream));
  auto host_parse = [&](const std::vector<int> &cl) {
    b->pool->run((int)cl.size(), [&](int j) { const int i = cl[j]; rc[i] = parse_host(b->parsers[i].get(), data[i], len[i], &offsets[i], b->cur[i]); });
  };
  if (!host_clips.empty()) { // while the GPU parses its clips, the host pool parses its own and sends their command lists up beside it
    if (int e = ensure_stream(b->stream2)) return e;
    if (int e = ensure_event(B.ev_up)) return e;
    host_parse(host_clips);
    if (int e = dp_override(b, host_clips, rc, B.h_over, B, 0, b->stream2)) return e; // (no kernel touches these clips' rows: MOBI_DP_SKIP)
    HIP_TRY(hipEventRecord(B.ev_up, b->stream2));
    HIP_TRY(hipStreamWaitEvent(b->stream, B.ev_up, 0));
    HIP_TRY(hipStreamSynchronize(b->stream2));
  }
  HIP_TRY(hipStreamSynchronize(b->stream)); // the launch sizes below depend on what the parse found
  b->phase_ms[2] = ms_since(q0);
  b->ptimer.read(b->ktiming, b->last_parse_ms);
  // frames the device parsers could not finish: the host parser takes them over from the state they started with
  std::vector<int> fb;
  for (int i = 0; i < n; i++)
    if (!b->on_host[i] && !is_idle(i) && res[i].rc != MOBI_OK) fb.push_back(i);
  if (!fb.empty()) {
    if (int e = dp_seed_step(b, fb, state_in, B.h_ret, [&](int c) { return b->parsers[c].get(); })) return e; // (the stream is idle: it was waited for above)
    host_parse(fb);
    for (int c : fb) {
      b->route_to_host(c);
      host_clips.push_back(c);
    }
    b->fallbacks += fb.size();
    if (int e = dp_override(b, fb, rc, B.h_over, B, 0, b->stream)) return e; // (behind the parse kernels, which blanked these clips' rows)
  }
  // (dp_report's loop over the caller's own arrays: rc[] and offsets[] already hold the host parser's results, where dp_report wants a copy of them)
  uint32_t K = 0;
  b->ls_finished = b->lockstep ? 0 : -1;
  for (int i = 0; i < n; i++) {
    if (is_idle(i)) { rc[i] = MOBI_IDLE; continue; } // (Offset as handed in; Quantizer / YuvFormat stay the last live frame's)
    if (b->on_host[i]) {
      b->dev_quant[i] = b->parsers[i]->quantizer();
      b->dev_yuvfmt[i] = b->parsers[i]->yuv_format();
      if (rc[i] == MOBI_OK) K = std::max(K, b->cur[i].hdr.n_intra);
      continue;
    }
    if (b->lockstep && res[i].pad == MOBI_LS_MAGIC) b->ls_finished++;
    rc[i] = res[i].rc;
    offsets[i] += res[i].consumed;
    b->dev_quant[i] = res[i].quant;
    b->dev_yuvfmt[i] = res[i].yuvfmt;
    K = std::max(K, res[i].n_intra);
  }
  // 3. reconstruction straight from what the parse left in HBM
  FailAll fail_all{rc, n, b->stream}; // rc[], Offset, the ring and the decoder state have advanced: the launches below must complete
  if (int e = b->begin_step()) return e;
  MobiReconArgs a = b->args(B.desc.p, B.pay.p);
  a.pay_clip_words = b->pay_clip_words;
  a.done = b->d_done;
  if (mobi_launch_inter(&a, b->stream) != 0) return MOBI_E_DEVICE;
  if (int e = b->motion_step(a)) return e;
  if (K && mobi_launch_intra_cl(&a, (const uint32_t *)B.items.p, &d_res[0].n_intra, (int)(sizeof(MobiDevResult) / 4), (int)K, 0, b->stream) != 0)
    return MOBI_E_DEVICE;
  if (int e = b->sink_step(a)) return e;
  if (int e = b->read_faults(b->h_fault.data())) return e;
  if (!host_clips.empty())
    if (int e = dp_return(b, host_clips, rc, b->ps_cur, B, b->stream)) return e; // (ps_cur: what the next step's parse reads)
  b->phase_ms[3] = ms_since(q0);
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->phase_ms[4] = ms_since(q0);
  fail_all.armed = false;
  for (int i = 0; i < n; i++) rc[i] = fault_rc(rc[i], b->h_fault[i]);
  return MOBI_OK;
}

// Frames of SOME clips through the reconstruction kernels on their own, into the ring slot `ring_base` names: the repair of clips whose
// asynchronous step had been enqueued before anybody knew that their frame was not the device parser's to finish (mobi_batch_wait).
// `clips` ascending, frames[j] = clips[j]'s parsed frame (nullptr: the host parser rejected it: nothing is written).  Neighbouring clips
// form a run, and a run is one compact frame step of its own -- its descriptor table, its payload arena, its launch items, planes and
// tags offset to its first clip -- so "every clip of the batch at once" is ONE set of launches and a lone glitch a set of its own.  One
// upload, one read-back of the fault words, one wait for the lot (r05: a parse, an upload, launches and a wait PER CLIP, on the calling thread).
static int recon_clips(mobi_batch *b, const std::vector<int> &clips, const ParsedFrame *const *frames, int ring_base, int *fault_out) {
  const int n_mbs = b->g.mbw * b->g.mbh, k = (int)clips.size();
  if (k == 0) return MOBI_OK;
  struct Run { int j0, j1; size_t desc_off, pay_off, item_off; LevelPlan plan; };
  std::vector<Run> runs;
  size_t total = 0;
  for (int j0 = 0; j0 < k;) {
    int j1 = j0 + 1;
    while (j1 < k && clips[j1] == clips[j1 - 1] + 1) j1++;
    Run r;
    r.j0 = j0; r.j1 = j1;
    std::vector<const ParsedFrame *> fr(frames + j0, frames + j1);
    r.plan.build(fr, b->g.mbw);
    const size_t desc_bytes = align_up((size_t)(j1 - j0) * n_mbs * sizeof(MbDesc) + 8 * sizeof(MbDesc), kAlign), pay_bytes = align_up(step_payload_words(fr) * 4 + kPaySlack, kAlign);
    if (step_payload_words(fr) + kPaySlack / 4 >= ((uint64_t)1 << 32)) return MOBI_E_ARG;
    r.desc_off = total; r.pay_off = total + desc_bytes; r.item_off = r.pay_off + pay_bytes;
    total = r.item_off + align_up(r.plan.items.size() * 4 + 16, kAlign);
    runs.push_back(std::move(r));
    j0 = j1;
  }
  if (int e = b->h_fix.reserve(total)) return e;
  if (int e = b->d_fix.reserve(total)) return e;
  b->pool->run((int)runs.size(), [&](int i) {
    const Run &r = runs[i];
    std::vector<const ParsedFrame *> fr(frames + r.j0, frames + r.j1);
    memset(b->h_fix.p + r.desc_off, 0, r.item_off - r.desc_off);
    step_write(fr, n_mbs, (MbDesc *)(b->h_fix.p + r.desc_off), (uint32_t *)(b->h_fix.p + r.pay_off));
    if (!r.plan.items.empty()) memcpy(b->h_fix.p + r.item_off, r.plan.items.data(), r.plan.items.size() * 4);
  });
  HIP_TRY(hipMemcpyAsync(b->d_fix.p, b->h_fix.p, total, hipMemcpyHostToDevice, b->stream));
  b->next_tag(); // (one tag for all runs: they touch different clips' tags)
  for (const Run &r : runs) {
    const int c0 = clips[r.j0], m = r.j1 - r.j0;
    MobiReconArgs a = b->args(b->d_fix.p + r.desc_off, b->d_fix.p + r.pay_off);
    a.planes += (size_t)c0 * b->clip_bytes;
    a.n_clips = m;
    a.fault = b->d_fault + c0;
    a.done = b->d_done + (size_t)c0 * n_mbs;
    a.ring_base = ring_base;
    // (two launches, never the one-launch step: its give-up path -- fault bit 2, a dispatch order never seen -- has no retry here)
    if (int e = b->launch_plan(a, r.plan, (const uint32_t *)(b->d_fix.p + r.item_off), m, false)) return e;
  }
  HIP_TRY(hipMemcpyAsync(b->h_fault.data(), b->d_fault, sizeof(int) * b->n, hipMemcpyDeviceToHost, b->stream));
  for (const Run &r : runs) HIP_TRY(hipMemsetAsync(b->d_fault + clips[r.j0], 0, sizeof(int) * (r.j1 - r.j0), b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->drain_events();
  for (int j = 0; j < k; j++) fault_out[j] = b->h_fault[clips[j]];
  return MOBI_OK;
}

// ---- asynchronous frame steps (device parse) -------------------------------------------------------------------------------
// mobi_batch_decode is DecodeFrame(): it returns when the frame is there.  A caller that already holds the next frame of every clip
// (demuxed Moflex / Mods packets: Offset does not depend on the previous frame's parse) can keep two steps in flight instead:
// submit gathers the bytes into pinned memory, uploads them on a second stream and enqueues parse + reconstruction behind the
// previous step without a host round trip in between (the intra launch covers every slot a clip could use; workgroups past a
// clip's count leave at once); wait hands out rc[] / Offset of the oldest step when its reconstruction is done.  The host gathers
// step n + 1 while the GPU parses step n, and the GPU never waits for the host between parse and reconstruction.
// A frame the device parser cannot finish shows up in wait: the clip's frame (and the next one, if a second step is in flight) is then
// parsed by the host parser and reconstructed on its own there (async_repair), and the clip is the host parser's in later submits.
int mobi_batch_submit(mobi_batch *b, const uint8_t *const *data, const size_t *len, const int32_t *offsets) {
  if (!b || !data || !len || !offsets) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  const int n = b->n, n_mbs = b->g.mbw * b->g.mbh;
  settle_parse_mode(b, b->frames_started == 0 && b->async_seq == 0, 0, true); // an asynchronous batch parses on the GPU from its first frame
  if (b->poisoned) return MOBI_E_DEVICE;
  if (b->parse_mode == 0) return MOBI_E_ARG; // the decoder state of this batch lives in the host parsers
  if (!b->version_known()) return MOBI_E_VERSION;
  if (b->g.mbw > 64 || b->async_count >= 2 || b->gop_count) return MOBI_E_ARG;
  std::vector<uint8_t> idle; // [clip] 0: an idle slot (mobi_batch_set_idle); empty: none
  if (int e = idle_check(b, 1, idle)) return e;
  const bool dev_state = b->d_pstate[0] != nullptr;
  if (int e = dp_init(b)) return e;
  b->mark_hybrid_share();
  const uint64_t serial = b->handover + 1;
  reset_apply_host(b, serial); // (before the staging: the routing decides which clips the device parses)
  mobi_batch::AsyncSlot &S = b->aslot[(b->async_head + b->async_count) & 1];
  DpSet &B = S.B;
  HostShare &H = S.H;
  StageImage &st = S.img;
  for (Event *ev : {&B.ev_up, &S.ev_done, &B.ev_parsed})
    if (int e = ensure_event(*ev)) return e;
  if (int e = ensure_stream(b->stream2)) return e;
  if (int e = ensure_stream(b->stream_p)) return e;
  if (int e = dp_stage_step(b, st, B, data, len, offsets, idle, dev_state, true, nullptr)) return e; // (this slot's previous step was waited for: its upload is done)
  if (int e = B.reserve_results(n)) return e;
  if (int e = B.h_fault.reserve(sizeof(int) * n)) return e;
  S.serial = serial;
  b->lockstep = H.lockstep = ls_decide(b, st);
  H.K = 1;
  H.offs.assign(offsets, offsets + n);
  H.idle_from = idle;
  H.clear(n);
  // the host parser's clips: parsed now (the caller's bytes are only good during this call), their command lists staged for the copy below
  std::vector<int> host_clips;
  for (int i = 0; i < n; i++)
    if (b->on_host[i] && !S.is_idle(i)) host_clips.push_back(i);
  if (!host_clips.empty()) {
    for (int i : host_clips) { H.host_from[i] = 0; H.off[i] = offsets[i]; }
    b->pool->run((int)host_clips.size(), [&](int j) {
      const int i = host_clips[j];
      H.rc[i] = parse_host(b->parsers[i].get(), data[i], len[i], &H.off[i], b->cur[i]);
      H.quant[i] = b->parsers[i]->quantizer();
      H.yuv[i] = b->parsers[i]->yuv_format();
    });
  }
  // Everything that can fail without touching the device is behind us.  From the first enqueue on, a failure leaves work in flight
  // that reads this slot's pinned memory and (later) a ring that has turned without a step to wait for: the batch is drained and
  // POISONED -- every later call reports MOBI_E_DEVICE -- rather than left in a state where the next submit reuses the slot.
  Poison poison{b};
  HIP_TRY(hipMemcpyAsync(B.bits.p, B.h_stage.p, st.bytes, hipMemcpyHostToDevice, b->stream2)); // beside whatever the step before is doing
  HIP_TRY(hipEventRecord(B.ev_up, b->stream2));
  // Three streams: the upload (stream2), the parse (stream_p: after the upload; the decoder state goes from parse to parse in its order)
  // and the reconstruction (stream: after this step's parse; the ring goes from step to step in its order).  The parse of this step
  // runs under the reconstruction of the one before -- the lock-step parser leaves most of the chip idle -- because what it writes
  // (descriptors, payload, intra lists, results) belongs to the slot, whose previous step has been waited for.
  // (Only the lock-step parser gets the stream of its own: the one-wave-per-clip parser fills every wave slot of the chip with 122-register
  // waves, and a reconstruction launched beside it waits for them to leave anyway -- 20.5 instead of 13.2 ms per step of 4096 clips.)
  hipStream_t ps = b->lockstep ? b->stream_p : b->stream;
  HIP_TRY(hipStreamWaitEvent(ps, B.ev_up, 0));
  { // the parser in front is chosen step by step (ls_decide), and with it the stream: the state this parse reads is the one the step before wrote
    mobi_batch::AsyncSlot &prev = b->aslot[(b->async_head + b->async_count + 1) & 1];
    if (b->async_seq > 0 && prev.B.ev_parsed && prev.parsed_recorded) HIP_TRY(hipStreamWaitEvent(ps, prev.B.ev_parsed, 0));
  }
  const MobiDevResult *d_res = (const MobiDevResult *)B.res.p;
  // clips reset from this step on: a new decoder's state into the entry the parse reads, behind whatever the step before wrote there
  if (st.n_reset && mobi_launch_reset_state((const int32_t *)(B.bits.p + st.reset_off), st.n_reset, n, b->d_pstate[b->ps_cur], b->d_ptail[b->ps_cur], ps) != 0)
    return MOBI_E_DEVICE;
  if (int e = dp_parse(b, st, B, ps, true, &S.state_in)) return e;
  if (!host_clips.empty()) {
    if (int e = dp_override(b, host_clips, H.rc.data(), B.h_over, B, 0, ps)) return e;
    if (int e = dp_return(b, host_clips, H.rc.data(), b->ps_cur, B, ps)) return e; // (the parse kernels skip these clips: their entries are free to write)
  }
  HIP_TRY(hipMemcpyAsync(B.h_res.p, d_res, sizeof(MobiDevResult) * n, hipMemcpyDeviceToHost, ps));
  HIP_TRY(hipEventRecord(B.ev_parsed, ps));
  S.parsed_recorded = true;
  if (ps != b->stream) HIP_TRY(hipStreamWaitEvent(b->stream, B.ev_parsed, 0));
  // reconstruction straight from what the parse leaves in HBM (failed clips: blank descriptors, no items)
  if (int e = b->begin_step()) return e;
  S.ring_base = b->ring_base;
  MobiReconArgs a = b->args(B.desc.p, B.pay.p);
  a.pay_clip_words = b->pay_clip_words;
  a.done = b->d_done;
  if (mobi_launch_inter(&a, b->stream) != 0) return MOBI_E_DEVICE;
  if (int e = b->motion_step(a)) return e;
  // the parse has not run yet, so nobody knows how many intra macroblocks the longest list will have: MOBI_ASYNC_INTRA_SLOTS slots are launched
  // (a P-frame's lists are shorter), and a second launch (mobi_recon_intra_walk, one workgroup per four clips) goes through the rest of theirs (an I-frame: every macroblock)
  if (mobi_launch_intra_cl(&a, (const uint32_t *)B.items.p, &d_res[0].n_intra, (int)(sizeof(MobiDevResult) / 4), std::min(n_mbs, MOBI_ASYNC_INTRA_SLOTS), 1, b->stream) != 0) return MOBI_E_DEVICE;
  if (int e = b->sink_step(a)) return e;
  if (int e = b->read_faults(B.faults())) return e;
  HIP_TRY(hipEventRecord(S.ev_done, b->stream));
  poison.armed = false;
  idle_commit(b, 1, idle);
  reset_commit(b, serial);
  b->async_count++;
  b->async_seq++;
  return MOBI_OK;
}
// Clips of the oldest step in flight whose frame the device parser could not finish.  Everything enqueued is drained first (a second step
// in flight parsed these clips from a state the failed frame left behind: its frame is repaired as well); then, per clip: the state the
// frame started from goes into the host parser, the staged bitstream is parsed again, and the frame is reconstructed on its own into the
// ring slot its step wrote.  The results replace the device's in the slots' host-side tables.
static int async_repair(mobi_batch *b, mobi_batch::AsyncSlot &S, const std::vector<int> &failed) {
  if (b->stream2) HIP_TRY(hipStreamSynchronize(b->stream2));
  if (b->stream_p) HIP_TRY(hipStreamSynchronize(b->stream_p));
  HIP_TRY(hipStreamSynchronize(b->stream));
  mobi_batch::AsyncSlot *S1 = b->async_count == 2 ? &b->aslot[(b->async_head + 1) & 1] : nullptr;
  const int k = (int)failed.size(), nT = S1 ? 2 : 1;
  mobi_batch::AsyncSlot *const T[2] = {&S, S1};
  // A clip reset between the two steps (mobi_batch_reset_clips) has its new stream's first frame in S1, parsed from a new decoder's state: the
  // repair stays in S, with the parser of the stream S belongs to (mobi_batch::parser_at), and leaves the clip's current state alone.
  std::vector<MobiStreamParser *> parser(k);
  std::vector<uint8_t> cascade(k, 0);
  for (int j = 0; j < k; j++) {
    parser[j] = b->parser_at(S.serial, failed[j]);
    cascade[j] = S1 && b->stale(S.serial, failed[j]) == b->stale(S1->serial, failed[j]) && !S1->is_idle(failed[j]); // (an idle slot behind: nothing to repair there)
  }
  // r06: a batch operation.  The start states in one go, the parses on the pool (a clip's two frames in order), then per affected step ONE
  // reconstruction of the failed clips (recon_clips) -- r05 did all of it clip by clip on the calling thread: a GOP damaged in every clip of a
  // batch, or a ModsDS batch that cuts to a quantiser below 12 in one frame, stalled mobi_batch_wait for ~1.5 ms x 2 x clips.
  if (int e = dp_seed_step(b, failed, S.state_in, S.B.h_ret, [&](int c) { return b->parser_at(S.serial, c); })) return e;
  if (b->gop_frames.size() < (size_t)k * 2) b->gop_frames.resize((size_t)k * 2);
  std::vector<int> prc((size_t)k * 2, MOBI_OK);
  b->pool->run(k, [&](int j) {
    const int c = failed[j];
    for (int t = 0; t < (cascade[j] ? 2 : 1); t++) {
      const StageImage &img = T[t]->img;
      HostShare &H = T[t]->H;
      int32_t off = 0;
      prc[(size_t)j * 2 + t] = parser[j]->parse_frame(T[t]->B.h_stage.p + img.hdr_bytes + img.boff[c], img.lens[c], &off, b->gop_frames[(size_t)j * 2 + t]);
      H.host_from[c] = 0;
      H.off[c] = H.offs[c] + off;
      H.quant[c] = parser[j]->quantizer();
      H.yuv[c] = parser[j]->yuv_format();
    }
  });
  for (int t = 0; t < nT; t++) {
    std::vector<int> cl;
    std::vector<const ParsedFrame *> fr;
    std::vector<int> js;
    for (int j = 0; j < k; j++)
      if (t == 0 || cascade[j]) {
        cl.push_back(failed[j]);
        js.push_back(j);
        fr.push_back(prc[(size_t)j * 2 + t] == MOBI_OK ? &b->gop_frames[(size_t)j * 2 + t] : nullptr);
      }
    std::vector<int> fault(cl.size());
    if (int e = recon_clips(b, cl, fr.data(), T[t]->ring_base, fault.data())) return e;
    for (size_t i = 0; i < cl.size(); i++) {
      T[t]->H.rc[cl[i]] = fault_rc(prc[(size_t)js[i] * 2 + t], fault[i]);
      T[t]->B.faults()[cl[i]] = 0;
    }
  }
  for (int c : failed) {
    if (b->stale(S.serial, c)) continue; // (the clip's current stream started with S1 or starts with the next step: its routing is a new decoder's)
    b->route_to_host(c);
  }
  b->fallbacks += failed.size();
  return MOBI_OK;
}
int mobi_batch_wait(mobi_batch *b, int32_t *offsets_out, int *rc) {
  if (!b || !rc) return MOBI_E_ARG;
  HIP_TRY(hipSetDevice(b->device));
  if (b->poisoned) return MOBI_E_DEVICE;
  if (b->async_count == 0) return MOBI_E_ARG;
  mobi_batch::AsyncSlot &S = b->aslot[b->async_head & 1];
  HIP_TRY(hipEventSynchronize(S.ev_done));
  const MobiDevResult *res = S.B.results();
  std::vector<int> failed;
  for (int i = 0; i < b->n; i++)
    if (S.H.host_from[i] && !S.is_idle(i) && res[i].rc != MOBI_OK) failed.push_back(i);
  if (!failed.empty())
    if (int e = async_repair(b, S, failed)) { b->poisoned = true; return e; }
  dp_report(b, S.H, S.B, 0, 1, offsets_out, rc); // (ls_finished: of the step being reported, not of the one submitted last: ADVICE r05)
  b->async_head ^= 1;
  b->async_count--;
  return MOBI_OK;
}
// What frames k0 .. k1 - 1 of a hand-over came to, in rc / offsets_out [(k - k0) * n + c]: rc and Offset, the host parser's where the frame was
// its, and Quantizer / YuvFormat behind each clip's last LIVE frame among them.  An idle slot: MOBI_IDLE, Offset as handed in, Quantizer /
// YuvFormat stay the last live frame's.
void dp_report(mobi_batch *b, const HostShare &H, const DpSet &B, int k0, int k1, int32_t *offsets_out, int *rc) {
  const int n = b->n;
  const MobiDevResult *res = B.results();
  const int *fault = B.faults();
  if (k0 == 0) b->ls_finished = H.lockstep ? 0 : -1;
  for (int k = k0; k < k1; k++)
    for (int c = 0; c < n; c++) {
      const size_t v = (size_t)k * n + c, o = (size_t)(k - k0) * n + c;
      if (k >= H.live_end(c)) {
        rc[o] = MOBI_IDLE;
        if (offsets_out) offsets_out[o] = H.offs[v];
        continue;
      }
      const bool host = k >= H.host_from[c];
      if (!host && H.lockstep && res[v].pad == MOBI_LS_MAGIC) b->ls_finished++;
      rc[o] = fault_rc(host ? H.rc[v] : res[v].rc, fault[v]);
      if (offsets_out) offsets_out[o] = host ? H.off[v] : H.offs[v] + (int32_t)res[v].consumed;
      if (k == std::min(k1, H.live_end(c)) - 1) {
        b->dev_quant[c] = host ? H.quant[v] : res[v].quant;
        b->dev_yuvfmt[c] = host ? H.yuv[v] : res[v].yuvfmt;
      }
    }
}
