// mobi_batch.h -- internal to the C-ABI layer of libmobiclip_hip.so (include/mobiclip_hip.h), never installed: the buffer and handle holders,
// the host parse pool, the launch plan, struct mobi_batch and the one copy of every idiom a frame step is made of -- among them what a
// device-parsed hand-over (a step, an asynchronous step, a group) owns and reports: DpSet, HostShare, and the staged image of mobi_handover.h.
// The entry points are in mobi_batch.cpp, mobi_step_host.cpp, mobi_step_device.cpp, mobi_step_groups.cpp, mobi_replay.cpp, mobi_pictures.cpp and mobi_sink.cpp.  There is no CPU
// reconstruction path: every entry point that produces pixels goes through mobi_launch_inter / mobi_launch_intra.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/mobiclip_hip.h"
#include "mobi_cmd.h"
#include "mobi_dparse.h"
#include "mobi_exporter.h"
#define MOBI_GOP_DEVICE_DECLS
#include "mobi_gop.h"
#include "mobi_handover.h"
static_assert(StageImage::kSkip == MOBI_DP_SKIP, "the staged image and the parse kernels name a skipped lane alike");
#include "mobi_kernels.h"
#include "mobi_motion_ring.h"
#include "mobi_tile.h"
#include "mobi_parse.h"

constexpr size_t kPaySlack = 2048; // lanes of the inter kernel with nothing to fetch re-read up to ~1 KB past their macroblock's payload
constexpr size_t kGuard = 65536; // slack on both ends of the plane arena: the slow MC path fetches the dwords of the row below a window's last
                                 // row whether its phase needs them or not, and in the tiled planes (mobi_tile.h) that row may be a tile row (<= 16 KB) away
constexpr size_t kAlign = 16;
constexpr size_t kFusedStepMbs = (size_t)256 * 1200; // steps of at most this many macroblocks go out as ONE launch (mobi_recon_step); MOBI_FUSED_STEP_MBS overrides, 0 = never

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

#define HIP_TRY(expr)                                                             \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess) {                                                       \
      snprintf(g_last_hip_error, sizeof(g_last_hip_error), "%s: %s", #expr, hipGetErrorString(e_)); \
      (void)hipGetLastError(); /* HIP keeps the error until somebody reads it: the next launch wrapper's hipGetLastError() must not find this one \
                                  (r05: an allocation that failed in one batch made the first launch of the NEXT batch report "out of memory") */ \
      return MOBI_E_DEVICE;                                                       \
    }                                                                             \
  } while (0)
extern thread_local char g_last_hip_error[256]; // (mobi_batch.cpp; mobi_error_string hands it out)
template <bool Pinned> struct GrowBuf { // growable buffer: pinned host staging memory (PinnedBuf) or device memory (DevBuf)
  uint8_t *p = nullptr;
  size_t cap = 0;
  void release() { if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
  int reserve(size_t n) {
    if (n <= cap) return MOBI_OK;
    release();
    size_t want = std::max(n, (size_t)1 << 20);
    HIP_TRY(Pinned ? hipHostMalloc((void **)&p, want, hipHostMallocDefault) : hipMalloc((void **)&p, want));
    cap = want;
    return MOBI_OK;
  }
  int grow(size_t n) { return n <= cap ? MOBI_OK : reserve(n + n / 4); } // growing is slow (pinned memory) or a device-wide stall (hipFree): leave room for the longer frames to come
  ~GrowBuf() { release(); }
};
using PinnedBuf = GrowBuf<true>;
using DevBuf = GrowBuf<false>;
template <class T> struct DevArr { // a device array of fixed size: allocated once (exactly `count` elements), released with its owner
  T *p = nullptr;
  int alloc(size_t count) { HIP_TRY(hipMalloc((void **)&p, count * sizeof(T))); return MOBI_OK; }
  void free() { if (p) (void)hipFree(p); p = nullptr; }
  operator T *() const { return p; }
  DevArr() = default; DevArr(const DevArr &) = delete;
  ~DevArr() { free(); }
};
template <class H, hipError_t (*Destroy)(H)> struct Owned { // an event or a stream its owner made (h == nullptr: not yet) and destroys
  H h = nullptr;
  operator H() const { return h; }
  Owned() = default; Owned(const Owned &) = delete;
  ~Owned() { if (h) (void)Destroy(h); }
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
inline int ensure_event(Event &e) { if (!e.h) HIP_TRY(hipEventCreateWithFlags(&e.h, hipEventDisableTiming)); return MOBI_OK; } // (ordering only: no timing)
inline int ensure_stream(Stream &s) { if (!s.h) HIP_TRY(hipStreamCreateWithFlags(&s.h, hipStreamNonBlocking)); return MOBI_OK; }
struct EventPool { std::vector<hipEvent_t> v; ~EventPool() { for (auto e : v) (void)hipEventDestroy(e); } }; // timing events not in use (mobi_batch::get_event)
inline float ms_since(std::chrono::steady_clock::time_point x) { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - x).count(); }

// One frame step on the device = [MbDesc table: n_clips * n_mbs][payload arena: all clips back to back].
// Clips whose parse failed (nullptr) get descriptors typed "intra" that no launch list references, so
// nothing of theirs is ever written (the reference leaves a partial frame; content is unspecified here).
inline size_t step_payload_words(const std::vector<const ParsedFrame *> &frames) {
  size_t w = 0;
  for (auto *f : frames)
    if (f) w += f->payload.size();
  return w;
}
// one clip's share of the step image; base = where its payload starts in the arena
inline void step_write_clip(const ParsedFrame *f, size_t base, int n_mbs, MbDesc *dd, uint32_t *payload) {
  if (!f) {
    for (int i = 0; i < n_mbs; i++) dd[i] = MbDesc{0, MOBI_MB_INTRA, 0, 0, 0, 0, 0, 0};
    return;
  }
  for (int i = 0; i < n_mbs; i++) {
    dd[i] = f->desc[i];
    dd[i].payload_off += (uint32_t)base;
  }
  if (!f->payload.empty()) memcpy(payload + base, f->payload.data(), f->payload.size() * 4);
}
inline void step_write(const std::vector<const ParsedFrame *> &frames, int n_mbs, MbDesc *desc, uint32_t *payload) {
  size_t base = 0;
  for (size_t c = 0; c < frames.size(); c++) {
    step_write_clip(frames[c], base, n_mbs, desc + c * (size_t)n_mbs, payload);
    if (frames[c]) base += frames[c]->payload.size();
  }
}

struct LevelPlan { // launch plan of one frame step: the intra macroblocks of all clips, sorted by dependency level
  // One item = MOBI_INTRA_ITEM_WORDS words, everything a wave needs to start (mobi_recon_intra); its layout: mobi_cmd.h, the intra launch item
  std::vector<uint32_t> items;
  uint32_t n_items = 0;         // launch items, padding included
  uint32_t n_intra = 0;         // intra macroblocks among them
  bool any_inter = false;
  uint64_t cmd_bytes = 0;       // descriptors + payload of every macroblock of the step
  uint64_t intra_cmd_bytes = 0; // ... of the intra ones: descriptor, 24 block records, level words (the inter kernel never reads them)
  void build(const std::vector<const ParsedFrame *> &frames, int /*mbw*/) {
    // Few intra macroblocks (small batches): every one gets a wave of its own (three null items behind it) -- the chip has room for
    // them all at once, and a lone macroblock's wave is shorter than a wave that runs the longest step list of four.  Measured
    // (640x480 P-frames, intra launch): 8 clips 45 -> 33 us, 64 clips 53 -> 41 us, 512 clips 78 -> 110 us: dense from there on.
#if defined(MOBI_PROFILING)
    static const int sparse_env = getenv("MOBI_INTRA_SPARSE") ? atoi(getenv("MOBI_INTRA_SPARSE")) : -1; // (measurements only)
#else
    const int sparse_env = -1;
#endif
    uint64_t total_intra = 0;
    for (auto *f : frames)
      if (f) total_intra += f->hdr.n_intra;
    const bool sparse = sparse_env >= 0 ? sparse_env != 0 : total_intra <= 4096;
    uint32_t maxl = 0;
    any_inter = false;
    cmd_bytes = 0;
    intra_cmd_bytes = 0;
    for (auto *f : frames)
      if (f) {
        maxl = std::max(maxl, f->hdr.n_levels);
        if (f->hdr.n_intra < f->hdr.n_mbs) any_inter = true;
        cmd_bytes += f->hdr.cmd_bytes;
      }
    items.clear();
    std::vector<size_t> base(frames.size() + 1, 0); // where each clip's payload starts in the step's arena (as step_write lays it out)
    for (size_t c = 0; c < frames.size(); c++) base[c + 1] = base[c] + (frames[c] ? frames[c]->payload.size() : 0);
    n_intra = 0;
    size_t total = 0;
    for (auto *f : frames)
      if (f) total += f->intra_items.size();
    items.reserve((sparse ? 4 : 1) * total + 16 * (size_t)maxl);
    const uint32_t none[4] = {MOBI_ITEM_NONE, 0, 0, 0};
    for (uint32_t L = 1; L <= maxl; L++) {
      // inside a level by class (mobi_parse.cpp, finish_levels): macroblocks away from the picture's edges first, those nobody depends on first, by the number of split areas
      // (a wave runs as many steps as the longest of its four macroblocks has, and publishes if any of them must); the ones at an edge (on Width == Stride pictures their halo
      // needs the per-sample ownership test, mobi_recon_intra) behind them, so that few waves of four carry one.  The parsers wrote the items
      // (ParsedFrame::intra_items): this is a concatenation with the clip number and the clip's place in the arena added.
      for (uint32_t k = 0; k < MOBI_INTRA_CLASSES; k++)
        for (size_t c = 0; c < frames.size(); c++) {
          const ParsedFrame *f = frames[c];
          if (!f || L > f->hdr.n_levels) continue;
          for (uint32_t i = f->class_start[(size_t)L * MOBI_INTRA_CLASSES + k]; i < f->class_start[(size_t)L * MOBI_INTRA_CLASSES + k + 1]; i++) {
            const uint32_t *it = &f->intra_items[(size_t)i * 4];
            intra_cmd_bytes += sizeof(MbDesc) + 4 * (MOBI_INTRA_RECORDS + mobi_item_coefs(it[3]));
            const uint32_t item[4] = {MOBI_ITEM(c, it[0]), it[1], it[2] + (uint32_t)base[c], mobi_item_shipped(it[3])};
            items.insert(items.end(), item, item + 4);
            n_intra++;
            for (int q = 1; q < 4 && sparse; q++) items.insert(items.end(), none, none + 4);
          }
        }
      // a wave carries four macroblocks, and a macroblock may wait for one of the level before: levels start on a wave boundary
      while ((items.size() / MOBI_INTRA_ITEM_WORDS) & 3) items.insert(items.end(), none, none + 4);
    }
    n_items = (uint32_t)(items.size() / MOBI_INTRA_ITEM_WORDS);
  }
};

// Host-side parse pool: the VLC parse is serial inside a clip but clips are independent (MD.cs:15-39), so the clips of a
// batch are parsed by a few persistent threads (the reference runs one decode thread per open file, Form1.cs:199-215).
class ParsePool {
 public:
  explicit ParsePool(int n_threads) {
    for (int i = 0; i < n_threads; i++) th_.emplace_back([this] { worker(); });
  }
  ~ParsePool() {
    { std::lock_guard<std::mutex> l(m_); stop_ = true; gen_++; }
    cv_.notify_all();
    for (auto &t : th_) t.join();
  }
  int size() const { return (int)th_.size(); }
  // runs f(0..n-1), the caller's thread included; returns when all are done
  void run(int n, const std::function<void(int)> &f) {
    if (th_.empty() || n < 2) { for (int i = 0; i < n; i++) f(i); return; }
    { std::lock_guard<std::mutex> l(m_); job_ = &f; n_ = n; next_.store(0); busy_ = (int)th_.size(); gen_++; }
    cv_.notify_all();
    drain();
    std::unique_lock<std::mutex> l(m_);
    done_.wait(l, [this] { return busy_ == 0; });
    job_ = nullptr;
  }

 private:
  void drain() {
    for (int i; (i = next_.fetch_add(1)) < n_;) (*job_)(i);
  }
  void worker() {
    uint64_t seen = 0;
    for (;;) {
      { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [&] { return gen_ != seen; }); seen = gen_; if (stop_) return; }
      drain();
      { std::lock_guard<std::mutex> l(m_); if (--busy_ == 0) done_.notify_one(); }
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  const std::function<void(int)> *job_ = nullptr;
  std::atomic<int> next_{0};
  int n_ = 0, busy_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

// one frame through a host parser.  Data == null: nothing readable, as Data.Length == 0
inline int parse_host(MobiStreamParser *p, const uint8_t *data, size_t len, int32_t *off, ParsedFrame &out) {
  static const uint8_t kNoData[2] = {0, 0}; return p->parse_frame(data ? data : kNoData, data ? len : 0, off, out);
}
// a reconstruction fault word behind an rc that is still MOBI_OK (bit 1: an intra dependency never arrived)
static inline int fault_rc(int rc, int fault) { return rc == MOBI_OK && fault ? ((fault & 2) ? MOBI_E_DEVICE : MOBI_E_CLAMP) : rc; }

// What a device-parsed hand-over of `frames` x n lanes owns: the staged image's two copies, what its parse leaves in HBM ([v][n_mbs] descriptors
// and items, cap_words payload words per lane, [v] results), the pinned copies of results and fault words, the staging of the host parser's
// command lists (dp_override) and of states on their way back (dp_return_list), and the events "uploaded" and "parsed".  One in mobi_batch
// (mobi_batch_decode), one per AsyncSlot, one per GopSlot.
struct DpSet {
  DevBuf bits, desc, pay, items, res;
  PinnedBuf h_stage, h_res, h_fault, h_over, h_ret;
  Event ev_up, ev_parsed;
  size_t cap_words = 0, n = 0, n_mbs = 0;
  int reserve_results(size_t lanes) { if (int e = res.reserve(lanes * sizeof(MobiDevResult))) return e; return h_res.reserve(lanes * sizeof(MobiDevResult)); }
  // MbDesc.payload_off is relative to the lane's own part of the arena, which may then be as large as HBM lets it (24576 clips of
  // 640x480 need 13 G words for an I-frame); the host parser's clips write into their own parts like everybody else (dp_override)
  int reserve_tables(size_t lanes, int n_clips, int mbs, size_t words) {
    n = (size_t)n_clips; n_mbs = (size_t)mbs; cap_words = words;
    if (int e = desc.reserve(align_up(lanes * n_mbs * sizeof(MbDesc) + 8 * sizeof(MbDesc), kAlign))) return e;
    if (int e = pay.reserve(align_up(lanes * cap_words * 4 + kPaySlack, kAlign))) return e;
    return items.reserve(lanes * n_mbs * 4);
  }
  struct Rows { uint8_t *desc, *pay, *items; MobiDevResult *res; };
  Rows rows(int k) const { const size_t v = (size_t)k * n; return {desc.p + v * n_mbs * sizeof(MbDesc), pay.p + v * cap_words * 4, items.p + v * n_mbs * 4, (MobiDevResult *)res.p + v}; } // frame k's tables
  const MobiDevResult *results() const { return (const MobiDevResult *)h_res.p; }
  int *faults() const { return (int *)h_fault.p; }
};
// The host parser's share of a hand-over of K frames and what it came to, [v] = [k * n + c]: its own clips when the parse was enqueued (from
// frame 0) and the clips it took over at the first frame the device parsers could not finish.  A step is K = 1.
struct HostShare {
  int K = 0;
  bool lockstep = false;           // the lock-step parser was in front of THIS hand-over (ls_decide)
  std::vector<int32_t> offs;       // [v] Offset at submission
  std::vector<uint8_t> idle_from;  // [c] the clip's first idle frame (K: none; mobi_batch_set_idle); empty: the hand-over has no idle slot
  std::vector<int> host_from, rc;  // [c] the first frame that is the host parser's (K: none); [v] its rc
  std::vector<int32_t> off;        // [v] Offset behind a host-parsed frame
  std::vector<uint32_t> quant, yuv; // [v] Quantizer / YuvFormat behind it (the parser itself may be further by the time of the report)
  int live_end(int c) const { return idle_from.empty() ? K : idle_from[c]; } // frames [0, live_end) of clip c are live
  void clear(int n) { const size_t nv = (size_t)n * K; host_from.assign(n, K); rc.assign(nv, MOBI_OK); off.assign(nv, 0); quant.assign(nv, 0); yuv.assign(nv, 0); }
};
struct DpSeed { const MobiDevState *state; const MobiDevTail *tail; MobiStreamParser *parser; }; // device addresses of a start state, and whose it becomes (dp_seed_parsers)
struct ParseTimer { // HIP events around the parse launches (kernel timing on): made on demand
  Event a, b;
  bool on(bool timing) { if (timing && !a) { (void)hipEventCreate(&a.h); (void)hipEventCreate(&b.h); } return timing && a && b; }
  void start(bool timing, hipStream_t s) { if (on(timing)) (void)hipEventRecord(a, s); }
  void stop(bool timing, hipStream_t s) { if (on(timing)) (void)hipEventRecord(b, s); }
  void read(bool timing, float &ms_out) { float ms = 0; if (timing && a && b && hipEventElapsedTime(&ms, a, b) == hipSuccess) ms_out = ms; }
};

struct mobi_batch {
  int n = 0, device = 0, version = 0;
  MobiGeom g{};
  // the streams first: members go in reverse order of declaration, so every event and buffer below is released before them, and `stream` last of all
  Stream stream;
  Stream stream2;  // parse mode 2, asynchronous steps, groups: uploads and the host parser's command lists go up on this stream, beside the parse kernel
  Stream stream_p; // asynchronous steps, groups: the parse kernels (upload on stream2, reconstruction on stream)
  DevArr<uint8_t> arena; // guard | clips x 6 slots | guard
  size_t slot_bytes = 0, clip_bytes = 0;
  int ring_base = 0;
  int frames_started = 0;
  bool poisoned = false; // an asynchronous submit failed half-way (mobi_batch_submit): nothing further is accepted
  int debug = 0;
  std::vector<std::unique_ptr<MobiStreamParser>> parsers;
  std::vector<ParsedFrame> cur; // per clip, current frame (batch_decode)
  DevArr<int> d_fault;
  std::vector<int> h_fault;
  // per-call staging (batch_decode)
  PinnedBuf h_stage;
  PinnedBuf h_items;                   // host-parsed steps: the launch list (the staging buffer's chunks are in flight by then)
  DevBuf d_cmd, d_items;
  DevArr<int32_t> d_scale; // [MOBI_SCALE_QMAX][MOBI_SCALE_STRIDE]
  DevArr<unsigned long long> d_prof; // MOBI_DEBUG=9: in-kernel cycle accumulators
  std::unique_ptr<ParsePool> pool;      // host parse threads (MOBI_PARSE_THREADS, default min(clips, cores, 32) - 1 helpers)
  DevArr<uint32_t> d_argb;              // Bitmap output of mobi_batch_convert_argb / mobi_batch_get_argb (lazily allocated)
  size_t argb_bytes = 0;
  bool argb_all_valid = false;          // d_argb holds every clip's Bitmap of the current frame
  DevArr<uint8_t> d_lin;                // one frame in the reference's linear layout: what mobi_batch_get_planes copies out (lazily allocated)
  DevArr<uint32_t> d_done;              // [clip * n_mbs + mb]: step tag of the last step that reconstructed this intra macroblock
  uint32_t step_tag = 0;                // bumped once per frame step, never 0
  // device-side parse (mobi_dparse.hip): parse_mode 1 = mobi_batch_decode parses on the GPU (env MOBI_DEVICE_PARSE=1 or
  // mobi_batch_set_parse_mode); the per-clip decoder state then lives in d_pstate and the host parsers stay untouched
  int parse_mode = 0; // explicit (env / mobi_batch_set_parse_mode), or by batch size and settled at the first frame (parse_auto)
  bool parse_auto = false;
  int hybrid_host = 0;           // parse mode 2: the last hybrid_host clips are parsed by the host pool while the GPU parses the others
  DpSet dp; // mobi_batch_decode's device-parsed steps
  size_t last_pay_cap = 0; // payload bound of the last step's parse, synchronous or not (mobi_debug_read_parse)
  float last_parse_ms = 0; // duration of the last mobi_parse_frames launch (kernel timing on)
  float last_decode_ms = 0, last_stage_ms = 0; // wall time of the last mobi_batch_decode call / of its host staging part
  float phase_ms[6] = {0, 0, 0, 0, 0, 0};      // (profiling) host-parsed step: parse loop, plan, stage + upload enqueue, launch enqueue, sync; device-parsed step: cumulative ms after gather + upload, parse enqueued, parse done, launches enqueued, all done
  float last_hostparse_ms = 0;                 // ... / of its host parse part (host parse mode)
  DevBuf d_src, d_search; // mobi_batch_motion_search: the pictures being analysed, the packed results
  // the decoder state of the device-parsed clips: a ring of three entries (a step reads ps_cur, writes ps_cur + 1), so that the state a frame
  // STARTED from is still there when the host parser has to take the frame over (decode_device_parse, async_repair; mobi_state.h)
  DevArr<MobiDevState> d_pstate[3];
  DevArr<MobiDevTail> d_ptail[3];
  int ps_cur = 0;
  DevArr<MobiDevState> d_pstate_ls;    // shadow copy the lock-step parser writes (mobi_lsparse.hip)
  std::vector<uint8_t> on_host;        // [clip] device-parse modes: this clip is the host parser's (the hybrid mode's share; clips with a frame the
                                       // device parser could not finish, from that frame on)
  unsigned long fallbacks = 0;         // frames taken over so far
  unsigned long returns = 0;           // clips handed back to the device parsers so far (dp_return)
  std::vector<uint8_t> host_share;     // [clip] 1: the hybrid mode's share (stays with the host parser by design)
  std::vector<uint16_t> clean_run, clean_need; // [clip] consecutive frames the device parsers could have finished; how many it takes to go back
  PinnedBuf h_fix;                     // async_repair: one clip's command list
  DevBuf d_fix;
  uint32_t pay_clip_words = 0;         // of the last device-parsed step (MobiReconArgs.pay_clip_words)
  int ls_finished = -1;                // clips of the last step it finished itself
  int ls_policy = 0;                   // 0: never (parse modes 1, 2 named by the caller); 1: always (mode 3); 2: by step (the default, ls_decide)
  bool lockstep = false;               // this step: mobi_parse_frames_ls in front of mobi_parse_frames
  int host_chunk = 256;                // host-parsed steps: clips per chunk of the parse / stage / upload pipeline (mobi_batch_decode)
  size_t fused_mbs = kFusedStepMbs;     // launch_plan: steps of at most this many macroblocks go out as one launch
  DevArr<uint8_t> d_ptables;
  std::vector<uint32_t> dev_quant, dev_yuvfmt;
  // asynchronous steps (mobi_batch_submit / mobi_batch_wait, device parse only): two sets of staging so that the bytes of step
  // n + 1 are gathered and uploaded while the GPU works on step n; everything else follows stream order
  struct AsyncSlot {
    // (what the parse of this step leaves in HBM is the slot's, so that the parse of step n + 1 -- on stream_p -- may run under the
    // reconstruction of step n -- on stream --, which still reads step n's)
    DpSet B;
    StageImage img;                  // of the staged bitstream (B.h_stage): async_repair parses from it
    HostShare H;                     // clips whose result is the host parser's (its own clips at submission; clips repaired in mobi_batch_wait)
    Event ev_done;
    bool parsed_recorded = false;    // B.ev_parsed has been recorded at least once
    int state_in = 0, ring_base = 0; // the entry of the state ring this step's parse read; the ring position its reconstruction wrote
    uint64_t serial = 0;             // the step's place among the steps handed over (stream generations: mobi_batch::stale)
    bool is_idle(int c) const { return H.live_end(c) == 0; } // an idle slot of this step (mobi_batch_set_idle)
  };
  AsyncSlot aslot[2];
  // frame-parallel groups (mobi_batch_gop_begin / mobi_batch_gop_finish, mobi_gop.h): K frames of every clip parsed side by side as n * K
  // virtual clips (v = k * n + c), reconstructed as K steps.  Two slots: the bytes of group g + 1 are gathered and uploaded, and its parse
  // enqueued, while group g is reconstructed.
  struct GopSlot {
    DpSet B;
    StageImage img;                  // boff / lens: where the host parser finds its frames (the header's copy says MOBI_DP_SKIP for its clips)
    HostShare H;                     // host_from ... : what the group's first mobi_batch_gop_finish settles for all K frames (a group of more than six is finished in two calls)
    PinnedBuf h_over[MOBI_GOP_PARSE_MAX], h_seed;
    DevBuf d_sin, d_sout, d_sls, d_tails, d_fault;
    Event ev_recon;
    bool parse_enqueued = false;
    int ring_in = 0;                 // the state ring entry the group's parse read
    uint64_t serial = 0;             // the group's place among the steps handed over (stream generations: mobi_batch::stale)
    std::vector<uint8_t> is_host;    // [c] the host parser's clip when the parse was enqueued
    bool resolved = false, returned = false; // (returned: the clips that go back to the device parsers have been sent)
    bool sorted = false;             // the group's intra macroblocks were put in wavefront order on the device (mobi_launch_gop_sort)
    DevBuf d_sorted, d_hist;
    uint64_t sorted_off[MOBI_GOP_PARSE_MAX] = {0};
    uint32_t sorted_items[MOBI_GOP_PARSE_MAX] = {0};
    int done = 0;                    // frames reconstructed and reported so far
    std::vector<int> hslot, all_host;
    std::vector<uint8_t> hready;
  };
  GopSlot gslot[2];
  int gop_head = 0, gop_count = 0;
  std::vector<ParsedFrame> gop_frames; // host-parsed frames of the group being finished
  int async_head = 0, async_count = 0; // oldest step in flight, number of steps in flight (<= 2)
  size_t dp_len_hint = 0;              // longest frame seen so far (+ 25 %): sizes the payload arena of the device-side parser
  uint64_t async_seq = 0;
  // preloaded replay
  // [clip] -> frames; clones share the host copy (each clip still gets its own bytes in HBM at commit)
  std::vector<std::shared_ptr<std::vector<ParsedFrame>>> staged;
  std::vector<std::shared_ptr<std::vector<int>>> staged_rc;
  int n_frames_loaded = 0;
  DevBuf r_cmd, r_items;
  std::vector<LevelPlan> r_plan;        // per frame
  std::vector<size_t> r_items_off;      // per frame: word offset of its items in r_items
  std::vector<size_t> r_desc_off, r_payload_off; // per frame: byte offsets inside r_cmd
  bool committed = false;
  // timing
  Event ev_begin, ev_end;
  ParseTimer ptimer;  // around the parse launch (kernel timing on)
  int ktiming = 0; // HIP events around launches: 0 none, 1 the inter launches (the dominant kernel: roofline), 2 every launch
  struct EvPair { hipEvent_t a, b; int kind; };
  std::vector<EvPair> evs;
  EventPool ev_pool;
  float acc_ms[2] = {0, 0};
  int acc_launches[2] = {0, 0};
  // export to host memory (mobi_batch_export, mobi_export.cpp): created at the first export; its staging chunks with it
  MobiExporter *exporter = nullptr;
  // clip resets (mobi_batch_reset_clips).  A reset is recorded here and applied with the next step handed over (decode, submit, group): the
  // host side (parser, routing) at once, the device side (mobi_reset_state) in front of that step's parse.  Stream generations: every step
  // handed over gets the next serial, and stream_gen[c] is the serial of the step clip c's current stream started with; a step in flight
  // with serial < stream_gen[c] belongs to the stream before, and its late bookkeeping (repairs and their cascade, on_host, dp_return,
  // clean_run) leaves the clip's current state alone.  Its host parser is then retired[c] -- at most one older stream is ever in flight.
  std::vector<int32_t> reset_list;     // clips reset and not handed over yet, each once
  std::vector<uint8_t> reset_pending;  // [clip] in reset_list
  std::vector<int> frames_base;        // [clip] the value of frames_started at which the current stream's first frame has turned the ring
  std::vector<uint64_t> stream_gen;    // [clip] serial of the current stream's first step (0: the batch's first stream)
  std::vector<std::unique_ptr<MobiStreamParser>> retired; // [clip] the parser of the stream before, while a step of it may be in flight
  uint64_t handover = 0;               // serial of the last step handed over
  bool stale(uint64_t serial, int c) const { return serial < stream_gen[c]; }
  MobiStreamParser *parser_at(uint64_t serial, int c) const { return stale(serial, c) ? retired[c].get() : parsers[c].get(); }
  // idle frame slots (mobi_batch_set_idle).  The mask waits here for the next hand-over, which checks it (idle_check: before anything changes),
  // keeps the slots out of gather, upload and both parsers, launches mobi_idle_rows in front of its parse (only with idle slots) and books
  // the slots (idle_commit, beside reset_commit).  A caller that never sets a mask has idle_frames == 0 and n_ended == 0: nothing below runs.
  std::vector<uint8_t> idle_mask;      // [k * n + c] of the next hand-over
  int idle_frames = 0;                 // its n_frames (0: no mask set)
  std::vector<uint8_t> ended;          // [clip] the stream has ended (an idle slot was handed over): live frames only after a reset
  int n_ended = 0;                     // clips with the mark
  std::vector<int32_t> idle_count;     // [clip] idle slots handed over since the clip's last live frame or reset
  int idle_launches = 0;               // launches of mobi_idle_rows so far (mobi_batch_idle_launches)
  // the motion ring (mobi_batch_set_motion; mobi_motion_ring.h): six slots per clip beside the picture ring's, the slot index is ring_base.
  // A batch that never asks for motion has motion_on == false: no allocation, and motion_step below returns at its first test.
  bool motion_on = false;
  DevArr<uint32_t> d_mcells;           // [clip][slot][mb][64]
  DevArr<int32_t> d_mmbs;              // [clip][slot][mb][MOBI_MOTION_MB_WORDS]
  int motion_from = 0;                 // frames_started when motion was switched on: frames after that one have a motion slot
  long motion_launches = 0;            // launches of mobi_motion_field so far (mobi_batch_motion_launches)
  size_t motion_bytes() const { return motion_on ? (size_t)n * 6 * g.mbw * g.mbh * (64 + MOBI_MOTION_MB_WORDS) * 4 : 0; }
  bool motion_has(int ring_idx) const { return motion_on && frames_started - ring_idx > motion_from; }
  // The hook of every place that launches reconstruction: the step's command list -> its motion slot, directly behind the step's inter launch
  // on the batch's stream, i.e. before whatever lets the next parse reuse the list's tables.  a = the step's own arguments (a partial launch
  // carries its first clip in `planes`).  The slot is the step's, which begin_step has guarded; a repair writes the slot of an earlier
  // step (recon_clips) and takes the guard here.  Idempotent: a step launched twice writes the same words twice.
  int motion_step(const MobiReconArgs &a) {
    if (!motion_on) return MOBI_OK;
    if (a.ring_base != ring_base)
      if (int e = exporter ? mobi_exporter_guard(exporter, a.ring_base, stream) : MOBI_OK) return e;
    const MobiMotionRing ring{d_mcells, d_mmbs};
    if (mobi_launch_motion_field(&a, (int)((size_t)(a.planes - (arena + kGuard)) / clip_bytes), &ring, stream) != 0) return MOBI_E_DEVICE;
    motion_launches++;
    return MOBI_OK;
  }

  // the clip sink (mobi_batch_set_sink; mobi_sink.h, mobi_sink.cpp): armed, it rides along with the frame steps.  A batch that never arms
  // one has sink.on == false: no allocation, and sink_step below returns at its first test.
  struct Sink {
    bool on = false;                   // armed, or complete with a step that may still be repaired in flight (begin_step retires it)
    int planar = 0, esize = 0;
    MobiRgbAffine sb{};
    MobiResampleCall call{};           // out size, the largest tiling and LDS of the clips, the records in device memory
    MobiSinkSched sch{};               // stride, T, the three strides (step: filled per launch)
    uint8_t *dst = nullptr;
    std::vector<uint32_t> start;       // [clip], the host's copy of the records' `start`
    DevArr<MobiResampleClip> d_recs;   // [clip], uploaded once at arming
    int64_t now = -1;                  // the step begun last (-1: none since arming)
    int64_t counted = -1;              // steps up to this one have been taken off `pending` (a repair launches an earlier step again)
    int64_t last = 0;                  // the last step in which any clip contributes
    int64_t pending = 0;               // (clip, t) pictures not launched yet
  };
  Sink sink;
  long sink_launches = 0;              // launches of mobi_sink so far (mobi_batch_sink_launches)
  int sink_launch(const MobiReconArgs &a); // mobi_sink.cpp
  // The hook of every place that launches reconstruction into a ring slot, directly behind the step's LAST reconstruction launch (the intra
  // one) on the batch's stream: the pictures this step contributes go to the tensor.  a = the step's own arguments; a partial launch (a
  // repair, recon_clips) carries its first clip in `planes`, its clip count in n_clips and the ring slot of the EARLIER step it rewrites,
  // from which the step's number follows.  No guard: the sink reads the slot behind its writers and in front of the next, in stream order.
  // Idempotent: a step launched twice writes the same words twice.
  int sink_step(const MobiReconArgs &a) { return sink.on ? sink_launch(a) : MOBI_OK; }

  // The ring-slot guard, called by every step that writes a ring slot, right after the ring has turned and before anything of the step is
  // enqueued: the slot the step writes (ring_base) may still be read by the pack of an export; the batch's stream then waits for it.  With no
  // export outstanding (or none ever) it does nothing.
  int guard_slot() { return exporter ? mobi_exporter_guard(exporter, ring_base, stream) : MOBI_OK; }
  // a frame step begins: the ring turns -- Y[i] = Y[i-1]; Y[0] = new (MD.cs:102-108), even if the parse threw --, the step gets its tag, its slot is guarded
  void next_tag() { step_tag = step_tag + 1 ? step_tag + 1 : 1; }
  // (an armed sink counts the step; a complete one goes once no submitted step, which mobi_batch_wait may still repair, is in flight)
  void sink_begin_step() { if (sink.pending == 0 && async_count == 0) sink.on = false; else sink.now++; }
  int begin_step() { ring_base = (ring_base + 1) % 6; next_tag(); argb_all_valid = false; frames_started++; if (sink.on) sink_begin_step(); return guard_slot(); }
  // the fault words of the step(s) enqueued, read back into dst[n] and cleared for the next, in stream order
  int read_faults(int *dst) {
    HIP_TRY(hipMemcpyAsync(dst, d_fault, sizeof(int) * n, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemsetAsync(d_fault, 0, sizeof(int) * n, stream));
    return MOBI_OK;
  }
  // clip c is the host parser's from now on; the way back (dp_return) takes twice as many clean frames with every hand-over
  void route_to_host(int c) { on_host[c] = 1; clean_run[c] = 0; clean_need[c] = (uint16_t)std::min(256, 2 * (int)clean_need[c]); }
  // hybrid: the last clips are the host parsers' from the start (their state is a new decoder's: nothing to seed); after dp_init
  void mark_hybrid_share() { if (frames_started == 0) for (int i = n - hybrid_host; i < n; i++) on_host[i] = host_share[i] = 1; }
  bool version_known() const { return version == MOBI_VERSION_MODSDS || version == MOBI_VERSION_MOFLEX3DS; } // (the versions the device parsers know)

  MobiReconArgs args(const uint8_t *desc, const uint8_t *payload) const {
    MobiReconArgs a;
    memset(&a, 0, sizeof(a));
    a.planes = arena + kGuard;
    a.desc = (const MbDesc *)desc;
    a.payload = (const uint32_t *)payload;
    a.scale = d_scale;
    a.fault = d_fault;
    a.clip_bytes = clip_bytes;
    a.slot_bytes = (uint32_t)slot_bytes;
    a.ring_base = ring_base;
    a.width = g.width; a.height = g.height; a.stride = g.stride; a.mbw = g.mbw;
    a.n_mbs = g.mbw * g.mbh;
    a.n_clips = n;
    auto magic = [](uint32_t d) { uint64_t m = ((uint64_t)1 << 32) / d; return (uint32_t)(m > 0xFFFFFFFFull ? 0xFFFFFFFFull : m); }; // d == 1 must not wrap to 0
    a.step_tag = step_tag;
    a.done = d_done;
    a.prof = d_prof;
    a.qpr = (uint32_t)(a.mbw + 3) / 4;
    a.qpc = a.qpr * (uint32_t)g.mbh;
    a.magic_qpr = magic(a.qpr);
    a.magic_qpc = magic(a.qpc);
    return a;
  }
  hipEvent_t get_event() {
    if (!ev_pool.v.empty()) { hipEvent_t e = ev_pool.v.back(); ev_pool.v.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  // one frame step = the inter launch, then ONE intra launch for all dependency levels (items sorted by level, waves wait for
  // the tags of the macroblocks they depend on).  r01 also had a launch per level and a whole-step launch; both were slower.
  bool last_fused = false; // the last launch_plan went out as one launch (mobi_recon_step)
  int launch_plan(const MobiReconArgs &a, const LevelPlan &plan, const uint32_t *items_dev, int n_clips = -1, bool allow_fused = true) {
    if (n_clips < 0) n_clips = n;
    last_fused = false;
    // Small steps (BASELINE config 4: 8 clips per GPU): one launch carries both kinds of macroblock -- the kernel boundary between the two
    // launches is a fifth of such a step.  Large ones keep two: the fused kernel has the octet's registers and LDS for the intra fours too.
    if (allow_fused && plan.any_inter && plan.n_items && (size_t)n_clips * g.mbw * g.mbh <= fused_mbs) {
      last_fused = true;
      EvPair ep{nullptr, nullptr, 0};
      if (ktiming) { ep.a = get_event(); ep.b = get_event(); (void)hipEventRecord(ep.a, stream); }
      if (mobi_launch_step(&a, items_dev, (int)plan.n_items, stream) != 0) return MOBI_E_DEVICE;
      if (ktiming) { (void)hipEventRecord(ep.b, stream); evs.push_back(ep); }
      if (int e = motion_step(a)) return e;
      return sink_step(a);
    }
    if (plan.any_inter) {
      EvPair ep{nullptr, nullptr, 0};
      if (ktiming) { ep.a = get_event(); ep.b = get_event(); (void)hipEventRecord(ep.a, stream); }
      if (mobi_launch_inter(&a, stream) != 0) return MOBI_E_DEVICE;
      if (ktiming) { (void)hipEventRecord(ep.b, stream); evs.push_back(ep); }
    }
    if (int e = motion_step(a)) return e;
    if (plan.n_items) {
      EvPair ep{nullptr, nullptr, 1};
      if (ktiming >= 2) { ep.a = get_event(); ep.b = get_event(); (void)hipEventRecord(ep.a, stream); }
      if (mobi_launch_intra(&a, items_dev, (int)plan.n_items, stream) != 0) return MOBI_E_DEVICE;
      if (ktiming >= 2) { (void)hipEventRecord(ep.b, stream); evs.push_back(ep); }
    }
    return sink_step(a);
  }
  void drain_events() {
    for (auto &e : evs) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) { acc_ms[e.kind] += ms; acc_launches[e.kind]++; }
      ev_pool.v.push_back(e.a);
      ev_pool.v.push_back(e.b);
    }
    evs.clear();
  }
  ~mobi_batch() {
    if (exporter) mobi_exporter_delete(exporter); // (waits for the exports outstanding: they read the ring and write the callers' memory)
    exporter = nullptr;
    if (stream2) (void)hipStreamSynchronize(stream2); // an upload of a submitted step may still be reading pinned memory we are about to free
    if (stream_p) (void)hipStreamSynchronize(stream_p);
    if (stream) (void)hipStreamSynchronize(stream);
    drain_events(); // (the timing events go back to the pool; the members release everything else)
  }
};

struct mobi_dec { mobi_batch *b; };

// Once the parsers have consumed a frame and the ring has turned, a call that fails before its reconstruction is complete must not leave
// any clip reporting MOBI_OK for a frame that was never reconstructed (host-parsed and device-parsed steps alike: ADVICE r03)
struct FailAll {
  int *rc; int n; hipStream_t stream = nullptr; bool armed = true;
  ~FailAll() {
    if (!armed) return;
    for (int i = 0; i < n; i++) if (rc[i] == MOBI_OK) rc[i] = MOBI_E_DEVICE;
    //  copies out of the pinned staging buffers may still be in flight on the error paths: the next call refills those buffers
    if (stream) (void)hipStreamSynchronize(stream);
  }
};
// a failure with work in flight: the batch is drained and POISONED, every later call reports MOBI_E_DEVICE (mobi_batch_submit, mobi_batch_gop_finish)
struct Poison {
  mobi_batch *b; bool armed = true;
  ~Poison() {
    if (!armed) return;
    if (b->stream2) (void)hipStreamSynchronize(b->stream2);
    if (b->stream_p) (void)hipStreamSynchronize(b->stream_p);
    (void)hipStreamSynchronize(b->stream);
    b->poisoned = true;
  }
};

// ---- shared between the translation units (mobi_batch.cpp, mobi_step_device.cpp, mobi_pictures.cpp) ----
void settle_parse_mode(mobi_batch *b, bool first, size_t lanes, bool force_device, const uint8_t *const *data = nullptr, const size_t *len = nullptr, const int32_t *offsets = nullptr);
void reset_apply_host(mobi_batch *b, uint64_t serial);
void reset_commit(mobi_batch *b, uint64_t serial);
// idle slots of a hand-over of K frames: from[c] = clip c's first idle frame (K: none), empty when there is no idle slot at all.  MOBI_E_ARG for
// a mask of another n_frames, idle slots that are not a suffix, a live frame of an ended clip no pending reset names; changes nothing.
int idle_check(const mobi_batch *b, int K, std::vector<uint8_t> &from);
void idle_commit(mobi_batch *b, int K, const std::vector<uint8_t> &from); // the hand-over is made: marks and counts, the mask is consumed; BEFORE reset_commit
int dp_init(mobi_batch *b);
bool ls_decide(const mobi_batch *b, const StageImage &img);
// the staged image of a hand-over (mobi_handover.h; resets: its reset list, img.n_reset clips) gathered into B.h_stage by the pool in `chunks` rounds of tasks of `run` frames; up != nullptr:
// and sent to B.bits on `up`, each round's bytes while the next is gathered (header_too: the header with the first, else the bits only)
// t0: when the caller began planning it (last_stage_ms counts from there)
int dp_stage(mobi_batch *b, const StageImage &img, DpSet &B, const uint8_t *const *data, const int32_t *offsets, const uint8_t *idle_from, const int32_t *resets, int chunks, int run,
             hipStream_t up, bool header_too, std::chrono::steady_clock::time_point t0);
size_t dp_cap_words(mobi_batch *b, size_t max_len);
void dp_parse_args(const mobi_batch *b, const StageImage &img, const DpSet &B, MobiDevParseArgs &pa);
int dp_idle_rows(mobi_batch *b, const StageImage &img, const DpSet &B, const MobiDevParseArgs &pa, bool carry_state, hipStream_t s);
int dp_seed_parsers(mobi_batch *b, const std::vector<DpSeed> &seeds, PinnedBuf &stage, hipStream_t s);
int dp_override(mobi_batch *b, const std::vector<int> &clips, const int *rc, PinnedBuf &stage, const DpSet &B, int k, hipStream_t s,
                const ParsedFrame *const *frames = nullptr, const int *rcs = nullptr);
int dp_return_list(mobi_batch *b, const std::vector<int> &back, int entry, DpSet &B, hipStream_t s);
void dp_report(mobi_batch *b, const HostShare &H, const DpSet &B, int k0, int k1, int32_t *offsets_out, int *rc);
int decode_device_parse(mobi_batch *b, const uint8_t *const *data, const size_t *len, int32_t *offsets, int *rc);
int ensure_argb(mobi_batch *b, int n_clips);
