// mobi_export.cpp -- decoded pictures out to host and device memory (include/mobiclip_hip.h, mobi_batch_export*): the pinned-block registry of
// mobi_host_alloc, the staging pipeline, the tickets and the ring-slot guard.  The C entry points are in mobi_pictures.cpp; what they hand
// over is mobi_exporter.h's.
//
// Pipeline ("Export"): an export is cut into chunks of whole pictures.  Chunk i goes to staging chunk k = i mod kChunks:
//   pack stream:  [once per export: wait for the batch's stream]  wait ev_copied[k]  pack (mobi_export_i420 / mobi_yuv_to_argb)  ev_packed[k]
//   copy stream:  wait ev_packed[k]  hipMemcpyAsync D2H into dst (pinned) or into bounce chunk k (any other dst)  ev_copied[k]
// so the pack of chunk i + 1 runs under the copy of chunk i, and a staging chunk is packed again only once the copy engine has read it.
// The copy stream is in order: the event behind an export's last copy says "this export and every earlier one is in dst" (the ticket).
//
// Export to device memory (mobi_batch_export_device) has no pipeline: the caller's stream waits for the batch's stream and the kernels
// write straight into dst.  A batch that only does that creates no streams and allocates no staging (init_events, not init_staging).
//
// An export whose kernel needs per-call data in device memory (mobi_batch_export_device_boxes: a record per clip) hands it over as
// MobiExportParams; it travels in a parameter block of a small pool: filled on the host, copied on the caller's stream in front of the
// launch, free again when the event recorded behind the launch has completed.
//
// The ring-slot guard keeps, per ring slot, the events of the exports that read it and may still run: packs on the pack stream and
// device exports on callers' streams, which sit behind whatever the caller has enqueued there.  A step that writes the slot waits for
// all of them (mobi_exporter_guard); finished ones are dropped whenever the set is looked at.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/mobiclip_hip.h"
#include "mobi_export.h"
#include "mobi_exporter.h"

namespace {

// Staging: kChunks device chunks of kChunkBytes (256 MB of HBM), allocated at a batch's first export (batches that never export hold none).
// The chunk size is what counts: every chunk is one copy, and the copy engine loses a gap per copy (waiting for the pack's event).  Measured
// on one MI355X (tools/exp_export.py --export-only, 640x480 into mobi_host_alloc memory, ceiling 56.9 GB/s; profiles/export_staging_ab.jsonl):
// I420 / ARGB at 4 x 16 MB 49.2 / 49.4 GB/s, 8 x 16 MB 48.0 / 50.2, 4 x 32 MB 52.0 / 52.2, 8 x 32 MB 51.8 / 52.3, 2 x 64 MB 53.3 / 54.2,
// 4 x 64 MB 53.8 / 53.7.  More chunks buy nothing once the pack (tens of microseconds) is far ahead of the copy (1.2 ms per 64 MB);
// four rather than two leave the packs -- and so the ring-slot guard -- a little more room ahead of the copies.
constexpr int kChunks = 4;
constexpr size_t kChunkBytes = (size_t)64 << 20;

std::mutex g_reg_mutex;
std::map<uintptr_t, size_t> g_reg; // mobi_host_alloc blocks: start -> bytes

// has everything in front of event e completed?  1: yes, 0: still running, MOBI_E_DEVICE: the query failed.  No error stays with the
// thread (hipErrorNotReady would otherwise).
int event_done(hipEvent_t e) {
  const hipError_t q = hipEventQuery(e);
  if (q == hipSuccess) return 1;
  (void)hipGetLastError();
  return q == hipErrorNotReady ? 0 : MOBI_E_DEVICE;
}

} // namespace

bool mobi_host_registered(const void *p, size_t bytes) {
  const uintptr_t a = (uintptr_t)p;
  std::lock_guard<std::mutex> l(g_reg_mutex);
  auto it = g_reg.upper_bound(a);
  if (it == g_reg.begin()) return false;
  --it;
  return a - it->first <= it->second && bytes <= it->second - (a - it->first);
}

struct MobiExporter {
  int device = 0;
  int n_chunks = kChunks;
  size_t chunk_bytes = kChunkBytes;
  hipStream_t pack_s = nullptr, copy_s = nullptr;
  hipEvent_t ev_src = nullptr;
  std::vector<uint8_t *> stage, bounce;   // device staging chunks; pinned bounce chunks (destinations outside mobi_host_alloc blocks)
  std::vector<hipEvent_t> ev_packed, ev_copied;
  std::vector<bool> used;                 // staging chunk k has been copied from at least once (ev_copied[k] recorded)
  uint64_t next_chunk = 0;                // chunks issued so far: chunk i uses staging chunk i mod n_chunks
  std::vector<hipEvent_t> readers[6];     // the ring-slot guard: the exports that read slot s and may still be running
  uint64_t next_ticket = 1, retired = 0;  // tickets 1 .. next_ticket - 1 issued; 1 .. retired known to be complete
  std::deque<std::pair<uint64_t, hipEvent_t>> pending;
  std::vector<hipEvent_t> ev_pool;
  // parameter blocks: `bytes` of pinned host memory, as many of device memory, and the event behind the last launch that read the latter
  struct ParamBlock { void *host = nullptr, *dev = nullptr; size_t bytes = 0; hipEvent_t ev = nullptr; };
  std::vector<ParamBlock> params;

  // a block of at least `bytes` that no launch still reads (its event has completed), or a new one.  *out points into `params`: it holds
  // until the next take_params (a push_back moves the blocks), which is longer than mobi_exporter_run_device, its one caller, keeps it.
  // The pool grows by a block for every export enqueued while all are still in flight and does not shrink before the exporter goes.
  int take_params(size_t bytes, ParamBlock **out) {
    for (auto &pb : params) {
      if (pb.bytes < bytes) continue;
      const int done = event_done(pb.ev);
      if (done == 1) { *out = &pb; return MOBI_OK; }
      if (done != 0) return done;
    }
    ParamBlock pb;
    pb.bytes = std::max<size_t>(4096, bytes + bytes / 2); // (a caller whose batches grow a little finds room in the blocks it has)
    if (hipHostMalloc(&pb.host, pb.bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return MOBI_E_DEVICE; }
    if (hipMalloc(&pb.dev, pb.bytes) != hipSuccess || hipEventCreateWithFlags(&pb.ev, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      if (pb.dev) (void)hipFree(pb.dev);
      (void)hipHostFree(pb.host);
      return MOBI_E_DEVICE;
    }
    params.push_back(pb);
    *out = &params.back();
    return MOBI_OK;
  }

  int get_event(hipEvent_t *e) {
    if (!ev_pool.empty()) { *e = ev_pool.back(); ev_pool.pop_back(); return MOBI_OK; }
    return hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess ? MOBI_OK : MOBI_E_DEVICE;
  }
  // drop the events of slot s's readers that have finished (the set stays small: only exports still in flight are in it)
  int prune(int s) {
    auto &v = readers[s];
    for (size_t i = 0; i < v.size();) {
      const int done = event_done(v[i]);
      if (done == 1) { ev_pool.push_back(v[i]); v[i] = v.back(); v.pop_back(); continue; }
      if (done != 0) return done;
      i++;
    }
    return MOBI_OK;
  }
  // an export that reads slot s is enqueued on `stream`: a step that writes s waits for what is enqueued there now
  int arm(int s, hipStream_t stream) {
    if (int e = prune(s)) return e;
    hipEvent_t ev = nullptr;
    if (int e = get_event(&ev)) return e;
    if (hipEventRecord(ev, stream) != hipSuccess) { ev_pool.push_back(ev); return MOBI_E_DEVICE; }
    readers[s].push_back(ev);
    return MOBI_OK;
  }
  bool events_ready = false;              // init_events() went through
  int init_events() {
    if (events_ready) return MOBI_OK;
    if (!ev_src && hipEventCreateWithFlags(&ev_src, hipEventDisableTiming) != hipSuccess) { ev_src = nullptr; return MOBI_E_DEVICE; }
    events_ready = true;
    return MOBI_OK;
  }
  bool ready = false;                     // init_staging() went through (a failed one is not tried again: the batch's host exports are refused)
  int init_staging() {
    if (ready) return MOBI_OK;
    if (pack_s) return MOBI_E_DEVICE;
    if (int e = init_events()) return e;
#if defined(MOBI_PROFILING)
    if (const char *e = getenv("MOBI_EXPORT_CHUNKS")) n_chunks = std::max(2, atoi(e));          // (A/B of the staging size: tools/exp_export.py)
    if (const char *e = getenv("MOBI_EXPORT_CHUNK_MB")) chunk_bytes = (size_t)std::max(9, atoi(e)) << 20;
#endif
    // a chunk holds at least one picture: the largest the batch accepts is 1024 x 8191 macroblocks' worth of ARGB, 8.4 MB
    // Both export streams at the highest priority.  At normal priority they share the hardware queues of the batch's own streams (HIP hands
    // out a few queues per priority, round robin), and a pack or a copy queued behind a parse or reconstruction launch waited for all of it:
    // in a trace of tools/exp_export.py's end-to-end run the copy engine idled for the whole 295 ms parse of every next group and for 6 ms
    // of every part's reconstruction.  With queues of their own the pack starts at once (it still has to wait for room on the CUs the
    // parse fills): 28.3 -> 28.8 Gpixels/s end to end, alternating A/B on one box (profiles/export_e2e_trace.txt).
    int prio_lo = 0, prio_hi = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) { (void)hipGetLastError(); prio_hi = prio_lo = 0; }
#if defined(MOBI_PROFILING)
    if (getenv("MOBI_EXPORT_NORMAL_PRIORITY")) prio_hi = prio_lo; // (A/B: tools/exp_export.py)
#endif
    if (hipStreamCreateWithPriority(&pack_s, hipStreamNonBlocking, prio_hi) != hipSuccess) { pack_s = nullptr; return MOBI_E_DEVICE; }
    if (hipStreamCreateWithPriority(&copy_s, hipStreamNonBlocking, prio_hi) != hipSuccess) return MOBI_E_DEVICE;
    stage.assign(n_chunks, nullptr);
    ev_packed.assign(n_chunks, nullptr);
    ev_copied.assign(n_chunks, nullptr);
    used.assign(n_chunks, false);
    for (int k = 0; k < n_chunks; k++) {
      if (hipMalloc((void **)&stage[k], chunk_bytes) != hipSuccess) { stage[k] = nullptr; return MOBI_E_DEVICE; }
      if (hipEventCreateWithFlags(&ev_packed[k], hipEventDisableTiming) != hipSuccess) return MOBI_E_DEVICE;
      if (hipEventCreateWithFlags(&ev_copied[k], hipEventDisableTiming) != hipSuccess) return MOBI_E_DEVICE;
    }
    ready = true;
    return MOBI_OK;
  }
  int init_bounce() {
    if (!bounce.empty()) return MOBI_OK;
    std::vector<uint8_t *> b(n_chunks, nullptr);
    for (int k = 0; k < n_chunks; k++)
      if (hipHostMalloc((void **)&b[k], chunk_bytes, hipHostMallocDefault) != hipSuccess) {
        for (auto p : b) if (p) (void)hipHostFree(p);
        return MOBI_E_DEVICE;
      }
    bounce = b;
    return MOBI_OK;
  }
  void drain() {
    if (pack_s) (void)hipStreamSynchronize(pack_s);
    if (copy_s) (void)hipStreamSynchronize(copy_s);
  }
  void retire_upto(uint64_t t) {
    while (!pending.empty() && pending.front().first <= t) { ev_pool.push_back(pending.front().second); pending.pop_front(); }
    retired = std::max(retired, t);
  }
  ~MobiExporter() {
    (void)hipSetDevice(device);
    drain(); // the copies of outstanding exports still read the staging chunks and write the callers' memory
    for (auto &v : readers) // ... and device exports still read the ring, on the callers' streams
      for (auto e : v) { (void)hipEventSynchronize(e); (void)hipEventDestroy(e); }
    for (auto &pb : params) { // (behind the readers' events on their streams; a block whose launch failed to be enqueued may be behind none)
      (void)hipEventSynchronize(pb.ev);
      (void)hipEventDestroy(pb.ev);
      (void)hipFree(pb.dev);
      (void)hipHostFree(pb.host);
    }
    for (auto &p : pending) (void)hipEventDestroy(p.second);
    for (auto e : ev_pool) (void)hipEventDestroy(e);
    for (auto e : ev_packed) if (e) (void)hipEventDestroy(e);
    for (auto e : ev_copied) if (e) (void)hipEventDestroy(e);
    for (auto p : stage) if (p) (void)hipFree(p);
    for (auto p : bounce) if (p) (void)hipHostFree(p);
    if (ev_src) (void)hipEventDestroy(ev_src);
    if (pack_s) (void)hipStreamDestroy(pack_s);
    if (copy_s) (void)hipStreamDestroy(copy_s);
  }
};

namespace {
// Whatever fails once something of an export is enqueued: nothing of it may still run when the caller gets the error.  Unless disarmed,
// waits for the exporter's streams (x: a host export, which then issues no ticket) or for the caller's stream s (x == nullptr: a device export).
struct Drain {
  MobiExporter *x;
  hipStream_t s;
  bool armed = true;
  ~Drain() {
    if (!armed) return;
    if (x) x->drain();
    else (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
  }
};
} // namespace

MobiExporter *mobi_exporter_new(int device) {
  auto *x = new MobiExporter();
  x->device = device;
  return x;
}
void mobi_exporter_delete(MobiExporter *x) { delete x; }

int mobi_exporter_guard(MobiExporter *x, int slot, hipStream_t stream) {
  if (!x || x->readers[slot].empty()) return MOBI_OK;
  if (int e = x->prune(slot)) return e;
  for (hipEvent_t ev : x->readers[slot]) // (kept until they are seen finished: a later step may have to wait for them too)
    if (hipStreamWaitEvent(stream, ev, 0) != hipSuccess) return MOBI_E_DEVICE;
  return MOBI_OK;
}

bool mobi_exporter_busy(MobiExporter *x) {
  if (!x) return false;
  while (!x->pending.empty() && event_done(x->pending.front().second) == 1) x->retire_upto(x->pending.front().first);
  if (!x->pending.empty()) return true;
  for (int s = 0; s < 6; s++)
    if (x->prune(s) != MOBI_OK || !x->readers[s].empty()) return true; // (a query that failed: not known to be idle)
  return false;
}

int mobi_exporter_run(MobiExporter *x, const MobiExportJob &job, uint64_t *ticket_out) {
  if (int e = x->init_staging()) return e;
  // tickets nobody waits for or asks about: the ones already done give their events back (a caller that never waits holds at most the
  // exports still in flight)
  while (!x->pending.empty() && event_done(x->pending.front().second) == 1) x->retire_upto(x->pending.front().first);
  const MobiExportGeom &g = job.g;
  const size_t pic = job.format == MOBI_EXPORT_I420 ? (size_t)mobi_export_i420_bytes((uint32_t)g.width, (uint32_t)g.height)
                                                    : (size_t)g.width * g.height * 4;
  const uint64_t n_pics = (uint64_t)job.n_frames * job.n_clips;
  const uint64_t per_chunk = x->chunk_bytes / pic;
  if (per_chunk == 0) return MOBI_E_ARG;
  const uint64_t n_chunks = (n_pics + per_chunk - 1) / per_chunk;
  const bool pinned = mobi_host_registered(job.dst, n_pics * pic);
  if (!pinned)
    if (int e = x->init_bounce()) return e;
  uint8_t *dst = (uint8_t *)job.dst;
  Drain drain{x, nullptr};
  auto hip = [](hipError_t e) { return e == hipSuccess ? MOBI_OK : MOBI_E_DEVICE; };
  if (int e = hip(hipEventRecord(x->ev_src, job.src_stream))) return e; // the reconstruction of every frame exported is in front of this
  if (int e = hip(hipStreamWaitEvent(x->pack_s, x->ev_src, 0))) return e;
  // a destination outside the registry: chunk i is read out of bounce chunk i mod n by the host threads once its copy is done
  auto consume = [&](uint64_t i) -> int {
    const int k = (int)((x->next_chunk - n_chunks + i) % (uint64_t)x->n_chunks);
    if (int e = hip(hipEventSynchronize(x->ev_copied[k]))) return e;
    const uint64_t q0 = i * per_chunk, q1 = std::min(n_pics, q0 + per_chunk);
    const size_t bytes = (size_t)(q1 - q0) * pic, piece = (size_t)1 << 20;
    const uint8_t *src = x->bounce[k];
    uint8_t *d = dst + q0 * pic;
    job.run((int)((bytes + piece - 1) / piece), [&](int t) {
      const size_t a = (size_t)t * piece;
      memcpy(d + a, src + a, std::min(piece, bytes - a));
    });
    return MOBI_OK;
  };
  x->next_chunk += n_chunks; // (consume() counts back from here: chunk i of this export is chunk next_chunk - n_chunks + i overall)
  const uint64_t first = x->next_chunk - n_chunks;
  for (uint64_t i = 0; i < n_chunks; i++) {
    const int k = (int)((first + i) % (uint64_t)x->n_chunks);
    if (!pinned && i >= (uint64_t)x->n_chunks)
      if (int e = consume(i - x->n_chunks)) return e; // bounce chunk k is free again
    if (x->used[k])
      if (int e = hip(hipStreamWaitEvent(x->pack_s, x->ev_copied[k], 0))) return e;
    const uint64_t q0 = i * per_chunk, q1 = std::min(n_pics, q0 + per_chunk);
    uint8_t *st = x->stage[k];
    if (job.format == MOBI_EXPORT_I420) {
      if (mobi_launch_export_i420(&g, (uint32_t)q0, (int)(q1 - q0), job.n_clips, job.clip0, job.slot0, st, x->pack_s) != 0) return MOBI_E_DEVICE;
    } else {
      for (uint64_t q = q0; q < q1;) { // the Bitmap kernel converts clips of one slot: one launch per frame the chunk touches
        const uint64_t j = q / job.n_clips, c = q - j * job.n_clips, e = std::min(q1, (j + 1) * job.n_clips);
        if (job.argb(job.clip0 + (int)c, (int)(e - q), (int)((job.slot0 + j) % 6), (uint32_t *)(st + (q - q0) * pic), x->pack_s) != 0) return MOBI_E_DEVICE;
        q = e;
      }
    }
    if (int e = hip(hipEventRecord(x->ev_packed[k], x->pack_s))) return e;
    if (int e = hip(hipStreamWaitEvent(x->copy_s, x->ev_packed[k], 0))) return e;
    uint8_t *to = pinned ? dst + q0 * pic : x->bounce[k];
    if (int e = hip(hipMemcpyAsync(to, st, (size_t)(q1 - q0) * pic, hipMemcpyDeviceToHost, x->copy_s))) return e;
    if (int e = hip(hipEventRecord(x->ev_copied[k], x->copy_s))) return e;
    x->used[k] = true;
  }
  // the guard: a step that will write one of these slots waits for the packs that read it
  for (int j = 0; j < job.n_frames && j < 6; j++)
    if (int e = x->arm((job.slot0 + j) % 6, x->pack_s)) return e;
  if (!pinned) {
    for (uint64_t i = n_chunks > (uint64_t)x->n_chunks ? n_chunks - x->n_chunks : 0; i < n_chunks; i++)
      if (int e = consume(i)) return e;
    drain.armed = false;
    const uint64_t t = x->next_ticket++;
    x->retire_upto(t); // (the copy stream is in order: every earlier export is in its destination too)
    *ticket_out = t;
    return MOBI_OK;
  }
  hipEvent_t done = nullptr;
  if (int e = x->get_event(&done)) return e;
  if (hipEventRecord(done, x->copy_s) != hipSuccess) { x->ev_pool.push_back(done); return MOBI_E_DEVICE; }
  drain.armed = false;
  const uint64_t t = x->next_ticket++;
  x->pending.emplace_back(t, done);
  *ticket_out = t;
  return MOBI_OK;
}

int mobi_exporter_run_device(MobiExporter *x, const MobiExportJob &job, hipStream_t stream, const std::function<int(hipStream_t)> &launch,
                             MobiExportParams *params) {
  if (int e = x->init_events()) return e;
  MobiExporter::ParamBlock *pb = nullptr;
  if (params) { // (before anything is enqueued: a call that finds no block enqueues nothing)
    if (int e = x->take_params(params->bytes, &pb)) return e;
    memcpy(pb->host, params->host, params->bytes);
    params->dev = pb->dev;
  }
  Drain drain{nullptr, stream};
  if (hipEventRecord(x->ev_src, job.src_stream) != hipSuccess) { drain.armed = false; (void)hipGetLastError(); return MOBI_E_DEVICE; }
  if (hipStreamWaitEvent(stream, x->ev_src, 0) != hipSuccess) return MOBI_E_DEVICE; // the reconstruction of every frame exported is in front
  if (pb && hipMemcpyAsync(pb->dev, pb->host, params->bytes, hipMemcpyHostToDevice, stream) != hipSuccess) return MOBI_E_DEVICE;
  const int rc = launch(stream);
  // the block is free once the copy and the kernels behind it have run (also after a launch that failed half way: the drain is behind it)
  if (pb && hipEventRecord(pb->ev, stream) != hipSuccess) return MOBI_E_DEVICE;
  if (rc != 0) return MOBI_E_DEVICE;
  for (int j = 0; j < job.n_frames && j < 6; j++) // the guard: a step that will write one of these slots waits for these kernels
    if (int e = x->arm((job.slot0 + j) % 6, stream)) return e;
  drain.armed = false;
  return MOBI_OK;
}

int mobi_exporter_wait(MobiExporter *x, uint64_t ticket) {
  if (!x || ticket == 0 || ticket >= x->next_ticket) return MOBI_E_ARG;
  if (ticket <= x->retired) return MOBI_OK;
  for (auto &p : x->pending)
    if (p.first >= ticket) { // (the first pending ticket at or after this one: its event is behind this export's copies)
      if (hipEventSynchronize(p.second) != hipSuccess) { (void)hipGetLastError(); return MOBI_E_DEVICE; }
      x->retire_upto(p.first);
      return MOBI_OK;
    }
  return MOBI_E_DEVICE; // (not reached: every ticket above `retired` is pending)
}

int mobi_exporter_query(MobiExporter *x, uint64_t ticket) {
  if (!x || ticket == 0 || ticket >= x->next_ticket) return MOBI_E_ARG;
  if (ticket <= x->retired) return 1;
  for (auto &p : x->pending)
    if (p.first >= ticket) {
      const int done = event_done(p.second);
      if (done == 1) x->retire_upto(p.first);
      return done;
    }
  return MOBI_E_DEVICE;
}

extern "C" {

void *mobi_host_alloc(size_t bytes) {
  int ndev = 0;
  if (bytes == 0 || hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return nullptr;
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  std::lock_guard<std::mutex> l(g_reg_mutex);
  g_reg[(uintptr_t)p] = bytes;
  return p;
}

void mobi_host_free(void *p) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> l(g_reg_mutex);
    auto it = g_reg.find((uintptr_t)p);
    if (it == g_reg.end()) return; // not ours
    g_reg.erase(it);
  }
  (void)hipHostFree(p);
}

} // extern "C"
