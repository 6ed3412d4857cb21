// mobi_encode_ctx.h -- HOST ONLY: what the entry points of the two encoders (mobi_encode.cpp, mobi_encode_inter.cpp) share, once: the
// common part of the encoder object, the carve of its one device allocation, destroy, the prologue of an _async call (device, quantiser
// rows, zeroed outputs, the MobiEncArgs base) and the host-pointer twin (staging made at first use, kept and grown; the copies back).
// The refusals and the alignment rules stay with each entry point: they differ.  mobi_enc_ctx_rate is the loop of the two _target_async
// calls (include/mobiclip_encode_rate.h): the rate rule's kernels around the encoder's own launches.
#ifndef MOBI_ENCODE_CTX_H
#define MOBI_ENCODE_CTX_H
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/mobiclip_hip.h"
#include "mobi_encode_rate.h"

extern "C" int mobi_launch_rate_begin(const MobiEncRateArgs *a, int rounds, hipStream_t s);
extern "C" int mobi_launch_rate_step(const MobiEncRateArgs *a, int last, hipStream_t s);

enum { MOBI_ENC_STATS_BYTES = 64 }; // either encoder's statistics record: zeroed and staged as bytes
static_assert(sizeof(mobi_enc_stats) == MOBI_ENC_STATS_BYTES && sizeof(mobi_enc_inter_stats) == MOBI_ENC_STATS_BYTES, "a statistics record is 64 bytes");

struct MobiEncCtx {
  int max_pictures, version, device;
  uint32_t width, height;
  size_t frame, nmb;
  // one device allocation, carved: the constants at its start, then macroblock records, bit offsets, what the encoder adds, fit flags,
  // quantiser rows (the pictures' own quantisers are the last row), the reconstruction
  uint8_t *mem;
  MobiEncMb *mbs;
  uint32_t *mb_off, *fits;
  uint8_t *q, *rec;
  // the rate rule's state between its rounds, an allocation of its own made at create: a row of lo, a row of hi
  uint8_t *rate;
  // the host-pointer call's device copies, made at its first use and kept: pictures in, reconstruction, lengths, statistics; the slots
  // grow with the largest slot_bytes seen
  uint8_t *st_in, *st_rec, *st_streams, *st_bytes, *st_stats;
  size_t st_stream_bytes;
  hipStream_t st_stream;
};

inline void mobi_enc_ctx_destroy(MobiEncCtx *e) {
  if (!e) return;
  if (e->st_stream) (void)hipStreamDestroy(e->st_stream);
  for (void *p : {(void *)e->mem, (void *)e->rate, (void *)e->st_in, (void *)e->st_rec, (void *)e->st_streams, (void *)e->st_bytes, (void *)e->st_stats})
    if (p) (void)hipFree(p);
  free(e);
}

// a zeroed encoder object of type Ctx (MobiEncCtx or plain data derived from it) with its dimensions, on `device`; the caller has checked them
template <class Ctx>
Ctx *mobi_enc_ctx_new(int max_pictures, uint32_t width, uint32_t height, int version, int device) {
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  Ctx *e = (Ctx *)calloc(1, sizeof *e);
  if (!e) return nullptr;
  e->max_pictures = max_pictures;
  e->version = version;
  e->device = device;
  e->width = width;
  e->height = height;
  e->frame = (size_t)width * height * 3 / 2;
  e->nmb = (size_t)(width / 16) * (height / 16);
  return e;
}

struct MobiEncPart { // one part of the carve: the pointer that receives its address, its size
  void *at;
  size_t bytes;
};
// the one allocation: the constants `build` makes, uploaded; the common parts with q_rows quantiser rows, `more` behind the bit offsets;
// each at a multiple of 256 bytes.  On failure the object is destroyed and the answer is false.
template <class Const>
bool mobi_enc_ctx_carve(MobiEncCtx *e, void (*build)(Const *), int q_rows, std::initializer_list<MobiEncPart> more) {
  const size_t N = (size_t)e->max_pictures;
  std::vector<MobiEncPart> parts = {{&e->mbs, N * e->nmb * sizeof(MobiEncMb)}, {&e->mb_off, N * e->nmb * 4}};
  parts.insert(parts.end(), more);
  parts.insert(parts.end(), {{&e->fits, N * 4}, {&e->q, (size_t)q_rows * N}, {&e->rec, N * e->frame}});
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  size_t total = up(sizeof(Const));
  for (const MobiEncPart &p : parts) total += up(p.bytes);
  Const *h = new Const;
  build(h);
  const bool ok = hipMalloc((void **)&e->mem, total) == hipSuccess && hipMemcpy(e->mem, h, sizeof *h, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMalloc((void **)&e->rate, 2 * N) == hipSuccess;
  delete h;
  if (!ok) {
    mobi_enc_ctx_destroy(e);
    return false;
  }
  uint8_t *at = e->mem + up(sizeof(Const));
  for (const MobiEncPart &p : parts) {
    memcpy(p.at, &at, sizeof at);
    at += up(p.bytes);
  }
  return true;
}

// What an _async call does once its arguments are accepted: the device; the quantiser rows (pageable sources: the copies have left the
// arrays when the call returns); slots and statistics zeroed; the launch arguments both encoders read.  q_rows[r] holds n quantisers.
inline int mobi_enc_ctx_begin(const MobiEncCtx *e, hipStream_t s, int n, const uint8_t *i420, size_t picture_pitch, std::initializer_list<const uint8_t *> q_rows,
                              uint8_t *streams, size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420, void *stats, MobiEncArgs *a) {
  if (hipSetDevice(e->device) != hipSuccess) return MOBI_E_DEVICE;
  const size_t N = (size_t)e->max_pictures;
  uint8_t *q = e->q;
  for (const uint8_t *row : q_rows) {
    if (hipMemcpyAsync(q, row, (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess) return MOBI_E_DEVICE;
    q += N;
  }
  if (slot_bytes && hipMemsetAsync(streams, 0, (size_t)n * slot_bytes, s) != hipSuccess) return MOBI_E_DEVICE;
  if (stats && hipMemsetAsync(stats, 0, (size_t)n * MOBI_ENC_STATS_BYTES, s) != hipSuccess) return MOBI_E_DEVICE;
  a->src = i420;
  a->src_pitch = picture_pitch;
  a->rec = recon_i420 ? recon_i420 : e->rec;
  a->mbs = e->mbs;
  a->mb_off = e->mb_off;
  a->fits = e->fits;
  a->q = q - N;
  a->k = (const MobiEncConst *)e->mem;
  a->streams = streams;
  a->slot_bytes = slot_bytes;
  a->bytes_out = bytes_out;
  a->W = (int32_t)e->width;
  a->H = (int32_t)e->height;
  a->mbw = (int32_t)(e->width / 16);
  a->mbh = (int32_t)(e->height / 16);
  a->n = n;
  return MOBI_OK;
}

// The loop of a _target_async call behind mobi_enc_ctx_begin (called with no quantiser rows: they are made here, on the device).
// launch(stages) enqueues the encoder's stage kernels and answers 0; `trial` is its stages up to and including the scan -- no slot is
// written or zeroed --, `whole` the frame's.  prev_in / prev_row: the inter encoder's previous quantisers, the caller's and the
// encoder's row (NULL for I-frames); q_row: the row the stage kernels read.  Everything is enqueued on s; the host reads no device value.
template <class Launch>
int mobi_enc_ctx_rate(const MobiEncCtx *e, hipStream_t s, int n, const int32_t *target_bytes, int qmin, int qmax, const uint8_t *prev_in, uint8_t *prev_row,
                      uint8_t *q_row, uint8_t *quantizers_out, const int32_t *bytes_out, void *stats, int trial, int whole, Launch launch) {
  MobiEncRateArgs r;
  memset(&r, 0, sizeof r);
  r.target = target_bytes;
  r.prev_in = prev_in;
  r.prev_q = prev_row;
  r.q = q_row;
  r.lo = e->rate;
  r.hi = e->rate + (size_t)e->max_pictures;
  r.q_out = quantizers_out;
  r.bytes = bytes_out;
  r.stats = (uint64_t *)stats;
  r.n = n;
  r.qmin = qmin;
  r.qmax = qmax;
  const int rounds = mobi_enc_rate_rounds_of(qmin, qmax);
  if (mobi_launch_rate_begin(&r, rounds, s) != 0) return MOBI_E_DEVICE;
  for (int k = 0; k < rounds; k++)
    if (launch(trial) != 0 || mobi_launch_rate_step(&r, k == rounds - 1, s) != 0) return MOBI_E_DEVICE;
  return launch(whole) == 0 ? MOBI_OK : MOBI_E_DEVICE;
}

// The host-pointer twin of an _async call, its arguments accepted: the pictures up into st_in, `call(stream, slots)` -- the encoder's
// further uploads and its _async call on the st_* copies --, the outputs asked for back, all of it waited for.
inline bool mobi_enc_ctx_need(uint8_t **p, size_t bytes) { return *p || hipMalloc((void **)p, bytes) == hipSuccess; }
template <class Call>
int mobi_enc_ctx_host(MobiEncCtx *e, int n, const uint8_t *i420, size_t picture_pitch, uint8_t *streams, size_t slot_bytes, int32_t *bytes_out,
                      uint8_t *recon_i420, void *stats, Call call) {
  if (hipSetDevice(e->device) != hipSuccess) return MOBI_E_DEVICE;
  const size_t N = (size_t)e->max_pictures;
  if (!mobi_enc_ctx_need(&e->st_in, N * e->frame) || !mobi_enc_ctx_need(&e->st_rec, N * e->frame) || !mobi_enc_ctx_need(&e->st_bytes, N * 4) ||
      !mobi_enc_ctx_need(&e->st_stats, N * MOBI_ENC_STATS_BYTES) ||
      (!e->st_stream && hipStreamCreateWithFlags(&e->st_stream, hipStreamNonBlocking) != hipSuccess))
    return MOBI_E_DEVICE;
  if (N * slot_bytes > e->st_stream_bytes) {
    if (e->st_streams) (void)hipFree(e->st_streams);
    e->st_streams = nullptr;
    e->st_stream_bytes = 0;
    if (hipMalloc((void **)&e->st_streams, N * slot_bytes) != hipSuccess) return MOBI_E_DEVICE;
    e->st_stream_bytes = N * slot_bytes;
  }
  uint8_t *d_streams = e->st_streams ? e->st_streams : e->st_in; // slot_bytes == 0: nothing is written there
  hipStream_t s = e->st_stream;
  if (hipMemcpy2DAsync(e->st_in, e->frame, i420, picture_pitch, e->frame, (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess) return MOBI_E_DEVICE;
  int rc = call(s, d_streams);
  if (rc == MOBI_OK &&
      ((slot_bytes && hipMemcpyAsync(streams, d_streams, (size_t)n * slot_bytes, hipMemcpyDeviceToHost, s) != hipSuccess) ||
       hipMemcpyAsync(bytes_out, e->st_bytes, (size_t)n * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
       (recon_i420 && hipMemcpyAsync(recon_i420, e->st_rec, (size_t)n * e->frame, hipMemcpyDeviceToHost, s) != hipSuccess) ||
       (stats && hipMemcpyAsync(stats, e->st_stats, (size_t)n * MOBI_ENC_STATS_BYTES, hipMemcpyDeviceToHost, s) != hipSuccess)))
    rc = MOBI_E_DEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = MOBI_E_DEVICE;
  return rc;
}
#endif
