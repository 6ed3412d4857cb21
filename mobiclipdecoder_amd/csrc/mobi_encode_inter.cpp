// mobi_encode_inter.cpp -- the C entry points of the inter encoder (include/mobiclip_encode_inter.h): the encoder object with everything
// the three stages (mobi_encode_inter.hip) need, allocated once; the refusals; the host-pointer twin.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>

#include "../../include/mobiclip_hip.h"
#include "mobi_encode_inter.h"

extern "C" int mobi_launch_encode_inter(const MobiEncInterArgs *a, int stages, hipStream_t s);

struct mobi_enc_inter_ctx {
  int max_pictures, version, device;
  uint32_t width, height;
  size_t frame, nmb;
  // one device allocation, carved: constants, macroblock records, bit offsets, vectors, predictors, fit flags, quantisers (previous, then
  // current), the reconstruction
  uint8_t *mem;
  MobiEncInterConst *k;
  MobiEncMb *mbs;
  uint32_t *mb_off, *mv, *mvp, *fits;
  uint8_t *q, *rec;
  // the host-pointer call's device copies, made at its first use and kept: pictures and references in, reconstruction, lengths,
  // statistics; the slots grow with the largest slot_bytes seen
  uint8_t *st_in, *st_ref, *st_rec, *st_streams;
  int32_t *st_bytes;
  mobi_enc_inter_stats *st_stats;
  size_t st_stream_bytes;
  hipStream_t st_stream;
};

namespace {
int g_stages = 7; // what the launch runs; only the profiling twin's hook below changes it (tools/exp_encode_inter.py)
size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
} // namespace

#if defined(MOBI_PROFILING)
extern "C" __attribute__((visibility("default"))) void mobi_debug_encp_select(int stages) { g_stages = stages; }
#endif

size_t mobi_enc_inter_stream_bound(uint32_t width, uint32_t height) { return mobi_encp_bound(width, height); }

int mobi_enc_inter_check(int max_pictures, uint32_t width, uint32_t height, int version, int n, size_t picture_pitch, size_t ref_pitch,
                         const uint8_t *prev_quantizers, const uint8_t *quantizers, size_t slot_bytes) {
  return mobi_encp_check_args(max_pictures, width, height, version, n, picture_pitch, ref_pitch, prev_quantizers, quantizers, slot_bytes);
}

mobi_enc_inter_ctx *mobi_enc_inter_create(int max_pictures, uint32_t width, uint32_t height, int version, int device) {
  const uint8_t q = MOBI_ENC_QMIN;
  const size_t frame = (size_t)width * height * 3 / 2;
  if (device < 0 || max_pictures < 1 || mobi_encp_check_args(max_pictures, width, height, version, 1, frame, frame, &q, &q, 0) != MOBI_OK) return nullptr;
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  mobi_enc_inter_ctx *e = (mobi_enc_inter_ctx *)calloc(1, sizeof *e);
  if (!e) return nullptr;
  e->max_pictures = max_pictures;
  e->version = version;
  e->device = device;
  e->width = width;
  e->height = height;
  e->frame = frame;
  e->nmb = (size_t)(width / 16) * (height / 16);
  const size_t N = (size_t)max_pictures, cells = up(N * e->nmb * 4);
  const size_t o_mbs = up(sizeof(MobiEncInterConst)), o_off = o_mbs + up(N * e->nmb * sizeof(MobiEncMb)), o_mv = o_off + cells, o_mvp = o_mv + cells,
               o_fits = o_mvp + cells, o_q = o_fits + up(N * 4), o_rec = o_q + up(2 * N), total = o_rec + up(N * e->frame);
  MobiEncInterConst *h = new MobiEncInterConst;
  mobi_encp_build_const(h);
  const bool ok = hipMalloc((void **)&e->mem, total) == hipSuccess && hipMemcpy(e->mem, h, sizeof *h, hipMemcpyHostToDevice) == hipSuccess;
  delete h;
  if (!ok) {
    mobi_enc_inter_destroy(e);
    return nullptr;
  }
  e->k = (MobiEncInterConst *)e->mem;
  e->mbs = (MobiEncMb *)(e->mem + o_mbs);
  e->mb_off = (uint32_t *)(e->mem + o_off);
  e->mv = (uint32_t *)(e->mem + o_mv);
  e->mvp = (uint32_t *)(e->mem + o_mvp);
  e->fits = (uint32_t *)(e->mem + o_fits);
  e->q = e->mem + o_q;
  e->rec = e->mem + o_rec;
  return e;
}

void mobi_enc_inter_destroy(mobi_enc_inter_ctx *e) {
  if (!e) return;
  if (e->st_stream) (void)hipStreamDestroy(e->st_stream);
  for (void *p : {(void *)e->mem, (void *)e->st_in, (void *)e->st_ref, (void *)e->st_rec, (void *)e->st_streams, (void *)e->st_bytes, (void *)e->st_stats})
    if (p) (void)hipFree(p);
  free(e);
}

int mobi_enc_inter_async(mobi_enc_inter_ctx *e, void *stream, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *ref_i420,
                         size_t ref_pitch, const uint8_t *prev_quantizers, const uint8_t *quantizers, uint8_t *streams, size_t slot_bytes,
                         int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_inter_stats *stats) {
  if (!e) return MOBI_E_ARG;
  const int rc = mobi_encp_check_args(e->max_pictures, e->width, e->height, e->version, n, picture_pitch, ref_pitch, prev_quantizers, quantizers, slot_bytes);
  if (rc != MOBI_OK) return rc;
  // the kernels read pictures 8 bytes, references 4 bytes and write reconstruction 8 and slots 4 bytes at a time
  if (!i420 || !ref_i420 || !streams || !bytes_out || (uintptr_t)i420 % 8 || (uintptr_t)ref_i420 % 8 || (uintptr_t)streams % 4 || (uintptr_t)recon_i420 % 8 ||
      (uintptr_t)bytes_out % 4 || (uintptr_t)stats % 8)
    return MOBI_E_ARG;
  if (hipSetDevice(e->device) != hipSuccess) return MOBI_E_DEVICE;
  hipStream_t s = (hipStream_t)stream;
  const size_t N = (size_t)e->max_pictures;
  // (pageable sources: the copies have left both arrays when the call returns)
  if (hipMemcpyAsync(e->q, prev_quantizers, (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(e->q + N, quantizers, (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess)
    return MOBI_E_DEVICE;
  if (slot_bytes && hipMemsetAsync(streams, 0, (size_t)n * slot_bytes, s) != hipSuccess) return MOBI_E_DEVICE;
  if (stats && hipMemsetAsync(stats, 0, (size_t)n * sizeof *stats, s) != hipSuccess) return MOBI_E_DEVICE;
  MobiEncInterArgs a;
  memset((void *)&a, 0, sizeof a);
  a.src = i420;
  a.src_pitch = picture_pitch;
  a.rec = recon_i420 ? recon_i420 : e->rec;
  a.mbs = e->mbs;
  a.mb_off = e->mb_off;
  a.fits = e->fits;
  a.q = e->q + N;
  a.k = e->k;
  a.streams = streams;
  a.slot_bytes = slot_bytes;
  a.bytes_out = bytes_out;
  a.W = (int32_t)e->width;
  a.H = (int32_t)e->height;
  a.mbw = (int32_t)(e->width / 16);
  a.mbh = (int32_t)(e->height / 16);
  a.n = n;
  a.ref = ref_i420;
  a.ref_pitch = ref_pitch;
  a.prev_q = e->q;
  a.mv = e->mv;
  a.mvp = e->mvp;
  a.kp = e->k;
  a.pstats = stats;
  a.ver = mobi_encp_ver(e->version);
  return mobi_launch_encode_inter(&a, g_stages, s) == 0 ? MOBI_OK : MOBI_E_DEVICE;
}

int mobi_enc_inter(mobi_enc_inter_ctx *e, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *ref_i420, size_t ref_pitch,
                   const uint8_t *prev_quantizers, const uint8_t *quantizers, uint8_t *streams, size_t slot_bytes, int32_t *bytes_out,
                   uint8_t *recon_i420, mobi_enc_inter_stats *stats) {
  if (!e) return MOBI_E_ARG;
  int rc = mobi_encp_check_args(e->max_pictures, e->width, e->height, e->version, n, picture_pitch, ref_pitch, prev_quantizers, quantizers, slot_bytes);
  if (rc != MOBI_OK) return rc;
  if (!i420 || !ref_i420 || !streams || !bytes_out) return MOBI_E_ARG;
  if (hipSetDevice(e->device) != hipSuccess) return MOBI_E_DEVICE;
  const size_t N = (size_t)e->max_pictures;
  if (!e->st_in) {
    if (hipMalloc((void **)&e->st_in, N * e->frame) != hipSuccess || hipMalloc((void **)&e->st_ref, N * e->frame) != hipSuccess ||
        hipMalloc((void **)&e->st_rec, N * e->frame) != hipSuccess || hipMalloc((void **)&e->st_bytes, N * 4) != hipSuccess ||
        hipMalloc((void **)&e->st_stats, N * sizeof(mobi_enc_inter_stats)) != hipSuccess ||
        hipStreamCreateWithFlags(&e->st_stream, hipStreamNonBlocking) != hipSuccess)
      return MOBI_E_DEVICE;
  }
  if (N * slot_bytes > e->st_stream_bytes) {
    if (e->st_streams) (void)hipFree(e->st_streams);
    e->st_streams = nullptr;
    e->st_stream_bytes = 0;
    if (hipMalloc((void **)&e->st_streams, N * slot_bytes) != hipSuccess) return MOBI_E_DEVICE;
    e->st_stream_bytes = N * slot_bytes;
  }
  uint8_t *d_streams = e->st_streams ? e->st_streams : e->st_in; // slot_bytes == 0: nothing is written there
  hipStream_t s = e->st_stream;
  if (hipMemcpy2DAsync(e->st_in, e->frame, i420, picture_pitch, e->frame, (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpy2DAsync(e->st_ref, e->frame, ref_i420, ref_pitch, e->frame, (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess)
    return MOBI_E_DEVICE;
  rc = mobi_enc_inter_async(e, s, n, e->st_in, e->frame, e->st_ref, e->frame, prev_quantizers, quantizers, d_streams, slot_bytes, e->st_bytes, e->st_rec,
                            e->st_stats);
  if (rc == MOBI_OK &&
      ((slot_bytes && hipMemcpyAsync(streams, d_streams, (size_t)n * slot_bytes, hipMemcpyDeviceToHost, s) != hipSuccess) ||
       hipMemcpyAsync(bytes_out, e->st_bytes, (size_t)n * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
       (recon_i420 && hipMemcpyAsync(recon_i420, e->st_rec, (size_t)n * e->frame, hipMemcpyDeviceToHost, s) != hipSuccess) ||
       (stats && hipMemcpyAsync(stats, e->st_stats, (size_t)n * sizeof *stats, hipMemcpyDeviceToHost, s) != hipSuccess)))
    rc = MOBI_E_DEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = MOBI_E_DEVICE;
  return rc;
}
