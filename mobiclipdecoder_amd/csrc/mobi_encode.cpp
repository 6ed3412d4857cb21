// mobi_encode.cpp -- the C entry points of the intra encoder (include/mobiclip_encode.h): the refusals, and the launch of stage 1 and stage 2
// (mobi_encode.hip), and the intra encoder's call with byte targets (include/mobiclip_encode_rate.h).  The encoder object, the prologue
// of the call, the loop of the target call and the host-pointer twin are mobi_encode_ctx.h's.
#include "mobi_encode_ctx.h"

extern "C" int mobi_launch_encode(const MobiEncArgs *a, int stages, int loop_shape, hipStream_t s);

struct mobi_enc : MobiEncCtx {};

namespace {
int g_stages = 7, g_loop_shape = 0; // what the launch runs; only the profiling twin's hook below changes them (tools/exp_encode.py)
} // namespace

#if defined(MOBI_PROFILING)
extern "C" __attribute__((visibility("default"))) void mobi_debug_enc_select(int stages, int loop_shape) {
  g_stages = stages;
  g_loop_shape = loop_shape;
}
#endif

size_t mobi_enc_stream_bound(uint32_t width, uint32_t height) { return mobi_enc_bound(width, height); }

int mobi_enc_check(int max_pictures, uint32_t width, uint32_t height, int version, int n, size_t picture_pitch, const uint8_t *quantizers,
                   int yuv_format, size_t slot_bytes) {
  return mobi_enc_check_args(max_pictures, width, height, version, n, picture_pitch, quantizers, yuv_format, slot_bytes);
}

mobi_enc *mobi_enc_create(int max_pictures, uint32_t width, uint32_t height, int version, int device) {
  const uint8_t q = MOBI_ENC_QMIN;
  if (device < 0 || max_pictures < 1 ||
      mobi_enc_check_args(max_pictures, width, height, version, 1, (size_t)width * height * 3 / 2, &q, 0, 0) != MOBI_OK)
    return nullptr;
  mobi_enc *e = mobi_enc_ctx_new<mobi_enc>(max_pictures, width, height, version, device);
  return e && mobi_enc_ctx_carve(e, mobi_enc_build_const, 1, {}) ? e : nullptr;
}

void mobi_enc_destroy(mobi_enc *e) { mobi_enc_ctx_destroy(e); }

int mobi_enc_intra_async(mobi_enc *e, void *stream, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *quantizers, int yuv_format,
                         uint8_t *streams, size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_stats *stats) {
  if (!e) return MOBI_E_ARG;
  int rc = mobi_enc_check_args(e->max_pictures, e->width, e->height, e->version, n, picture_pitch, quantizers, yuv_format, slot_bytes);
  if (rc != MOBI_OK) return rc;
  // the kernels read pictures 8 bytes and write reconstruction and slots 4 bytes at a time
  if (!i420 || !streams || !bytes_out || (uintptr_t)i420 % 8 || (uintptr_t)streams % 4 || (uintptr_t)recon_i420 % 4 || (uintptr_t)bytes_out % 4 ||
      (uintptr_t)stats % 8)
    return MOBI_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  MobiEncArgs a;
  memset(&a, 0, sizeof a);
  rc = mobi_enc_ctx_begin(e, s, n, i420, picture_pitch, {quantizers}, streams, slot_bytes, bytes_out, recon_i420, stats, &a);
  if (rc != MOBI_OK) return rc;
  a.stats = stats;
  a.yuv_format = yuv_format;
  return mobi_launch_encode(&a, g_stages, g_loop_shape, s) == 0 ? MOBI_OK : MOBI_E_DEVICE;
}

int mobi_enc_rate_rounds(int qmin, int qmax) { return mobi_enc_rate_rounds_of(qmin, qmax); }

int mobi_enc_intra_target_async(mobi_enc *e, void *stream, int n, const uint8_t *i420, size_t picture_pitch, const int32_t *target_bytes, int qmin,
                                int qmax, int yuv_format, uint8_t *streams, size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420,
                                mobi_enc_stats *stats, uint8_t *quantizers_out) {
  if (!e) return MOBI_E_ARG;
  const uint8_t q1 = MOBI_ENC_QMIN; // the quantisers are made on the device: the check sees one that passes
  int rc = mobi_enc_check_args(e->max_pictures, e->width, e->height, e->version, 1, picture_pitch, &q1, yuv_format, slot_bytes);
  if (rc != MOBI_OK) return rc;
  if (n < 1 || n > e->max_pictures || mobi_enc_rate_check_args(target_bytes, qmin, qmax, quantizers_out) != 0) return MOBI_E_ARG;
  if (!i420 || !streams || !bytes_out || (uintptr_t)i420 % 8 || (uintptr_t)streams % 4 || (uintptr_t)recon_i420 % 4 || (uintptr_t)bytes_out % 4 ||
      (uintptr_t)stats % 8)
    return MOBI_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  MobiEncArgs a;
  memset(&a, 0, sizeof a);
  rc = mobi_enc_ctx_begin(e, s, n, i420, picture_pitch, {}, streams, slot_bytes, bytes_out, recon_i420, stats, &a);
  if (rc != MOBI_OK) return rc;
  a.q = e->q;
  a.stats = stats;
  a.yuv_format = yuv_format;
  // a trial: decide and scan; the profiling twin's stage switch holds for the final encode alone
  return mobi_enc_ctx_rate(e, s, n, target_bytes, qmin, qmax, nullptr, nullptr, e->q, quantizers_out, bytes_out, stats, 3, g_stages,
                           [&](int stages) { return mobi_launch_encode(&a, stages, g_loop_shape, s); });
}

int mobi_enc_intra(mobi_enc *e, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *quantizers, int yuv_format, uint8_t *streams,
                   size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_stats *stats) {
  if (!e) return MOBI_E_ARG;
  const int rc = mobi_enc_check_args(e->max_pictures, e->width, e->height, e->version, n, picture_pitch, quantizers, yuv_format, slot_bytes);
  if (rc != MOBI_OK) return rc;
  if (!i420 || !streams || !bytes_out) return MOBI_E_ARG;
  return mobi_enc_ctx_host(e, n, i420, picture_pitch, streams, slot_bytes, bytes_out, recon_i420, stats, [&](hipStream_t s, uint8_t *d_streams) {
    return mobi_enc_intra_async(e, s, n, e->st_in, e->frame, quantizers, yuv_format, d_streams, slot_bytes, (int32_t *)e->st_bytes, e->st_rec,
                                (mobi_enc_stats *)e->st_stats);
  });
}
