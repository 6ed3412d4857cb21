// mobi_encode_inter.cpp -- the C entry points of the inter encoder (include/mobiclip_encode_inter.h) and of its partition mode
// (include/mobiclip_encode_parts.h) and of its intra mode (include/mobiclip_encode_pintra.h): the refusals, and the launch of the stages
// (mobi_encode_inter.hip; in partition mode 1 mobi_encode_parts.hip; in intra mode 1 two more stages, mobi_encode_pintra.hip), and the inter encoder's call with byte targets (include/mobiclip_encode_rate.h).  The encoder object, the
// prologue of the call, the loop of the target call and the host-pointer twin are mobi_encode_ctx.h's; this encoder adds the vectors and their predictors, the previous frames' quantiser row and the staged references.
#include "mobi_encode_ctx.h"
#include "mobi_encode_parts.h"
#include "mobi_encode_pintra.h"

extern "C" int mobi_launch_encode_inter(const MobiEncInterArgs *a, int stages, hipStream_t s);
extern "C" int mobi_launch_encode_parts(const MobiEncPartsArgs *a, int stages, hipStream_t s);

struct mobi_enc_inter_ctx : MobiEncCtx {
  uint32_t *mv, *mvp; // carved with the rest
  uint32_t *mv4;      // ... and the quadrants' vectors of mode 1
  int partitions;     // the mode: 0 after create
  int64_t *jp;        // the intra mode's side arrays, carved in every mode: a cost ...
  uint32_t *kind;     // ... and a kind word per macroblock
  int intra;          // that mode: 0 after create; never on together with partitions
  uint8_t *st_ref;    // the host-pointer call's copy of the references
};

namespace {
enum { BASE_STAGES = 15,           // search, code, scan, write
       PINTRA_STAGES = 16 | 32 };  // decide and finish: what the intra mode adds to a frame and to a trial
int g_stages = BASE_STAGES | PINTRA_STAGES; // what the launch runs; only the profiling twin's hook below changes it (tools/exp_encode_inter.py)

// the launch of a call's stages in the encoder's mode: the intra mode's two stages run in that mode alone
int launch(const mobi_enc_inter_ctx *e, const MobiEncPartsArgs *a, int stages, hipStream_t s) {
  if (e->partitions) return mobi_launch_encode_parts(a, stages & BASE_STAGES, s);
  return mobi_launch_encode_inter(a, e->intra ? stages : stages & BASE_STAGES, s);
}
// what both calls add to mobi_enc_ctx_begin's arguments
void inter_args(const mobi_enc_inter_ctx *e, const uint8_t *ref_i420, size_t ref_pitch, mobi_enc_inter_stats *stats, MobiEncPartsArgs *a) {
  a->ref = ref_i420;
  a->ref_pitch = ref_pitch;
  a->prev_q = e->q;
  a->mv = e->mv;
  a->mvp = e->mvp;
  a->kp = (const MobiEncInterConst *)e->mem;
  a->pstats = stats;
  a->ver = mobi_encp_ver(e->version);
  a->jp = e->jp;
  a->kind = e->kind;
  a->mv4 = e->mv4;
  a->kq = (const MobiEncPartsConst *)e->mem;
}
} // namespace

#if defined(MOBI_PROFILING)
extern "C" __attribute__((visibility("default"))) void mobi_debug_encp_select(int stages) { g_stages = stages; }
#endif

size_t mobi_enc_inter_stream_bound(uint32_t width, uint32_t height) { return mobi_encp_bound(width, height); }
size_t mobi_enc_inter_stream_bound_partitions(uint32_t width, uint32_t height, int mode) { return mobi_encq_bound(width, height, mode); }

int mobi_enc_inter_set_partitions(mobi_enc_inter_ctx *e, int mode) {
  return e ? mobi_encpi_set_mode(&e->partitions, e->intra, mode) : MOBI_E_ARG;
}
int mobi_enc_inter_get_partitions(const mobi_enc_inter_ctx *e) { return e ? e->partitions : MOBI_E_ARG; }

int mobi_enc_inter_set_intra(mobi_enc_inter_ctx *e, int mode) {
  return e ? mobi_encpi_set_mode(&e->intra, e->partitions, mode) : MOBI_E_ARG;
}
int mobi_enc_inter_get_intra(const mobi_enc_inter_ctx *e) { return e ? e->intra : MOBI_E_ARG; }

int mobi_enc_inter_check(int max_pictures, uint32_t width, uint32_t height, int version, int n, size_t picture_pitch, size_t ref_pitch,
                         const uint8_t *prev_quantizers, const uint8_t *quantizers, size_t slot_bytes) {
  return mobi_encp_check_args(max_pictures, width, height, version, n, picture_pitch, ref_pitch, prev_quantizers, quantizers, slot_bytes);
}

mobi_enc_inter_ctx *mobi_enc_inter_create(int max_pictures, uint32_t width, uint32_t height, int version, int device) {
  const uint8_t q = MOBI_ENC_QMIN;
  const size_t frame = (size_t)width * height * 3 / 2;
  if (device < 0 || max_pictures < 1 || mobi_encp_check_args(max_pictures, width, height, version, 1, frame, frame, &q, &q, 0) != MOBI_OK) return nullptr;
  mobi_enc_inter_ctx *e = mobi_enc_ctx_new<mobi_enc_inter_ctx>(max_pictures, width, height, version, device);
  if (!e) return nullptr;
  const size_t cells = (size_t)max_pictures * e->nmb * 4;
  // the constants of mode 1 begin with those of mode 0; quantiser rows: previous, current
  return mobi_enc_ctx_carve(e, mobi_encq_build_const, 2, {{&e->mv, cells}, {&e->mvp, cells}, {&e->mv4, 4 * cells}, {&e->jp, 2 * cells}, {&e->kind, cells}}) ? e : nullptr;
}

void mobi_enc_inter_destroy(mobi_enc_inter_ctx *e) {
  if (e && e->st_ref) (void)hipFree(e->st_ref);
  mobi_enc_ctx_destroy(e);
}

int mobi_enc_inter_async(mobi_enc_inter_ctx *e, void *stream, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *ref_i420,
                         size_t ref_pitch, const uint8_t *prev_quantizers, const uint8_t *quantizers, uint8_t *streams, size_t slot_bytes,
                         int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_inter_stats *stats) {
  if (!e) return MOBI_E_ARG;
  int rc = mobi_encp_check_args(e->max_pictures, e->width, e->height, e->version, n, picture_pitch, ref_pitch, prev_quantizers, quantizers, slot_bytes);
  if (rc != MOBI_OK) return rc;
  // the kernels read pictures 8 bytes, references 4 bytes and write reconstruction 8 and slots 4 bytes at a time
  if (!i420 || !ref_i420 || !streams || !bytes_out || (uintptr_t)i420 % 8 || (uintptr_t)ref_i420 % 8 || (uintptr_t)streams % 4 || (uintptr_t)recon_i420 % 8 ||
      (uintptr_t)bytes_out % 4 || (uintptr_t)stats % 8)
    return MOBI_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  MobiEncPartsArgs a;
  memset((void *)&a, 0, sizeof a);
  rc = mobi_enc_ctx_begin(e, s, n, i420, picture_pitch, {prev_quantizers, quantizers}, streams, slot_bytes, bytes_out, recon_i420, stats, &a);
  if (rc != MOBI_OK) return rc;
  inter_args(e, ref_i420, ref_pitch, stats, &a);
  return launch(e, &a, g_stages, s) == 0 ? MOBI_OK : MOBI_E_DEVICE;
}

int mobi_enc_inter_target_async(mobi_enc_inter_ctx *e, void *stream, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *ref_i420,
                                size_t ref_pitch, const uint8_t *prev_quantizers, const int32_t *target_bytes, int qmin, int qmax, uint8_t *streams,
                                size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_inter_stats *stats, uint8_t *quantizers_out) {
  if (!e) return MOBI_E_ARG;
  const uint8_t q1 = MOBI_ENC_QMIN; // both quantiser rows are made on the device: the check sees one that passes
  int rc = mobi_encp_check_args(e->max_pictures, e->width, e->height, e->version, 1, picture_pitch, ref_pitch, &q1, &q1, slot_bytes);
  if (rc != MOBI_OK) return rc;
  if (n < 1 || n > e->max_pictures || !prev_quantizers || mobi_enc_rate_check_args(target_bytes, qmin, qmax, quantizers_out) != 0) return MOBI_E_ARG;
  if (!i420 || !ref_i420 || !streams || !bytes_out || (uintptr_t)i420 % 8 || (uintptr_t)ref_i420 % 8 || (uintptr_t)streams % 4 || (uintptr_t)recon_i420 % 8 ||
      (uintptr_t)bytes_out % 4 || (uintptr_t)stats % 8)
    return MOBI_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  MobiEncPartsArgs a;
  memset((void *)&a, 0, sizeof a);
  rc = mobi_enc_ctx_begin(e, s, n, i420, picture_pitch, {}, streams, slot_bytes, bytes_out, recon_i420, stats, &a);
  if (rc != MOBI_OK) return rc;
  uint8_t *q_row = e->q + (size_t)e->max_pictures; // rows: previous, current
  a.q = q_row;
  inter_args(e, ref_i420, ref_pitch, stats, &a);
  // a trial: search, code (in the intra mode decide and finish too) and scan; the profiling twin's stage switch holds for the final encode alone
  return mobi_enc_ctx_rate(e, s, n, target_bytes, qmin, qmax, prev_quantizers, e->q, q_row, quantizers_out, bytes_out, stats, 7 | PINTRA_STAGES, g_stages,
                           [&](int stages) { return launch(e, &a, stages, s); });
}

int mobi_enc_inter(mobi_enc_inter_ctx *e, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *ref_i420, size_t ref_pitch,
                   const uint8_t *prev_quantizers, const uint8_t *quantizers, uint8_t *streams, size_t slot_bytes, int32_t *bytes_out,
                   uint8_t *recon_i420, mobi_enc_inter_stats *stats) {
  if (!e) return MOBI_E_ARG;
  const int rc = mobi_encp_check_args(e->max_pictures, e->width, e->height, e->version, n, picture_pitch, ref_pitch, prev_quantizers, quantizers, slot_bytes);
  if (rc != MOBI_OK) return rc;
  if (!i420 || !ref_i420 || !streams || !bytes_out) return MOBI_E_ARG;
  return mobi_enc_ctx_host(e, n, i420, picture_pitch, streams, slot_bytes, bytes_out, recon_i420, stats, [&](hipStream_t s, uint8_t *d_streams) {
    if (!mobi_enc_ctx_need(&e->st_ref, (size_t)e->max_pictures * e->frame) ||
        hipMemcpy2DAsync(e->st_ref, e->frame, ref_i420, ref_pitch, e->frame, (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess)
      return (int)MOBI_E_DEVICE;
    return mobi_enc_inter_async(e, s, n, e->st_in, e->frame, e->st_ref, e->frame, prev_quantizers, quantizers, d_streams, slot_bytes, (int32_t *)e->st_bytes,
                                e->st_rec, (mobi_enc_inter_stats *)e->st_stats);
  });
}
