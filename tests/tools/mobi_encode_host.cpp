// mobi_encode_host.cpp -- TEST TOOL: the intra encoder on the CPU, from the product's own header (csrc/mobi_encode.h): the host model that
// the kernels (csrc/mobi_encode.hip) are compared against byte for byte, and the thing the oracle judges without a GPU.
// The constants-once idiom and the picture pool are enc_host_pool.h's.
// Built by mobiclipdecoder_amd/build.py (build_enc_host) and, with sanitizers, into tests/tools/enc_host_main.cpp's program.
#include "enc_host_pool.h"
#include "mobi_encode.h"

extern "C" {

size_t enc_host_bound(uint32_t width, uint32_t height) { return mobi_enc_bound(width, height); }
int enc_host_check(int max_pictures, uint32_t width, uint32_t height, int version, int n, size_t picture_pitch, const uint8_t *quantizers,
                   int yuv_format, size_t slot_bytes) {
  return mobi_enc_check_args(max_pictures, width, height, version, n, picture_pitch, quantizers, yuv_format, slot_bytes);
}
size_t enc_host_mb_bytes(void) { return sizeof(MobiEncMb); }

// mobi_enc_intra's arguments (host pointers) plus: mbs [n][macroblocks] records (may be NULL), forms [4] code forms written, summed (may be
// NULL), threads >= 1 (pictures are dealt to them).  Returns 0, the check's refusal, or 1 if some stream's written bits were not its priced bits.
int enc_host_intra(uint32_t width, uint32_t height, int version, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *quantizers,
                   int yuv_format, uint8_t *streams, size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_stats *stats,
                   MobiEncMb *mbs, uint32_t *forms, int threads) {
  const int rc = mobi_enc_check_args(n, width, height, version, n, picture_pitch, quantizers, yuv_format, slot_bytes);
  if (rc) return rc;
  if (!i420 || !streams || !bytes_out || threads < 1) return -7;
  const MobiEncConst *K = enc_host_const(mobi_enc_build_const);
  const size_t frame = (size_t)width * height * 3 / 2, nmb = (size_t)(width / 16) * (height / 16);
  return enc_host_pool(n, threads, forms, [&](int i, uint32_t *tforms) {
    std::vector<uint8_t> rec(recon_i420 ? 0 : frame);
    std::vector<MobiEncMb> mb(mbs ? 0 : nmb);
    return mobi_enc_picture(K, (int)width, (int)height, quantizers[i], yuv_format, i420 + (size_t)i * picture_pitch, streams + (size_t)i * slot_bytes,
                            slot_bytes, bytes_out + i, recon_i420 ? recon_i420 + (size_t)i * frame : rec.data(), stats ? stats + i : nullptr,
                            mbs ? mbs + (size_t)i * nmb : mb.data(), tforms);
  });
}

// every (|level|, run, last) the writer can meet: the length mobi_enc_symbol writes against the price mobi_tc_cost states.
// Returns the number of disagreements; patterns [44 * 64 * 2] and lengths receive what was written for a positive level (may be NULL).
int enc_host_symbol_walk(uint32_t *patterns, int32_t *lengths, int32_t *form_out) {
  const MobiEncConst *K = enc_host_const(mobi_enc_build_const);
  int16_t ref[32 * 64 * 2];
  mobi_tc_build_ref(ref);
  int wrong = 0;
  for (int v = 1; v <= MOBI_ENC_MAX_LEVEL; v++)
    for (int run = 0; run < 64; run++)
      for (int last = 0; last < 2; last++) {
        int n, form, n2, form2;
        const uint32_t pat = mobi_enc_symbol(K, v, run, last, &n, &form);
        const uint32_t neg = mobi_enc_symbol(K, -v, run, last, &n2, &form2);
        wrong += n != mobi_tc_cost(ref, mobi_vx2table0_a, mobi_vx2table0_b, v, run, last) || n2 != n || form2 != form || (n < 32 && (pat >> n) != 0);
        if (form != MOBI_ENC_FORM_RAW) wrong += neg != (pat | 1u) || (pat & 1u);
        if (v < MOBI_TC_LUT_V) {
          wrong += n != K->lut[mobi_tc_lut_index(v, run, last)];
          const int at = (v * 64 + run) * 2 + last;
          if (patterns) patterns[at] = pat;
          if (lengths) lengths[at] = n;
          if (form_out) form_out[at] = form;
        }
      }
  return wrong;
}

// one block through the block rule at ANY table quantiser (the encoder itself refuses q < 12, where alone a level can leave the raw
// escape's 12 bits): src / pred 64 bytes; lev [64] scan order, rec [64]; out = {sad, bits, coded, clamp fallback, level-range fallback}
void enc_host_block(int q, const uint8_t *src, const uint8_t *pred, int16_t *lev, uint8_t *rec, int32_t *out) {
  const MobiEncConst *K = enc_host_const(mobi_enc_build_const);
  int s[64], p[64], r[64];
  for (int i = 0; i < 64; i++) { s[i] = src[i]; p[i] = pred[i]; }
  const MobiEncBlock b = mobi_enc_block(K, q, s, p, lev, r);
  for (int i = 0; i < 64; i++) rec[i] = (uint8_t)r[i];
  out[0] = b.sad; out[1] = b.bits; out[2] = b.coded; out[3] = b.clamp; out[4] = b.range;
}

// the bit writer alone over given macroblock records (their bits fields are filled in): the stream into slot (slot_bytes, zeroed first);
// returns its length in bytes, or 0 if it does not fit
size_t enc_host_write(uint32_t width, uint32_t height, int q, int yuv_format, MobiEncMb *mbs, uint8_t *slot, size_t slot_bytes) {
  const MobiEncConst *K = enc_host_const(mobi_enc_build_const);
  const size_t nmb = (size_t)(width / 16) * (height / 16);
  uint64_t total = 0;
  for (size_t i = 0; i < nmb; i++) {
    uint64_t n = 0;
    mobi_enc_write_mb(K, mbs + i, [&](uint32_t, int nb) { n += (uint64_t)nb; }, (uint32_t *)nullptr);
    mbs[i].bits = (uint32_t)n;
    total += n;
  }
  const uint64_t bytes = mobi_enc_stream_bytes(total);
  memset(slot, 0, slot_bytes);
  if (bytes <= slot_bytes) {
    MobiEncHostSink sink{slot, 0};
    sink(mobi_enc_header(yuv_format, q), MOBI_ENC_HEADER_BITS);
    for (size_t i = 0; i < nmb; i++) mobi_enc_write_mb(K, mbs + i, [&](uint32_t v, int nb) { sink(v, nb); }, (uint32_t *)nullptr);
  }
  return bytes <= slot_bytes ? (size_t)bytes : 0;
}
}
