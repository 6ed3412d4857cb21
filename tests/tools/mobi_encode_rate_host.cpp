// mobi_encode_rate_host.cpp -- TEST TOOL: the encoders' rate rule on the CPU, from the product's own header (csrc/mobi_encode_rate.h): the
// host model that the _target_async calls (csrc/mobi_encode_rate.hip around the encoders' kernels) are compared against byte for byte.
// A loop of its own over the three models' picture functions: mobi_enc_picture (I-frames), mobi_encp_picture (P-frames, mode 0) and
// mobi_encq_picture (P-frames, partition mode 1).  A trial is the picture function with a slot of no bytes: it prices the stream and
// writes none of it.  The constants-once idiom and the picture pool are enc_host_pool.h's.
// Built by mobiclipdecoder_amd/build.py (build_encratehost) and, with sanitizers, into tests/tools/enc_rate_host_main.cpp's program.
#include "enc_host_pool.h"
#include "mobi_encode_rate.h"

extern "C" {

int encr_host_rounds(int qmin, int qmax) { return mobi_enc_rate_rounds_of(qmin, qmax); }
size_t encr_host_bound(uint32_t width, uint32_t height, int kind) {
  return kind == 0 ? mobi_enc_bound(width, height) : mobi_encq_bound(width, height, kind - 1);
}

// kind 0: mobi_enc_intra_target_async's arguments; kind 1 / 2: mobi_enc_inter_target_async's in partition mode 0 / 1 -- all host
// pointers; what a kind does not have (ref_i420, prev_quantizers; yuv_format) is ignored.  stats: the kind's 64-byte records or NULL.
// trials [n][6][2] (may be NULL): every round's (quantiser, stream bytes), -1 where there was no round.  threads >= 1.
// Returns 0, a refusal, or 1 if some final stream's written bits were not its priced bits.
int encr_host_target(uint32_t width, uint32_t height, int version, int kind, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *ref_i420,
                     size_t ref_pitch, const uint8_t *prev_quantizers, const int32_t *target_bytes, int qmin, int qmax, int yuv_format, uint8_t *streams,
                     size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420, void *stats, uint8_t *quantizers_out, int32_t *trials, int threads) {
  if (kind < 0 || kind > 2 || threads < 1) return -7;
  const uint8_t q1 = MOBI_ENC_QMIN;
  const int rc = kind == 0 ? mobi_enc_check_args(n, width, height, version, 1, picture_pitch, &q1, yuv_format, slot_bytes)
                           : mobi_encp_check_args(n, width, height, version, 1, picture_pitch, ref_pitch, &q1, &q1, slot_bytes);
  if (rc) return rc;
  if (n < 1 || mobi_enc_rate_check_args(target_bytes, qmin, qmax, quantizers_out) != 0 || !i420 || !streams || !bytes_out) return -7;
  if (kind != 0 && (!ref_i420 || !prev_quantizers)) return -7;
  const MobiEncPartsConst *K = enc_host_const(mobi_encq_build_const); // begins with the inter encoder's constants, those with the intra encoder's
  const int W = (int)width, H = (int)height, ver = mobi_encp_ver(version), rounds = mobi_enc_rate_rounds_of(qmin, qmax);
  const size_t frame = (size_t)width * height * 3 / 2, nmb = (size_t)(width / 16) * (height / 16);
  if (trials)
    for (size_t i = 0; i < (size_t)n * 12; i++) trials[i] = -1;
  return enc_host_pool(n, threads, nullptr, [&](int i, uint32_t *tforms) {
    std::vector<uint8_t> own(recon_i420 ? 0 : frame);
    std::vector<MobiEncMb> mb(nmb);
    std::vector<uint32_t> v(nmb), vp(nmb), v4(4 * nmb);
    uint8_t *rec = recon_i420 ? recon_i420 + (size_t)i * frame : own.data();
    const uint8_t *src = i420 + (size_t)i * picture_pitch, *ref = kind ? ref_i420 + (size_t)i * ref_pitch : nullptr;
    const int prev_q = kind ? mobi_enc_rate_clamp_q(prev_quantizers[i]) : 0;
    // the picture at q into `slot` of `room` bytes
    auto picture = [&](int q, uint8_t *slot, size_t room, int32_t *bytes, void *st) {
      if (kind == 0) return mobi_enc_picture(K, W, H, q, yuv_format, src, slot, room, bytes, rec, (mobi_enc_stats *)st, mb.data(), tforms);
      if (kind == 1)
        return mobi_encp_picture(K, ver, W, H, prev_q, q, src, ref, slot, room, bytes, rec, (mobi_enc_inter_stats *)st, mb.data(), v.data(), vp.data(), tforms);
      return mobi_encq_picture(K, ver, 1, W, H, prev_q, q, src, ref, slot, room, bytes, rec, (mobi_enc_inter_stats *)st, mb.data(), v.data(), vp.data(),
                               v4.data(), tforms);
    };
    MobiEncRateState s;
    s.lo = qmin;
    s.hi = qmax;
    for (int k = 0; k < rounds; k++) {
      int32_t bytes = 0;
      const int mid = mobi_enc_rate_mid(s);
      uint8_t none = 0; // a slot of no bytes
      picture(mid, &none, 0, &bytes, nullptr);
      if (trials) {
        trials[((size_t)i * 6 + k) * 2] = mid;
        trials[((size_t)i * 6 + k) * 2 + 1] = bytes;
      }
      s = mobi_enc_rate_step(s, bytes, target_bytes[i]);
    }
    const int q = mobi_enc_rate_mid(s);
    quantizers_out[i] = (uint8_t)q;
    return picture(q, streams + (size_t)i * slot_bytes, slot_bytes, bytes_out + i, stats ? (uint8_t *)stats + (size_t)i * 64 : nullptr);
  });
}
}
