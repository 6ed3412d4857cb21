// mobi_encode_inter_host.cpp -- TEST TOOL: the inter encoder on the CPU, from the product's own header (csrc/mobi_encode_inter.h): the host
// model that the kernels (csrc/mobi_encode_inter.hip) are compared against byte for byte, and the thing the oracle judges without a GPU.
// A scalar loop of its own: search, prediction and block coding share the kernels' rule functions, not their lane code.
// The constants-once idiom and the picture pool are enc_host_pool.h's.
// Built by mobiclipdecoder_amd/build.py (build_enc_host) and, with sanitizers, into tests/tools/enc_inter_host_main.cpp's program.
#include "enc_host_pool.h"
#include "mobi_encode_inter.h"

extern "C" {

size_t encp_host_bound(uint32_t width, uint32_t height) { return mobi_encp_bound(width, height); }
int encp_host_check(int max_pictures, uint32_t width, uint32_t height, int version, int n, size_t picture_pitch, size_t ref_pitch,
                    const uint8_t *prev_quantizers, const uint8_t *quantizers, size_t slot_bytes) {
  return mobi_encp_check_args(max_pictures, width, height, version, n, picture_pitch, ref_pitch, prev_quantizers, quantizers, slot_bytes);
}
size_t encp_host_mb_bytes(void) { return sizeof(MobiEncMb); }
int encp_host_range(void) { return MOBI_ENCP_RANGE; }

// mobi_enc_inter's arguments (host pointers) plus: mbs [n][macroblocks] records, mv and mvp [n][macroblocks] v* and predictors (dx low,
// dy high 16 bits), forms [4] code forms written, summed (each may be NULL), threads >= 1 (pictures are dealt to them).
// Returns 0, the check's refusal, or 1 if some stream's written bits were not its priced bits.
int encp_host_inter(uint32_t width, uint32_t height, int version, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *ref_i420,
                    size_t ref_pitch, const uint8_t *prev_quantizers, const uint8_t *quantizers, uint8_t *streams, size_t slot_bytes,
                    int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_inter_stats *stats, MobiEncMb *mbs, uint32_t *mv, uint32_t *mvp,
                    uint32_t *forms, int threads) {
  const int rc = mobi_encp_check_args(n, width, height, version, n, picture_pitch, ref_pitch, prev_quantizers, quantizers, slot_bytes);
  if (rc) return rc;
  if (!i420 || !ref_i420 || !streams || !bytes_out || threads < 1) return -7;
  const MobiEncInterConst *K = enc_host_const(mobi_encp_build_const);
  const size_t frame = (size_t)width * height * 3 / 2, nmb = (size_t)(width / 16) * (height / 16);
  return enc_host_pool(n, threads, forms, [&](int i, uint32_t *tforms) {
    std::vector<uint8_t> rec(recon_i420 ? 0 : frame);
    std::vector<MobiEncMb> mb(mbs ? 0 : nmb);
    std::vector<uint32_t> v(mv ? 0 : nmb), vp(mvp ? 0 : nmb);
    return mobi_encp_picture(K, mobi_encp_ver(version), (int)width, (int)height, prev_quantizers[i], quantizers[i], i420 + (size_t)i * picture_pitch,
                             ref_i420 + (size_t)i * ref_pitch, streams + (size_t)i * slot_bytes, slot_bytes, bytes_out + i,
                             recon_i420 ? recon_i420 + (size_t)i * frame : rec.data(), stats ? stats + i : nullptr, mbs ? mbs + (size_t)i * nmb : mb.data(),
                             mv ? mv + (size_t)i * nmb : v.data(), mvp ? mvp + (size_t)i * nmb : vp.data(), tforms);
  });
}
}
