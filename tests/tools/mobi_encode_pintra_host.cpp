// mobi_encode_pintra_host.cpp -- TEST TOOL: the inter encoder with its intra mode on the CPU, from the product's own header
// (csrc/mobi_encode_pintra.h): the host model that the kernels (csrc/mobi_encode_pintra.hip) are compared against byte for byte, and the
// thing the oracle judges without a GPU.  Scalar, macroblock by macroblock in raster order: search, inter coding, trials and decision share
// the kernels' rule functions, not their lane code.  The constants-once idiom and the picture pool are enc_host_pool.h's.
// Built by mobiclipdecoder_amd/build.py (build_encpintrahost).
#include "enc_host_pool.h"
#include "mobi_encode_pintra.h"

extern "C" {

size_t encpi_host_bound(uint32_t width, uint32_t height) { return mobi_encp_bound(width, height); }
size_t encpi_host_mb_bytes(void) { return sizeof(MobiEncMb); }
int encpi_host_stat_intra(void) { return MOBI_ENC_PINTRA_STAT_INTRA; }
// the code word of partition code 6 at 16x16 and its length
uint32_t encpi_host_code_word(int version) { return enc_host_const(mobi_encp_build_const)->part6_code[mobi_encp_ver(version)]; }
int encpi_host_code_bits(int version) { return enc_host_const(mobi_encp_build_const)->part6_nbits[mobi_encp_ver(version)]; }
int encpi_host_code_bits_bound(void) { return MOBI_ENCPI_CODE_BITS; } // the figure the stream bound's static_assert counts

// the setters' rule: modes[0] = partitions, modes[1] = intra; sets modes[which] as mobi_enc_inter_set_partitions / _set_intra would
int encpi_host_set_mode(int *modes, int which, int mode) { return mobi_encpi_set_mode(&modes[which], modes[1 - which], mode); }

// encp_host_inter's arguments (tests/tools/mobi_encode_inter_host.cpp) plus the mode and, in front of forms, kind [n][macroblocks] (bit 0:
// sent intra) and jp [n][macroblocks] (the inter coding's cost; 64-bit), which mode 1 fills (each may be NULL).  mv holds the EFFECTIVE
// vectors: zero in intra macroblocks.  Returns 0, the check's refusal, or 1 if some stream's written bits were not its priced bits.
int encpi_host_inter(uint32_t width, uint32_t height, int version, int mode, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *ref_i420,
                     size_t ref_pitch, const uint8_t *prev_quantizers, const uint8_t *quantizers, uint8_t *streams, size_t slot_bytes,
                     int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_inter_stats *stats, MobiEncMb *mbs, uint32_t *mv, uint32_t *mvp, uint32_t *kind,
                     int64_t *jp, uint32_t *forms, int threads) {
  const int rc = mobi_encp_check_args(n, width, height, version, n, picture_pitch, ref_pitch, prev_quantizers, quantizers, slot_bytes);
  if (rc) return rc;
  if (!i420 || !ref_i420 || !streams || !bytes_out || threads < 1 || (mode != 0 && mode != 1)) return -7;
  const MobiEncInterConst *K = enc_host_const(mobi_encp_build_const);
  const size_t frame = (size_t)width * height * 3 / 2, nmb = (size_t)(width / 16) * (height / 16);
  return enc_host_pool(n, threads, forms, [&](int i, uint32_t *tforms) {
    std::vector<uint8_t> rec(recon_i420 ? 0 : frame);
    std::vector<MobiEncMb> mb(mbs ? 0 : nmb);
    std::vector<uint32_t> v(mv ? 0 : nmb), vp(mvp ? 0 : nmb), kd(kind ? 0 : nmb);
    std::vector<int64_t> j(jp ? 0 : nmb);
    return mobi_encpi_picture(K, mobi_encp_ver(version), mode, (int)width, (int)height, prev_quantizers[i], quantizers[i], i420 + (size_t)i * picture_pitch,
                              ref_i420 + (size_t)i * ref_pitch, streams + (size_t)i * slot_bytes, slot_bytes, bytes_out + i,
                              recon_i420 ? recon_i420 + (size_t)i * frame : rec.data(), stats ? stats + i : nullptr, mbs ? mbs + (size_t)i * nmb : mb.data(),
                              mv ? mv + (size_t)i * nmb : v.data(), mvp ? mvp + (size_t)i * nmb : vp.data(), kind ? kind + (size_t)i * nmb : kd.data(),
                              jp ? jp + (size_t)i * nmb : j.data(), tforms);
  });
}
}
