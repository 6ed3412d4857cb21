// mobi_encode_parts_host.cpp -- TEST TOOL: the inter encoder with its partition mode on the CPU, from the product's own header
// (csrc/mobi_encode_parts.h): the host model that the kernels (csrc/mobi_encode_parts.hip) are compared against byte for byte, and the thing
// the oracle judges without a GPU.  Scalar, sample by sample: search, tree, prediction and block coding share the kernels' rule functions,
// not their lane code.  The constants-once idiom and the picture pool are enc_host_pool.h's.
// Built by mobiclipdecoder_amd/build.py (build_encpartshost) and, with sanitizers, into tests/tools/enc_parts_host_main.cpp's program.
#include "enc_host_pool.h"
#include "mobi_encode_parts.h"

extern "C" {

size_t encq_host_bound(uint32_t width, uint32_t height, int mode) { return mobi_encq_bound(width, height, mode); }
size_t encq_host_mb_bytes(void) { return sizeof(MobiEncMb); }
// the generalised candidate predicate and the one it generalises (tests pin them equal at 16x16)
int encq_host_leaf_ok(int W, int H, int x, int y, int w, int h, int dx, int dy) { return mobi_encq_leaf_ok(W, H, x, y, w, h, dx, dy); }
int encq_host_vector_ok(int W, int H, int mbx, int mby, int dx, int dy) { return mobi_encp_vector_ok(W, H, mbx, mby, dx, dy); }

// encp_host_inter's arguments (tests/tools/mobi_encode_inter_host.cpp) plus the mode and mv4 [n][macroblocks][4] the quadrants' vectors
// (may be NULL); the trees are the records' luma_mode.  Returns 0, the check's refusal, or 1 if some stream's written bits were not its
// priced bits.
int encq_host_inter(uint32_t width, uint32_t height, int version, int mode, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *ref_i420,
                    size_t ref_pitch, const uint8_t *prev_quantizers, const uint8_t *quantizers, uint8_t *streams, size_t slot_bytes,
                    int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_inter_stats *stats, MobiEncMb *mbs, uint32_t *mv, uint32_t *mvp, uint32_t *mv4,
                    uint32_t *forms, int threads) {
  const int rc = mobi_encp_check_args(n, width, height, version, n, picture_pitch, ref_pitch, prev_quantizers, quantizers, slot_bytes);
  if (rc) return rc;
  if (!i420 || !ref_i420 || !streams || !bytes_out || threads < 1 || (mode != 0 && mode != 1)) return -7;
  const MobiEncPartsConst *K = enc_host_const(mobi_encq_build_const);
  const size_t frame = (size_t)width * height * 3 / 2, nmb = (size_t)(width / 16) * (height / 16);
  return enc_host_pool(n, threads, forms, [&](int i, uint32_t *tforms) {
    std::vector<uint8_t> rec(recon_i420 ? 0 : frame);
    std::vector<MobiEncMb> mb(mbs ? 0 : nmb);
    std::vector<uint32_t> v(mv ? 0 : nmb), vp(mvp ? 0 : nmb), v4(mv4 ? 0 : 4 * nmb);
    return mobi_encq_picture(K, mobi_encp_ver(version), mode, (int)width, (int)height, prev_quantizers[i], quantizers[i], i420 + (size_t)i * picture_pitch,
                             ref_i420 + (size_t)i * ref_pitch, streams + (size_t)i * slot_bytes, slot_bytes, bytes_out + i,
                             recon_i420 ? recon_i420 + (size_t)i * frame : rec.data(), stats ? stats + i : nullptr, mbs ? mbs + (size_t)i * nmb : mb.data(),
                             mv ? mv + (size_t)i * nmb : v.data(), mvp ? mvp + (size_t)i * nmb : vp.data(), mv4 ? mv4 + (size_t)i * nmb * 4 : v4.data(), tforms);
  });
}
}
