// mobi_encode_pintra.h -- the inter encoder's intra mode (include/mobiclip_encode_pintra.h; DESIGN.md, "Inter encoder", "Intra
// macroblocks"): the rules that the kernels (mobi_encode_pintra.hip, the code kernel of mobi_encode_inter.hip), the host entry points
// (mobi_encode_inter.cpp), the host model (tests/tools/mobi_encode_pintra_host.cpp) and the CPU tests compile alike.  Search, prediction,
// predictor and P-syntax are mobi_encode_inter.h's, the trials, the block rule and the intra macroblock's syntax mobi_encode.h's; nothing
// is copied.
//
//   Jp        the inter coding of the search's v*: sum of mobi_enc_cost over its six blocks + lam * (mobi_encp_mv_bits against the ZERO
//             predictor + mobi_encp_cbp_bits): the true predictor needs the top-right neighbour's decision, which lies on the macroblock's
//             own anti-diagonal
//   Ji        the best luma trial + the best chroma trial as mobi_enc_macroblock chooses them, the border from THIS frame's final
//             reconstruction of the left and upper macroblocks, + lam * (bits of partition code 6 + ue(cbp) + the two 3-bit modes)
//   decision  intra iff Ji < Jp; a tie stays inter.  Jp <= 12 lam cannot be beaten (Ji >= lam * (5 + 1 + 6)): such a macroblock may skip
//             its trials
//   vectors   an intra macroblock's effective vector is (0, 0) (parse_p clears its MV slot): the mv array holds it once the decisions
//             stand, so that mobi_encp_predictor serves; predictors, code 0 / 1, bits and statistics are made after all decisions
//   syntax    inter: mobi_encp_write_mb; intra: partition code 6, then mobi_enc_write_mb_body
#ifndef MOBI_ENCODE_PINTRA_H
#define MOBI_ENCODE_PINTRA_H
#include "../../include/mobiclip_encode_pintra.h"
#include "mobi_encode_inter.h"

enum { MOBI_ENCPI_CODE = 6,      // the partition code of an intra macroblock in the full-block syntax (16x16 only): MobiEncInterConst::part6_*
       MOBI_ENCPI_CODE_BITS = 5 }; // its length in both versions' 16x16 tables.  mobi_part_bits is no constant expression (the tables are
                                   // plain C data), so the figure stands here for the bound below and tests/test_encode_pintra_model.py
                                   // holds it against the tables; every cost and every stream takes the length from the tables' part6_nbits
// an intra macroblock in front of its blocks: code 6, ue() of a number below 64, two modes; the inter bound counts 3 + 2 x 13 + 13
static_assert(MOBI_ENCPI_CODE_BITS + 13 + 6 <= 3 + 2 * 13 + 13, "mobi_encp_max_mb_bits covers an intra macroblock: mobi_enc_inter_stream_bound stays");

// ---- the intra mode and the partition mode exclude each other (with leaves, the exported vector and the tree's pricing need a finish
// pass of their own).  What either setter does: *mine becomes mode (0 or 1) unless mode is neither or would be on beside `other`;
// MOBI_E_ARG then, and nothing changes ----
static inline int mobi_encpi_set_mode(int *mine, int other, int mode) {
  if ((mode != 0 && mode != 1) || (mode && other)) return -7; // MOBI_E_ARG
  *mine = mode;
  return 0;
}

// ---- a macroblock's kind word (MobiEncInterArgs::kind): bit 0 = sent intra; the chosen coding's figures for the statistics: blocks that
// fell back by the clamp (bits 1..3) and by the level range (4..6), the sad (from bit 8: at most 6 * 64 * 255 < 2^17) ----
MOBI_TC_FN uint32_t mobi_encpi_kind(bool intra, uint32_t sad, uint32_t clamp, uint32_t range) { return (uint32_t)intra | clamp << 1 | range << 4 | sad << 8; }
MOBI_TC_FN bool mobi_encpi_is_intra(uint32_t kind) { return kind & 1u; }
MOBI_TC_FN uint32_t mobi_encpi_clamp(uint32_t kind) { return (kind >> 1) & 7u; }
MOBI_TC_FN uint32_t mobi_encpi_range(uint32_t kind) { return (kind >> 4) & 7u; }
MOBI_TC_FN uint32_t mobi_encpi_sad(uint32_t kind) { return kind >> 8; }

// ---- the two costs.  sad / block_bits: the sums over the coding's six blocks (mobi_enc_cost is linear in both) ----
MOBI_TC_FN int64_t mobi_encpi_jp(const MobiEncInterConst *K, int ver, int64_t lam, uint32_t sad, uint32_t block_bits, uint32_t v, uint32_t cbp) {
  return ((int64_t)sad << 8) + lam * (int64_t)(block_bits + mobi_encp_mv_bits(K, ver, v, 0u) + mobi_encp_cbp_bits(K, cbp));
}
// an intra macroblock's bits in front of its blocks: the I-frame's (mobi_enc_mb_header_bits) with code 6 in the leading bit's place
MOBI_TC_FN uint32_t mobi_encpi_header_bits(const MobiEncInterConst *K, int ver, uint32_t cbp) { return mobi_enc_mb_header_bits(K, cbp) - 1u + K->part6_nbits[ver]; }
// trials: the winners' costs, luma + chroma
MOBI_TC_FN int64_t mobi_encpi_ji(const MobiEncInterConst *K, int ver, int64_t lam, int64_t trials, uint32_t cbp) {
  return trials + lam * (int64_t)mobi_encpi_header_bits(K, ver, cbp);
}
// no Ji is below lam * (code 6 + the shortest ue(cbp) + the modes): a macroblock with Jp at or below that stays inter whatever its trials give
MOBI_TC_FN bool mobi_encpi_skip(const MobiEncInterConst *K, int ver, int64_t lam, int64_t jp) { return jp <= lam * (int64_t)(K->part6_nbits[ver] + 1 + 6); }
MOBI_TC_FN bool mobi_encpi_wins(int64_t ji, int64_t jp) { return ji < jp; } // a tie stays inter

// ---- what the finish pass makes of macroblock i once every decision stands (mv holds the effective vectors): the predictor and the bits
// in front of ue(cbp) -- an inter macroblock's code 0 / 1 and difference, an intra one's code 6 ----
MOBI_TC_FN uint32_t mobi_encpi_finish_mb(const MobiEncInterConst *K, int ver, const uint32_t *mv, int mbw, int mbx, int mby, bool intra, uint32_t *pred) {
  *pred = intra ? 0u : mobi_encp_predictor(mv, mbw, mbx, mby);
  return intra ? (uint32_t)K->part6_nbits[ver] : mobi_encp_mv_bits(K, ver, mv[mby * mbw + mbx], *pred);
}

// ---- the bit string of either kind ----
template <class Put>
MOBI_TC_FN void mobi_encpi_write_mb(const MobiEncInterConst *K, int ver, const MobiEncMb *m, bool intra, uint32_t v, uint32_t pred, Put put, uint32_t *forms) {
  if (!intra) {
    mobi_encp_write_mb(K, ver, m, v, pred, put, forms);
    return;
  }
  put(K->part6_code[ver], K->part6_nbits[ver]);
  mobi_enc_write_mb_body(K, m, put, forms);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- one picture on the CPU.  mode 0 is mobi_encp_picture.  mode 1: search every macroblock; in raster order (every macroblock behind
// its left and upper neighbours, as the anti-diagonals are) the inter coding, its cost, the trials on the picture's reconstruction so far
// and the decision; then predictors, bits and statistics.  kind and jp (macroblocks each) are required in mode 1. ----
static inline bool mobi_encpi_picture(const MobiEncInterConst *K, int ver, int mode, int W, int H, int prev_q, int q, const uint8_t *i420, const uint8_t *ref_i420,
                                      uint8_t *slot, size_t slot_bytes, int32_t *bytes_out, uint8_t *rec, mobi_enc_inter_stats *stats, MobiEncMb *mbs,
                                      uint32_t *mv, uint32_t *mvp, uint32_t *kind, int64_t *jp, uint32_t *forms) {
  if (!mode) return mobi_encp_picture(K, ver, W, H, prev_q, q, i420, ref_i420, slot, slot_bytes, bytes_out, rec, stats, mbs, mv, mvp, forms);
  const size_t ysz = (size_t)W * H;
  const uint8_t *const src[3] = {i420, i420 + ysz, i420 + ysz + ysz / 4};
  const uint8_t *const ref[3] = {ref_i420, ref_i420 + ysz, ref_i420 + ysz + ysz / 4};
  uint8_t *const r3[3] = {rec, rec + ysz, rec + ysz + ysz / 4};
  const int mbw = W / 16, mbh = H / 16;
  const int64_t lam = mobi_enc_lambda(q);
  for (int y = 0; y < mbh; y++)
    for (int x = 0; x < mbw; x++) mv[y * mbw + x] = mobi_encp_search(q, W, H, x, y, src[0], ref[0]);
  for (int y = 0; y < mbh; y++)
    for (int x = 0; x < mbw; x++) {
      const int i = y * mbw + x;
      MobiEncMbStats ms;
      mobi_encp_macroblock(K, q, W, x, y, mv[i], src, ref, r3, mbs + i, &ms); // bits: the blocks' alone until the finish pass
      jp[i] = mobi_encpi_jp(K, ver, lam, ms.sad, mbs[i].bits, mv[i], mbs[i].cbp);
      kind[i] = mobi_encpi_kind(false, ms.sad, ms.clamp, ms.range);
      if (mobi_encpi_skip(K, ver, lam, jp[i])) continue;
      // the inter coding set aside: mobi_enc_macroblock writes the winners into the picture and the record
      const MobiEncMb inter = mbs[i];
      uint8_t px[16 * 16 + 2 * 8 * 8];
      for (int k = 0, o = 0; k < 3; k++) {
        const int n = k ? 8 : 16, pitch = k ? W / 2 : W;
        for (int r = 0; r < n; r++, o += n) memcpy(px + o, r3[k] + (size_t)(y * n + r) * pitch + x * n, (size_t)n);
      }
      MobiEncMbStats is;
      mobi_enc_macroblock(K, q, W, x, y, src, r3, mbs + i, &is);
      const uint32_t block_bits = mbs[i].bits - mobi_enc_mb_header_bits(K, mbs[i].cbp);
      const int64_t ji = mobi_encpi_ji(K, ver, lam, ((int64_t)is.sad << 8) + lam * (int64_t)block_bits, mbs[i].cbp);
      if (mobi_encpi_wins(ji, jp[i])) {
        mbs[i].bits = block_bits + mobi_encpi_header_bits(K, ver, mbs[i].cbp);
        kind[i] = mobi_encpi_kind(true, is.sad, is.clamp, is.range);
        mv[i] = 0u;
      } else {
        mbs[i] = inter;
        for (int k = 0, o = 0; k < 3; k++) {
          const int n = k ? 8 : 16, pitch = k ? W / 2 : W;
          for (int r = 0; r < n; r++, o += n) memcpy(r3[k] + (size_t)(y * n + r) * pitch + x * n, px + o, (size_t)n);
        }
      }
    }
  mobi_enc_inter_stats st;
  memset(&st, 0, sizeof st);
  uint64_t mb_bits = 0;
  for (int y = 0; y < mbh; y++)
    for (int x = 0; x < mbw; x++) {
      const int i = y * mbw + x;
      const bool intra = mobi_encpi_is_intra(kind[i]);
      const uint32_t vb = mobi_encpi_finish_mb(K, ver, mv, mbw, x, y, intra, mvp + i);
      if (!intra) mbs[i].bits += vb + mobi_encp_cbp_bits(K, mbs[i].cbp);
      mb_bits += mbs[i].bits;
      st.sad += mobi_encpi_sad(kind[i]);
      st.mv_bits += vb;
      st.coded_blocks += (uint32_t)__builtin_popcount(mbs[i].cbp);
      st.fallback_clamp += mobi_encpi_clamp(kind[i]);
      st.fallback_level += mobi_encpi_range(kind[i]);
      st.reserved[MOBI_ENC_PINTRA_STAT_INTRA] += intra;
      if (intra) continue;
      st.code0 += mv[i] == mvp[i];
      st.nonzero_mv += mv[i] != 0;
      st.halfpel_mv += ((mobi_encp_dx(mv[i]) | mobi_encp_dy(mv[i])) & 1) != 0;
    }
  return mobi_enc_finish_picture((uint64_t)mobi_encp_header_bits(q, prev_q), mb_bits, st, stats, slot, slot_bytes, bytes_out, [&](auto put) {
    mobi_encp_write_header(put, q, prev_q);
    for (int i = 0; i < mbw * mbh; i++) mobi_encpi_write_mb(K, ver, mbs + i, mobi_encpi_is_intra(kind[i]), mv[i], mvp[i], put, forms);
  });
}
#endif
#endif
