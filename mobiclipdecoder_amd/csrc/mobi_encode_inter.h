// mobi_encode_inter.h -- the inter encoder's rules (include/mobiclip_encode_inter.h; DESIGN.md, "Inter encoder") that the kernels
// (mobi_encode_inter.hip), the host entry points (mobi_encode_inter.cpp), the host model (tests/tools/mobi_encode_inter_host.cpp) and the
// CPU tests compile alike.  The block rule, the cost's lambda, the symbol writer and the sinks are mobi_encode.h's; nothing is copied.
//
//   scope           P-frames, one reference (the previous frame's reconstruction: partition codes 0 and 1 at 16x16), every macroblock one
//                   16x16 leaf with an 8x8-transform residual
//   candidates      vectors (dx, dy) in half-pels whose Y, U and V windows lie inside the picture RECTANGLE (mobi_encp_vector_ok: stricter
//                   than mobi_mc_windows_ok, which lets a row wrap)
//   search          step 1: every full-pel vector with |dx|, |dy| <= MOBI_ENCP_RANGE; step 2: the winner and its eight half-pel neighbours
//                   (so |dx|, |dy| <= MOBI_ENCP_RANGE + 1).  cost = (SAD_luma16x16 << 8) + lam[q] * (se_bits(dx) + se_bits(dy)) -- priced
//                   against the ZERO vector, so that the search needs no neighbour --; the smallest cost wins, ties go to the smaller
//                   |dx| + |dy|, then the smaller dy, then the smaller dx: all of it one 64-bit key (mobi_encp_key), the argmin is its minimum
//   syntax          the macroblock's vector is always the search's v*; predictor = median of the left, top and top-right v* (zeros outside
//                   the picture: parse_p's mvc_ walk); code 0 when equal, else code 1, se(dx - predx), se(dy - predy); ue(inverse of
//                   mobi_cbp_inter at cbp6); per coded area 1 + its symbols
//   header          0, se(q - prev_q)
#ifndef MOBI_ENCODE_INTER_H
#define MOBI_ENCODE_INTER_H
#include "../../include/mobiclip_encode_inter.h"
#include "mobi_encode.h"
#include "mobi_txcode.h"

enum { MOBI_ENCP_RANGE = 16,                  // half-pels: the reach of the full-pel step either way
       MOBI_ENCP_REACH = MOBI_ENCP_RANGE + 1, // ... of a chosen vector: the half-pel step goes one further
       MOBI_ENCP_MAX_HEADER_BITS = 1 + 13 };  // 0, se(dq) with |dq| <= 40

// ---- se(): v > 0 is code number 2v - 1, v <= 0 is -2v (mobi_gamma_signed read backwards); written as ue() ----
MOBI_TC_FN uint32_t mobi_encp_se_value(int v) { return v > 0 ? 2u * (uint32_t)v - 1u : (uint32_t)(-2 * v); }
MOBI_TC_FN int mobi_encp_se_bits(int v) { return mobi_enc_ue_bits(mobi_encp_se_value(v)); }
MOBI_TC_FN int mobi_encp_median(int a, int b, int c) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo > (hi < c ? hi : c) ? lo : (hi < c ? hi : c); // max(min(a, b), min(max(a, b), c))
}
MOBI_TC_FN int mobi_encp_header_bits(int q, int prev_q) { return 1 + mobi_encp_se_bits(q - prev_q); }

// ---- the candidate set: the 16x16 luma window and the two 8x8 chroma windows of vector (dx, dy), with the extra column / row their
// half-pel phases read, inside the planes' rectangles.  The chroma vector is (dx >> 1, dy >> 1) with its own phase (mc_leaf). ----
MOBI_TC_FN bool mobi_encp_vector_ok(int W, int H, int mbx, int mby, int dx, int dy) {
  const int x = mbx * 16 + (dx >> 1), y = mby * 16 + (dy >> 1);
  const int cdx = dx >> 1, cdy = dy >> 1, cx = mbx * 8 + (cdx >> 1), cy = mby * 8 + (cdy >> 1);
  return x >= 0 && y >= 0 && x + 15 + (dx & 1) < W && y + 15 + (dy & 1) < H && cx >= 0 && cy >= 0 && cx + 7 + (cdx & 1) < W / 2 &&
         cy + 7 + (cdy & 1) < H / 2;
}
// cost and tie rule as one key: cost < 2^27 ((255 * 256 << 8) + lam[52] * 22), |dx| + |dy| <= 34, dy and dx offset into 7 bits each
MOBI_TC_FN uint64_t mobi_encp_key(int64_t lam, uint32_t sad, int dx, int dy) {
  const uint64_t cost = ((uint64_t)sad << 8) + (uint64_t)lam * (uint64_t)(mobi_encp_se_bits(dx) + mobi_encp_se_bits(dy));
  const uint32_t len = (uint32_t)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy));
  return cost << 20 | (uint64_t)len << 14 | (uint64_t)(uint32_t)(dy + 64) << 7 | (uint64_t)(uint32_t)(dx + 64);
}
MOBI_TC_FN int mobi_encp_key_dx(uint64_t key) { return (int)(key & 127) - 64; }
MOBI_TC_FN int mobi_encp_key_dy(uint64_t key) { return (int)((key >> 7) & 127) - 64; }
#define MOBI_ENCP_NO_KEY (~(uint64_t)0)

// a vector as the kernels and the model keep it: dx in the low, dy in the high 16 bits
MOBI_TC_FN uint32_t mobi_encp_pack(int dx, int dy) { return ((uint32_t)dx & 0xFFFFu) | (uint32_t)dy << 16; }
MOBI_TC_FN int mobi_encp_dx(uint32_t v) { return (int16_t)(v & 0xFFFFu); }
MOBI_TC_FN int mobi_encp_dy(uint32_t v) { return (int16_t)(v >> 16); }
// the predictor of macroblock (mbx, mby) from the picture's vectors: left, top, top-right, zeros outside (a pure function of v*)
MOBI_TC_FN uint32_t mobi_encp_predictor(const uint32_t *mv, int mbw, int mbx, int mby) {
  const uint32_t l = mbx > 0 ? mv[mby * mbw + mbx - 1] : 0u, t = mby > 0 ? mv[(mby - 1) * mbw + mbx] : 0u,
                 tr = mby > 0 && mbx + 1 < mbw ? mv[(mby - 1) * mbw + mbx + 1] : 0u;
  return mobi_encp_pack(mobi_encp_median(mobi_encp_dx(l), mobi_encp_dx(t), mobi_encp_dx(tr)),
                        mobi_encp_median(mobi_encp_dy(l), mobi_encp_dy(t), mobi_encp_dy(tr)));
}

// per-device constants: the intra encoder's (block coder, symbol writer) as the base, the P-macroblock syntax behind them
struct MobiEncInterConst : MobiEncConst {
  uint8_t inv_cbp_p[64];  // the ue() number whose mobi_cbp_inter entry is cbp6
  uint8_t part_code[2][2]; // [0: Moflex3DS, 1: ModsDS][partition code 0 / 1 at 16x16]: the code word ...
  uint8_t part_nbits[2][2]; // ... and its length
  uint8_t part6_code[2], part6_nbits[2]; // [version table] partition code 6 at 16x16, an intra macroblock in the full-block syntax (mobi_encode_pintra.h)
};
MOBI_TC_FN int mobi_encp_ver(int version) { return version == 2 ? 0 : 1; } // MOBI_VERSION_MOFLEX3DS: table 0

// a macroblock's bits in front of its blocks
MOBI_TC_FN uint32_t mobi_encp_mv_bits(const MobiEncInterConst *K, int ver, uint32_t v, uint32_t pred) {
  if (v == pred) return K->part_nbits[ver][0];
  return (uint32_t)K->part_nbits[ver][1] + (uint32_t)mobi_encp_se_bits(mobi_encp_dx(v) - mobi_encp_dx(pred)) +
         (uint32_t)mobi_encp_se_bits(mobi_encp_dy(v) - mobi_encp_dy(pred));
}
MOBI_TC_FN uint32_t mobi_encp_cbp_bits(const MobiEncInterConst *K, uint32_t cbp) { return (uint32_t)mobi_enc_ue_bits(K->inv_cbp_p[cbp]); }

// ---- the bit strings: put(pattern, nbits) as in mobi_enc_write_mb ----
template <class Put>
MOBI_TC_FN void mobi_encp_put_se(Put put, int v) {
  const uint32_t u = mobi_encp_se_value(v);
  put(u + 1u, mobi_enc_ue_bits(u));
}
template <class Put>
MOBI_TC_FN void mobi_encp_write_header(Put put, int q, int prev_q) {
  put(0u, 1); // a P-frame
  mobi_encp_put_se(put, q - prev_q);
}
// what follows a macroblock's partition tree (here and in mobi_encode_parts.h): ue(cbp), the coded blocks
template <class Put>
MOBI_TC_FN void mobi_encp_write_residual(const MobiEncInterConst *K, const MobiEncMb *m, Put put, uint32_t *forms) {
  put(K->inv_cbp_p[m->cbp] + 1u, mobi_enc_ue_bits(K->inv_cbp_p[m->cbp]));
  for (int k = 0; k < 6; k++)
    if ((m->cbp >> k) & 1) mobi_enc_write_block(K, m->lev[k], put, forms);
}
template <class Put>
MOBI_TC_FN void mobi_encp_write_mb(const MobiEncInterConst *K, int ver, const MobiEncMb *m, uint32_t v, uint32_t pred, Put put, uint32_t *forms) {
  const int code = v != pred;
  put(K->part_code[ver][code], K->part_nbits[ver][code]);
  if (code) {
    mobi_encp_put_se(put, mobi_encp_dx(v) - mobi_encp_dx(pred));
    mobi_encp_put_se(put, mobi_encp_dy(v) - mobi_encp_dy(pred));
  }
  mobi_encp_write_residual(K, m, put, forms);
}

// one call's launch arguments (device pointers): the intra call's, with its stats NULL and yuv_format unused, and the inter call's own
struct MobiEncInterArgs : MobiEncArgs {
  const uint8_t *ref;       // n reference pictures, packed I420
  size_t ref_pitch;
  const uint8_t *prev_q;    // [n]
  uint32_t *mv, *mvp;       // [n][mbw * mbh] v* and its predictor (mobi_encp_pack)
  const MobiEncInterConst *kp;
  mobi_enc_inter_stats *pstats; // [n] or NULL
  int32_t ver;
  // the intra mode's side arrays (mobi_encode_pintra.h), carved in every mode and untouched outside it: [n][mbw * mbh] the inter coding's
  // cost Jp, and the macroblock's kind with the chosen coding's figures (mobi_encpi_kind)
  int64_t *jp;
  uint32_t *kind;
};

// where the prediction of the 8x8 block k (0..3 luma, 4: U, 5: V) of a macroblock with vector (dx, dy) starts in its reference plane
struct MobiEncpBlockRef {
  int plane, pitch, x0, y0; // the block itself (mobi_enc_block_at)
  int rx, ry, phase;        // its prediction's corner in the reference plane and the half-pel phase (x: bit 0, y: bit 1)
};
MOBI_TC_FN MobiEncpBlockRef mobi_encp_block_ref(int k, int mbx, int mby, int W, int dx, int dy) {
  const bool chroma = k >= 4;
  const MobiEncBlockAt at = mobi_enc_block_at(chroma, chroma ? k - 4 : k, mbx, mby, W);
  const int vx = chroma ? dx >> 1 : dx, vy = chroma ? dy >> 1 : dy;
  MobiEncpBlockRef b;
  b.plane = at.plane; b.pitch = at.pitch; b.x0 = at.x0; b.y0 = at.y0;
  b.rx = at.x0 + (vx >> 1);
  b.ry = at.y0 + (vy >> 1);
  b.phase = (vx & 1) | (vy & 1) << 1;
  return b;
}
// one predicted sample: the decoder's truncating interpolation (mobi_mc4 on single bytes) at p = the sample's place in the reference
MOBI_TC_FN int mobi_encp_pred_px(const uint8_t *p, int pitch, int phase) {
  return (int)(mobi_mc4(p[0], (phase & 1) ? p[1] : 0u, (phase & 2) ? p[pitch] : 0u, phase == 3 ? p[pitch + 1] : 0u, phase) & 0xFFu);
}

// ---- what needs no device: the refusals and the bound ----
// A macroblock: 3 (the longer partition code) + 2 x 13 (se() of a difference of at most 2 * MOBI_ENCP_REACH) + 13 (ue() of a number below
// 64) + six blocks of 1 + 64 symbols of at most 28 bits; a stream: at most 14 header bits, the macroblocks, 16 zero bits, to the word.
MOBI_TC_FN uint64_t mobi_encp_max_mb_bits() { return 3 + 2 * 13 + 13 + 6 * (1 + 64 * (uint64_t)MOBI_TC_ESCAPE_BITS); }

#if !defined(__HIP_DEVICE_COMPILE__)
static inline size_t mobi_encp_bound(uint32_t width, uint32_t height) {
  if (!mobi_enc_dims_ok(width, height)) return 0;
  const uint64_t bytes = mobi_enc_stream_bytes_h(MOBI_ENCP_MAX_HEADER_BITS, (uint64_t)(width / 16) * (height / 16) * mobi_encp_max_mb_bits());
  return (size_t)((bytes + 3) & ~(uint64_t)3);
}
static inline int mobi_encp_check_args(int max_pictures, uint32_t width, uint32_t height, int version, int n, size_t picture_pitch, size_t ref_pitch,
                                       const uint8_t *prev_quantizers, const uint8_t *quantizers, size_t slot_bytes) {
  const int rc = mobi_enc_check_args(max_pictures, width, height, version, n, picture_pitch, quantizers, 0, slot_bytes);
  if (rc) return rc;
  if (ref_pitch < (size_t)width * height * 3 / 2 || ref_pitch % 8 != 0 || !prev_quantizers) return -7; // MOBI_E_ARG
  for (int i = 0; i < n; i++)
    if (prev_quantizers[i] < MOBI_ENC_QMIN || prev_quantizers[i] > MOBI_ENC_QMAX) return -7;
  return 0;
}

// the constants from the decoder's tables: the reverse of mobi_part_lut at 16x16 as mobi_tc_build_ref reverses the VLC (the first window
// index that reads as the code, cut to the code's length)
static inline void mobi_encp_build_const(MobiEncInterConst *K) {
  memset(K, 0, sizeof *K);
  mobi_enc_build_const(K);
  for (int i = 63; i >= 0; i--) K->inv_cbp_p[mobi_cbp_inter[i]] = (uint8_t)i;
  for (int ver = 0; ver < 2; ver++) {
    const int peek = 32 - mobi_part_shift[ver][0];
    for (int code = 0; code < 2; code++) {
      const int nb = mobi_part_bits[ver][0][code];
      K->part_nbits[ver][code] = (uint8_t)nb;
      for (int i = (1 << peek) - 1; i >= 0; i--)
        if (mobi_part_lut[ver][0][i] == code) K->part_code[ver][code] = (uint8_t)(i >> (peek - nb));
    }
    const int nb6 = mobi_part_bits[ver][0][6];
    K->part6_nbits[ver] = (uint8_t)nb6;
    for (int i = (1 << peek) - 1; i >= 0; i--)
      if (mobi_part_lut[ver][0][i] == 6) K->part6_code[ver] = (uint8_t)(i >> (peek - nb6));
  }
}

// ---- the search of one macroblock, scalar (the host model).  src_y / ref_y: the luma planes at pitch W. ----
static inline uint32_t mobi_encp_luma_sad(const uint8_t *src_y, const uint8_t *ref_y, int W, int mbx, int mby, int dx, int dy) {
  const int phase = (dx & 1) | (dy & 1) << 1;
  const uint8_t *s = src_y + (size_t)(mby * 16) * W + mbx * 16, *r = ref_y + (ptrdiff_t)(mby * 16 + (dy >> 1)) * W + mbx * 16 + (dx >> 1);
  uint32_t sad = 0;
  for (int y = 0; y < 16; y++)
    for (int x = 0; x < 16; x++) {
      const int d = (int)s[y * W + x] - mobi_encp_pred_px(r + y * W + x, W, phase);
      sad += (uint32_t)(d < 0 ? -d : d);
    }
  return sad;
}
static inline uint32_t mobi_encp_search(int q, int W, int H, int mbx, int mby, const uint8_t *src_y, const uint8_t *ref_y) {
  const int64_t lam = mobi_enc_lambda(q);
  uint64_t best = MOBI_ENCP_NO_KEY;
  for (int dy = -MOBI_ENCP_RANGE; dy <= MOBI_ENCP_RANGE; dy += 2)
    for (int dx = -MOBI_ENCP_RANGE; dx <= MOBI_ENCP_RANGE; dx += 2) {
      if (!mobi_encp_vector_ok(W, H, mbx, mby, dx, dy)) continue;
      const uint64_t key = mobi_encp_key(lam, mobi_encp_luma_sad(src_y, ref_y, W, mbx, mby, dx, dy), dx, dy);
      if (key < best) best = key;
    }
  const int fx = mobi_encp_key_dx(best), fy = mobi_encp_key_dy(best); // (0, 0) is always a candidate
  for (int j = -1; j <= 1; j++)
    for (int i = -1; i <= 1; i++) {
      if ((!i && !j) || !mobi_encp_vector_ok(W, H, mbx, mby, fx + i, fy + j)) continue;
      const uint64_t key = mobi_encp_key(lam, mobi_encp_luma_sad(src_y, ref_y, W, mbx, mby, fx + i, fy + j), fx + i, fy + j);
      if (key < best) best = key;
    }
  return mobi_encp_pack(mobi_encp_key_dx(best), mobi_encp_key_dy(best));
}

// ---- one macroblock's prediction and residual, scalar: src / ref / rec point at the pictures' planes ----
static inline void mobi_encp_macroblock(const MobiEncInterConst *K, int q, int W, int mbx, int mby, uint32_t v, const uint8_t *const src[3],
                                        const uint8_t *const ref[3], uint8_t *const rec[3], MobiEncMb *out, MobiEncMbStats *st) {
  memset(out, 0, sizeof *out);
  st->sad = st->coded = st->clamp = st->range = 0;
  for (int k = 0; k < 6; k++) {
    const MobiEncpBlockRef b = mobi_encp_block_ref(k, mbx, mby, W, mobi_encp_dx(v), mobi_encp_dy(v));
    int s[64], p[64], r[64];
    for (int y = 0; y < 8; y++)
      for (int x = 0; x < 8; x++) {
        s[y * 8 + x] = src[b.plane][(size_t)(b.y0 + y) * b.pitch + b.x0 + x];
        p[y * 8 + x] = mobi_encp_pred_px(ref[b.plane] + (ptrdiff_t)(b.ry + y) * b.pitch + b.rx + x, b.pitch, b.phase);
      }
    const MobiEncBlock res = mobi_enc_block(K, q, s, p, out->lev[k], r);
    for (int y = 0; y < 8; y++)
      for (int x = 0; x < 8; x++) rec[b.plane][(size_t)(b.y0 + y) * b.pitch + b.x0 + x] = (uint8_t)r[y * 8 + x];
    out->cbp |= (uint8_t)(res.coded << k);
    out->bits += (uint32_t)res.bits;
    st->sad += (uint32_t)res.sad;
    st->coded += res.coded;
    st->clamp += res.clamp;
    st->range += res.range;
  }
}

// ---- one picture on the CPU: search every macroblock, then predictors, residuals and bits.  rec (W * H * 3 / 2), mbs, mv and mvp
// (macroblocks each) are required; slot is zeroed and filled as the device does.  Returns whether the bits written are the bits priced. ----
static inline bool mobi_encp_picture(const MobiEncInterConst *K, int ver, int W, int H, int prev_q, int q, const uint8_t *i420, const uint8_t *ref_i420,
                                     uint8_t *slot, size_t slot_bytes, int32_t *bytes_out, uint8_t *rec, mobi_enc_inter_stats *stats, MobiEncMb *mbs,
                                     uint32_t *mv, uint32_t *mvp, uint32_t *forms) {
  const size_t ysz = (size_t)W * H;
  const uint8_t *const src[3] = {i420, i420 + ysz, i420 + ysz + ysz / 4};
  const uint8_t *const ref[3] = {ref_i420, ref_i420 + ysz, ref_i420 + ysz + ysz / 4};
  uint8_t *const r3[3] = {rec, rec + ysz, rec + ysz + ysz / 4};
  const int mbw = W / 16, mbh = H / 16;
  mobi_enc_inter_stats st;
  memset(&st, 0, sizeof st);
  for (int y = 0; y < mbh; y++)
    for (int x = 0; x < mbw; x++) mv[y * mbw + x] = mobi_encp_search(q, W, H, x, y, src[0], ref[0]);
  uint64_t mb_bits = 0;
  for (int y = 0; y < mbh; y++)
    for (int x = 0; x < mbw; x++) {
      const int i = y * mbw + x;
      MobiEncMbStats ms;
      mobi_encp_macroblock(K, q, W, x, y, mv[i], src, ref, r3, mbs + i, &ms);
      mvp[i] = mobi_encp_predictor(mv, mbw, x, y);
      const uint32_t vb = mobi_encp_mv_bits(K, ver, mv[i], mvp[i]);
      mbs[i].bits += vb + mobi_encp_cbp_bits(K, mbs[i].cbp);
      mb_bits += mbs[i].bits;
      st.sad += ms.sad;
      st.mv_bits += vb;
      st.coded_blocks += ms.coded;
      st.fallback_clamp += ms.clamp;
      st.fallback_level += ms.range;
      st.code0 += mv[i] == mvp[i];
      st.nonzero_mv += mv[i] != 0;
      st.halfpel_mv += ((mobi_encp_dx(mv[i]) | mobi_encp_dy(mv[i])) & 1) != 0;
    }
  return mobi_enc_finish_picture((uint64_t)mobi_encp_header_bits(q, prev_q), mb_bits, st, stats, slot, slot_bytes, bytes_out, [&](auto put) {
    mobi_encp_write_header(put, q, prev_q);
    for (int i = 0; i < mbw * mbh; i++) mobi_encp_write_mb(K, ver, mbs + i, mv[i], mvp[i], put, forms);
  });
}
#endif
#endif
