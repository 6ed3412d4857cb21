// mobi_encode.h -- the intra encoder's rules (include/mobiclip_encode.h; DESIGN.md, "Intra encoder") that the kernels (mobi_encode.hip), the
// host entry points (mobi_encode.cpp), the host model (mobi_encode_host.cpp) and the CPU tests compile alike.
//
//   cost            J = sum over a trial's blocks of (sad << 8) + lam[q] * bits, 64-bit integers; the argmin with ties to the smaller mode
//   block rule      coded iff some level is nonzero; sent uncoded (reconstruction = prediction, 0 bits) when the reconstruction would
//                   leave the clamp table or some |level| > 2047
//   one block       mobi_enc_block: the arithmetic of mobi_transform_code at n = 8 (mobi_txcode.h), scalar: the host model's; the kernel
//                   runs the same functions eight lanes to a block (mobi_txcode_lanes.h) and shares mobi_enc_block_result's rule
//   one macroblock  mobi_enc_macroblock: three luma and three chroma trials on the decoder's own predictors (mobi_recon_math.h)
//   bit writer      mobi_enc_symbol (one (last, run, level) in the order mobi_tc_cost prices the forms), mobi_enc_write_mb (a macroblock's
//                   bit string into any sink: MobiEncHostSink here, the kernel's word-at-a-time sink in mobi_encode.hip; both put bits
//                   MSB-first into 16-bit little-endian words), mobi_enc_picture (a whole picture on the CPU), mobi_enc_finish_picture
//                   (how a picture ends there, for this encoder and for mobi_encode_inter.h's: length, statistics, slot, sink)
#ifndef MOBI_ENCODE_H
#define MOBI_ENCODE_H
#include <stdint.h>
#include <string.h>

#include "../../include/mobiclip_encode.h"
#include "mobi_recon_math.h"
#include "mobi_txcode.h"

enum { MOBI_ENC_QMIN = 12, MOBI_ENC_QMAX = 52,
       MOBI_ENC_HEADER_BITS = 9,        // 1 (intra), yuv_format, 0 (VLC table 0), quantiser in 6
       MOBI_ENC_TAIL_BITS = 16,         // zero bits behind the last macroblock, then zeros to a 16-bit boundary
       MOBI_ENC_MAX_LEVEL = MOBI_TC_MAX_LEVEL, // the raw escape holds 12 bits, two's complement
       MOBI_ENC_NMODES = 3,
       MOBI_ENC_FORM_OWN = 0, MOBI_ENC_FORM_RUN = 1, MOBI_ENC_FORM_LEVEL = 2, MOBI_ENC_FORM_RAW = 3 };

// candidate k of a trial -> the decoder's mode number: vertical, horizontal, DC
MOBI_TC_FN int mobi_enc_mode(int k) { return k == 2 ? 3 : k; }
// vertical needs the row above the macroblock, horizontal the column to its left: no wrapped or padding read is ever chosen
MOBI_TC_FN bool mobi_enc_mode_allowed(int mode, int mbx, int mby) { return mode == 0 ? mby > 0 : mode == 1 ? mbx > 0 : true; }

// lam[q] = round(256 * 0.85 * 2^((q - 12) / 3)): base {218, 274, 345} doubled every three quantisers (Analyzer.cs:706, rounded once)
MOBI_TC_FN int64_t mobi_enc_lambda(int q) {
  const int k = (q - MOBI_ENC_QMIN) % 3, base = k == 0 ? 218 : k == 1 ? 274 : 345;
  return (int64_t)base << ((q - MOBI_ENC_QMIN) / 3);
}

// what a trial keeps of one block
struct MobiEncBlock {
  int32_t sad, bits; // bits = 1 + the VLC bits when coded, 0 when not
  uint8_t coded, clamp, range;
};
// the block rule on the figures of the transform coding: nz = some level nonzero, clamp = the reconstruction left the clamp table,
// range = some |level| > 2047, vlc_bits / sad_rec = the coded block's, sad_pred = the prediction's
MOBI_TC_FN MobiEncBlock mobi_enc_block_result(bool nz, bool clamp, bool range, int vlc_bits, int sad_rec, int sad_pred) {
  MobiEncBlock b;
  b.clamp = nz && clamp;
  b.range = nz && !clamp && range; // a block counts once: the clamp first
  b.coded = nz && !clamp && !range;
  b.bits = b.coded ? 1 + vlc_bits : 0;
  b.sad = b.coded ? sad_rec : sad_pred;
  return b;
}
MOBI_TC_FN int64_t mobi_enc_cost(int64_t lam, const MobiEncBlock &b) { return ((int64_t)b.sad << 8) + lam * b.bits; }

// per-device constants, built on the host once per encoder (mobi_enc_build_const): the transform coding's (mobi_tc_build_const: Q rows,
// reciprocals, scan orders, the cost table) as the base, so that the block coder takes the same pointer, and the bit writer's behind them
struct MobiEncConst : MobiTcConst {
  uint32_t code[2 * 64 * 32]; // [(last * 64 + run) * 32 + v]: length << 16 | the code word with a positive sign; 0 = the pair has none
  uint8_t esc[256];           // mobi_vx2table0_b
  uint8_t inv_cbp[64];        // the ue() number whose mobi_cbp_intra entry is cbp6
};

// ---- small rules the host model and the kernels or their launcher share ----
// the length of ue(code): z zeros, a one, z more bits of code + 1 (BitWriter.WriteVarIntUnsigned)
MOBI_TC_FN int mobi_enc_ue_bits(uint32_t code) { return 2 * (31 - __builtin_clz(code + 1u)) + 1; }
// a macroblock's bits in front of its blocks: 0 (the full-block syntax), ue(cbp), two 3-bit modes
MOBI_TC_FN uint32_t mobi_enc_mb_header_bits(const MobiEncConst *K, uint32_t cbp) { return 1u + (uint32_t)mobi_enc_ue_bits(K->inv_cbp[cbp]) + 6u; }
// macroblocks of anti-diagonal d: x from max(0, d - mbh + 1) to min(d, mbw - 1), y = d - x
MOBI_TC_FN void mobi_enc_diag_range(int mbw, int mbh, int d, int *x_lo, int *count) {
  *x_lo = d - mbh + 1 > 0 ? d - mbh + 1 : 0;
  const int x_hi = d < mbw - 1 ? d : mbw - 1;
  *count = x_hi - *x_lo + 1;
}
// where block k of a macroblock's luma (k = 0..3) or chroma (k = 0: U, 1: V) lies: plane 0..2 of the I420 picture, its pitch, the corner
struct MobiEncBlockAt {
  int plane, pitch, x0, y0;
};
MOBI_TC_FN MobiEncBlockAt mobi_enc_block_at(bool chroma, int k, int mbx, int mby, int W) {
  MobiEncBlockAt a;
  a.plane = chroma ? 1 + k : 0;
  a.pitch = chroma ? W / 2 : W;
  a.x0 = chroma ? mbx * 8 : mbx * 16 + (k & 1) * 8;
  a.y0 = chroma ? mby * 8 : mby * 16 + (k >> 1) * 8;
  return a;
}

// one macroblock as stage 1 leaves it for the bit writer
struct MobiEncMb {
  int16_t lev[6][64]; // Y0..Y3, U, V in scan order (of coded blocks; zeros elsewhere)
  uint32_t bits;      // the macroblock's length in the stream
  uint8_t luma_mode, chroma_mode, cbp, pad;
};

// one call's launch arguments (device pointers)
struct MobiEncArgs {
  const uint8_t *src;      // n pictures, packed I420
  size_t src_pitch;
  uint8_t *rec;            // n reconstructions at pitch W * H * 3 / 2
  MobiEncMb *mbs;          // [n][mbw * mbh]
  uint32_t *mb_off;        // [n][mbw * mbh] bit offset of every macroblock in its stream
  uint32_t *fits;          // [n] the stream fits its slot
  const uint8_t *q;        // [n]
  const MobiEncConst *k;
  mobi_enc_stats *stats;   // [n] or NULL
  uint8_t *streams;
  size_t slot_bytes;
  int32_t *bytes_out;
  int32_t W, H, mbw, mbh, n, yuv_format;
};

// ---- one symbol: pattern (right-aligned) and length, forms tried in mobi_tc_cost's order.  v = |level| in [1, 2047]. ----
MOBI_TC_FN uint32_t mobi_enc_symbol(const MobiEncConst *K, int level, int run, int last, int *nbits, int *form) {
  const int v = level < 0 ? -level : level;
  const uint32_t neg = level < 0;
  const uint32_t *row = K->code + (last * 64) * 32;
  uint32_t c;
  if (v <= 31) {
    if ((c = row[run * 32 + v]) != 0) { *nbits = (int)(c >> 16); *form = MOBI_ENC_FORM_OWN; return (c & 0xFFFF) | neg; }
    const int s2 = run - K->esc[(v | last << 6) + 0x80];
    if (s2 >= 0 && (c = row[s2 * 32 + v]) != 0) { // 0000011 10, then the code of the shorter run
      const int n = (int)(c >> 16);
      *nbits = 9 + n; *form = MOBI_ENC_FORM_RUN;
      return 14u << n | (c & 0xFFFF) | neg;
    }
  }
  const int v2 = v - K->esc[run | last << 6];
  if (v2 >= 1 && v2 <= 31 && (c = row[run * 32 + v2]) != 0) { // 0000011 0, then the code of the smaller value
    const int n = (int)(c >> 16);
    *nbits = 8 + n; *form = MOBI_ENC_FORM_LEVEL;
    return 6u << n | (c & 0xFFFF) | neg;
  }
  *nbits = MOBI_TC_ESCAPE_BITS; *form = MOBI_ENC_FORM_RAW; // 0000011 11 last(1) run(6) level(12)
  return 15u << 19 | (uint32_t)last << 18 | (uint32_t)run << 12 | ((uint32_t)level & 0xFFF);
}

// ---- one coded block's bit string: 1 (one 8x8 transform), then its symbols; lev = 64 levels in scan order, some nonzero ----
template <class Put>
MOBI_TC_FN void mobi_enc_write_block(const MobiEncConst *K, const int16_t *lev, Put put, uint32_t *forms) {
  put(1u, 1); // one 8x8 transform
  int lastpos = 0;
  for (int p = 0; p < 64; p++)
    if (lev[p]) lastpos = p;
  int prev = -1;
  for (int p = 0; p <= lastpos; p++) {
    const int lv = lev[p];
    if (!lv) continue;
    int n, form;
    const uint32_t bits = mobi_enc_symbol(K, lv, p - prev - 1, p == lastpos, &n, &form);
    put(bits, n);
    if (forms) forms[form]++;
    prev = p;
  }
}
// ---- a macroblock's bit string: put(pattern, nbits) with nbits <= 28; forms[4] (may be NULL) counts the code forms written ----
// what follows the bit(s) that say "an intra macroblock in the full-block syntax" (an I-frame's leading 0 below, a P-frame's partition
// code 6 in mobi_encode_pintra.h): ue(cbp), the modes in front of their blocks, the coded blocks
template <class Put>
MOBI_TC_FN void mobi_enc_write_mb_body(const MobiEncConst *K, const MobiEncMb *m, Put put, uint32_t *forms) {
  put(K->inv_cbp[m->cbp] + 1u, mobi_enc_ue_bits(K->inv_cbp[m->cbp])); // ue(): the leading zeros are the pattern's own
  for (int k = 0; k < 6; k++) {
    if (k == 0) put(m->luma_mode, 3);
    if (k == 4) put(m->chroma_mode, 3);
    if ((m->cbp >> k) & 1) mobi_enc_write_block(K, m->lev[k], put, forms);
  }
}
template <class Put>
MOBI_TC_FN void mobi_enc_write_mb(const MobiEncConst *K, const MobiEncMb *m, Put put, uint32_t *forms) {
  put(0u, 1); // the full-block syntax
  mobi_enc_write_mb_body(K, m, put, forms);
}

// ---- the sink of the host model: bits MSB-first into 16-bit little-endian words of a zeroed buffer, at bit position pos ----
struct MobiEncHostSink {
  uint8_t *buf;
  uint64_t pos;
  void operator()(uint32_t v, int n) {
    for (int i = n - 1; i >= 0; i--, pos++)
      if ((v >> i) & 1) buf[(pos >> 4) * 2 + (((pos >> 3) & 1) ^ 1)] |= (uint8_t)(0x80 >> (pos & 7));
  }
};
MOBI_TC_FN uint32_t mobi_enc_header(int yuv_format, int q) { return 1u << 8 | (uint32_t)(yuv_format & 1) << 7 | (uint32_t)q; }
// a stream's bytes from its header's bits and the sum of its macroblocks' bits (an I-frame's header is MOBI_ENC_HEADER_BITS long)
MOBI_TC_FN uint64_t mobi_enc_stream_bytes_h(uint64_t header_bits, uint64_t mb_bits) {
  return (header_bits + mb_bits + MOBI_ENC_TAIL_BITS + 15) / 16 * 2;
}
MOBI_TC_FN uint64_t mobi_enc_stream_bytes(uint64_t mb_bits) { return mobi_enc_stream_bytes_h(MOBI_ENC_HEADER_BITS, mb_bits); }

// ---- one block, scalar: src / pred 8x8 row-major; lev = levels in scan order, rec = the block's reconstruction under the rule ----
MOBI_TC_FN MobiEncBlock mobi_enc_block(const MobiEncConst *K, int q, const int *src, const int *pred, int16_t *lev, int *rec) {
  int t[64], d[64], x[8], o[8], nat[64];
  for (int r = 0; r < 8; r++) { // rows of the residual x 64
    for (int k = 0; k < 8; k++) x[k] = (src[r * 8 + k] - pred[r * 8 + k]) * 64;
    mobi_dct8_pass(x, o);
    for (int k = 0; k < 8; k++) t[r * 8 + k] = o[k];
  }
  for (int r = 0; r < 8; r++) { // columns: natural coefficients r * 8 + k
    for (int j = 0; j < 8; j++) x[j] = t[j * 8 + r];
    mobi_dct8_pass(x, o);
    for (int k = 0; k < 8; k++) d[r * 8 + k] = o[k];
  }
  bool range = false;
  for (int r = 0; r < 8; r++) { // quantise, first inverse pass, stored transposed
    for (int k = 0; k < 8; k++) {
      const int Q = K->q8[q][r * 8 + k], l = mobi_tc_quant(d[r * 8 + k], Q, K->rq8[q][r * 8 + k]);
      nat[r * 8 + k] = l;
      range |= l > MOBI_ENC_MAX_LEVEL || l < -MOBI_ENC_MAX_LEVEL;
      x[k] = l * Q;
    }
    if (r == 0) x[0] += 0x20;
    mobi_bfly8(x, o);
    for (int k = 0; k < 8; k++) t[k * 8 + r] = o[k];
  }
  int vlc = 0, prev = -1, lastpos = -1;
  for (int p = 0; p < 64; p++) {
    lev[p] = (int16_t)nat[K->zz8[p]]; // |level| <= 23500 / 4 fits (tests/test_txcode.py, the DCT bound)
    if (nat[K->zz8[p]]) lastpos = p;
  }
  for (int p = 0; p <= lastpos; p++) {
    const int l = nat[K->zz8[p]];
    if (!l) continue;
    const int v = l < 0 ? -l : l;
    vlc += v < MOBI_TC_LUT_V ? K->lut[mobi_tc_lut_index(v, p - prev - 1, p == lastpos)] : MOBI_TC_ESCAPE_BITS;
    prev = p;
  }
  int sad_rec = 0, sad_pred = 0;
  int clamp = 0;
  for (int r = 0; r < 8; r++) {
    for (int j = 0; j < 8; j++) x[j] = t[r * 8 + j];
    mobi_bfly8(x, o);
    for (int k = 0; k < 8; k++) {
      const int s = src[r * 8 + k], p = pred[r * 8 + k];
      rec[r * 8 + k] = mobi_add_clamp(p, o[k] >> 6, &clamp);
      sad_rec += s > rec[r * 8 + k] ? s - rec[r * 8 + k] : rec[r * 8 + k] - s;
      sad_pred += s > p ? s - p : p - s;
    }
  }
  const MobiEncBlock b = mobi_enc_block_result(lastpos >= 0, clamp != 0, range, vlc, sad_rec, sad_pred);
  if (!b.coded)
    for (int i = 0; i < 64; i++) { rec[i] = pred[i]; lev[i] = 0; }
  return b;
}

// what a macroblock adds to its picture's statistics (mobi_enc_stats without the bit total)
struct MobiEncMbStats {
  uint32_t sad, coded, clamp, range;
};

// ---- one macroblock, scalar (the host model).  src_* / rec_* point at the picture's planes (pitch W for Y, W / 2 for U and V); the
// reconstruction of the macroblocks above and to the left is in rec_* already, this one's is written there. ----
#if !defined(__HIP_DEVICE_COMPILE__)
static inline void mobi_enc_macroblock(const MobiEncConst *K, int q, int W, int mbx, int mby, const uint8_t *const src[3], uint8_t *const rec[3],
                                       MobiEncMb *out, MobiEncMbStats *st) {
  const int64_t lam = mobi_enc_lambda(q);
  memset(out, 0, sizeof *out);
  st->sad = st->coded = st->clamp = st->range = 0;
  for (int chroma = 0; chroma < 2; chroma++) {
    const int nb = chroma ? 2 : 4;
    int64_t bestJ = 0;
    int best = -1;
    int brec[4][64];
    int16_t blev[4][64];
    MobiEncBlock bres[4];
    for (int c = 0; c < MOBI_ENC_NMODES; c++) {
      const int mode = mobi_enc_mode(c);
      if (!mobi_enc_mode_allowed(mode, mbx, mby)) continue;
      int trec[4][64];
      int16_t tlev[4][64];
      MobiEncBlock tres[4];
      int64_t J = 0;
      for (int k = 0; k < nb; k++) {
        const MobiEncBlockAt at = mobi_enc_block_at(chroma, k, mbx, mby, W);
        const int plane = at.plane, pitch = at.pitch, x0 = at.x0, y0 = at.y0;
        // neighbours: earlier blocks of this trial first, the picture's reconstruction elsewhere
        auto nbr = [&](int dy, int dx) -> int {
          const int y = y0 + dy, x = x0 + dx;
          if (!chroma)
            for (int e = 0; e < k; e++) {
              const int ex = mbx * 16 + (e & 1) * 8, ey = mby * 16 + (e >> 1) * 8;
              if (x >= ex && x < ex + 8 && y >= ey && y < ey + 8) return trec[e][(y - ey) * 8 + (x - ex)];
            }
          return rec[plane][(size_t)y * pitch + x];
        };
        int s[64], p[64];
        for (int y = 0; y < 8; y++)
          for (int x = 0; x < 8; x++) {
            s[y * 8 + x] = src[plane][(size_t)(y0 + y) * pitch + x0 + x];
            p[y * 8 + x] = mobi_pred_px(mode, 8, y, x, y0 != 0, x0 != 0, nbr);
          }
        tres[k] = mobi_enc_block(K, q, s, p, tlev[k], trec[k]);
        J += mobi_enc_cost(lam, tres[k]);
      }
      if (best < 0 || J < bestJ) { // candidates run in mode order: a tie keeps the smaller mode
        best = mode;
        bestJ = J;
        memcpy(brec, trec, sizeof brec);
        memcpy(blev, tlev, sizeof blev);
        memcpy(bres, tres, sizeof bres);
      }
    }
    (chroma ? out->chroma_mode : out->luma_mode) = (uint8_t)best;
    for (int k = 0; k < nb; k++) {
      const int a = chroma ? 4 + k : k;
      const MobiEncBlockAt at = mobi_enc_block_at(chroma, k, mbx, mby, W);
      for (int y = 0; y < 8; y++)
        for (int x = 0; x < 8; x++) rec[at.plane][(size_t)(at.y0 + y) * at.pitch + at.x0 + x] = (uint8_t)brec[k][y * 8 + x];
      memcpy(out->lev[a], blev[k], sizeof blev[k]);
      out->cbp |= (uint8_t)(bres[k].coded << a);
      out->bits += (uint32_t)bres[k].bits;
      st->sad += (uint32_t)bres[k].sad;
      st->coded += bres[k].coded;
      st->clamp += bres[k].clamp;
      st->range += bres[k].range;
    }
  }
  out->bits += mobi_enc_mb_header_bits(K, out->cbp);
}

// the constants from the decoder's tables
static inline void mobi_enc_build_const(MobiEncConst *K) {
  memset(K, 0, sizeof *K);
  mobi_tc_build_const(K);
  int16_t ref[32 * 64 * 2];
  mobi_tc_build_ref(ref);
  // the code word of table index j (the reader's 12-bit window) with length nb, sign included: the window's top nb bits, where the first j
  // of a word has the sign bit clear; a 13-bit word is the whole window and the sign behind it.
  // v = 0 is left out: its only entry is index 0, which no reader can tell from what follows it, and no (v, run, last) reaches it
  // (tests/test_encode_model.py walks them all)
  for (int last = 0; last < 2; last++)
    for (int run = 0; run < 64; run++)
      for (int v = 1; v < 32; v++) {
        const int j = ref[(v * 64 + run) * 2 + last];
        if (j < 0) continue;
        const uint32_t nb = mobi_vx2table0_a[j] & 0xF;
        K->code[(last * 64 + run) * 32 + v] = nb << 16 | (nb <= 12 ? (uint32_t)j >> (12 - nb) : (uint32_t)j << (nb - 12));
      }
  memcpy(K->esc, mobi_vx2table0_b, sizeof K->esc);
  for (int i = 63; i >= 0; i--) K->inv_cbp[mobi_cbp_intra[i]] = (uint8_t)i;
}
// ---- what needs no device: the refusals and the bound (include/mobiclip_encode.h states both) ----
static inline bool mobi_enc_dims_ok(uint32_t width, uint32_t height) {
  return width >= 16 && height >= 16 && width % 16 == 0 && height % 16 == 0 && width <= 1024 && height <= 16384;
}
// A macroblock: 1 (full-block syntax) + 13 (ue() of a number below 64) + 3 + 3 (modes) + six blocks of 1 + 64 symbols of at most 28 bits
// (the raw escape is the longest form); a stream: 9 header bits, the macroblocks, 16 zero bits, below 16 bits to the word boundary.
static inline size_t mobi_enc_bound(uint32_t width, uint32_t height) {
  if (!mobi_enc_dims_ok(width, height)) return 0;
  const uint64_t mb_bits = 1 + 13 + 6 + 6 * (1 + 64 * (uint64_t)MOBI_TC_ESCAPE_BITS);
  const uint64_t bytes = mobi_enc_stream_bytes((uint64_t)(width / 16) * (height / 16) * mb_bits);
  return (size_t)((bytes + 3) & ~(uint64_t)3);
}
static inline int mobi_enc_check_args(int max_pictures, uint32_t width, uint32_t height, int version, int n, size_t picture_pitch,
                                      const uint8_t *quantizers, int yuv_format, size_t slot_bytes) {
  if (version != 1 && version != 2) return -4; // MOBI_E_VERSION: MOBI_VERSION_MODSDS, MOBI_VERSION_MOFLEX3DS
  // (pictures are one grid dimension of the kernels: at most 65535)
  if (!mobi_enc_dims_ok(width, height) || max_pictures < 1 || max_pictures > 65535 || n < 1 || n > max_pictures) return -7; // MOBI_E_ARG
  if (picture_pitch < (size_t)width * height * 3 / 2 || picture_pitch % 8 != 0 || !quantizers) return -7;
  for (int i = 0; i < n; i++)
    if (quantizers[i] < MOBI_ENC_QMIN || quantizers[i] > MOBI_ENC_QMAX) return -7;
  if ((yuv_format != 0 && yuv_format != 1) || slot_bytes % 4 != 0) return -7;
  return 0;
}

// ---- how a picture on the CPU ends, for either encoder (st: mobi_enc_stats or mobi_enc_inter_stats), once its macroblocks are priced:
// the length from the header's and the macroblocks' bits, the statistics handed out, the slot zeroed as the device does and, if the
// stream fits, filled by write(put): header, then macroblocks.  Returns whether the bits written are the bits priced. ----
template <class Stats, class Write>
static inline bool mobi_enc_finish_picture(uint64_t header_bits, uint64_t mb_bits, Stats &st, Stats *stats, uint8_t *slot, size_t slot_bytes,
                                           int32_t *bytes_out, Write write) {
  st.bits = header_bits + mb_bits;
  const uint64_t bytes = mobi_enc_stream_bytes_h(header_bits, mb_bits);
  *bytes_out = (int32_t)bytes;
  if (stats) *stats = st;
  memset(slot, 0, slot_bytes);
  if (bytes > slot_bytes) return true;
  MobiEncHostSink sink{slot, 0};
  write([&](uint32_t v, int n) { sink(v, n); });
  return sink.pos == header_bits + mb_bits;
}

// ---- one picture on the CPU: the whole encoder in raster order.  rec (W * H * 3 / 2) and mbs (macroblocks) are required; forms[4] may
// be NULL.  Returns what mobi_enc_finish_picture returns. ----
static inline bool mobi_enc_picture(const MobiEncConst *K, int W, int H, int q, int yuv_format, const uint8_t *i420, uint8_t *slot, size_t slot_bytes,
                                    int32_t *bytes_out, uint8_t *rec, mobi_enc_stats *stats, MobiEncMb *mbs, uint32_t *forms) {
  const size_t ysz = (size_t)W * H;
  const uint8_t *const src[3] = {i420, i420 + ysz, i420 + ysz + ysz / 4};
  uint8_t *const r3[3] = {rec, rec + ysz, rec + ysz + ysz / 4};
  const int mbw = W / 16, mbh = H / 16;
  mobi_enc_stats st;
  memset(&st, 0, sizeof st);
  uint64_t mb_bits = 0;
  for (int y = 0; y < mbh; y++)
    for (int x = 0; x < mbw; x++) {
      MobiEncMb *m = mbs + (size_t)y * mbw + x;
      MobiEncMbStats ms;
      mobi_enc_macroblock(K, q, W, x, y, src, r3, m, &ms);
      mb_bits += m->bits;
      st.sad += ms.sad;
      st.luma_modes[m->luma_mode]++;
      st.chroma_modes[m->chroma_mode]++;
      st.coded_blocks += ms.coded;
      st.fallback_clamp += ms.clamp;
      st.fallback_level += ms.range;
    }
  return mobi_enc_finish_picture(MOBI_ENC_HEADER_BITS, mb_bits, st, stats, slot, slot_bytes, bytes_out, [&](auto put) {
    put(mobi_enc_header(yuv_format, q), MOBI_ENC_HEADER_BITS);
    for (int i = 0; i < mbw * mbh; i++) mobi_enc_write_mb(K, mbs + i, put, forms);
  });
}
#endif
#endif
