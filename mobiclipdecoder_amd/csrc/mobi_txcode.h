// mobi_txcode.h -- the integer parts of the encoder's transform coding (include/mobiclip_hip.h, mobi_transform_code) that the kernel
// (mobi_txcode.hip), the host side (mobi_txcode.cpp) and the CPU tests (tests/test_txcode.py) compile alike.
//
//   forward transforms   MobiEncoder.DCT64 / DCT16 (Encoder/MobiEncoder.cs:962-1010, 1146-1178): one pass over a row or a column
//                        (mobi_forward_dct and mobi_transform_code share them)
//   inverse transforms   MobiEncoder.IDCT64 / IDCT16 (:1012-1144, 1180-1240): the decoder's butterflies and clamp (mobi_recon_math.h)
//   quantise             (int)Math.Round(dct / QTable) (Encoder/MacroBlock.cs:591-595, 612-616): round half to even of an exact
//                        integer quotient (why that is what the reference computes: DESIGN.md, "Transform coding")
//   bit cost             CalculateNrBitsDCT(EncodeDct, 0) (MobiEncoder.cs:767-858) of one coefficient, and the [2][64][44] table of it
//   table builders       SetupQuantizationTables (MobiEncoder.cs:930-960); the encoder's reverse VLC table VxTable0_A_Ref derived from
//                        mobi_vx2table0_a (host only: they read mobi_tables.h)
#ifndef MOBI_TXCODE_H
#define MOBI_TXCODE_H
#include <stdint.h>

#include "mobi_recon_math.h"

#if defined(__HIPCC__)
#define MOBI_TC_FN static __host__ __device__ __forceinline__
#else
#define MOBI_TC_FN static inline
#endif

enum { MOBI_TC_NQ = 54,                 // quantisers 0..53
       MOBI_TC_LUT_V = 44,              // |level| >= 44 always costs 28 bits: max mobi_vx2table0_b[0..127] = 12, so v - B <= 31 needs v <= 43
       MOBI_TC_LUT_BYTES = 2 * 64 * MOBI_TC_LUT_V,
       MOBI_TC_ESCAPE_BITS = 28,        // the fallback of :847-853: 7 + 1 + 1 + 1 + 6 + 12
       MOBI_TC_MAX_LEVEL = 2047 };      // what those 12 bits hold, two's complement

// ---- forward transforms: x = samples 0..7 (0..3) of one row or column, already x64 in the first pass ----
MOBI_TC_FN void mobi_dct8_pass(const int (&x)[8], int (&o)[8]) {
  const int p = x[0], q = x[7], r = x[2], s = x[5], t = x[3], u = x[4], v = x[1], w = x[6];
  o[0] = (w + v + u + t + s + r + q + p) / 8;
  o[1] = (-40 * w + 40 * v - 12 * u + 12 * t - 24 * s + 24 * r - 48 * q + 48 * p) / 289;
  o[2] = (w + v - 2 * u - 2 * t - s - r + 2 * q + 2 * p) / 10;
  o[3] = (12 * w - 12 * v + 24 * u - 24 * t + 48 * s - 48 * r - 40 * q + 40 * p) / 289;
  o[4] = (-w - v + u + t - s - r + q + p) / 8;
  o[5] = (48 * w - 48 * v - 40 * u + 40 * t - 12 * s + 12 * r - 24 * q + 24 * p) / 289;
  o[6] = (-2 * w - 2 * v - u - t + 2 * s + 2 * r + q + p) / 10;
  o[7] = (24 * w - 24 * v + 48 * u - 48 * t - 40 * s + 40 * r - 12 * q + 12 * p) / 289;
}
MOBI_TC_FN void mobi_dct4_pass(const int (&x)[4], int (&o)[4]) {
  const int q = x[0], r = x[1], s = x[2], t = x[3];
  o[0] = (t + s + r + q) / 4;
  o[1] = (-2 * t - s + r + 2 * q) / 5;
  o[2] = (t - s - r + q) / 4;
  o[3] = (-t + 2 * s - 2 * r + q) / 5;
}

// ---- inverse transforms, one 1-D pass: mobi_bfly8 / mobi_bfly4 of mobi_recon_math.h.  MobiEncoder.IDCT64 / IDCT16 are the decoder's
// butterflies term for term (one was written from the reference's encoder, the other from its decoder).  The reference runs the pass
// over the rows of the coefficients (the DC row with + 0x20, :1024), stores the results transposed, runs it again over the rows of that
// and adds (result >> 6) to the prediction (:1119-1126) through the clamp table: mobi_add_clamp. ----

// ---- quantise: round_half_even(d / Q), Q an integer in [4, 7424].  rq is any float within a few ulps of 1 / Q (the host table holds
// 1.0f / Q): |d| * rq is then within 2^-10 of |d| / Q for |d| < 2^15, so its truncation is floor(|d| / Q) or one off, and the remainder
// puts it right.  Exact integer arithmetic from there on: a tie (remainder exactly Q / 2) goes to the even quotient, as Math.Round does.
// tests/test_txcode.py checks it against float32 division + round-half-even for every Q and every |d| <= 40 000. ----
MOBI_TC_FN int mobi_tc_quant(int d, int Q, float rq) {
  const int a = d < 0 ? -d : d;
  int q = (int)((float)a * rq), r = a - q * Q;
  if (r < 0) { q--; r += Q; }
  else if (r >= Q) { q++; r -= Q; }
  q += (2 * r > Q) | ((2 * r == Q) & q);
  return d < 0 ? -q : q;
}

// ---- bit cost of one nonzero level of |value| v (>= 1) after `skip` zeros; last = it is the block's last nonzero level.  The cases of
// CalculateNrBitsDCT (:787-853) on the reverse table ref[(v * 64 + skip) * 2 + last] (VxTable0_A_Ref), code length nb(j) = A[j] & 0xF. ----
MOBI_TC_FN int mobi_tc_cost(const int16_t *ref, const uint16_t *A, const uint8_t *B, int v, int skip, int last) {
  if (v <= 31) {
    int j = ref[(v * 64 + skip) * 2 + last];
    if (j >= 0) return A[j] & 0xF;                                        // the pair has a code of its own (:790-803)
    const int s2 = skip - B[(v | last << 6) + 0x80];                      // shorter run, 9 bits of escape (:804-824)
    if (s2 >= 0 && (j = ref[(v * 64 + s2) * 2 + last]) >= 0) return 9 + (A[j] & 0xF);
  }
  const int v2 = v - B[skip | last << 6];                                 // smaller value, 8 bits of escape (:826-845)
  if (v2 >= 0 && v2 <= 31) {
    const int j = ref[(v2 * 64 + skip) * 2 + last];
    if (j >= 0) return 8 + (A[j] & 0xF);
  }
  return MOBI_TC_ESCAPE_BITS;
}
// the table the kernel reads: lut[(last * 64 + skip) * MOBI_TC_LUT_V + v], v < 44 (entry v = 0 unused)
MOBI_TC_FN int mobi_tc_lut_index(int v, int skip, int last) { return (last * 64 + skip) * MOBI_TC_LUT_V + v; }

// per-device constants, built on the host once (mobi_txcode.cpp) and uploaded once: Q rows of every quantiser (natural order) with their
// reciprocals, the scan orders, the cost table
struct MobiTcConst {
  int32_t q8[MOBI_TC_NQ][64];
  float rq8[MOBI_TC_NQ][64];
  int32_t q4[MOBI_TC_NQ][16];
  float rq4[MOBI_TC_NQ][16];
  uint8_t zz8[64], zz4[16];
  uint8_t lut[MOBI_TC_LUT_BYTES];
};
// one launch: n_blocks blocks x n_q quantisers q[0 .. n_q); entry e = qi * n_blocks + b (levels, recon, sad may be NULL)
struct MobiTcArgs {
  const uint8_t *src, *pred;
  int16_t *levels;
  uint8_t *recon;
  int32_t *bits, *sad;
  uint8_t *flags;
  const MobiTcConst *k;
  uint32_t n_blocks;
  int32_t n_q;
  uint8_t q[MOBI_TC_NQ];
};

#if !defined(__HIP_DEVICE_COMPILE__)
#include <string.h>

#include "mobi_tables.h"

// VxTable0_A_Ref[v][skip][last] (MobiConst.cs, 32 x 64 x 2): the first j whose code word in mobi_vx2table0_a says value v, skip, last
// ((A[j] & 0xFFF0) == v << 4 | skip << 9 | last << 15), else -1 -- the derivation the reference's own tool uses (MobiclipDecoder/Form1.cs:47-64)
static inline void mobi_tc_build_ref(int16_t *ref) {
  for (int i = 0; i < 32 * 64 * 2; i++) ref[i] = -1;
  for (int j = 4095; j >= 0; j--) { // downwards: the first j wins
    const int w = mobi_vx2table0_a[j] & 0xFFF0, v = (w >> 4) & 31, skip = (w >> 9) & 63, last = w >> 15;
    ref[(v * 64 + skip) * 2 + last] = (int16_t)j;
  }
}
static inline void mobi_tc_build_lut(uint8_t *lut) {
  int16_t ref[32 * 64 * 2];
  mobi_tc_build_ref(ref);
  for (int last = 0; last < 2; last++)
    for (int skip = 0; skip < 64; skip++)
      for (int v = 0; v < MOBI_TC_LUT_V; v++)
        lut[mobi_tc_lut_index(v, skip, last)] = (uint8_t)(v ? mobi_tc_cost(ref, mobi_vx2table0_a, mobi_vx2table0_b, v, skip, last) : 0);
}
// SetupQuantizationTables (:930-960) for quantiser q: Q[natural index] of the n x n table (the reference's float[] holds these integers)
static inline void mobi_tc_qtable(int q, int n, int32_t *Q) {
  const int sh = mobi_qdiv6[q] + (n == 4 ? 8 : 6), m = mobi_qmod6[q];
  for (int k = 0; k < n * n; k++) Q[n == 4 ? mobi_zz4[k] : mobi_zz8[k]] = (n == 4 ? mobi_dq4[m * 16 + k] : mobi_dq8[m * 64 + k]) << sh >> 8;
}
// the constants from the decoder's tables
static inline void mobi_tc_build_const(MobiTcConst *K) {
  for (int q = 0; q < MOBI_TC_NQ; q++) {
    mobi_tc_qtable(q, 8, K->q8[q]);
    mobi_tc_qtable(q, 4, K->q4[q]);
    for (int i = 0; i < 64; i++) K->rq8[q][i] = 1.0f / (float)K->q8[q][i];
    for (int i = 0; i < 16; i++) K->rq4[q][i] = 1.0f / (float)K->q4[q][i];
  }
  memcpy(K->zz8, mobi_zz8, sizeof K->zz8);
  memcpy(K->zz4, mobi_zz4, sizeof K->zz4);
  mobi_tc_build_lut(K->lut);
}
#endif
#endif
