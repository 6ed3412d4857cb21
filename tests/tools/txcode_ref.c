/* txcode_ref.c -- TEST TOOL: a plain scalar restatement of the encoder's transform coding, the yardstick of mobi_transform_code
 * (tests/test_txcode.py builds it with gcc into a shared library).  Written from the reference's encoder, statement group by statement
 * group, and deliberately NOT from the product's mobi_txcode.h: the forward transforms as coefficient matrices, the quantiser as the
 * float division + Math.Round the reference performs, the bit count as the literal branches of CalculateNrBitsDCT over the reference's
 * own reverse table VxTable0_A_Ref (passed in: tests/golden/encoder_vlc_ref.npy), the clamp as a bounds-checked table read.
 * Only the codec's constant tables come from the product (mobi_tables.h). */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "mobi_tables.h"

/* MobiEncoder.SetupQuantizationTables (Encoder/MobiEncoder.cs:930-960).  byte_119004 = mobi_qdiv6, byte_11903A = mobi_qmod6,
 * byte_118F94 = mobi_dq4, byte_118DD4 = mobi_dq8, DeZigZagTable4x4 / 8x8 = mobi_zz4 / mobi_zz8. */
void ref_qtables(int quantizer, float *qt4, float *qt8) {
  float table[64];
  int shift = mobi_qdiv6[quantizer] + 8, base = mobi_qmod6[quantizer] << 4;
  for (int i = 0; i < 16; i++) table[i] = (float)((mobi_dq4[base + i] << shift) >> 8);
  for (int i = 0; i < 16; i++) qt4[mobi_zz4[i]] = table[i];
  shift -= 2;
  base = mobi_qmod6[quantizer] << 6;
  for (int i = 0; i < 64; i++) table[i] = (float)((mobi_dq8[base + i] << shift) >> 8);
  for (int i = 0; i < 64; i++) qt8[mobi_zz8[i]] = table[i];
}

/* DCT64 (:962-1010) and DCT16 (:1146-1178): every output of a pass is one integer row of weights against the 8 (4) inputs, then one
 * truncating division.  Rows first (pixels x 64), then columns, and the column results land in row `column`. */
static const int W8[8][8] = {{1, 1, 1, 1, 1, 1, 1, 1},         {48, 40, 24, 12, -12, -24, -40, -48}, {2, 1, -1, -2, -2, -1, 1, 2},
                             {40, -12, -48, -24, 24, 48, 12, -40}, {1, -1, -1, 1, 1, -1, -1, 1},        {24, -48, 12, 40, -40, -12, 48, -24},
                             {1, -2, 2, -1, -1, 2, -2, 1},        {12, -24, 40, -48, 48, -40, 24, -12}};
static const int D8[8] = {8, 289, 10, 289, 8, 289, 10, 289};
static const int W4[4][4] = {{1, 1, 1, 1}, {2, 1, -1, -2}, {1, -1, -1, 1}, {1, -2, 2, -1}};
static const int D4[4] = {4, 5, 4, 5};

void ref_dct(int n, const int32_t *in, int32_t *out) {
  int32_t tmp[64];
  for (int i = 0; i < n; i++)
    for (int u = 0; u < n; u++) {
      int acc = 0;
      for (int j = 0; j < n; j++) acc += (n == 8 ? W8[u][j] : W4[u][j]) * (in[i * n + j] * 64);
      tmp[i * n + u] = acc / (n == 8 ? D8[u] : D4[u]);
    }
  for (int i = 0; i < n; i++)
    for (int u = 0; u < n; u++) {
      int acc = 0;
      for (int j = 0; j < n; j++) acc += (n == 8 ? W8[u][j] : W4[u][j]) * tmp[j * n + i];
      out[i * n + u] = acc / (n == 8 ? D8[u] : D4[u]);
    }
}

/* IDCT64 (:1012-1144) / IDCT16 (:1180-1240): the 1-D butterfly (arithmetic shifts), first over the coefficient rows -- + 0x20 on the very
 * first coefficient -- with the results written down a column, then over the rows of that, each result >> 6 added to the prediction
 * through Vx2MinMaxTable.  Returns 1 where an index leaves the table (the reference's IndexOutOfRangeException), 0 otherwise. */
static void butterfly(int n, const int *x, int *y) {
  if (n == 4) {
    int a = x[0] + x[2], b = x[0] - x[2], c = (x[1] >> 1) - x[3], d = x[1] + (x[3] >> 1);
    y[0] = a + d, y[1] = b + c, y[2] = b - c, y[3] = a - d;
    return;
  }
  int ev[4], od[4];
  {
    int a = x[0] + x[4], b = x[0] - x[4], c = x[2] + (x[6] >> 1), d = (x[2] >> 1) - x[6];
    ev[0] = a + c, ev[1] = b + d, ev[2] = b - d, ev[3] = a - c;
  }
  {
    int a = x[1] + x[7] - x[3] - (x[3] >> 1);
    int b = x[7] - x[1] + x[5] + (x[5] >> 1);
    int c = x[5] - x[7] - (x[7] >> 1) - x[3];
    int d = x[3] + x[5] + x[1] + (x[1] >> 1);
    od[0] = d - (c >> 2), od[1] = (a >> 2) - b, od[2] = a + (b >> 2), od[3] = c + (d >> 2);
  }
  for (int k = 0; k < 4; k++) y[k] = ev[k] + od[k], y[7 - k] = ev[k] - od[k];
}
int ref_idct(int n, const int32_t *coef, const uint8_t *pred, uint8_t *out) {
  int inter[64], in[8], res[8], fault = 0;
  for (int row = 0; row < n; row++) {
    for (int j = 0; j < n; j++) in[j] = coef[row * n + j];
    if (row == 0) in[0] += 0x20;
    butterfly(n, in, res);
    for (int j = 0; j < n; j++) inter[j * n + row] = res[j];
  }
  for (int row = 0; row < n; row++) {
    butterfly(n, inter + row * n, res);
    for (int j = 0; j < n; j++) {
      int idx = 0x40 + pred[row * n + j] + (res[j] >> 6);
      if (idx < 0 || idx >= (int)sizeof mobi_vx2minmaxtable) {
        fault = 1;
        out[row * n + j] = 0;
      } else
        out[row * n + j] = mobi_vx2minmaxtable[idx];
    }
  }
  return fault;
}

/* One coefficient of CalculateNrBitsDCT(.., 0) (:767-858): val = |level| != 0, skip = zeros since the previous nonzero level, last = it
 * is the last nonzero one.  vxref = VxTable0_A_Ref[32][64][2]; r11A = Vx2Table0_A, table B = Vx2Table0_B. */
int ref_coef_bits(int val, int skip, int last, const int16_t *vxref) {
  int result = 0;
  if (val <= 31) {
    int idx = vxref[(val * 64 + skip) * 2 + last];
    if (idx >= 0) return result + (mobi_vx2table0_a[idx] & 0xF);
    int newskip = skip - mobi_vx2table0_b[(val | (last << 6)) + 0x80];
    if (newskip >= 0) {
      idx = vxref[(val * 64 + newskip) * 2 + last];
      if (idx >= 0) {
        result += 7;
        result++;
        result++;
        return result + (mobi_vx2table0_a[idx] & 0xF);
      }
    }
  }
  int newval = val - mobi_vx2table0_b[skip | (last << 6)];
  if (newval >= 0 && newval <= 31) {
    int idx = vxref[(newval * 64 + skip) * 2 + last];
    if (idx >= 0) {
      result += 7;
      result++;
      return result + (mobi_vx2table0_a[idx] & 0xF);
    }
  }
  result += 7;
  result++;
  result++;
  result++; /* last or not: one bit either way */
  result += 6;
  result += 12;
  return result;
}
int ref_nrbits(const int *dct, int len, const int16_t *vxref) {
  int lastnonzero = 0, skip = 0, result = 0;
  for (int i = 0; i < len; i++)
    if (dct[i] != 0) lastnonzero = i;
  if (lastnonzero == 0 && dct[0] == 0) return 0;
  for (int i = 0; i < len; i++) {
    if (dct[i] == 0 && lastnonzero != 0) {
      skip++;
      continue;
    }
    int val = dct[i] < 0 ? -dct[i] : dct[i];
    result += ref_coef_bits(val, skip, i == lastnonzero, vxref);
    skip = 0;
    if (i == lastnonzero) break;
  }
  return result;
}

/* MacroBlock.EncodeDecode8x8Block / 4x4Block (Encoder/MacroBlock.cs:577-597, 605-626) for one block at one quantiser, plus the
 * analyzer's SAD (GetScore8x8 / 4x4).  levels = EncodeDct (scan order).  flags: 1 coded, 2 clamp fault. */
void ref_encode_block(int n, int quantizer, const uint8_t *block, const uint8_t *compvals, const int16_t *vxref, int16_t *levels, uint8_t *recon,
                      int32_t *bits, int32_t *sad, uint8_t *flags) {
  const int nn = n * n;
  float qt4[16], qt8[64];
  ref_qtables(quantizer, qt4, qt8);
  const float *qt = n == 8 ? qt8 : qt4;
  const uint8_t *dezigzag = n == 8 ? mobi_zz8 : mobi_zz4;
  int zigzag[64]; /* ZigZagTable: natural index -> scan position */
  for (int k = 0; k < nn; k++) zigzag[dezigzag[k]] = k;
  int32_t block2[64], dctres[64], realdct[64];
  int encodedct[64], coded = 0;
  for (int i = 0; i < nn; i++) block2[i] = block[i] - compvals[i];
  ref_dct(n, block2, dctres);
  for (int i = 0; i < nn; i++) {
    float quot = (float)dctres[i] / qt[i];     /* int / float: a float32 quotient */
    int val = (int)rint((double)quot);         /* Math.Round(double): to nearest, ties to even */
    encodedct[zigzag[i]] = val;
    realdct[i] = val * (int)qt[i];
    coded |= val != 0;
  }
  for (int k = 0; k < nn; k++) levels[k] = (int16_t)encodedct[k];
  *bits = ref_nrbits(encodedct, nn, vxref);
  int fault = ref_idct(n, realdct, compvals, recon);
  int s = 0;
  for (int i = 0; i < nn; i++) s += block[i] > recon[i] ? block[i] - recon[i] : recon[i] - block[i];
  *sad = s;
  *flags = (uint8_t)(coded | fault << 1);
}

/* a batch, laid out as mobi_transform_code lays it out: entry e = qi * n_blocks + b */
void ref_encode_batch(int n, int n_q, const int *quantizers, long n_blocks, const uint8_t *src, const uint8_t *pred, const int16_t *vxref,
                      int16_t *levels, uint8_t *recon, int32_t *bits, int32_t *sad, uint8_t *flags) {
  const int nn = n * n;
  for (int qi = 0; qi < n_q; qi++)
    for (long b = 0; b < n_blocks; b++) {
      const long e = qi * n_blocks + b;
      ref_encode_block(n, quantizers[qi], src + b * nn, pred + b * nn, vxref, levels + e * nn, recon + e * nn, bits + e, sad + e, flags + e);
    }
}
