// mobi_sx.h -- the Sx audio codec's arithmetic (include/mobiclip_sx.h) that the kernel (mobi_sx.hip) and a stand-alone host program
// (tests/tools/mobi_sx_host.cpp) compile alike, in the manner of mobi_audio.h.
//
//   Sx   LibMobiclip.Codec.Sx.SxDecoder (SxDecoder.cs): a packet of 16-bit LE words -> 128 samples of one channel.
//        word 0   15..9 lag (0x7F: a reset packet, sub_8BC; 0x7E: no long-term prediction), 8..6 gain step, 5..0 stage-0 row
//        word 1   15..14 first pulse position, 13..12 rate, 11..6 stage-1 row, 5..0 stage-2 row
//        rate 0   8 words of five 3-bit codes, their bits 0 gathered into two more: 42 pulses 3 apart, g (2c - 7)       (sub_1B8)
//        rate r   6 - r words of eight 2-bit codes: pulses 2 + r apart, g (2c - 3)                                       (sub_170)
//        so a packet is 20, 14, 12 or 10 bytes (table_83E), known from word 1.
//   The excitation is long-term prediction (128 words of the past from word 0x7F - lag of a 256-word window, halved, six words tapered at
//   each end: sub_28) plus pulses.  The coefficients are eight sums -- the previous sums, or the codebook's base vector on a reset packet,
//   plus one row of each of three stages (sub_3B4) -- through a Q15 step-up recursion, negated and halved (sub_244); a normal packet
//   filters its four quarters with 1/4, 1/2, 3/4 and all of the way from the previous packet's coefficients (sub_728, sub_6C0).  The
//   filter is 8-tap all-pole, y = (e 2^14 + sum h[k] c[k]) >> 14 (sub_3F8); a sample is y clamped to int16.
//
// STATE.  The reference keeps everything in Internal[0x8B8] and so does this, word for word where a word outlives a packet.  The two
// 256-word buffers (Internal + 0xB8, + 0x4B8) are NOT a clean sliding window: a normal packet of parity P builds its excitation in the
// second half of buffer P from buffer P ^ 1 and writes its UNCLAMPED OUTPUTS over the first half of buffer P ^ 1; a reset packet clears
// nothing, builds in the second half of buffer 1, writes its outputs to the first half of buffer 0 and leaves parity 0.  The packet after a
// reset therefore reads, as older past, the first half of buffer 1 as it happened to be: the outputs of the packet before the reset (that
// packet had parity 0) or the excitation of two packets before it (parity 1).  Both buffers are kept whole: `buf` is Internal + 0xB8.
// The two coefficient sets at 0x20 and 0x40 alternate with the parity; they are kept as `last` (the previous packet's) and `stale`.
//
// All arithmetic is C# int, WHICH WRAPS: the gain is a geometric product, the filter sums products of arbitrary 32-bit values.  As in
// mobi_audio.h: computed in uint32_t, shifted right arithmetically as int32_t, no 24-bit multiply.
#ifndef MOBI_SX_H
#define MOBI_SX_H
#include <stdint.h>

#include "mobi_audio.h"

enum { MOBI_SX_SAMPLES = 128,        // per packet
       MOBI_SX_CODEBOOK = 0xC34,     // bytes: three stages of 64 rows of 8 s16 (0, 0x400, 0x800), 8 s16 gain steps (0xC00), 8 s32 base
                                     // sums (0xC10), s32 first gain (0xC30)
       MOBI_SX_BOOK_PITCH = 0xC40,   // between the codebooks of two lanes in device memory: rows stay 16-byte aligned
       MOBI_SX_BUF_WORDS = 512,      // the two buffers
       MOBI_SX_REG_WORDS = 34,       // sum, last, stale, h, gain, parity
       MOBI_SX_STATE_WORDS = MOBI_SX_REG_WORDS + MOBI_SX_BUF_WORDS }; // per lane in device memory, word w of lane g at state[w * n_lanes + g]

struct MobiSxState {
  int32_t sum[8];   // Internal + 0x00
  int32_t last[8];  // the previous packet's coefficients: Internal + 0x40 when parity == 0, + 0x20 when 1
  int32_t stale[8]; // the other set (never read again; kept because the reference keeps it)
  int32_t h[8];     // Internal + 0x70: the filter's last eight outputs, h[j] = that of sample 8 n + j
  int32_t gain;     // Internal + 0x60
  int32_t parity;   // Internal + 0x64
};

// a packet between mobi_sx_begin and mobi_sx_end
struct MobiSxPacket {
  int32_t nw[8];  // its coefficients
  int32_t in;     // its excitation: 128 words at buf + in
  int32_t out;    // its unclamped outputs go to buf + out
  int32_t reset;
};

MOBI_AU_FN int mobi_sx_packet_bytes(uint32_t w1) { // table_83E[(w1 >> 12) & 3]
  const int rate = (int)(w1 >> 12) & 3;
  return rate ? 16 - 2 * rate : 20;
}

// word i of a packet; the kernel's packets start on even addresses (every length is even, a lane's first is 16-byte aligned)
MOBI_AU_FN uint32_t mobi_sx_word(const uint8_t *p, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ((const uint16_t *)p)[i];
#else
  return (uint32_t)p[2 * i] | ((uint32_t)p[2 * i + 1] << 8);
#endif
}
// the codebook: the kernel's copies are 16-byte aligned, a caller's need not be
MOBI_AU_FN int32_t mobi_sx_cb16(const uint8_t *cb, int off) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const int16_t *)(cb + off);
#else
  return (int16_t)(uint16_t)(cb[off] | (cb[off + 1] << 8));
#endif
}
MOBI_AU_FN int32_t mobi_sx_cb32(const uint8_t *cb, int off) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const int32_t *)(cb + off);
#else
  return (int32_t)((uint32_t)cb[off] | ((uint32_t)cb[off + 1] << 8) | ((uint32_t)cb[off + 2] << 16) | ((uint32_t)cb[off + 3] << 24));
#endif
}
// sub_3B4: sum[i] += the row's eight s16
MOBI_AU_FN void mobi_sx_add_row(const uint8_t *cb, int off, int32_t (&sum)[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 v = *(const uint4 *)(cb + off);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    sum[2 * i] = (int32_t)((uint32_t)sum[2 * i] + (uint32_t)(int32_t)(int16_t)(w[i] & 0xFFFFu));
    sum[2 * i + 1] = (int32_t)((uint32_t)sum[2 * i + 1] + (uint32_t)((int32_t)w[i] >> 16));
  }
#else
  for (int i = 0; i < 8; i++) sum[i] = (int32_t)((uint32_t)sum[i] + (uint32_t)mobi_sx_cb16(cb, off + 2 * i));
#endif
}

MOBI_AU_FN int32_t mobi_sx_mul15(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b) >> 15; }
MOBI_AU_FN int32_t mobi_sx_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }

// sub_244 behind the sums: the step-up recursion over c (the sums on entry), negated and halved
MOBI_AU_FN void mobi_sx_step_up(int32_t (&c)[8]) {
#define MOBI_SX_PAIR(i, j, k) /* c[i], c[j] += (c[j], c[i]) * c[k] >> 15, both from the values before */ \
  { const int32_t t_ = mobi_sx_mul15(c[i], c[k]); c[i] = mobi_sx_add(c[i], mobi_sx_mul15(c[j], c[k])); c[j] = mobi_sx_add(c[j], t_); }
#define MOBI_SX_SELF(i, k) c[i] = mobi_sx_add(c[i], mobi_sx_mul15(c[i], c[k]));
  MOBI_SX_SELF(0, 1)
  MOBI_SX_PAIR(0, 1, 2)
  MOBI_SX_PAIR(0, 2, 3) MOBI_SX_SELF(1, 3)
  MOBI_SX_PAIR(0, 3, 4) MOBI_SX_PAIR(1, 2, 4)
  MOBI_SX_PAIR(0, 4, 5) MOBI_SX_PAIR(1, 3, 5) MOBI_SX_SELF(2, 5)
  MOBI_SX_PAIR(0, 5, 6) MOBI_SX_PAIR(1, 4, 6) MOBI_SX_PAIR(2, 3, 6)
  MOBI_SX_PAIR(0, 6, 7) MOBI_SX_PAIR(1, 5, 7) MOBI_SX_PAIR(2, 4, 7) MOBI_SX_SELF(3, 7)
#undef MOBI_SX_PAIR
#undef MOBI_SX_SELF
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) c[i] = (int32_t)(0u - (uint32_t)(c[i] >> 1));
}

// sub_8FC's copy and sub_28 / sub_0: cur[0..127] = other[128..255]; cur[128..255] = the long-term prediction from other, or zeros
MOBI_AU_FN void mobi_sx_window(int32_t *cur, const int32_t *other, uint32_t lag) {
  for (int i = 0; i < 128; i++) cur[i] = other[128 + i];
  int32_t *e = cur + 128;
  if (lag == 0x7E) {
    for (int i = 0; i < 128; i++) e[i] = 0;
    return;
  }
  const int32_t *s = other + (0x7F - lag); // lag <= 0x7D: words 2 .. 254
  for (int i = 0; i < 7; i++) e[i] = (int32_t)((uint32_t)s[i] * (uint32_t)(i + 1)) >> 4;
  for (int i = 7; i < 121; i++) e[i] = s[i] >> 1;
  for (int i = 121; i < 128; i++) e[i] = (int32_t)((uint32_t)s[i] * (uint32_t)(128 - i)) >> 4;
}

// sub_1B8 / sub_170: the pulses of the packet at p added to e[0..127]; g = the packet's gain.  The last pulse lies at most at 126, 120, 127, 118.
MOBI_AU_FN void mobi_sx_pulses(int32_t *e, const uint8_t *p, uint32_t w1, int32_t g) {
  const int rate = (int)(w1 >> 12) & 3;
  const uint32_t g2 = (uint32_t)g * 2u;
  e += w1 >> 14;
  if (rate == 0) {
    const uint32_t base = 0u - (uint32_t)g * 7u;
    uint32_t low = 0;
    for (int i = 0; i < 8; i++) {
      const uint32_t w = mobi_sx_word(p, 2 + i);
      for (int sh = 13; sh >= 0; sh -= 3, e += 3) *e = (int32_t)((uint32_t)*e + g2 * ((w >> sh) & 7) + base);
      low = (low << 1) | (w & 1);
    }
    e[0] = (int32_t)((uint32_t)e[0] + g2 * ((low >> 5) & 7) + base);
    e[3] = (int32_t)((uint32_t)e[3] + g2 * ((low >> 2) & 7) + base);
  } else {
    const uint32_t base = 0u - (uint32_t)g * 3u;
    const int step = 2 + rate;
    for (int i = 0; i < 6 - rate; i++) {
      const uint32_t w = mobi_sx_word(p, 2 + i);
      for (int sh = 14; sh >= 0; sh -= 2, e += step) *e = (int32_t)((uint32_t)*e + g2 * ((w >> sh) & 3) + base);
    }
  }
}

// Everything of a packet before its filter: the window, the gain, the pulses, the sums and the coefficients.  buf = the lane's two buffers,
// cb = its codebook, p = the packet.  Returns the packet's length in bytes.
MOBI_AU_FN int mobi_sx_begin(MobiSxState &st, int32_t *buf, const uint8_t *cb, const uint8_t *p, MobiSxPacket &pk) {
  const uint32_t w0 = mobi_sx_word(p, 0), w1 = mobi_sx_word(p, 1), lag = w0 >> 9;
  pk.reset = lag == 0x7F;
  if (pk.reset) { // sub_8BC, sub_798: nothing else is cleared
    st.gain = mobi_sx_cb32(cb, 0xC30);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 8; i++) st.h[i] = 0, st.sum[i] = mobi_sx_cb32(cb, 0xC10 + 4 * i);
    pk.in = 256 + 128;
    pk.out = 0;
    for (int i = 0; i < 128; i++) buf[pk.in + i] = 0;
  } else { // sub_8FC
    const int32_t cur = st.parity * 256, other = 256 - cur;
    mobi_sx_window(buf + cur, buf + other, lag);
    pk.in = cur + 128;
    pk.out = other;
  }
  st.gain = (int32_t)((uint32_t)mobi_sx_cb16(cb, 0xC00 + 2 * (int)((w0 >> 6) & 7)) * (uint32_t)st.gain) >> 13; // sub_844
  mobi_sx_pulses(buf + pk.in, p, w1, st.gain);
  mobi_sx_add_row(cb, 16 * (int)(w0 & 0x3F), st.sum);
  mobi_sx_add_row(cb, 0x400 + 16 * (int)((w1 >> 6) & 0x3F), st.sum);
  mobi_sx_add_row(cb, 0x800 + 16 * (int)(w1 & 0x3F), st.sum);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) pk.nw[i] = st.sum[i];
  mobi_sx_step_up(pk.nw);
  return mobi_sx_packet_bytes(w1);
}

// the coefficients of quarter q (32 samples) of the packet: sub_728's order of sub_6C0 calls; a reset packet uses its own throughout
MOBI_AU_FN void mobi_sx_quarter(const MobiSxState &st, const MobiSxPacket &pk, int q, int32_t (&c)[8]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) {
    const int32_t half = mobi_sx_add(pk.nw[i], st.last[i]) >> 1;
    c[i] = (pk.reset || q == 3) ? pk.nw[i] : q == 1 ? half : mobi_sx_add(half, q == 0 ? st.last[i] : pk.nw[i]) >> 1;
  }
}

// sub_3F8 for eight samples: y[i] = (e[i] << 14 + sum over k of c[k] * the output k + 1 samples back) >> 14
MOBI_AU_FN void mobi_sx_filter8(const int32_t (&e)[8], const int32_t (&c)[8], int32_t (&h)[8], int32_t (&y)[8]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) {
    uint32_t acc = (uint32_t)e[i] << 14;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) acc += (uint32_t)h[(i + 7 - k) & 7] * (uint32_t)c[k];
    y[i] = h[i] = (int32_t)acc >> 14;
  }
}
MOBI_AU_FN int32_t mobi_sx_clamp(int32_t y) { return y > 32767 ? 32767 : y < -32768 ? -32768 : y; }

// behind the packet's 128 samples: the coefficient sets and the parity move on (sub_728's store, sub_8BC's store to 0x40, Decode's ^= 1)
MOBI_AU_FN void mobi_sx_end(MobiSxState &st, const MobiSxPacket &pk) {
  const bool keep_stale = pk.reset && st.parity == 0; // the reset's set replaces `last` in place (0x40)
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) {
    if (!keep_stale) st.stale[i] = st.last[i];
    st.last[i] = pk.nw[i];
  }
  st.parity = pk.reset ? 0 : st.parity ^ 1;
}

#endif
