// mobi_encode_rate.h -- the rate rule of both encoders (include/mobiclip_encode_rate.h; DESIGN.md "Rate control"), one definition for the
// kernels (mobi_encode_rate.hip), the entry points and the host model (tests/tools/mobi_encode_rate_host.cpp).
//
// Per picture: a byte target and the call's quantiser range qmin <= qmax in [12, 52].  lo = qmin, hi = qmax; K = mobi_enc_rate_rounds
// rounds, the same for every picture of the call; in each round the picture is ENCODED at mid = (lo + hi) >> 1 and the stream's length
// read: fits (bytes <= target) -> hi = mid, else lo = min(mid + 1, hi).  Every round halves hi - lo + 1 rounding up, so after K rounds
// lo == hi: q_out, at which the picture is encoded for good.  hi only ever becomes a quantiser whose stream fitted, so the stream at q_out
// fits or q_out == qmax.  The length is NOT monotone in the quantiser: q_out is what this bisection returns, not the smallest that fits.
#ifndef MOBI_ENCODE_RATE_H
#define MOBI_ENCODE_RATE_H
#include "../../include/mobiclip_encode_rate.h"
#include "mobi_encode_parts.h"

// the smallest k with 2^k >= qmax - qmin + 1 (0 .. 6); -1 for a range the calls refuse
MOBI_TC_FN int mobi_enc_rate_rounds_of(int qmin, int qmax) {
  if (qmin < MOBI_ENC_QMIN || qmax > MOBI_ENC_QMAX || qmin > qmax) return -1;
  int k = 0;
  while ((1 << k) < qmax - qmin + 1) k++;
  return k;
}

// a quantiser read from device memory, before use
MOBI_TC_FN int mobi_enc_rate_clamp_q(int q) { return q < MOBI_ENC_QMIN ? MOBI_ENC_QMIN : q > MOBI_ENC_QMAX ? MOBI_ENC_QMAX : q; }

struct MobiEncRateState {
  int lo, hi;
};
MOBI_TC_FN int mobi_enc_rate_mid(MobiEncRateState s) { return (s.lo + s.hi) >> 1; }
// one round: the trial at mobi_enc_rate_mid(s) gave a stream of `bytes`
MOBI_TC_FN MobiEncRateState mobi_enc_rate_step(MobiEncRateState s, int64_t bytes, int32_t target) {
  const int mid = mobi_enc_rate_mid(s);
  if (bytes <= (int64_t)target) s.hi = mid;
  else s.lo = mid + 1 < s.hi ? mid + 1 : s.hi;
  return s;
}

// what the rate kernels read and write: one lane per picture
struct MobiEncRateArgs {
  const int32_t *target;      // [n]
  const uint8_t *prev_in;     // [n] the caller's previous quantisers, or NULL (I-frames)
  uint8_t *prev_q;            // [n] the encoder's row of them, clamped (NULL with prev_in)
  uint8_t *q;                 // [n] the encoder's quantiser row: the next trial's, at last q_out
  uint8_t *lo, *hi;           // [n] each: the state between the rounds
  uint8_t *q_out;             // [n] the caller's
  const int32_t *bytes;       // [n] the trial's lengths (bytes_out)
  uint64_t *stats;            // [n][8] or NULL: zeroed behind every trial, the code kernels add to it
  int32_t n, qmin, qmax;
};

#if !defined(__HIP_DEVICE_COMPILE__)
// the refusals the two target calls add to their encoder's check
static inline int mobi_enc_rate_check_args(const int32_t *target_bytes, int qmin, int qmax, const uint8_t *quantizers_out) {
  if (mobi_enc_rate_rounds_of(qmin, qmax) < 0 || !target_bytes || (uintptr_t)target_bytes % 4 || !quantizers_out) return -7; // MOBI_E_ARG
  return 0;
}
#endif
#endif
