// mobi_encode_rate.hip -- the rate rule's two kernels on gfx950 (mobi_encode_rate.h; include/mobiclip_encode_rate.h; DESIGN.md "Rate
// control").  One lane per picture; everything between two of them is the encoders' own stage kernels up to the scan.
//
// mobi_enc_rate_begin: the previous quantisers clamped into the encoder's row, lo = qmin, hi = qmax, the first trial's quantiser
// (with no round to run: q_out itself, to the caller too).
// mobi_enc_rate_step: behind a trial's scan.  Reads the stream's length, applies the rule, writes the next quantiser -- in the last
// round q_out, to the caller too -- and zeroes the picture's statistics, to which the next encode's code kernels add.
#include <hip/hip_runtime.h>

#include "mobi_encode_rate.h"

extern "C" __global__ __launch_bounds__(64) void mobi_enc_rate_begin(MobiEncRateArgs A, int rounds) {
  const int pic = blockIdx.x * 64 + threadIdx.x;
  if (pic >= A.n) return;
  if (A.prev_in) A.prev_q[pic] = (uint8_t)mobi_enc_rate_clamp_q(A.prev_in[pic]);
  MobiEncRateState s;
  s.lo = A.qmin;
  s.hi = A.qmax;
  A.lo[pic] = (uint8_t)s.lo;
  A.hi[pic] = (uint8_t)s.hi;
  const uint8_t q = (uint8_t)mobi_enc_rate_mid(s);
  A.q[pic] = q;
  if (rounds == 0) A.q_out[pic] = q;
}

extern "C" __global__ __launch_bounds__(64) void mobi_enc_rate_step(MobiEncRateArgs A, int last) {
  const int pic = blockIdx.x * 64 + threadIdx.x;
  if (pic >= A.n) return;
  MobiEncRateState s;
  s.lo = A.lo[pic];
  s.hi = A.hi[pic];
  s = mobi_enc_rate_step(s, A.bytes[pic], A.target[pic]);
  A.lo[pic] = (uint8_t)s.lo;
  A.hi[pic] = (uint8_t)s.hi;
  const uint8_t q = (uint8_t)mobi_enc_rate_mid(s); // in the last round lo == hi
  A.q[pic] = q;
  if (last) A.q_out[pic] = q;
  if (A.stats) {
#pragma unroll
    for (int i = 0; i < 8; i++) A.stats[(size_t)pic * 8 + i] = 0;
  }
}

extern "C" int mobi_launch_rate_begin(const MobiEncRateArgs *a, int rounds, hipStream_t s) {
  hipLaunchKernelGGL(mobi_enc_rate_begin, dim3((a->n + 63) / 64), dim3(64), 0, s, *a, rounds);
  return (int)hipGetLastError();
}

extern "C" int mobi_launch_rate_step(const MobiEncRateArgs *a, int last, hipStream_t s) {
  hipLaunchKernelGGL(mobi_enc_rate_step, dim3((a->n + 63) / 64), dim3(64), 0, s, *a, last);
  return (int)hipGetLastError();
}
