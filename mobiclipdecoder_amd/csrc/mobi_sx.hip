// mobi_sx.hip -- the Sx audio decode kernel for gfx950 (include/mobiclip_sx.h; arithmetic and the state's meaning: mobi_sx.h).
//
//   mobi_sx_packets   The all-pole filter is serial in a channel's samples, so, as in mobi_audio_blocks, ONE LANE per (stream, channel)
//       walks that channel's packets of the call in order; a workgroup is one wave of which (64 / C) * C lanes are used.  Sums,
//       coefficient sets, filter history, gain and parity live in registers.  The two 256-word excitation buffers are indexed per lane
//       (the long-term prediction starts at word 0x7F - lag), so they live in LDS: 512 words per lane, lanes 513 dwords apart (bank =
//       lane + index: the common same-index accesses of a wave are conflict-free), 128.25 KiB, beside the 8.25 KiB write-out tile.  That is
//       one workgroup per CU, which costs nothing here: a call has few waves and each is bound by its lanes' dependent chains.  Both
//       buffers are kept whole rather than as a 384-word window because a reset packet makes the first half of buffer 1 -- unclamped
//       outputs or old excitation, by parity -- the next packet's past (mobi_sx.h).  The persistent state is word-major in device memory
//       (state[word * n_lanes + lane]): every load and store of the wave is one coalesced row.
//       A packet's 128 samples leave as two 64-sample chunks through the LDS tile and write_out (mobi_audio_out.h).  Packet counts differ
//       per lane and may be 0: such a lane computes nothing, still takes part in every barrier and write-out, and the loop's exit is
//       wave-uniform.
#include <hip/hip_runtime.h>

#include "../../include/mobiclip_audio.h"
#include "mobi_audio.h"
#include "mobi_sx.h"

namespace {

#include "mobi_audio_out.h"

constexpr int kWin = MOBI_SX_BUF_WORDS + 1; // dwords between the buffers of two lanes

__global__ __launch_bounds__(64) void mobi_sx_packets(const MobiAudioArgs a, const uint8_t *books) {
  __shared__ int32_t win[64 * kWin];
  __shared__ uint32_t chunk[64 * kRow];
  const int tid = (int)threadIdx.x, C = (int)a.n_channels, used = 64 / C * C;
  const uint32_t base = blockIdx.x * (uint32_t)used, g = base + tid;
  const bool live = tid < used && g < a.n_lanes;

  MobiAudioLane ln = {0, 0, 0, 0, 0, 0};
  if (live) ln = a.lanes[g];
  const int npk = ln.nblk;
  const bool touch = live && (npk || (ln.flags & MOBI_AU_ZERO));
  int32_t *buf = win + tid * kWin;
  int32_t *word = a.state + g; // word w of this lane: word[w * n_lanes]
  const size_t nl = a.n_lanes;
  MobiSxState st = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}, 0, 0};
  if (touch) {
    if (ln.flags & MOBI_AU_ZERO) {
      for (int w = 0; w < MOBI_SX_BUF_WORDS; w++) buf[w] = 0;
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        st.sum[i] = word[(size_t)i * nl];
        st.last[i] = word[(size_t)(8 + i) * nl];
        st.stale[i] = word[(size_t)(16 + i) * nl];
        st.h[i] = word[(size_t)(24 + i) * nl];
      }
      st.gain = word[(size_t)32 * nl];
      st.parity = word[(size_t)33 * nl] & 1;
#pragma unroll 32 // 32 loads in flight: the 512 rows are 16 round trips to memory, not 64
      for (int w = 0; w < MOBI_SX_BUF_WORDS; w++) buf[w] = word[(size_t)(MOBI_SX_REG_WORDS + w) * nl];
    }
  }
  const uint8_t *cb = books + (size_t)g * MOBI_SX_BOOK_PITCH;
  const uint8_t *src = a.data + ln.off;
  const int i0 = tid / C, c0 = tid % C;
  uint32_t *mine = chunk + tid * kRow;

  for (int b = 0;; b++) {
    const bool on = b < npk;
    const uint64_t mask = __ballot(on);
    if (!mask) break; // wave-uniform: the workgroup is this one wave
    MobiSxPacket pk = {{0, 0, 0, 0, 0, 0, 0, 0}, 0, 0, 0};
    if (on) src += mobi_sx_begin(st, buf, cb, src, pk);
#pragma unroll 1
    for (int half = 0; half < 2; half++) {
      if (on) {
#pragma unroll 1
        for (int q = 2 * half; q < 2 * half + 2; q++) {
          int32_t c[8];
          mobi_sx_quarter(st, pk, q, c);
#pragma unroll 1
          for (int i = 32 * q; i < 32 * q + 32; i += 8) {
            int32_t e[8], y[8];
#pragma unroll
            for (int j = 0; j < 8; j++) e[j] = buf[pk.in + i + j];
            mobi_sx_filter8(e, c, st.h, y);
#pragma unroll
            for (int j = 0; j < 8; j++) buf[pk.out + i + j] = y[j];
#pragma unroll
            for (int j = 0; j < 4; j++)
              mine[(i & 63) / 2 + j] = ((uint32_t)mobi_sx_clamp(y[2 * j]) & 0xFFFFu) | ((uint32_t)mobi_sx_clamp(y[2 * j + 1]) << 16);
          }
        }
      }
      __syncthreads();
      write_out(a, chunk, mask, (uint32_t)b * MOBI_SX_SAMPLES + half * MOBI_AU_CHUNK, base, used, tid, i0, c0);
      __syncthreads();
    }
    if (on) mobi_sx_end(st, pk);
  }

  if (touch) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      word[(size_t)i * nl] = st.sum[i];
      word[(size_t)(8 + i) * nl] = st.last[i];
      word[(size_t)(16 + i) * nl] = st.stale[i];
      word[(size_t)(24 + i) * nl] = st.h[i];
    }
    word[(size_t)32 * nl] = st.gain;
    word[(size_t)33 * nl] = st.parity;
#pragma unroll 8
    for (int w = 0; w < MOBI_SX_BUF_WORDS; w++) word[(size_t)(MOBI_SX_REG_WORDS + w) * nl] = buf[w];
  }
}

} // namespace

extern "C" int mobi_launch_sx(const MobiAudioArgs *a, const uint8_t *books, hipStream_t s) {
  const unsigned used = 64 / a->n_channels * a->n_channels, waves = (a->n_lanes + used - 1) / used;
  mobi_sx_packets<<<waves, 64, 0, s>>>(*a, books);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
