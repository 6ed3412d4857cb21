// mobi_audio.hip -- the audio decode kernels for gfx950 (include/mobiclip_audio.h; arithmetic and tables: mobi_audio.h).
//
//   mobi_audio_blocks<FASTAUDIO | IMA>   The work is serial in the samples of a channel (the lattice rounds at every stage), so the
//       parallelism is streams x channels: ONE LANE per (stream, channel) walks that channel's blocks of the call in order, its states and
//       coefficients in registers.  A workgroup is one wave; of its 64 lanes (64 / C) * C are used, so that the channels of a stream sit in one
//       wave.  A FastAudio block's ten words are loaded once and its excitation is computed sample by sample, never stored.  A lane that
//       stored its own samples would give the wave 64 scattered 2-byte stores per instruction; instead every lane stages a chunk of 64
//       samples (a FastAudio subframe, a quarter of an IMA block) in LDS as 32 packed dwords, rows 33 dwords apart (bank = lane + i: no
//       conflict), and the wave writes whole rows: one row's 64 consecutive samples per store in planar layout (a 128-byte line as int16),
//       the C channels of a stream side by side in interleaved layout.  All lanes are at the same position of their rows (every row
//       starts at 0 in a call and a chunk is whole or absent), so the write-out needs nothing per row but a ballot of the lanes that had a
//       block.  Block counts differ per lane and may be 0: a lane without work computes nothing and still takes part in both barriers and
//       in the write-out; the loop's exit is wave-uniform.
//   mobi_audio_pcm16                     de-interleave and convert, one thread per sample.
#include <hip/hip_runtime.h>

#include "../../include/mobiclip_audio.h"
#include "mobi_audio.h"

namespace {

#include "mobi_audio_out.h" // put, write_out, kRow: shared with mobi_sx.hip

template <int CODEC> __global__ __launch_bounds__(64) void mobi_audio_blocks(const MobiAudioArgs a) {
  __shared__ uint32_t chunk[64 * kRow];
  __shared__ int16_t tab[CODEC == MOBI_AUDIO_FASTAUDIO ? 512 : 96];
  const int tid = (int)threadIdx.x, C = (int)a.n_channels, used = 64 / C * C;
  const uint32_t base = blockIdx.x * (uint32_t)used, g = base + tid;
  const bool live = tid < used && g < a.n_lanes;
  for (int i = tid; i < (CODEC == MOBI_AUDIO_FASTAUDIO ? 512 : 96); i += 64) tab[i] = CODEC == MOBI_AUDIO_FASTAUDIO ? a.k->pulse[i] : a.k->step[i];
  __syncthreads();

  MobiAudioLane ln = {0, 0, 0, 0, 0, 0};
  if (live) ln = a.lanes[g];
  const int nblk = ln.nblk;
  const bool touch = live && (nblk || (ln.flags & MOBI_AU_ZERO));
  MobiFaState fa = {{0, 0, 0, 0, 0, 0, 0, 0}, 0};
  MobiImaState ima = {0, 0};
  if (touch && !(ln.flags & MOBI_AU_ZERO)) {
    if (CODEC == MOBI_AUDIO_FASTAUDIO) {
#pragma unroll
      for (int w = 0; w < 8; w++) fa.s[w] = a.state[(size_t)w * a.n_lanes + g];
      fa.de = a.state[(size_t)8 * a.n_lanes + g];
    } else {
      ima.last = a.state[g];
      ima.index = a.state[(size_t)a.n_lanes + g];
    }
  }
  if (CODEC == MOBI_AUDIO_IMA && (ln.flags & MOBI_AU_HEADER)) {
    ima.last = ln.hdr_last;
    ima.index = ln.hdr_index;
  }
  const uint8_t *src = a.data + ln.off;
  const int i0 = tid / C, c0 = tid % C;
  uint32_t *mine = chunk + tid * kRow;

  for (int b = 0;; b++) {
    const bool on = b < nblk;
    const uint64_t mask = __ballot(on);
    if (!mask) break; // wave-uniform: the workgroup is this one wave
    if (CODEC == MOBI_AUDIO_FASTAUDIO) {
      uint32_t w[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      int32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (on) {
        const uint2 *p = (const uint2 *)(src + (size_t)b * MOBI_FA_BLOCK_BYTES); // 8-byte aligned: the lane's bytes start on 16, blocks are 40
#pragma unroll
        for (int j = 0; j < 5; j++) {
          const uint2 v = p[j];
          w[2 * j] = v.x;
          w[2 * j + 1] = v.y;
        }
        mobi_fa_coefficients(w[0], mobi_fa_low4(w[3], w[5], w[7], w[9]), a.k->k01, a.k->k2, a.k->k3, a.k->k4, a.k->k5, a.k->k6, a.k->k7, k);
      }
#pragma unroll 1
      for (int sub = 0; sub < 4; sub++) {
        if (on) {
          const uint32_t wa = sub == 0 ? w[2] : sub == 1 ? w[4] : sub == 2 ? w[6] : w[8];
          const uint32_t wb = sub == 0 ? w[3] : sub == 1 ? w[5] : sub == 2 ? w[7] : w[9];
          MobiFaExc e;
          mobi_fa_exc_begin(e, w[1], sub, wa, wb);
#pragma unroll 1
          for (int i = 0; i < MOBI_AU_CHUNK / 2; i++) {
            const int32_t lo = mobi_fa_sample(mobi_fa_exc_next(e, 2 * i, tab), k, fa);
            const int32_t hi = mobi_fa_sample(mobi_fa_exc_next(e, 2 * i + 1, tab), k, fa);
            mine[i] = ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
          }
        }
        __syncthreads();
        write_out(a, chunk, mask, (uint32_t)b * MOBI_AU_BLOCK_SAMPLES + sub * MOBI_AU_CHUNK, base, used, tid, i0, c0);
        __syncthreads();
      }
    } else {
#pragma unroll 1
      for (int sub = 0; sub < 4; sub++) {
        if (on) {
          const uint4 *p = (const uint4 *)(src + (size_t)b * MOBI_IMA_BLOCK_BYTES + sub * (MOBI_AU_CHUNK / 2)); // 16-byte aligned
          const uint4 v0 = p[0], v1 = p[1];
          const uint32_t w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
          for (int j = 0; j < 8; j++) {
#pragma unroll
            for (int n = 0; n < 4; n++) { // bytes in address order, low nibble first
              const int32_t lo = mobi_ima_sample((w[j] >> (8 * n)) & 0xF, ima, tab);
              const int32_t hi = mobi_ima_sample((w[j] >> (8 * n + 4)) & 0xF, ima, tab);
              mine[4 * j + n] = ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
            }
          }
        }
        __syncthreads();
        write_out(a, chunk, mask, (uint32_t)b * MOBI_AU_BLOCK_SAMPLES + sub * MOBI_AU_CHUNK, base, used, tid, i0, c0);
        __syncthreads();
      }
    }
  }

  if (touch) {
    if (CODEC == MOBI_AUDIO_FASTAUDIO) {
#pragma unroll
      for (int w = 0; w < 8; w++) a.state[(size_t)w * a.n_lanes + g] = fa.s[w];
      a.state[(size_t)8 * a.n_lanes + g] = fa.de;
    } else {
      a.state[g] = ima.last;
      a.state[(size_t)a.n_lanes + g] = ima.index;
    }
  }
}

// element e of stream s = sample e / C of channel e % C, two bytes little endian at the stream's staged bytes + 2 e; every stream gets
// the blocks the longest one needs
__global__ __launch_bounds__(256) void mobi_audio_pcm16(const MobiAudioArgs a, uint32_t blocks_per_stream) {
  const uint32_t s = blockIdx.x / blocks_per_stream, C = a.n_channels;
  const MobiAudioLane ln = a.lanes[s];
  const uint64_t e = (uint64_t)(blockIdx.x % blocks_per_stream) * 256 + threadIdx.x;
  if (e >= (uint64_t)ln.n_pcm * C) return;
  const int32_t v = *(const int16_t *)(a.data + ln.off + 2 * e); // ln.off is 16-byte aligned
  const uint64_t i = e / C, c = e % C;
  put(a, a.layout == MOBI_AUDIO_PLANAR ? ((uint64_t)s * C + c) * a.max_samples + i : ((uint64_t)s * a.max_samples + i) * C + c, v);
}

} // namespace

extern "C" int mobi_launch_audio(const MobiAudioArgs *a, hipStream_t s) {
  if (a->codec == MOBI_AUDIO_PCM16) {
    if (!a->pcm_max) return 0;
    const uint64_t bps = ((uint64_t)a->pcm_max * a->n_channels + 255) / 256;
    if (bps * a->n_lanes > 0x7FFFFFFFull) return -1;
    mobi_audio_pcm16<<<(unsigned)(bps * a->n_lanes), 256, 0, s>>>(*a, (uint32_t)bps);
  } else {
    const unsigned used = 64 / a->n_channels * a->n_channels, waves = (a->n_lanes + used - 1) / used;
    if (a->codec == MOBI_AUDIO_FASTAUDIO) mobi_audio_blocks<MOBI_AUDIO_FASTAUDIO><<<waves, 64, 0, s>>>(*a);
    else mobi_audio_blocks<MOBI_AUDIO_IMA><<<waves, 64, 0, s>>>(*a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
