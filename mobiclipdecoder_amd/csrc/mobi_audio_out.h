// mobi_audio_out.h -- how the audio kernels (mobi_audio.hip, mobi_sx.hip) get samples into the caller's tensor: one element (put), and the
// wave's write-out of the 64-sample chunks its lanes staged in LDS (write_out).  Device code; include it inside the kernel file's own
// unnamed namespace.
#ifndef MOBI_AUDIO_OUT_H
#define MOBI_AUDIO_OUT_H

constexpr int kRow = MOBI_AU_CHUNK / 2 + 1; // dwords between the LDS rows of two lanes: 32 of samples, 1 of padding

__device__ __forceinline__ void put(const MobiAudioArgs &a, uint64_t idx, int32_t v) {
  if (a.dtype == MOBI_AUDIO_F32) ((float *)a.dst)[idx] = (float)v * (1.0f / 32768.0f);
  else ((int16_t *)a.dst)[idx] = (int16_t)v;
}

// The wave writes the chunk every lane staged: `mask` = the lanes that had a block, `pos` = the chunk's first sample in its row (the
// same for all), `base` = the wave's first lane as a global lane number, `used` = lanes in use per wave.  (i0, c0) = (tid / C, tid % C).
__device__ __forceinline__ void write_out(const MobiAudioArgs &a, const uint32_t *chunk, uint64_t mask, uint32_t pos, uint32_t base, int used,
                                          int tid, int i0, int c0) {
  const int16_t *sm = (const int16_t *)chunk;
  const int C = (int)a.n_channels;
  if (a.layout == MOBI_AUDIO_PLANAR) {
    for (int r = 0; r < used; r++) {
      if (!((mask >> r) & 1)) continue; // wave-uniform
      put(a, (uint64_t)(base + r) * a.max_samples + pos + tid, sm[r * (2 * kRow) + tid]);
    }
  } else {
    // a stream's chunk is 64 * C consecutive elements of dst: element e = sample e / C of channel e % C; lane tid takes e = 64 k + tid
    for (int q = 0; q * C < used; q++) {
      if (!((mask >> (q * C)) & 1)) continue; // wave-uniform; the channels of a stream have equal counts (checked on the host)
      const uint64_t at = ((uint64_t)(base / C + q) * a.max_samples + pos) * C;
      int i = i0, c = c0;
      for (int k = 0; k < C; k++) {
        put(a, at + 64 * k + tid, sm[(q * C + c) * (2 * kRow) + i]);
        i += 64 / C;
        c += 64 % C;
        if (c >= C) { c -= C; i++; }
      }
    }
  }
}

#endif
