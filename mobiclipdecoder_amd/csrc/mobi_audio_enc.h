// mobi_audio_enc.h -- the audio encoder's rule (include/mobiclip_audio_enc.h; DESIGN.md "Audio encoder"), one definition for the kernels
// (mobi_audio_enc.hip), the entry points (mobi_audio_enc.cpp) and the host model (tests/tools/mobi_audio_enc_host.cpp).  It builds on
// mobi_audio.h: every candidate sample IS what the decoder's mobi_ima_sample returns, and the tables are that header's.  One thing is
// restated here, the decoder's difference before its clamp (mobi_aenc_raw), because mobi_ima_sample hands out only the clamped sample and
// the `clamped` count needs the other; it decides no byte of a frame, and the tests hold the count against the plain-Python model.
//
//   nibble   from a decoder state, the code of sample x is the val in 0..15 whose decoded (clamped) sample lies nearest to x; ties go to
//            the smallest val.  The sixteen candidates are tried literally: near the clamp the nearest one may carry the "wrong" sign
//            (last = x = -32768: val 8 reproduces x, val 0 does not), so no shortcut over the sign of x - last is taken.
//   header   last = x[0]; the index is the i0 in 0..88 with the least squared error over block 0 (a 64-bit sum), ties to the smallest.
//   frame    C headers (s16le index, s16le last), then for b, c the 128 bytes of block b of channel c at 4 C + 128 (b C + c).
//   PCM16    the S C samples interleaved, s16le.
#ifndef MOBI_AUDIO_ENC_RULE_H
#define MOBI_AUDIO_ENC_RULE_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/mobiclip_audio_enc.h"
#include "mobi_audio.h"

enum { MOBI_AENC_INDICES = 89,          // start indices tried per (stream, channel)
       MOBI_AENC_MAX_BLOCKS = 65535,    // per channel and call, as the decoder's limit
       MOBI_AENC_STATS_BYTES = 16 };

// mobi_audio_enc_stats of include/mobiclip_audio_enc.h, as the kernels write it
struct MobiAencStats {
  uint64_t sse;
  uint32_t clamped, start_index;
};

// the bytes of a frame of `blocks` blocks per channel; 0 for a codec this encoder does not write
MOBI_AU_FN uint64_t mobi_aenc_frame_bytes(int codec, uint64_t C, uint64_t blocks) {
  if (codec == MOBI_AUDIO_IMA) return MOBI_IMA_HEADER_BYTES * C + MOBI_IMA_BLOCK_BYTES * C * blocks;
  if (codec == MOBI_AUDIO_PCM16) return 2 * C * MOBI_AU_BLOCK_SAMPLES * blocks;
  return 0;
}
MOBI_AU_FN uint64_t mobi_aenc_block_offset(uint64_t C, uint64_t b, uint64_t c) { return MOBI_IMA_HEADER_BYTES * C + MOBI_IMA_BLOCK_BYTES * (b * C + c); }

// what an encoder object may be made with: MOBI_OK, MOBI_E_UNSUPPORTED (FastAudio, Sx), MOBI_E_ARG
MOBI_AU_FN int mobi_aenc_check_create(int codec, int n_streams, int n_channels, int max_blocks) {
  if (codec == MOBI_AUDIO_FASTAUDIO || codec == MOBI_AUDIO_SX) return MOBI_E_UNSUPPORTED;
  if (codec != MOBI_AUDIO_IMA && codec != MOBI_AUDIO_PCM16) return MOBI_E_ARG;
  if (n_channels < 1 || n_channels > MOBI_AU_MAX_CHANNELS) return MOBI_E_ARG;
  if (n_streams < 1 || (int64_t)n_streams * n_channels >= (1 << 24)) return MOBI_E_ARG;
  if (max_blocks < 1 || max_blocks > MOBI_AENC_MAX_BLOCKS) return MOBI_E_ARG;
  return MOBI_OK;
}

// every refusal of an encode call that needs no device
MOBI_AU_FN int mobi_aenc_check_call(int codec, int n_streams, int n_channels, int max_blocks, int n, const void *samples, size_t sample_pitch, int blocks,
                                    const void *slots, size_t slot_pitch, size_t slot_bytes, const void *sizes, const void *recon, size_t recon_pitch,
                                    const void *stats) {
  const int rc = mobi_aenc_check_create(codec, n_streams, n_channels, max_blocks);
  if (rc != MOBI_OK) return rc;
  if (!samples || !slots || !sizes || (uintptr_t)samples % 2 || (uintptr_t)slots % 4 || (uintptr_t)sizes % 4) return MOBI_E_ARG;
  if ((uintptr_t)recon % 2 || (uintptr_t)stats % 8) return MOBI_E_ARG;
  if (n < 1 || n > n_streams || blocks < 1 || blocks > max_blocks) return MOBI_E_ARG;
  const size_t S = (size_t)MOBI_AU_BLOCK_SAMPLES * (size_t)blocks;
  if (sample_pitch < S || (recon && recon_pitch < S)) return MOBI_E_ARG;
  if (slot_bytes % 4 || slot_pitch % 4 || slot_pitch < slot_bytes || slot_bytes > 0x7FFFFFFC) return MOBI_E_ARG;
  if (slot_bytes < mobi_aenc_frame_bytes(codec, (uint64_t)n_channels, (uint64_t)blocks)) return MOBI_E_ARG;
  return MOBI_OK;
}

// what the step from `st` adds or takes for `val`, before the clamp: mobi_ima_sample's difference restated, for the `clamped` count alone
MOBI_AU_FN int32_t mobi_aenc_raw(uint32_t val, const MobiImaState &st, const int16_t *step_tab) {
  const int32_t step = step_tab[st.index];
  const int32_t diff = step / 8 + ((val & 1) ? step / 4 : 0) + ((val & 2) ? step / 2 : 0) + ((val & 4) ? step : 0);
  return st.last + ((val & 8) ? -diff : diff);
}

// THE nibble: the val whose decoded sample is nearest to x, the smallest such; the state is not moved
MOBI_AU_FN uint32_t mobi_aenc_nibble(int32_t x, const MobiImaState &st, const int16_t *step_tab) {
  uint32_t best = 0;
  int32_t best_d = 0x7FFFFFFF;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t val = 0; val < 16; val++) {
    MobiImaState t = st;
    const int32_t d = x - mobi_ima_sample(val, t, step_tab);
    const int32_t ad = d < 0 ? -d : d;
    if (ad < best_d) {
      best_d = ad;
      best = val;
    }
  }
  return best;
}

// one sample: its nibble; the state advances as the decoder's does; *r the reconstruction, *clamped counts the decoder's clamp acting
MOBI_AU_FN uint32_t mobi_aenc_sample(int32_t x, MobiImaState &st, const int16_t *step_tab, int32_t *r, uint32_t *clamped) {
  const uint32_t val = mobi_aenc_nibble(x, st, step_tab);
  const int32_t raw = mobi_aenc_raw(val, st, step_tab);
  *r = mobi_ima_sample(val, st, step_tab);
  *clamped += raw != *r;
  return val;
}

// E(i0) of the header rule: the squared error of `n` samples coded from (x[0], i0)
template <class Load> MOBI_AU_FN uint64_t mobi_aenc_trial(Load x, int n, int32_t i0, const int16_t *step_tab) {
  MobiImaState st = {x(0), i0};
  uint64_t e = 0;
  uint32_t unused = 0;
  for (int k = 0; k < n; k++) {
    int32_t r;
    const int32_t v = x(k);
    mobi_aenc_sample(v, st, step_tab, &r, &unused);
    const int64_t d = (int64_t)v - r;
    e += (uint64_t)(d * d);
  }
  return e;
}

// (E, i0) as one key whose minimum is the rule's choice: E < 2^41, so the index rides in the low 7 bits and ties go to the smallest
MOBI_AU_FN uint64_t mobi_aenc_key(uint64_t e, uint32_t i0) { return e << 7 | i0; }
MOBI_AU_FN uint32_t mobi_aenc_key_index(uint64_t key) { return (uint32_t)(key & 127); }

// what the kernels read
struct MobiAencArgs {
  const int16_t *step;     // device: mobi_ima_step, 96 entries
  uint32_t *start;         // device: [n_streams * n_channels], the trial kernel's choice for the encode kernel
  const int16_t *samples;  // [stream][channel][sample_pitch]
  uint64_t sample_pitch;
  uint8_t *slots;
  uint64_t slot_pitch;
  int32_t *sizes;
  int16_t *recon;          // [stream][channel][recon_pitch], or NULL
  uint64_t recon_pitch;
  MobiAencStats *stats;    // [stream][channel], or NULL
  uint32_t n_lanes, n_channels, blocks;
  int32_t codec;
};
#endif
