// mobi_audio.h -- the audio codecs' tables and per-sample arithmetic (include/mobiclip_audio.h) that the kernels (mobi_audio.hip), the host
// side (mobi_audio.cpp) and a stand-alone host program compile alike, in the manner of mobi_recon_math.h.
//
//   FastAudio   LibMobiclip.Codec.FastAudio.FastAudioDecoder (FastAudioDecoder.cs:41-311): a 40-byte block = ten LE words -> 256 samples.
//               Word 0 picks lattice coefficients 0-4, 6, 7 (:137-143), word 1 four 6-bit gains and four 2-bit offsets (:149-156), words
//               2..9 per 64-sample subframe 21 three-bit pulse codes (:162-283), bit 0 of words 3, 5, 7, 9 coefficient 5 (:284).  A subframe
//               is `offset` zeros, 21 pulses three samples apart, 3 - offset zeros (:287-311); every sample runs through the 8-stage Q15
//               lattice and the one-pole de-emphasis (0x6E14, Q15), is doubled and saturated (:51-70).
//   IMA-ADPCM   MobiConverter.IMAADPCMDecoder.GetWaveData (IMAADPCMDecoder.cs:17-50): 128 bytes -> 256 samples, low nibble first.
//
// All arithmetic is the reference's int32 two's complement THAT WRAPS (C# unchecked): on arbitrary bytes the lattice's products leave
// int32 often, so the wrap is part of the format.  It is computed in uint32_t here (defined behaviour; the low 32 bits of a product do not
// depend on the operands' signs) and shifted right arithmetically as int32_t.  No 24-bit multiply: the states are arbitrary 32-bit values.
#ifndef MOBI_AUDIO_H
#define MOBI_AUDIO_H
#include <stdint.h>

#if defined(__HIPCC__)
#define MOBI_AU_FN static __host__ __device__ __forceinline__
#else
#define MOBI_AU_FN static inline
#endif

enum { MOBI_FA_BLOCK_BYTES = 40, MOBI_IMA_BLOCK_BYTES = 128, MOBI_IMA_HEADER_BYTES = 4, MOBI_AU_BLOCK_SAMPLES = 256,
       MOBI_AU_CHUNK = 64,            // samples a lane stages in LDS before the wave writes rows out: one FastAudio subframe
       MOBI_AU_MAX_CHANNELS = 8 };

// ---- tables: constants of the formats (every entry fits int16; tests/test_audio_model.py pins length and CRC-32 of each) ----
// coefficient tables: index = a field of word 0 (k5: the four low bits of words 3, 5, 7, 9); pulses: [gain 0..63][code 0..7]
static const int16_t mobi_fa_k01[64] = {
    -32665, -32460, -32256, -32051, -31846, -31641, -31436, -31232, -30719, -29901, -29081, -28261, -27443, -26623, -25805, -24985,
    -24165, -23347, -22527, -21300, -19660, -18024, -16384, -14744, -13108, -11468, -9832, -8192, -6552, -4916, -3276, -1640,
    0, 1640, 3276, 4916, 6552, 8192, 9832, 11468, 13108, 14744, 16384, 18024, 19660, 21300, 22527, 23347,
    24167, 24985, 25805, 26623, 27443, 28261, 29081, 29901, 30719, 31232, 31436, 31641, 31846, 32051, 32256, 32460};
static const int16_t mobi_fa_k2[32] = {
    -27443, -26623, -25805, -24985, -24165, -23347, -22527, -21300, -19660, -18024, -16384, -14744, -13108, -11468, -9832, -8192,
    -6552, -4916, -3276, -1640, 0, 1640, 3276, 4916, 6552, 8192, 9832, 11468, 13108, 14744, 16384, 18024};
static const int16_t mobi_fa_k3[32] = {
    -18024, -16384, -14744, -13108, -11468, -9832, -8192, -6552, -4916, -3276, -1640, 0, 1640, 3276, 4916, 6552,
    8192, 9832, 11468, 13108, 14744, 16384, 18024, 19660, 21300, 22527, 23347, 24167, 24985, 25805, 26623, 27443};
static const int16_t mobi_fa_k4[16] = {
    -19664, -17260, -14860, -12456, -10052, -7648, -5248, -2844, -440, 1960, 4364, 6768, 9172, 11572, 13976, 16380};
static const int16_t mobi_fa_k6[8] = {
    -13108, -9176, -5244, -1312, 2620, 6552, 10484, 14412};
static const int16_t mobi_fa_k7[8] = {
    -6556, -2844, 872, 4584, 8296, 12012, 15724, 19436};
static const int16_t mobi_fa_k5[16] = {
    -9832, -7644, -5460, -3276, -1092, 1092, 3276, 5460, 7644, 9832, 12016, 14200, 16384, 18568, 20752, 22527};
static const int16_t mobi_fa_pulse[512] = {
    -28, -20, -12, -4, 4, 12, 20, 28,
    -56, -40, -24, -8, 8, 24, 40, 56,
    -84, -60, -36, -12, 12, 36, 60, 84,
    -112, -80, -48, -16, 16, 48, 80, 112,
    -140, -100, -60, -20, 20, 60, 100, 140,
    -168, -120, -72, -24, 24, 72, 120, 168,
    -196, -140, -84, -28, 28, 84, 140, 196,
    -224, -160, -96, -32, 32, 96, 160, 224,
    -252, -180, -108, -36, 36, 108, 180, 252,
    -280, -200, -120, -40, 40, 120, 200, 280,
    -308, -220, -132, -44, 44, 132, 220, 308,
    -336, -240, -144, -48, 48, 144, 240, 336,
    -364, -260, -156, -52, 52, 156, 260, 364,
    -392, -280, -168, -56, 56, 168, 280, 392,
    -420, -300, -180, -60, 60, 180, 300, 420,
    -448, -320, -192, -64, 64, 192, 320, 448,
    -504, -360, -216, -72, 72, 216, 360, 504,
    -560, -400, -240, -80, 80, 240, 400, 560,
    -616, -440, -264, -88, 88, 264, 440, 616,
    -672, -480, -288, -96, 96, 288, 480, 672,
    -728, -520, -312, -104, 104, 312, 520, 728,
    -784, -560, -336, -112, 112, 336, 560, 784,
    -840, -600, -360, -120, 120, 360, 600, 840,
    -896, -640, -384, -128, 128, 384, 640, 896,
    -1008, -720, -432, -144, 144, 432, 720, 1008,
    -1120, -800, -480, -160, 160, 480, 800, 1120,
    -1232, -880, -528, -176, 176, 528, 880, 1232,
    -1344, -960, -576, -192, 192, 576, 960, 1344,
    -1456, -1040, -624, -208, 208, 624, 1040, 1456,
    -1568, -1120, -672, -224, 224, 672, 1120, 1568,
    -1680, -1200, -720, -240, 240, 720, 1200, 1680,
    -1792, -1280, -768, -256, 256, 768, 1280, 1792,
    -2016, -1440, -864, -288, 288, 864, 1440, 2016,
    -2240, -1600, -960, -320, 320, 960, 1600, 2240,
    -2464, -1760, -1056, -352, 352, 1056, 1760, 2464,
    -2688, -1920, -1152, -384, 384, 1152, 1920, 2688,
    -2912, -2080, -1248, -416, 416, 1248, 2080, 2912,
    -3136, -2240, -1344, -448, 448, 1344, 2240, 3136,
    -3360, -2400, -1440, -480, 480, 1440, 2400, 3360,
    -3584, -2560, -1536, -512, 512, 1536, 2560, 3584,
    -4032, -2880, -1728, -576, 576, 1728, 2880, 4032,
    -4480, -3200, -1920, -640, 640, 1920, 3200, 4480,
    -4928, -3520, -2112, -704, 704, 2112, 3520, 4928,
    -5376, -3840, -2304, -768, 768, 2304, 3840, 5376,
    -5824, -4160, -2496, -832, 832, 2496, 4160, 5824,
    -6272, -4480, -2688, -896, 896, 2688, 4480, 6272,
    -6720, -4800, -2880, -960, 960, 2880, 4800, 6720,
    -7168, -5120, -3072, -1024, 1024, 3072, 5120, 7168,
    -8063, -5759, -3456, -1152, 1152, 3456, 5760, 8064,
    -8959, -6399, -3840, -1280, 1280, 3840, 6400, 8960,
    -9855, -7039, -4224, -1408, 1408, 4224, 7040, 9856,
    -10751, -7679, -4608, -1536, 1536, 4608, 7680, 10752,
    -11647, -8319, -4992, -1664, 1664, 4992, 8320, 11648,
    -12543, -8959, -5376, -1792, 1792, 5376, 8960, 12544,
    -13439, -9599, -5760, -1920, 1920, 5760, 9600, 13440,
    -14335, -10239, -6144, -2048, 2048, 6144, 10240, 14336,
    -16127, -11519, -6912, -2304, 2304, 6912, 11519, 16127,
    -17919, -12799, -7680, -2560, 2560, 7680, 12799, 17919,
    -19711, -14079, -8448, -2816, 2816, 8448, 14079, 19711,
    -21503, -15359, -9216, -3072, 3072, 9216, 15359, 21503,
    -23295, -16639, -9984, -3328, 3328, 9984, 16639, 23295,
    -25087, -17919, -10752, -3584, 3584, 10752, 17919, 25087,
    -26879, -19199, -11520, -3840, 3840, 11520, 19199, 26879,
    -28671, -20479, -12288, -4096, 4096, 12288, 20479, 28671};
static constexpr int16_t mobi_ima_index[16] = {
    -1, -1, -1, -1, 2, 4, 6, 8, -1, -1, -1, -1, 2, 4, 6, 8};
static const int16_t mobi_ima_step[89] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31,
    34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
    157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658,
    724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024,
    3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899,
    15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

// the tables as a kernel reads them: built on the host and uploaded once per device (mobi_audio.cpp); pulse and step go to LDS, the
// coefficient tables are read eight times per block
struct MobiAudioConst {
  int16_t pulse[512];
  int16_t step[96]; // 89 used
  int16_t k01[64], k2[32], k3[32], k4[16], k5[16], k6[8], k7[8];
};

// one (stream, channel) of a decode call -- PCM16: one stream -- as the kernels read it from the front of the staging buffer
struct MobiAudioLane {
  uint32_t off;      // of the lane's blocks (back to back) in the staged bytes; 16-byte aligned.  PCM16: of the stream's bytes
  uint16_t nblk;     // blocks of this call (0: nothing to decode)
  uint8_t flags;     // MOBI_AU_ZERO, MOBI_AU_HEADER
  uint8_t hdr_index; // MOBI_AU_HEADER: the IMA decoder starts from this index (<= 88) and hdr_last
  int32_t hdr_last;
  uint32_t n_pcm;    // PCM16: samples per channel
};
enum { MOBI_AU_ZERO = 1,     // a new decoder: zero the state first (mobi_audio_reset)
       MOBI_AU_HEADER = 2 };
enum { MOBI_AU_STATE_WORDS = 10 }; // per lane in device memory, word w of lane g at state[w * n_lanes + g]: FastAudio s[0..7], de; IMA last, index

struct MobiAudioArgs {
  const MobiAudioConst *k;
  const MobiAudioLane *lanes;
  const uint8_t *data;
  int32_t *state;
  void *dst;
  uint64_t max_samples;
  uint32_t n_lanes;     // n_streams * n_channels (PCM16: n_streams)
  uint32_t n_channels;
  uint32_t pcm_max;     // PCM16: the largest n_pcm of the call
  int32_t codec, dtype, layout; // MOBI_AUDIO_* of include/mobiclip_audio.h
};

// ---- FastAudio ----
struct MobiFaState {
  int32_t s[8];  // Internal[100..107]: s[0] the lattice's input state, s[1..7] the stage states (Internal[108] is written and never read)
  int32_t de;    // Internal[109]: the de-emphasis state
};

MOBI_AU_FN int32_t mobi_au_asr15(uint32_t v) { return (int32_t)(v + 0x4000u) >> 15; } // (v + 0x4000) >> 15, arithmetic

// word 0 and the four low bits -> Internal[0..7] (:137-143, :284)
MOBI_AU_FN void mobi_fa_coefficients(uint32_t w0, uint32_t low4, const int16_t *k01, const int16_t *k2, const int16_t *k3, const int16_t *k4,
                                     const int16_t *k5, const int16_t *k6, const int16_t *k7, int32_t (&k)[8]) {
  k[0] = k01[w0 >> 26];
  k[1] = k01[(w0 >> 20) & 0x3F];
  k[2] = k2[(w0 >> 15) & 0x1F];
  k[3] = k3[(w0 >> 10) & 0x1F];
  k[4] = k4[(w0 >> 6) & 0xF];
  k[5] = k5[low4 & 0xF];
  k[6] = k6[(w0 >> 3) & 7];
  k[7] = k7[w0 & 7];
}
MOBI_AU_FN uint32_t mobi_fa_low4(uint32_t w3, uint32_t w5, uint32_t w7, uint32_t w9) {
  return (w9 & 1) | ((w7 & 1) << 1) | ((w5 & 1) << 2) | ((w3 & 1) << 3);
}
MOBI_AU_FN uint32_t mobi_fa_gain(uint32_t w1, int sub) { return (w1 >> (8 + 6 * sub)) & 0x3F; }   // Internal[12 + sub]
MOBI_AU_FN uint32_t mobi_fa_offset(uint32_t w1, int sub) { return (w1 >> (2 * sub)) & 3; }          // Internal[8 + sub]
// a subframe's 21 codes as one bit string, first code in bits 63..61: ten from each word (bits 31..2), the 21st from both (:187)
MOBI_AU_FN uint64_t mobi_fa_codes(uint32_t wa, uint32_t wb) {
  return ((uint64_t)(wa >> 2) << 34) | ((uint64_t)(wb >> 2) << 4) | ((uint64_t)(((wb >> 1) & 1) | ((wa & 3) << 1)) << 1);
}
// one sample: excitation x through the lattice (:56-63), the de-emphasis, doubled and saturated (:64-68)
MOBI_AU_FN int32_t mobi_fa_sample(int32_t x, const int32_t (&k)[8], MobiFaState &st) {
  uint32_t r5 = (uint32_t)x;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int j = 0; j < 8; j++) {
    const uint32_t r6 = (uint32_t)k[7 - j], r7 = (uint32_t)st.s[7 - j];
    r5 -= (uint32_t)mobi_au_asr15(r6 * r7);
    if (j) st.s[8 - j] = (int32_t)(r7 + (uint32_t)mobi_au_asr15(r6 * r5));
  }
  st.s[0] = (int32_t)r5;
  const uint32_t r9 = r5 + (uint32_t)mobi_au_asr15((uint32_t)st.de * 0x6E14u);
  st.de = (int32_t)r9;
  const int32_t r8 = (int32_t)(r9 * 2u);
  return r8 > 32767 ? 32767 : r8 < -32768 ? -32768 : r8;
}
// The excitation of a subframe, sample by sample and never stored: sample p is a pulse iff q = p - offset >= 0, q % 3 == 0 and
// q / 3 <= 20.  `ph` walks q % 3 (negative before the first pulse); `codes` loses its top three bits at every pulse.
struct MobiFaExc {
  uint64_t codes;
  int32_t ph, last, gain8;
};
MOBI_AU_FN void mobi_fa_exc_begin(MobiFaExc &e, uint32_t w1, int sub, uint32_t wa, uint32_t wb) {
  const int32_t off = (int32_t)mobi_fa_offset(w1, sub);
  e.codes = mobi_fa_codes(wa, wb);
  e.ph = -off;
  e.last = 60 + off;
  e.gain8 = (int32_t)mobi_fa_gain(w1, sub) * 8;
}
MOBI_AU_FN int32_t mobi_fa_exc_next(MobiFaExc &e, int p, const int16_t *pulse) {
  const bool hit = e.ph == 0 && p <= e.last;
  const int32_t x = hit ? (int32_t)pulse[e.gain8 + (int32_t)(e.codes >> 61)] : 0;
  if (hit) e.codes <<= 3;
  e.ph = e.ph == 2 ? 0 : e.ph + 1;
  return x;
}

// ---- IMA-ADPCM ----
struct MobiImaState {
  int32_t last, index;
};
// one nibble (IMAADPCMDecoder.cs:35-46); index in 0..88 on entry and on exit.  IndexTable[val & 7] is -1 below 4, else 2 * (val & 7) - 6
// (mobi_audio_plan.cpp holds the static_assert that mobi_ima_index, which the getter hands out, says the same).
MOBI_AU_FN int32_t mobi_ima_sample(uint32_t val, MobiImaState &st, const int16_t *step_tab) {
  const int32_t step = step_tab[st.index];
  const int32_t diff = step / 8 + ((val & 1) ? step / 4 : 0) + ((val & 2) ? step / 2 : 0) + ((val & 4) ? step : 0);
  int32_t samp = st.last + ((val & 8) ? -diff : diff);
  samp = samp > 32767 ? 32767 : samp < -32768 ? -32768 : samp;
  st.last = samp;
  int32_t idx = st.index + ((val & 4) ? 2 * (int32_t)(val & 7) - 6 : -1);
  st.index = idx < 0 ? 0 : idx > 88 ? 88 : idx;
  return samp;
}

#endif
