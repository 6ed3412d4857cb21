// mobi_audio_plan.cpp -- the host-only part of the audio decode (include/mobiclip_audio.h): the framing rules of the reference's converter
// (mobi_audio_plan, and mobi_sx_plan of include/mobiclip_sx.h: which bytes of a frame are which channel's blocks) and the tables' getter.  No HIP: the CPU tests and a stand-alone
// host program call these without a GPU; mobi_audio_decode (mobi_audio.cpp) plans every stream with the same function.
#include <stddef.h>
#include <stdint.h>

#include "../../include/mobiclip_audio.h"
#include "../../include/mobiclip_hip.h"
#include "../../include/mobiclip_sx.h"
#include "mobi_audio.h"
#include "mobi_sx.h"

bool mobi_audio_args_ok(int framing, int codec, int C) {
  if (framing != MOBI_AUDIO_FRAMING_MOFLEX && framing != MOBI_AUDIO_FRAMING_MODS) return false;
  if (codec < MOBI_AUDIO_FASTAUDIO || codec > MOBI_AUDIO_SX) return false;
  if (codec == MOBI_AUDIO_PCM16 && framing != MOBI_AUDIO_FRAMING_MOFLEX) return false;
  return C >= 1 && C <= MOBI_AUDIO_MAX_CHANNELS;
}

static int s16le(const uint8_t *p) { return (int16_t)(uint16_t)(p[0] | (p[1] << 8)); }

int mobi_audio_plan(int framing, int codec, int n_channels, const uint8_t *data, size_t len, size_t offset, uint32_t n_packets, int *cursor,
                    const uint8_t *fresh, mobi_audio_block *blocks, size_t max_blocks, size_t *n_blocks, int32_t *n_samples) {
  const int C = n_channels;
  if (!mobi_audio_args_ok(framing, codec, C) || !n_blocks || !n_samples || (!data && len) || (!blocks && max_blocks) || len >= 0xFFFFFFFFull)
    return MOBI_E_ARG;
  const bool mods = framing == MOBI_AUDIO_FRAMING_MODS;
  if (mods && (!cursor || *cursor < 0 || *cursor >= C)) return MOBI_E_ARG;
  *n_blocks = 0;
  for (int c = 0; c < C; c++) n_samples[c] = 0;
  if (codec == MOBI_AUDIO_SX) return MOBI_E_UNSUPPORTED;
  if (len == 0 || (mods && n_packets == 0)) return MOBI_OK;

  size_t n = 0;
  uint32_t per[MOBI_AUDIO_MAX_CHANNELS] = {0};
  auto emit = [&](size_t off, size_t header_off, int c, bool header) {
    if (n < max_blocks) blocks[n] = mobi_audio_block{(uint32_t)off, (uint32_t)header_off, (uint16_t)c, (uint16_t)header};
    n++;
    per[c]++;
  };
  auto header_ok = [&](size_t off) { return (s16le(data + off) & 0x7F) <= 88; }; // StepTable[Index] throws above (IMAADPCMDecoder.cs:38)

  if (codec == MOBI_AUDIO_PCM16) {
    const size_t frames = len / (2 * (size_t)C); // Data.Length - Data.Length % (C * 2) bytes (Program.cs:154)
    if (frames > 0x7FFFFFFF) return MOBI_E_ARG;
    for (int c = 0; c < C; c++) n_samples[c] = (int32_t)frames;
    return MOBI_OK;
  }
  const size_t blk = codec == MOBI_AUDIO_FASTAUDIO ? MOBI_FA_BLOCK_BYTES : MOBI_IMA_BLOCK_BYTES;
  int cur = mods ? *cursor : 0;
  if (!mods && codec == MOBI_AUDIO_FASTAUDIO) {
    // while (offset + 40 < Length) one block per channel (Program.cs:101-112): the reads throw where the C blocks do not fit
    for (size_t off = 0; off + blk < len;) {
      if (blk * C > len - off) return MOBI_E_INDEX;
      for (int c = 0; c < C; c++, off += blk) emit(off, 0, c, false);
    }
  } else if (!mods) {
    // C headers, then while (offset + 128 C < Length) one block per channel (Program.cs:124-142): new decoders every frame
    if ((size_t)MOBI_IMA_HEADER_BYTES * C > len) return MOBI_E_INDEX;
    for (int c = 0; c < C; c++)
      if (!header_ok((size_t)MOBI_IMA_HEADER_BYTES * c)) return MOBI_E_INDEX;
    bool head = true;
    for (size_t off = (size_t)MOBI_IMA_HEADER_BYTES * C; off + blk * C < len; head = false)
      for (int c = 0; c < C; c++, off += blk) emit(off, (size_t)MOBI_IMA_HEADER_BYTES * c, c, head);
  } else {
    // one packet per block, channels round robin from the cursor (Program.cs:266-299); IMA: a new decoder's packet is 132 bytes
    uint8_t is_new[MOBI_AUDIO_MAX_CHANNELS];
    for (int c = 0; c < C; c++) is_new[c] = codec == MOBI_AUDIO_IMA && fresh && fresh[c];
    size_t off = offset;
    for (uint32_t i = 0; i < n_packets; i++) {
      const size_t need = blk + (is_new[cur] ? MOBI_IMA_HEADER_BYTES : 0);
      if (off > len || need > len - off) return MOBI_E_INDEX;
      if (is_new[cur] && !header_ok(off)) return MOBI_E_INDEX;
      emit(off + (is_new[cur] ? MOBI_IMA_HEADER_BYTES : 0), off, cur, is_new[cur]);
      off += need;
      is_new[cur] = 0;
      cur = cur + 1 >= C ? 0 : cur + 1;
    }
  }
  for (int c = 0; c < C; c++) {
    if ((uint64_t)per[c] * MOBI_AU_BLOCK_SAMPLES > 0x7FFFFFFFull) return MOBI_E_ARG;
    n_samples[c] = (int32_t)(per[c] * MOBI_AU_BLOCK_SAMPLES);
  }
  *n_blocks = n;
  if (mods) *cursor = cur;
  return MOBI_OK;
}

// Sx in Mods framing (Program.cs:275-288): one packet per channel, round robin from the cursor; SxDecoder.Decode reads two words, then the
// pulse words its rate asks for, and throws where they end behind the buffer
int mobi_sx_plan(int n_channels, const uint8_t *data, size_t len, size_t offset, uint32_t n_packets, int *cursor, mobi_audio_block *blocks,
                 size_t max_blocks, size_t *n_blocks, int32_t *n_samples) {
  const int C = n_channels;
  if (C < 1 || C > MOBI_AUDIO_MAX_CHANNELS || !n_blocks || !n_samples || (!data && len) || (!blocks && max_blocks) || len >= 0xFFFFFFFFull ||
      !cursor || *cursor < 0 || *cursor >= C)
    return MOBI_E_ARG;
  *n_blocks = 0;
  for (int c = 0; c < C; c++) n_samples[c] = 0;
  if (len == 0 || n_packets == 0) return MOBI_OK;
  uint32_t per[MOBI_AUDIO_MAX_CHANNELS] = {0};
  size_t off = offset;
  int cur = *cursor;
  for (uint32_t i = 0; i < n_packets; i++) {
    if (off > len || len - off < 4) return MOBI_E_INDEX;
    const size_t need = (size_t)mobi_sx_packet_bytes((uint32_t)data[off + 3] << 8);
    if (need > len - off) return MOBI_E_INDEX;
    if (i < max_blocks) blocks[i] = mobi_audio_block{(uint32_t)off, 0, (uint16_t)cur, 0};
    per[cur]++;
    off += need;
    cur = cur + 1 >= C ? 0 : cur + 1;
  }
  for (int c = 0; c < C; c++)
    if ((uint64_t)per[c] * MOBI_SX_SAMPLES > 0x7FFFFFFFull) return MOBI_E_ARG;
  for (int c = 0; c < C; c++) n_samples[c] = (int32_t)(per[c] * MOBI_SX_SAMPLES);
  *n_blocks = n_packets;
  *cursor = cur;
  return MOBI_OK;
}

// mobi_ima_sample computes IndexTable[val] in closed form; the table is what the getter hands out: keep the two the same
constexpr bool ima_index_is_closed_form() {
  for (int v = 0; v < 16; v++)
    if (mobi_ima_index[v] != ((v & 4) ? 2 * (v & 7) - 6 : -1)) return false;
  return true;
}
static_assert(ima_index_is_closed_form(), "mobi_ima_sample's index step differs from mobi_ima_index");

int mobi_audio_table(int which, int32_t *out) {
  const int16_t *t[] = {mobi_fa_k01, mobi_fa_k2, mobi_fa_k3, mobi_fa_k4, mobi_fa_k5, mobi_fa_k6, mobi_fa_k7, mobi_fa_pulse, mobi_ima_index, mobi_ima_step};
  const int n[] = {64, 32, 32, 16, 16, 8, 8, 512, 16, 89};
  if (which < 0 || which >= 10) return MOBI_E_ARG;
  if (out)
    for (int i = 0; i < n[which]; i++) out[i] = t[which][i];
  return n[which];
}

