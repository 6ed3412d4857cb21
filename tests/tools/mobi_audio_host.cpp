// mobi_audio_host.cpp -- TEST TOOL: the host build of the audio arithmetic header (csrc/mobi_audio.h), block by block as the kernel
// (mobi_audio.hip) walks it, so that tests/test_audio_model.py can hold it against the Python model without a GPU.
//
// With -DMOBI_AUDIO_HOST_MAIN it is a stand-alone program for the host sanitizers: it runs the wild byte sequence of the tests (and a
// tamed copy) through both codecs and through mobi_audio_plan at every length around the framing's boundaries, and prints checksums.
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -DMOBI_AUDIO_HOST_MAIN -I mobiclipdecoder_amd/csrc \
//       tests/tools/mobi_audio_host.cpp mobiclipdecoder_amd/csrc/mobi_audio_plan.cpp -o audio_host_san && ./audio_host_san
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/mobiclip_audio.h"
#include "mobi_audio.h"

// state: s[0..7], de.  out: 256 samples per block.
extern "C" void mobi_audio_host_fastaudio(int32_t *state, const uint8_t *data, int n_blocks, int16_t *out) {
  MobiFaState st;
  memcpy(st.s, state, sizeof st.s);
  st.de = state[8];
  for (int b = 0; b < n_blocks; b++) {
    uint32_t w[10];
    for (int i = 0; i < 10; i++) {
      const uint8_t *p = data + (size_t)b * MOBI_FA_BLOCK_BYTES + 4 * i;
      w[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
    int32_t k[8];
    mobi_fa_coefficients(w[0], mobi_fa_low4(w[3], w[5], w[7], w[9]), mobi_fa_k01, mobi_fa_k2, mobi_fa_k3, mobi_fa_k4, mobi_fa_k5, mobi_fa_k6, mobi_fa_k7, k);
    for (int sub = 0; sub < 4; sub++) {
      MobiFaExc e;
      mobi_fa_exc_begin(e, w[1], sub, w[2 + 2 * sub], w[3 + 2 * sub]);
      for (int p = 0; p < MOBI_AU_CHUNK; p++)
        out[(size_t)b * MOBI_AU_BLOCK_SAMPLES + sub * MOBI_AU_CHUNK + p] = (int16_t)mobi_fa_sample(mobi_fa_exc_next(e, p, mobi_fa_pulse), k, st);
    }
  }
  memcpy(state, st.s, sizeof st.s);
  state[8] = st.de;
}

// state: last, index (0..88)
extern "C" void mobi_audio_host_ima(int32_t *state, const uint8_t *data, int n_blocks, int16_t *out) {
  MobiImaState st = {state[0], state[1]};
  for (size_t i = 0; i < (size_t)n_blocks * MOBI_IMA_BLOCK_BYTES; i++) {
    out[2 * i] = (int16_t)mobi_ima_sample(data[i] & 0xF, st, mobi_ima_step);
    out[2 * i + 1] = (int16_t)mobi_ima_sample(data[i] >> 4, st, mobi_ima_step);
  }
  state[0] = st.last;
  state[1] = st.index;
}

#ifdef MOBI_AUDIO_HOST_MAIN
static uint32_t g_x;
static uint8_t next_byte() {
  g_x = (uint32_t)(((uint64_t)g_x * 1103515245u + 12345u) & 0x7FFFFFFFu);
  return (uint8_t)(g_x >> 16);
}
static uint32_t crc32_of(const void *p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) {
    c ^= ((const uint8_t *)p)[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
  }
  return ~c;
}

int main() {
  // the wild FastAudio set of the tests: eight blocks from x = 1; then the same with every gain forced to at most 8
  std::vector<uint8_t> fa(8 * MOBI_FA_BLOCK_BYTES);
  g_x = 1;
  for (auto &b : fa) b = next_byte();
  std::vector<int16_t> out(8 * MOBI_AU_BLOCK_SAMPLES);
  int32_t st[9] = {0};
  mobi_audio_host_fastaudio(st, fa.data(), 8, out.data());
  printf("fastaudio wild crc %08x\n", crc32_of(out.data(), out.size() * 2));
  for (int b = 0; b < 8; b++) {
    uint8_t *p = fa.data() + b * MOBI_FA_BLOCK_BYTES + 4;
    uint32_t w = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    for (int sh = 8; sh < 32; sh += 6) {
      const uint32_t g = (w >> sh) & 0x3F;
      w = (w & ~(0x3Fu << sh)) | ((g > 8 ? 8 : g) << sh);
    }
    p[0] = (uint8_t)w, p[1] = (uint8_t)(w >> 8), p[2] = (uint8_t)(w >> 16), p[3] = (uint8_t)(w >> 24);
  }
  memset(st, 0, sizeof st);
  mobi_audio_host_fastaudio(st, fa.data(), 8, out.data());
  printf("fastaudio tame crc %08x\n", crc32_of(out.data(), out.size() * 2));
  // the IMA set: four blocks from x = 7, started at last = -1234, index = 40
  std::vector<uint8_t> ima(4 * MOBI_IMA_BLOCK_BYTES);
  g_x = 7;
  for (auto &b : ima) b = next_byte();
  int32_t is[2] = {-1234, 40};
  out.resize(4 * MOBI_AU_BLOCK_SAMPLES);
  mobi_audio_host_ima(is, ima.data(), 4, out.data());
  printf("ima crc %08x last %d index %d\n", crc32_of(out.data(), out.size() * 2), is[0], is[1]);

  // mobi_audio_plan over exactly-sized heap copies of wild bytes: every framing, codec, channel count, and every length up to a few
  // blocks (so every boundary d = -1..3 is among them); Mods with every cursor, odd packet counts and new decoders
  std::vector<uint8_t> wild(1100);
  g_x = 3;
  for (auto &b : wild) b = next_byte();
  uint64_t sum = 0;
  size_t calls = 0;
  for (int framing = 0; framing < 2; framing++)
    for (int codec = 0; codec < 4; codec++)
      for (int C = 1; C <= 3; C++)
        for (size_t len = 0; len <= wild.size(); len += (len < 700 ? 1 : 37)) {
          std::vector<uint8_t> data(wild.begin(), wild.begin() + len); // its own allocation: a read past len is a heap overflow
          std::vector<mobi_audio_block> blocks(len / 40 + 8);
          for (int cur = 0; cur < (framing ? C : 1); cur++)
            for (uint32_t np = 0; np <= (framing ? 5u : 0u); np++) {
              uint8_t fresh[8] = {(uint8_t)(np & 1), (uint8_t)(cur & 1), 1, 0, 0, 0, 0, 0};
              int c = cur;
              size_t n = 0;
              int32_t ns[8];
              const int rc = mobi_audio_plan(framing, codec, C, data.data(), len, len % 7, np, &c, fresh, blocks.data(), blocks.size(), &n, ns);
              sum = sum * 31 + (uint64_t)(rc + 16) + n * 7 + (uint64_t)c;
              for (size_t i = 0; i < n && i < blocks.size(); i++) {
                // what mobi_audio_decode reads: the block's bytes and its header
                const size_t blk = codec == MOBI_AUDIO_FASTAUDIO ? MOBI_FA_BLOCK_BYTES : MOBI_IMA_BLOCK_BYTES;
                for (size_t j = 0; j < blk; j++) sum += data[blocks[i].offset + j];
                if (blocks[i].header) sum += data[blocks[i].header_offset] + data[blocks[i].header_offset + 3];
              }
              calls++;
            }
        }
  printf("plan calls %zu sum %016llx\n", calls, (unsigned long long)sum);
  return 0;
}
#endif
