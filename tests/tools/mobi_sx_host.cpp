// mobi_sx_host.cpp -- TEST TOOL: the host build of the Sx arithmetic header (csrc/mobi_sx.h), packet by packet as the kernel (mobi_sx.hip)
// walks it, so that tests/test_sx_model.py can hold samples AND STATE against the Python model without a GPU.  The state travels as the
// reference's Internal array (558 int32 words): the mapping between it and MobiSxState is here.
//
// With -DMOBI_SX_HOST_MAIN it is a stand-alone program for the host sanitizers: every argument is a file holding a codebook (0xC34
// bytes) and packets back to back; it decodes each from a new decoder, prints the samples' CRC-32, and sweeps mobi_sx_plan over
// exactly-sized heap copies of the packets.
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -DMOBI_SX_HOST_MAIN -I mobiclipdecoder_amd/csrc
//       tests/tools/mobi_sx_host.cpp mobiclipdecoder_amd/csrc/mobi_audio_plan.cpp -o sx_host_san && ./sx_host_san case.bin ...
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/mobiclip_hip.h"
#include "../../include/mobiclip_sx.h"
#include "mobi_sx.h"

enum { kInternalWords = 0x8B8 / 4, kSum = 0x00 / 4, kSetA = 0x20 / 4, kSetB = 0x40 / 4, kGain = 0x60 / 4, kParity = 0x64 / 4, kHist = 0x70 / 4, kBuf = 0xB8 / 4 };
// words 0x68 (rows and rate) and 0x6C (output cursor) are written before they are read in every packet: no state, left as they are

static void from_internal(const int32_t *I, MobiSxState &st, int32_t *buf) {
  memcpy(st.sum, I + kSum, sizeof st.sum);
  st.gain = I[kGain], st.parity = I[kParity];
  memcpy(st.last, I + (st.parity == 0 ? kSetB : kSetA), sizeof st.last);
  memcpy(st.stale, I + (st.parity == 0 ? kSetA : kSetB), sizeof st.stale);
  memcpy(st.h, I + kHist, sizeof st.h);
  memcpy(buf, I + kBuf, MOBI_SX_BUF_WORDS * 4);
}
static void to_internal(const MobiSxState &st, const int32_t *buf, int32_t *I) {
  memcpy(I + kSum, st.sum, sizeof st.sum);
  I[kGain] = st.gain, I[kParity] = st.parity;
  memcpy(I + (st.parity == 0 ? kSetB : kSetA), st.last, sizeof st.last);
  memcpy(I + (st.parity == 0 ? kSetA : kSetB), st.stale, sizeof st.stale);
  memcpy(I + kHist, st.h, sizeof st.h);
  memcpy(I + kBuf, buf, MOBI_SX_BUF_WORDS * 4);
}

// one packet as the kernel decodes it: two chunks of 64 samples, two quarters each, eight samples at a time
static int packet(MobiSxState &st, int32_t *buf, const uint8_t *cb, const uint8_t *p, int16_t *out) {
  MobiSxPacket pk;
  const int n = mobi_sx_begin(st, buf, cb, p, pk);
  for (int q = 0; q < 4; q++) {
    int32_t c[8];
    mobi_sx_quarter(st, pk, q, c);
    for (int i = 32 * q; i < 32 * q + 32; i += 8) {
      int32_t e[8], y[8];
      memcpy(e, buf + pk.in + i, sizeof e);
      mobi_sx_filter8(e, c, st.h, y);
      memcpy(buf + pk.out + i, y, sizeof y);
      for (int j = 0; j < 8; j++) out[i + j] = (int16_t)mobi_sx_clamp(y[j]);
    }
  }
  mobi_sx_end(st, pk);
  return n;
}

// internal: the reference's Internal as 558 words, in and out.  p: a whole packet (the caller knows it fits: mobi_sx_plan).  Returns its bytes.
extern "C" int mobi_sx_host_packet(int32_t *internal, const uint8_t *codebook, const uint8_t *p, int16_t *out) {
  MobiSxState st;
  int32_t buf[MOBI_SX_BUF_WORDS];
  from_internal(internal, st, buf);
  const int n = packet(st, buf, codebook, p, out);
  to_internal(st, buf, internal);
  return n;
}

#ifdef MOBI_SX_HOST_MAIN
static uint32_t crc32_of(const void *p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) {
    c ^= ((const uint8_t *)p)[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
  }
  return ~c;
}

int main(int argc, char **argv) {
  for (int f = 1; f < argc; f++) {
    FILE *fp = fopen(argv[f], "rb");
    if (!fp) return 2;
    std::vector<uint8_t> all;
    uint8_t tmp[4096];
    for (size_t n; (n = fread(tmp, 1, sizeof tmp, fp)) > 0;) all.insert(all.end(), tmp, tmp + n);
    fclose(fp);
    if (all.size() < MOBI_SX_CODEBOOK) return 2;
    const std::vector<uint8_t> cb(all.begin(), all.begin() + MOBI_SX_CODEBOOK), data(all.begin() + MOBI_SX_CODEBOOK, all.end()); // own allocations

    // every packet the plan finds, through one new decoder
    size_t n_blocks = 0;
    int32_t ns[1];
    int cur = 0;
    std::vector<mobi_audio_block> blocks(data.size() / 10 + 1);
    uint32_t n_packets = 0;
    for (uint32_t n = 1; n <= blocks.size(); n++) { // the largest count that still fits
      int c = 0;
      if (mobi_sx_plan(1, data.data(), data.size(), 0, n, &c, nullptr, 0, &n_blocks, ns) != MOBI_OK) break;
      n_packets = n;
    }
    if (mobi_sx_plan(1, data.data(), data.size(), 0, n_packets, &cur, blocks.data(), blocks.size(), &n_blocks, ns) != MOBI_OK) return 3;
    std::vector<int32_t> internal(kInternalWords, 0);
    std::vector<int16_t> out(n_blocks * MOBI_SX_SAMPLES);
    size_t used = 0;
    for (size_t b = 0; b < n_blocks; b++) {
      const std::vector<uint8_t> one(data.begin() + blocks[b].offset, data.begin() + (b + 1 < n_blocks ? blocks[b + 1].offset : blocks[b].offset + mobi_sx_packet_bytes((uint32_t)data[blocks[b].offset + 3] << 8)));
      used += (size_t)mobi_sx_host_packet(internal.data(), cb.data(), one.data(), out.data() + b * MOBI_SX_SAMPLES); // a read past the packet is a heap overflow
    }
    printf("%s packets %zu bytes %zu crc %08x\n", argv[f], n_blocks, used, crc32_of(out.data(), out.size() * 2));

    // mobi_sx_plan over exactly-sized heap copies: every length up to a few packets, every channel count up to 3, cursor, count and offset
    uint64_t sum = 0;
    size_t calls = 0;
    for (size_t len = 0; len <= 90 && len <= data.size(); len++) {
      const std::vector<uint8_t> d(data.begin(), data.begin() + len);
      for (int C = 1; C <= 3; C++)
        for (int c0 = 0; c0 < C; c0++)
          for (uint32_t np = 0; np <= 6; np++)
            for (size_t off = 0; off <= len + 1; off += (off < 24 ? 1 : 7)) {
              int c = c0;
              size_t n = 0;
              int32_t s[8];
              mobi_audio_block bl[6];
              const int rc = mobi_sx_plan(C, d.data(), len, off, np, &c, bl, 6, &n, s);
              sum = sum * 31 + (uint64_t)(rc + 16) + n * 7 + (uint64_t)c;
              for (size_t i = 0; i < n && i < 6; i++) // what mobi_audio_decode gathers: the packet's bytes
                for (int j = 0; j < mobi_sx_packet_bytes((uint32_t)d[bl[i].offset + 3] << 8); j++) sum += d[bl[i].offset + j];
              calls++;
            }
    }
    printf("plan calls %zu sum %016llx\n", calls, (unsigned long long)sum);
  }
  return 0;
}
#endif
