// mobi_handover.h -- the staged bitstream image of a device-parsed hand-over: the bytes of K frames of each of n clips (lane v = k * n + c; a
// frame step is K = 1) as the host lays them out in pinned memory and the device reads them.  Host only and free of HIP, so that
// tests/test_stage_image.py holds it against a model of the layout without a GPU (tests/tools/mobi_stage_host.cpp).  The image, in order:
//   [bit_off u64 x lanes][bit_len u32 x lanes]   the header, hdr_bytes = 16-aligned: mobi_parse_frames*, mobi_gop_prepare, mobi_gop_chain
//   the bits: every lane that has any starts 8-aligned at hdr_bytes + bit_off, kBitPad zero bytes (and the alignment's) behind its last
//   zero bytes up to the lists, 64 at least      (a lane without bits has an offset too, and it points at readable, zeroed bytes)
//   the reset list, n_reset x int32 at reset_off (16-aligned): mobi_reset_state
//   the idle list, n_idle x int32 at idle_off (16-aligned): the clips with an idle slot, for mobi_idle_rows
//   idle_from[n] u8 at idle_from_off (16-aligned), groups with an idle slot only: mobi_idle_rows, mobi_gop_prepare, mobi_gop_chain
// A lane whose header says MOBI_DP_SKIP is no device parser's: an idle slot (nothing of it is read, gathered or uploaded) or the host parser's.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

struct StageImage {
  static constexpr size_t kBitPad = 32; // the reader runs two 8-byte registers ahead
  static constexpr uint32_t kSkip = 0xFFFFFFFFu; // MOBI_DP_SKIP (mobi_dparse.h, which needs HIP's headers; mobi_batch.h holds the two together)
  int n = 0, K = 0;
  size_t hdr_bytes = 0, bits_end = 0, bytes = 0, max_len = 0; // bits_end: where the last lane's bits and padding end; max_len: the longest frame (the host parser's too: their share of the payload bound counts)
  size_t reset_off = 0, idle_off = 0, idle_from_off = 0; // (idle_from_off == 0: idle_from does not ride)
  int n_reset = 0, n_idle = 0;
  int n_dev = 0, n_iframes = 0; // lanes the GPU parses; of them, I-frames by their first bit (ls_decide).  Counted when the routing is known
  std::vector<uint64_t> boff;   // [v] where the lane's bytes start, behind the header
  std::vector<uint32_t> lens;   // [v] their number; MOBI_DP_SKIP: the lane has none
  size_t lanes() const { return (size_t)n * K; }
  static size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }
  static bool first_bit(const uint8_t *frame, size_t l) { return l >= 2 && (frame[1] & 0x80) != 0; } // the top bit of the first 16-bit little-endian word (MD.cs:110-113)

  // The layout for data / len / offsets [k * n + c].  idle_from: [c] the clip's first idle frame (K: none), or nullptr; n_resets: clips in the
  // reset list.  The two things steps and groups do differently:
  //   on_host != nullptr (steps: the routing is known): a lane of the host parser's clip has no bytes and says MOBI_DP_SKIP at once.
  //   on_host == nullptr (groups: the parse may be enqueued a finish later): every live lane keeps its bytes -- the host parser reads its own
  //   from the image -- and its length; route() marks the host parser's lanes when the parse is enqueued.
  //   ride_idle_from (groups): idle_from[n] rides behind the idle list.
  void plan(int n_clips, int n_frames, int n_mbs, const uint8_t *const *data, const size_t *len, const int32_t *offsets, const uint8_t *on_host,
            const uint8_t *idle_from, size_t n_resets, bool ride_idle_from) {
    n = n_clips; K = n_frames;
    boff.resize(lanes()); lens.resize(lanes());
    // MOC5 callers pass the whole file as Data (Form1.cs:292-302).  The reader advances two bytes per refill and refills at most
    // once per syntax element: <= ~1450 refills per macroblock (127 partition nodes, 384 levels of up to three reads each), so
    // bytes beyond 4 KB per macroblock cannot influence the parse of this frame
    const size_t frame_bound = (size_t)n_mbs * 4096 + 64;
    size_t pos = 0;
    max_len = 0; n_dev = n_iframes = n_idle = 0;
    for (int k = 0; k < K; k++)
      for (int c = 0; c < n; c++) {
        const size_t v = (size_t)k * n + c;
        boff[v] = pos;
        lens[v] = kSkip;
        if (idle_from && k >= idle_from[c]) continue;
        const int64_t o = offsets[v];
        const size_t l = std::min(data[v] && o >= 0 && (uint64_t)o < len[v] ? len[v] - (size_t)o : 0, frame_bound); // nothing readable: the first ReadU16LE throws
        max_len = std::max(max_len, l);
        if (on_host && on_host[c]) continue;
        lens[v] = (uint32_t)l;
        pos += up(l + kBitPad, 8);
        n_dev++;
        if (on_host && l) n_iframes += first_bit(data[v] + o, l);
      }
    for (int c = 0; c < n && idle_from; c++) n_idle += idle_from[c] < K;
    hdr_bytes = up(lanes() * 12, 16);
    n_reset = (int)n_resets;
    bits_end = hdr_bytes + pos;
    reset_off = up(bits_end + 64, 16);
    idle_off = reset_off + up(n_resets * 4, 16);
    idle_from_off = ride_idle_from && n_idle ? idle_off + up((size_t)n_idle * 4, 16) : 0;
    bytes = idle_from_off ? idle_from_off + up((size_t)n, 16) : idle_off + up((size_t)n_idle * 4, 16);
  }
  // everything but the bits, into an image of `bytes` bytes at hs
  void write_header(uint8_t *hs, const int32_t *resets, const uint8_t *idle_from) const {
    memcpy(hs, boff.data(), lanes() * 8);
    memcpy(hs + lanes() * 8, lens.data(), lanes() * 4);
    memset(hs + bits_end, 0, reset_off - bits_end);
    if (n_reset) memcpy(hs + reset_off, resets, (size_t)n_reset * 4);
    int32_t *list = (int32_t *)(hs + idle_off);
    for (int c = 0; c < n && n_idle; c++)
      if (idle_from[c] < K) *list++ = c;
    if (idle_from_off) memcpy(hs + idle_from_off, idle_from, (size_t)n);
  }
  // lane v's bits and the zeros behind them
  void gather(uint8_t *hs, size_t v, const uint8_t *const *data, const int32_t *offsets) const {
    const size_t l = lens[v];
    if (l == kSkip) return;
    uint8_t *dst = hs + hdr_bytes + boff[v];
    if (l) memcpy(dst, data[v] + offsets[v], l);
    memset(dst + l, 0, up(l + kBitPad, 8) - l);
  }
  // groups, when the parse is enqueued: the host parser's lanes say MOBI_DP_SKIP in the header (lens keeps their length), the others are counted
  void route(uint8_t *hs, const uint8_t *on_host) {
    uint32_t *bit_len = (uint32_t *)(hs + lanes() * 8);
    n_dev = n_iframes = 0;
    for (size_t v = 0; v < lanes(); v++) {
      if (lens[v] == kSkip) continue;
      if (on_host[v % n]) { bit_len[v] = kSkip; continue; }
      n_dev++;
      n_iframes += first_bit(hs + hdr_bytes + boff[v], lens[v]);
    }
  }
};
