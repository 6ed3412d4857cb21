// mobi_mux.h -- the muxing rule (include/mobiclip_mux.h; DESIGN.md "Muxing"), one definition for the kernels (mobi_mux.hip), the entry
// points (mobi_mux.cpp) and the host models (tests/tools/mobi_mux_host.cpp, mobi_mux_audio_host.cpp).  It frames bytes and never looks inside a stream; it
// includes nothing from the encoders.
//
// A frame of L bytes is cut into PIECES that are placed independently of each other: piece p of a frame that starts at `pos` finds its
// source and its destination from (L, p, pos) alone.
//   Moflex: a piece is a block of at most B = 0xF80 payload bytes: the flag byte 1, an EP header (stream 0: 2 bytes "1 0 0, len - 1 in 13
//   bits" on a block that does not end the frame, 6 bytes "1 0 1, 1 0 0 1, 28 zero bits, len - 1 in 13 bits" on the one that does), the
//   payload, the byte 0.  Every block but the last is full and takes B + 4 bytes, so block p starts at pos + p (B + 4); the frame takes
//   L + 4 (blocks - 1) + 8 bytes, blocks = ceil(L / B).
//   Mods: a piece is a run of at most 4096 bytes at pos + 4 + 4096 p; piece 0 also writes the u32 L << 14 at pos.
//
// Audio (include/mobiclip_mux_audio.h; Moflex only): with a frequency set the head carries a MoLiveStreamAudio chunk for stream 1 behind
// the video chunk and is 38 bytes long; a frame of stream 1 is framed as one of stream 0, the index bits "1 1" in place of "1 0": the
// byte behind the flag byte has 0x40 set.  With audio off every function below gives what it gave before.
#ifndef MOBI_MUX_RULE_H
#define MOBI_MUX_RULE_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/mobiclip_mux.h"
#include "../../include/mobiclip_mux_audio.h"

#if defined(__HIPCC__)
#define MOBI_MUX_FN __host__ __device__ inline
#else
#define MOBI_MUX_FN inline
#endif

enum {
  MOBI_MUX_MOFLEX_HEAD = 30,      // synchro header 14, varbytes 1 and 12, the video chunk 12, varbytes 0 and 0
  MOBI_MUX_MOFLEX_AUDIO_CHUNK = 8, // varbytes 2 and 6, the audio chunk 6: in front of the terminating varbytes when audio is on
  MOBI_MUX_MOFLEX_BLOCK = 0xF80,  // payload bytes of a full block: 0x1000 - 0x80
  MOBI_MUX_MOFLEX_TAIL = 0x1000,  // FinalizeMoflex
  MOBI_MUX_MODS_HEAD = 0x30,
  MOBI_MUX_MODS_PIECE = 4096,
  MOBI_MUX_MODS_FRAME_LIMIT = 1 << 18, // a frame's length field is 18 bits wide
  MOBI_MUX_PIECE_HEAD_MAX = 7,    // the longest piece header: flag byte + 6
};

// what the muxer object was made with
struct MobiMuxCfg {
  int32_t container, max_keys;
  uint32_t width, height, fps_rate, fps_scale, fps_raw;
};
// the audio stream of a Moflex muxer (mobi_mux_set_audio); it stays out of MobiMuxCfg, so that the kernels of a video-only session
// take the arguments, and compile to the code, they always did
struct MobiMuxAudio {
  uint32_t frequency, channels, codec; // frequency 0: no audio stream
};
MOBI_MUX_FN bool mobi_mux_has_audio(const MobiMuxCfg &c, const MobiMuxAudio &au) { return c.container == MOBI_MUX_MOFLEX && au.frequency != 0; }

// a clip's state between the calls, in device memory
struct MobiMuxState {
  uint64_t pos;     // the write position: the file's length so far
  uint32_t frames;  // frames appended
  uint32_t biggest; // the longest of them
  uint32_t keys;    // entries of the key-frame table
  uint32_t status;  // MOBI_MUX_ST_*, sticky
};

MOBI_MUX_FN uint32_t mobi_mux_pieces(int container, uint64_t L) {
  const uint64_t per = container == MOBI_MUX_MOFLEX ? MOBI_MUX_MOFLEX_BLOCK : MOBI_MUX_MODS_PIECE;
  return (uint32_t)((L + per - 1) / per);
}

// the bytes a frame of L >= 1 stream bytes takes in the file
MOBI_MUX_FN uint64_t mobi_mux_framed(int container, uint64_t L) {
  if (container == MOBI_MUX_MOFLEX) return L + 4 * (uint64_t)(mobi_mux_pieces(container, L) - 1) + 8;
  return L + 4;
}

// head + tail, or header + index
MOBI_MUX_FN uint64_t mobi_mux_fixed(int container, uint64_t key_frames, bool audio = false) {
  if (container == MOBI_MUX_MOFLEX) return MOBI_MUX_MOFLEX_HEAD + (audio ? MOBI_MUX_MOFLEX_AUDIO_CHUNK : 0) + MOBI_MUX_MOFLEX_TAIL;
  return MOBI_MUX_MODS_HEAD + 8 * key_frames;
}

MOBI_MUX_FN uint64_t mobi_mux_head_bytes(int container, bool audio = false) {
  if (container != MOBI_MUX_MOFLEX) return MOBI_MUX_MODS_HEAD;
  return MOBI_MUX_MOFLEX_HEAD + (audio ? MOBI_MUX_MOFLEX_AUDIO_CHUNK : 0);
}

// what finish adds behind the last frame
MOBI_MUX_FN uint64_t mobi_mux_tail_bytes(int container, uint32_t keys) { return container == MOBI_MUX_MOFLEX ? (uint64_t)MOBI_MUX_MOFLEX_TAIL : 8 * (uint64_t)keys; }

// begin: the state of a fresh clip; a capacity below the head is refused here
MOBI_MUX_FN MobiMuxState mobi_mux_begin_state(int container, uint64_t capacity, bool audio = false) {
  MobiMuxState s;
  s.pos = mobi_mux_head_bytes(container, audio);
  s.frames = s.biggest = s.keys = 0;
  s.status = s.pos > capacity ? MOBI_MUX_ST_CAPACITY : 0;
  return s;
}

// THE predicate of append: the bits this frame raises; 0 = it is written.  A clip with a status keeps it and takes nothing more.
MOBI_MUX_FN uint32_t mobi_mux_frame_status(const MobiMuxCfg &c, const MobiMuxState &s, int32_t size, uint64_t slot_bytes, uint64_t capacity, int key_frame) {
  if (s.status) return s.status;
  if (size <= 0 || (uint64_t)size > slot_bytes) return MOBI_MUX_ST_STREAM;
  uint32_t bits = 0;
  if (c.container == MOBI_MUX_MODS && size >= MOBI_MUX_MODS_FRAME_LIMIT) bits |= MOBI_MUX_ST_FRAME;
  if (s.pos + mobi_mux_framed(c.container, (uint64_t)size) > capacity) bits |= MOBI_MUX_ST_CAPACITY;
  if (c.container == MOBI_MUX_MODS && key_frame && s.keys >= (uint32_t)c.max_keys) bits |= MOBI_MUX_ST_KEYS;
  return bits;
}

// append, behind the copy: the state after this frame.  key_at: where the clip's table takes (frame number, offset), written when the
// answer is true.
MOBI_MUX_FN bool mobi_mux_advance(const MobiMuxCfg &c, MobiMuxState *s, int32_t size, uint64_t slot_bytes, uint64_t capacity, int key_frame, uint32_t key_at[2]) {
  const uint32_t bits = mobi_mux_frame_status(c, *s, size, slot_bytes, capacity, key_frame);
  if (bits) {
    s->status = bits;
    return false;
  }
  const bool key = c.container == MOBI_MUX_MODS && key_frame;
  if (key) {
    key_at[0] = s->frames;
    key_at[1] = (uint32_t)s->pos;
    s->keys++;
  }
  s->pos += mobi_mux_framed(c.container, (uint64_t)size);
  s->frames++;
  if ((uint32_t)size > s->biggest) s->biggest = (uint32_t)size;
  return key;
}

// finish: the status with the tail's room checked; 0 = the tail is written and the file is pos + tail long
MOBI_MUX_FN uint32_t mobi_mux_finish_status(const MobiMuxCfg &c, const MobiMuxState &s, uint64_t capacity) {
  if (s.status) return s.status;
  return s.pos + mobi_mux_tail_bytes(c.container, s.keys) > capacity ? MOBI_MUX_ST_CAPACITY : 0;
}

// one piece of a frame: where its payload comes from and goes to, and the bytes around it
struct MobiMuxPiece {
  uint64_t src;     // the payload's offset in the stream
  uint64_t dst;     // the piece's offset from the frame's position: its header's first byte
  uint32_t len;     // payload bytes, >= 1
  uint32_t head_n;  // header bytes in front of the payload
  uint32_t term;    // 1: a zero byte follows the payload
  uint64_t head;    // the header's bytes, the first in the lowest byte
};
MOBI_MUX_FN uint8_t mobi_mux_piece_head(const MobiMuxPiece &q, uint32_t i) { return (uint8_t)(q.head >> (8 * i)); }

// stream_index: 0 video, 1 audio (Moflex)
MOBI_MUX_FN MobiMuxPiece mobi_mux_piece(int container, uint64_t L, uint32_t p, uint32_t stream_index = 0) {
  MobiMuxPiece q;
  if (container == MOBI_MUX_MOFLEX) {
    const uint32_t blocks = mobi_mux_pieces(container, L);
    const bool end = p + 1 == blocks;
    q.src = (uint64_t)p * MOBI_MUX_MOFLEX_BLOCK;
    q.dst = (uint64_t)p * (MOBI_MUX_MOFLEX_BLOCK + 4);
    q.len = end ? (uint32_t)(L - q.src) : (uint32_t)MOBI_MUX_MOFLEX_BLOCK;
    const uint32_t v = q.len - 1; // 13 bits
    // byte 0: the flag byte 1, variable packet size
    if (end) { // 1 0 1 | 1 0 0 1 | 28 zero bits | v: 48 bits, (48 + 4) / 8 bytes: B2 00 00 00 v.hi v.lo
      q.head = 1 | (uint64_t)0xB2 << 8 | (uint64_t)(v >> 8) << 40 | (uint64_t)(v & 0xFF) << 48;
      q.head_n = 7;
    } else {   // 1 0 0 | v: 16 bits, (16 + 4) / 8 bytes
      q.head = 1 | (uint64_t)(0x80 | (v >> 8)) << 8 | (uint64_t)(v & 0xFF) << 16;
      q.head_n = 3;
    }
    q.head |= (uint64_t)(stream_index << 6) << 8; // the index bit behind the unary "1"
    q.term = 1;
  } else {
    q.src = (uint64_t)p * MOBI_MUX_MODS_PIECE;
    q.len = L - q.src < MOBI_MUX_MODS_PIECE ? (uint32_t)(L - q.src) : (uint32_t)MOBI_MUX_MODS_PIECE;
    q.term = 0;
    if (p == 0) {
      q.dst = 0;
      q.head_n = 4;
      q.head = (uint32_t)L << 14; // little-endian u32, no audio packets
    } else {
      q.dst = 4 + q.src;
      q.head_n = 0;
      q.head = 0;
    }
  }
  return q;
}

MOBI_MUX_FN void mobi_mux_put16be(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 8);
  p[1] = (uint8_t)v;
}
MOBI_MUX_FN void mobi_mux_put32le(uint8_t *p, uint32_t v) {
  for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}

// the Moflex head: WriteSynchroHeader with ts = 1 (check word 0xAAAA ^ 1) and packet-size field 0x1000, varbytes 1 and 12, the
// MoLiveStreamVideo chunk of stream 0, varbytes 0 and 0
MOBI_MUX_FN void mobi_mux_moflex_head(const MobiMuxCfg &c, uint8_t out[MOBI_MUX_MOFLEX_HEAD]) {
  for (int i = 0; i < MOBI_MUX_MOFLEX_HEAD; i++) out[i] = 0;
  out[0] = 0x4C;
  out[1] = 0x32;
  mobi_mux_put16be(out + 2, 0xAAAA ^ 1);
  out[11] = 1; // ts, big-endian u64 at 4
  mobi_mux_put16be(out + 12, 0x1000);
  out[14] = 1;
  out[15] = 12;
  // out[16] stream index 0, out[17] zero
  mobi_mux_put16be(out + 18, c.fps_rate);
  mobi_mux_put16be(out + 20, c.fps_scale);
  mobi_mux_put16be(out + 22, c.width);
  mobi_mux_put16be(out + 24, c.height);
  out[26] = 1;
  out[27] = 1;
}

// the head of a file with an audio stream: in front of the terminating varbytes, varbytes 2 and 6 and the MoLiveStreamAudio chunk of
// stream 1 (stream index, codec id, frequency - 1 as u24be, channels - 1)
MOBI_MUX_FN void mobi_mux_moflex_head_audio(const MobiMuxCfg &c, const MobiMuxAudio &au, uint8_t out[MOBI_MUX_MOFLEX_HEAD + MOBI_MUX_MOFLEX_AUDIO_CHUNK]) {
  mobi_mux_moflex_head(c, out);
  const uint32_t f = au.frequency - 1;
  out[28] = 2;
  out[29] = 6;
  out[30] = 1;
  out[31] = (uint8_t)au.codec;
  out[32] = (uint8_t)(f >> 16);
  out[33] = (uint8_t)(f >> 8);
  out[34] = (uint8_t)f;
  out[35] = (uint8_t)(au.channels - 1);
  out[36] = out[37] = 0;
}

// the Mods header, known at finish: s.pos is the index offset
MOBI_MUX_FN void mobi_mux_mods_head(const MobiMuxCfg &c, const MobiMuxState &s, uint8_t out[MOBI_MUX_MODS_HEAD]) {
  for (int i = 0; i < MOBI_MUX_MODS_HEAD; i++) out[i] = 0;
  out[0] = 'M';
  out[1] = 'O';
  out[2] = 'D';
  out[3] = 'S';
  out[4] = 0x0A;
  out[6] = 0x0C;
  mobi_mux_put32le(out + 8, s.frames);
  mobi_mux_put32le(out + 12, c.width);
  mobi_mux_put32le(out + 16, c.height);
  mobi_mux_put32le(out + 20, c.fps_raw);
  // audio codec, channels, frequency: 0
  mobi_mux_put32le(out + 32, s.biggest);
  // audio offset 0
  mobi_mux_put32le(out + 40, (uint32_t)s.pos);
  mobi_mux_put32le(out + 44, s.keys);
}

// what the kernels read: the muxer's memory and one session's rows
struct MobiMuxArgs {
  MobiMuxCfg cfg;
  MobiMuxState *state; // [max_clips]
  uint32_t *keys;      // [max_clips][max_keys][2]
  uint8_t *files;
  uint64_t pitch, capacity;
  const uint8_t *slots;
  uint64_t slot_pitch, slot_bytes;
  const int32_t *sizes;
  int64_t *bytes_out;
  int32_t *status_out;
  int32_t n, key_frame;
};
#endif
