// mobi_mux_audio_host.cpp -- TEST TOOL: the muxing rule (csrc/mobi_mux.h) on the CPU for a session of video AND audio append calls
// (include/mobiclip_mux_audio.h): begin, append and finish as a loop of its own over clips and calls, beside mobi_mux_host.cpp, which stays
// the video-only model it was.  The host model the kernels of csrc/mobi_mux.hip and csrc/mobi_mux_audio.hip are compared against byte for
// byte (tests/test_mux_audio_gpu.py) and that tests/test_mux_audio_model.py compares against a restated writer and, with audio off,
// against mobi_mux_host.cpp's images.
// Built by mobiclipdecoder_amd/build.py (build_muxaudiohost) and, with sanitizers, into tests/tools/audio_enc_host_main.cpp's program.
#include <cstring>

#include "mobi_mux.h"

// One session: begin, T appends, finish.  Arguments as mobi_mux_host.cpp's mux_host_run; audio_frequency != 0: the files carry an audio
// stream; stream_idx[t] says what append call t brings: 0 a video frame, 1 an audio frame (NULL: video only).  The refusals of the
// entry points.
extern "C" int mux_host_run_audio(int container, uint32_t width, uint32_t height, uint32_t fps_rate, uint32_t fps_scale, uint32_t fps_raw, int max_keys, int n,
                                  int T, uint8_t *files, size_t pitch, size_t capacity, const uint8_t *slots, size_t slot_pitch, size_t slot_bytes,
                                  const int32_t *sizes, const uint8_t *key_flags, int64_t *bytes_out, int32_t *status_out, int audio_codec,
                                  uint32_t audio_frequency, int audio_channels, const uint8_t *stream_idx) {
  if (container != MOBI_MUX_MOFLEX && container != MOBI_MUX_MODS) return MOBI_E_ARG;
  if (audio_frequency && container != MOBI_MUX_MOFLEX) return MOBI_E_UNSUPPORTED;
  if (audio_frequency && (audio_frequency > (1u << 24) || audio_channels < 1 || audio_channels > 8 || audio_codec < 0 || audio_codec > 2)) return MOBI_E_ARG;
  if (!files || n < 1 || T < 0 || max_keys < 0 || pitch < capacity || !bytes_out || !status_out) return MOBI_E_ARG;
  if (container == MOBI_MUX_MODS && (uint64_t)capacity >= ((uint64_t)1 << 32)) return MOBI_E_ARG;
  if (T && (!slots || !sizes || !key_flags || slot_pitch % 4 || slot_bytes % 4 || !slot_bytes || slot_pitch < slot_bytes)) return MOBI_E_ARG;
  for (int t = 0; stream_idx && t < T; t++)
    if (stream_idx[t] > 1 || (stream_idx[t] && !audio_frequency)) return MOBI_E_ARG;
  MobiMuxCfg c;
  c.container = container;
  c.max_keys = container == MOBI_MUX_MODS ? max_keys : 0;
  c.width = width;
  c.height = height;
  c.fps_rate = fps_rate;
  c.fps_scale = fps_scale;
  c.fps_raw = fps_raw;
  const MobiMuxAudio au = {audio_frequency, audio_frequency ? (uint32_t)audio_channels : 0, audio_frequency ? (uint32_t)audio_codec : 0};
  const bool audio = mobi_mux_has_audio(c, au);
  uint32_t *keys = new uint32_t[(size_t)c.max_keys * 2 + 1];
  for (int clip = 0; clip < n; clip++) {
    uint8_t *row = files + (size_t)clip * pitch;
    MobiMuxState s = mobi_mux_begin_state(container, capacity, audio);
    if (!s.status && container == MOBI_MUX_MOFLEX) {
      uint8_t head[MOBI_MUX_MOFLEX_HEAD + MOBI_MUX_MOFLEX_AUDIO_CHUNK];
      if (audio) mobi_mux_moflex_head_audio(c, au, head);
      else mobi_mux_moflex_head(c, head);
      memcpy(row, head, (size_t)mobi_mux_head_bytes(container, audio));
    }
    for (int t = 0; t < T; t++) {
      const int32_t size = sizes[(size_t)t * n + clip];
      const uint8_t *slot = slots + ((size_t)t * n + clip) * slot_pitch;
      const uint32_t index = stream_idx ? stream_idx[t] : 0;
      if (!mobi_mux_frame_status(c, s, size, slot_bytes, capacity, key_flags[t])) {
        const uint32_t pieces = mobi_mux_pieces(container, (uint64_t)size);
        for (uint32_t p = 0; p < pieces; p++) {
          const MobiMuxPiece q = mobi_mux_piece(container, (uint64_t)size, p, index);
          uint8_t *d = row + s.pos + q.dst;
          for (uint32_t i = 0; i < q.head_n; i++) d[i] = mobi_mux_piece_head(q, i);
          memcpy(d + q.head_n, slot + q.src, q.len);
          if (q.term) d[q.head_n + q.len] = 0;
        }
      }
      uint32_t key[2];
      const uint32_t at = s.keys;
      if (mobi_mux_advance(c, &s, size, slot_bytes, capacity, key_flags[t], key)) {
        keys[2 * (size_t)at] = key[0];
        keys[2 * (size_t)at + 1] = key[1];
      }
    }
    s.status = mobi_mux_finish_status(c, s, capacity);
    if (!s.status) {
      if (container == MOBI_MUX_MOFLEX) {
        memset(row + s.pos, 0, MOBI_MUX_MOFLEX_TAIL);
      } else {
        for (uint32_t k = 0; k < s.keys; k++) {
          mobi_mux_put32le(row + s.pos + 8 * (size_t)k, keys[2 * (size_t)k]);
          mobi_mux_put32le(row + s.pos + 8 * (size_t)k + 4, keys[2 * (size_t)k + 1]);
        }
        uint8_t head[MOBI_MUX_MODS_HEAD];
        mobi_mux_mods_head(c, s, head);
        memcpy(row, head, sizeof head);
      }
      s.pos += mobi_mux_tail_bytes(container, s.keys);
    }
    bytes_out[clip] = s.status ? 0 : (int64_t)s.pos;
    status_out[clip] = (int32_t)s.status;
  }
  delete[] keys;
  return MOBI_OK;
}

extern "C" uint64_t mux_host_fixed_bytes_audio(int container, int key_frames, int audio) { return mobi_mux_fixed(container, (uint64_t)key_frames, audio != 0); }
extern "C" uint64_t mux_host_framed_bytes_audio(int container, uint64_t stream_bytes) { return mobi_mux_framed(container, stream_bytes); }
