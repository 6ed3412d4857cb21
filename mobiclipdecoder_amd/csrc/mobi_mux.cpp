// mobi_mux.cpp -- HOST: the entry points of include/mobiclip_mux.h.  The object holds what it was made with, one device allocation (the
// clips' states, then their key-frame tables) and the rows of the session begun last.  Every _async call checks its arguments, fills a
// MobiMuxArgs and enqueues the kernels of mobi_mux.hip: no allocation, no wait, no device value read here.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>

#include "mobi_mux.h"

extern "C" int mobi_launch_mux_begin(const MobiMuxArgs *a, hipStream_t s);
extern "C" int mobi_launch_mux_begin_audio(const MobiMuxArgs *a, const MobiMuxAudio *au, hipStream_t s);
extern "C" int mobi_launch_mux_append(const MobiMuxArgs *a, hipStream_t s);
extern "C" int mobi_launch_mux_append_audio(const MobiMuxArgs *a, hipStream_t s);
extern "C" int mobi_launch_mux_finish(const MobiMuxArgs *a, hipStream_t s);

struct mobi_mux {
  MobiMuxCfg cfg;
  MobiMuxAudio audio; // mobi_mux_set_audio; frequency 0: none
  int max_clips, device;
  uint8_t *mem; // the one allocation: states, then key-frame tables, each at a multiple of 256 bytes
  MobiMuxState *state;
  uint32_t *keys;
  // the session: set by begin, ended by finish
  uint8_t *files;
  size_t pitch, capacity;
  int n; // 0: none begun
};

extern "C" {

size_t mobi_mux_framed_bytes(int container, size_t stream_bytes) {
  if (container != MOBI_MUX_MOFLEX && container != MOBI_MUX_MODS) return 0;
  return (size_t)mobi_mux_framed(container, stream_bytes);
}

size_t mobi_mux_fixed_bytes(int container, int key_frames) {
  if ((container != MOBI_MUX_MOFLEX && container != MOBI_MUX_MODS) || key_frames < 0) return 0;
  return (size_t)mobi_mux_fixed(container, (uint64_t)key_frames);
}

mobi_mux *mobi_mux_create(int container, uint32_t width, uint32_t height, uint32_t fps_rate, uint32_t fps_scale, uint32_t fps_raw, int max_clips,
                          int max_key_frames, int device) {
  if (container != MOBI_MUX_MOFLEX && container != MOBI_MUX_MODS) return nullptr;
  if (max_clips < 1 || max_clips > 65535 || max_key_frames < 0 || !width || !height) return nullptr;
  if (container == MOBI_MUX_MOFLEX && (width > 0xFFFF || height > 0xFFFF || fps_rate > 0xFFFF || fps_scale > 0xFFFF)) return nullptr;
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  mobi_mux *m = (mobi_mux *)calloc(1, sizeof *m);
  if (!m) return nullptr;
  m->cfg.container = container;
  m->cfg.max_keys = container == MOBI_MUX_MODS ? max_key_frames : 0;
  m->cfg.width = width;
  m->cfg.height = height;
  m->cfg.fps_rate = fps_rate;
  m->cfg.fps_scale = fps_scale;
  m->cfg.fps_raw = fps_raw;
  m->max_clips = max_clips;
  m->device = device;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t states = up((size_t)max_clips * sizeof(MobiMuxState)), keys = up((size_t)max_clips * (size_t)m->cfg.max_keys * 8);
  if (hipMalloc((void **)&m->mem, states + keys) != hipSuccess) {
    free(m);
    return nullptr;
  }
  m->state = (MobiMuxState *)m->mem;
  m->keys = (uint32_t *)(m->mem + states);
  return m;
}

void mobi_mux_destroy(mobi_mux *m) {
  if (!m) return;
  if (m->mem) (void)hipFree(m->mem);
  free(m);
}

static void mux_args(const mobi_mux *m, int n, MobiMuxArgs *a) {
  memset(a, 0, sizeof *a);
  a->cfg = m->cfg;
  a->state = m->state;
  a->keys = m->keys;
  a->files = m->files;
  a->pitch = m->pitch;
  a->capacity = m->capacity;
  a->n = n;
}

int mobi_mux_begin_async(mobi_mux *m, void *stream, int n, uint8_t *files, size_t file_pitch, size_t file_capacity) {
  if (!m || !files || n < 1 || n > m->max_clips || file_pitch < file_capacity) return MOBI_E_ARG;
  if (m->cfg.container == MOBI_MUX_MODS && (uint64_t)file_capacity >= ((uint64_t)1 << 32)) return MOBI_E_ARG;
  if (hipSetDevice(m->device) != hipSuccess) return MOBI_E_DEVICE;
  m->files = files;
  m->pitch = file_pitch;
  m->capacity = file_capacity;
  m->n = 0;
  MobiMuxArgs a;
  mux_args(m, n, &a);
  if ((mobi_mux_has_audio(m->cfg, m->audio) ? mobi_launch_mux_begin_audio(&a, &m->audio, (hipStream_t)stream) : mobi_launch_mux_begin(&a, (hipStream_t)stream)) != 0)
    return MOBI_E_DEVICE;
  m->n = n;
  return MOBI_OK;
}

// the append of both streams: stream_index 0 video, 1 audio
static int mux_append(mobi_mux *m, void *stream, int n, const uint8_t *slots, size_t slot_pitch, size_t slot_bytes, const int32_t *sizes, int key_frame,
                      uint32_t stream_index) {
  if (!m || !slots || !sizes || !m->n || n < 1 || n > m->n) return MOBI_E_ARG;
  if (stream_index && !mobi_mux_has_audio(m->cfg, m->audio)) return MOBI_E_ARG;
  if ((uintptr_t)slots % 4 || (uintptr_t)sizes % 4 || slot_pitch % 4 || slot_bytes % 4 || !slot_bytes || slot_pitch < slot_bytes) return MOBI_E_ARG;
  if (slot_bytes > 0x7FFFFFFC) return MOBI_E_ARG; // a length is an int32
  if (hipSetDevice(m->device) != hipSuccess) return MOBI_E_DEVICE;
  MobiMuxArgs a;
  mux_args(m, n, &a);
  a.slots = slots;
  a.slot_pitch = slot_pitch;
  a.slot_bytes = slot_bytes;
  a.sizes = sizes;
  a.key_frame = key_frame != 0;
  return (stream_index ? mobi_launch_mux_append_audio(&a, (hipStream_t)stream) : mobi_launch_mux_append(&a, (hipStream_t)stream)) == 0 ? MOBI_OK : MOBI_E_DEVICE;
}

int mobi_mux_append_async(mobi_mux *m, void *stream, int n, const uint8_t *slots, size_t slot_pitch, size_t slot_bytes, const int32_t *sizes,
                          int key_frame) {
  return mux_append(m, stream, n, slots, slot_pitch, slot_bytes, sizes, key_frame, 0);
}

// ---- include/mobiclip_mux_audio.h ----
int mobi_mux_set_audio(mobi_mux *m, int codec_id, uint32_t frequency, int channels) {
  if (!m || m->n) return MOBI_E_ARG;
  if (m->cfg.container != MOBI_MUX_MOFLEX) return MOBI_E_UNSUPPORTED;
  if (frequency == 0) {
    m->audio.frequency = m->audio.channels = m->audio.codec = 0;
    return MOBI_OK;
  }
  if (frequency > (1u << 24) || channels < 1 || channels > 8 || codec_id < 0 || codec_id > 2) return MOBI_E_ARG;
  m->audio.frequency = frequency;
  m->audio.channels = (uint32_t)channels;
  m->audio.codec = (uint32_t)codec_id;
  return MOBI_OK;
}

size_t mobi_mux_fixed_bytes_audio(int container, int key_frames, int audio) {
  if ((container != MOBI_MUX_MOFLEX && container != MOBI_MUX_MODS) || key_frames < 0 || (audio && container != MOBI_MUX_MOFLEX)) return 0;
  return (size_t)mobi_mux_fixed(container, (uint64_t)key_frames, audio != 0);
}

int mobi_mux_append_audio_async(mobi_mux *m, void *stream, int n, const uint8_t *slots, size_t slot_pitch, size_t slot_bytes, const int32_t *sizes) {
  return mux_append(m, stream, n, slots, slot_pitch, slot_bytes, sizes, 0, 1);
}

int mobi_mux_finish_async(mobi_mux *m, void *stream, int n, int64_t *file_bytes_out, int32_t *status_out) {
  if (!m || !file_bytes_out || !status_out || !m->n || n != m->n) return MOBI_E_ARG;
  if ((uintptr_t)file_bytes_out % 8 || (uintptr_t)status_out % 4) return MOBI_E_ARG;
  if (hipSetDevice(m->device) != hipSuccess) return MOBI_E_DEVICE;
  MobiMuxArgs a;
  mux_args(m, n, &a);
  a.bytes_out = file_bytes_out;
  a.status_out = status_out;
  m->n = 0;
  return mobi_launch_mux_finish(&a, (hipStream_t)stream) == 0 ? MOBI_OK : MOBI_E_DEVICE;
}

} // extern "C"
