// mobi_mux_audio.hip -- the muxer's kernels for a Moflex session with an audio stream (include/mobiclip_mux_audio.h; mobi_mux.h), beside
// mobi_mux.hip's and in a translation unit of their own: the video-only kernels stay, instruction for instruction, what they were.
//
// mobi_mux_begin_audio    mobi_mux_begin with the 38-byte head: the audio chunk behind the video chunk.
// mobi_mux_append_audio   mobi_mux_append's body (mobi_mux_append_body.h) for stream index 1: one header bit differs.  mobi_mux_advance
//                         (mobi_mux.hip) follows it as it follows the video append.
#include <hip/hip_runtime.h>

#include "mobi_mux.h"
#include "mobi_mux_copy.h"

extern "C" int mobi_launch_mux_advance(const MobiMuxArgs *a, hipStream_t s);

extern "C" __global__ __launch_bounds__(64) void mobi_mux_begin_audio(MobiMuxArgs A, MobiMuxAudio au) {
  const int clip = blockIdx.x * 64 + threadIdx.x;
  if (clip >= A.n) return;
  const MobiMuxState s = mobi_mux_begin_state(A.cfg.container, A.capacity, true);
  A.state[clip] = s;
  if (s.status) return;
  uint8_t head[MOBI_MUX_MOFLEX_HEAD + MOBI_MUX_MOFLEX_AUDIO_CHUNK];
  mobi_mux_moflex_head_audio(A.cfg, au, head);
  uint8_t *row = A.files + (uint64_t)clip * A.pitch;
#pragma unroll
  for (int i = 0; i < MOBI_MUX_MOFLEX_HEAD + MOBI_MUX_MOFLEX_AUDIO_CHUNK; i++) row[i] = head[i];
}

extern "C" __global__ __launch_bounds__(MUX_LANES) void mobi_mux_append_audio(MobiMuxArgs A) {
#define MUX_STREAM_INDEX 1
#include "mobi_mux_append_body.h"
#undef MUX_STREAM_INDEX
}

extern "C" int mobi_launch_mux_begin_audio(const MobiMuxArgs *a, const MobiMuxAudio *au, hipStream_t s) {
  hipLaunchKernelGGL(mobi_mux_begin_audio, dim3((a->n + 63) / 64), dim3(64), 0, s, *a, *au);
  return (int)hipGetLastError();
}

extern "C" int mobi_launch_mux_append_audio(const MobiMuxArgs *a, hipStream_t s) {
  const uint32_t pieces = mobi_mux_pieces(a->cfg.container, a->slot_bytes);
  hipLaunchKernelGGL(mobi_mux_append_audio, dim3(pieces < MUX_GRID_X ? pieces : MUX_GRID_X, a->n), dim3(MUX_LANES), 0, s, *a);
  if (hipGetLastError() != hipSuccess) return 1;
  return mobi_launch_mux_advance(a, s);
}
