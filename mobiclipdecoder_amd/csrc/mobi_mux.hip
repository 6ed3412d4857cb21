// mobi_mux.hip -- the muxer's kernels on gfx950 (mobi_mux.h; include/mobiclip_mux.h; DESIGN.md "Muxing").  Order exists only through
// kernel boundaries on the stream: no wave waits on a value in memory, and no kernel reads a state word another workgroup of the same
// launch writes.
//
// mobi_mux_begin     one lane per clip: the fresh state; the Moflex head.  (A session with an audio stream: mobi_mux_begin_audio and
//                    mobi_mux_append_audio, mobi_mux_audio.hip.)
// mobi_mux_append    grid (pieces, clips), 256 lanes: a workgroup copies the pieces blockIdx.x, blockIdx.x + gridDim.x, ... of its clip's
//                    frame.  It applies the rule's predicate itself (a refused frame writes nothing) and finds every piece's place from
//                    the clip's position alone.  The source (a slot) is 4-byte aligned, the destination has any alignment: every aligned
//                    16-byte word that lies wholly inside the payload is stored whole, assembled from the five source words it spans
//                    (v_alignbyte_b32); the payload's bytes in front of the first and behind the last such word, the piece's header and
//                    its terminating byte are stored bytewise by the first lanes.  Nothing outside [pos, pos + framed) is written.
// mobi_mux_advance   behind it, one lane per clip: status, position, frame count, largest frame, the key-frame table entry.
// mobi_mux_tail      finish, grid (clips), 256 lanes: the Moflex zero tail, or the Mods index and header; the same predicate as
// mobi_mux_finish    behind it, one lane per clip: the status for good, the file's length and the status to the caller.
#include <hip/hip_runtime.h>

#include "mobi_mux.h"
#include "mobi_mux_copy.h" // MUX_LANES, MUX_GRID_X, mux_copy: shared with mobi_mux_audio.hip

extern "C" __global__ __launch_bounds__(64) void mobi_mux_begin(MobiMuxArgs A) {
  const int clip = blockIdx.x * 64 + threadIdx.x;
  if (clip >= A.n) return;
  const MobiMuxState s = mobi_mux_begin_state(A.cfg.container, A.capacity);
  A.state[clip] = s;
  if (s.status || A.cfg.container != MOBI_MUX_MOFLEX) return;
  uint8_t head[MOBI_MUX_MOFLEX_HEAD];
  mobi_mux_moflex_head(A.cfg, head);
  uint8_t *row = A.files + (uint64_t)clip * A.pitch;
#pragma unroll
  for (int i = 0; i < MOBI_MUX_MOFLEX_HEAD; i++) row[i] = head[i];
}

// the body is text shared with mobi_mux_append_audio (mobi_mux_audio.hip: a translation unit of its own, so that this kernel is the code
// it always was)
extern "C" __global__ __launch_bounds__(MUX_LANES) void mobi_mux_append(MobiMuxArgs A) {
#define MUX_STREAM_INDEX 0
#include "mobi_mux_append_body.h"
#undef MUX_STREAM_INDEX
}

extern "C" __global__ __launch_bounds__(64) void mobi_mux_advance(MobiMuxArgs A) {
  const int clip = blockIdx.x * 64 + threadIdx.x;
  if (clip >= A.n) return;
  MobiMuxState s = A.state[clip];
  uint32_t key[2];
  if (mobi_mux_advance(A.cfg, &s, A.sizes[clip], A.slot_bytes, A.capacity, A.key_frame, key)) {
    uint32_t *k = A.keys + ((uint64_t)clip * (uint32_t)A.cfg.max_keys + (s.keys - 1)) * 2;
    k[0] = key[0];
    k[1] = key[1];
  }
  A.state[clip] = s;
}

extern "C" __global__ __launch_bounds__(MUX_LANES) void mobi_mux_tail(MobiMuxArgs A) {
  const int clip = blockIdx.x;
  const MobiMuxState s = A.state[clip];
  if (mobi_mux_finish_status(A.cfg, s, A.capacity)) return;
  uint8_t *row = A.files + (uint64_t)clip * A.pitch;
  const uint32_t lane = threadIdx.x;
  if (A.cfg.container == MOBI_MUX_MOFLEX) {
    uint8_t *d = row + s.pos + (uint64_t)lane * (MOBI_MUX_MOFLEX_TAIL / MUX_LANES);
#pragma unroll
    for (int i = 0; i < MOBI_MUX_MOFLEX_TAIL / MUX_LANES; i++) d[i] = 0;
    return;
  }
  const uint32_t *keys = A.keys + (uint64_t)clip * (uint32_t)A.cfg.max_keys * 2;
  for (uint32_t k = lane; k < s.keys; k += MUX_LANES) {
    uint8_t *d = row + s.pos + 8 * (uint64_t)k;
    mobi_mux_put32le(d, keys[2 * k]);
    mobi_mux_put32le(d + 4, keys[2 * k + 1]);
  }
  if (lane == 0) {
    uint8_t head[MOBI_MUX_MODS_HEAD];
    mobi_mux_mods_head(A.cfg, s, head);
#pragma unroll
    for (int i = 0; i < MOBI_MUX_MODS_HEAD; i++) row[i] = head[i];
  }
}

extern "C" __global__ __launch_bounds__(64) void mobi_mux_finish(MobiMuxArgs A) {
  const int clip = blockIdx.x * 64 + threadIdx.x;
  if (clip >= A.n) return;
  MobiMuxState s = A.state[clip];
  s.status = mobi_mux_finish_status(A.cfg, s, A.capacity);
  if (!s.status) s.pos += mobi_mux_tail_bytes(A.cfg.container, s.keys);
  A.state[clip] = s;
  A.bytes_out[clip] = s.status ? 0 : (int64_t)s.pos;
  A.status_out[clip] = (int32_t)s.status;
}

extern "C" int mobi_launch_mux_begin(const MobiMuxArgs *a, hipStream_t s) {
  hipLaunchKernelGGL(mobi_mux_begin, dim3((a->n + 63) / 64), dim3(64), 0, s, *a);
  return (int)hipGetLastError();
}

extern "C" int mobi_launch_mux_append(const MobiMuxArgs *a, hipStream_t s) {
  const uint32_t pieces = mobi_mux_pieces(a->cfg.container, a->slot_bytes);
  hipLaunchKernelGGL(mobi_mux_append, dim3(pieces < MUX_GRID_X ? pieces : MUX_GRID_X, a->n), dim3(MUX_LANES), 0, s, *a);
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(mobi_mux_advance, dim3((a->n + 63) / 64), dim3(64), 0, s, *a);
  return (int)hipGetLastError();
}

// the advance alone: behind mobi_mux_audio.hip's append kernel
extern "C" int mobi_launch_mux_advance(const MobiMuxArgs *a, hipStream_t s) {
  hipLaunchKernelGGL(mobi_mux_advance, dim3((a->n + 63) / 64), dim3(64), 0, s, *a);
  return (int)hipGetLastError();
}

extern "C" int mobi_launch_mux_finish(const MobiMuxArgs *a, hipStream_t s) {
  hipLaunchKernelGGL(mobi_mux_tail, dim3(a->n), dim3(MUX_LANES), 0, s, *a);
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(mobi_mux_finish, dim3((a->n + 63) / 64), dim3(64), 0, s, *a);
  return (int)hipGetLastError();
}
