// mobi_mux.hip -- the muxer's kernels on gfx950 (mobi_mux.h; include/mobiclip_mux.h; DESIGN.md "Muxing").  Order exists only through
// kernel boundaries on the stream: no wave waits on a value in memory, and no kernel reads a state word another workgroup of the same
// launch writes.
//
// mobi_mux_begin     one lane per clip: the fresh state; the Moflex head.
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

enum { MUX_LANES = 256, MUX_GRID_X = 32 }; // pieces of one clip side by side: 32 Moflex blocks are 124 KB, more than a 640x480 frame takes

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

// the payload of one piece: src is 4-byte aligned and readable up to len rounded up to 4; dst is any address
__device__ __forceinline__ void mux_copy(uint8_t *dst, const uint8_t *src, uint32_t len, uint32_t lane) {
  const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + len;
  uintptr_t a0 = (d0 + 15) & ~(uintptr_t)15, a1 = d1 & ~(uintptr_t)15; // the whole words are [a0, a1)
  if (a0 > a1) a0 = a1 = d1 < a0 ? d1 : a0;                            // none: the head below is the whole payload
  const uint32_t head = (uint32_t)((a0 < d1 ? a0 : d1) - d0);          // < 16, or len
  const uint32_t tail0 = a1 > a0 ? (uint32_t)(a1 - d0) : head;          // bytes [tail0, len) behind the last whole word: < 16
  if (lane < 16) {
    if (lane < head) dst[lane] = src[lane];
  } else if (lane < 32) {
    const uint32_t i = tail0 + (lane - 16);
    if (i < len) dst[i] = src[i];
  }
  if (a1 <= a0) return;
  const uint32_t words = (uint32_t)((a1 - a0) >> 4);
  const uint32_t sh = head & 3; // the source offset of every whole word is head + 16 i: one shift for the piece
  const uint32_t *s4 = (const uint32_t *)(src + (head & ~3u));
  uint4 *d16 = (uint4 *)a0;
  for (uint32_t i = lane; i < words; i += MUX_LANES) {
    const uint32_t *w = s4 + 4 * i;
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    const uint32_t w4 = sh ? w[4] : 0; // with sh == 0 the fifth word may lie behind the slot
    uint4 o;
    o.x = __builtin_amdgcn_alignbyte(w1, w0, sh);
    o.y = __builtin_amdgcn_alignbyte(w2, w1, sh);
    o.z = __builtin_amdgcn_alignbyte(w3, w2, sh);
    o.w = __builtin_amdgcn_alignbyte(w4, w3, sh);
    d16[i] = o;
  }
}

extern "C" __global__ __launch_bounds__(MUX_LANES) void mobi_mux_append(MobiMuxArgs A) {
  const int clip = blockIdx.y;
  const int32_t size = A.sizes[clip];
  const MobiMuxState s = A.state[clip];
  if (mobi_mux_frame_status(A.cfg, s, size, A.slot_bytes, A.capacity, A.key_frame)) return;
  const uint32_t pieces = mobi_mux_pieces(A.cfg.container, (uint64_t)size);
  const uint8_t *slot = A.slots + (uint64_t)clip * A.slot_pitch;
  uint8_t *at = A.files + (uint64_t)clip * A.pitch + s.pos;
  const uint32_t lane = threadIdx.x;
  for (uint32_t p = blockIdx.x; p < pieces; p += gridDim.x) {
    const MobiMuxPiece q = mobi_mux_piece(A.cfg.container, (uint64_t)size, p);
    uint8_t *d = at + q.dst;
    mux_copy(d + q.head_n, slot + q.src, q.len, lane);
    if (lane >= 32 && lane < 32 + MOBI_MUX_PIECE_HEAD_MAX) {
      const uint32_t i = lane - 32;
      if (i < q.head_n) d[i] = mobi_mux_piece_head(q, i);
    } else if (lane == 32 + MOBI_MUX_PIECE_HEAD_MAX && q.term) {
      d[q.head_n + q.len] = 0;
    }
  }
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

extern "C" int mobi_launch_mux_finish(const MobiMuxArgs *a, hipStream_t s) {
  hipLaunchKernelGGL(mobi_mux_tail, dim3(a->n), dim3(MUX_LANES), 0, s, *a);
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(mobi_mux_finish, dim3((a->n + 63) / 64), dim3(64), 0, s, *a);
  return (int)hipGetLastError();
}
