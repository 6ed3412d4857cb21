// mobi_mux_copy.h -- what the append kernels of mobi_mux.hip and mobi_mux_audio.hip share besides the rule (mobi_mux.h): the launch shape
// and the copy of one piece's payload.  Device code only.
#ifndef MOBI_MUX_COPY_H
#define MOBI_MUX_COPY_H
#include <hip/hip_runtime.h>

enum { MUX_LANES = 256, MUX_GRID_X = 32 }; // pieces of one clip side by side: 32 Moflex blocks are 124 KB, more than a 640x480 frame takes

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
#endif
