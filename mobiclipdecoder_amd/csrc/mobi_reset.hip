// mobi_reset.hip -- new MobiclipDecoder(Width, Height, Version) (MD.cs:41-54) for a list of clips of a batch, on the device side: the decoder
// state a fresh decoder starts from is all zero (dp_init memsets the state ring), so a reset writes zero MobiDevState and MobiDevTail records
// (64 + 1056 bytes per clip) into the state ring entry the next parse reads (mobi_batch_reset_clips, mobi_batch.cpp).  One wave per clip, 70
// 16-byte vector stores per clip over 64 lanes; the list is unique (the host removes duplicates) and every index is below n_clips.
#include <hip/hip_runtime.h>

#include "mobi_dparse.h"

namespace {
constexpr int kStateQuads = (int)(sizeof(MobiDevState) / 16); // 4
constexpr int kTailQuads = (int)(sizeof(MobiDevTail) / 16);   // 66
constexpr int kWavesPerBlock = 4;
} // namespace

extern "C" __global__ __launch_bounds__(64 * kWavesPerBlock) void mobi_reset_state(const int32_t *__restrict__ clips, int count, int n_clips,
                                                                                  MobiDevState *__restrict__ state, MobiDevTail *__restrict__ tail) {
  const int j = blockIdx.x * kWavesPerBlock + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= count) return;
  const int c = clips[j];
  if (c < 0 || c >= n_clips) return; // (the host checked every index: a guard, not a path)
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  uint4 *t = reinterpret_cast<uint4 *>(tail + c);
  uint4 *s = reinterpret_cast<uint4 *>(state + c);
  for (int q = lane; q < kTailQuads + kStateQuads; q += 64) {
    if (q < kTailQuads) t[q] = z;
    else s[q - kTailQuads] = z;
  }
}

extern "C" int mobi_launch_reset_state(const int32_t *clips_dev, int count, int n_clips, MobiDevState *state, MobiDevTail *tail, hipStream_t s) {
  if (count <= 0) return 0;
  hipLaunchKernelGGL(mobi_reset_state, dim3((unsigned)((count + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0, s, clips_dev, count,
                     n_clips, state, tail);
  return (int)hipGetLastError();
}
