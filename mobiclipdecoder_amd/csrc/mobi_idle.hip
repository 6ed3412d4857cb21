// mobi_idle.hip -- idle frame slots (mobi_batch_set_idle) on the device side.  A clip whose stream has ended still has rows in every table of
// the step: the parse kernels are kept off them (its length says MOBI_DP_SKIP, as for the host parser's clips), and this kernel writes what a
// frame with no macroblock leaves there -- descriptors typed "intra" that no launch list references, a result record with rc 0 and no intra
// macroblock -- so that the unchanged reconstruction launches do nothing for the clip.  In a single step it also carries the clip's decoder
// state from the state ring entry the parse reads to the one it writes (in a group mobi_gop_chain does: mobi_gop.h).  It runs in FRONT of the
// parse kernels: the record it zeroes may still carry the lock-step parser's mark from the step before.
// One wave per idle slot, 16-byte vector stores: 2 * n_mbs for the descriptors (38 per lane at 640x480), 2 for the record, 70 for the state.
#include <hip/hip_runtime.h>

#include "mobi_dparse.h"

namespace {
constexpr int kStateQuads = (int)(sizeof(MobiDevState) / 16); // 4
constexpr int kTailQuads = (int)(sizeof(MobiDevTail) / 16);   // 66
constexpr int kResQuads = (int)(sizeof(MobiDevResult) / 16);  // 2
constexpr int kWavesPerBlock = 4;
static_assert(sizeof(MbDesc) == 32 && sizeof(MobiDevResult) == 32, "two 16-byte stores per record");
} // namespace

// grid: x = idle clips / 4, y = frame of the hand-over
extern "C" __global__ __launch_bounds__(64 * kWavesPerBlock) void mobi_idle_rows(MobiIdleArgs A) {
  const int j = blockIdx.x * kWavesPerBlock + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63, k = blockIdx.y;
  if (j >= A.count || k >= A.K) return;
  const int c = A.clips[j];
  if (c < 0 || c >= A.n) return; // (the host built the list: a guard, not a path)
  if (A.idle_from && k < (int)A.idle_from[c]) return; // a live frame of the clip
  const size_t v = (size_t)k * A.n + c;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u), blank = make_uint4(0u, (unsigned)MOBI_MB_INTRA, 0u, 0u);
  uint4 *d = reinterpret_cast<uint4 *>(A.desc + v * (size_t)A.n_mbs);
  for (int q = lane; q < 2 * A.n_mbs; q += 64) d[q] = (q & 1) ? z : blank;
  if (lane < kResQuads) reinterpret_cast<uint4 *>(A.res + v)[lane] = z;
  if (A.state_out) { // a single step: the entry the next parse reads carries the clip's state on unchanged
    const uint4 *ti = reinterpret_cast<const uint4 *>(A.tail_in + c), *si = reinterpret_cast<const uint4 *>(A.state_in + c);
    uint4 *to = reinterpret_cast<uint4 *>(A.tail_out + c), *so = reinterpret_cast<uint4 *>(A.state_out + c);
    for (int q = lane; q < kTailQuads + kStateQuads; q += 64) {
      if (q < kTailQuads) to[q] = ti[q];
      else so[q - kTailQuads] = si[q - kTailQuads];
    }
  }
}

extern "C" int mobi_launch_idle_rows(const MobiIdleArgs *a, hipStream_t s) {
  if (a->count <= 0 || a->K <= 0) return 0;
  hipLaunchKernelGGL(mobi_idle_rows, dim3((unsigned)((a->count + kWavesPerBlock - 1) / kWavesPerBlock), (unsigned)a->K), dim3(64 * kWavesPerBlock), 0, s, *a);
  return (int)hipGetLastError();
}
