// mobi_encode.hip -- the intra encoder on gfx950 (include/mobiclip_encode.h; the rules are mobi_encode.h's, DESIGN.md "Intra encoder").
//
// Stage 1, decide and reconstruct (the trials themselves: mobi_encode_trials.h, shared with the inter encoder's intra mode).  One wave =
// one macroblock.  Its 64 lanes are eight groups of eight: groups 0..2 try the luma modes
// 0, 1, 3 side by side, groups 3..5 the chroma modes, groups 6 and 7 ride along.  A group runs its trial's blocks in sequence (four luma
// blocks; U, then V), one lane = one row of the block: the block coder of mobi_txcode_lanes.h at wave scope.  Every trial keeps
// its own reconstruction in an LDS patch whose border row and column come from the picture's reconstruction, so a block predicts from
// the earlier blocks of the same trial.  The two winners' patches and levels go to memory; lane 0 adds the macroblock to the statistics.
// Macroblock (x, y) needs (x - 1, y) and (x, y - 1): anti-diagonals are independent, and the order between them is kept ONLY by kernel
// boundaries: mobi_enc_decide_diag is launched once per diagonal over all pictures.  The other shape -- mobi_enc_decide_loop, one
// workgroup per picture whose waves share a diagonal's macroblocks with __syncthreads() between diagonals -- was measured against it:
// slower at 8 and 512 pictures, level at 4096; it lives on in the profiling twin for that comparison.  No wave ever waits on memory.
//
// Stage 2, write bits (mobi_encode_write.h, shared with the inter encoder; the I-frame's speller is here).  mobi_enc_scan: one workgroup per
// picture, exclusive scan of the macroblocks' bit lengths behind the 9 header bits, the stream's length, whether it fits its slot.
// mobi_enc_write: one lane per macroblock spells its bit string at its own offset into the zeroed slot: whole 32-bit words by plain
// stores, its first and last (shared with the neighbours) by atomic OR.
#include <hip/hip_runtime.h>

#include "mobi_encode.h"
#include "mobi_encode_trials.h"
#include "mobi_encode_write.h"

namespace {

constexpr int WAVES = MOBI_ENC_TRIAL_WAVES; // per workgroup, both stage-1 shapes
using WaveLds = MobiEncTrialLds;

// one macroblock: the six trials and their argmin (mobi_encode_trials.h), the winners to memory, the record and the statistics by lane 0
__device__ __forceinline__ void encode_mb(const MobiEncArgs &A, int pic, int mbx, int mby, WaveLds &L, const uint8_t *lut) {
  const MobiEncConst *K = A.k;
  const MobiSyncWave wave_sync;
  const int lane = threadIdx.x & 63;
  MobiEncTrialResult R;
  mobi_enc_trials(A, pic, mbx, mby, L, lut, R);
  MobiEncMb *mb = A.mbs + (size_t)pic * ((size_t)A.mbw * A.mbh) + (size_t)mby * A.mbw + mbx;
  mobi_enc_trials_store(A, pic, mbx, mby, L, R, mb);
  if (lane == 0) {
    const uint32_t cbp = R.cbp();
    mb->bits = mobi_enc_mb_header_bits(K, cbp) + R.bl + R.bc;
    mb->luma_mode = (uint8_t)mobi_enc_mode(R.gl);
    mb->chroma_mode = (uint8_t)mobi_enc_mode(R.gc - 3);
    mb->cbp = (uint8_t)cbp;
    mb->pad = 0;
    if (A.stats) {
      mobi_enc_stats *st = A.stats + pic;
      atomicAdd((unsigned long long *)&st->sad, (unsigned long long)(R.sl + R.sc));
      atomicAdd(&st->luma_modes[mobi_enc_mode(R.gl)], 1u);
      atomicAdd(&st->chroma_modes[mobi_enc_mode(R.gc - 3)], 1u);
      if (__popc(cbp)) atomicAdd(&st->coded_blocks, (uint32_t)__popc(cbp));
      if (R.kl + R.kc) atomicAdd(&st->fallback_clamp, R.kl + R.kc);
      if (R.rl + R.rc) atomicAdd(&st->fallback_level, R.rl + R.rc);
    }
  }
  wave_sync(); // the patches and levels are read before the wave's next macroblock writes them
}

__device__ __forceinline__ const uint8_t *stage_lut(const MobiEncArgs &A, uint32_t (&lut32)[MOBI_TC_LUT_BYTES / 4]) { return mobi_enc_trials_stage_lut(A, lut32); }

} // namespace

#if defined(MOBI_PROFILING)
// the shape that was measured against the kept one and did not win ("Intra encoder"): in the profiling twin only, for tools/exp_encode.py
extern "C" __global__ __launch_bounds__(WAVES * 64) void mobi_enc_decide_loop(MobiEncArgs A) {
  __shared__ uint32_t lut32[MOBI_TC_LUT_BYTES / 4];
  __shared__ WaveLds lds[WAVES];
  const uint8_t *lut = stage_lut(A, lut32);
  const int wave = threadIdx.x >> 6, pic = blockIdx.x;
  for (int d = 0; d < A.mbw + A.mbh - 1; d++) {
    int x_lo, count;
    mobi_enc_diag_range(A.mbw, A.mbh, d, &x_lo, &count);
    for (int i = wave; i < count; i += WAVES) encode_mb(A, pic, x_lo + i, d - (x_lo + i), lds[wave], lut);
    __syncthreads(); // this diagonal's reconstruction is written before the next one reads it (every wave arrives, whatever it encoded)
  }
}
#endif

extern "C" __global__ __launch_bounds__(WAVES * 64) void mobi_enc_decide_diag(MobiEncArgs A, int d) {
  __shared__ uint32_t lut32[MOBI_TC_LUT_BYTES / 4];
  __shared__ WaveLds lds[WAVES];
  const uint8_t *lut = stage_lut(A, lut32);
  const int wave = threadIdx.x >> 6, pic = blockIdx.y;
  int x_lo, count;
  mobi_enc_diag_range(A.mbw, A.mbh, d, &x_lo, &count);
  const int i = blockIdx.x * WAVES + wave;
  if (i < count) encode_mb(A, pic, x_lo + i, d - (x_lo + i), lds[wave], lut);
}

// ---- stage 2: mobi_encode_write.h's scan and writer with the I-frame's speller ----
namespace {
struct IntraSpeller {
  __device__ static uint32_t header_bits(const MobiEncArgs &, int) { return MOBI_ENC_HEADER_BITS; }
  template <class Put> __device__ static void header(const MobiEncArgs &A, int pic, Put put) { put(mobi_enc_header(A.yuv_format, A.q[pic]), MOBI_ENC_HEADER_BITS); }
  template <class Put> __device__ static void macroblock(const MobiEncArgs &A, int pic, int i, Put put) {
    mobi_enc_write_mb(A.k, A.mbs + (size_t)pic * ((size_t)A.mbw * A.mbh) + i, put, (uint32_t *)nullptr);
  }
  __device__ static void total(const MobiEncArgs &A, int pic, uint32_t bits) {
    if (A.stats) A.stats[pic].bits = bits;
  }
};
} // namespace

extern "C" __global__ __launch_bounds__(256) void mobi_enc_scan(MobiEncArgs A) { mobi_enc_scan_body<IntraSpeller>(A); }
extern "C" __global__ __launch_bounds__(64) void mobi_enc_write(MobiEncArgs A) { mobi_enc_write_body<IntraSpeller>(A); }

// stages: bit 0 = decide, bit 1 = scan, bit 2 = write (a frame runs all three; a trial of the rate rule, mobi_encode_rate.h, stops behind the
// scan and touches no slot); loop_shape: the profiling twin's other stage-1 shape
extern "C" int mobi_launch_encode(const MobiEncArgs *a, int stages, int loop_shape, hipStream_t s) {
  const int nmb = a->mbw * a->mbh;
  if (stages & 1) {
#if defined(MOBI_PROFILING)
    if (loop_shape) hipLaunchKernelGGL(mobi_enc_decide_loop, dim3(a->n), dim3(WAVES * 64), 0, s, *a);
    else
#endif
      for (int d = 0; d < a->mbw + a->mbh - 1; d++) {
        int x_lo, count;
        mobi_enc_diag_range(a->mbw, a->mbh, d, &x_lo, &count);
        hipLaunchKernelGGL(mobi_enc_decide_diag, dim3((count + WAVES - 1) / WAVES, a->n), dim3(WAVES * 64), 0, s, *a, d);
      }
  }
  if (stages & 2) hipLaunchKernelGGL(mobi_enc_scan, dim3(a->n), dim3(256), 0, s, *a);
  if (stages & 4) hipLaunchKernelGGL(mobi_enc_write, dim3((nmb + 63) / 64, a->n), dim3(64), 0, s, *a);
  return (int)hipGetLastError();
}
