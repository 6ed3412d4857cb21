// mobi_encode_pintra.hip -- the inter encoder's intra mode on gfx950 (include/mobiclip_encode_pintra.h; the rules are mobi_encode_pintra.h's,
// DESIGN.md "Inter encoder", "Intra macroblocks").  Search and code run as in mode 0, one launch each over all macroblocks; the mode's code
// kernel (mobi_encp_code_pintra, mobi_encode_inter.hip) leaves every macroblock's inter coding, its cost Jp and its kind word.
//
// Decide (mobi_encpi_decide).  An intra macroblock predicts from the frame's final reconstruction of the macroblocks to its left and above,
// whatever their kind, so the decisions of an anti-diagonal need those of the one before: one launch per anti-diagonal over all pictures,
// one wave per macroblock, four to a workgroup, kernel boundaries the only ordering -- the shape the intra encoder measured best
// (mobi_encode.hip).  A wave whose Jp cannot be beaten (mobi_encpi_skip) ends at once.  Otherwise it runs the six trials of
// mobi_encode_trials.h on A.rec and compares; where intra wins it overwrites the macroblock's pixels, its record, its kind, and zeroes its
// vector: the effective vector the neighbours' predictors see.  No wave waits on memory.
//
// Finish (mobi_encpi_finish).  One launch, one lane per macroblock: the predictor from the effective vectors, the bits in front of
// ue(cbp), the record's length, the picture's statistics (summed per wave, then integer atomics).
//
// Scan / write.  mobi_encode_write.h's bodies with a speller that writes either kind.
#include <hip/hip_runtime.h>

#include "mobi_encode_pintra.h"
#include "mobi_encode_trials.h"
#include "mobi_encode_write.h"

namespace {
constexpr int WAVES = MOBI_ENC_TRIAL_WAVES;
constexpr int FINISH_THREADS = 256;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
  return v;
}
} // namespace

extern "C" __global__ __launch_bounds__(WAVES * 64) void mobi_encpi_decide(MobiEncInterArgs A, int d) {
  __shared__ uint32_t lut32[MOBI_TC_LUT_BYTES / 4];
  __shared__ MobiEncTrialLds lds[WAVES];
  const uint8_t *lut = mobi_enc_trials_stage_lut(A, lut32);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, pic = blockIdx.y;
  int x_lo, count;
  mobi_enc_diag_range(A.mbw, A.mbh, d, &x_lo, &count);
  const int i = blockIdx.x * WAVES + wave;
  if (i >= count) return; // a whole wave: nothing below synchronises beyond the wave
  const int mbx = x_lo + i, mby = d - mbx;
  const size_t at = (size_t)pic * ((size_t)A.mbw * A.mbh) + (size_t)mby * A.mbw + mbx;
  const int64_t lam = mobi_enc_lambda(A.q[pic]), jp = A.jp[at];
  if (mobi_encpi_skip(A.kp, A.ver, lam, jp)) return; // the same for the whole wave
  MobiEncTrialResult R;
  mobi_enc_trials(A, pic, mbx, mby, lds[wave], lut, R);
  const uint32_t cbp = R.cbp();
  if (!mobi_encpi_wins(mobi_encpi_ji(A.kp, A.ver, lam, R.Jl + R.Jc, cbp), jp)) return;
  MobiEncMb *mb = A.mbs + at;
  mobi_enc_trials_store(A, pic, mbx, mby, lds[wave], R, mb);
  if (lane == 0) {
    mb->bits = mobi_encpi_header_bits(A.kp, A.ver, cbp) + R.bl + R.bc;
    mb->luma_mode = (uint8_t)mobi_enc_mode(R.gl);
    mb->chroma_mode = (uint8_t)mobi_enc_mode(R.gc - 3);
    mb->cbp = (uint8_t)cbp;
    mb->pad = 0;
    A.kind[at] = mobi_encpi_kind(true, R.sl + R.sc, R.kl + R.kc, R.rl + R.rc);
    A.mv[at] = 0u;
  }
}

extern "C" __global__ __launch_bounds__(FINISH_THREADS) void mobi_encpi_finish(MobiEncInterArgs A) {
  const int pic = blockIdx.y, nmb = A.mbw * A.mbh, i = blockIdx.x * FINISH_THREADS + threadIdx.x;
  const bool live = i < nmb;
  uint32_t sad = 0, vb = 0, coded = 0, clamp = 0, range = 0, code0 = 0, nonzero = 0, halfpel = 0, intra_n = 0;
  if (live) {
    const size_t at = (size_t)pic * nmb + i;
    const uint32_t *mvs = A.mv + (size_t)pic * nmb;
    const int mby = i / A.mbw, mbx = i - mby * A.mbw;
    const uint32_t kind = A.kind[at], v = mvs[i];
    const bool intra = mobi_encpi_is_intra(kind);
    MobiEncMb *mb = A.mbs + at;
    uint32_t pred;
    vb = mobi_encpi_finish_mb(A.kp, A.ver, mvs, A.mbw, mbx, mby, intra, &pred);
    A.mvp[at] = pred;
    const uint32_t cbp = mb->cbp;
    if (!intra) mb->bits += vb + mobi_encp_cbp_bits(A.kp, cbp);
    sad = mobi_encpi_sad(kind);
    coded = (uint32_t)__popc(cbp);
    clamp = mobi_encpi_clamp(kind);
    range = mobi_encpi_range(kind);
    intra_n = intra;
    if (!intra) {
      code0 = v == pred;
      nonzero = v != 0;
      halfpel = ((mobi_encp_dx(v) | mobi_encp_dy(v)) & 1) != 0;
    }
  }
  if (!A.pstats) return;
  // per wave: sad < 64 * 2^17, everything else smaller
  sad = wave_sum(sad); vb = wave_sum(vb); coded = wave_sum(coded); clamp = wave_sum(clamp); range = wave_sum(range);
  code0 = wave_sum(code0); nonzero = wave_sum(nonzero); halfpel = wave_sum(halfpel); intra_n = wave_sum(intra_n);
  if ((threadIdx.x & 63) == 0) {
    mobi_enc_inter_stats *st = A.pstats + pic;
    if (sad) atomicAdd((unsigned long long *)&st->sad, (unsigned long long)sad);
    if (vb) atomicAdd((unsigned long long *)&st->mv_bits, (unsigned long long)vb);
    if (coded) atomicAdd(&st->coded_blocks, coded);
    if (clamp) atomicAdd(&st->fallback_clamp, clamp);
    if (range) atomicAdd(&st->fallback_level, range);
    if (code0) atomicAdd(&st->code0, code0);
    if (nonzero) atomicAdd(&st->nonzero_mv, nonzero);
    if (halfpel) atomicAdd(&st->halfpel_mv, halfpel);
    if (intra_n) atomicAdd(&st->reserved[MOBI_ENC_PINTRA_STAT_INTRA], intra_n);
  }
}

// ---- write: mobi_encode_write.h's scan and writer with a speller of either kind ----
namespace {
struct PintraSpeller {
  __device__ static uint32_t header_bits(const MobiEncInterArgs &A, int pic) { return (uint32_t)mobi_encp_header_bits(A.q[pic], A.prev_q[pic]); }
  template <class Put> __device__ static void header(const MobiEncInterArgs &A, int pic, Put put) { mobi_encp_write_header(put, A.q[pic], A.prev_q[pic]); }
  template <class Put> __device__ static void macroblock(const MobiEncInterArgs &A, int pic, int i, Put put) {
    const size_t at = (size_t)pic * ((size_t)A.mbw * A.mbh) + i;
    mobi_encpi_write_mb(A.kp, A.ver, A.mbs + at, mobi_encpi_is_intra(A.kind[at]), A.mv[at], A.mvp[at], put, (uint32_t *)nullptr);
  }
  __device__ static void total(const MobiEncInterArgs &A, int pic, uint32_t bits) {
    if (A.pstats) A.pstats[pic].bits = bits;
  }
};
} // namespace

extern "C" __global__ __launch_bounds__(256) void mobi_encpi_scan(MobiEncInterArgs A) { mobi_enc_scan_body<PintraSpeller>(A); }
extern "C" __global__ __launch_bounds__(64) void mobi_encpi_write(MobiEncInterArgs A) { mobi_enc_write_body<PintraSpeller>(A); }

// the mode's stages behind search and code (mobi_launch_encode_inter): bit 4 = decide, bit 5 = finish, bit 2 = scan, bit 3 = write
extern "C" int mobi_launch_encode_pintra(const MobiEncInterArgs *a, int stages, hipStream_t s) {
  const int nmb = a->mbw * a->mbh;
  if (stages & 16)
    for (int d = 0; d < a->mbw + a->mbh - 1; d++) {
      int x_lo, count;
      mobi_enc_diag_range(a->mbw, a->mbh, d, &x_lo, &count);
      hipLaunchKernelGGL(mobi_encpi_decide, dim3((count + WAVES - 1) / WAVES, a->n), dim3(WAVES * 64), 0, s, *a, d);
    }
  if (stages & 32) hipLaunchKernelGGL(mobi_encpi_finish, dim3((nmb + FINISH_THREADS - 1) / FINISH_THREADS, a->n), dim3(FINISH_THREADS), 0, s, *a);
  if (stages & 4) hipLaunchKernelGGL(mobi_encpi_scan, dim3(a->n), dim3(256), 0, s, *a);
  if (stages & 8) hipLaunchKernelGGL(mobi_encpi_write, dim3((nmb + 63) / 64, a->n), dim3(64), 0, s, *a);
  return (int)hipGetLastError();
}
