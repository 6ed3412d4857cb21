// mobi_encode_trials.h -- DEVICE ONLY: the six intra trials of one macroblock by one wave, written once.  mobi_encode.hip runs them for
// every macroblock of an I-frame (stage 1 there), mobi_encode_pintra.hip for the macroblocks of a P-frame that may be sent intra.
//
// The wave's 64 lanes are eight groups of eight: groups 0..2 try the luma modes 0, 1, 3 side by side, groups 3..5 the chroma modes, groups
// 6 and 7 ride along.  A group runs its trial's blocks in sequence (four luma blocks; U, then V), one lane = one row of the block: the
// block coder of mobi_txcode_lanes.h at wave scope.  Every trial keeps its own reconstruction in an LDS patch whose border row and column
// come from the picture's reconstruction (A.rec: whatever the macroblocks to the left and above left there), so a block predicts from the
// earlier blocks of the same trial.  mobi_enc_trials ends with the argmin of each half in every lane; mobi_enc_trials_store puts the two
// winners' patches and levels to memory.  The caller keeps the order between a macroblock and its left and upper neighbours.
#ifndef MOBI_ENCODE_TRIALS_H
#define MOBI_ENCODE_TRIALS_H
#include <hip/hip_runtime.h>

#include "mobi_encode.h"
#include "mobi_txcode_lanes.h"

constexpr int MOBI_ENC_TRIAL_WAVES = 4; // per workgroup of the kernels that run the trials

struct MobiEncTrialLds {
  uint8_t patch[6][18][20]; // luma: [1 + y][1 + x] of the 16x16, row 0 / column 0 = the border; chroma: U rows 0..8, V rows 9..17
  int tile[8][8][9];        // transposes (pitch 9: a column read of eight lanes hits eight banks)
  int16_t nat[8][64];       // a block's levels in natural order
  int16_t lev[6][4][64];    // every trial's levels in scan order
};

// the winners, the same in every lane: gl / gc the winning groups (0..2, 3..5), Jl / Jc their costs, and per half the coded mask and the
// sums of bits, sad and fallbacks over the winner's blocks
struct MobiEncTrialResult {
  int gl, gc;
  int64_t Jl, Jc;
  uint32_t cl, cc, bl, bc, sl, sc, kl, kc, rl, rc;
  __device__ uint32_t cbp() const { return cl | cc << 4; }
};

__device__ __forceinline__ int64_t mobi_enc_shfl64(int64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), src);
  return (int64_t)((uint64_t)hi << 32 | lo);
}

__device__ __forceinline__ void mobi_enc_trials(const MobiEncArgs &A, int pic, int mbx, int mby, MobiEncTrialLds &L, const uint8_t *lut, MobiEncTrialResult &R) {
  const MobiEncConst *K = A.k;
  const MobiSyncWave wave_sync; // a wave owns its LDS: no workgroup barrier inside a macroblock
  const int lane = threadIdx.x & 63, g = lane >> 3, r = lane & 7;
  const bool chroma = g >= 3 && g < 6;
  const int gp = g < 6 ? g : 0;                   // the patch a group works in (6 and 7 shadow group 0 and keep nothing)
  const int mode = mobi_enc_mode(g % 3);
  const int W = A.W, q = A.q[pic];
  const size_t ysz = (size_t)W * A.H, frame = ysz + ysz / 2;
  const uint8_t *src = A.src + (size_t)pic * A.src_pitch;
  const uint8_t *rec = A.rec + (size_t)pic * frame;
  const int64_t lam = mobi_enc_lambda(q);
  int zi[8];
  mobi_lanes_scan<8>(K, r, zi);

  // the luma border: 16 samples above, 16 to the left (read only where they exist)
  if (!chroma) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int i = r + 8 * h;
      L.patch[gp][0][1 + i] = mby > 0 ? rec[(size_t)(mby * 16 - 1) * W + mbx * 16 + i] : 0;
      L.patch[gp][1 + i][0] = mbx > 0 ? rec[(size_t)(mby * 16 + i) * W + mbx * 16 - 1] : 0;
    }
  }
  int64_t J = 0;
  uint32_t coded_m = 0, bits_t = 0, sad_t = 0, clamp_t = 0, range_t = 0;
#pragma unroll 1
  for (int it = 0; it < 4; it++) {
    const bool live = g < 6 && (!chroma || it < 2);
    const int cp = it < 2 ? it : 1; // the chroma plane of this round
    const MobiEncBlockAt at = mobi_enc_block_at(chroma, chroma ? cp : it, mbx, mby, W);
    const int pitch = at.pitch, x0 = at.x0, y0 = at.y0;
    const size_t plane = at.plane ? ysz + (size_t)(at.plane - 1) * (ysz / 4) : 0;
    const int oy = chroma ? 1 + 9 * cp : 1 + 8 * (it >> 1), ox = chroma ? 1 : 1 + 8 * (it & 1);
    if (chroma && it < 2) { // this plane's border
      L.patch[gp][oy - 1][1 + r] = y0 > 0 ? rec[plane + (size_t)(y0 - 1) * pitch + x0 + r] : 0;
      L.patch[gp][oy + r][0] = x0 > 0 ? rec[plane + (size_t)(y0 + r) * pitch + x0 - 1] : 0;
    }
    wave_sync();
    int s[8], p[8], x[8], d[8];
    Row<8>::unpack(*(const uint2 *)(src + plane + (size_t)(y0 + r) * pitch + x0), s);
    // the decoder's predictor on the trial's own reconstruction
    auto nb = [&](int dy, int dx) -> int { return L.patch[gp][oy + dy][ox + dx]; };
    if (mode == 3) {
      const int dc = mobi_pred_px(3, 8, 0, 0, y0 != 0, x0 != 0, nb);
#pragma unroll
      for (int k = 0; k < 8; k++) p[k] = dc;
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) p[k] = mobi_pred_px(mode, 8, r, k, 1, 1, nb);
    }
    // the block coder's steps (mobi_txcode_lanes.h) at wave scope; every group runs them, the idle ones too: the shuffles stay convergent
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = s[k] - p[k];
    mobi_lanes_forward<8>(x, r, L.tile[g], wave_sync, d);
    MobiLaneCoded<8> c;
    mobi_lanes_code<8>(K, lut, q, r, zi, s, p, d, L.tile[g], L.nat[g], wave_sync, c);
    // the prediction's sad with the level-range flag above it
    const uint32_t sum2 = mobi_lanes_sum<8>(c.sad_pred | c.range << 14);
    const MobiEncBlock b = mobi_enc_block_result(c.mask != 0, c.clamp(), (sum2 >> 14) != 0, (int)c.bits(), (int)c.sad(), (int)(sum2 & 0x3FFF));
    if (live) {
      J += mobi_enc_cost(lam, b);
      coded_m |= (uint32_t)b.coded << it;
      bits_t += (uint32_t)b.bits;
      sad_t += (uint32_t)b.sad;
      clamp_t += b.clamp;
      range_t += b.range;
#pragma unroll
      for (int k = 0; k < 8; k++) L.patch[g][oy + r][ox + k] = (uint8_t)(b.coded ? c.px[k] : p[k]);
#pragma unroll
      for (int j = 0; j < 8; j++) L.lev[g][it][r * 8 + j] = (int16_t)(b.coded ? c.lv[j] : 0);
    }
  }
  wave_sync();

  // ---- the argmin of each half: candidates in mode order, a tie keeps the smaller mode ----
  int gl = -1, gc = -1;
  int64_t Jl = 0, Jc = 0;
#pragma unroll
  for (int c = 0; c < MOBI_ENC_NMODES; c++) {
    const int64_t a = mobi_enc_shfl64(J, c * 8), b = mobi_enc_shfl64(J, (3 + c) * 8);
    if (!mobi_enc_mode_allowed(mobi_enc_mode(c), mbx, mby)) continue;
    if (gl < 0 || a < Jl) { gl = c; Jl = a; }
    if (gc < 0 || b < Jc) { gc = 3 + c; Jc = b; }
  }
  R.gl = gl; R.gc = gc; R.Jl = Jl; R.Jc = Jc;
  R.cl = (uint32_t)__shfl((int)coded_m, gl * 8); R.cc = (uint32_t)__shfl((int)coded_m, gc * 8);
  R.bl = (uint32_t)__shfl((int)bits_t, gl * 8); R.bc = (uint32_t)__shfl((int)bits_t, gc * 8);
  R.sl = (uint32_t)__shfl((int)sad_t, gl * 8); R.sc = (uint32_t)__shfl((int)sad_t, gc * 8);
  R.kl = (uint32_t)__shfl((int)clamp_t, gl * 8); R.kc = (uint32_t)__shfl((int)clamp_t, gc * 8);
  R.rl = (uint32_t)__shfl((int)range_t, gl * 8); R.rc = (uint32_t)__shfl((int)range_t, gc * 8);
}

// the winners' reconstruction (64 words of luma, 32 of chroma) into the picture, their levels (6 x 64 = 192 words) into the record
__device__ __forceinline__ void mobi_enc_trials_store(const MobiEncArgs &A, int pic, int mbx, int mby, const MobiEncTrialLds &L, const MobiEncTrialResult &R, MobiEncMb *mb) {
  const int lane = threadIdx.x & 63, W = A.W;
  const size_t ysz = (size_t)W * A.H, frame = ysz + ysz / 2;
  uint8_t *rec = A.rec + (size_t)pic * frame;
  {
    const int row = lane >> 2, cw = lane & 3;
    const uint8_t *s4 = &L.patch[R.gl][1 + row][1 + 4 * cw];
    *(uint32_t *)(rec + (size_t)(mby * 16 + row) * W + mbx * 16 + 4 * cw) = (uint32_t)s4[0] | (uint32_t)s4[1] << 8 | (uint32_t)s4[2] << 16 | (uint32_t)s4[3] << 24;
    if (lane < 32) {
      const int cp = lane >> 4, crow = (lane & 15) >> 1, ccw = lane & 1;
      const uint8_t *c4 = &L.patch[R.gc][1 + 9 * cp + crow][1 + 4 * ccw];
      *(uint32_t *)(rec + ysz + (size_t)cp * (ysz / 4) + (size_t)(mby * 8 + crow) * (W / 2) + mbx * 8 + 4 * ccw) =
          (uint32_t)c4[0] | (uint32_t)c4[1] << 8 | (uint32_t)c4[2] << 16 | (uint32_t)c4[3] << 24;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int w = lane + 64 * i, a = w >> 5, idx = w & 31;
    ((uint32_t *)mb->lev[a])[idx] = ((const uint32_t *)L.lev[a < 4 ? R.gl : R.gc][a < 4 ? a : a - 4])[idx];
  }
}

// the cost table in LDS, staged by the whole workgroup
__device__ __forceinline__ const uint8_t *mobi_enc_trials_stage_lut(const MobiEncArgs &A, uint32_t (&lut32)[MOBI_TC_LUT_BYTES / 4]) {
  const uint8_t *lut = mobi_lanes_stage_lut<MOBI_ENC_TRIAL_WAVES * 64>(A.k, lut32);
  __syncthreads();
  return lut;
}
#endif
