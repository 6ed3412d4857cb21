// mobi_encode.hip -- the intra encoder on gfx950 (include/mobiclip_encode.h; the rules are mobi_encode.h's, DESIGN.md "Intra encoder").
//
// Stage 1, decide and reconstruct.  One wave = one macroblock.  Its 64 lanes are eight groups of eight: groups 0..2 try the luma modes
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
#include "mobi_encode_write.h"
#include "mobi_txcode_lanes.h"

namespace {

constexpr int WAVES = 4; // per workgroup, both stage-1 shapes

struct WaveLds {
  uint8_t patch[6][18][20]; // luma: [1 + y][1 + x] of the 16x16, row 0 / column 0 = the border; chroma: U rows 0..8, V rows 9..17
  int tile[8][8][9];        // transposes (pitch 9: a column read of eight lanes hits eight banks)
  int16_t nat[8][64];       // a block's levels in natural order
  int16_t lev[6][4][64];    // every trial's levels in scan order
};

__device__ __forceinline__ int64_t shfl64(int64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), src);
  return (int64_t)((uint64_t)hi << 32 | lo);
}

__device__ __forceinline__ void encode_mb(const MobiEncArgs &A, int pic, int mbx, int mby, WaveLds &L, const uint8_t *lut) {
  const MobiEncConst *K = A.k;
  const MobiSyncWave wave_sync; // a wave owns its WaveLds: no workgroup barrier inside a macroblock
  const int lane = threadIdx.x & 63, g = lane >> 3, r = lane & 7;
  const bool chroma = g >= 3 && g < 6;
  const int gp = g < 6 ? g : 0;                   // the patch a group works in (6 and 7 shadow group 0 and keep nothing)
  const int mode = mobi_enc_mode(g % 3);
  const int W = A.W, q = A.q[pic];
  const size_t ysz = (size_t)W * A.H, frame = ysz + ysz / 2;
  const uint8_t *src = A.src + (size_t)pic * A.src_pitch;
  uint8_t *rec = A.rec + (size_t)pic * frame;
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
    const int64_t a = shfl64(J, c * 8), b = shfl64(J, (3 + c) * 8);
    if (!mobi_enc_mode_allowed(mobi_enc_mode(c), mbx, mby)) continue;
    if (gl < 0 || a < Jl) { gl = c; Jl = a; }
    if (gc < 0 || b < Jc) { gc = 3 + c; Jc = b; }
  }
  // the winners' reconstruction: 64 words of luma, 32 of chroma
  {
    const int row = lane >> 2, cw = lane & 3;
    const uint8_t *s4 = &L.patch[gl][1 + row][1 + 4 * cw];
    *(uint32_t *)(rec + (size_t)(mby * 16 + row) * W + mbx * 16 + 4 * cw) = (uint32_t)s4[0] | (uint32_t)s4[1] << 8 | (uint32_t)s4[2] << 16 | (uint32_t)s4[3] << 24;
    if (lane < 32) {
      const int cp = lane >> 4, crow = (lane & 15) >> 1, ccw = lane & 1;
      const uint8_t *c4 = &L.patch[gc][1 + 9 * cp + crow][1 + 4 * ccw];
      *(uint32_t *)(rec + ysz + (size_t)cp * (ysz / 4) + (size_t)(mby * 8 + crow) * (W / 2) + mbx * 8 + 4 * ccw) =
          (uint32_t)c4[0] | (uint32_t)c4[1] << 8 | (uint32_t)c4[2] << 16 | (uint32_t)c4[3] << 24;
    }
  }
  MobiEncMb *mb = A.mbs + (size_t)pic * ((size_t)A.mbw * A.mbh) + (size_t)mby * A.mbw + mbx;
#pragma unroll
  for (int i = 0; i < 3; i++) { // 6 x 64 levels = 192 words
    const int w = lane + 64 * i, a = w >> 5, idx = w & 31;
    ((uint32_t *)mb->lev[a])[idx] = ((const uint32_t *)L.lev[a < 4 ? gl : gc][a < 4 ? a : a - 4])[idx];
  }
  const uint32_t cl = (uint32_t)__shfl((int)coded_m, gl * 8), cc = (uint32_t)__shfl((int)coded_m, gc * 8);
  const uint32_t bl = (uint32_t)__shfl((int)bits_t, gl * 8), bc = (uint32_t)__shfl((int)bits_t, gc * 8);
  const uint32_t sl = (uint32_t)__shfl((int)sad_t, gl * 8), sc = (uint32_t)__shfl((int)sad_t, gc * 8);
  const uint32_t kl = (uint32_t)__shfl((int)clamp_t, gl * 8), kc = (uint32_t)__shfl((int)clamp_t, gc * 8);
  const uint32_t rl = (uint32_t)__shfl((int)range_t, gl * 8), rc = (uint32_t)__shfl((int)range_t, gc * 8);
  if (lane == 0) {
    const uint32_t cbp = cl | cc << 4;
    mb->bits = mobi_enc_mb_header_bits(K, cbp) + bl + bc;
    mb->luma_mode = (uint8_t)mobi_enc_mode(gl);
    mb->chroma_mode = (uint8_t)mobi_enc_mode(gc - 3);
    mb->cbp = (uint8_t)cbp;
    mb->pad = 0;
    if (A.stats) {
      mobi_enc_stats *st = A.stats + pic;
      atomicAdd((unsigned long long *)&st->sad, (unsigned long long)(sl + sc));
      atomicAdd(&st->luma_modes[mobi_enc_mode(gl)], 1u);
      atomicAdd(&st->chroma_modes[mobi_enc_mode(gc - 3)], 1u);
      if (__popc(cbp)) atomicAdd(&st->coded_blocks, (uint32_t)__popc(cbp));
      if (kl + kc) atomicAdd(&st->fallback_clamp, kl + kc);
      if (rl + rc) atomicAdd(&st->fallback_level, rl + rc);
    }
  }
  wave_sync(); // the patches and levels are read before the wave's next macroblock writes them
}

// the cost table in LDS, staged by the whole workgroup
__device__ __forceinline__ const uint8_t *stage_lut(const MobiEncArgs &A, uint32_t (&lut32)[MOBI_TC_LUT_BYTES / 4]) {
  const uint8_t *lut = mobi_lanes_stage_lut<WAVES * 64>(A.k, lut32);
  __syncthreads();
  return lut;
}

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
