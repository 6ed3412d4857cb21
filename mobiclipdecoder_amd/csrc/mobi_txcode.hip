// mobi_txcode.hip -- the encoder's transform coding of residual blocks on gfx950 (the DCT / quant half):
// MacroBlock.EncodeDecode8x8Block / EncodeDecode4x4Block (Encoder/MacroBlock.cs:577-597, 605-626) plus the SAD the analyzer scores
// with (Analyzer.GetScore8x8 / 4x4, Analyzer.cs:1201, 1269), for n_blocks blocks at n_q quantisers (include/mobiclip_hip.h,
// mobi_transform_code; the arithmetic is mobi_txcode.h).
//
// One lane = one row of one block: N lanes per block (N = 8 or 4), 256 / N blocks per workgroup.  The forward transform runs once per
// block, then the per-quantiser step for every quantiser: both are mobi_txcode_lanes.h's, with workgroup barriers.  This file holds the
// loads, the quantiser loop and the coalesced stores of levels, pixel rows and the block's figures.
#include <hip/hip_runtime.h>

#include "mobi_txcode_lanes.h"

template <int N> __device__ __forceinline__ void txcode(const MobiTcArgs &A) {
  constexpr int NN = N * N, BPW = 256 / N;
  using R = Row<N>;
  __shared__ uint32_t lut32[MOBI_TC_LUT_BYTES / 4];
  __shared__ int tile[BPW][N][N + 1];  // transposes; pitch N + 1: a column read of the N lanes hits N banks
  __shared__ int16_t lev_s[BPW][NN];   // the block's levels in natural order
  const MobiSyncWorkgroup sync;        // a block's lanes share a wave, but the staged table and the arrays are the workgroup's
  const uint8_t *lut = mobi_lanes_stage_lut<256>(A.k, lut32); // (the forward step's barrier comes before the first lookup)

  const int lb = threadIdx.x / N, r = threadIdx.x % N;
  const uint32_t blk = blockIdx.x * (uint32_t)BPW + (uint32_t)lb;
  const bool on = blk < A.n_blocks;
  const size_t row = (size_t)blk * NN + (size_t)r * N; // this lane's row of src / pred, and of every entry's levels / recon
  // lanes past n_blocks code a block of zeros and store nothing: the steps below contain barriers, every lane runs them
  int s[N], p[N], x[N], d[N], zi[N];
  if (on) {
    R::unpack(*(const typename R::Pix *)(A.src + row), s);
    R::unpack(*(const typename R::Pix *)(A.pred + row), p);
  } else {
#pragma unroll
    for (int k = 0; k < N; k++) s[k] = p[k] = 0;
  }
#pragma unroll
  for (int k = 0; k < N; k++) x[k] = s[k] - p[k];
  mobi_lanes_forward<N>(x, r, tile[lb], sync, d);
  mobi_lanes_scan<N>(A.k, r, zi);

  for (int qi = 0; qi < A.n_q; qi++) {
    MobiLaneCoded<N> c; // (its level-range flag and the prediction's SAD are the intra encoder's: unused here, they leave no code)
    mobi_lanes_code<N>(A.k, lut, A.q[qi], r, zi, s, p, d, tile[lb], lev_s[lb], sync, c);
    if (on) {
      const size_t e = (size_t)qi * A.n_blocks + blk;
      const size_t at = e * NN + (size_t)r * N;
      if (A.levels) *(typename R::Lev *)(A.levels + at) = R::pack_lev(c.lv);
      if (A.recon) *(typename R::Pix *)(A.recon + at) = R::pack(c.px);
      if (r == 0) {
        A.bits[e] = (int32_t)c.bits();
        if (A.sad) A.sad[e] = (int32_t)c.sad();
        A.flags[e] = (uint8_t)((c.mask != 0) | c.clamp() << 1);
      }
    }
  }
}

extern "C" __global__ __launch_bounds__(256) void mobi_txcode8(MobiTcArgs A) { txcode<8>(A); }
extern "C" __global__ __launch_bounds__(256) void mobi_txcode4(MobiTcArgs A) { txcode<4>(A); }

extern "C" int mobi_launch_txcode(int n, const MobiTcArgs *a, hipStream_t s) {
  if (a->n_blocks == 0) return 0;
  if (n == 8) hipLaunchKernelGGL(mobi_txcode8, dim3((a->n_blocks + 31) / 32), dim3(256), 0, s, *a);
  else if (n == 4) hipLaunchKernelGGL(mobi_txcode4, dim3((a->n_blocks + 63) / 64), dim3(256), 0, s, *a);
  else return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}
