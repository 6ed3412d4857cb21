// mobi_txcode.hip -- the encoder's transform coding of residual blocks on gfx950 (the DCT / quant half):
// MacroBlock.EncodeDecode8x8Block / EncodeDecode4x4Block (Encoder/MacroBlock.cs:577-597, 605-626) plus the SAD the analyzer scores
// with (Analyzer.GetScore8x8 / 4x4, Analyzer.cs:1201, 1269), for n_blocks blocks at n_q quantisers (include/mobiclip_hip.h,
// mobi_transform_code; the arithmetic is mobi_txcode.h).
//
// One lane = one row of one block: N lanes per block (N = 8 or 4), 256 / N blocks per workgroup.  The forward transform runs once per
// block (rows, transpose through LDS, columns: lane r then holds coefficients r * N .. r * N + N - 1); then for every quantiser:
//   quantise the lane's N coefficients, store them to LDS in natural order, and the first inverse pass of the dequantised row to a tile
//   -- barrier --
//   read N consecutive SCAN positions (the lane's part of the reference's EncodeDct) and column r of the tile;
//   the block's nonzero mask (OR over its N lanes) gives every level its run and whether it is the last one: bit cost from the LDS copy
//   of the [2][64][44] cost table, no serial walk;
//   second inverse pass = pixel row r, through the clamp, SAD against the source row;
//   bits, SAD and the clamp count summed over the block's lanes in one packed word; coalesced stores of levels and pixel rows.
#include <hip/hip_runtime.h>

#include "mobi_txcode.h"

namespace {

template <int N> struct Row;
template <> struct Row<8> {
  using Pix = uint2;  // 8 bytes
  using Lev = int4;   // 8 int16
  __device__ static void unpack(Pix v, int (&x)[8]) {
#pragma unroll
    for (int k = 0; k < 4; k++) { x[k] = (v.x >> (8 * k)) & 0xFF; x[k + 4] = (v.y >> (8 * k)) & 0xFF; }
  }
  __device__ static Pix pack(const int (&x)[8]) {
    return Pix{(uint32_t)x[0] | (uint32_t)x[1] << 8 | (uint32_t)x[2] << 16 | (uint32_t)x[3] << 24,
               (uint32_t)x[4] | (uint32_t)x[5] << 8 | (uint32_t)x[6] << 16 | (uint32_t)x[7] << 24};
  }
  __device__ static Lev pack_lev(const int (&x)[8]) {
    return Lev{(int)((x[0] & 0xFFFF) | (uint32_t)x[1] << 16), (int)((x[2] & 0xFFFF) | (uint32_t)x[3] << 16),
               (int)((x[4] & 0xFFFF) | (uint32_t)x[5] << 16), (int)((x[6] & 0xFFFF) | (uint32_t)x[7] << 16)};
  }
  __device__ static void dct(const int (&x)[8], int (&o)[8]) { mobi_dct8_pass(x, o); }
  __device__ static void idct(const int (&x)[8], int (&o)[8]) { mobi_idct8_pass(x, o); }
};
template <> struct Row<4> {
  using Pix = uint32_t;
  using Lev = int2;
  __device__ static void unpack(Pix v, int (&x)[4]) {
#pragma unroll
    for (int k = 0; k < 4; k++) x[k] = (v >> (8 * k)) & 0xFF;
  }
  __device__ static Pix pack(const int (&x)[4]) { return (uint32_t)x[0] | (uint32_t)x[1] << 8 | (uint32_t)x[2] << 16 | (uint32_t)x[3] << 24; }
  __device__ static Lev pack_lev(const int (&x)[4]) {
    return Lev{(int)((x[0] & 0xFFFF) | (uint32_t)x[1] << 16), (int)((x[2] & 0xFFFF) | (uint32_t)x[3] << 16)};
  }
  __device__ static void dct(const int (&x)[4], int (&o)[4]) { mobi_dct4_pass(x, o); }
  __device__ static void idct(const int (&x)[4], int (&o)[4]) { mobi_idct4_pass(x, o); }
};

// sum over the N lanes of one block (aligned groups of N lanes of the wave)
template <int N> __device__ __forceinline__ uint32_t block_sum(uint32_t v) {
#pragma unroll
  for (int m = 1; m < N; m <<= 1) v += (uint32_t)__shfl_xor((int)v, m, N);
  return v;
}
template <int N> __device__ __forceinline__ uint32_t block_or(uint32_t v) {
#pragma unroll
  for (int m = 1; m < N; m <<= 1) v |= (uint32_t)__shfl_xor((int)v, m, N);
  return v;
}

} // namespace

template <int N> __device__ __forceinline__ void txcode(const MobiTcArgs &A) {
  constexpr int NN = N * N, BPW = 256 / N;
  using R = Row<N>;
  __shared__ uint32_t lut32[MOBI_TC_LUT_BYTES / 4];
  __shared__ int tile[BPW][N][N + 1];  // transposes; pitch N + 1: a column read of the N lanes hits N banks
  __shared__ int16_t lev_s[BPW][NN];   // the block's levels in natural order
  const MobiTcConst *K = A.k;
  for (int i = threadIdx.x; i < MOBI_TC_LUT_BYTES / 4; i += 256) lut32[i] = ((const uint32_t *)K->lut)[i];
  const uint8_t *lut = (const uint8_t *)lut32;

  const int lb = threadIdx.x / N, r = threadIdx.x % N;
  const uint32_t blk = blockIdx.x * (uint32_t)BPW + (uint32_t)lb;
  const bool on = blk < A.n_blocks;
  const size_t row = (size_t)blk * NN + (size_t)r * N; // this lane's row of src / pred, and of every entry's levels / recon
  int s[N], p[N], x[N], o[N], d[N];
  if (on) {
    R::unpack(*(const typename R::Pix *)(A.src + row), s);
    R::unpack(*(const typename R::Pix *)(A.pred + row), p);
  } else {
#pragma unroll
    for (int k = 0; k < N; k++) s[k] = p[k] = 0;
  }
  // forward transform (mobi_forward_dct's: residual x 64, rows, columns)
#pragma unroll
  for (int k = 0; k < N; k++) x[k] = (s[k] - p[k]) * 64;
  R::dct(x, o);
#pragma unroll
  for (int k = 0; k < N; k++) tile[lb][r][k] = o[k];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; j++) x[j] = tile[lb][j][r];
  R::dct(x, d); // natural coefficients r * N + k
  // the natural index of each of this lane's scan positions r * N + j
  const uint8_t *zz = N == 8 ? K->zz8 : K->zz4;
  int zi[N];
#pragma unroll
  for (int j = 0; j < N; j++) zi[j] = zz[r * N + j];

  for (int qi = 0; qi < A.n_q; qi++) {
    const int q = A.q[qi];
    const int32_t *Qrow = (N == 8 ? K->q8[q] : K->q4[q]) + r * N;
    const float *RQrow = (N == 8 ? K->rq8[q] : K->rq4[q]) + r * N;
    __syncthreads(); // the previous quantiser's reads of lev_s and tile are done
#pragma unroll
    for (int k = 0; k < N; k++) {
      const int Q = Qrow[k], lev = mobi_tc_quant(d[k], Q, RQrow[k]);
      lev_s[lb][r * N + k] = (int16_t)lev;
      x[k] = lev * Q;              // dequantised (RealDCT)
    }
    if (r == 0) x[0] += 0x20;      // the rounding term rides on the DC coefficient through both passes
    R::idct(x, o);
#pragma unroll
    for (int k = 0; k < N; k++) tile[lb][k][r] = o[k]; // stored transposed
    __syncthreads();

    // ---- levels in scan order, run / last from the block's nonzero mask, bit cost ----
    int lv[N];
    uint32_t nzl = 0; // bit j: scan position r * N + j is nonzero
#pragma unroll
    for (int j = 0; j < N; j++) {
      lv[j] = lev_s[lb][zi[j]];
      nzl |= (uint32_t)(lv[j] != 0) << j;
    }
    uint32_t bits = 0;
    uint64_t mask; // bit k: scan position k nonzero
    if (N == 8) {
      const uint32_t lo = block_or<N>(r < 4 ? nzl << (8 * r) : 0u), hi = block_or<N>(r >= 4 ? nzl << (8 * (r - 4)) : 0u);
      mask = (uint64_t)hi << 32 | lo;
    } else {
      mask = block_or<N>(nzl << (4 * r));
    }
    if (mask) {
      const int last = 63 - __builtin_clzll(mask);
#pragma unroll
      for (int j = 0; j < N; j++) {
        const int k = r * N + j;
        const uint64_t below = mask & ((1ull << k) - 1ull);
        const int prev = below ? 63 - __builtin_clzll(below) : -1;
        const int v = lv[j] < 0 ? -lv[j] : lv[j];
        const int c = v < MOBI_TC_LUT_V ? (int)lut[mobi_tc_lut_index(v, k - prev - 1, k == last)] : MOBI_TC_ESCAPE_BITS;
        bits += lv[j] ? (uint32_t)c : 0u;
      }
    }

    // ---- reconstruction: second inverse pass of pixel row r, the clamp table, SAD ----
#pragma unroll
    for (int j = 0; j < N; j++) x[j] = tile[lb][r][j];
    R::idct(x, o);
    uint32_t sad = 0, bad = 0;
    int px[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
      const int t = 0x40 + p[k] + (o[k] >> 6);                        // index into mobi_vx2minmaxtable[384]
      bad += (uint32_t)t >= 384u;                                      // where the reference throws IndexOutOfRangeException
      px[k] = t < 0x40 ? 0 : t > 0x40 + 255 ? 255 : t - 0x40;        // the table's content on [0, 384)
      sad += (uint32_t)__builtin_abs(s[k] - px[k]);
    }
    // sad <= 64 * 255 < 2^14, bits <= 64 * 28 < 2^11, clamp faults <= 64 < 2^7
    const uint32_t sum = block_sum<N>(sad | bits << 14 | bad << 25);

    if (on) {
      const size_t e = (size_t)qi * A.n_blocks + blk;
      const size_t at = e * NN + (size_t)r * N;
      if (A.levels) *(typename R::Lev *)(A.levels + at) = R::pack_lev(lv);
      if (A.recon) *(typename R::Pix *)(A.recon + at) = R::pack(px);
      if (r == 0) {
        A.bits[e] = (int32_t)((sum >> 14) & 0x7FF);
        if (A.sad) A.sad[e] = (int32_t)(sum & 0x3FFF);
        A.flags[e] = (uint8_t)((mask != 0) | ((sum >> 25) != 0) << 1);
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
