// mobi_txcode_lanes.h -- the lane-per-row block coder of the encoder kernels, written once (device only): mobi_txcode8 / mobi_txcode4
// (mobi_txcode.hip), the intra encoder's stage 1 (mobi_encode.hip) and mobi_fwd_dct8 / mobi_fwd_dct4 (mobi_analysis.hip) call these steps;
// the arithmetic is mobi_txcode.h's.
//
// One lane = one row of one N x N block (N = 8 or 4): the N lanes of a block are an aligned group of N lanes of a wave, r = the lane's
// row.  A block has a tile (int [N][N + 1], the transposes) and, for mobi_lanes_code, its levels in natural order (int16_t [N * N]) in LDS.
//   mobi_lanes_forward   residual row x 64, rows, the tile, columns: the lane ends up with natural coefficients r * N .. r * N + N - 1
//   mobi_lanes_code      one quantiser: quantise, levels to LDS in natural order, first inverse pass into the tile (transposed)
//                        -- sync --
//                        N consecutive SCAN positions (the lane's part of the reference's EncodeDct) and column r of the tile; the
//                        block's nonzero mask (OR over its lanes) gives every level its run and whether it is the last one: bit cost
//                        from the LDS copy of the [2][64][44] cost table, no serial walk; second inverse pass = pixel row r, through the
//                        clamp, SAD against the source row; SAD, bits and clamp faults summed over the block in one packed word
//
// Synchronisation is the caller's: `sync` is MobiSyncWorkgroup where the lanes of a block may sit in a workgroup whose other waves share
// the arrays' declaration (the txcode and forward-DCT kernels: __syncthreads()), MobiSyncWave where a wave owns its arrays (the intra
// encoder).  Both steps CONTAIN sync points: with MobiSyncWorkgroup every lane of the workgroup must call them, whatever it has to do
// (lanes without a block pass zeros and are masked at the caller's stores); with MobiSyncWave every lane of the wave must, so that the
// shuffles stay convergent.  mobi_lanes_forward syncs once (between rows and columns); mobi_lanes_code twice (on entry: the tile's and
// the levels' last readers are done; after its LDS writes).
#ifndef MOBI_TXCODE_LANES_H
#define MOBI_TXCODE_LANES_H
#include <hip/hip_runtime.h>

#include "mobi_txcode.h"

struct MobiSyncWorkgroup {
  __device__ __forceinline__ void operator()() const { __syncthreads(); }
};
// the lanes of one wave exchange data through LDS: LDS operations of a wave complete in order, the fences keep the compiler from moving them
struct MobiSyncWave {
  __device__ __forceinline__ void operator()() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
};

// a row of a block in memory: N bytes of pixels, N int16 levels
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
  __device__ static void idct(const int (&x)[8], int (&o)[8]) { mobi_bfly8(x, o); }
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
  __device__ static void idct(const int (&x)[4], int (&o)[4]) { mobi_bfly4(x, o); }
};

// sum / OR over the N lanes of one block
template <int N> __device__ __forceinline__ uint32_t mobi_lanes_sum(uint32_t v) {
#pragma unroll
  for (int m = 1; m < N; m <<= 1) v += (uint32_t)__shfl_xor((int)v, m, N);
  return v;
}
template <int N> __device__ __forceinline__ uint32_t mobi_lanes_or(uint32_t v) {
#pragma unroll
  for (int m = 1; m < N; m <<= 1) v |= (uint32_t)__shfl_xor((int)v, m, N);
  return v;
}

// the cost table into LDS by the workgroup's THREADS threads; the caller synchronises them before the first mobi_lanes_code
template <int THREADS> __device__ __forceinline__ const uint8_t *mobi_lanes_stage_lut(const MobiTcConst *K, uint32_t (&lut32)[MOBI_TC_LUT_BYTES / 4]) {
  for (int i = threadIdx.x; i < MOBI_TC_LUT_BYTES / 4; i += THREADS) lut32[i] = ((const uint32_t *)K->lut)[i];
  return (const uint8_t *)lut32;
}
// the natural index of each of the lane's scan positions r * N + j
template <int N> __device__ __forceinline__ void mobi_lanes_scan(const MobiTcConst *K, int r, int (&zi)[N]) {
  const uint8_t *zz = N == 8 ? K->zz8 : K->zz4;
#pragma unroll
  for (int j = 0; j < N; j++) zi[j] = zz[r * N + j];
}

// ---- forward step (mobi_forward_dct's: residual x 64, rows, columns): res = the lane's row of the residual, d = its natural coefficients ----
template <int N, class Sync> __device__ __forceinline__ void mobi_lanes_forward(const int (&res)[N], int r, int (&tile)[N][N + 1], Sync sync, int (&d)[N]) {
  int x[N], o[N];
#pragma unroll
  for (int k = 0; k < N; k++) x[k] = res[k] * 64;
  Row<N>::dct(x, o);
#pragma unroll
  for (int k = 0; k < N; k++) tile[r][k] = o[k];
  sync();
#pragma unroll
  for (int j = 0; j < N; j++) x[j] = tile[j][r];
  Row<N>::dct(x, d);
}

// what a lane holds of its block after one quantiser
template <int N> struct MobiLaneCoded {
  int lv[N];         // the levels at scan positions r * N + j
  int px[N];         // pixel row r of the reconstruction
  uint64_t mask;     // the block's: bit k = scan position k is nonzero
  uint32_t sum;      // the block's: SAD of the reconstruction | bits << 14 | lanes with a clamp fault << 25
  uint32_t sad_pred; // the lane's: SAD of the prediction's row
  uint32_t range;    // the lane's: some |level| of natural row r is above MOBI_TC_MAX_LEVEL
  __device__ __forceinline__ uint32_t sad() const { return sum & 0x3FFF; }
  __device__ __forceinline__ uint32_t bits() const { return (sum >> 14) & 0x7FF; }
  __device__ __forceinline__ bool clamp() const { return (sum >> 25) != 0; }
};

// ---- per-quantiser step: s / p = the lane's row of the source and the prediction, d = mobi_lanes_forward's, zi = mobi_lanes_scan's,
// lut = the staged cost table; tile and nat are the block's ----
template <int N, class Sync>
__device__ __forceinline__ void mobi_lanes_code(const MobiTcConst *K, const uint8_t *lut, int q, int r, const int (&zi)[N], const int (&s)[N], const int (&p)[N],
                                                const int (&d)[N], int (&tile)[N][N + 1], int16_t (&nat)[N * N], Sync sync, MobiLaneCoded<N> &c) {
  using R = Row<N>;
  const int32_t *Qrow = (N == 8 ? K->q8[q] : K->q4[q]) + r * N;
  const float *RQrow = (N == 8 ? K->rq8[q] : K->rq4[q]) + r * N;
  int x[N], o[N];
  sync(); // the last reads of nat and tile are done
  c.range = 0;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const int Q = Qrow[k], lev = mobi_tc_quant(d[k], Q, RQrow[k]);
    nat[r * N + k] = (int16_t)lev;
    c.range |= (uint32_t)(lev > MOBI_TC_MAX_LEVEL || lev < -MOBI_TC_MAX_LEVEL);
    x[k] = lev * Q;              // dequantised (RealDCT)
  }
  if (r == 0) x[0] += 0x20;      // the rounding term rides on the DC coefficient through both passes
  R::idct(x, o);
#pragma unroll
  for (int k = 0; k < N; k++) tile[k][r] = o[k]; // stored transposed
  sync();

  // ---- levels in scan order, run / last from the block's nonzero mask, bit cost ----
  uint32_t nzl = 0; // bit j: scan position r * N + j is nonzero
#pragma unroll
  for (int j = 0; j < N; j++) {
    c.lv[j] = nat[zi[j]];
    nzl |= (uint32_t)(c.lv[j] != 0) << j;
  }
  uint32_t bits = 0;
  if (N == 8) {
    const uint32_t lo = mobi_lanes_or<N>(r < 4 ? nzl << (8 * r) : 0u), hi = mobi_lanes_or<N>(r >= 4 ? nzl << (8 * (r - 4)) : 0u);
    c.mask = (uint64_t)hi << 32 | lo;
  } else {
    c.mask = mobi_lanes_or<N>(nzl << (4 * r));
  }
  if (c.mask) {
    const int last = 63 - __builtin_clzll(c.mask);
#pragma unroll
    for (int j = 0; j < N; j++) {
      const int k = r * N + j;
      const uint64_t below = c.mask & ((1ull << k) - 1ull);
      const int prev = below ? 63 - __builtin_clzll(below) : -1;
      const int v = c.lv[j] < 0 ? -c.lv[j] : c.lv[j];
      const int cost = v < MOBI_TC_LUT_V ? (int)lut[mobi_tc_lut_index(v, k - prev - 1, k == last)] : MOBI_TC_ESCAPE_BITS;
      bits += c.lv[j] ? (uint32_t)cost : 0u;
    }
  }

  // ---- reconstruction: second inverse pass of pixel row r, the clamp table (a fault is where the reference throws), both SADs ----
#pragma unroll
  for (int j = 0; j < N; j++) x[j] = tile[r][j];
  R::idct(x, o);
  uint32_t sad = 0;
  int fault = 0;
  c.sad_pred = 0;
#pragma unroll
  for (int k = 0; k < N; k++) {
    c.px[k] = mobi_add_clamp(p[k], o[k] >> 6, &fault);
    sad += (uint32_t)__builtin_abs(s[k] - c.px[k]);
    c.sad_pred += (uint32_t)__builtin_abs(s[k] - p[k]);
  }
  // sad <= 64 * 255 < 2^14, bits <= 64 * 28 < 2^11, faulting lanes <= 8 < 2^7
  c.sum = mobi_lanes_sum<N>(sad | bits << 14 | (uint32_t)fault << 25);
}

#endif
