// mobi_encode_parts.hip -- the inter encoder's partition mode on gfx950 (include/mobiclip_encode_parts.h; the rules are mobi_encode_parts.h's,
// DESIGN.md "Inter encoder", "Partitions").  The stages and the launch count are mobi_encode_inter.hip's: search, code, scan, write.
//
// Search (mobi_encq_search).  One wave = one macroblock, the window and the source staged in LDS as in mobi_encp_search.  Step 1: a lane
// walks its full-pel candidate's 16 rows once and keeps four sums, the left and right word pairs of rows 0..7 and 8..15: the quadrants'
// SADs; the halves' and the macroblock's are sums of them.  Nine keys per candidate, each gated by its leaf's own candidate set (three
// spans per axis: mobi_encq_span_ok), nine wave minima.  Step 2: the 9 x 8 half-pel neighbours in four passes of 64 lanes, each pass
// eight neighbours of the leaves of one shape: eight lanes a neighbour, a lane 2 rows x 16 or 4 rows x 8 samples of its leaf; the minimum
// runs over the lanes of a leaf only.  Every lane then holds the nine keys and decides the tree (mobi_encq_decide); lane 0 stores the tree
// (the record's luma_mode), the quadrants' vectors and the last leaf's vector.
//
// Code (mobi_encq_code).  mobi_encp_code with a vector per half row: a lane predicts the two 4-sample halves of its row, for a luma block
// both with the quadrant's vector, for a chroma block with the chroma vectors of the two quadrants its row crosses.  Lane 0 prices tree and
// leaves against the predictor and adds the statistics.
//
// Write.  mobi_encode_write.h's scan and writer with the partition speller.
#include <hip/hip_runtime.h>

#include "mobi_encode_parts.h"
#include "mobi_encode_write.h"
#include "mobi_txcode_lanes.h"

namespace {

constexpr int WAVES = 4;                                          // per workgroup of the code kernel
constexpr int WIN_BACK = MOBI_ENCP_REACH / 2 + 1;                 // 9: samples in front of the macroblock a vector can reach (-17 >> 1)
constexpr int WIN_LEFT = (WIN_BACK + 3) & ~3;                     // 12: the window starts on a word
constexpr int WIN_ROWS = WIN_BACK + 16 + MOBI_ENCP_REACH / 2 + 1; // 34
constexpr int WIN_DW = (WIN_LEFT + 16 + MOBI_ENCP_REACH / 2 + 1 + 3) / 4; // 10 words: columns -12 .. +27
constexpr int NFULL = MOBI_ENCP_RANGE + 1;
static_assert(WIN_ROWS == 34 && WIN_DW == 10 && WIN_LEFT == 12, "the window the index arithmetic below was checked for");

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  return (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m) << 32 | (uint32_t)__shfl_xor((int)(uint32_t)v, m);
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int lane) {
  return (uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), lane) << 32 | (uint32_t)__shfl((int)(uint32_t)v, lane);
}
// the minimum over the lanes that differ in the bits of masks FROM..32
template <int FROM> __device__ __forceinline__ uint64_t lanes_min64(uint64_t v) {
#pragma unroll
  for (int m = 32; m >= FROM; m >>= 1) {
    const uint64_t o = shfl_xor64(v, m);
    v = o < v ? o : v;
  }
  return v;
}
// the word at byte offset 4 * k + sh (sh in 0..4) of the row whose words are w[0..]
template <int N> __device__ __forceinline__ uint32_t row_word(const uint32_t (&w)[N], int k, int sh) {
  const bool carry = sh >> 2;
  return __builtin_amdgcn_alignbyte(carry ? w[k + 2] : w[k + 1], carry ? w[k + 1] : w[k], (uint32_t)(sh & 3));
}
// a half-pel candidate's SAD over NR rows from row0 and NW words from sample column col of the macroblock.  Every vector of at most
// MOBI_ENCP_REACH half-pels stays inside the window: bytes col + (dx >> 1) + 12 >= 3, words b .. b + NW <= 9 (col + 4 NW <= 16, dx >> 1 <= 8);
// rows row0 + (dy >> 1) + 9 >= 0, the row below the last <= 15 + 8 + 9 + 1 = 33.
template <int NW, int NR>
__device__ __forceinline__ uint32_t halfpel_sad(const uint32_t *win, const uint32_t *srcm, int col, int row0, int dx, int dy) {
  const int ox = col + (dx >> 1) + WIN_LEFT, oy = row0 + (dy >> 1) + WIN_BACK, phase = (dx & 1) | (dy & 1) << 1, b = ox >> 2, sh = ox & 3;
  uint32_t sad = 0;
#pragma unroll
  for (int h = 0; h < NR; h++) {
    const uint32_t *w0 = win + (oy + h) * WIN_DW + b, *w1 = w0 + WIN_DW;
    uint32_t wa[NW + 2], wc[NW + 2];
#pragma unroll
    for (int k = 0; k <= NW; k++) {
      wa[k] = w0[k];
      wc[k] = w1[k];
    }
    wa[NW + 1] = wc[NW + 1] = 0u; // only shifted out
#pragma unroll
    for (int k = 0; k < NW; k++) {
      const uint32_t p = mobi_mc4(row_word(wa, k, sh), row_word(wa, k, sh + 1), row_word(wc, k, sh), row_word(wc, k, sh + 1), phase);
      sad = __builtin_amdgcn_sad_u8(p, srcm[(row0 + h) * 4 + (col >> 2) + k], sad);
    }
  }
  return sad;
}
// neighbour idx (0..7, the centre left out) of a full-pel winner
__device__ __forceinline__ void neighbour(uint64_t best, int cand, int *dx, int *dy) {
  const int idx = cand < 4 ? cand : cand + 1;
  *dx = mobi_encp_key_dx(best) + idx % 3 - 1;
  *dy = mobi_encp_key_dy(best) + idx / 3 - 1;
}

} // namespace

extern "C" __global__ __launch_bounds__(64) void mobi_encq_search(MobiEncPartsArgs A) {
  __shared__ uint32_t win[WIN_ROWS * WIN_DW];
  __shared__ uint32_t srcm[16 * 4];
  const int lane = threadIdx.x, pic = blockIdx.y, mb = blockIdx.x;
  const int mby = mb / A.mbw, mbx = mb - mby * A.mbw, W = A.W, H = A.H, X0 = mbx * 16, Y0 = mby * 16;
  const uint8_t *src = A.src + (size_t)pic * A.src_pitch, *ref = A.ref + (size_t)pic * A.ref_pitch;
  const int64_t lam = mobi_enc_lambda(A.q[pic]);
  for (int idx = lane; idx < WIN_ROWS * WIN_DW; idx += 64) {
    const int r = idx / WIN_DW, dw = idx - r * WIN_DW, row = Y0 - WIN_BACK + r, col = X0 - WIN_LEFT + 4 * dw;
    // bytes outside the picture are zeros and never priced: mobi_encq_leaf_ok leaves those candidates without a key
    win[idx] = row >= 0 && row < H && col >= 0 && col < W ? *(const uint32_t *)(ref + (size_t)row * W + col) : 0u;
  }
  srcm[lane] = *(const uint32_t *)(src + (size_t)(Y0 + (lane >> 2)) * W + X0 + 4 * (lane & 3));
  __syncthreads(); // (one wave)

  // ---- step 1: full-pel candidates, one to a lane, four sums a walk ----
  uint64_t best[MOBI_ENCQ_LEAVES];
#pragma unroll
  for (int l = 0; l < MOBI_ENCQ_LEAVES; l++) best[l] = MOBI_ENCP_NO_KEY;
#pragma unroll 1
  for (int c0 = 0; c0 < NFULL * NFULL; c0 += 64) {
    const int c = c0 + lane, cy = c / NFULL, cx = c - cy * NFULL;
    const bool in = c < NFULL * NFULL;
    const int dx = in ? 2 * cx - MOBI_ENCP_RANGE : 0, dy = in ? 2 * cy - MOBI_ENCP_RANGE : 0; // a lane without a candidate walks the centre
    const int ox = (dx >> 1) + WIN_LEFT, oy = (dy >> 1) + WIN_BACK, b = ox >> 2, sh = ox & 3;
    uint32_t qs[4] = {0, 0, 0, 0};
#pragma unroll
    for (int hv = 0; hv < 2; hv++) {
#pragma unroll 4
      for (int r8 = 0; r8 < 8; r8++) {
        const int r = hv * 8 + r8;
        const uint32_t *wr = win + (oy + r) * WIN_DW + b; // b + 4 <= 9
        const uint32_t w[6] = {wr[0], wr[1], wr[2], wr[3], wr[4], 0u};
#pragma unroll
        for (int k = 0; k < 4; k++) qs[hv * 2 + (k >> 1)] = __builtin_amdgcn_sad_u8(row_word(w, k, sh), srcm[r * 4 + k], qs[hv * 2 + (k >> 1)]);
      }
    }
    // the spans of the three extents per axis: the whole, the first half, the second half
    const bool okx[3] = {in && mobi_encq_span_ok(W, X0, 16, dx), in && mobi_encq_span_ok(W, X0, 8, dx), in && mobi_encq_span_ok(W, X0 + 8, 8, dx)};
    const bool oky[3] = {mobi_encq_span_ok(H, Y0, 16, dy), mobi_encq_span_ok(H, Y0, 8, dy), mobi_encq_span_ok(H, Y0 + 8, 8, dy)};
    const uint32_t sads[MOBI_ENCQ_LEAVES] = {qs[0] + qs[1] + qs[2] + qs[3], qs[0] + qs[1], qs[2] + qs[3], qs[0] + qs[2], qs[1] + qs[3], qs[0], qs[1], qs[2], qs[3]};
    const uint64_t rate = mobi_encp_key(lam, 0u, dx, dy); // the key is linear in the SAD: cost << 20 with cost = (sad << 8) + rate
#pragma unroll
    for (int l = 0; l < MOBI_ENCQ_LEAVES; l++) {
      const MobiEncqLeaf f = mobi_encq_leaf(l);
      const bool ok = okx[f.w == 16 ? 0 : 1 + f.x / 8] && oky[f.h == 16 ? 0 : 1 + f.y / 8];
      const uint64_t key = ok ? rate + ((uint64_t)sads[l] << 28) : MOBI_ENCP_NO_KEY;
      best[l] = key < best[l] ? key : best[l];
    }
  }
#pragma unroll
  for (int l = 0; l < MOBI_ENCQ_LEAVES; l++) best[l] = lanes_min64<1>(best[l]); // (0, 0) always has a key

  // ---- step 2: eight half-pel neighbours of every leaf; lane = 8 * neighbour + part, a leaf's parts are neighbouring lanes ----
  const int cand = lane >> 3, part = lane & 7;
  {
    int dx, dy;
    neighbour(best[0], cand, &dx, &dy);
    const uint32_t sad = mobi_lanes_sum<8>(halfpel_sad<4, 2>(win, srcm, 0, 2 * part, dx, dy));
    const uint64_t key = mobi_encq_leaf_ok(W, H, X0, Y0, 16, 16, dx, dy) ? mobi_encp_key(lam, sad, dx, dy) : MOBI_ENCP_NO_KEY;
    best[0] = lanes_min64<8>(key < best[0] ? key : best[0]);
  }
  { // top and bottom: parts 0..3 and 4..7, two rows each
    const int half = part >> 2;
    const uint64_t mine = half ? best[2] : best[1];
    int dx, dy;
    neighbour(mine, cand, &dx, &dy);
    const uint32_t sad = mobi_lanes_sum<4>(halfpel_sad<4, 2>(win, srcm, 0, 2 * part, dx, dy));
    const uint64_t key = mobi_encq_leaf_ok(W, H, X0, Y0 + 8 * half, 16, 8, dx, dy) ? mobi_encp_key(lam, sad, dx, dy) : MOBI_ENCP_NO_KEY;
    const uint64_t m = lanes_min64<8>(key < mine ? key : mine);
    best[1] = shfl64(m, 0);
    best[2] = shfl64(m, 4);
  }
  { // left and right: parts 0..3 and 4..7, four rows of two words each
    const int half = part >> 2;
    const uint64_t mine = half ? best[4] : best[3];
    int dx, dy;
    neighbour(mine, cand, &dx, &dy);
    const uint32_t sad = mobi_lanes_sum<4>(halfpel_sad<2, 4>(win, srcm, 8 * half, 4 * (part & 3), dx, dy));
    const uint64_t key = mobi_encq_leaf_ok(W, H, X0 + 8 * half, Y0, 8, 16, dx, dy) ? mobi_encp_key(lam, sad, dx, dy) : MOBI_ENCP_NO_KEY;
    const uint64_t m = lanes_min64<8>(key < mine ? key : mine);
    best[3] = shfl64(m, 0);
    best[4] = shfl64(m, 4);
  }
  { // the quadrants: parts 2 qd and 2 qd + 1, four rows of two words each
    const int qd = part >> 1;
    const uint64_t mine = qd == 0 ? best[5] : qd == 1 ? best[6] : qd == 2 ? best[7] : best[8];
    int dx, dy;
    neighbour(mine, cand, &dx, &dy);
    const uint32_t sad = mobi_lanes_sum<2>(halfpel_sad<2, 4>(win, srcm, 8 * (qd & 1), 8 * (qd >> 1) + 4 * (part & 1), dx, dy));
    const uint64_t key = mobi_encq_leaf_ok(W, H, X0 + 8 * (qd & 1), Y0 + 8 * (qd >> 1), 8, 8, dx, dy) ? mobi_encp_key(lam, sad, dx, dy) : MOBI_ENCP_NO_KEY;
    const uint64_t m = lanes_min64<8>(key < mine ? key : mine);
#pragma unroll
    for (int k = 0; k < 4; k++) best[5 + k] = shfl64(m, 2 * k);
  }

  // ---- the tree: every lane holds the nine keys ----
  uint64_t C[MOBI_ENCQ_LEAVES];
#pragma unroll
  for (int l = 0; l < MOBI_ENCQ_LEAVES; l++) C[l] = mobi_encq_key_cost(best[l]);
  const int tree = mobi_encq_decide(A.kq, A.ver, lam, C);
  if (lane < 4) {
    uint64_t k = best[0];
    const int l = mobi_encq_leaf_of(tree, lane);
#pragma unroll
    for (int j = 1; j < MOBI_ENCQ_LEAVES; j++) k = l == j ? best[j] : k;
    const uint32_t v = mobi_encp_pack(mobi_encp_key_dx(k), mobi_encp_key_dy(k));
    const size_t at = (size_t)pic * ((size_t)A.mbw * A.mbh) + mb;
    A.mv4[at * 4 + lane] = v;
    if (lane == 3) {
      A.mv[at] = v; // the last leaf: what the neighbours' predictors see
      A.mbs[at].luma_mode = (uint8_t)tree;
    }
  }
}

namespace {
struct CodeLds {
  int tile[8][8][9];  // transposes (pitch 9: a column read of eight lanes hits eight banks)
  int16_t nat[8][64]; // a block's levels in natural order
};
// four predicted samples at (x, y) of a plane for a vector's whole part already added and its phase: the aligned words that hold bytes
// x .. x + 3 (+ 1 for a horizontal phase) of the row (and of the row below for a vertical phase), the second word only when they reach it
__device__ __forceinline__ uint32_t pred4(const uint8_t *plane, int pitch, int x, int y, int phase) {
  const int off = x & 3;
  const uint32_t *w = (const uint32_t *)(plane + (size_t)y * pitch + (x - off)), *wn = (const uint32_t *)((const uint8_t *)w + pitch);
  const bool second = off + (phase & 1) > 0;
  const uint32_t wa[3] = {w[0], second ? w[1] : 0u, 0u};
  uint32_t wc[3] = {0u, 0u, 0u};
  if (phase & 2) {
    wc[0] = wn[0];
    wc[1] = second ? wn[1] : 0u;
  }
  return mobi_mc4(row_word(wa, 0, off), row_word(wa, 0, off + 1), row_word(wc, 0, off), row_word(wc, 0, off + 1), phase);
}
} // namespace

extern "C" __global__ __launch_bounds__(WAVES * 64) void mobi_encq_code(MobiEncPartsArgs A) {
  __shared__ uint32_t lut32[MOBI_TC_LUT_BYTES / 4];
  __shared__ CodeLds lds[WAVES];
  const MobiEncPartsConst *K = A.kq;
  const uint8_t *lut = mobi_lanes_stage_lut<WAVES * 64>(K, lut32);
  __syncthreads();
  const int wave = threadIdx.x >> 6, pic = blockIdx.y, nmb = A.mbw * A.mbh, mb = blockIdx.x * WAVES + wave;
  if (mb >= nmb) return; // a whole wave: nothing below synchronises beyond the wave
  CodeLds &L = lds[wave];
  const MobiSyncWave wave_sync;
  const int lane = threadIdx.x & 63, g = lane >> 3, r = lane & 7, k = g < 6 ? g : 0;
  const int mby = mb / A.mbw, mbx = mb - mby * A.mbw, W = A.W, q = A.q[pic];
  const size_t ysz = (size_t)W * A.H, frame = ysz + ysz / 2;
  const uint32_t *mvs = A.mv + (size_t)pic * nmb;
  const uint4 v4 = *(const uint4 *)(A.mv4 + ((size_t)pic * nmb + mb) * 4);
  const uint32_t vq[4] = {v4.x, v4.y, v4.z, v4.w};
  const MobiEncpBlockRef at = mobi_encp_block_ref(k, mbx, mby, W, 0, 0); // the block's place; the vectors follow per half row
  const size_t plane = at.plane ? ysz + (size_t)(at.plane - 1) * (ysz / 4) : 0;
  int zi[8], s[8], p[8], x[8], d[8];
  mobi_lanes_scan<8>(K, r, zi);
  Row<8>::unpack(*(const uint2 *)(A.src + (size_t)pic * A.src_pitch + plane + (size_t)(at.y0 + r) * at.pitch + at.x0), s);
  {
    // a luma block's row: both halves with its quadrant's vector; a chroma block's: the chroma vectors of the quadrants the row crosses.
    // Each half's window lies inside the plane's rectangle: it is part of a window mobi_encq_leaf_ok admitted.
    const uint8_t *rp = A.ref + (size_t)pic * A.ref_pitch + plane;
    uint32_t pr[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int qd = k < 4 ? k : (r >> 2) * 2 + h;
      uint32_t v = vq[0];
#pragma unroll
      for (int j = 1; j < 4; j++) v = qd == j ? vq[j] : v;
      const int vx = k < 4 ? mobi_encp_dx(v) : mobi_encp_dx(v) >> 1, vy = k < 4 ? mobi_encp_dy(v) : mobi_encp_dy(v) >> 1;
      pr[h] = pred4(rp, at.pitch, at.x0 + 4 * h + (vx >> 1), at.y0 + r + (vy >> 1), (vx & 1) | (vy & 1) << 1);
    }
    Row<8>::unpack(uint2{pr[0], pr[1]}, p);
  }
  // the block coder's steps at wave scope; every group runs them, 6 and 7 too: the shuffles stay convergent
#pragma unroll
  for (int j = 0; j < 8; j++) x[j] = s[j] - p[j];
  mobi_lanes_forward<8>(x, r, L.tile[g], wave_sync, d);
  MobiLaneCoded<8> c;
  mobi_lanes_code<8>(K, lut, q, r, zi, s, p, d, L.tile[g], L.nat[g], wave_sync, c);
  const uint32_t sum2 = mobi_lanes_sum<8>(c.sad_pred | c.range << 14);
  const MobiEncBlock b = mobi_enc_block_result(c.mask != 0, c.clamp(), (sum2 >> 14) != 0, (int)c.bits(), (int)c.sad(), (int)(sum2 & 0x3FFF));
  MobiEncMb *rec_mb = A.mbs + (size_t)pic * nmb + mb;
  if (g < 6) {
    int px[8], lv[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      px[j] = b.coded ? c.px[j] : p[j];
      lv[j] = b.coded ? c.lv[j] : 0;
    }
    *(uint2 *)(A.rec + (size_t)pic * frame + plane + (size_t)(at.y0 + r) * at.pitch + at.x0) = Row<8>::pack(px);
    const int4 l4 = Row<8>::pack_lev(lv);
    uint2 *dst = (uint2 *)(rec_mb->lev[g] + r * 8); // records are 8-byte aligned, not 16
    dst[0] = uint2{(uint32_t)l4.x, (uint32_t)l4.y};
    dst[1] = uint2{(uint32_t)l4.z, (uint32_t)l4.w};
  }
  // every block's figures to every lane: coded, clamp, range, bits (< 2^11), sad (< 2^14)
  const uint32_t mine = (uint32_t)b.coded | (uint32_t)b.clamp << 1 | (uint32_t)b.range << 2 | (uint32_t)b.bits << 3 | (uint32_t)b.sad << 14;
  uint32_t cbp = 0, bits = 0, sad = 0, clamp = 0, range = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
    const uint32_t o = (uint32_t)__shfl((int)mine, a * 8);
    cbp |= (o & 1) << a;
    clamp += (o >> 1) & 1;
    range += (o >> 2) & 1;
    bits += (o >> 3) & 0x7FF;
    sad += o >> 14;
  }
  if (lane == 0) {
    const int tree = rec_mb->luma_mode; // the search's
    const uint32_t pred = mobi_encp_predictor(mvs, A.mbw, mbx, mby);
    const MobiEncqSyntax sx = mobi_encq_syntax(K, A.ver, tree, vq, pred);
    A.mvp[(size_t)pic * nmb + mb] = pred;
    rec_mb->bits = sx.bits + mobi_encp_cbp_bits(K, cbp) + bits;
    rec_mb->chroma_mode = rec_mb->pad = 0;
    rec_mb->cbp = (uint8_t)cbp;
    if (A.pstats) {
      mobi_enc_inter_stats *st = A.pstats + pic;
      atomicAdd((unsigned long long *)&st->sad, (unsigned long long)sad);
      atomicAdd((unsigned long long *)&st->mv_bits, (unsigned long long)sx.bits);
      if (cbp) atomicAdd(&st->coded_blocks, (uint32_t)__popc(cbp));
      if (clamp) atomicAdd(&st->fallback_clamp, clamp);
      if (range) atomicAdd(&st->fallback_level, range);
      if (sx.code0) atomicAdd(&st->code0, sx.code0);
      if (sx.nonzero) atomicAdd(&st->nonzero_mv, sx.nonzero);
      if (sx.halfpel) atomicAdd(&st->halfpel_mv, sx.halfpel);
      if (tree != MOBI_ENCQ_ROOT_LEAF) atomicAdd(&st->reserved[MOBI_ENC_PARTS_STAT_SPLIT], 1u);
      atomicAdd(&st->reserved[MOBI_ENC_PARTS_STAT_LEAVES], sx.leaves);
    }
  }
}

// ---- write: mobi_encode_write.h's scan and writer with the partition speller ----
namespace {
struct PartsSpeller {
  __device__ static uint32_t header_bits(const MobiEncPartsArgs &A, int pic) { return (uint32_t)mobi_encp_header_bits(A.q[pic], A.prev_q[pic]); }
  template <class Put> __device__ static void header(const MobiEncPartsArgs &A, int pic, Put put) { mobi_encp_write_header(put, A.q[pic], A.prev_q[pic]); }
  template <class Put> __device__ static void macroblock(const MobiEncPartsArgs &A, int pic, int i, Put put) {
    const size_t at = (size_t)pic * ((size_t)A.mbw * A.mbh) + i;
    const uint4 v4 = *(const uint4 *)(A.mv4 + at * 4);
    const uint32_t vq[4] = {v4.x, v4.y, v4.z, v4.w};
    mobi_encq_write_mb(A.kq, A.ver, A.mbs + at, vq, A.mvp[at], put, (uint32_t *)nullptr);
  }
  __device__ static void total(const MobiEncPartsArgs &A, int pic, uint32_t bits) {
    if (A.pstats) A.pstats[pic].bits = bits;
  }
};
} // namespace

extern "C" __global__ __launch_bounds__(256) void mobi_encq_scan(MobiEncPartsArgs A) { mobi_enc_scan_body<PartsSpeller>(A); }
extern "C" __global__ __launch_bounds__(64) void mobi_encq_write(MobiEncPartsArgs A) { mobi_enc_write_body<PartsSpeller>(A); }

// stages: as mobi_launch_encode_inter
extern "C" int mobi_launch_encode_parts(const MobiEncPartsArgs *a, int stages, hipStream_t s) {
  const int nmb = a->mbw * a->mbh;
  if (stages & 1) hipLaunchKernelGGL(mobi_encq_search, dim3(nmb, a->n), dim3(64), 0, s, *a);
  if (stages & 2) hipLaunchKernelGGL(mobi_encq_code, dim3((nmb + WAVES - 1) / WAVES, a->n), dim3(WAVES * 64), 0, s, *a);
  if (stages & 4) hipLaunchKernelGGL(mobi_encq_scan, dim3(a->n), dim3(256), 0, s, *a);
  if (stages & 8) hipLaunchKernelGGL(mobi_encq_write, dim3((nmb + 63) / 64, a->n), dim3(64), 0, s, *a);
  return (int)hipGetLastError();
}
