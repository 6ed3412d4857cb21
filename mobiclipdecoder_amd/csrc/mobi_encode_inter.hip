// mobi_encode_inter.hip -- the inter encoder on gfx950 (include/mobiclip_encode_inter.h; the rules are mobi_encode_inter.h's, DESIGN.md
// "Inter encoder").  No macroblock of a P-frame reads another's pixels, so every stage is one launch over all macroblocks of all pictures.
//
// Search (mobi_encp_search).  One wave = one macroblock.  The 34 x 40 byte window of the reference's luma around the macroblock (17
// half-pels either way, the extra row and column of the half-pel phases, rows cut to whole words) and the macroblock's 16 x 16 source
// are staged in LDS once.  Step 1: the 289 full-pel candidates are dealt to the lanes, five rounds; a lane walks its candidate's 16 rows:
// five words of the window, v_alignbyte_b32 to the candidate's column, v_sad_u8 against the source row.  Step 2: the eight half-pel
// neighbours of the winner, eight lanes each, a lane two rows: the decoder's mobi_mc4 on the aligned words.  Cost and tie rule are one
// 64-bit key (mobi_encp_key); both argmins are wave-level minima of it.  A candidate outside the picture's rectangle has no key.
//
// Code (mobi_encp_code).  One wave = one macroblock, four to a workgroup.  Lane groups 0..5 code the blocks Y0..Y3, U, V, one lane per
// row, with the block coder of mobi_txcode_lanes.h at wave scope; groups 6 and 7 shadow group 0 so that the shuffles stay convergent, and
// store nothing.  A lane fetches its row of the prediction straight from the reference (two or three aligned words per row, two rows
// for a vertical phase) and runs the decoder's mobi_mc4 on it.  Lane 0 takes the predictor from the neighbours' v*, prices the
// macroblock's syntax, writes the record and adds to the picture's statistics by integer atomics.  The body is mobi_encode_inter_code.h's
// text; mobi_encp_code_pintra is the same text for the intra mode (mobi_encode_pintra.h), whose lane 0 leaves the cost Jp and a kind word.
//
// Write.  mobi_encode_write.h's scan and bit writer with the P-frame's speller.
#include <hip/hip_runtime.h>

#include "mobi_encode_inter.h"
#include "mobi_encode_pintra.h"
#include "mobi_encode_write.h"
#include "mobi_txcode_lanes.h"

namespace {

constexpr int WAVES = 4;                                         // per workgroup of the code kernel
constexpr int WIN_BACK = MOBI_ENCP_REACH / 2 + 1;                // 9: samples in front of the macroblock a vector can reach (-17 >> 1)
constexpr int WIN_LEFT = (WIN_BACK + 3) & ~3;                    // 12: the window starts on a word
constexpr int WIN_ROWS = WIN_BACK + 16 + MOBI_ENCP_REACH / 2 + 1; // 34: ... and behind it, with the row a vertical phase adds
constexpr int WIN_DW = (WIN_LEFT + 16 + MOBI_ENCP_REACH / 2 + 1 + 3) / 4; // 10 words: columns -12 .. +27
constexpr int NFULL = MOBI_ENCP_RANGE + 1;                       // 17 full-pel positions either way, 289 candidates
static_assert(WIN_ROWS == 34 && WIN_DW == 10 && WIN_LEFT == 12, "the window the index arithmetic below was checked for");

__device__ __forceinline__ uint64_t wave_min64(uint64_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    const uint64_t o = (uint64_t)hi << 32 | lo;
    v = o < v ? o : v;
  }
  return v;
}
// the word at byte offset 4 * k + sh (sh in 0..4) of the row whose words are w[0..4] (w5 = what lies behind: only shifted out)
__device__ __forceinline__ uint32_t row_word(const uint32_t (&w)[6], int k, int sh) {
  const bool carry = sh >> 2;
  return __builtin_amdgcn_alignbyte(carry ? w[k + 2] : w[k + 1], carry ? w[k + 1] : w[k], (uint32_t)(sh & 3));
}

} // namespace

extern "C" __global__ __launch_bounds__(64) void mobi_encp_search(MobiEncInterArgs A) {
  __shared__ uint32_t win[WIN_ROWS * WIN_DW];
  __shared__ uint32_t srcm[16 * 4];
  const int lane = threadIdx.x, pic = blockIdx.y, mb = blockIdx.x;
  const int mby = mb / A.mbw, mbx = mb - mby * A.mbw, W = A.W, H = A.H, X0 = mbx * 16, Y0 = mby * 16;
  const uint8_t *src = A.src + (size_t)pic * A.src_pitch, *ref = A.ref + (size_t)pic * A.ref_pitch;
  const int64_t lam = mobi_enc_lambda(A.q[pic]);
  for (int idx = lane; idx < WIN_ROWS * WIN_DW; idx += 64) {
    const int r = idx / WIN_DW, dw = idx - r * WIN_DW, row = Y0 - WIN_BACK + r, col = X0 - WIN_LEFT + 4 * dw;
    // (W is a multiple of 16 and col of 4: a word is inside the row or outside it.)  Bytes outside the picture are never used:
    // mobi_encp_vector_ok leaves those candidates without a key.
    win[idx] = row >= 0 && row < H && col >= 0 && col < W ? *(const uint32_t *)(ref + (size_t)row * W + col) : 0u;
  }
  srcm[lane] = *(const uint32_t *)(src + (size_t)(Y0 + (lane >> 2)) * W + X0 + 4 * (lane & 3));
  __syncthreads(); // (one wave)

  // ---- step 1: full-pel candidates, one to a lane ----
  uint64_t best = MOBI_ENCP_NO_KEY;
#pragma unroll 1
  for (int c0 = 0; c0 < NFULL * NFULL; c0 += 64) {
    const int c = c0 + lane, cy = c / NFULL, cx = c - cy * NFULL, dx = 2 * cx - MOBI_ENCP_RANGE, dy = 2 * cy - MOBI_ENCP_RANGE;
    const bool ok = c < NFULL * NFULL && mobi_encp_vector_ok(W, H, mbx, mby, dx, dy);
    const int ox = (ok ? dx >> 1 : 0) + WIN_LEFT, oy = (ok ? dy >> 1 : 0) + WIN_BACK; // a lane without a candidate walks the centre
    const int b = ox >> 2, sh = ox & 3;
    uint32_t sad = 0;
#pragma unroll 4
    for (int r = 0; r < 16; r++) {
      const uint32_t *wr = win + (oy + r) * WIN_DW + b; // b + 4 <= 9
      const uint32_t w[6] = {wr[0], wr[1], wr[2], wr[3], wr[4], 0u};
#pragma unroll
      for (int k = 0; k < 4; k++) sad = __builtin_amdgcn_sad_u8(row_word(w, k, sh), srcm[r * 4 + k], sad);
    }
    const uint64_t key = ok ? mobi_encp_key(lam, sad, dx, dy) : MOBI_ENCP_NO_KEY;
    best = key < best ? key : best;
  }
  best = wave_min64(best); // (0, 0) always has a key

  // ---- step 2: the eight half-pel neighbours, eight lanes each, two rows a lane ----
  {
    const int cand = lane >> 3, rp = lane & 7, idx = cand < 4 ? cand : cand + 1; // 0..8 without the centre
    const int dx = mobi_encp_key_dx(best) + idx % 3 - 1, dy = mobi_encp_key_dy(best) + idx / 3 - 1;
    const bool ok = mobi_encp_vector_ok(W, H, mbx, mby, dx, dy);
    const int ox = (ok ? dx >> 1 : 0) + WIN_LEFT, oy = (ok ? dy >> 1 : 0) + WIN_BACK, phase = (dx & 1) | (dy & 1) << 1;
    const int b = ox >> 2, sh = ox & 3; // bytes ox .. ox + 16 lie in words b .. b + 4, b + 4 <= 9
    uint32_t sad = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int r = 2 * rp + h;
      const uint32_t *w0 = win + (oy + r) * WIN_DW + b, *w1 = w0 + WIN_DW; // row oy + r + 1 <= 33
      const uint32_t wa[6] = {w0[0], w0[1], w0[2], w0[3], w0[4], 0u}, wc[6] = {w1[0], w1[1], w1[2], w1[3], w1[4], 0u};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t p = mobi_mc4(row_word(wa, k, sh), row_word(wa, k, sh + 1), row_word(wc, k, sh), row_word(wc, k, sh + 1), phase);
        sad = __builtin_amdgcn_sad_u8(p, srcm[r * 4 + k], sad);
      }
    }
    sad = mobi_lanes_sum<8>(sad);
    const uint64_t key = ok ? mobi_encp_key(lam, sad, dx, dy) : MOBI_ENCP_NO_KEY;
    best = wave_min64(key < best ? key : best);
  }
  if (lane == 0) A.mv[(size_t)pic * ((size_t)A.mbw * A.mbh) + mb] = mobi_encp_pack(mobi_encp_key_dx(best), mobi_encp_key_dy(best));
}

namespace {
struct CodeLds {
  int tile[8][8][9];  // transposes (pitch 9: a column read of eight lanes hits eight banks)
  int16_t nat[8][64]; // a block's levels in natural order
};
// eight bytes at byte offset k (0..4) of the twelve in lo (bytes 0..7) and hi (bytes 8..11)
__device__ __forceinline__ uint64_t bytes8(uint64_t lo, uint32_t hi, int k) { return k ? lo >> (8 * k) | (uint64_t)hi << (64 - 8 * k) : lo; }

} // namespace

// the two code kernels: one body (mobi_encode_inter_code.h), mode 0's and the intra mode's
extern "C" __global__ __launch_bounds__(WAVES * 64) void mobi_encp_code(MobiEncInterArgs A) {
  constexpr bool PINTRA = false;
#include "mobi_encode_inter_code.h"
}
extern "C" __global__ __launch_bounds__(WAVES * 64) void mobi_encp_code_pintra(MobiEncInterArgs A) {
  constexpr bool PINTRA = true;
#include "mobi_encode_inter_code.h"
}

// ---- write: mobi_encode_write.h's scan and writer with the P-frame's speller ----
namespace {
struct InterSpeller {
  __device__ static uint32_t header_bits(const MobiEncInterArgs &A, int pic) { return (uint32_t)mobi_encp_header_bits(A.q[pic], A.prev_q[pic]); }
  template <class Put> __device__ static void header(const MobiEncInterArgs &A, int pic, Put put) { mobi_encp_write_header(put, A.q[pic], A.prev_q[pic]); }
  template <class Put> __device__ static void macroblock(const MobiEncInterArgs &A, int pic, int i, Put put) {
    const size_t at = (size_t)pic * ((size_t)A.mbw * A.mbh) + i;
    mobi_encp_write_mb(A.kp, A.ver, A.mbs + at, A.mv[at], A.mvp[at], put, (uint32_t *)nullptr);
  }
  __device__ static void total(const MobiEncInterArgs &A, int pic, uint32_t bits) {
    if (A.pstats) A.pstats[pic].bits = bits;
  }
};
} // namespace

extern "C" __global__ __launch_bounds__(256) void mobi_encp_scan(MobiEncInterArgs A) { mobi_enc_scan_body<InterSpeller>(A); }
extern "C" __global__ __launch_bounds__(64) void mobi_encp_write(MobiEncInterArgs A) { mobi_enc_write_body<InterSpeller>(A); }

extern "C" int mobi_launch_encode_pintra(const MobiEncInterArgs *a, int stages, hipStream_t s); // mobi_encode_pintra.hip

// stages: bit 0 = search, bit 1 = code, bit 2 = scan, bit 3 = write (a frame runs all four; a trial of the rate rule, mobi_encode_rate.h,
// stops behind the scan and touches no slot).  The intra mode adds bit 4 = decide and bit 5 = finish, which run between code and scan; with
// either set the code kernel is the mode's, and scan and write spell either kind of macroblock (mobi_encode_pintra.hip).
extern "C" int mobi_launch_encode_inter(const MobiEncInterArgs *a, int stages, hipStream_t s) {
  const int nmb = a->mbw * a->mbh;
  const bool pintra = (stages & (16 | 32)) != 0;
  if (stages & 1) hipLaunchKernelGGL(mobi_encp_search, dim3(nmb, a->n), dim3(64), 0, s, *a);
  if ((stages & 2) && pintra) hipLaunchKernelGGL(mobi_encp_code_pintra, dim3((nmb + WAVES - 1) / WAVES, a->n), dim3(WAVES * 64), 0, s, *a);
  if (pintra) return mobi_launch_encode_pintra(a, stages, s);
  if (stages & 2) hipLaunchKernelGGL(mobi_encp_code, dim3((nmb + WAVES - 1) / WAVES, a->n), dim3(WAVES * 64), 0, s, *a);
  if (stages & 4) hipLaunchKernelGGL(mobi_encp_scan, dim3(a->n), dim3(256), 0, s, *a);
  if (stages & 8) hipLaunchKernelGGL(mobi_encp_write, dim3((nmb + 63) / 64, a->n), dim3(64), 0, s, *a);
  return (int)hipGetLastError();
}
