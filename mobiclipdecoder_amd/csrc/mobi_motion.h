// mobi_motion.h -- command list -> motion: what the stream says about every 2x2 cell and every macroblock of a frame, read back out of
// the command list the parsers wrote (mobi_cmd.h).  Host and device code, like mobi_audio.h and mobi_recon_math.h: the kernel
// (mobi_motion.hip), the export kernels behind it and the CPU statement of the tests (tests/tools/mobi_motion_host.cpp) all compile this.
// It reads the command list through mobi_cmd.h's readers only.
//
// A cell is the 2x2 luma block at (x, y) of its macroblock, cell = (y / 2) * 8 + x / 2, the grain of the MV cell map.  Its motion is
// (dx, dy, ref): half samples, ref 1..5 = frames back, ref 0 = the macroblock is intra (dx = dy = 0).  The vector points from the block to
// its source in the reference picture: the decoder's sign.
//
// CANONICAL FORM.  The reference addresses linearly (MD.cs:400-416), so (dx - 4 t S, dy + 4 t), S = Stride, is the same copy for every t
// (mobi_parse.cpp, mc_leaf).  A leaf record (MbDesc.w3..w6, mobi_syntax.h: mobi_leaf_record) keeps a position and phases, i.e. the class and
// not the member the stream coded.  Every vector that leaves this header is therefore the member of its class with -2 S <= dx < 2 S: the
// leaf decoder below yields exactly that member, and cell-map vectors are brought to it (mobi_motion_canonical), so that the result does
// not depend on how the macroblock was partitioned.  Stride >= Width: a vector that moves by less than a picture width is exported as the
// stream codes it.
#ifndef MOBI_MOTION_H
#define MOBI_MOTION_H
#include "mobi_cmd.h"
#include "mobi_syntax.h" /* (mobi_leaf_record, for the checks at the end: what this header reads is mobi_cmd.h's) */

struct MobiMotion { int dx, dy, ref; };

// floor(a / b), b > 0
MOBI_CMD_FN int mobi_floor_div(int a, int b) { return a >= 0 ? a / b : -((b - 1 - a) / b); }
// the member of (dx, dy)'s class with -2 S <= dx < 2 S
MOBI_CMD_FN MobiMotion mobi_motion_canonical(int dx, int dy, int ref, int S) {
  if (dx >= -2 * S && dx < 2 * S) return MobiMotion{dx, dy, ref};
  const int t = mobi_floor_div(dx + 2 * S, 4 * S);
  return MobiMotion{dx - 4 * t * S, dy + 4 * t, ref};
}
// macroblock mb's offset in the luma plane: the cur_off of mobi_leaf_record, for leaf A and leaf B alike
MOBI_CMD_FN uint32_t mobi_mb_offset(uint32_t mb, uint32_t mbw, uint32_t S) { return (mb / mbw) * 16u * S + (mb % mbw) * 16u; }
// Leaf record i (0: leaf A, 1: leaf B) of a macroblock without a cell map -> its vector.  pos_y = cur_off + (dy >> 1) * S + (dx >> 1), so
// L = pos_y - cur_off splits into a column X in [-S / 2, S / 2) and a row Y; X's low bit is the chroma phase's bit 0 whatever the split
// (S is even), and where Y's low bit is not the chroma phase's bit 1 the true column lies one stride away, on the side that keeps it in [-S, S).
MOBI_CMD_FN MobiMotion mobi_motion_of_leaf(const MbDesc &d, int i, uint32_t cur_off, int S) {
  const int32_t L = (int32_t)((i ? d.w5 : d.w3) - cur_off);
  const int phase = (int)mobi_w2_phase(d.w2, i), cphase = (int)mobi_w2_cphase(d.w2, i);
  int Y = mobi_floor_div(L + S / 2, S), X = L - Y * S;
  if ((Y & 1) != (cphase >> 1)) {
    if (X < 0) { X += S; Y -= 1; }
    else { X -= S; Y += 1; }
  }
  return MobiMotion{2 * X + (phase & 1), 2 * Y + (phase >> 1), (int)mobi_w2_ref(d.w2, i)};
}
// which leaf record of a macroblock without a cell map moved `cell`: one leaf, or a DUAL pair (A = top / left, B = bottom / right)
MOBI_CMD_FN int mobi_motion_leaf_of_cell(uint32_t dual, int cell) {
  return dual == MOBI_DUAL_TB ? (cell >> 3) * 2 >= 8 : dual == MOBI_DUAL_LR ? (cell & 7) * 2 >= 8 : 0;
}
// a word of the MV cell map -> its vector, canonical
MOBI_CMD_FN MobiMotion mobi_motion_of_cell_word(uint32_t c, int S) { return mobi_motion_canonical(mobi_cell_dx(c), mobi_cell_dy(c), mobi_cell_ref(c), S); }
MOBI_CMD_FN bool mobi_motion_has_cells(uint32_t w1) { return !mobi_w1_intra(w1) && mobi_inter_hdr_words(mobi_w1_leaves(w1), (int)mobi_w1_dual(w1)) != 0; }
// THE STATEMENT: macroblock descriptor d (its offset in the luma plane: cur_off), pay = its payload (MbDesc.payload_off applied), cell 0..63
MOBI_CMD_FN MobiMotion mobi_motion_cell(const MbDesc &d, const uint32_t *pay, uint32_t cur_off, int S, int cell) {
  if (mobi_w1_intra(d.w1)) return MobiMotion{0, 0, 0};
  if (mobi_motion_has_cells(d.w1)) return mobi_motion_of_cell_word(pay[cell], S);
  return mobi_motion_of_leaf(d, mobi_motion_leaf_of_cell(mobi_w1_dual(d.w1), cell), cur_off, S);
}

// ---- per-macroblock data: five int32 values ----
enum { MOBI_MBV_TYPE = 0,   // MOBI_MB_INTER / MOBI_MB_INTRA
       MOBI_MBV_QUANT = 1,  // the quantiser field of MbDesc.w1 as shipped (MOBI_SCALE_LITERAL, MOBI_TQ_NONE included)
       MOBI_MBV_CBP = 2,    // cbp6
       MOBI_MBV_COEFS = 3,  // level words
       MOBI_MBV_LEVELS = 4, // sum of |level| over them
       MOBI_MB_VALUES = 5 };
MOBI_CMD_FN int32_t mobi_motion_mb_value(const MbDesc &d, int v) {
  return v == MOBI_MBV_TYPE ? (int32_t)mobi_w1_type(d.w1) : v == MOBI_MBV_QUANT ? (int32_t)mobi_w1_quant(d.w1) : v == MOBI_MBV_CBP ? (int32_t)mobi_w1_cbp6(d.w1)
                                                                                                                                  : (int32_t)mobi_w2_coefs(d.w2);
}
// the level words first, first + step, ... of the macroblock's share: pay as above.  (0, 1): the whole sum; (lane, lanes): one lane's part
MOBI_CMD_FN int32_t mobi_motion_level_sum(const MbDesc &d, const uint32_t *pay, uint32_t first, uint32_t step) {
  const uint32_t *lv = pay + mobi_levels_offset(d.w1);
  int32_t s = 0;
  for (uint32_t i = first, n = mobi_w2_coefs(d.w2); i < n; i += step) {
    const int32_t v = mobi_level_value(lv[i]);
    s += v < 0 ? -v : v;
  }
  return s;
}

// ---- the motion ring's cell word (mobi_batch_set_motion: [clip][slot][mb][64], beside the picture ring) ----
// [13:0] dx  [28:14] dy  [31:29] ref (0: intra).  A canonical dx is a vector the parsers accepted or smaller (|dx| <= MOBI_MV_LIMIT); its dy
// is that vector's dy moved by at most 4 * (MOBI_MV_LIMIT / 64 + 1) rows, which the fifteenth bit holds.
enum { MOBI_MCELL_DX_S = 0, MOBI_MCELL_DX_N = 14, MOBI_MCELL_DY_S = 14, MOBI_MCELL_DY_N = 15, MOBI_MCELL_REF_S = 29, MOBI_MCELL_REF_N = 3 };
MOBI_ASSERT_DISJOINT(mcell, MOBI_MASK_AT(MOBI_MCELL_DX), MOBI_MASK_AT(MOBI_MCELL_DY), MOBI_MASK_AT(MOBI_MCELL_REF))
MOBI_CMD_FN uint32_t mobi_mcell(MobiMotion m) { return MOBI_PUT(m.dx, MOBI_MCELL_DX) | MOBI_PUT(m.dy, MOBI_MCELL_DY) | MOBI_PUT(m.ref, MOBI_MCELL_REF); }
MOBI_CMD_FN int mobi_mcell_dx(uint32_t c) { return (int)(c << (32 - MOBI_MCELL_DX_S - MOBI_MCELL_DX_N)) >> (32 - MOBI_MCELL_DX_N); }
MOBI_CMD_FN int mobi_mcell_dy(uint32_t c) { return (int)(c << (32 - MOBI_MCELL_DY_S - MOBI_MCELL_DY_N)) >> (32 - MOBI_MCELL_DY_N); }
MOBI_CMD_FN int mobi_mcell_ref(uint32_t c) { return (int)MOBI_GET(c, MOBI_MCELL_REF); }
#define MOBI_MOTION_MB_WORDS 8 /* the ring's per-macroblock record: the five values, padded to the size of a descriptor */

// MOBI_MOTION_FLOW: a cell's displacement times 60 / ref (an integer: ref <= 5), 0 for intra cells; the sums over a block's cells are exact
MOBI_CMD_FN int mobi_flow_weight(int ref) { return ref ? 60 / ref : 0; }

namespace mobi_motion_check {
constexpr bool same(MobiMotion a, int dx, int dy, int ref) { return a.dx == dx && a.dy == dy && a.ref == ref; }
// through mobi_leaf_record (mobi_syntax.h) and back: the vector itself inside [-2 S, 2 S), else its class's member there
constexpr MobiMotion round_trip(int i, int dx, int dy, int ref, uint32_t cur_off, int S) {
  MbDesc d{};
  d.w2 = mobi_leaf_record(i, mobi_leaf_w0(0, 0, 0, 0, ref), mobi_leaf_w1(dx, dy), (long)cur_off, (long)S, i ? d.w5 : d.w3, i ? d.w6 : d.w4);
  return mobi_motion_of_leaf(d, i, cur_off, S);
}
static_assert(same(round_trip(0, 0, 0, 1, 4112, 256), 0, 0, 1) && same(round_trip(1, -511, 3, 5, 4112, 256), -511, 3, 5) && same(round_trip(0, 511, -7, 2, 4112, 256), 511, -7, 2) &&
              same(round_trip(0, -512, -2, 3, 4112, 256), -512, -2, 3) && same(round_trip(1, 255, 2, 1, 4112, 256), 255, 2, 1) && same(round_trip(0, 257, 1, 1, 4112, 256), 257, 1, 1),
              "a vector inside [-2 S, 2 S) comes back as it went in");
static_assert(same(round_trip(0, 512, 0, 1, 4112, 256), -512, 4, 1) && same(round_trip(0, 8191, -9, 4, 4112, 256), 8191 - 8 * 1024, -9 + 32, 4) &&
              same(mobi_motion_canonical(8191, -9, 4, 256), 8191 - 8 * 1024, -9 + 32, 4) && same(mobi_motion_canonical(-513, 0, 1, 256), 511, -4, 1),
              "a vector outside comes back as the canonical member, from a leaf record and from a cell word alike");
constexpr bool fours_share_a_leaf() { // (mobi_motion.hip: a lane takes four consecutive cells and decodes one leaf for them)
  for (uint32_t dual = MOBI_DUAL_NONE; dual <= MOBI_DUAL_LR; dual++)
    for (int c = 0; c < MOBI_MV_CELLS; c += 4)
      for (int k = 1; k < 4; k++)
        if (mobi_motion_leaf_of_cell(dual, c + k) != mobi_motion_leaf_of_cell(dual, c)) return false;
  return true;
}
static_assert(fours_share_a_leaf(), "four consecutive cells lie in one half of a DUAL macroblock");
constexpr uint32_t M = mobi_mcell(MobiMotion{-8192, 16383, 5});
static_assert(mobi_mcell_dx(M) == -8192 && mobi_mcell_dy(M) == 16383 && mobi_mcell_ref(M) == 5 && mobi_mcell_ref(mobi_mcell(MobiMotion{0, 0, 0})) == 0, "ring cell round trip");
} // namespace mobi_motion_check
#endif
