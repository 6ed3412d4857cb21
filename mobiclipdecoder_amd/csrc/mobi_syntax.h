// mobi_syntax.h -- what the parsers know about the bitstream's leaves, ONCE.
//
// Three walks read the same grammar -- mobi_parse.cpp (recursion, exceptions), mobi_dparse.hip (a work stack, a sticky error code),
// mobi_lsparse.h (a state machine that bails out) -- and mobi_gop.h reads the frame header a fourth time.  Their control flow differs for
// good reasons and stays with them.  The facts below do not differ: small pure functions, no state, compiled for host and device alike;
// every error policy (throw, fail, bail) stays with the caller, which gets a bool or a code to act on.
//
// One copy is NOT here: mobi_kernels.hip's Geo has its own owner_luma / owner_chroma.  That file is one of the four whose hash says whether
// the recorded memory-traffic profile still belongs to the kernels (bench.py), so it does not take a new include for two functions.
// The command list's words -- every position, width, reader and writer -- are mobi_cmd.h's; nothing here knows where a field sits.
#ifndef MOBI_SYNTAX_H
#define MOBI_SYNTAX_H
#include <stdint.h>

#include "mobi_cmd.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define MOBI_SYN_NOUNROLL _Pragma("nounroll")
#else
#define MOBI_SYN_NOUNROLL
#endif

// ---------------------------------------------------------------- geometry
// Which macroblock owns the sample at linear address `a` of the Y / UV plane; -1 = padding / outside.  The stride is 256 / 512 / 1024
// (MD.cs:50-52; lg = its log2), so rows and columns come by shift and mask.  A = the caller's address type (the host parser keeps long).
template <class A>
MOBI_CMD_FN int mobi_owner_luma(int width, int height, int stride, int lg, int mbw, A a) {
  if (a < 0) return -1;
  const A row = a >> lg, col = a & (stride - 1);
  if (col >= width || row >= height) return -1;
  return (int)((row >> 4) * mbw + (col >> 4));
}
template <class A>
MOBI_CMD_FN int mobi_owner_chroma(int width, int height, int stride, int lg, int mbw, A a) {
  if (a < 0) return -1;
  const A row = a >> lg, col = a & (stride - 1);
  const A x = col >= stride / 2 ? col - stride / 2 : col;
  if (x >= width / 2 || row >= height / 2) return -1;
  return (int)((row >> 3) * mbw + (x >> 3));
}
// plane offset of 8x8 area 0..5 (Y TL, TR, BL, BR, U, V) of the macroblock at luma offset cur_off, and of 4x4 block `sub` inside it
template <class A>
MOBI_CMD_FN A mobi_area_offset(A cur_off, A S, int area, int sub) {
  const A o = (area < 4) ? cur_off + (area >> 1) * 8 * S + (area & 1) * 8 : cur_off / 2 + (area == 5 ? S / 2 : 0);
  return o + (sub >> 1) * 4 * S + (sub & 1) * 4;
}

// ---------------------------------------------------------------- dependencies of an intra macroblock (MbDesc.w4..w7)
// The prediction halo of the macroblock at luma offset `off` is the row above (columns -1 .. +23 luma, -1 .. +15 chroma) and the columns
// left and right of it.  Its owners change only at 16-sample (8 for chroma) boundaries and, in the side columns, between the first row and
// the rest (row wrap when width == stride), so these 21 probes meet every distinct owner, in the order a full scan would.  f(owner).
template <class A, class F>
MOBI_CMD_FN void mobi_halo_owners(int width, int height, int stride, int lg, int mbw, A off, F f) {
  const A S = stride;
  f(mobi_owner_luma(width, height, stride, lg, mbw, off - S - 1));
  f(mobi_owner_luma(width, height, stride, lg, mbw, off - S));
  f(mobi_owner_luma(width, height, stride, lg, mbw, off - S + 16));
  f(mobi_owner_luma(width, height, stride, lg, mbw, off - 1));
  f(mobi_owner_luma(width, height, stride, lg, mbw, off + 16));
  f(mobi_owner_luma(width, height, stride, lg, mbw, off + S - 1));
  f(mobi_owner_luma(width, height, stride, lg, mbw, off + S + 16));
  MOBI_SYN_NOUNROLL
  for (int v = 0; v < 2; v++) {
    const A b = off / 2 + v * (S / 2);
    f(mobi_owner_chroma(width, height, stride, lg, mbw, b - S - 1));
    f(mobi_owner_chroma(width, height, stride, lg, mbw, b - S));
    f(mobi_owner_chroma(width, height, stride, lg, mbw, b - S + 8));
    f(mobi_owner_chroma(width, height, stride, lg, mbw, b - 1));
    f(mobi_owner_chroma(width, height, stride, lg, mbw, b + 8));
    f(mobi_owner_chroma(width, height, stride, lg, mbw, b + S - 1));
    f(mobi_owner_chroma(width, height, stride, lg, mbw, b + S + 8));
  }
}
// One probe's owner `o` against the list of macroblock mb.  Raster-later owners read as the fresh plane's zeros (the kernels mask them) and
// are no dependencies; an owner is listed once; is_intra(o) is only asked about an owner that gets listed.
enum { MOBI_DEP_FULL = -1,  // a ninth owner (cannot happen: the halo touches at most 7 macroblocks); nothing was added
       MOBI_DEP_SKIP = 0,   // outside, raster-later, or listed already
       MOBI_DEP_ADDED_INTER = 1, MOBI_DEP_ADDED_INTRA = 2 };
template <class I>
MOBI_CMD_FN int mobi_dep_add(uint32_t *deps, int &n, int mb, int o, I is_intra) {
  if (o < 0 || o >= mb) return MOBI_DEP_SKIP;
  MOBI_SYN_NOUNROLL
  for (int k = 0; k < n; k++)
    if ((int)mobi_dep_mb(deps[k]) == o) return MOBI_DEP_SKIP;
  if (n == MOBI_INTRA_DEPS) return MOBI_DEP_FULL;
  const bool intra = is_intra(o);
  deps[n++] = (uint32_t)o | (intra ? 0u : MOBI_DEP_INTER);
  return intra ? MOBI_DEP_ADDED_INTRA : MOBI_DEP_ADDED_INTER;
}
// the list's n entries, the rest MOBI_DEP_NONE, as the four descriptor words
MOBI_CMD_FN void mobi_deps_pack(uint32_t *deps, int n, uint32_t &w4, uint32_t &w5, uint32_t &w6, uint32_t &w7) {
  MOBI_SYN_NOUNROLL
  for (int k = n; k < MOBI_INTRA_DEPS; k++) deps[k] = MOBI_DEP_NONE;
  w4 = mobi_dep_pair(deps[0], deps[1]);
  w5 = mobi_dep_pair(deps[2], deps[3]);
  w6 = mobi_dep_pair(deps[4], deps[5]);
  w7 = mobi_dep_pair(deps[6], deps[7]);
}

// ---------------------------------------------------------------- motion (MD.cs:400-456)
// Would CopyBlock throw?  Rows are visited top to bottom, so first row / last row bound the rest.  One w x h window at `pos` with
// half-pel phase (dx & 1) | (dy & 1) << 1 inside a plane of plane_len samples.
template <class A>
MOBI_CMD_FN bool mobi_window_ok(A pos, int w, int h, int phase, A S, A plane_len) {
  if (pos < 0) return false;
  A hi = pos + (A)(h - 1) * S + w - 1; // highest index touched (phase 0: Array.Copy end is exclusive)
  if (phase & 1) hi += 1;
  if (phase & 2) hi += S;
  return hi < plane_len;
}
// The three windows of a leaf whose vector lies within +-MOBI_MV_LIMIT (every position fits A) at once: the luma one, and of the two chroma
// ones U starts first and V (S / 2 further) ends last.  off = the leaf's luma offset, w x h its size.
template <class A>
MOBI_CMD_FN bool mobi_mc_windows_ok(A S, int height, A off, int w, int h, int dx, int dy) {
  const A ylen = S * height;
  const A pos = off + (A)(dy >> 1) * S + (dx >> 1);
  const A hi_y = pos + (A)(h - 1) * S + w - 1 + (dx & 1) + ((dy & 1) ? S : 0);
  const int cdx = dx >> 1, cdy = dy >> 1;
  const A cpos = off / 2 + (A)(cdy >> 1) * S + (cdx >> 1);
  const A hi_c = cpos + S / 2 + (A)((h >> 1) - 1) * S + (w >> 1) - 1 + (cdx & 1) + ((cdy & 1) ? S : 0);
  return !(pos < 0 || hi_y >= ylen || cpos < 0 || hi_c >= ylen / 2);
}
// an inter macroblock of exactly two leaves (their mobi_leaf_w0 words, in stream order): two 16x8 halves, two 8x16 halves, or neither
MOBI_CMD_FN int mobi_dual_kind(uint32_t w0a, uint32_t w0b) {
  const uint32_t a = mobi_leaf_shape(w0a), b = mobi_leaf_shape(w0b); // position and size, whatever the ref slot
  if (a == mobi_leaf_w0(0, 0, 0, 1, 0) && b == mobi_leaf_w0(0, 8, 0, 1, 0)) return MOBI_DUAL_TB;
  if (a == mobi_leaf_w0(0, 0, 1, 0, 0) && b == mobi_leaf_w0(8, 0, 1, 0, 0)) return MOBI_DUAL_LR;
  return MOBI_DUAL_NONE;
}
// Leaf record i (0: leaf A, 1: leaf B) of a macroblock that travels without a cell map: positions and phases instead of a motion vector
// (MD.cs:400-416).  pos_y / pos_c: MbDesc.w3 / w4 (A) or w5 / w6 (B); returns the bits of MbDesc.w2.
template <class A>
MOBI_CMD_FN uint32_t mobi_leaf_record(int i, uint32_t w0, uint32_t w1, A cur_off, A S, uint32_t &pos_y, uint32_t &pos_c) {
  const int ref = mobi_leaf_ref(w0);
  // (dx, dy as expressions: through mobi_leaf_dy() the device parser's kernel compiles to other instructions)
  const int dx = (int16_t)(w1 & MOBI_MASK(MOBI_LEAF_DX)), dy = (int16_t)(w1 >> MOBI_LEAF_DY_S), cdx = dx >> 1, cdy = dy >> 1;
  pos_y = (uint32_t)(int32_t)(cur_off + (A)(dy >> 1) * S + (dx >> 1));
  pos_c = (uint32_t)(int32_t)(cur_off / 2 + (A)(cdy >> 1) * S + (cdx >> 1));
  // = mobi_w2_leaf(i, ref, phase, chroma phase), spelled out (through the function mobi_parse_frames_ls compiles to another order)
  return ((uint32_t)ref << (MOBI_W2_REFA_S + MOBI_W2_REF_STEP * i)) | ((uint32_t)((dx & 1) | ((dy & 1) << 1)) << (MOBI_W2_PHA_S + MOBI_W2_PH_STEP * i)) |
         ((uint32_t)((cdx & 1) | ((cdy & 1) << 1)) << (MOBI_W2_CPHA_S + MOBI_W2_PH_STEP * i));
}

// ---------------------------------------------------------------- intra syntax
// Reads PredictIntra (MD.cs:1883-2774) / the plane predictors (:3017-3327) make outside the block at plane offset `off`: the row above needs
// off - stride >= 0, the column to the left off - 1 >= 0; anything else is in range.  false: the reference indexes below the plane and throws.
#define MOBI_MODES_READ_TOP 0x1E5u  /* modes 0, 2, 5, 6, 7, 8 */
#define MOBI_MODES_READ_LEFT 0x0F6u /* modes 1, 2, 4, 5, 6, 7 */
template <class A>
MOBI_CMD_FN bool mobi_intra_reads_ok(int mode, A off, int stride) {
  return !((((MOBI_MODES_READ_TOP >> mode) & 1) && off < stride) || (((MOBI_MODES_READ_LEFT >> mode) & 1) && off < 1));
}
// predicted-mode code shared by loc_116220 / loc_116368 / sub_1163DC (MD.cs:1840-1859, 2785-2804, 2841-2858): top / left = the mode cache's
// entries above and to the left (MOBI_MODE_NONE: no neighbour), win = the reader's 32-bit window; the code is nbits (1 or 4) long
#define MOBI_MODE_NONE 9
MOBI_CMD_FN int mobi_pmode_decode(int top, int left, uint32_t win, int &nbits) {
  int pred = top < left ? top : left;
  if (pred == MOBI_MODE_NONE) pred = 3;
  int v = (int)(win >> 28), mode = pred;
  nbits = 1;
  if (v >= pred) v++;
  if (v < 9) { mode = v; nbits = 4; }
  return mode;
}

// ---------------------------------------------------------------- frame header: SetupQuantizationTables' visible part (MD.cs:3884-3925)
#define MOBI_QUANT_LIMIT 54 /* the table index throws from here on -- after Quantizer was assigned (MD.cs:3886-3890) */
MOBI_CMD_FN uint32_t mobi_clamp_quant(bool moflex3ds, uint32_t q) { return !moflex3ds ? q : q < 12 ? 12 : q > 52 ? 52 : q; }
// the mode cache's eight "no neighbour" marks, re-armed only there; at(i) = byte i of Internal[0..9] as an lvalue
template <class F>
MOBI_CMD_FN void mobi_rearm_borders(F at) {
  at(1) = MOBI_MODE_NONE; at(2) = MOBI_MODE_NONE; at(3) = MOBI_MODE_NONE; at(4) = MOBI_MODE_NONE;
  at(8) = MOBI_MODE_NONE; at(0x10) = MOBI_MODE_NONE; at(0x18) = MOBI_MODE_NONE; at(0x20) = MOBI_MODE_NONE;
}

// ---------------------------------------------------------------- Elias-gamma codes (MD.cs:2992-3015)
// z zeros, a one, z more bits at the top of a 32-bit window: 2z + 1 bits, value = 2^z - 1 + those bits.  Shift counts are masked to 5 bits
// as C# does, so z = 32 (an empty window) gives what the reference computes.  "Too long" is the caller's policy.
MOBI_CMD_FN uint32_t mobi_shl(uint32_t x, int n) { return x << (n & 31); }
MOBI_CMD_FN uint32_t mobi_shr(uint32_t x, int n) { return x >> (n & 31); }
MOBI_CMD_FN int mobi_clz32(uint32_t v) { return v ? __builtin_clz(v) : 32; } // MD.cs:3927
MOBI_CMD_FN uint32_t mobi_gamma_value(uint32_t win, int z) {
  return ((z == 0) ? 0u : mobi_shr(mobi_shl(win, z + 1), 32 - z)) + mobi_shl(1u, z) - 1u; // (z = 31: the window is 1 and either form gives 0 + 2^31 - 1)
}
MOBI_CMD_FN int mobi_gamma_bits(int z) { return 2 * z + 1; }
MOBI_CMD_FN int mobi_gamma_signed(uint32_t value) { // odd code numbers map to non-positive values (MD.cs:3009-3010)
  const uint32_t u = value + 1u;
  int v = (int)u;
  if (v & 1) v = (int)(1u - u);
  return v >> 1;
}

// ---------------------------------------------------------------- the reference's bit reader (MD.cs:2970-3015)
// R has win (r3), nbr (nrBitsRemaining) and fill_bits() (FillBits: one 16-bit word; its source and its end-of-data policy are R's own).
template <class R>
MOBI_CMD_FN void mobi_rd_take(R &r, int n) {
  r.win = mobi_shl(r.win, n);
  r.nbr -= n;
  if (r.nbr < 0) r.fill_bits();
}
template <class R>
MOBI_CMD_FN uint32_t mobi_rd_ue(R &r) {
  const int z = mobi_clz32(r.win);
  const uint32_t v = mobi_gamma_value(r.win, z);
  r.win = mobi_shl(mobi_shl(r.win, z) << 1, z);
  r.nbr -= 2 * z;
  if (--r.nbr < 0) r.fill_bits();
  return v;
}
template <class R>
MOBI_CMD_FN int mobi_rd_se(R &r) { return mobi_gamma_signed(mobi_rd_ue(r)); }
// One residual token (MD.cs:3346-3420): a table code, or behind the escape prefix 0000011 a table code whose level ("0") or run ("10")
// grows by a second table's entry, or ("11") last(1) run(6) level(s12) spelled out.  A: the 4096-entry code table (entry = length |
// level << 4 | run << 9 | last << 15), B: its escape table; TA / TB are the caller's pointer types (the device keeps them in LDS).
// Returns the token's "last" bit.
template <class R, class TA, class TB>
MOBI_CMD_RT uint32_t mobi_rd_token(R &r, TA A, TB B, int &skip, int &value) {
  uint32_t e;
  if ((r.win >> 25) == 3) { // escape prefix 0000011
    r.win <<= 7;
    bool c = (r.win >> 31) == 1;
    r.win <<= 1;
    if (!c) { // "0": table code, level += B[last<<6|run]
      r.nbr -= 8;
      if (r.nbr < 0) r.fill_bits();
      e = A[r.win >> 20];
      value = (int)((e >> 4) & 0x1F) + B[e >> 9];
      r.win = mobi_shl(r.win, (int)(e & 0xF) - 1);
      if (r.win >> 31) value = -value;
      r.win <<= 1;
      r.nbr -= (int)(e & 0xF);
      if (r.nbr < 0) r.fill_bits();
      skip = (int)((e >> 9) & 0x3F);
      e >>= 15;
    } else {
      c = (r.win >> 31) == 1;
      r.win <<= 1;
      r.nbr -= 9;
      if (r.nbr < 0) r.fill_bits();
      if (!c) { // "10": table code, run += B[0x80 + level + (last<<6)]
        e = A[r.win >> 20];
        value = (int)((e >> 4) & 0x1F);
        skip = (int)((e >> 9) & 0x3F) + B[0x80 + value + ((e >> 15) << 6)];
        r.win = mobi_shl(r.win, (int)(e & 0xF) - 1);
        if (r.win >> 31) value = -value;
        r.win <<= 1;
        r.nbr -= (int)(e & 0xF);
        if (r.nbr < 0) r.fill_bits();
        e >>= 15;
      } else { // "11": raw last(1) run(6) level(s12)
        e = r.win >> 31;
        r.win <<= 1;
        skip = (int)(r.win >> 26);
        r.win <<= 6;
        r.nbr -= 7;
        if (r.nbr < 0) r.fill_bits();
        value = (int32_t)r.win >> 20;
        r.win <<= 12;
        r.nbr -= 12;
        if (r.nbr < 0) r.fill_bits();
      }
    }
  } else {
    e = A[r.win >> 20];
    value = (int)((e >> 4) & 0x1F);
    r.win = mobi_shl(r.win, (int)(e & 0xF) - 1);
    if (r.win >> 31) value = -value;
    r.win <<= 1;
    r.nbr -= (int)(e & 0xF);
    if (r.nbr < 0) r.fill_bits();
    skip = (int)((e >> 9) & 0x3F);
    e >>= 15;
  }
  return e & 1;
}
#endif
