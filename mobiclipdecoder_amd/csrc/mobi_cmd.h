// mobi_cmd.h -- the host->GPU command list: what the serial bitstream parser (mobi_parse.cpp)
// emits per frame and what the reconstruction kernels (mobi_kernels.hip) consume.
//
// One frame of one clip =
//   MbDesc   desc[n_mbs]           32 B per macroblock, raster order (leaves of 1- and 2-leaf inter MBs are inline)
//   uint32_t payload[...]          variable: MV cell maps, intra block records, residual levels
//   uint32_t intra_items[...]      MB indices of intra MBs grouped by dependency level (host side only;
//                                  merged across clips into per-level launch lists)
//
// Positions are NOT stored as MB coordinates: like the reference, everything is a linear byte
// offset into the strided plane (MD.cs:212-217, SURVEY hard part 3); desc index -> offset is
// (mb / mbw) * 16 * stride + (mb % mbw) * 16 because widths are multiples of 16 here.
#ifndef MOBI_CMD_H
#define MOBI_CMD_H
#include <stdint.h>

#if defined(__HIPCC__)
#define MOBI_CMD_RT static __host__ __device__ inline __attribute__((always_inline)) /* (= __forceinline__, without needing hip_runtime.h) */
#else
#define MOBI_CMD_RT static inline
#endif
#define MOBI_CMD_FN MOBI_CMD_RT constexpr /* everything here and in mobi_syntax.h but the one function C++17 does not take as constexpr */

// THE ONLY PLACE THAT KNOWS A BIT POSITION.  Every field below is an enum pair NAME_S (shift) / NAME_N (width), a constexpr reader and
// a writer built from the same pair; the static_asserts at the end of this header hold the fields of a word apart and take every
// writer's output back through its readers, under the host compiler and the device compiler alike.  Where a reader function would change
// what a kernel compiles to (a lane-dependent shift folded into the field's; or only the order its operands are read in, which is enough
// to move this compiler's schedule: HISTORY.md), the site uses NAME_S / MOBI_MASK(NAME) / MOBI_GET in its own expression and says so;
// nothing outside this header writes a position or a width as a number.
#define MOBI_MASK(F) ((uint32_t)((1ull << F##_N) - 1ull))              /* the field's mask at bit 0 */
#define MOBI_MASK_AT(F) ((uint32_t)(((1ull << F##_N) - 1ull) << F##_S)) /* ... in place */
#define MOBI_GET(w, F) (((w) >> F##_S) & MOBI_MASK(F))
#define MOBI_PUT(v, F) (((uint32_t)(v) & MOBI_MASK(F)) << F##_S)

enum { MOBI_MB_INTER = 0, MOBI_MB_INTRA = 1 };

// ---- MbDesc: 32 B per macroblock; on the device one flat table per frame step, index = clip*n_mbs + mb,
//      so a wave's first load already tells it everything it needs to start fetching pixels ------------
// w0  payload word offset (host: inside the clip's payload; device: inside the frame step's payload arena)
// w1  [0]      type (MOBI_MB_*)
//     [7:1]    n_leaves   (inter: 1 = the single 16x16 leaf; 2 with a DUAL kind = both halves; both kinds ride in the
//                          descriptor as LEAF RECORDS, see below; otherwise the payload starts with the 64-word MV cell map)
//     [13:8]   cbp6       coded 8x8 areas: bits 0-3 luma TL,TR,BL,BR; 4 U; 5 V   (MD.cs:1820-1832)
//     [19:14]  t8mask     coded area uses ONE 8x8 transform (else four 4x4s)      (MD.cs:2911)
//     [25:20]  quantizer  of the frame (selects the dequant scale table, MD.cs:3884-3912)
//     [27:26]  MOBI_DUAL_*: the macroblock is exactly two halves (partition codes 8 / 9 at the 16x16 level with two
//              plain leaves, MD.cs:585-600 -- by far the most common split), leaf A = top / left, B = bottom / right
//     [28]     reserved (r02: "right neighbour is intra", for the edge side buffer the tiled planes made unnecessary)
// w2  [9:0]    n_coefs (<= 384)
//     inter leaf records, decoded by the host so that the kernel does no motion-vector arithmetic (MD.cs:400-416):
//     [12:10] ref slot 1..5 of leaf A   [15:13] of leaf B
//     [17:16] luma CopyBlock phase (dx&1)|((dy&1)<<1) of A   [19:18] chroma phase of A   [21:20], [23:22] the same for B
// w3  inter: luma source position of leaf A = MB offset + (dy>>1)*Stride + (dx>>1), linear inside the reference's Y plane
//            (signed: a bottom/right half may point above/left of its macroblock's origin; its own rows/columns add back)
//     intra: [0] plane16 present, [1] some dependency (w4..w7) is an intra macroblock, [2] some intra macroblock depends on this one,
//            [4] the plane16 parameter does not fit [31:16]: it is wide parameter 24 (below), [31:16] plane16 parameter
// w4  inter: chroma source position of leaf A = MB offset/2 + ((dy>>1)>>1)*Stride + ((dx>>1)>>1), inside the UV plane (U half)
// w5, w6  inter DUAL: the same two positions for leaf B
// w7  reserved (0) for inter macroblocks
// intra: w4..w7 hold up to 8 uint16 macroblock indices (MOBI_DEP_NONE = unused): the raster-earlier macroblocks of the
//        same frame, inter or intra, whose pixels this one's prediction halo reads.  When a frame step runs as one
//        launch the macroblock waits for exactly these (mobi_recon_step in mobi_kernels.hip).
struct MbDesc {
  uint32_t payload_off;
  uint32_t w1;
  uint32_t w2;
  uint32_t w3;
  uint32_t w4;
  uint32_t w5;
  uint32_t w6;
  uint32_t w7;
};
enum { MOBI_DUAL_NONE = 0, MOBI_DUAL_TB = 1, MOBI_DUAL_LR = 2 }; // two 16x8 (top, bottom) / two 8x16 (left, right)
#define MOBI_MV_CELLS 64
#define MOBI_INTRA_RECORDS 24

enum { MOBI_W1_TYPE_S = 0, MOBI_W1_TYPE_N = 1, MOBI_W1_LEAVES_S = 1, MOBI_W1_LEAVES_N = 7, MOBI_W1_CBP_S = 8, MOBI_W1_CBP_N = 6,
       MOBI_W1_T8_S = 14, MOBI_W1_T8_N = 6, MOBI_W1_QUANT_S = 20, MOBI_W1_QUANT_N = 6, MOBI_W1_DUAL_S = 26, MOBI_W1_DUAL_N = 2 };
MOBI_CMD_FN uint32_t mobi_desc_w1(int type, uint32_t n_leaves, uint32_t cbp6, uint32_t t8mask, uint32_t quant, int dual) {
  return (uint32_t)type | (n_leaves << MOBI_W1_LEAVES_S) | (cbp6 << MOBI_W1_CBP_S) | (t8mask << MOBI_W1_T8_S) | MOBI_PUT(quant, MOBI_W1_QUANT) |
         ((uint32_t)dual << MOBI_W1_DUAL_S);
}
MOBI_CMD_FN uint32_t mobi_w1_type(uint32_t w1) { return w1 & MOBI_MASK(MOBI_W1_TYPE); }
MOBI_CMD_FN bool mobi_w1_intra(uint32_t w1) { return mobi_w1_type(w1) == MOBI_MB_INTRA; }
MOBI_CMD_FN uint32_t mobi_w1_leaves(uint32_t w1) { return MOBI_GET(w1, MOBI_W1_LEAVES); }
MOBI_CMD_FN uint32_t mobi_w1_cbp6(uint32_t w1) { return MOBI_GET(w1, MOBI_W1_CBP); }
MOBI_CMD_FN uint32_t mobi_w1_t8mask(uint32_t w1) { return MOBI_GET(w1, MOBI_W1_T8); }
MOBI_CMD_FN uint32_t mobi_w1_quant(uint32_t w1) { return MOBI_GET(w1, MOBI_W1_QUANT); }
MOBI_CMD_FN uint32_t mobi_w1_dual(uint32_t w1) { return MOBI_GET(w1, MOBI_W1_DUAL); }
MOBI_CMD_FN bool mobi_w1_area_coded(uint32_t w1, int area) { return ((w1 >> (MOBI_W1_CBP_S + area)) & 1) != 0; }
MOBI_CMD_FN bool mobi_w1_area_is8(uint32_t w1, int area) { return ((w1 >> (MOBI_W1_T8_S + area)) & 1) != 0; } // one 8x8 transform
MOBI_CMD_FN uint32_t mobi_w1_with_quant(uint32_t w1, uint32_t quant) { return (w1 & ~MOBI_MASK_AT(MOBI_W1_QUANT)) | MOBI_PUT(quant, MOBI_W1_QUANT); }
// what an inter macroblock's payload starts with: nothing when its one or two leaves ride in the descriptor, else the MV cell map
MOBI_CMD_FN uint32_t mobi_inter_hdr_words(uint32_t n_leaves, int dual) { return (n_leaves > 1 && !dual) ? MOBI_MV_CELLS : 0; }
// where a macroblock's level words start inside its payload
MOBI_CMD_FN uint32_t mobi_levels_offset(uint32_t w1) {
  return mobi_w1_intra(w1) ? MOBI_INTRA_RECORDS : mobi_inter_hdr_words(mobi_w1_leaves(w1), (int)mobi_w1_dual(w1));
}

// w2: the leaf records of leaf i (0: A, 1: B) sit MOBI_W2_REF_STEP resp. MOBI_W2_PH_STEP bits behind leaf A's
enum { MOBI_W2_COEFS_S = 0, MOBI_W2_COEFS_N = 10, MOBI_W2_REFA_S = 10, MOBI_W2_REFA_N = 3, MOBI_W2_REFB_S = 13, MOBI_W2_REFB_N = 3,
       MOBI_W2_PHA_S = 16, MOBI_W2_PHA_N = 2, MOBI_W2_CPHA_S = 18, MOBI_W2_CPHA_N = 2, MOBI_W2_PHB_S = 20, MOBI_W2_PHB_N = 2,
       MOBI_W2_CPHB_S = 22, MOBI_W2_CPHB_N = 2,
       MOBI_W2_REF_STEP = MOBI_W2_REFB_S - MOBI_W2_REFA_S, MOBI_W2_PH_STEP = MOBI_W2_PHB_S - MOBI_W2_PHA_S };
static_assert(MOBI_W2_CPHB_S - MOBI_W2_CPHA_S == MOBI_W2_PH_STEP, "leaf B's phases: one step behind leaf A's");
MOBI_CMD_FN uint32_t mobi_w2_coefs(uint32_t w2) { return MOBI_GET(w2, MOBI_W2_COEFS); }
MOBI_CMD_FN uint32_t mobi_w2_leaf(int i, uint32_t ref, uint32_t phase, uint32_t cphase) {
  return (ref << (MOBI_W2_REFA_S + MOBI_W2_REF_STEP * i)) | (phase << (MOBI_W2_PHA_S + MOBI_W2_PH_STEP * i)) | (cphase << (MOBI_W2_CPHA_S + MOBI_W2_PH_STEP * i));
}
MOBI_CMD_FN uint32_t mobi_w2_ref(uint32_t w2, int i) { return (w2 >> (MOBI_W2_REFA_S + MOBI_W2_REF_STEP * i)) & MOBI_MASK(MOBI_W2_REFA); }
MOBI_CMD_FN uint32_t mobi_w2_phase(uint32_t w2, int i) { return (w2 >> (MOBI_W2_PHA_S + MOBI_W2_PH_STEP * i)) & MOBI_MASK(MOBI_W2_PHA); }
MOBI_CMD_FN uint32_t mobi_w2_cphase(uint32_t w2, int i) { return (w2 >> (MOBI_W2_CPHA_S + MOBI_W2_PH_STEP * i)) & MOBI_MASK(MOBI_W2_CPHA); }

// w3 of an intra macroblock.  The two dependency bits are set where the dependency lists are made (mobi_syntax.h: mobi_dep_add's callers)
enum { MOBI_W3_PARAM_S = 16, MOBI_W3_PARAM_N = 16 };
#define MOBI_W3_PLANE16 0x1u
#define MOBI_W3_HAS_INTRA_DEPS 0x2u
#define MOBI_W3_HAS_DEPENDENTS 0x4u
#define MOBI_W3_WIDE 0x10u
// a 16x16 plane whose parameter fits int16 / is wide parameter MOBI_WIDE_PLANE16
MOBI_CMD_FN uint32_t mobi_w3_plane16(int param) { return MOBI_W3_PLANE16 | MOBI_PUT(param, MOBI_W3_PARAM); }
MOBI_CMD_FN uint32_t mobi_w3_plane16_wide() { return MOBI_W3_PLANE16 | MOBI_W3_WIDE; }
MOBI_CMD_FN bool mobi_w3_has_plane16(uint32_t w3) { return (w3 & MOBI_W3_PLANE16) != 0; }
MOBI_CMD_FN bool mobi_w3_wide(uint32_t w3) { return (w3 & MOBI_W3_WIDE) != 0; }
MOBI_CMD_FN int mobi_w3_param(uint32_t w3) { return (int)(int16_t)(w3 >> MOBI_W3_PARAM_S); }

// dependency index (a uint16 half of w4..w7)
#define MOBI_DEP_NONE 0xFFFFu
#define MOBI_DEP_INTER 0x8000u /* flag on a dependency index: that macroblock is an inter one */
#define MOBI_INTRA_DEPS 8
enum { MOBI_DEP_S = 0, MOBI_DEP_N = 16, MOBI_DEP_MB_S = 0, MOBI_DEP_MB_N = 13 }; // the whole index (two to a word); the macroblock in it
MOBI_CMD_FN uint32_t mobi_dep_mb(uint32_t dep) { return dep & MOBI_MASK(MOBI_DEP_MB); }
MOBI_CMD_FN uint32_t mobi_dep_pair(uint32_t even, uint32_t odd) { return even | (odd << MOBI_DEP_N); } // dependencies 2k, 2k + 1 = one of w4..w7
MOBI_CMD_FN uint32_t mobi_dep_of_pair(uint32_t w, int odd) { return (w >> (MOBI_DEP_N * odd)) & MOBI_MASK(MOBI_DEP); }

// ---- MC leaf as the parser records it while walking the partition tree (host only) ----------------
//  w0: [3:0] x/2  [7:4] y/2  [9:8] log2(16/w)  [11:10] log2(16/h)  [14:12] ref slot 1..5
//  w1: [15:0] dx (int16, half-pel, absolute)  [31:16] dy                         (MD.cs:400-416)
enum { MOBI_LEAF_X_S = 0, MOBI_LEAF_X_N = 4, MOBI_LEAF_Y_S = 4, MOBI_LEAF_Y_N = 4, MOBI_LEAF_WI_S = 8, MOBI_LEAF_WI_N = 2,
       MOBI_LEAF_HI_S = 10, MOBI_LEAF_HI_N = 2, MOBI_LEAF_REF_S = 12, MOBI_LEAF_REF_N = 3, MOBI_LEAF_DX_S = 0, MOBI_LEAF_DX_N = 16,
       MOBI_LEAF_DY_S = 16, MOBI_LEAF_DY_N = 16 };
MOBI_CMD_FN uint32_t mobi_leaf_w0(int x, int y, int wi, int hi, int ref) {
  return (uint32_t)((x >> 1) | ((y >> 1) << MOBI_LEAF_Y_S) | (wi << MOBI_LEAF_WI_S) | (hi << MOBI_LEAF_HI_S) | (ref << MOBI_LEAF_REF_S));
}
MOBI_CMD_FN uint32_t mobi_leaf_w1(int dx, int dy) { return ((uint32_t)dx & MOBI_MASK(MOBI_LEAF_DX)) | ((uint32_t)dy << MOBI_LEAF_DY_S); }
MOBI_CMD_FN int mobi_leaf_x(uint32_t w0) { return (int)MOBI_GET(w0, MOBI_LEAF_X) * 2; }
MOBI_CMD_FN int mobi_leaf_y(uint32_t w0) { return (int)MOBI_GET(w0, MOBI_LEAF_Y) * 2; }
MOBI_CMD_FN int mobi_leaf_wi(uint32_t w0) { return (int)MOBI_GET(w0, MOBI_LEAF_WI); }
MOBI_CMD_FN int mobi_leaf_hi(uint32_t w0) { return (int)MOBI_GET(w0, MOBI_LEAF_HI); }
MOBI_CMD_FN int mobi_leaf_ref(uint32_t w0) { return (int)MOBI_GET(w0, MOBI_LEAF_REF); }
MOBI_CMD_FN uint32_t mobi_leaf_shape(uint32_t w0) { return w0 & ((1u << MOBI_LEAF_REF_S) - 1u); } // x, y, wi, hi: everything below the ref slot
MOBI_CMD_FN int mobi_leaf_dx(uint32_t w1) { return (int16_t)(w1 & MOBI_MASK(MOBI_LEAF_DX)); }
MOBI_CMD_FN int mobi_leaf_dy(uint32_t w1) { return (int16_t)(w1 >> MOBI_LEAF_DY_S); }

// ---- MV cell map (macroblocks with more than one leaf that are not DUAL): 64 words, first thing in the payload ---
// The partition tree bottoms out at 2x2 luma (MD.cs:1683-1746), so an 8x8 grid of 2x2-pixel cells
// (= one chroma sample each) says for every pixel which leaf moved it.  cell[(y/2)*8 + x/2] =
//  [13:0] dx (signed 14)  [27:14] dy (signed 14)  [30:28] ref slot 1..5
// Every lane fetches the cells under its own pixels, so all reference reads of a macroblock are in
// flight together, however deep the tree was.
#define MOBI_MV_LIMIT 8191
enum { MOBI_CELL_DX_S = 0, MOBI_CELL_DX_N = 14, MOBI_CELL_DY_S = 14, MOBI_CELL_DY_N = 14, MOBI_CELL_REF_S = 28, MOBI_CELL_REF_N = 3 };
static_assert(MOBI_MV_LIMIT == (1 << (MOBI_CELL_DX_N - 1)) - 1, "the vectors a cell can hold");
MOBI_CMD_FN uint32_t mobi_cell(int dx, int dy, int ref) {
  return ((uint32_t)dx & MOBI_MASK(MOBI_CELL_DX)) | (((uint32_t)dy & MOBI_MASK(MOBI_CELL_DY)) << MOBI_CELL_DY_S) | ((uint32_t)ref << MOBI_CELL_REF_S);
}
MOBI_CMD_FN int mobi_cell_dx(uint32_t c) { return (int)(c << (32 - MOBI_CELL_DX_S - MOBI_CELL_DX_N)) >> (32 - MOBI_CELL_DX_N); }
MOBI_CMD_FN int mobi_cell_dy(uint32_t c) { return (int)(c << (32 - MOBI_CELL_DY_S - MOBI_CELL_DY_N)) >> (32 - MOBI_CELL_DY_N); }
MOBI_CMD_FN int mobi_cell_ref(uint32_t c) { return (int)(c >> MOBI_CELL_REF_S) & (int)MOBI_MASK(MOBI_CELL_REF); }

// ---- residual level: one word ---------------------------------------------------------------
//  [8:0]   tile position = area*64 + p, area = 0..5 (Y0..Y3,U,V)
//            8x8 transform:  p = natural-order coefficient index (MD.cs:3426 zigzag target)
//            4x4 transforms: p = sub*16 + natural index inside that 4x4 (sub = 0..3: TL,TR,BL,BR)
//  [15]    host parser only, never shipped: the upper half is a coefficient VALUE already (mobi_parse.cpp, literal_frame clears it)
//  [31:16] level (int16); the GPU multiplies by the dequant scale (MD.cs:3427-3429)
enum { MOBI_LEVEL_POS_S = 0, MOBI_LEVEL_POS_N = 9, MOBI_LEVEL_P_S = 0, MOBI_LEVEL_P_N = 6, MOBI_LEVEL_AREA_S = 6, MOBI_LEVEL_AREA_N = 3,
       MOBI_LEVEL_P4_S = 0, MOBI_LEVEL_P4_N = 4, MOBI_LEVEL_SUB_S = 4, MOBI_LEVEL_SUB_N = 2, // p of a 4x4 area: index inside the block, block
       MOBI_LEVEL_VALUE_S = 16, MOBI_LEVEL_VALUE_N = 16 };
#define MOBI_LEVEL_IS_VALUE 0x8000u
MOBI_CMD_FN uint32_t mobi_level_word(int pos, int level) { return (uint32_t)pos | ((uint32_t)level << MOBI_LEVEL_VALUE_S); }
MOBI_CMD_FN uint32_t mobi_coef(int area, int p, int level) { return mobi_level_word(area * (1 << MOBI_LEVEL_AREA_S) + p, level); }
MOBI_CMD_FN uint32_t mobi_level_pos(uint32_t e) { return e & MOBI_MASK(MOBI_LEVEL_POS); }
MOBI_CMD_FN uint32_t mobi_level_area(uint32_t e) { return MOBI_GET(e, MOBI_LEVEL_AREA); }
MOBI_CMD_FN int mobi_level_value(uint32_t e) { return (int32_t)e >> MOBI_LEVEL_VALUE_S; }
// ... of a tile position (mobi_level_pos), in the caller's integer type
template <class T> MOBI_CMD_FN T mobi_pos_area(T pos) { return pos >> MOBI_LEVEL_AREA_S; }
template <class T> MOBI_CMD_FN T mobi_pos_p(T pos) { return pos & (T)MOBI_MASK(MOBI_LEVEL_P); }
template <class T> MOBI_CMD_FN T mobi_pos_p4(T pos) { return pos & (T)MOBI_MASK(MOBI_LEVEL_P4); }
template <class T> MOBI_CMD_FN T mobi_pos_sub(T pos) { return (pos >> MOBI_LEVEL_SUB_S) & (T)MOBI_MASK(MOBI_LEVEL_SUB); }

// ---- intra MB payload: 24 block records (6 areas x 4) then the levels ------------------------
// record for area a, slot s (s = 0 only when the area is predicted as one 8x8):
//  [3:0]  mode 0..9 (8x8 numbering; 4x4 blocks use the same numbering, MD.cs mode-10)
//  [4]    residual coded for this block
//  [5]    split: the area is four 4x4 blocks (slots 0..3 all valid)
//  [6]    slot 0 of U / V with mode 9: run the 8x8 plane with this record's parameter before this area (keeps decode order)
//  [7]    the plane parameter does not fit int16 (a code of 33 bits and more): it is WIDE PARAMETER r, r = this record's index
//  [31:16] plane parameter (int16) when mode == 2 or bit 6 is set                (MD.cs:3019,3170,3255)
// Wide parameters (r05): MOBI_WIDE_PARAMS words behind the macroblock's level words -- payload word MOBI_INTRA_RECORDS + n_coefs + r, r = the
// record's index, MOBI_WIDE_PLANE16 = the 16x16 plane's -- present only when some record or MbDesc.w3 says so.  The plane predictors compute in
// int32 and OR their samples into words (MD.cs:3055-3062): every bit of the parameter reaches the picture.
#define MOBI_WIDE_PARAMS 25
#define MOBI_WIDE_PLANE16 24
enum { MOBI_REC_MODE_S = 0, MOBI_REC_MODE_N = 4, MOBI_REC_CODED_S = 4, MOBI_REC_CODED_N = 1, MOBI_REC_SPLIT_S = 5, MOBI_REC_SPLIT_N = 1,
       MOBI_REC_PRE_S = 6, MOBI_REC_PRE_N = 1, MOBI_REC_WIDE_S = 7, MOBI_REC_WIDE_N = 1, MOBI_REC_PARAM_S = 16, MOBI_REC_PARAM_N = 16 };
#define MOBI_REC_WIDE (1u << MOBI_REC_WIDE_S)
MOBI_CMD_FN uint32_t mobi_intra_rec(int mode, int coded, int split, int pre_plane, int param) {
  return (uint32_t)(mode | (coded << MOBI_REC_CODED_S) | (split << MOBI_REC_SPLIT_S) | (pre_plane << MOBI_REC_PRE_S)) | ((uint32_t)param << MOBI_REC_PARAM_S);
}
MOBI_CMD_FN uint32_t mobi_rec_param_bits(int param) { return MOBI_PUT(param, MOBI_REC_PARAM); } // an int16 parameter, to OR into a record
MOBI_CMD_FN int mobi_rec_mode(uint32_t r) { return (int)(r & MOBI_MASK(MOBI_REC_MODE)); }
MOBI_CMD_FN bool mobi_rec_coded(uint32_t r) { return MOBI_GET(r, MOBI_REC_CODED); }
MOBI_CMD_FN bool mobi_rec_split(uint32_t r) { return MOBI_GET(r, MOBI_REC_SPLIT); }
MOBI_CMD_FN bool mobi_rec_pre_plane(uint32_t r) { return MOBI_GET(r, MOBI_REC_PRE); }
MOBI_CMD_FN bool mobi_rec_wide(uint32_t r) { return (r & MOBI_REC_WIDE) != 0; }
MOBI_CMD_FN int mobi_rec_param(uint32_t r) { return (int)(int16_t)(r >> MOBI_REC_PARAM_S); }

// ---- intra launch item: 16 bytes per intra macroblock (MOBI_INTRA_ITEM_WORDS words), what a row of mobi_recon_intra's lanes starts from ----
//  word 0  [12:0] macroblock, [31:13] clip (the device parsers' per-clip lists are this word alone); MOBI_ITEM_NONE = padding: every
//          dependency level starts on a wave of four items
//  word 1  MbDesc.w1        word 2  MbDesc.payload_off (inside the step's arena)
//  word 3  MbDesc.w3's plane16 bits where w3 has them ([0] present, [4] wide, [31:16] parameter), and
//          [1] has intra dependencies: poll their tags   [2] has intra dependents: publish its own   (MOBI_W3_HAS_*, same places)
//          [3] host only: the macroblock's launch class is an edge one (mobi_parse.cpp, finish_levels); LevelPlan (mobi_batch.h) strips it
//          [14:5] number of level words (MbDesc.w2's)
#define MOBI_INTRA_ITEM_WORDS 4
#define MOBI_ITEM_NONE 0xFFFFFFFFu
enum { MOBI_ITEM_MB_S = 0, MOBI_ITEM_MB_N = 13, MOBI_ITEM_CLIP_S = 13, MOBI_ITEM_CLIP_N = 19, MOBI_ITEM_COEFS_S = 5, MOBI_ITEM_COEFS_N = 10 };
static_assert((int)MOBI_ITEM_MB_N == (int)MOBI_DEP_MB_N, "a dependency names a macroblock as an item does");
#define MOBI_ITEM(clip, mb) (((uint32_t)(clip) << MOBI_ITEM_CLIP_S) | (uint32_t)(mb))
#define MOBI_ITEM_MB(item) ((item) & MOBI_MASK(MOBI_ITEM_MB))
MOBI_CMD_FN uint32_t mobi_item_clip(uint32_t item) { return item >> MOBI_ITEM_CLIP_S; }
#define MOBI_ITEM_EDGE 0x8u
#define MOBI_ITEM_W3_BITS (MOBI_W3_PLANE16 | MOBI_W3_WIDE | MOBI_MASK_AT(MOBI_W3_PARAM))
#define MOBI_ITEM_DEP_BITS (MOBI_W3_HAS_INTRA_DEPS | MOBI_W3_HAS_DEPENDENTS)
// from the macroblock's finished descriptor: w3 with its dependency bits set, w2.  (The host parser ORs MOBI_ITEM_EDGE in.  A macro, as
// MOBI_ITEM is: as a function its arguments are read before either is masked, and mobi_gop_scatter's instructions come out in another order.)
#define MOBI_ITEM_FLAGS(w3, w2) ((uint32_t)(((w3) & (MOBI_ITEM_W3_BITS | MOBI_ITEM_DEP_BITS)) | (mobi_w2_coefs(w2) << MOBI_ITEM_COEFS_S)))
MOBI_CMD_FN uint32_t mobi_item_w3(uint32_t flags) { return flags & MOBI_ITEM_W3_BITS; } // what the kernel needs of MbDesc.w3
MOBI_CMD_FN uint32_t mobi_item_coefs(uint32_t flags) { return MOBI_GET(flags, MOBI_ITEM_COEFS); }
MOBI_CMD_FN bool mobi_item_has_deps(uint32_t flags) { return (flags & MOBI_W3_HAS_INTRA_DEPS) != 0; }
MOBI_CMD_FN bool mobi_item_publishes(uint32_t flags) { return (flags & MOBI_W3_HAS_DEPENDENTS) != 0; }
MOBI_CMD_FN uint32_t mobi_item_shipped(uint32_t flags) { return flags & ~MOBI_ITEM_EDGE; }

// ---- the header checks itself: no two fields of a word overlap (disjoint masks add up to their union), and what a writer packs its
//      readers give back ----
MOBI_CMD_FN bool mobi_disjoint(const uint32_t *m, int n) {
  uint64_t sum = 0;
  uint32_t all = 0;
  for (int i = 0; i < n; i++) { sum += m[i]; all |= m[i]; }
  return sum == all;
}
#define MOBI_ASSERT_DISJOINT(name, ...) \
  namespace mobi_cmd_check { constexpr uint32_t name[] = {__VA_ARGS__}; \
  static_assert(mobi_disjoint(name, (int)(sizeof(name) / sizeof(name[0]))), #name ": fields overlap"); }
MOBI_ASSERT_DISJOINT(w1, MOBI_MASK_AT(MOBI_W1_TYPE), MOBI_MASK_AT(MOBI_W1_LEAVES), MOBI_MASK_AT(MOBI_W1_CBP), MOBI_MASK_AT(MOBI_W1_T8),
                     MOBI_MASK_AT(MOBI_W1_QUANT), MOBI_MASK_AT(MOBI_W1_DUAL))
MOBI_ASSERT_DISJOINT(w2, MOBI_MASK_AT(MOBI_W2_COEFS), MOBI_MASK_AT(MOBI_W2_REFA), MOBI_MASK_AT(MOBI_W2_REFB), MOBI_MASK_AT(MOBI_W2_PHA),
                     MOBI_MASK_AT(MOBI_W2_CPHA), MOBI_MASK_AT(MOBI_W2_PHB), MOBI_MASK_AT(MOBI_W2_CPHB))
MOBI_ASSERT_DISJOINT(w3_intra, MOBI_W3_PLANE16, MOBI_W3_HAS_INTRA_DEPS, MOBI_W3_HAS_DEPENDENTS, MOBI_W3_WIDE, MOBI_MASK_AT(MOBI_W3_PARAM))
MOBI_ASSERT_DISJOINT(dep, MOBI_MASK_AT(MOBI_DEP_MB), MOBI_DEP_INTER)
MOBI_ASSERT_DISJOINT(leaf_w0, MOBI_MASK_AT(MOBI_LEAF_X), MOBI_MASK_AT(MOBI_LEAF_Y), MOBI_MASK_AT(MOBI_LEAF_WI), MOBI_MASK_AT(MOBI_LEAF_HI), MOBI_MASK_AT(MOBI_LEAF_REF))
MOBI_ASSERT_DISJOINT(leaf_w1, MOBI_MASK_AT(MOBI_LEAF_DX), MOBI_MASK_AT(MOBI_LEAF_DY))
MOBI_ASSERT_DISJOINT(cell, MOBI_MASK_AT(MOBI_CELL_DX), MOBI_MASK_AT(MOBI_CELL_DY), MOBI_MASK_AT(MOBI_CELL_REF))
MOBI_ASSERT_DISJOINT(level, MOBI_MASK_AT(MOBI_LEVEL_P), MOBI_MASK_AT(MOBI_LEVEL_AREA), MOBI_LEVEL_IS_VALUE, MOBI_MASK_AT(MOBI_LEVEL_VALUE))
MOBI_ASSERT_DISJOINT(rec, MOBI_MASK_AT(MOBI_REC_MODE), MOBI_MASK_AT(MOBI_REC_CODED), MOBI_MASK_AT(MOBI_REC_SPLIT), MOBI_MASK_AT(MOBI_REC_PRE),
                     MOBI_MASK_AT(MOBI_REC_WIDE), MOBI_MASK_AT(MOBI_REC_PARAM))
MOBI_ASSERT_DISJOINT(item_w0, MOBI_MASK_AT(MOBI_ITEM_MB), MOBI_MASK_AT(MOBI_ITEM_CLIP))
MOBI_ASSERT_DISJOINT(item_w3, MOBI_ITEM_W3_BITS, MOBI_ITEM_DEP_BITS, MOBI_ITEM_EDGE, MOBI_MASK_AT(MOBI_ITEM_COEFS))
static_assert(MOBI_MASK_AT(MOBI_LEVEL_POS) == (MOBI_MASK_AT(MOBI_LEVEL_P) | MOBI_MASK_AT(MOBI_LEVEL_AREA)) && 6 * 64 <= (1 << MOBI_LEVEL_POS_N) && 6 * 64 <= (1 << MOBI_W2_COEFS_N),
              "a tile position is area * 64 + p; six areas of 64 levels");
namespace mobi_cmd_check {
constexpr uint32_t W1 = mobi_desc_w1(MOBI_MB_INTRA, 0x55, 0x2A, 0x15, 53, MOBI_DUAL_LR);
static_assert(mobi_w1_type(W1) == MOBI_MB_INTRA && mobi_w1_intra(W1) && mobi_w1_leaves(W1) == 0x55 && mobi_w1_cbp6(W1) == 0x2A && mobi_w1_t8mask(W1) == 0x15 &&
              mobi_w1_quant(W1) == 53 && mobi_w1_dual(W1) == MOBI_DUAL_LR, "w1 round trip");
static_assert(mobi_w1_area_coded(W1, 1) && !mobi_w1_area_coded(W1, 0) && mobi_w1_area_is8(W1, 0) && !mobi_w1_area_is8(W1, 1), "w1 per-area bits");
static_assert(mobi_w1_quant(mobi_w1_with_quant(W1, 63)) == 63 && (mobi_w1_with_quant(W1, 63) ^ W1) == ((53u ^ 63u) << MOBI_W1_QUANT_S), "w1 quantiser patch");
static_assert(mobi_levels_offset(W1) == MOBI_INTRA_RECORDS && mobi_levels_offset(mobi_desc_w1(MOBI_MB_INTER, 2, 0, 0, 0, MOBI_DUAL_TB)) == 0 &&
              mobi_levels_offset(mobi_desc_w1(MOBI_MB_INTER, 3, 0, 0, 0, MOBI_DUAL_NONE)) == MOBI_MV_CELLS, "where the levels start");
constexpr uint32_t W2 = 383u | mobi_w2_leaf(0, 5, 1, 2) | mobi_w2_leaf(1, 3, 3, 1);
static_assert(mobi_w2_coefs(W2) == 383 && mobi_w2_ref(W2, 0) == 5 && mobi_w2_phase(W2, 0) == 1 && mobi_w2_cphase(W2, 0) == 2 && mobi_w2_ref(W2, 1) == 3 &&
              mobi_w2_phase(W2, 1) == 3 && mobi_w2_cphase(W2, 1) == 1, "w2 round trip");
static_assert(MOBI_GET(W2, MOBI_W2_REFB) == 3 && MOBI_GET(W2, MOBI_W2_PHB) == 3 && MOBI_GET(W2, MOBI_W2_CPHB) == 1, "leaf B's named fields");
static_assert(mobi_w3_has_plane16(mobi_w3_plane16(-1234)) && !mobi_w3_wide(mobi_w3_plane16(-1234)) && mobi_w3_param(mobi_w3_plane16(-1234)) == -1234 &&
              mobi_w3_wide(mobi_w3_plane16_wide()) && mobi_w3_has_plane16(mobi_w3_plane16_wide()), "w3 round trip");
static_assert(mobi_dep_mb(8100u | MOBI_DEP_INTER) == 8100 && mobi_dep_of_pair(mobi_dep_pair(17u | MOBI_DEP_INTER, MOBI_DEP_NONE), 0) == (17u | MOBI_DEP_INTER) &&
              mobi_dep_of_pair(mobi_dep_pair(17u, 8191u), 1) == 8191u, "dependency round trip");
constexpr uint32_t L0 = mobi_leaf_w0(14, 6, 3, 1, 5), L1 = mobi_leaf_w1(-300, 77);
static_assert(mobi_leaf_x(L0) == 14 && mobi_leaf_y(L0) == 6 && mobi_leaf_wi(L0) == 3 && mobi_leaf_hi(L0) == 1 && mobi_leaf_ref(L0) == 5 &&
              mobi_leaf_shape(L0) == mobi_leaf_w0(14, 6, 3, 1, 0) && mobi_leaf_dx(L1) == -300 && mobi_leaf_dy(L1) == 77, "leaf round trip");
constexpr uint32_t C = mobi_cell(-MOBI_MV_LIMIT, MOBI_MV_LIMIT, 5);
static_assert(mobi_cell_dx(C) == -MOBI_MV_LIMIT && mobi_cell_dy(C) == MOBI_MV_LIMIT && mobi_cell_ref(C) == 5, "cell round trip");
constexpr uint32_t E = mobi_coef(5, 63, -32768);
static_assert(mobi_level_pos(E) == 5 * 64 + 63 && mobi_level_area(E) == 5 && mobi_pos_area(5 * 64 + 63) == 5 && mobi_pos_p(5 * 64 + 63) == 63 &&
              mobi_pos_p4(63) == 15 && mobi_pos_sub(63) == 3 && mobi_level_value(E) == -32768 && !(E & MOBI_LEVEL_IS_VALUE) && mobi_level_word(383, 7) == mobi_coef(5, 63, 7), "level word round trip");
constexpr uint32_t R = mobi_intra_rec(9, 1, 0, 1, -2);
static_assert(mobi_rec_mode(R) == 9 && mobi_rec_coded(R) && !mobi_rec_split(R) && mobi_rec_pre_plane(R) && !mobi_rec_wide(R) && mobi_rec_param(R) == -2 &&
              mobi_rec_split(mobi_intra_rec(2, 0, 1, 0, 0)) && mobi_rec_wide(mobi_intra_rec(2, 0, 0, 0, 0) | MOBI_REC_WIDE) &&
              (mobi_intra_rec(2, 0, 0, 0, 0) | mobi_rec_param_bits(-2)) == mobi_intra_rec(2, 0, 0, 0, -2), "block record round trip");
static_assert(MOBI_ITEM_MB(MOBI_ITEM(24575, 8100)) == 8100 && mobi_item_clip(MOBI_ITEM(24575, 8100)) == 24575 && MOBI_ITEM(24575, 8100) != MOBI_ITEM_NONE, "item word 0 round trip");
constexpr uint32_t F = MOBI_ITEM_FLAGS(mobi_w3_plane16(-7) | MOBI_W3_HAS_DEPENDENTS, W2) | MOBI_ITEM_EDGE;
static_assert(mobi_item_w3(F) == mobi_w3_plane16(-7) && mobi_item_coefs(F) == 383 && !mobi_item_has_deps(F) && mobi_item_publishes(F) && (F & MOBI_ITEM_EDGE) &&
              !(mobi_item_shipped(F) & MOBI_ITEM_EDGE) && (mobi_item_shipped(F) | MOBI_ITEM_EDGE) == F &&
              mobi_item_has_deps(MOBI_ITEM_FLAGS(MOBI_W3_HAS_INTRA_DEPS, 0)) && mobi_item_w3(MOBI_ITEM_FLAGS(mobi_w3_plane16_wide(), 0)) == mobi_w3_plane16_wide(),
              "item flags round trip");
} // namespace mobi_cmd_check

// ---- per-frame info kept on the host (launch planning, accounting); the kernels never read it ----------
struct FrameHdr {
  uint32_t frame_type;   // 0 = P, 1 = I
  uint32_t n_mbs;
  uint32_t n_intra;      // number of intra MBs
  uint32_t n_levels;     // highest intra dependency level (0 when no intra MBs)
  uint32_t payload_words;
  uint32_t quantizer;
  uint32_t cmd_bytes;    // bytes of this frame's command list the kernels read (desc + payload)
  uint32_t reserved;
};

// Dequant scale tables by NATURAL coefficient index for one quantizer: scale = dequant word >> 8
// (MD.cs:3897-3911; 4x4: tbl<<(q/6), 8x8: tbl<<(q/6-2)).  Valid for q in [12,53] (no zigzag-byte leak).
// Layout of one entry of the device table: int[80] = scale8[64] then scale4[16].
#define MOBI_SCALE_STRIDE 80
#define MOBI_SCALE_QMAX 54
// Intra tap table (mobi_build_intra_taps): behind the 64 rows of scale tables in the same device buffer.  Entry = 4 x int16 tile
// offsets; 8x8 blocks: entry mi * 64 + y * 8 + x, 4x4 blocks: MOBI_TAP_4X4 + mi * 16 + y * 4 + x, mi = mode < 2 ? mode : mode - 2
#define MOBI_TAP_MODES 7
#define MOBI_TAP_4X4 (MOBI_TAP_MODES * 64)
#define MOBI_TAP_ENTRIES (MOBI_TAP_MODES * 80)
#define MOBI_TAP_PITCH 32 /* the intra kernel's tile pitch */
#define MOBI_SCALE_ROWS 64
#define MOBI_SCALE_LITERAL 63 /* the row of ones: MbDesc.w1's quantiser field of a frame whose residual words carry coefficient VALUES
                                 (the host parser's Internal[] walk, mobi_parse.cpp); no real quantiser reaches 54 (MD.cs:3864-3880) */
#define MOBI_TQ_NONE 62      /* a row of zeros: MbDesc.w1's field while SetupQuantizationTables has never run -- every dequant word is 0
                                 (MD.cs:28: a fresh Internal[]), so every coefficient is.  The field is the quantiser the TABLES were built for,
                                 which is not Quantizer after a SetupQuantizationTables that threw (MD.cs:3886-3890; ModsDS, q >= 54) */

#endif
