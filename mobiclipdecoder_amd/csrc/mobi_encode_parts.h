// mobi_encode_parts.h -- the inter encoder's partition mode (include/mobiclip_encode_parts.h; DESIGN.md, "Inter encoder", "Partitions"): the
// rules that the kernels (mobi_encode_parts.hip), the host entry points (mobi_encode_inter.cpp), the host model
// (tests/tools/mobi_encode_parts_host.cpp) and the CPU tests compile alike.  Key, candidate steps, predictor, block rule, symbol writer and
// sinks are mobi_encode_inter.h's and mobi_encode.h's; nothing is copied.
//
//   leaves          nine candidates per macroblock: the 16x16 (shape s = 4 wi + hi = 0), top / bottom 16x8 (1), left / right 8x16 (4), the
//                   quadrants Q0..Q3 in raster order (5); one reference; a leaf is sent with code 0 or 1 at its own shape
//   candidates      mobi_encq_leaf_ok: the leaf's luma window and its two (w / 2) x (h / 2) chroma windows inside the picture rectangle; at
//                   16x16 it is mobi_encp_vector_ok
//   search          per leaf the two steps and the key of mobi_encode_inter.h, the SAD taken over the leaf
//   tree            bottom-up minimum of J = C + lam * bits with every leaf priced as code 1 (mobi_encq_decide); ties: unsplit, then code 8;
//                   inside a half the leaf before the split
//   syntax          every leaf against the macroblock's predictor, the median of the neighbours' LAST leaves (bottom-right quadrants: kept in
//                   the mv array, so that mobi_encp_predictor serves); the tree's codes in pblock's order, then ue(cbp) and the blocks
//   prediction      luma block k with Qk's vector; a chroma block's four 4x4 quadrants with the chroma vectors of Q0..Q3
#ifndef MOBI_ENCODE_PARTS_H
#define MOBI_ENCODE_PARTS_H
#include "../../include/mobiclip_encode_parts.h"
#include "mobi_encode_inter.h"
#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif

enum { MOBI_ENCQ_LEAVES = 9,
       // the tree as one byte (MobiEncMb::luma_mode of a P-macroblock): the root in bits 0..1, bit 2 / 3 = the first / second half is split
       MOBI_ENCQ_ROOT_MASK = 3, MOBI_ENCQ_ROOT_LEAF = 0, MOBI_ENCQ_ROOT_8 = 1, MOBI_ENCQ_ROOT_9 = 2, MOBI_ENCQ_SPLIT_FIRST = 4, MOBI_ENCQ_SPLIT_SECOND = 8,
       // rows of the code tables: shapes 0, 1, 4, 5 and partition codes 0, 1, 8, 9
       MOBI_ENCQ_C8 = 2, MOBI_ENCQ_C9 = 3 };

// leaf l of the nine: 0 the 16x16; 1, 2 top, bottom; 3, 4 left, right; 5..8 Q0..Q3
struct MobiEncqLeaf {
  int x, y, w, h; // inside the macroblock
};
MOBI_TC_FN MobiEncqLeaf mobi_encq_leaf(int l) {
  MobiEncqLeaf f;
  f.w = l == 0 || l == 1 || l == 2 ? 16 : 8;
  f.h = l == 0 || l == 3 || l == 4 ? 16 : 8;
  f.x = l == 4 || l == 6 || l == 8 ? 8 : 0;
  f.y = l == 2 || l == 7 || l == 8 ? 8 : 0;
  return f;
}
MOBI_TC_FN int mobi_encq_shape_row(int l) { return l == 0 ? 0 : l <= 2 ? 1 : l <= 4 ? 2 : 3; } // the code tables' row of leaf l's shape
MOBI_TC_FN int mobi_encq_shape(int row) { return row == 0 ? 0 : row == 1 ? 1 : row == 2 ? 4 : 5; } // ... and the shape index s of a row

// ---- the candidate set of a leaf, one axis at a time: n samples at p of a plane L long, moved by d half-pels, with the sample a
// half-pel phase adds; the chroma span is n / 2 samples at p / 2 moved by d >> 1 ----
MOBI_TC_FN bool mobi_encq_span_ok(int L, int p, int n, int d) {
  const int a = p + (d >> 1), c = d >> 1, ca = p / 2 + (c >> 1);
  return a >= 0 && a + n - 1 + (d & 1) < L && ca >= 0 && ca + n / 2 - 1 + (c & 1) < L / 2;
}
// the leaf at pixel (x, y) of size w x h
MOBI_TC_FN bool mobi_encq_leaf_ok(int W, int H, int x, int y, int w, int h, int dx, int dy) {
  return mobi_encq_span_ok(W, x, w, dx) && mobi_encq_span_ok(H, y, h, dy);
}

// per-device constants: the inter encoder's, and the code words of the four shapes behind them
struct MobiEncPartsConst : MobiEncInterConst {
  uint8_t q_code[2][4][4];  // [version table][shape row][code 0, 1, 8, 9]: the code word ...
  uint8_t q_nbits[2][4][4]; // ... and its length; 0 where the shape has no such code
};

// ---- the tree decision: C[l] = the cost part of leaf l's best key.  (All-8x8 is reachable through both roots; the tables spell it no
// longer through code 8, tests/test_encode_parts_model.py::test_code_8_spells_all_8x8, so with ties to code 8 it is always spelled so.) ----
MOBI_TC_FN uint64_t mobi_encq_key_cost(uint64_t key) { return key >> 20; }
MOBI_TC_FN int mobi_encq_decide(const MobiEncPartsConst *K, int ver, int64_t lam, const uint64_t *C) {
  const uint64_t L = (uint64_t)lam;
  uint64_t J[MOBI_ENCQ_LEAVES];
  for (int l = 0; l < MOBI_ENCQ_LEAVES; l++) J[l] = C[l] + L * K->q_nbits[ver][mobi_encq_shape_row(l)][1];
  int tree[2];
  uint64_t Jroot[2];
  for (int root = 0; root < 2; root++) { // code 8: halves 1, 2 of quadrants (0, 1), (2, 3); code 9: halves 3, 4 of (0, 2), (1, 3)
    const int row = 1 + root, split = root ? MOBI_ENCQ_C8 : MOBI_ENCQ_C9;
    tree[root] = root ? MOBI_ENCQ_ROOT_9 : MOBI_ENCQ_ROOT_8;
    Jroot[root] = L * K->q_nbits[ver][0][root ? MOBI_ENCQ_C9 : MOBI_ENCQ_C8];
    for (int half = 0; half < 2; half++) {
      const int qa = root ? half : 2 * half, qb = root ? half + 2 : 2 * half + 1;
      const uint64_t whole = J[1 + 2 * root + half], parts = L * K->q_nbits[ver][row][split] + J[5 + qa] + J[5 + qb];
      if (parts < whole) tree[root] |= half ? MOBI_ENCQ_SPLIT_SECOND : MOBI_ENCQ_SPLIT_FIRST; // a tie keeps the leaf
      Jroot[root] += parts < whole ? parts : whole;
    }
  }
  if (J[0] <= Jroot[0] && J[0] <= Jroot[1]) return MOBI_ENCQ_ROOT_LEAF; // ties: unsplit, then code 8
  return Jroot[0] <= Jroot[1] ? tree[0] : tree[1];
}
// which of the nine leaves covers quadrant qd under a tree
MOBI_TC_FN int mobi_encq_leaf_of(int tree, int qd) {
  const int root = tree & MOBI_ENCQ_ROOT_MASK;
  if (root == MOBI_ENCQ_ROOT_LEAF) return 0;
  const int half = root == MOBI_ENCQ_ROOT_8 ? qd >> 1 : qd & 1;
  if (tree & (half ? MOBI_ENCQ_SPLIT_SECOND : MOBI_ENCQ_SPLIT_FIRST)) return 5 + qd;
  return (root == MOBI_ENCQ_ROOT_8 ? 1 : 3) + half;
}

// ---- the tree in pblock's order: node(shape row, code column 2 / 3) for a split, leaf(shape row, the leaf's first quadrant) for a leaf ----
template <class Node, class Leaf>
MOBI_TC_FN void mobi_encq_walk(int tree, Node node, Leaf leaf) {
  const int root = tree & MOBI_ENCQ_ROOT_MASK;
  if (root == MOBI_ENCQ_ROOT_LEAF) {
    leaf(0, 0);
    return;
  }
  const bool by9 = root == MOBI_ENCQ_ROOT_9;
  node(0, by9 ? MOBI_ENCQ_C9 : MOBI_ENCQ_C8);
  for (int half = 0; half < 2; half++) {
    const int qa = by9 ? half : 2 * half, qb = by9 ? half + 2 : 2 * half + 1, row = by9 ? 2 : 1;
    if (tree & (half ? MOBI_ENCQ_SPLIT_SECOND : MOBI_ENCQ_SPLIT_FIRST)) {
      node(row, by9 ? MOBI_ENCQ_C8 : MOBI_ENCQ_C9);
      leaf(3, qa);
      leaf(3, qb);
    } else {
      leaf(row, qa);
    }
  }
}
// what a tree adds to the statistics and the stream in front of ue(cbp): v4 = the quadrants' vectors
struct MobiEncqSyntax {
  uint32_t bits, leaves, code0, nonzero, halfpel;
};
MOBI_TC_FN MobiEncqSyntax mobi_encq_syntax(const MobiEncPartsConst *K, int ver, int tree, const uint32_t *v4, uint32_t pred) {
  MobiEncqSyntax s = {0, 0, 0, 0, 0};
  mobi_encq_walk(
      tree, [&](int row, int col) { s.bits += K->q_nbits[ver][row][col]; },
      [&](int row, int qd) {
        const uint32_t v = v4[qd];
        s.leaves++;
        s.code0 += v == pred;
        s.nonzero += v != 0;
        s.halfpel += ((mobi_encp_dx(v) | mobi_encp_dy(v)) & 1) != 0;
        s.bits += K->q_nbits[ver][row][v != pred];
        if (v != pred) s.bits += (uint32_t)(mobi_encp_se_bits(mobi_encp_dx(v) - mobi_encp_dx(pred)) + mobi_encp_se_bits(mobi_encp_dy(v) - mobi_encp_dy(pred)));
      });
  return s;
}
template <class Put>
MOBI_TC_FN void mobi_encq_write_mb(const MobiEncPartsConst *K, int ver, const MobiEncMb *m, const uint32_t *v4, uint32_t pred, Put put, uint32_t *forms) {
  mobi_encq_walk(
      m->luma_mode, [&](int row, int col) { put(K->q_code[ver][row][col], K->q_nbits[ver][row][col]); },
      [&](int row, int qd) {
        const uint32_t v = v4[qd];
        const int code = v != pred;
        put(K->q_code[ver][row][code], K->q_nbits[ver][row][code]);
        if (code) {
          mobi_encp_put_se(put, mobi_encp_dx(v) - mobi_encp_dx(pred));
          mobi_encp_put_se(put, mobi_encp_dy(v) - mobi_encp_dy(pred));
        }
      });
  mobi_encp_write_residual(K, m, put, forms);
}

// one call's launch arguments: the inter call's, the quadrants' vectors (mv keeps the last leaf's) and the constants as this mode sees them
struct MobiEncPartsArgs : MobiEncInterArgs {
  uint32_t *mv4; // [n][mbw * mbh][4]
  const MobiEncPartsConst *kq;
};

// The deepest tree: root (at most 4 bits), two half codes (at most 4 each), four leaves of at most 4 + 2 x 13 bits; then as mode 0.
MOBI_TC_FN uint64_t mobi_encq_max_mb_bits() { return 4 + 2 * 4 + 4 * (4 + 2 * 13) + 13 + 6 * (1 + 64 * (uint64_t)MOBI_TC_ESCAPE_BITS); }

#if !defined(__HIP_DEVICE_COMPILE__)
static inline size_t mobi_encq_bound(uint32_t width, uint32_t height, int mode) {
  if (mode == 0) return mobi_encp_bound(width, height);
  if (mode != 1 || !mobi_enc_dims_ok(width, height)) return 0;
  const uint64_t bytes = mobi_enc_stream_bytes_h(MOBI_ENCP_MAX_HEADER_BITS, (uint64_t)(width / 16) * (height / 16) * mobi_encq_max_mb_bits());
  return (size_t)((bytes + 3) & ~(uint64_t)3);
}

// the constants: mobi_encp_build_const's, and its reverse-table rule at the four shapes
static inline void mobi_encq_build_const(MobiEncPartsConst *K) {
  memset(K, 0, sizeof *K);
  mobi_encp_build_const(K);
  static const int codes[4] = {0, 1, 8, 9};
  for (int ver = 0; ver < 2; ver++)
    for (int row = 0; row < 4; row++) {
      const int s = mobi_encq_shape(row), peek = 32 - mobi_part_shift[ver][s];
      for (int col = 0; col < 4; col++) {
        const int code = codes[col], nb = mobi_part_bits[ver][s][code];
        if (nb == 0 || nb == 255 || code >= mobi_part_nbits_len[ver][s]) continue;
        K->q_nbits[ver][row][col] = (uint8_t)nb;
        for (int i = (1 << peek) - 1; i >= 0; i--)
          if (mobi_part_lut[ver][s][i] == code) K->q_code[ver][row][col] = (uint8_t)(i >> (peek - nb));
      }
    }
}

// ---- the search of one leaf, scalar: mobi_encp_search's two steps with the SAD over the leaf at pixel (x, y).  Returns the best key. ----
static inline uint32_t mobi_encq_leaf_sad(const uint8_t *src_y, const uint8_t *ref_y, int W, int x, int y, int w, int h, int dx, int dy) {
  const int phase = (dx & 1) | (dy & 1) << 1;
  const uint8_t *s = src_y + (size_t)y * W + x, *r = ref_y + (ptrdiff_t)(y + (dy >> 1)) * W + x + (dx >> 1);
  uint32_t sad = 0;
  for (int j = 0; j < h; j++)
    for (int i = 0; i < w; i++) {
      const int d = (int)s[j * W + i] - mobi_encp_pred_px(r + j * W + i, W, phase);
      sad += (uint32_t)(d < 0 ? -d : d);
    }
  return sad;
}
static inline uint64_t mobi_encq_leaf_search(int q, int W, int H, int x, int y, int w, int h, const uint8_t *src_y, const uint8_t *ref_y) {
  const int64_t lam = mobi_enc_lambda(q);
  uint64_t best = MOBI_ENCP_NO_KEY;
  for (int dy = -MOBI_ENCP_RANGE; dy <= MOBI_ENCP_RANGE; dy += 2)
    for (int dx = -MOBI_ENCP_RANGE; dx <= MOBI_ENCP_RANGE; dx += 2) {
      if (!mobi_encq_leaf_ok(W, H, x, y, w, h, dx, dy)) continue;
      const uint64_t key = mobi_encp_key(lam, mobi_encq_leaf_sad(src_y, ref_y, W, x, y, w, h, dx, dy), dx, dy);
      if (key < best) best = key;
    }
  const int fx = mobi_encp_key_dx(best), fy = mobi_encp_key_dy(best); // (0, 0) is always a candidate
  for (int j = -1; j <= 1; j++)
    for (int i = -1; i <= 1; i++) {
      if ((!i && !j) || !mobi_encq_leaf_ok(W, H, x, y, w, h, fx + i, fy + j)) continue;
      const uint64_t key = mobi_encp_key(lam, mobi_encq_leaf_sad(src_y, ref_y, W, x, y, w, h, fx + i, fy + j), fx + i, fy + j);
      if (key < best) best = key;
    }
  return best;
}
// one macroblock: its tree and the quadrants' vectors
static inline int mobi_encq_search(const MobiEncPartsConst *K, int ver, int q, int W, int H, int mbx, int mby, const uint8_t *src_y, const uint8_t *ref_y,
                                   uint32_t *v4) {
  uint64_t key[MOBI_ENCQ_LEAVES], C[MOBI_ENCQ_LEAVES];
  for (int l = 0; l < MOBI_ENCQ_LEAVES; l++) {
    const MobiEncqLeaf f = mobi_encq_leaf(l);
    key[l] = mobi_encq_leaf_search(q, W, H, mbx * 16 + f.x, mby * 16 + f.y, f.w, f.h, src_y, ref_y);
    C[l] = mobi_encq_key_cost(key[l]);
  }
  const int tree = mobi_encq_decide(K, ver, mobi_enc_lambda(q), C);
  for (int qd = 0; qd < 4; qd++) {
    const uint64_t k = key[mobi_encq_leaf_of(tree, qd)];
    v4[qd] = mobi_encp_pack(mobi_encp_key_dx(k), mobi_encp_key_dy(k));
  }
  return tree;
}

// ---- one macroblock's prediction and residual, scalar: mobi_encp_macroblock with a vector per sample ----
static inline void mobi_encq_macroblock(const MobiEncInterConst *K, int q, int W, int mbx, int mby, const uint32_t *v4, const uint8_t *const src[3],
                                        const uint8_t *const ref[3], uint8_t *const rec[3], MobiEncMb *out, MobiEncMbStats *st) {
  memset(out, 0, sizeof *out);
  st->sad = st->coded = st->clamp = st->range = 0;
  for (int k = 0; k < 6; k++) {
    int s[64], p[64], r[64];
    const MobiEncpBlockRef at = mobi_encp_block_ref(k, mbx, mby, W, 0, 0);
    for (int y = 0; y < 8; y++)
      for (int x = 0; x < 8; x++) {
        const uint32_t v = v4[k < 4 ? k : (y >> 2) * 2 + (x >> 2)];
        const MobiEncpBlockRef b = mobi_encp_block_ref(k, mbx, mby, W, mobi_encp_dx(v), mobi_encp_dy(v));
        s[y * 8 + x] = src[b.plane][(size_t)(b.y0 + y) * b.pitch + b.x0 + x];
        p[y * 8 + x] = mobi_encp_pred_px(ref[b.plane] + (ptrdiff_t)(b.ry + y) * b.pitch + b.rx + x, b.pitch, b.phase);
      }
    const MobiEncBlock res = mobi_enc_block(K, q, s, p, out->lev[k], r);
    for (int y = 0; y < 8; y++)
      for (int x = 0; x < 8; x++) rec[at.plane][(size_t)(at.y0 + y) * at.pitch + at.x0 + x] = (uint8_t)r[y * 8 + x];
    out->cbp |= (uint8_t)(res.coded << k);
    out->bits += (uint32_t)res.bits;
    st->sad += (uint32_t)res.sad;
    st->coded += res.coded;
    st->clamp += res.clamp;
    st->range += res.range;
  }
}

// ---- one picture on the CPU.  mode 0 is mobi_encp_picture (trees 0, the four vectors v*); mode 1 searches the nine leaves of every
// macroblock.  mv4 (4 per macroblock) is required besides what mobi_encp_picture requires. ----
static inline bool mobi_encq_picture(const MobiEncPartsConst *K, int ver, int mode, int W, int H, int prev_q, int q, const uint8_t *i420,
                                     const uint8_t *ref_i420, uint8_t *slot, size_t slot_bytes, int32_t *bytes_out, uint8_t *rec, mobi_enc_inter_stats *stats,
                                     MobiEncMb *mbs, uint32_t *mv, uint32_t *mvp, uint32_t *mv4, uint32_t *forms) {
  const int mbw = W / 16, mbh = H / 16;
  if (!mode) {
    const bool ok = mobi_encp_picture(K, ver, W, H, prev_q, q, i420, ref_i420, slot, slot_bytes, bytes_out, rec, stats, mbs, mv, mvp, forms);
    for (int i = 0; i < mbw * mbh; i++) mv4[4 * i] = mv4[4 * i + 1] = mv4[4 * i + 2] = mv4[4 * i + 3] = mv[i];
    return ok;
  }
  const size_t ysz = (size_t)W * H;
  const uint8_t *const src[3] = {i420, i420 + ysz, i420 + ysz + ysz / 4};
  const uint8_t *const ref[3] = {ref_i420, ref_i420 + ysz, ref_i420 + ysz + ysz / 4};
  uint8_t *const r3[3] = {rec, rec + ysz, rec + ysz + ysz / 4};
  mobi_enc_inter_stats st;
  memset(&st, 0, sizeof st);
  std::vector<uint8_t> trees((size_t)mbw * mbh);
  for (int y = 0; y < mbh; y++)
    for (int x = 0; x < mbw; x++) {
      const int i = y * mbw + x;
      trees[i] = (uint8_t)mobi_encq_search(K, ver, q, W, H, x, y, src[0], ref[0], mv4 + 4 * i);
      mv[i] = mv4[4 * i + 3]; // the last leaf: what the neighbours' predictors see
    }
  uint64_t mb_bits = 0;
  for (int y = 0; y < mbh; y++)
    for (int x = 0; x < mbw; x++) {
      const int i = y * mbw + x;
      MobiEncMbStats ms;
      mobi_encq_macroblock(K, q, W, x, y, mv4 + 4 * i, src, ref, r3, mbs + i, &ms);
      mbs[i].luma_mode = trees[i];
      mvp[i] = mobi_encp_predictor(mv, mbw, x, y);
      const MobiEncqSyntax sx = mobi_encq_syntax(K, ver, trees[i], mv4 + 4 * i, mvp[i]);
      mbs[i].bits += sx.bits + mobi_encp_cbp_bits(K, mbs[i].cbp);
      mb_bits += mbs[i].bits;
      st.sad += ms.sad;
      st.mv_bits += sx.bits;
      st.coded_blocks += ms.coded;
      st.fallback_clamp += ms.clamp;
      st.fallback_level += ms.range;
      st.code0 += sx.code0;
      st.nonzero_mv += sx.nonzero;
      st.halfpel_mv += sx.halfpel;
      st.reserved[MOBI_ENC_PARTS_STAT_SPLIT] += trees[i] != MOBI_ENCQ_ROOT_LEAF;
      st.reserved[MOBI_ENC_PARTS_STAT_LEAVES] += sx.leaves;
    }
  return mobi_enc_finish_picture((uint64_t)mobi_encp_header_bits(q, prev_q), mb_bits, st, stats, slot, slot_bytes, bytes_out, [&](auto put) {
    mobi_encp_write_header(put, q, prev_q);
    for (int i = 0; i < mbw * mbh; i++) mobi_encq_write_mb(K, ver, mbs + i, mv4 + 4 * i, mvp[i], put, forms);
  });
}
#endif
#endif
