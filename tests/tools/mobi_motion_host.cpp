// mobi_motion_host.cpp -- TEST TOOL: the host build of csrc/mobi_motion.h, "command list -> motion", so that tests/test_motion_field.py can
// hold it against scripted streams without a GPU and tests/test_motion_export_gpu.py can hold the kernels against it.  Never linked into
// the library.
#include <stddef.h>
#include <stdint.h>

#include "mobi_motion.h"
#include "mobi_syntax.h"

// One frame of one clip as a parser left it (desc[n_mbs], payload: MbDesc.payload_off indexes it) -> cells[n_mbs][64][3] = dx, dy, ref and
// mbs[n_mbs][5] = the five values, macroblock after macroblock.
extern "C" void mobi_motion_host_frame(const MbDesc *desc, int n_mbs, const uint32_t *payload, int mbw, int stride, int32_t *cells, int32_t *mbs) {
  for (int mb = 0; mb < n_mbs; mb++) {
    const MbDesc &d = desc[mb];
    const uint32_t *pay = payload + d.payload_off;
    const uint32_t cur_off = mobi_mb_offset((uint32_t)mb, (uint32_t)mbw, (uint32_t)stride);
    for (int c = 0; c < MOBI_MV_CELLS; c++) {
      const MobiMotion m = mobi_motion_cell(d, pay, cur_off, stride, c);
      int32_t *o = cells + ((size_t)mb * MOBI_MV_CELLS + c) * 3;
      o[0] = m.dx; o[1] = m.dy; o[2] = m.ref;
    }
    for (int v = 0; v < MOBI_MBV_LEVELS; v++) mbs[(size_t)mb * MOBI_MB_VALUES + v] = mobi_motion_mb_value(d, v);
    mbs[(size_t)mb * MOBI_MB_VALUES + MOBI_MBV_LEVELS] = mobi_motion_level_sum(d, pay, 0, 1);
  }
}

// (dx, dy, ref) of leaf `leaf` (0: A, 1: B) of the macroblock at cur_off -> rec[5] = pos_y, pos_c, ref, luma phase, chroma phase of its leaf
// record (mobi_leaf_record), and back through the decoder: out[3] = dx, dy, ref
extern "C" void mobi_motion_host_round_trip(int dx, int dy, int ref, uint32_t cur_off, int stride, int leaf, uint32_t *rec, int32_t *out) {
  MbDesc d{};
  uint32_t &pos_y = leaf ? d.w5 : d.w3, &pos_c = leaf ? d.w6 : d.w4;
  d.w1 = mobi_desc_w1(MOBI_MB_INTER, leaf ? 2 : 1, 0, 0, 0, leaf ? MOBI_DUAL_TB : MOBI_DUAL_NONE);
  d.w2 = mobi_leaf_record(leaf, mobi_leaf_w0(0, leaf ? 8 : 0, 0, leaf, ref), mobi_leaf_w1(dx, dy), (long)cur_off, (long)stride, pos_y, pos_c);
  rec[0] = pos_y; rec[1] = pos_c; rec[2] = mobi_w2_ref(d.w2, leaf); rec[3] = mobi_w2_phase(d.w2, leaf); rec[4] = mobi_w2_cphase(d.w2, leaf);
  const MobiMotion m = mobi_motion_cell(d, nullptr, cur_off, stride, leaf ? MOBI_MV_CELLS - 1 : 0);
  out[0] = m.dx; out[1] = m.dy; out[2] = m.ref;
}
