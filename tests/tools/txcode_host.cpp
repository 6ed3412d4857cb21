// txcode_host.cpp -- TEST TOOL: the product's mobi_txcode.h compiled for the host (tests/test_txcode.py builds it with g++), so that the
// quantiser, the cost table and the table builders the kernel uses can be checked exhaustively without a GPU.
#include "mobi_txcode.h"

extern "C" {
void tc_build_ref(int16_t *ref) { mobi_tc_build_ref(ref); }
void tc_build_lut(uint8_t *lut) { mobi_tc_build_lut(lut); }
int tc_lut_index(int v, int skip, int last) { return mobi_tc_lut_index(v, skip, last); }
void tc_qtable(int q, int n, int32_t *Q) { mobi_tc_qtable(q, n, Q); }
// out[i] = mobi_tc_quant(d, Q, 1.0f / Q) for d = d0 + i, i < count (the reciprocal the product's constant table holds)
void tc_quant_range(int d0, int count, int Q, int32_t *out) {
  const float rq = 1.0f / (float)Q;
  for (int i = 0; i < count; i++) out[i] = mobi_tc_quant(d0 + i, Q, rq);
}
}
