// mobi_idle_host.cpp -- TEST TOOL: the idle handling of the frame-parallel chain (mobi_gop.h: mobi_gop_prepare_clip / mobi_gop_chain_clip, the
// bodies of the two device kernels) on the CPU.  One group of K frames of n clips that all carry the SAME stream, clip c idle from frame
// idle_from[c] on: the tables the device would hold are built in host memory -- the staged bitstream image with MOBI_DP_SKIP for a length in
// every idle slot, the rows of the idle slots as mobi_idle_rows leaves them (rc 0), the rows of the live frames as a device parser that
// finishes them leaves them (the host parser's command list and state: the two are equal word for word, tests/test_lsparse.py) -- then
// prepare, "parse", chain, as the group's launches go.  Everything the chain wrote comes back for the test to compare, beside the truth:
// the host parser's state in front of every frame, in stream order.
// Built by mobiclipdecoder_amd/build.py into tests/tools/libmobi_idle_host.so; used by tests/test_idle_chain.py.  Not part of the product.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#define MOBI_GOP_DEVICE_DECLS
#include "mobi_gop.h"
#include "mobi_parse.h"

namespace {
template <class T> struct Aligned { // 16-byte aligned, as device allocations are (the chain loads descriptors 16 bytes at a time)
  std::vector<uint8_t> raw;
  T *p = nullptr;
  size_t count = 0;
  void alloc(size_t n, int fill) {
    count = n;
    raw.assign(n * sizeof(T) + 16, (uint8_t)fill);
    p = (T *)(((uintptr_t)raw.data() + 15) & ~(uintptr_t)15);
  }
};
} // namespace

extern "C" {
// data / frame_off: one stream of at least pre + K frames.  The first `pre` frames are decoded before the group (the state ring entry the
// group reads is then not a new decoder's).  idle_from: [n] (nullptr: no idle slot, MobiGopArgs.idle_from == nullptr).
// Out: rc_out[K * n] MobiDevResult.rc behind the chain; sin_out[K * n] the start-state slots (64 bytes each; 0xAB where nothing wrote);
// ring_out[n] / rtail_out[n] what goes into the batch's state ring; truth_state[K + 1] / truth_tail[K + 1]: the host parser's state in
// front of frame k of the group (k == K: behind the last).  Returns 0, or -1 for bad arguments / a frame the host parser rejects.
int mobi_idle_chain_run(uint32_t w, uint32_t h, int version, const uint8_t *data, const uint32_t *frame_off, int pre, int n, int K,
                        const uint8_t *idle_from, int32_t *rc_out, uint8_t *sin_out, uint8_t *ring_out, uint8_t *rtail_out,
                        uint8_t *truth_state, uint8_t *truth_tail) {
  if (n < 1 || K < 1 || K > MOBI_GOP_PARSE_MAX || pre < 0) return -1;
  MobiStreamParser A(w, h, version);
  const MobiGeom g = A.geom();
  const int n_mbs = g.mbw * g.mbh;
  const size_t nv = (size_t)n * K, cap_words = (size_t)n_mbs * 448 + 1024;
  ParsedFrame pf;
  for (int f = 0; f < pre; f++) {
    int32_t off = 0;
    if (A.parse_frame(data + frame_off[f], frame_off[f + 1] - frame_off[f], &off, pf) != 0 /* MOBI_OK */) return -1;
  }
  // the truth, in stream order, and every frame's command list
  std::vector<ParsedFrame> frames(K);
  std::vector<MobiDevState> ts(K + 1);
  std::vector<MobiDevTail> tt(K + 1);
  A.export_state(ts[0], tt[0]);
  for (int k = 0; k < K; k++) {
    int32_t off = 0;
    if (A.parse_frame(data + frame_off[pre + k], frame_off[pre + k + 1] - frame_off[pre + k], &off, frames[k]) != 0 /* MOBI_OK */ || !A.device_ready()) return -1;
    A.export_state(ts[k + 1], tt[k + 1]);
  }
  memcpy(truth_state, ts.data(), (K + 1) * sizeof(MobiDevState));
  memcpy(truth_tail, tt.data(), (K + 1) * sizeof(MobiDevTail));
  // the staged image
  std::vector<uint64_t> boff(nv);
  std::vector<uint32_t> blen(nv);
  std::vector<uint8_t> bits;
  for (size_t v = 0; v < nv; v++) {
    const int k = (int)(v / n), c = (int)(v % n);
    boff[v] = bits.size();
    if (idle_from && k >= idle_from[c]) { blen[v] = MOBI_DP_SKIP; continue; } // (an idle lane has no bytes: csrc/mobi_handover.h)
    const uint32_t l = frame_off[pre + k + 1] - frame_off[pre + k];
    blen[v] = l;
    bits.insert(bits.end(), data + frame_off[pre + k], data + frame_off[pre + k] + l);
    bits.resize((bits.size() + 32 + 7) & ~(size_t)7, 0);
  }
  bits.resize(bits.size() + 64, 0);
  std::vector<uint8_t> tables(MOBI_DT_BYTES);
  mobi_dparse_build_tables(version, tables.data());
  std::vector<int32_t> scale((size_t)MOBI_SCALE_ROWS * MOBI_SCALE_STRIDE, 0);
  for (int q = 0; q < MOBI_SCALE_QMAX; q++) mobi_build_scale_table(q, &scale[(size_t)q * MOBI_SCALE_STRIDE]);
  mobi_build_scale_table(MOBI_SCALE_LITERAL, &scale[(size_t)MOBI_SCALE_LITERAL * MOBI_SCALE_STRIDE]);
  Aligned<MobiDevState> sin, sout, rin, rout;
  Aligned<MobiDevTail> tails, tin, tout;
  Aligned<MobiDevResult> res;
  Aligned<MbDesc> desc;
  Aligned<uint32_t> pay;
  sin.alloc(nv, 0xAB); sout.alloc(nv, 0xCD); tails.alloc(nv, 0xEF); res.alloc(nv, 0x77);
  rin.alloc(n, 0); rout.alloc(n, 0xAB); tin.alloc(n, 0); tout.alloc(n, 0xAB);
  desc.alloc(nv * n_mbs, 0x55); pay.alloc(nv * cap_words, 0x33);
  for (int c = 0; c < n; c++) { rin.p[c] = ts[0]; tin.p[c] = tt[0]; }
  MobiGopArgs G;
  memset(&G, 0, sizeof(G));
  G.P.bits = bits.data(); G.P.bit_off = boff.data(); G.P.bit_len = blen.data();
  G.P.tables = tables.data();
  G.P.state_in = sin.p; G.P.state_out = sout.p; G.P.tail_out = tails.p;
  G.P.scale = scale.data();
  G.P.desc = desc.p; G.P.payload = pay.p; G.P.res = res.p;
  G.P.pay_cap = (uint32_t)cap_words;
  G.P.n_clips = (int)nv; G.P.version = version;
  G.P.width = g.width; G.P.height = g.height; G.P.stride = g.stride; G.P.lg = g.lg; G.P.mbw = g.mbw; G.P.mbh = g.mbh;
  G.P.pay_local = 1; G.P.clip_mod = n; G.P.skip_tail = 1;
  G.ring_in = rin.p; G.ring_out = rout.p; G.rtail_in = tin.p; G.rtail_out = tout.p;
  G.n = n; G.K = K;
  G.idle_from = idle_from;
  // mobi_idle_rows: the idle slots' records (in front of the parse kernels)
  for (size_t v = 0; v < nv; v++)
    if (blen[v] == MOBI_DP_SKIP) {
      memset(&res.p[v], 0, sizeof(MobiDevResult));
      for (int mb = 0; mb < n_mbs; mb++) desc.p[v * n_mbs + mb] = MbDesc{0, MOBI_MB_INTRA, 0, 0, 0, 0, 0, 0};
    }
  for (int c = 0; c < n; c++) mobi_gop_prepare_clip(G, c);
  // the parse kernels: every live virtual clip on its own, from its predicted start state.  What a frame's parse depends on is what
  // mobi_gop_guess_ok compares; a frame whose prediction holds leaves the host parser's command list and state.
  for (size_t v = 0; v < nv; v++) {
    if (blen[v] == MOBI_DP_SKIP) continue;
    const int k = (int)(v / n);
    const ParsedFrame &f = frames[k];
    if (f.payload.size() > cap_words) return -1;
    memcpy(&desc.p[v * n_mbs], f.desc.data(), (size_t)n_mbs * sizeof(MbDesc));
    if (!f.payload.empty()) memcpy(&pay.p[v * cap_words], f.payload.data(), f.payload.size() * 4);
    MobiDevResult r;
    memset(&r, 0, sizeof(r));
    r.n_intra = f.hdr.n_intra; r.payload_words = f.hdr.payload_words; r.quant = ts[k + 1].quant; r.yuvfmt = ts[k + 1].yuvfmt; r.frame_type = f.hdr.frame_type;
    res.p[v] = r;
    sout.p[v] = ts[k + 1];
    for (int i = 0; i < 40; i++) // bytes of the mode cache the frame did not write read "not written yet", as a parse from a predicted state leaves them
      if (mobi_mc_interior(i) && sin.p[v].mcache[i] == MOBI_MC_UNWRITTEN && ts[k + 1].mcache[i] == ts[k].mcache[i]) sout.p[v].mcache[i] = MOBI_MC_UNWRITTEN;
    memcpy(tails.p[v].mvc, tt[k + 1].mvc, sizeof(tt[k + 1].mvc));
  }
  uint8_t izz[80];
  for (int i = 0; i < 64; i++) izz[tables[MOBI_DT_ZZ8 + i]] = (uint8_t)i;
  for (int i = 0; i < 16; i++) izz[64 + tables[MOBI_DT_ZZ4 + i]] = (uint8_t)i;
  for (int c = 0; c < n; c++) mobi_gop_chain_clip(G, c, izz);
  for (size_t v = 0; v < nv; v++) rc_out[v] = res.p[v].rc;
  memcpy(sin_out, sin.p, nv * sizeof(MobiDevState));
  memcpy(ring_out, rout.p, n * sizeof(MobiDevState));
  memcpy(rtail_out, tout.p, n * sizeof(MobiDevTail));
  return 0;
}
}
