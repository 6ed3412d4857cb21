// mobi_motion.hip -- the motion the STREAM carries, kept and exported (mobi_batch_set_motion / mobi_batch_export_motion): mobi_motion_field
// reads a frame step's command list while it still sits in HBM -- descriptors and payload, as the reconstruction kernels read them -- and
// writes the step's slot of the motion ring (mobi_motion_ring.h); the three export kernels read the ring into the caller's tensors.  What a
// descriptor says about a cell and a macroblock is mobi_motion.h's, shared with the CPU statement of the tests.
//
// mobi_motion_field moves 32 B of descriptor and at most 1.8 KB of payload in and 288 B out per macroblock and computes next to nothing: what
// counts is the number of store instructions (16-byte stores at a quarter of the issue cost per byte of 4-byte ones).  So a lane takes four
// consecutive cells -- one 16-byte store --, sixteen lanes a macroblock, a wave four macroblocks at a time: its cell store is one instruction
// of 1 KB, eight whole lines.  The four cells of a lane lie in one half of a DUAL macroblock (mobi_motion.h asserts it), so a macroblock
// without a cell map costs a lane one leaf decode.  The sixteen lanes of a macroblock share the walk over its level words; one 16-lane
// reduction gives the sum.  The descriptor is read by all sixteen from one address (a broadcast).  A workgroup takes four rounds of sixteen
// macroblocks with every round's descriptors and cell maps loaded up front: with one round per wave the step's kernel took 0.69 ms at 4096
// clips of 640x480, with four 0.49 (1.2 M waves of two dependent loads each were the cost, not the bytes).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <algorithm>

#include "mobi_motion.h"
#include "mobi_motion_ring.h"

namespace {
constexpr int kThreads = 256;
constexpr int kLanesPerMb = 16, kMbsPerBlock = kThreads / kLanesPerMb, kRun = 4; // a workgroup: kRun rounds of sixteen macroblocks
constexpr unsigned kMaxGridY = 32768; // clips beyond it: the blocks loop
static_assert(sizeof(MbDesc) == 32 && MOBI_MV_CELLS == 4 * kLanesPerMb && MOBI_MOTION_MB_WORDS <= kLanesPerMb && MOBI_MB_VALUES <= MOBI_MOTION_MB_WORDS, "a lane: four cells, one word of the record");

struct FieldArgs {
  const MbDesc *desc;
  const uint32_t *payload;
  uint32_t *cells;
  int32_t *mbs;
  uint32_t pay_clip_words, n_mbs, mbw, stride, blocks_per_clip, clip0, slot;
};
// macroblock mb of clip c, ring slot s -> its index in the ring's two tables
__device__ __forceinline__ size_t ring_mb(uint32_t clip, uint32_t slot, uint32_t n_mbs, uint32_t mb) { return ((size_t)clip * 6 + slot) * n_mbs + mb; }
} // namespace

// grid: blocks_per_clip * clips of the launch.  A workgroup takes kRun * 16 consecutive macroblocks of one clip: in round i its sixteen groups of
// lanes take macroblocks base + 16 i .. base + 16 i + 15 (a wave's stores stay one run of whole lines), and the loads of all rounds are
// issued before the first store: descriptors, then the cell maps; only the level words wait for their round.
extern "C" __global__ __launch_bounds__(kThreads) void mobi_motion_field(FieldArgs A) {
  const uint32_t clip = blockIdx.x / A.blocks_per_clip, mb0 = (blockIdx.x - clip * A.blocks_per_clip) * (kMbsPerBlock * kRun) + (threadIdx.x / kLanesPerMb);
  const uint32_t sub = threadIdx.x % kLanesPerMb;
  const MbDesc *desc = A.desc + (size_t)clip * A.n_mbs;
  const uint32_t *pay_clip = A.payload + (size_t)clip * A.pay_clip_words; // (as mobi_recon_inter8 and mobi_recon_intra address it)
  const int S = (int)A.stride;
  MbDesc d[kRun];
  uint32_t cw[kRun][4];
#pragma unroll
  for (int i = 0; i < kRun; i++) {
    const uint32_t mb = mb0 + i * kMbsPerBlock;
    d[i] = MbDesc{0, MOBI_MB_INTRA, 0, 0, 0, 0, 0, 0}; // past the clip's last macroblock: nothing to read (the sixteen lanes of a macroblock agree)
    if (mb < A.n_mbs) {
      const uint4 *dp = reinterpret_cast<const uint4 *>(desc + mb);
      const uint4 lo = dp[0], hi = dp[1];
      d[i] = MbDesc{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    }
  }
#pragma unroll
  for (int i = 0; i < kRun; i++) {
    cw[i][0] = cw[i][1] = cw[i][2] = cw[i][3] = 0;
    if (mobi_motion_has_cells(d[i].w1)) {
#pragma unroll
      for (int k = 0; k < 4; k++) cw[i][k] = pay_clip[d[i].payload_off + 4 * sub + k];
    }
  }
#pragma unroll
  for (int i = 0; i < kRun; i++) {
    const uint32_t mb = mb0 + i * kMbsPerBlock;
    if (mb >= A.n_mbs) break;
    uint32_t w[4];
    if (mobi_motion_has_cells(d[i].w1)) {
#pragma unroll
      for (int k = 0; k < 4; k++) w[k] = mobi_mcell(mobi_motion_of_cell_word(cw[i][k], S));
    } else {
      MobiMotion m{0, 0, 0};
      if (!mobi_w1_intra(d[i].w1)) m = mobi_motion_of_leaf(d[i], mobi_motion_leaf_of_cell(mobi_w1_dual(d[i].w1), (int)(4 * sub)), mobi_mb_offset(mb, A.mbw, A.stride), S);
      w[0] = w[1] = w[2] = w[3] = mobi_mcell(m);
    }
    int32_t sum = mobi_motion_level_sum(d[i], pay_clip + d[i].payload_off, sub, kLanesPerMb);
#pragma unroll
    for (int o = kLanesPerMb / 2; o; o >>= 1) sum += __shfl_xor(sum, o, kLanesPerMb);
    const size_t r = ring_mb(A.clip0 + clip, A.slot, A.n_mbs, mb);
    reinterpret_cast<uint4 *>(A.cells + r * MOBI_MV_CELLS)[sub] = make_uint4(w[0], w[1], w[2], w[3]);
    if (sub < MOBI_MOTION_MB_WORDS) A.mbs[r * MOBI_MOTION_MB_WORDS + sub] = sub < MOBI_MBV_LEVELS ? mobi_motion_mb_value(d[i], (int)sub) : sub == MOBI_MBV_LEVELS ? sum : 0;
  }
}

extern "C" int mobi_launch_motion_field(const MobiReconArgs *a, int clip0, const MobiMotionRing *ring, hipStream_t s) {
  if (a->n_clips <= 0 || a->n_mbs <= 0) return 0;
  FieldArgs A;
  A.desc = a->desc; A.payload = a->payload; A.cells = ring->cells; A.mbs = ring->mbs;
  A.pay_clip_words = a->pay_clip_words; A.n_mbs = (uint32_t)a->n_mbs; A.mbw = (uint32_t)a->mbw; A.stride = (uint32_t)a->stride;
  A.blocks_per_clip = (A.n_mbs + kMbsPerBlock * kRun - 1) / (kMbsPerBlock * kRun); A.clip0 = (uint32_t)clip0; A.slot = (uint32_t)a->ring_base;
  hipLaunchKernelGGL(mobi_motion_field, dim3(A.blocks_per_clip * (unsigned)a->n_clips), dim3(kThreads), 0, s, A); // (< 2^19 clips of <= 128 blocks)
  return (int)hipGetLastError();
}

// ---- the exports: grid x = the picture's threads, y = clips (looping beyond kMaxGridY), z = frames ----
namespace {
struct ExportArgs {
  const uint32_t *cells;
  const int32_t *mbs;
  void *out;
  uint32_t mbw, mbh, n_clips, clip0, slot0;
  uint32_t block, esize; // flow
  float k;
};
__device__ __forceinline__ uint32_t pack16(int a, int b) { return ((uint32_t)a & 0xFFFFu) | ((uint32_t)b << 16); }
} // namespace

// MOBI_MOTION_CELLS.  A thread: one row of eight cells of a macroblock -- 32 B of the ring in, 16 B into each of the three planes
extern "C" __global__ __launch_bounds__(kThreads) void mobi_motion_export_cells(ExportArgs A) {
  const uint32_t rows = A.mbh * 8, wc = A.mbw * 8, i = blockIdx.x * kThreads + threadIdx.x, n_mbs = A.mbw * A.mbh;
  if (i >= rows * A.mbw) return;
  const uint32_t row = i / A.mbw, mbx = i - row * A.mbw, mb = (row >> 3) * A.mbw + mbx, slot = (A.slot0 + blockIdx.z) % 6;
  const size_t plane = (size_t)rows * wc;
  for (uint32_t c = blockIdx.y; c < A.n_clips; c += gridDim.y) {
    const uint4 *src = reinterpret_cast<const uint4 *>(A.cells + ring_mb(A.clip0 + c, slot, n_mbs, mb) * MOBI_MV_CELLS + (row & 7) * 8);
    const uint4 a = src[0], b = src[1];
    const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    int16_t *o = (int16_t *)A.out + ((size_t)blockIdx.z * A.n_clips + c) * 3 * plane + (size_t)row * wc + mbx * 8;
    uint32_t px[4], py[4], pr[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      px[q] = pack16(mobi_mcell_dx(v[2 * q]), mobi_mcell_dx(v[2 * q + 1]));
      py[q] = pack16(mobi_mcell_dy(v[2 * q]), mobi_mcell_dy(v[2 * q + 1]));
      pr[q] = pack16(mobi_mcell_ref(v[2 * q]), mobi_mcell_ref(v[2 * q + 1]));
    }
    *reinterpret_cast<uint4 *>(o) = make_uint4(px[0], px[1], px[2], px[3]);
    *reinterpret_cast<uint4 *>(o + plane) = make_uint4(py[0], py[1], py[2], py[3]);
    *reinterpret_cast<uint4 *>(o + 2 * plane) = make_uint4(pr[0], pr[1], pr[2], pr[3]);
  }
}

// MOBI_MOTION_MB.  A thread: one macroblock's record into the five planes
extern "C" __global__ __launch_bounds__(kThreads) void mobi_motion_export_mb(ExportArgs A) {
  const uint32_t n_mbs = A.mbw * A.mbh, mb = blockIdx.x * kThreads + threadIdx.x, slot = (A.slot0 + blockIdx.z) % 6;
  if (mb >= n_mbs) return;
  for (uint32_t c = blockIdx.y; c < A.n_clips; c += gridDim.y) {
    const int32_t *src = A.mbs + ring_mb(A.clip0 + c, slot, n_mbs, mb) * MOBI_MOTION_MB_WORDS;
    const int4 a = *reinterpret_cast<const int4 *>(src);
    const int32_t v[MOBI_MB_VALUES] = {a.x, a.y, a.z, a.w, src[4]};
    int32_t *o = (int32_t *)A.out + ((size_t)blockIdx.z * A.n_clips + c) * MOBI_MB_VALUES * n_mbs + mb;
#pragma unroll
    for (int q = 0; q < MOBI_MB_VALUES; q++) o[(size_t)q * n_mbs] = v[q];
  }
}

// MOBI_MOTION_FLOW.  A thread: one block of (block / 2)^2 cells, all of one macroblock -> its two values
extern "C" __global__ __launch_bounds__(kThreads) void mobi_motion_export_flow(ExportArgs A) {
  const uint32_t per = 16 / A.block, ow = A.mbw * per, oh = A.mbh * per, cb = A.block / 2, i = blockIdx.x * kThreads + threadIdx.x, n_mbs = A.mbw * A.mbh;
  if (i >= ow * oh) return;
  const uint32_t oy = i / ow, ox = i - oy * ow, cy = oy * cb, cx = ox * cb, mb = (cy >> 3) * A.mbw + (cx >> 3), slot = (A.slot0 + blockIdx.z) % 6;
  for (uint32_t c = blockIdx.y; c < A.n_clips; c += gridDim.y) {
    const uint32_t *src = A.cells + ring_mb(A.clip0 + c, slot, n_mbs, mb) * MOBI_MV_CELLS + (cy & 7) * 8 + (cx & 7);
    int32_t sx = 0, sy = 0;
    for (uint32_t y = 0; y < cb; y++)
      for (uint32_t x = 0; x < cb; x++) {
        const uint32_t w = src[y * 8 + x];
        const int f = mobi_flow_weight(mobi_mcell_ref(w));
        sx += mobi_mcell_dx(w) * f;
        sy += mobi_mcell_dy(w) * f;
      }
    const float fx = (float)sx * A.k, fy = (float)sy * A.k; // one conversion, one product: each rounded once
    const size_t at = ((size_t)blockIdx.z * A.n_clips + c) * 2 * ow * oh + i;
    if (A.esize == 4) {
      ((float *)A.out)[at] = fx;
      ((float *)A.out)[at + (size_t)ow * oh] = fy;
    } else {
      ((__half *)A.out)[at] = __float2half_rn(fx);
      ((__half *)A.out)[at + (size_t)ow * oh] = __float2half_rn(fy);
    }
  }
}

namespace {
template <class K> int launch_export(K kernel, const MobiMotionExport *x, uint32_t threads, ExportArgs A, hipStream_t s) {
  if (x->n_frames <= 0 || x->n_clips <= 0 || threads == 0) return 0;
  A.cells = x->ring.cells; A.mbs = x->ring.mbs;
  A.mbw = (uint32_t)x->mbw; A.mbh = (uint32_t)x->mbh; A.n_clips = (uint32_t)x->n_clips; A.clip0 = (uint32_t)x->clip0; A.slot0 = (uint32_t)x->slot0;
  hipLaunchKernelGGL(kernel, dim3((threads + kThreads - 1) / kThreads, std::min((unsigned)x->n_clips, kMaxGridY), (unsigned)x->n_frames), dim3(kThreads), 0, s, A);
  return (int)hipGetLastError();
}
} // namespace
extern "C" int mobi_launch_motion_cells(const MobiMotionExport *x, int16_t *out_dev, hipStream_t s) {
  ExportArgs A{};
  A.out = out_dev;
  return launch_export(mobi_motion_export_cells, x, (uint32_t)(x->mbh * 8 * x->mbw), A, s);
}
extern "C" int mobi_launch_motion_mb(const MobiMotionExport *x, int32_t *out_dev, hipStream_t s) {
  ExportArgs A{};
  A.out = out_dev;
  return launch_export(mobi_motion_export_mb, x, (uint32_t)(x->mbw * x->mbh), A, s);
}
extern "C" int mobi_launch_motion_flow(const MobiMotionExport *x, int block, int esize, float k, void *out_dev, hipStream_t s) {
  if ((block != 2 && block != 4 && block != 8 && block != 16) || (esize != 2 && esize != 4)) return -1;
  ExportArgs A{};
  A.out = out_dev; A.block = (uint32_t)block; A.esize = (uint32_t)esize; A.k = k;
  const uint32_t per = 16u / (uint32_t)block;
  return launch_export(mobi_motion_export_flow, x, (uint32_t)(x->mbw * x->mbh) * per * per, A, s);
}
