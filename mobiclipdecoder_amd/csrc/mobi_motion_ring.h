// mobi_motion_ring.h -- launch interface between the C-ABI layer (mobi_batch.h, mobi_pictures.cpp) and mobi_motion.hip: the motion ring of a
// batch (mobi_batch_set_motion) and the kernels that write and read it.  What a cell word and a macroblock record hold: mobi_motion.h.
#ifndef MOBI_MOTION_RING_H
#define MOBI_MOTION_RING_H
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "mobi_kernels.h"
#include "mobi_motion.h"

// The motion ring, beside the picture ring and turning with it (slot = the picture's ring slot):
//   cells : [clip][slot 0..5][mb][64] cell words, macroblock after macroblock: a wave's stores are whole lines
//   mbs   : [clip][slot 0..5][mb][MOBI_MOTION_MB_WORDS] int32
struct MobiMotionRing {
  uint32_t *cells;
  int32_t *mbs;
};
// mobi_motion_field: the slot a->ring_base of clips clip0 .. clip0 + a->n_clips - 1 from the step's own command list (a->desc, a->payload,
// a->pay_clip_words; clip 0 of the list is clip clip0 of the batch).  Idempotent.
extern "C" int mobi_launch_motion_field(const MobiReconArgs *a, int clip0, const MobiMotionRing *ring, hipStream_t s);

// the pictures of an export (n_frames x n_clips, picture q = frame q / n_clips = slot (slot0 + q / n_clips) % 6, clip clip0 + q % n_clips)
struct MobiMotionExport {
  MobiMotionRing ring;
  int mbw, mbh, n_frames, n_clips, clip0, slot0;
};
// MOBI_MOTION_CELLS: int16 [3][mbh * 8][mbw * 8] per picture
extern "C" int mobi_launch_motion_cells(const MobiMotionExport *x, int16_t *out_dev, hipStream_t s);
// MOBI_MOTION_MB: int32 [5][mbh][mbw]
extern "C" int mobi_launch_motion_mb(const MobiMotionExport *x, int32_t *out_dev, hipStream_t s);
// MOBI_MOTION_FLOW: [2][mbh * 16 / block][mbw * 16 / block] of float32 (esize 4) or float16 (esize 2), value = (float)sum * k
extern "C" int mobi_launch_motion_flow(const MobiMotionExport *x, int block, int esize, float k, void *out_dev, hipStream_t s);
#endif
