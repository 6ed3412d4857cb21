/*
 * mobiclip_encode_parts.h -- C ABI of the inter encoder's partition mode: an opt-in mode of a mobi_enc_inter_ctx
 * (mobiclip_encode_inter.h) in which a macroblock of a P-frame may be split into two 16x8, two 8x16 or 8x8 leaves, each with a half-pel
 * vector of its own.  Mode 0, the state after mobi_enc_inter_create, is that header's encoder byte for byte.
 *
 * In mode 1 a leaf's candidates are the vectors of at most 17 half-pels either way whose luma window and two chroma windows OF THE LEAF lie
 * inside the picture; every leaf is searched as a macroblock is in mode 0, and the tree is the minimum of an integer cost (DESIGN.md,
 * "Inter encoder", "Partitions").  Nothing below 8x8 is split; one reference.  The contract stays: every stream decodes to exactly the
 * reconstruction the encoder reports.
 *
 * Statistics in mode 1 (mobi_enc_inter_stats): code0, nonzero_mv and halfpel_mv count LEAVES, mv_bits holds the tree's codes too, and
 *   reserved[MOBI_ENC_PARTS_STAT_SPLIT]   macroblocks sent split
 *   reserved[MOBI_ENC_PARTS_STAT_LEAVES]  leaves sent
 * In mode 0 reserved stays zero.
 */
#ifndef MOBICLIP_ENCODE_PARTS_H
#define MOBICLIP_ENCODE_PARTS_H
#include "mobiclip_encode_inter.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

enum { MOBI_ENC_PARTS_STAT_SPLIT = 0, MOBI_ENC_PARTS_STAT_LEAVES = 1 };

/* mode 0: every macroblock one 16x16 leaf; mode 1: partitions down to 8x8.  Holds for the calls of mobi_enc_inter_async / mobi_enc_inter
 * made after it; neither allocates.  MOBI_E_ARG for a NULL encoder or another mode. */
int mobi_enc_inter_set_partitions(mobi_enc_inter_ctx *e, int mode);
/* the mode; MOBI_E_ARG for a NULL encoder */
int mobi_enc_inter_get_partitions(const mobi_enc_inter_ctx *e);

/* Host only.  mobi_enc_inter_stream_bound for a mode: mode 0 gives that bound.  In mode 1 a macroblock is at most 4 + 2 x 4 bits of split
 * codes (the root and both halves), four leaves of 4 + 13 + 13 bits of partition code and vector difference, 13 of ue(cbp) and six blocks
 * of 1 + 64 levels of at most 28 bits each; header, tail and padding as there.  0 for refused dimensions or another mode. */
size_t mobi_enc_inter_stream_bound_partitions(uint32_t width, uint32_t height, int mode);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
