/*
 * mobiclip_encode_pintra.h -- C ABI of the inter encoder's intra mode: an opt-in mode of a mobi_enc_inter_ctx (mobiclip_encode_inter.h) in
 * which a macroblock of a P-frame is sent either as that header's encoder sends it (the search's vector, an 8x8-transform residual) or as
 * an intra macroblock: partition code 6, then what the I-frame encoder (mobiclip_encode.h) writes for a macroblock behind its leading bit.
 * Mode 0, the state after mobi_enc_inter_create, is that header's encoder byte for byte.
 *
 * In mode 1 a macroblock is sent intra iff the intra coding's integer cost is strictly below the inter coding's ("Inter
 * encoder", "Intra macroblocks"); the intra coding predicts from this P-frame's own reconstruction of the macroblocks to its left and
 * above.  An intra macroblock counts as the zero vector in its neighbours' predictors.  The contract stays: every stream decodes to
 * exactly the reconstruction the encoder reports.  mobi_enc_inter_stream_bound holds in both modes.
 *
 * Statistics in mode 1 (mobi_enc_inter_stats): sad, coded_blocks and fallback_* describe the chosen coding; mv_bits holds every
 * macroblock's partition code, code 6 too; code0, nonzero_mv and halfpel_mv count inter macroblocks only, and
 *   reserved[MOBI_ENC_PINTRA_STAT_INTRA]  macroblocks sent intra
 * In mode 0 reserved stays as it is without this header.
 *
 * The intra mode and the partition mode (mobiclip_encode_parts.h) exclude each other: turning either on while the other is on is refused.
 */
#ifndef MOBICLIP_ENCODE_PINTRA_H
#define MOBICLIP_ENCODE_PINTRA_H
#include "mobiclip_encode_inter.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

enum { MOBI_ENC_PINTRA_STAT_INTRA = 2 };

/* mode 0: every macroblock inter; mode 1: intra where it is cheaper.  Holds for the calls of mobi_enc_inter_async, mobi_enc_inter and
 * mobi_enc_inter_target_async made after it; allocates nothing.  MOBI_E_ARG for a NULL encoder, another mode, or mode 1 while the
 * partition mode is on (nothing changes then). */
int mobi_enc_inter_set_intra(mobi_enc_inter_ctx *e, int mode);
/* the mode; MOBI_E_ARG for a NULL encoder */
int mobi_enc_inter_get_intra(const mobi_enc_inter_ctx *e);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
