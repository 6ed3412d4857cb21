/*
 * mobiclip_encode_rate.h -- C ABI of the encoders' rate control: the calls of mobiclip_encode.h and mobiclip_encode_inter.h with a byte
 * target per picture in place of a quantiser per picture.  The quantiser is chosen on the device, by a bisection over real trial encodes
 * ("Rate control"), and the host model makes the same choice byte for byte.
 *
 * The rule, per picture: lo = qmin, hi = qmax; K = mobi_enc_rate_rounds(qmin, qmax) rounds; in each the picture is encoded at
 * mid = (lo + hi) >> 1 (a P-frame with its real previous quantiser and reference) and fits when its stream is no longer than the target:
 * then hi = mid, else lo = min(mid + 1, hi).  After K rounds lo == hi: q_out, at which the picture is encoded for good.
 * A stream's length is not monotone in the quantiser, so the promise is procedural: q_out is what this bisection returns; the stream at
 * q_out is no longer than the target, or q_out == qmax.  It is not always the smallest quantiser that fits.  A target <= 0 fits nothing.
 * With qmin == qmax there is no trial and the call is the fixed-quantiser call byte for byte.
 *
 * Error codes: mobiclip_hip.h.
 */
#ifndef MOBICLIP_ENCODE_RATE_H
#define MOBICLIP_ENCODE_RATE_H
#include "mobiclip_encode.h"
#include "mobiclip_encode_inter.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Host only.  The trial encodes per picture of a call with this range: the smallest k with 2^k >= qmax - qmin + 1 (0 .. 6), the same for
 * every picture.  -1 for a range the calls refuse: qmin or qmax outside [12, 52], or qmin > qmax. */
int mobi_enc_rate_rounds(int qmin, int qmax);

/* mobi_enc_intra_async with targets.  Device pointers, everything enqueued on `stream`, returns after the enqueue: no allocation, no
 * wait, and the host reads no device value.
 *   target_bytes    DEVICE memory, int32[n], 4-byte aligned: the byte target of picture i
 *   qmin, qmax      the range of the call, 12 <= qmin <= qmax <= 52
 *   quantizers_out  DEVICE memory, uint8[n], required: q_out
 * Everything else as in mobi_enc_intra_async: slots (only the final encode writes them), bytes_out, recon_i420 and stats hold the final
 * encode only.  MOBI_E_ARG also for a refused range and for target_bytes or quantizers_out NULL or misaligned. */
int mobi_enc_intra_target_async(mobi_enc *e, void *stream, int n, const uint8_t *i420, size_t picture_pitch, const int32_t *target_bytes, int qmin,
                                int qmax, int yuv_format, uint8_t *streams, size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420,
                                mobi_enc_stats *stats, uint8_t *quantizers_out);

/* mobi_enc_inter_async with targets, in partition mode 0 and 1.
 *   prev_quantizers DEVICE memory, uint8[n]: the quantiser of the frame before picture i -- the quantizers_out of the call that made the
 *                   reference, which is how a clip chains without a wait.  An entry outside [12, 52] is clamped into it before use.
 *   target_bytes, qmin, qmax, quantizers_out as above; everything else as in mobi_enc_inter_async. */
int mobi_enc_inter_target_async(mobi_enc_inter_ctx *e, void *stream, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *ref_i420,
                                size_t ref_pitch, const uint8_t *prev_quantizers, const int32_t *target_bytes, int qmin, int qmax, uint8_t *streams,
                                size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_inter_stats *stats, uint8_t *quantizers_out);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
