/*
 * mobiclip_encode_inter.h -- C ABI of the inter encoder: a batch of I420 pictures in device memory, each with the reconstruction of the
 * frame before it, to Mobiclip P-frames, one stream per picture.
 *
 * The contract is the intra encoder's (mobiclip_encode.h): every stream decodes -- in the reference decoder and in this library's, behind
 * the frame whose reconstruction was given as the reference -- to exactly the reconstruction the encoder reports, and every decision is the
 * argmin of an integer cost ("Inter encoder").  It is NOT MobiEncoder.EncodeInter bit for bit.  MOBI_VERSION_MOFLEX3DS and
 * MOBI_VERSION_MODSDS; one reference (the previous frame), every macroblock one 16x16 leaf with a vector of at most 17 half-pels either
 * way whose three windows lie inside the picture, 8x8 transforms, VLC table 0.  Error codes: mobiclip_hip.h.
 * mobiclip_encode_parts.h adds an opt-in mode of the same encoder object in which a macroblock may be split down to 8x8 leaves; what is
 * said here holds for mode 0, the state after create.
 */
#ifndef MOBICLIP_ENCODE_INTER_H
#define MOBICLIP_ENCODE_INTER_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef struct mobi_enc_inter_ctx mobi_enc_inter_ctx;

/* per picture, 64 bytes */
typedef struct mobi_enc_inter_stats {
  uint64_t bits;             /* header + macroblocks: the stream without its trailing zeros */
  uint64_t sad;              /* sum |source - reconstruction| over Y, U and V */
  uint64_t mv_bits;          /* of those bits: the partition codes and the vector differences */
  uint32_t coded_blocks;     /* 8x8 blocks sent with levels */
  uint32_t fallback_clamp;   /* blocks sent uncoded because their reconstruction would leave the decoder's clamp table */
  uint32_t fallback_level;   /* ... because a level would not fit the 12-bit raw escape (and the clamp did not already refuse it) */
  uint32_t code0;            /* macroblocks sent with partition code 0: the vector is the predictor */
  uint32_t nonzero_mv;       /* macroblocks whose vector is not (0, 0) */
  uint32_t halfpel_mv;       /* macroblocks whose vector has an odd component */
  uint32_t reserved[4];
} mobi_enc_inter_stats;

/* An encoder for up to max_pictures pictures per call of width x height (multiples of 16, width <= 1024) on `device`.  All device memory
 * is allocated here; no call allocates.  NULL for arguments that the check below refuses or when the device cannot be used. */
mobi_enc_inter_ctx *mobi_enc_inter_create(int max_pictures, uint32_t width, uint32_t height, int version, int device);
void mobi_enc_inter_destroy(mobi_enc_inter_ctx *e);

/* Host only.  An upper bound of one stream's bytes; a multiple of 4, so it serves as slot_bytes.  0 for dimensions the encoder refuses.
 * A macroblock is at most 3 + 13 + 13 bits of partition code and vector difference, 13 of ue(cbp) and six blocks of 1 + 64 levels of at
 * most 28 bits each; the header is at most 1 + 13 bits, the tail 16, the padding below 16. */
size_t mobi_enc_inter_stream_bound(uint32_t width, uint32_t height);

/* Host only: every refusal of the two calls below that needs no device.  MOBI_OK or MOBI_E_ARG (MOBI_E_VERSION for a version other than
 * the two above): dimensions as for the create call, max_pictures outside [1, 65535], n outside [1, max_pictures], picture_pitch or
 * ref_pitch < width * height * 3 / 2 or no multiple of 8, prev_quantizers or quantizers NULL or an entry outside [12, 52], slot_bytes no
 * multiple of 4. */
int mobi_enc_inter_check(int max_pictures, uint32_t width, uint32_t height, int version, int n, size_t picture_pitch, size_t ref_pitch,
                         const uint8_t *prev_quantizers, const uint8_t *quantizers, size_t slot_bytes);

/* Encode n pictures; device pointers, everything enqueued on `stream`, returns after the enqueue.
 *   i420             8-byte aligned; picture i at i420 + i * picture_pitch: packed Y (width x height), U, V (width / 2 x height / 2 each)
 *   ref_i420         8-byte aligned; at ref_i420 + i * ref_pitch, packed alike: what the decoder holds as its newest frame when it meets
 *                    stream i -- the reconstruction the encoder (intra or inter) reported for the frame before
 *   prev_quantizers  HOST memory, n entries: the quantiser of the frame before picture i (the header sends the difference)
 *   quantizers       HOST memory, n entries; both are read before the call returns
 *   streams          n slots of slot_bytes (4-byte aligned): the stream, then zeros to the slot's end; a stream longer than slot_bytes
 *                    leaves its slot all zero, which is no error of the call
 *   bytes_out        [n] the stream's true length, always
  *   recon_i420       NULL, or (8-byte aligned) n pictures packed as the input at pitch width * height * 3 / 2; must not overlap ref_i420
 *   stats            NULL, or [n]
 * MOBI_E_ARG for what the check refuses and for NULL or misaligned required pointers; MOBI_E_DEVICE for a HIP error. */
int mobi_enc_inter_async(mobi_enc_inter_ctx *e, void *stream, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *ref_i420,
                         size_t ref_pitch, const uint8_t *prev_quantizers, const uint8_t *quantizers, uint8_t *streams, size_t slot_bytes,
                         int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_inter_stats *stats);

/* The same with host pointers, synchronous.  It copies through device memory that its first call allocates for max_pictures
 * and keeps (the slots' copy grows with the largest slot_bytes seen); recon_i420 and stats may be NULL. */
int mobi_enc_inter(mobi_enc_inter_ctx *e, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *ref_i420, size_t ref_pitch,
                   const uint8_t *prev_quantizers, const uint8_t *quantizers, uint8_t *streams, size_t slot_bytes, int32_t *bytes_out,
                   uint8_t *recon_i420, mobi_enc_inter_stats *stats);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
