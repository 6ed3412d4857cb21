/*
 * mobiclip_encode.h -- C ABI of the intra encoder: a batch of I420 pictures in device memory to Mobiclip I-frames, one stream per picture.
 *
 * The contract: every stream decodes -- in the reference decoder and in this library's -- to exactly the reconstruction the encoder
 * reports, and every decision is the argmin of an integer cost ("Intra encoder").  It is NOT MobiEncoder.EncodeIntra bit for
 * bit.  I-frames only, MOBI_VERSION_MOFLEX3DS and MOBI_VERSION_MODSDS; full-block syntax, 8x8 transforms, VLC table 0; luma and chroma
 * modes 0 (vertical), 1 (horizontal) and 3 (DC).  Error codes: mobiclip_hip.h.
 */
#ifndef MOBICLIP_ENCODE_H
#define MOBICLIP_ENCODE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef struct mobi_enc mobi_enc;

/* per picture */
typedef struct mobi_enc_stats {
  uint64_t bits;             /* header + macroblocks: the stream without its trailing zeros */
  uint64_t sad;              /* sum |source - reconstruction| over Y, U and V */
  uint32_t luma_modes[4];    /* macroblocks by chosen luma mode number (entry 2 stays 0) */
  uint32_t chroma_modes[4];  /* ... by chosen chroma mode */
  uint32_t coded_blocks;     /* 8x8 blocks sent with levels */
  uint32_t fallback_clamp;   /* blocks sent uncoded because their reconstruction would leave the decoder's clamp table */
  uint32_t fallback_level;   /* ... because a level would not fit the 12-bit raw escape (and the clamp did not already refuse it) */
  uint32_t reserved;
} mobi_enc_stats;

/* An encoder for up to max_pictures pictures per call of width x height (multiples of 16, width <= 1024) on `device`.  All device memory
 * is allocated here; no call allocates.  NULL for arguments that the check below refuses or when the device cannot be used. */
mobi_enc *mobi_enc_create(int max_pictures, uint32_t width, uint32_t height, int version, int device);
void mobi_enc_destroy(mobi_enc *e);

/* Host only.  An upper bound of one stream's bytes; a multiple of 4, so it serves as slot_bytes.  0 for dimensions the encoder refuses.
 * A macroblock is at most 1 + 13 + 3 + 3 bits of syntax and six blocks of 1 + 64 levels of at most 28 bits each; the header is 9 bits,
 * the tail 16, the padding below 16. */
size_t mobi_enc_stream_bound(uint32_t width, uint32_t height);

/* Host only: every refusal of the two calls below that needs no device.  MOBI_OK or MOBI_E_ARG (MOBI_E_VERSION for a version other than
 * the two above): dimensions as for the create call, max_pictures outside [1, 65535], n outside [1, max_pictures], picture_pitch < width * height * 3 / 2
 * or no multiple of 8, quantizers NULL or one outside [12, 52], yuv_format outside {0, 1}, slot_bytes no multiple of 4. */
int mobi_enc_check(int max_pictures, uint32_t width, uint32_t height, int version, int n, size_t picture_pitch, const uint8_t *quantizers,
                   int yuv_format, size_t slot_bytes);

/* Encode n pictures; device pointers, everything enqueued on `stream`, returns after the enqueue.
 *   i420           8-byte aligned; picture i at i420 + i * picture_pitch: packed Y (width x height), U, V (width / 2 x height / 2 each), pitch = plane width
 *   quantizers     HOST memory, n entries, read before the call returns
 *   streams        n slots of slot_bytes (4-byte aligned): the stream, then zeros to the slot's end; a stream longer than slot_bytes
 *                  leaves its slot all zero, which is no error of the call
 *   bytes_out      [n] the stream's true length, always
 *   recon_i420     NULL, or n pictures packed as the input at pitch width * height * 3 / 2: what every decoder makes of stream i
 *   stats          NULL, or [n]
 * MOBI_E_ARG for what the check refuses and for NULL or misaligned required pointers; MOBI_E_DEVICE for a HIP error. */
int mobi_enc_intra_async(mobi_enc *e, void *stream, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *quantizers, int yuv_format,
                         uint8_t *streams, size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_stats *stats);

/* The same with host pointers, synchronous.  It copies through device memory that its first call allocates for max_pictures
 * and keeps (the slots' copy grows with the largest slot_bytes seen); recon_i420 and stats may be NULL. */
int mobi_enc_intra(mobi_enc *e, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *quantizers, int yuv_format, uint8_t *streams,
                   size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_stats *stats);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
