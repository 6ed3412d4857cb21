/*
 * mobiclip_audio_enc.h -- C ABI of the audio encoder: int16 samples in device memory (what mobi_audio_decode wrote, planar) to Moflex
 * audio frames, IMA-ADPCM (Moflex codec 1) or PCM16 (codec 2), in device memory, one frame per stream and call ("Audio encoder").
 *
 * A Moflex IMA frame is read by decoders made new for it (Program.cs:122-151, IMAADPCMDecoder.cs:20-28): C headers of 4 bytes (s16le
 * index, s16le last), then for block b and channel c the 128 bytes of 256 samples, low nibble first, at 4 C + 128 (b C + c).  So every
 * (stream, channel, frame) is independent and the encoder keeps no state between calls.  The rule, in csrc/mobi_audio_enc.h:
 *   nibble   the code of sample x is the val in 0..15 whose decoded, clamped sample is nearest to x; ties go to the smallest val
 *   header   last = x[0]; index = the i0 in 0..88 with the least squared error over block 0, ties to the smallest
 * A PCM16 frame is the samples interleaved as s16le.  The decoder, fed a frame plus the two zero bytes the demuxer appends, returns the
 * reported reconstruction -- for PCM16 with ONE channel also one more sample, 0, which the appended bytes make (mobi_audio_plan counts
 * it); the encoder does not work round that.
 *
 * FastAudio, Sx and the Mods framing (audio packets inside the video packet) are not written: MOBI_E_UNSUPPORTED.  Error codes: mobiclip_hip.h.
 */
#ifndef MOBICLIP_AUDIO_ENC_H
#define MOBICLIP_AUDIO_ENC_H
#include "mobiclip_audio.h"
#include "mobiclip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef struct mobi_audio_enc mobi_audio_enc;

/* per (stream, channel) of a call, 16 bytes */
typedef struct {
  uint64_t sse;         /* the squared error over the frame's 256 B samples */
  uint32_t clamped;     /* samples at which the decoder's clamp to int16 acts */
  uint32_t start_index; /* the header's index */
} mobi_audio_enc_stats;

/* One small device allocation, made here.  codec: MOBI_AUDIO_IMA or MOBI_AUDIO_PCM16; n_channels in [1, 8]; n_streams >= 1 with
 * n_streams * n_channels < 2^24; max_blocks in [1, 65535] (blocks of 256 samples per channel and call).  NULL for refused arguments
 * (mobi_audio_enc_check says which), no device, or no memory. */
mobi_audio_enc *mobi_audio_enc_create(int device, int codec, int n_streams, int n_channels, int max_blocks);
void mobi_audio_enc_destroy(mobi_audio_enc *e);

/* Host only.  The length of a frame of `blocks` blocks per channel: 4 C + 128 C blocks (IMA), 512 C blocks (PCM16); 0 for another codec,
 * channels outside [1, 8] or blocks < 1. */
size_t mobi_audio_enc_frame_bytes(int codec, int n_channels, int blocks);

/* Host only: every refusal of the create and the encode call that needs no device, in their order.  MOBI_E_UNSUPPORTED for FastAudio and
 * Sx; MOBI_E_ARG for another codec, channels outside [1, 8], n_streams or max_blocks as above, and for the encode call's own (below). */
int mobi_audio_enc_check(int codec, int n_streams, int n_channels, int max_blocks, int n, const int16_t *samples, size_t sample_pitch, int blocks,
                         const uint8_t *slots, size_t slot_pitch, size_t slot_bytes, const int32_t *sizes, const int16_t *recon, size_t recon_pitch,
                         const void *stats);

/* One frame of `blocks` blocks per channel for each of the streams 0 .. n - 1.  All pointers DEVICE memory.
 *   samples, sample_pitch   int16, sample k of channel c of stream s at samples[(s C + c) sample_pitch + k]: a planar mobi_audio_decode
 *                           output with max_samples = sample_pitch is encoded where it lies; 2-byte aligned
 *   slots, slot_pitch,      the video encoders' convention, which mobi_mux_append_audio_async takes unchanged: n rows of slot_bytes at
 *   slot_bytes, sizes       slot_pitch, the frame at the row's start, bytes behind it untouched; sizes int32[n], the frames' lengths;
 *                           both 4-byte aligned, slot_pitch and slot_bytes multiples of 4
 *   recon, recon_pitch      NULL, or int16 laid out as samples: what a decoder returns for the frame; 2-byte aligned
 *   stats                   NULL, or mobi_audio_enc_stats[n C], 8-byte aligned
 * Enqueues on `stream` (a hipStream_t), allocates nothing, waits for nothing and reads no device value.  The object's scratch (the chosen
 * header indices) is written by every call: the calls of one object belong on one stream, or are ordered by the caller.
 * Refusals, with nothing enqueued -- MOBI_E_ARG: e NULL, NULL or misaligned pointers, n outside [1, n_streams], blocks outside
 * [1, max_blocks], sample_pitch (recon_pitch) below 256 blocks, slot_bytes below the frame or no multiple of 4, slot_pitch below
 * slot_bytes or no multiple of 4; MOBI_E_DEVICE for a HIP failure. */
int mobi_audio_enc_async(mobi_audio_enc *e, void *stream, int n, const int16_t *samples, size_t sample_pitch, int blocks, uint8_t *slots,
                         size_t slot_pitch, size_t slot_bytes, int32_t *sizes, int16_t *recon, size_t recon_pitch, mobi_audio_enc_stats *stats);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
