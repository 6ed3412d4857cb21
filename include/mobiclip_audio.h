/*
 * mobiclip_audio.h -- C ABI of the batched audio decode: the sound of many .moflex / .mods streams into device memory.
 *
 *   FastAudio   mirrors LibMobiclip.Codec.FastAudio.FastAudioDecoder (FastAudioDecoder.cs:41-311)
 *   IMA-ADPCM   mirrors MobiConverter.IMAADPCMDecoder (IMAADPCMDecoder.cs:17-50)
 *   PCM16       interleaved little-endian samples (Program.cs:152-156)
 *   framings    the converter's loops around them: Moflex (Program.cs:75-157), Mods (Program.cs:248-319)
 *
 * Bit-exact with the reference, its wrapping int32 arithmetic included.  Sx (Mods audio_codec 1) needs the file's codebooks: mobiclip_sx.h.
 * The packets come from host memory (what mobi_moflex_pop_frame / mobi_mods_read_frame hand out), the samples go to device memory on the
 * caller's stream; one lane per (stream, channel) decodes on the GPU, the decoder states live there.  Error codes: mobiclip_hip.h.
 */
#ifndef MOBICLIP_AUDIO_H
#define MOBICLIP_AUDIO_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: these declarations are all it exports */
#endif

typedef struct mobi_audio mobi_audio;

#define MOBI_AUDIO_FRAMING_MOFLEX 0 /* data[s] = one completed audio frame (chunk_id 2) with its two appended zero bytes */
#define MOBI_AUDIO_FRAMING_MODS 1   /* data[s] = the frame packet; the audio packets start at offsets[s], n_packets[s] of them */

/* codec numbers of this interface; Moflex codec_id c is MOBI_AUDIO_FASTAUDIO + c, Mods audio_codec 1, 2, 3 are SX, FASTAUDIO, IMA */
#define MOBI_AUDIO_FASTAUDIO 0
#define MOBI_AUDIO_IMA 1
#define MOBI_AUDIO_PCM16 2 /* Moflex framing only */
#define MOBI_AUDIO_SX 3    /* planned and created through mobiclip_sx.h; refused here: MOBI_E_UNSUPPORTED / NULL */

#define MOBI_AUDIO_S16 0 /* int16 */
#define MOBI_AUDIO_F32 1 /* float32 = sample / 32768, exact */

#define MOBI_AUDIO_PLANAR 0      /* dst[stream][channel][max_samples] */
#define MOBI_AUDIO_INTERLEAVED 1 /* dst[stream][max_samples][channel] */

#define MOBI_AUDIO_MAX_CHANNELS 8

/* One block of a frame: 40 (FastAudio) or 128 (IMA) bytes at data + offset giving 256 samples of `channel`.  header != 0: the 4-byte
 * IMA header (s16le index & 0x7F, s16le last) of that channel's new decoder is at data + header_offset. */
typedef struct {
  uint32_t offset;
  uint32_t header_offset;
  uint16_t channel;
  uint16_t header;
} mobi_audio_block;

/* The framing rules for ONE frame of ONE stream.  Host only: needs no GPU.  mobi_audio_decode plans every stream with this function.
 *   data, len    the frame (Moflex) or the frame packet (Mods)
 *   offset       Mods: where the audio packets start (Program.cs:250-252: the video decode's returned offset - 2, + 4 for tag 0x334E
 *                packets whose first word has bit 15 set); Moflex: ignored
 *   n_packets    Mods: NrAudioPackets; Moflex: ignored
 *   cursor       Mods: in: the channel of the first packet, out: that of the next frame's first (round robin); Moflex: ignored, may be NULL
 *   fresh        Mods IMA: fresh[c] != 0 = channel c's decoder is new, its next packet is 132 bytes (header, block); may be NULL (none is)
 *   blocks       receives the blocks in the reference's order, at most max_blocks of them (may be NULL with max_blocks 0: count only)
 *   n_blocks     the number of blocks the frame yields (also when it exceeds max_blocks)
 *   n_samples    [n_channels]: samples per channel (PCM16: len - len % (2 C) bytes' worth, the appended zeros included where they fit)
 * Returns MOBI_OK; MOBI_E_INDEX where the reference would throw -- a block or header that does not fit in len (a Moflex FastAudio
 * iteration that starts with fewer than 40 C bytes left is one), an IMA header index above 88 -- with n_blocks and n_samples zero and
 * the cursor unchanged; MOBI_E_UNSUPPORTED for Sx (mobi_sx_plan); MOBI_E_ARG for bad arguments (framing, codec, PCM16 in Mods framing, channels outside
 * [1, 8], a cursor outside [0, C), data NULL with len > 0).  len == 0 (and, in Mods framing, n_packets == 0) yields nothing: MOBI_OK. */
int mobi_audio_plan(int framing, int codec, int n_channels, const uint8_t *data, size_t len, size_t offset, uint32_t n_packets, int *cursor,
                    const uint8_t *fresh, mobi_audio_block *blocks, size_t max_blocks, size_t *n_blocks, int32_t *n_samples);

/* The constants of the formats as int32, for tests (host only).  which: 0 coefficients 0 and 1 (64 entries), 1 coefficient 2 (32),
 * 2 coefficient 3 (32), 3 coefficient 4 (16), 4 coefficient 5 (16), 5 coefficient 6 (8), 6 coefficient 7 (8), 7 pulses (512),
 * 8 IMA index (16), 9 IMA step (89).  Returns the number of entries (out may be NULL), or MOBI_E_ARG. */
int mobi_audio_table(int which, int32_t *out);

/* n_streams decoders of n_channels channels each on `device`, all new: states zero, Mods cursors 0.  NULL for bad arguments (as
 * mobi_audio_plan's; Sx, which mobi_sx_create makes; n_streams < 1 or n_streams * n_channels >= 2^24) or when the device cannot be used. */
mobi_audio *mobi_audio_create(int device, int framing, int codec, int n_streams, int n_channels);
void mobi_audio_destroy(mobi_audio *a);

/* New decoders for the listed streams (what a refilled slot calls beside mobi_batch_reset_clips; with keep_cursor = 1 what the
 * reference does at a Mods key frame with codec 3, Program.cs:255-265): FastAudio states zero, IMA reads its header again, the Mods
 * cursor 0 unless keep_cursor.  It takes effect in the next mobi_audio_decode, on that call's stream, and waits for nothing.
 * MOBI_E_ARG for count < 0, streams NULL with count > 0 or an index outside [0, n_streams), checked before anything changes. */
int mobi_audio_reset(mobi_audio *a, const int32_t *streams, int count, int keep_cursor);

/* One frame of every stream.  Plans each stream on the host, gathers the audio bytes alone into pinned staging (two buffers, each guarded
 * by an event: the call waits at most for the kernel of the call before the previous one), makes one host-to-device copy and launches on
 * `stream` (a hipStream_t; not one that is being captured).  The decoder states are one device array that the kernels of successive calls
 * read and write: a call's work is ordered behind the previous call's kernel (a stream wait on its event, no host wait), so the calls of
 * one handle may go to different streams; calls from several threads take the handle's lock in turn.
 *   data, len             [n_streams]; len[s] == 0 (or, Mods, n_packets[s] == 0): stream s decodes nothing and keeps its state
 *   offsets, n_packets    [n_streams], Mods framing only (NULL otherwise)
 *   dtype, layout         MOBI_AUDIO_S16 / F32, MOBI_AUDIO_PLANAR / INTERLEAVED
 *   dst, dst_bytes        device memory of the handle's device holding n_streams * n_channels * max_samples elements; samples beyond a
 *                         row's count are not written
 *   n_samples_out         [n_streams * n_channels], host: filled before the call returns (the counts are a function of the framing alone)
 *   rc                    [n_streams], host: MOBI_OK, or MOBI_E_INDEX (see mobi_audio_plan): that stream gets no samples and keeps its state
 *                         and cursor, as if the frame had never come; the other streams decode
 * Returns MOBI_OK, or refuses the whole call, with nothing enqueued and nothing changed: MOBI_E_ARG for bad arguments, a row that would
 * exceed max_samples, more than 65535 blocks for one channel, dst not device memory of this device or smaller than said, and for
 * MOBI_AUDIO_INTERLEAVED when the channels of a stream do not get equal counts (Moflex always does; Mods does when the cursor is 0 and
 * n_packets % C == 0); MOBI_E_DEVICE for a HIP failure. */
int mobi_audio_decode(mobi_audio *a, void *stream, const uint8_t *const *data, const size_t *len, const size_t *offsets,
                      const uint32_t *n_packets, int dtype, int layout, void *dst, size_t dst_bytes, size_t max_samples,
                      int32_t *n_samples_out, int *rc);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
