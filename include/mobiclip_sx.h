/*
 * mobiclip_sx.h -- C ABI of the batched Sx audio decode: Mods audio_codec 1, the sound of many .mods streams into device memory.
 *
 *   Sx          mirrors LibMobiclip.Codec.Sx.SxDecoder (SxDecoder.cs:42-476): a packet of 10, 12, 14 or 20 bytes gives 128 samples
 *   framing     the converter's loop around it (Program.cs:275-288): one packet per channel, round robin
 *
 * An Sx decoder needs its channel's codebook from the file (mobi_mods_audio_codebook of mobiclip_demux.h: MOBI_MODS_CODEBOOK_BYTES), so it
 * has entry points of its own for planning, creating and refilling.  The handle is mobiclip_audio.h's: mobi_audio_decode, mobi_audio_reset
 * and mobi_audio_destroy take a handle made here, and every rule mobi_audio_decode states holds (per-stream MOBI_E_INDEX, whole-call
 * refusals, equal counts for the interleaved layout, at most 65535 blocks -- here: packets -- per channel of a call).  Bit-exact with the
 * reference, its wrapping int32 arithmetic and the state that survives its reset packets included.  Error codes: mobiclip_hip.h.
 */
#ifndef MOBICLIP_SX_H
#define MOBICLIP_SX_H
#include <stddef.h>
#include <stdint.h>

#include "mobiclip_audio.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define MOBI_SX_PACKET_SAMPLES 128

/* The Mods framing for ONE frame of ONE stream.  Host only: needs no GPU.  mobi_audio_decode plans every stream of an Sx handle with it.
 *   data, len    the frame packet
 *   offset       where the audio packets start (as mobi_audio_plan's)
 *   n_packets    NrAudioPackets: that many packets from offset, dealt to the channels round robin from the cursor; the length of each
 *                (20, 14, 12, 10 bytes for rate 0, 1, 2, 3) comes from bits 13..12 of its own second word
 *   cursor       in: the channel of the first packet, out: that of the next frame's first
 *   blocks       receives one block per packet in the reference's order, at most max_blocks: offset = the packet's start, header = 0
 *                (may be NULL with max_blocks 0: count only)
 *   n_blocks     the number of packets; n_samples [n_channels]: MOBI_SX_PACKET_SAMPLES per packet of that channel
 * Returns MOBI_OK; MOBI_E_INDEX where the reference would read past the buffer -- fewer than 4 bytes left at a packet's start, or a packet
 * whose bytes do not fit in len -- with n_blocks and n_samples zero and the cursor unchanged; MOBI_E_ARG for bad arguments (channels
 * outside [1, 8], cursor NULL or outside [0, C), data NULL with len > 0, blocks NULL with max_blocks > 0).  len == 0 or n_packets == 0
 * yields nothing: MOBI_OK. */
int mobi_sx_plan(int n_channels, const uint8_t *data, size_t len, size_t offset, uint32_t n_packets, int *cursor, mobi_audio_block *blocks,
                 size_t max_blocks, size_t *n_blocks, int32_t *n_samples);

/* n_streams Sx decoders of n_channels channels each on `device`, all new: states zero, cursors 0.  A new decoder may be handed a packet
 * that is no reset packet: it decodes from zeros (gain 0: silence), as the reference's does.
 *   codebooks    [n_streams * n_channels] pointers, [s * n_channels + c] = MOBI_MODS_CODEBOOK_BYTES bytes of host memory for channel c of
 *                stream s; copied to the device before the call returns
 * NULL for the arguments mobi_audio_create refuses, for codebooks NULL or any NULL entry (the reference dereferences a null
 * AudioCodebooks when the file has none), or when the device cannot be used. */
mobi_audio *mobi_sx_create(int device, int n_streams, int n_channels, const uint8_t *const *codebooks);

/* New decoders WITH NEW CODEBOOKS for the listed streams: what a refilled slot calls beside mobi_batch_reset_clips.
 *   codebooks    [count * n_channels] pointers, [i * n_channels + c] = channel c of streams[i]; copied before the call returns
 * States zero, cursor 0.  It takes effect in the next mobi_audio_decode, on that call's stream, and waits for nothing.  MOBI_E_ARG for a
 * handle of another codec, count < 0, streams or codebooks NULL with count > 0, an index outside [0, n_streams), a NULL entry: checked
 * before anything changes.  mobi_audio_reset on an Sx handle gives new decoders that keep their codebooks.  The reference never makes new
 * Sx decoders in a file, not at key frames either (Program.cs:253-288: only codec 3 does), so a caller that follows it resets only when a
 * slot gets another file. */
int mobi_sx_reset(mobi_audio *a, const int32_t *streams, int count, const uint8_t *const *codebooks);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
