/*
 * mobiclip_mux_audio.h -- C ABI of the muxer's second Moflex stream: audio frames (what mobi_audio_enc_async leaves in device memory,
 * mobiclip_audio_enc.h) appended to the file images of mobiclip_mux.h as stream index 1 ("Muxing").  One audio stream, Moflex
 * only: a Mods file carries its audio packets inside the video packets, which this muxer does not write.
 *
 * With audio on, the head is 38 bytes: behind the video chunk come the variable bytes 2 and 6 and the MoLiveStreamAudio chunk (stream index
 * 1, codec id, frequency - 1 as a big-endian u24, channels - 1: MoLiveStreamAudio.cs:29-37), then the two terminating zero bytes.  A frame
 * of stream 1 is framed exactly as one of stream 0 -- blocks of at most 0xF80 payload bytes, EP headers of 2 bytes or, on the block that
 * ends the frame, 6 -- with the index bit set: the last block starts F2 00 00 00 where video has B2 00 00 00.  So mobi_mux_framed_bytes
 * holds for both streams.  Time stamp deltas are zero, as in the reference's muxer.  Frames lie in the file in the order of the append
 * calls.  A muxer on which audio was never switched on writes what it wrote without this header.
 */
#ifndef MOBICLIP_MUX_AUDIO_H
#define MOBICLIP_MUX_AUDIO_H
#include "mobiclip_mux.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Host only; between sessions (before a begin or after a finish), holds from the next begin on.  codec_id: the Moflex number, 0 FastAudio,
 * 1 IMA-ADPCM, 2 PCM16 (the muxer never looks inside a frame); frequency in [1, 2^24]; channels in [1, 8].  frequency == 0 switches audio
 * off again (codec_id and channels are then ignored).
 * MOBI_E_UNSUPPORTED: a Mods muxer.  MOBI_E_ARG: m NULL, a session begun and not finished, a value outside its range. */
int mobi_mux_set_audio(mobi_mux *m, int codec_id, uint32_t frequency, int channels);

/* Host only.  mobi_mux_fixed_bytes, plus the 8 bytes of the audio chunk when audio != 0 (Moflex).  0 for an unknown container, and for
 * Mods with audio != 0. */
size_t mobi_mux_fixed_bytes_audio(int container, int key_frames, int audio);

/* Appends one audio frame to each of the clips 0 .. n - 1, as stream index 1.  Arguments, alignment rules, the predicate, the status
 * bits and the refusals of mobi_mux_append_async (there is no key_frame).  MOBI_E_ARG also when audio is off. */
int mobi_mux_append_audio_async(mobi_mux *m, void *stream, int n, const uint8_t *slots, size_t slot_pitch, size_t slot_bytes, const int32_t *sizes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
