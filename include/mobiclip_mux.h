/*
 * mobiclip_mux.h -- C ABI of the muxer: the streams the encoders leave in device memory, framed into .moflex / .mods file images that
 * are built up in device memory, one frame per call, and cross to the host once ("Muxing").  Video only, one stream, stream
 * index 0, no audio.  Moflex carries MOBI_VERSION_MOFLEX3DS streams, Mods MOBI_VERSION_MODSDS; the muxer never looks inside a stream.
 *
 * Moflex: a 30-byte head (synchro header with time stamp 1 and packet-size field 0x1000, one MoLiveStreamVideo chunk, the terminator),
 * per frame blocks of at most 0xF80 payload bytes (flag byte 1, an EP header of 2 bytes or -- on the block that ends the frame -- 6, the
 * payload, a zero byte), and 0x1000 zero bytes behind the last frame.  Mods: the 0x30-byte header, per frame a u32 `length << 14` and the
 * stream, the key-frame index of (frame number, offset) pairs behind the last frame.
 *
 * A clip's state (write position, frame count, largest frame, key-frame table, a sticky status word) lives in the muxer object, in
 * device memory.  A clip whose status is not 0 is written no further, its file length is reported as 0, and the other clips are unaffected.
 * No byte at or behind a clip's capacity is ever written; bytes between a clean clip's file length and its capacity are unspecified.
 *
 * Every _async call enqueues on the caller's stream, allocates nothing, waits for nothing and reads no device value on the host.
 * Error codes: mobiclip_hip.h.
 */
#ifndef MOBICLIP_MUX_H
#define MOBICLIP_MUX_H
#include "mobiclip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define MOBI_MUX_MOFLEX 0
#define MOBI_MUX_MODS 1

/* status bits of a clip */
#define MOBI_MUX_ST_CAPACITY 1 /* the frame, or finish's tail, would pass the clip's capacity */
#define MOBI_MUX_ST_STREAM 2   /* the frame's length is <= 0 or above slot_bytes: what an encoder leaves when a stream did not fit its slot */
#define MOBI_MUX_ST_FRAME 4    /* a Mods frame of 2^18 bytes or more: the length field is 18 bits wide */
#define MOBI_MUX_ST_KEYS 8     /* more key frames than the table holds */

typedef struct mobi_mux mobi_mux;

/* One device allocation, made here.  width, height, fps_rate, fps_scale below 65536 for Moflex (fps_raw is the Mods header's fps word);
 * max_clips in [1, 65535]; max_key_frames >= 0 (the table of one clip; Moflex keeps none).  NULL for refused arguments, no device, or
 * no memory. */
mobi_mux *mobi_mux_create(int container, uint32_t width, uint32_t height, uint32_t fps_rate, uint32_t fps_scale, uint32_t fps_raw, int max_clips,
                          int max_key_frames, int device);
void mobi_mux_destroy(mobi_mux *m);

/* Host only.  What a frame of stream_bytes occupies in the file; head plus tail (Moflex) or header plus an index of key_frames entries
 * (Mods).  A file of T frames is mobi_mux_fixed_bytes + the sum of mobi_mux_framed_bytes long.  0 for an unknown container. */
size_t mobi_mux_framed_bytes(int container, size_t stream_bytes);
size_t mobi_mux_fixed_bytes(int container, int key_frames);

/* Starts n files.  files: DEVICE memory, n rows of file_capacity bytes at a pitch of file_pitch >= file_capacity, any alignment.  Resets
 * the state of clips 0 .. n - 1, writes the Moflex head (Mods: reserves the header) and remembers the rows.
 * MOBI_E_ARG: m or files NULL, n outside [1, max_clips], file_pitch < file_capacity, Mods with file_capacity >= 2^32 (offsets are u32). */
int mobi_mux_begin_async(mobi_mux *m, void *stream, int n, uint8_t *files, size_t file_pitch, size_t file_capacity);

/* Appends one frame to each of the clips 0 .. n - 1.  slots, sizes: DEVICE memory, exactly the (n, slot_bytes) bytes at a pitch of
 * slot_pitch and the int32[n] lengths an encoder call wrote; both 4-byte aligned, slot_pitch and slot_bytes multiples of 4.  They are
 * read on the device: the call may follow the encode call on its stream without a wait.  key_frame (0 / 1) holds for every clip of the
 * call; Moflex ignores it.
 * MOBI_E_ARG: NULL or misaligned pointers, n outside [1, the n of begin], slot_pitch < slot_bytes, slot_bytes == 0, no begin. */
int mobi_mux_append_async(mobi_mux *m, void *stream, int n, const uint8_t *slots, size_t slot_pitch, size_t slot_bytes, const int32_t *sizes,
                          int key_frame);

/* Ends the files: the Moflex tail, or the Mods header and index; then file_bytes_out[i] (DEVICE memory, int64[n], 8-byte aligned: the
 * file's length, 0 for a clip with a status) and status_out[i] (DEVICE memory, int32[n], 4-byte aligned: MOBI_MUX_ST_* bits).  The next
 * call must be a begin.
 * MOBI_E_ARG: NULL or misaligned pointers, n other than the n of begin, no begin. */
int mobi_mux_finish_async(mobi_mux *m, void *stream, int n, int64_t *file_bytes_out, int32_t *status_out);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
