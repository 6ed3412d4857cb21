/*
 * mobiclip_hip.h -- C ABI of libmobiclip_hip.so: MI355X (gfx950) Mobiclip frame reconstruction.
 *
 * The reference has no FFI seam; the seam is the public surface of
 *   LibMobiclip.Codec.Mobiclip.MobiclipDecoder   (MobiclipDecoder.cs:13-61, "MD.cs")
 * whose callers do   d.Data = frame; d.Offset = o; d.DecodeFrame(); ... d.Offset ...
 * (MobiConverter/Program.cs:69-71,243-250,393-395; MobiclipDecoder/Form1.cs:261-263,292-302,
 * 359-364,463-465,525-527).  Each entry point below names the member it replaces; the C#
 * binding a maintainer would add is in INTEGRATION.md.
 *
 * Split of work: the serial VLC / Exp-Golomb parse (MD.cs bit reader and syntax, :113-259,
 * :469-3432) runs on the host inside these calls and emits a flat per-macroblock command list;
 * dequant + inverse transforms, intra prediction, motion compensation and residual add
 * (MD.cs:418-456, :1883-2774, :3017-3327, :3435-3798) run as HIP kernels (one wavefront per eight
 * adjacent inter macroblocks, one per four intra macroblocks).  There is NO CPU reconstruction path in this library: without a HIP device every
 * create call fails.
 */
#ifndef MOBICLIP_HIP_H
#define MOBICLIP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: these declarations are all it exports */
#endif

/* MobiclipDecoder.MobiclipVersion, MD.cs:32-37 */
#define MOBI_VERSION_VXDS 0      /* unimplemented stub in the reference too (MD.cs:63-95) */
#define MOBI_VERSION_MODSDS 1
#define MOBI_VERSION_MOFLEX3DS 2

/* Return codes.  0 = frame decoded.  Negative = the reference would have thrown inside
 * DecodeVXS2 and returned a null Bitmap (MD.cs:325-328); the code says which check fired. */
#define MOBI_OK 0
#define MOBI_IDLE 1              /* not an error: the frame slot was marked idle (mobi_batch_set_idle) -- nothing parsed, nothing written */
#define MOBI_E_INDEX (-1)        /* managed array bounds: MC source window, intra neighbour at a negative
                                    offset, VLC/CBP/quantizer table index, bitstream read past Data */
#define MOBI_E_NULLREF (-2)      /* reference frame slot Y[ref] never decoded (MD.cs:413) */
#define MOBI_E_PARTCODE (-3)     /* illegal partition code: explicit throw (e.g. MD.cs:625,730,827) */
#define MOBI_E_VERSION (-4)      /* VxDS / unknown version */
#define MOBI_E_CLAMP (-5)        /* residual add left the clamp table domain (MobiConst.cs:587; MD.cs:3551);
                                    detected on the GPU, so the parser state has already advanced */
#define MOBI_E_UNSUPPORTED (-6)  /* the reference decodes this frame to something and this library refuses.  r05: ONE input is left -- a
                                    coefficient run that walks through `Internal` (MD.cs:3424-3429) and leaves a coefficient beyond
                                    int16 in a block whose residual nevertheless stays within +-319 everywhere (so that the clamp
                                    table need not fault): sums that cancel through 32-bit wrap-around; never seen in 40 000 corrupted
                                    frames.  Everything r01-r04 refused is decoded, wherever the parse runs (error table) */
#define MOBI_E_ARG (-7)          /* bad argument / dimensions not a multiple of 16 (the reference cannot
                                    decode those either: MD.cs:216-217) */
#define MOBI_E_DEVICE (-8)       /* HIP error (no device, allocation, launch) */

typedef struct mobi_dec mobi_dec;     /* one stream: replaces one MobiclipDecoder instance */
typedef struct mobi_batch mobi_batch; /* N independent streams of equal geometry, decoded in lock step */

/* ---- single stream ------------------------------------------------------------------------ */
/* new MobiclipDecoder(Width, Height, Version)  (MD.cs:41-54).  device = HIP ordinal. */
mobi_dec *mobi_create(uint32_t width, uint32_t height, int version, int device);
void mobi_destroy(mobi_dec *d);
/* d.Data = data (len bytes); d.Offset = *offset_inout; d.DecodeFrame(); *offset_inout = d.Offset
 * (MD.cs:56-61, 97-259).  Synchronous: returns after the frame is reconstructed on the device. */
int mobi_decode(mobi_dec *d, const uint8_t *data, size_t len, int32_t *offset_inout);
/* d.Y[ring_idx] / d.UV[ring_idx]  (MD.cs:19-20), copied in the reference layout:
 * y_out: Stride*Height bytes; uv_out: Stride*Height/2 bytes, U in columns [0,Stride/2), V in
 * [Stride/2,Stride) of each row (MD.cs:414-415).  Either pointer may be NULL.
 * Returns MOBI_E_NULLREF when that ring slot has never been produced.  After a call that returned an error, slot 0 of that
 * stream is not the reference's partial picture (a frame that failed in the parse is not reconstructed at all: the slot still
 * holds the picture of six frames earlier); and P-frames that predict from it differ from the reference's (which predict from its
 * partial picture) until the next I-frame, from which on both are identical again. */
int mobi_get_planes(mobi_dec *d, int ring_idx, uint8_t *y_out, uint8_t *uv_out);
/* The Bitmap that DecodeFrame() returns (MD.cs:260-323) for the frame just decoded: width*height 0xAARRGGBB
 * words, row pitch = width (Format32bppArgb as LockBits hands it out: bytes B,G,R,A).  Chroma is averaged from up
 * to four neighbours by pixel parity, then the float matrix with range stretch (Moflex3DS) or the integer form
 * (ModsDS); float arithmetic is IEEE single, one rounding per operator of the source, no FMA.
 * MOBI_E_NULLREF before the first frame. */
int mobi_get_argb(mobi_dec *d, uint32_t *out);
/* Self-test of the Bitmap kernel's arithmetic: its three-instruction x / 239f against the correctly rounded IEEE
 * division for every float bit pattern with 1e-30 <= |x| <= 1e30 (about 20 ms on the device).  Returns the number of
 * mismatches (0 is the only acceptable answer) or -1 when the device cannot be used. */
long long mobi_selftest_div239(int device);
int mobi_stride(const mobi_dec *d);            /* d.Stride     (MD.cs:30,50-52) */
uint32_t mobi_quantizer(const mobi_dec *d);    /* d.Quantizer  (MD.cs:26) */
uint32_t mobi_yuv_format(const mobi_dec *d);   /* d.YuvFormat  (MD.cs:27) */
uint32_t mobi_width(const mobi_dec *d);        /* d.Width      (MD.cs:17) */
uint32_t mobi_height(const mobi_dec *d);       /* d.Height     (MD.cs:18) */

/* ---- batch of independent clips (the throughput path) -------------------------------------- */
/* N decoder instances that share geometry/version; they share nothing else (MD.cs:15-39).
 * Tuning knobs read from the environment when a batch is created (none changes a result: rc, Offset, Quantizer and planes do not depend
 * on where a clip is parsed -- see mobi_batch_set_parse_mode): MOBI_PARSE_THREADS (host parse pool; default
 * one per two hardware threads, at most 64), MOBI_DEVICE_PARSE and MOBI_HYBRID_HOST_CLIPS (below), MOBI_FUSED_STEP_MBS (a frame step of
 * at most this many macroblocks is ONE launch, mobi_recon_step; default 256 x 1200, 0 = always two launches). */
mobi_batch *mobi_batch_create(int n_clips, uint32_t width, uint32_t height, int version, int device);
void mobi_batch_destroy(mobi_batch *b);
/* One DecodeFrame() per clip: data[i]/len[i]/offsets[i] as in mobi_decode; rc[i] per clip.
 * Parses on the host, uploads the command lists, launches, synchronises.  Returns MOBI_OK or a
 * MOBI_E_DEVICE/ARG failure of the call itself (per-clip stream errors go to rc[]). */
int mobi_batch_decode(mobi_batch *b, const uint8_t *const *data, const size_t *len, int32_t *offsets, int *rc);
/* Where mobi_batch_decode parses the bitstreams.  0: host threads, command lists uploaded per call.  1: on the GPU, one
 * wavefront per clip (mobi_dparse.hip): Data[Offset..) of every clip is uploaded instead and the command lists never leave
 * HBM; same rc / Offset / planes.  The parse of one clip is serial and a GPU lane is slow at it; the GPU wins by running
 * thousands of clips at once, from about 20 resident clips per host parse thread upward.  Default: by batch size (device parse from max(640, 20 x threads) clips,
 * unless the first call hands over far more than a frame per clip -- whole files as Data, MOC5 style -- which the device path
 * would have to upload again for every frame), or MOBI_DEVICE_PARSE=0/1/2/3.  2 = hybrid: the GPU parses most clips while the
 * host pool parses a fixed share of them (a fifth, at most 1024; MOBI_HYBRID_HOST_CLIPS) at the same time; one set of
 * reconstruction launches serves both.  3 = as 1 with the lock-step parser in front of EVERY step (mobi_lsparse.hip: a few clips per
 * wavefront, one per lane, all lanes in one instruction stream): it finishes the frames that decode without incident -- identically, word
 * for word -- and leaves every other clip to the one-wavefront-per-clip parser, which then runs for those alone.  By default the parser in
 * front is chosen step by step: the lock-step parser from 5120 clips (23 ms per 640x480 P-frame step of 24576 clips against 57) and for
 * I-frame steps from 768 clips (15 ms against 30 at 4096 clips); 1 = never.
 * THE RESULT DOES NOT DEPEND ON THE MODE (r05).  The device parsers finish the frames that decode without incident.  A frame they cannot
 * finish -- anything the reference throws on, a coefficient run that walks through `Internal` (MD.cs:3424-3429), a ModsDS quantiser below
 * 12, a value the command list has to escape -- is parsed again by the host parser inside the same call (mobi_batch_wait for asynchronous
 * steps), from the decoder state the clip had when that frame started, which the device keeps for exactly this; the clip then stays with the
 * host parser (mobi_batch_host_clips counts them), parsed beside the GPU's clips as the hybrid mode's share is, until it has had a run of
 * frames the device parsers finish (4, doubled with every hand-over, at most 256), and goes back with the host parser's state.
 * Can only be changed before the first frame: the decoder state lives on one side. */
int mobi_batch_set_parse_mode(mobi_batch *b, int device_parse);
/* how many clips of the batch the host parser parses at present: all of them in mode 0; in the other modes the hybrid share plus the clips
 * that have had a frame the device parsers could not finish and have not gone back yet */
int mobi_batch_host_clips(const mobi_batch *b);
/* Parse mode 3: how many clips of the last finished frame step the lock-step parser finished itself (the rest went to the other one);
 * -1 in the other modes or before the first step. */
int mobi_batch_lockstep_finished(const mobi_batch *b);
/* Give each listed clip a new MobiclipDecoder(Width, Height, Version) (MD.cs:41-54) for its next frame: the caller ends one stream in a
 * slot of the batch and starts the next file (or seeks: a suffix that starts at an I-frame) there, while the other clips go on.
 *   WHEN:      from the next frame step the caller hands over: mobi_batch_decode, mobi_batch_submit, or the first frame of
 *              mobi_batch_decode_gop / mobi_batch_gop_begin.  Steps and groups already in flight decode exactly as they would have without
 *              the call; frames they report afterwards (mobi_batch_wait, mobi_batch_gop_finish, repairs included) are the old stream's.
 *   NO WAIT:   never waits for the GPU and enqueues nothing; allowed while steps or groups are in flight (gop_begin(g + 1) before
 *              gop_finish(g)).  The device side runs in front of that step's parse, one launch per step (mobi_reset_state).
 *   WHAT:      everything a new decoder starts with: Quantizer, YuvFormat, Internal[] and the count of ring slots that hold a frame
 *              (MOBI_E_NULLREF for a reference the new stream has not decoded yet), on the host parser and on the device; and the routing:
 *              a clip the device parsers had handed to the host parser goes back to them (with a fresh count of clean frames, as at
 *              creation); a clip of the hybrid mode's host share (parse mode 2) stays there, with a fresh host parser.
 *   NOT:       no pixel.  The ring keeps the pictures it holds, and pictures being written by steps in flight, until it turns over them: the
 *              old stream's last frames can still be exported after the reset and after the new stream's first frame was handed over.  The
 *              getters and exports keep their batch-wide checks.  Ring index r of clip c holds a picture of the current stream exactly
 *              when r < min(6, clip_frames[c]).  Version and geometry stay batch-wide: the new stream must match them (not checked: frames
 *              carry neither, as with mobi_create).  The replay path parses with fresh parsers anyway: only the counts change there.
 *   REFUSED:   MOBI_E_ARG for count < 0, clips NULL with count > 0 or any index outside [0, n_clips) -- all checked before anything
 *              changes; MOBI_E_DEVICE for a poisoned batch (as mobi_batch_submit).  Duplicates are allowed; count == 0 does nothing. */
int mobi_batch_reset_clips(mobi_batch *b, const int32_t *clips, int count);
/* out[c] (n_clips entries) = frames handed over for clip c since the batch was created or the clip was last reset.  Host bookkeeping, never
 * reads the GPU.  Counts ring turns: one per step (steps in flight included), one per frame of a group, one per mobi_batch_replay; frames
 * that threw too (the reference turns its ring before anything can throw, MD.cs:102-108).  For a clip never reset: the frames the batch has
 * been handed.  A reset sets it to 0 and the frames of groups begun before it do not count. */
int mobi_batch_clip_frames(const mobi_batch *b, int32_t *out);
/* Idle frame slots: "clip c has no frame here, its stream has ended".  A batch moves in lock step, so a clip whose stream ends inside a
 * group (or a step before the caller has the next file) still owes the call a slot; an empty packet there is a damaged stream
 * (MOBI_E_INDEX, and the clip goes to the host parser).  An idle slot is never parsed, on either side, never handed to the host parser,
 * changes no decoder state and writes no pixel.
 *   MASK:      idle[k * n_clips + c] != 0 marks frame k of clip c of the NEXT step or group handed over (mobi_batch_decode,
 *              mobi_batch_submit: n_frames = 1; mobi_batch_decode_gop, mobi_batch_gop_begin: n_frames = that call's).  The mask is copied,
 *              consumed by that hand-over and forgotten.  idle == NULL drops a mask set and not yet consumed (n_frames is ignored then).
 *   NO WAIT:   never waits for the GPU and enqueues nothing; allowed while steps or groups are in flight.  The device side is one launch
 *              (mobi_idle_rows) in front of that hand-over's parse, and only when it has idle slots; a hand-over without a mask enqueues
 *              exactly what it always did.
 *   SLOT:      for an idle slot data[..] may be NULL and len[..] / offsets[..] are ignored; rc[..] is MOBI_IDLE and the Offset reported is
 *              the one handed in.
 *   ENDS:      an idle slot ENDS the clip's stream.  Within a group the idle slots of a clip are a suffix (once idle, idle to the group's
 *              end), and a clip that has had an idle slot takes a live frame again only after mobi_batch_reset_clips named it.  Resuming a
 *              paused stream is NOT supported: the ring turns batch-wide, so a clip that sat out a step has its references shifted.  A reset
 *              and an idle mark may name the same clip for the same hand-over if the idle slots still are a suffix (reset and idle from
 *              frame 0 on: an empty slot of the batch).
 *   RING:      the ring still turns once per frame for every clip.  An idle slot writes nothing: the clip's earlier pictures move to higher
 *              ring indices and the slot that comes round holds an older picture of that clip -- unspecified but initialised memory; the
 *              getters and exports keep their batch-wide checks and deliver it.  With idle[c] = mobi_batch_clip_idle and clip_frames[c] =
 *              mobi_batch_clip_frames (LIVE frames only; for a caller that never sets a mask what it always counted), ring index r of clip
 *              c holds a picture of the current stream exactly when idle[c] <= r < min(6, idle[c] + clip_frames[c]) -- this replaces the
 *              rule under mobi_batch_reset_clips.
 *   STATE:     mobi_batch_quantizer / mobi_batch_yuv_format of such a clip stay those of its last live frame.  The clip is not counted by
 *              mobi_batch_host_clips, and by mobi_batch_lockstep_finished neither as finished nor as left over.  mobi_batch_reset_clips
 *              works on it as on any other clip and clears the "ended" mark and the idle count with the step it applies to.
 *   REFUSED:   here: MOBI_E_ARG for n_frames outside [1, 128] with idle != NULL, MOBI_E_DEVICE for a poisoned batch.  By the hand-over,
 *              before anything changes: MOBI_E_ARG when its n_frames differs from the mask's (the mask stays), when a clip's idle slots are
 *              not a suffix, and for a live frame of a clip whose stream has ended and that no reset has named. */
int mobi_batch_set_idle(mobi_batch *b, const uint8_t *idle, int n_frames);
/* out[c] (n_clips entries) = idle slots handed over for clip c since its last live frame or reset.  Host bookkeeping, steps and groups in
 * flight included; never reads the GPU. */
int mobi_batch_clip_idle(const mobi_batch *b, int32_t *out);
/* how many launches of the idle-slot kernel (mobi_idle_rows) the batch has made so far: 0 for a caller that never sets a mask */
int mobi_batch_idle_launches(const mobi_batch *b);
/* Asynchronous frame steps, for callers that already hold the next frame of every clip (demuxed Moflex / Mods packets: the Offset
 * to start from does not depend on the previous frame's parse).  The batch must parse on the GPU (the default for large batches, see above;
 * mobi_batch_set_parse_mode(b, 1), 2 or 3 otherwise: the hybrid mode's host share is parsed inside mobi_batch_submit) and at most two steps
 * may be in flight.
 *   mobi_batch_submit: copies the bytes data[i][offsets[i] .. len[i]) of every clip into pinned memory and enqueues upload, parse and
 *                      reconstruction of one frame step behind the step before; returns without waiting for the GPU.  The caller's
 *                      buffers may be reused as soon as it returns.  The upload has a stream of its own, and so has the lock-step parser
 *                      (parse mode 3): the parse of step n + 1 then runs under the reconstruction of step n (its output buffers
 *                      belong to the step).
 *   mobi_batch_wait:   waits for the OLDEST step in flight and reports what mobi_batch_decode would have: rc[i] per clip,
 *                      offsets_out[i] = Offset after the frame (may be NULL).
 * mobi_batch_decode, mobi_batch_get_planes and the other calls that read results wait for everything enqueued; mobi_batch_decode is
 * refused (MOBI_E_ARG) while steps are in flight.
 * WHICH FRAME IS WHERE: mobi_batch_submit turns the ring at once (Y[i] = Y[i-1], MD.cs:102-106, happens at submission, not at
 * completion).  With steps in flight, ring_idx 0 of mobi_batch_get_planes / get_argb / convert_argb is the NEWEST submitted step's
 * frame, and the frame of the step mobi_batch_wait has just reported sits at ring_idx = mobi_batch_in_flight(b) (1 while one later
 * step is in flight).  The getters wait for everything enqueued before they copy, so reading results between submit and wait drains the
 * pipeline: read after the last wait, or accept the drain.  mobi_batch_quantizer / mobi_batch_yuv_format describe the step last
 * WAITED for.  If mobi_batch_submit fails after it has started to enqueue (MOBI_E_DEVICE), the batch is drained and refuses all
 * further steps: destroy it.  A frame the device parsers could not finish is repaired in mobi_batch_wait (every such clip of the step
 * at once: their start states in one copy, their parses on the host threads, one reconstruction of those clips per affected step); rc,
 * Offset, Quantizer and the frame's planes are then the host parser's, as in mobi_batch_decode.  ONE thing is unspecified in this mode
 * only: when such a clip's NEXT frame was already in flight (parsed by the device from the state the failed frame left and reconstructed
 * before anybody knew), that ring slot may hold what the wrong parse wrote -- so if the repaired parse of that next frame is itself
 * rejected (rc != MOBI_OK) the slot's content is unspecified (mobi_batch_decode leaves the picture of six frames earlier there), and a
 * repaired frame that predicts from the OLDEST ring picture (reference 5, the slot the step in flight was writing) may predict from it.
 * Both need a damaged stream; intact streams, and damaged ones under mobi_batch_decode / mobi_batch_decode_gop, are exact.
 * What it buys: the host gathers and uploads step n + 1 while the GPU parses step
 * n, and the GPU goes from parse to reconstruction without asking the host for launch sizes. */
int mobi_batch_submit(mobi_batch *b, const uint8_t *const *data, const size_t *len, const int32_t *offsets);
int mobi_batch_wait(mobi_batch *b, int32_t *offsets_out, int *rc);
int mobi_batch_in_flight(const mobi_batch *b); /* steps submitted and not yet waited for: 0, 1 or 2 */
/* Frame-parallel groups (r06): K = n_frames consecutive frames of EVERY clip in one call, 1 <= K <= 6 (the ring holds six pictures,
 * MD.cs:19-20: every frame of the group is still there when the call returns -- frame k of the group at ring_idx K - 1 - k).  For callers
 * that hold whole packets of a clip's next frames -- what the Moflex / Mods demuxers deliver (MoLiveDemux.cs:349-358, ModsDemuxer.cs:97-117);
 * not for MOC5-style callers whose next Offset is only known once the frame before has been parsed.  All arrays are [k * n_clips + c]:
 * frame k of clip c is data[..][offsets[..] .. len[..]), exactly what K calls of mobi_batch_decode would have been given; rc[..] and the
 * Offsets after the frames come back the same way, and rc, Offset, Quantizer and planes ARE what those K calls give (tests: fuzzed
 * streams, every parse mode).  What it buys: a frame's PARSE needs from the frame before it only what the frame headers determine
 * (Quantizer, YuvFormat, the frame count: MD.cs:113-143, 224-236, 3884-3925; measured, profiles/r06_framedep.txt), so the device parsers
 * run over n_clips * K frames side by side -- and their cost per frame falls with the number of lanes they are given -- while the
 * reconstruction stays one step per frame, in order.  A start state predicted wrong, like a frame the device parsers do not finish,
 * hands that clip's remaining frames to the host parser inside the same call (the prediction can cost time, never the result).
 *   mobi_batch_decode_gop: the whole group, synchronously.  A batch that parses on the host (small batches; mobi_batch_set_parse_mode(b, 0))
 *                          simply runs its K steps one after the other.
 *   mobi_batch_gop_begin / mobi_batch_gop_finish: the same in two halves, for callers that keep the GPU fed: begin gathers and uploads a
 *                          group (and starts its parse when no group is in front of it) and returns; finish reports the OLDEST group
 *                          begun and not finished.  At most two groups may be begun: with group g + 1 begun before group g is finished,
 *                          its upload runs beside group g's reconstruction and its parse goes out behind the steps of g's last part:
 *                          the GPU parses while the caller gathers the group after next.  The batch must parse on the GPU (as for
 *                          mobi_batch_submit).  The ring turns in finish, once per frame; planes are read after finish.
 *                          A group begun this way may hold up to 128 frames -- what is parsed side by side is not bound by the ring, and
 *                          a small batch fills the parsers' lanes only with that many -- and finish hands them out SIX AT A TIME, oldest
 *                          first: every call reconstructs and reports min(6, mobi_batch_gop_frames_pending(b)) frames of the oldest group
 *                          (rc / offsets_out [j * n_clips + c], j counted from the part's first frame; that part's frame j sits at ring
 *                          index part_size - 1 - j afterwards), so a group of 12 is finished by two calls, one of 32 by six, one of 128 by 22.
 *                          What a group writes lives in HBM until it is reconstructed (per frame of it about 40 KB of descriptors and
 *                          items and the worst-case payload part, 0.3 - 0.5 MB at 640x480): a group that does not fit is refused by
 *                          mobi_batch_gop_begin (the allocator's error, nothing enqueued, the batch goes on).
 * mobi_batch_decode / mobi_batch_submit are refused (MOBI_E_ARG) while a group is begun and not finished. */
int mobi_batch_decode_gop(mobi_batch *b, int n_frames, const uint8_t *const *data, const size_t *len, int32_t *offsets, int *rc);
int mobi_batch_gop_begin(mobi_batch *b, int n_frames, const uint8_t *const *data, const size_t *len, const int32_t *offsets);
int mobi_batch_gop_finish(mobi_batch *b, int32_t *offsets_out, int *rc);
int mobi_batch_gop_in_flight(const mobi_batch *b); /* groups begun and not yet finished: 0, 1 or 2 */
int mobi_batch_gop_frames_pending(const mobi_batch *b); /* frames of the oldest such group that no finish has reported yet (0: none begun) */
/* Every frame of the oldest group that no mobi_batch_gop_finish has reported yet, in one call: offsets_out and rc have
 * mobi_batch_gop_frames_pending(b) * n_clips entries, and the results equal those of mobi_batch_gop_finish called until nothing is
 * pending.  One host wait at the end instead of one per six frames -- the six-frame parts exist so that the caller can read the ring
 * between them; a caller that reads it through a clip sink (below), or wants only the group's last six frames, which the ring holds
 * afterwards, needs none.  The parse of the group begun behind goes out as behind a last part.  Allowed with or without a sink, and
 * after some parts of the group have been finished the ordinary way. */
int mobi_batch_gop_finish_all(mobi_batch *b, int32_t *offsets_out, int *rc);
/* Wall-clock milliseconds the last mobi_batch_decode call spent inside the library (parse or upload, launches, sync). */
float mobi_batch_last_decode_ms(const mobi_batch *b);
int mobi_batch_get_planes(mobi_batch *b, int clip, int ring_idx, uint8_t *y_out, uint8_t *uv_out);
/* Bitmaps (MD.cs:260-323): mobi_batch_convert_argb converts ring slot 0 of EVERY clip into a device-resident buffer
 * (asynchronously, on the batch's stream); mobi_batch_get_argb copies one clip's width*height words out, converting
 * just that clip first if the whole-batch conversion has not been run for the current frame. */
int mobi_batch_convert_argb(mobi_batch *b);
int mobi_batch_get_argb(mobi_batch *b, int clip, uint32_t *out);
/* ... of the frame at ring index ring_idx (0 = the newest; MOBI_E_NULLREF for a slot never produced): the Bitmap DecodeFrame() returned
 * ring_idx calls ago.  For callers that decode in groups and want every frame's Bitmap: frame k of a group of K is ring index K - 1 - k. */
int mobi_batch_get_argb_at(mobi_batch *b, int clip, int ring_idx, uint32_t *out);
/* ---- export of decoded pictures to host memory (the callers' decode -> AddFrame loop, MobiConverter/Program.cs:69-76) ----------------
 * The getters above move one clip's frame per call and wait for everything enqueued; these move many clips x frames per call, through a
 * copy pipeline of their own, and do not wait for anything the caller has enqueued. */
#define MOBI_EXPORT_I420 0 /* per picture: Y width*height, then U, then V, (width/2)*(height/2) each; rows packed, no stride padding.
                              = the reference's Y[0] / UV[0] (MD.cs:107-108, 414-415) restricted to the picture area */
#define MOBI_EXPORT_ARGB 1 /* per picture: width*height uint32 words, byte for byte what mobi_batch_get_argb_at returns */
/* Pinned, portable host memory for export destinations (plain C callers cannot reach hipHostMalloc).  NULL without a device.
 * mobi_host_free takes only what mobi_host_alloc returned (anything else is ignored). */
void *mobi_host_alloc(size_t bytes);
void mobi_host_free(void *p);
/* n_frames pictures of clips [clip0, clip0 + n_clips): picture j is ring index ring_idx - j (j = 0 .. n_frames - 1, oldest first), written to
 * dst + (j * n_clips + (c - clip0)) * picture_bytes.  After gop_finish reported a part of P frames, (ring_idx = P - 1, n_frames = P) gives
 * them in the order of its rc / offsets arrays.  Returns at once with *ticket_out when dst lies inside one mobi_host_alloc block; for any
 * other dst it returns when the data is in dst (the ticket is then already complete).  ticket_out may be NULL.
 *   SNAPSHOT: what lands in dst is the pictures as they are when the call returns.  Later decode / submit / gop_finish / replay calls turn
 *             the ring and write those slots; a step that will write a slot an export has not finished reading waits for it on the GPU
 *             (so a decode that outruns the copy engine runs at the export's pace; with no export outstanding nothing waits).
 *   NO DRAIN: the export waits for no step or group in flight (on the host); it goes behind the reconstruction already enqueued.
 *   REFUSED:  MOBI_E_NULLREF for ring_idx >= frames started.  MOBI_E_ARG for a bad format or clip range, ring_idx > 5 or
 *             ring_idx - n_frames + 1 < 0, dst NULL or dst_bytes too small, a poisoned batch, and ring indices below
 *             mobi_batch_in_flight(b): frames of submitted steps not waited for yet (mobi_batch_wait may still repair them).
 *             A refused or failed export changes nothing and issues no ticket.
 *   LIFETIME: dst stays valid until mobi_batch_export_wait for its ticket (or a later one) returned, or until mobi_batch_destroy, which waits
 *             for the exports outstanding before it frees anything.
 * The getters (mobi_batch_get_planes, convert_argb, get_argb, get_argb_at) are not affected: the export has buffers of its own (a few
 * staging chunks in HBM, allocated at the batch's first export). */
int mobi_batch_export(mobi_batch *b, int format, int ring_idx, int n_frames, int clip0, int n_clips, void *dst, size_t dst_bytes,
                      uint64_t *ticket_out);
int mobi_batch_export_wait(mobi_batch *b, uint64_t ticket);  /* this export and all earlier ones are in dst; MOBI_OK or MOBI_E_DEVICE
                                                                (MOBI_E_ARG: a ticket this batch never issued) */
int mobi_batch_export_query(mobi_batch *b, uint64_t ticket); /* 1 done, 0 not yet, < 0 error */
/* ---- export of decoded pictures into device memory, on the caller's stream -------------------------------------------------------
 * For consumers on the GPU (torch tensors, the caller's own HIP allocations): no staging, no copy engine, no ticket. */
#define MOBI_EXPORT_RGB_PLANAR 2 /* per picture: R, G, B planes, each height x width elements (CHW) */
#define MOBI_EXPORT_RGB_PACKED 3 /* per picture: height x width x 3 elements, R G B (HWC) */
#define MOBI_DTYPE_U8 0  /* uint8 */
#define MOBI_DTYPE_F16 1 /* IEEE half */
#define MOBI_DTYPE_F32 2 /* IEEE single */
/* The same pictures as mobi_batch_export, in the same order: picture j of clip c (ring index ring_idx - j) goes to
 * dst + (j * n_clips + (c - clip0)) * picture_bytes.  MOBI_EXPORT_I420 and MOBI_EXPORT_ARGB (dtype MOBI_DTYPE_U8, scale_bias NULL) are byte
 * for byte what mobi_batch_export writes.  RGB: R, G, B are bytes 2, 1, 0 of the Bitmap's 0xAARRGGBB word (mobi_batch_get_argb_at), in
 * both versions; uint8 stores them as they are (scale_bias must be NULL); float32 stores (float)v * scale[ch] + bias[ch], a product and a
 * sum each rounded in IEEE single (no fused multiply-add); float16 that float32 value rounded to nearest-even.  scale_bias = {scale R, G, B,
 * bias R, G, B}, or NULL for scale 1 and bias 0.
 *   STREAM:   stream is a hipStream_t (NULL: the null stream).  The export is enqueued on it and the call returns; on the GPU it waits for
 *             everything enqueued on the batch so far (through an event, as mobi_batch_export does), and work the caller enqueues on stream
 *             afterwards sees the data.  No host wait.
 *   SNAPSHOT: as for mobi_batch_export: a later step that writes an exported ring slot waits, on the GPU, for the kernels that read it, behind
 *             whatever the caller had enqueued on stream before them.  A caller that never lets stream run stalls the batch.
 *   REFUSED:  the refusals of mobi_batch_export (ring / clip range, ring indices of steps in flight, a poisoned batch, MOBI_E_NULLREF), and
 *             MOBI_E_ARG when dst is not device memory of the batch's device (host memory, mobi_host_alloc blocks, another device), when
 *             dst is not 16-byte aligned or [dst, dst + the bytes needed) is larger than dst_bytes or its allocation, for a format / dtype /
 *             scale_bias combination outside the list above, and when stream is capturing a graph.  A refused call enqueues nothing.
 *   LIFETIME: dst and stream stay valid until the export has run on stream; mobi_batch_destroy waits for device exports that still read the
 *             ring. */
int mobi_batch_export_device(mobi_batch *b, int format, int dtype, const float *scale_bias, int ring_idx, int n_frames, int clip0,
                             int n_clips, void *dst, size_t dst_bytes, void *stream);
/* The same export for consumers that want a fixed, smaller size: the crop (crop_x, crop_y, crop_w, crop_h) of every picture, area-averaged
 * down to out_w x out_h, as RGB tensors (MOBI_EXPORT_RGB_PLANAR / _PACKED only; dtype and scale_bias as above).  One kernel: no full-size
 * RGB is written anywhere.  Picture order, dst indexing, STREAM, SNAPSHOT and LIFETIME are mobi_batch_export_device's, with picture_bytes =
 * 3 * out_w * out_h * element size.  One crop per call, the same for every clip.
 *   VALUES:   exact, in integers.  P[y][x] is the Bitmap's word (mobi_batch_get_argb_at) and v one of its bytes 2, 1, 0 (R, G, B); the chroma
 *             neighbours and the last-row / last-column rule are the PICTURE's, not the crop's.  Separable area weights:
 *               wx(ox, s) = max(0, min((s + 1) * out_w, (ox + 1) * crop_w) - max(s * out_w, ox * crop_w)),  s = 0 .. crop_w - 1,
 *               wy(oy, t) the same with out_h and crop_h;   S = sum_t sum_s wy * wx * v[crop_y + t][crop_x + s];   D = crop_w * crop_h;
 *               q = (S + D / 2) / D   (floor division, D / 2 floored).
 *             uint8 stores q; float32 (float)q * scale[ch] + bias[ch], a product and a sum each rounded; float16 that value rounded to
 *             nearest-even.  out_w == crop_w and out_h == crop_h is a pure crop (q = v); the whole picture at its own size is byte for byte
 *             mobi_batch_export_device's RGB.  The result does not depend on the order of execution.
 *   REFUSED:  every refusal of mobi_batch_export_device, and MOBI_E_ARG for a format other than the two RGB ones, a crop that is empty or
 *             not inside the picture, out_w or out_h below 1, out_w > crop_w or out_h > crop_h (no upscaling), out_w not a multiple of 4,
 *             and crop_w * crop_h > 2^23 (the sums are 32-bit).  A refused call enqueues nothing. */
int mobi_batch_export_device_scaled(mobi_batch *b, int format, int dtype, const float *scale_bias, int crop_x, int crop_y, int crop_w, int crop_h,
                                    int out_w, int out_h, int ring_idx, int n_frames, int clip0, int n_clips, void *dst, size_t dst_bytes,
                                    void *stream);
/* The same export for consumers that want a different box of every clip at one fixed size, larger or smaller, mirrored or not (a training
 * loader's RandomResizedCrop and horizontal flip): boxes = n_clips rows of {x, y, w, h, flags} in HOST memory; row c - clip0 applies to every
 * frame of clip c in the call.  boxes is read and copied before the call returns: the caller may reuse it at once.  RGB tensors
 * (MOBI_EXPORT_RGB_PLANAR / _PACKED only; dtype and scale_bias as above), one kernel.  Picture order, dst indexing, STREAM, SNAPSHOT and
 * LIFETIME are mobi_batch_export_device_scaled's, with picture_bytes = 3 * out_w * out_h * element size.
 *   VALUES:   exact, in integers.  v[t][s] is one byte (R, G, B = bytes 2, 1, 0) of the Bitmap's word at picture row y + t, column x + s; the
 *             chroma neighbours and the last-row / last-column rule are the PICTURE's, not the box's.  Each axis (in_n source samples, out_n
 *             outputs: w and out_w, h and out_h) has a weight matrix W[o][s] and a denominator d:
 *               out_n <= in_n (area):   W[o][s] = max(0, min((s + 1) * out_n, (o + 1) * in_n) - max(s * out_n, o * in_n)),  d = in_n
 *                                       (mobi_batch_export_device_scaled's weights);
 *               out_n >  in_n (linear, sample centres aligned, clamped at the BOX's edge: crop, then resize):
 *                                       n = (2 * o + 1) * in_n - out_n,  i0 = floor(n / (2 * out_n)),  f = n - i0 * 2 * out_n;
 *                                       weight 2 * out_n - f goes to source clamp(i0, 0, in_n - 1), weight f to clamp(i0 + 1, 0, in_n - 1)
 *                                       (they add when both are one source);  d = 2 * out_n.
 *             Every row of W sums to d.  S = sum_t sum_s Wy[oy][t] * Wx[ox][s] * v[t][s];  D = dx * dy;  q = (S + D / 2) / D  (floor
 *             division, D / 2 floored).  With MOBI_BOX_FLIP_X output column ox holds the q of column out_w - 1 - ox.  uint8 stores q;
 *             float32 (float)q * scale[ch] + bias[ch], a product and a sum each rounded; float16 that value rounded to nearest-even.
 *             A box at its own size is a pure crop (q = v); where both axes shrink the values are mobi_batch_export_device_scaled's;
 *             where both grow, S / D is bilinear interpolation with half-pixel centres (align_corners = False) of the box.  The result
 *             does not depend on the order of execution.
 *   REFUSED:  every refusal of mobi_batch_export_device, and MOBI_E_ARG for a format other than the two RGB ones, boxes == NULL, a box that
 *             is empty or not inside the picture, flag bits other than MOBI_BOX_FLIP_X, out_w or out_h below 1, out_w not a multiple of 4,
 *             and a clip whose D > 2^23 (the sums are 32-bit).  One bad box refuses the whole call; a refused call enqueues nothing. */
#define MOBI_BOX_FLIP_X 1 /* mirror the output left to right */
int mobi_batch_export_device_boxes(mobi_batch *b, int format, int dtype, const float *scale_bias,
                                   const int32_t *boxes /* host, n_clips x 5: x, y, w, h, flags */, int out_w, int out_h, int ring_idx,
                                   int n_frames, int clip0, int n_clips, void *dst, size_t dst_bytes, void *stream);
/* ---- the motion the stream carries: the decoder's motion field and macroblock data as device tensors -------------------------------
 * What a decoder knows besides the pictures: the motion vector and reference of every 2x2 luma cell, which macroblocks are intra, the
 * quantiser and how much residual was coded.  (mobi_batch_motion_search below is the encoder's side: it ESTIMATES motion of new pictures.)
 * mobi_batch_set_motion(b, 1) allocates a motion ring of six slots per clip beside the picture ring (288 bytes per macroblock and slot);
 * from then on every frame step -- decode, submit / wait, groups, replay, the repair of a clip in mobi_batch_wait -- writes its slot with
 * one more kernel (mobi_motion_field) that reads the step's command list in HBM.  mobi_batch_set_motion(b, 0) frees the ring.  Allowed only
 * with nothing in flight: MOBI_E_ARG while a submitted step or a group is outstanding or an export (host or device) may still be running;
 * setting the state the batch is in is a no-op.  A batch that never switches motion on runs the code it ran before: no allocation, no launch
 * (mobi_batch_motion_bytes and mobi_batch_motion_launches stay 0).
 *   VECTORS:  (dx, dy) in half samples, pointing from the block to its source in the reference picture (the decoder's sign); ref = 1..5,
 *             frames back; ref 0 = an intra macroblock (dx = dy = 0).  The reference decoder addresses its planes linearly, so
 *             (dx - 4 t Stride, dy + 4 t) is the same copy for every t; the vector exported is the member of that class with
 *             -2 Stride <= dx < 2 Stride, however the macroblock was partitioned.  Stride >= Width: every vector that moves by less than a
 *             picture width is exported as the stream codes it.
 *   A clip whose frame was refused or idle: the content of its slot is unspecified, as its picture's is.
 *   RESET:    mobi_batch_reset_clips moves no motion word, as it moves no pixel, and the motion ring turns with the picture ring for every
 *             clip alike.  Whether a ring index has motion at all is a property of the batch (frames stepped since motion was switched
 *             on), not of the clip: after a reset, ring index r of the clip holds the new stream's motion for r < min(6,
 *             mobi_batch_clip_frames) and beyond that still the words of the OLD stream's frames, exactly as they were exported before
 *             the reset -- the same rule as for its pictures.  A step or group in flight when the reset is called writes the old stream's
 *             motion.  Neighbouring clips are not touched.
 * mobi_batch_export_motion follows mobi_batch_export_device in every respect -- picture order and dst + (j * n_clips + (c - clip0)) *
 * picture_bytes, STREAM, SNAPSHOT (a later step that writes a motion slot waits for the kernels reading it), LIFETIME, and its refusals --
 * and refuses with MOBI_E_ARG when motion is not enabled or format / dtype / block / scale are outside the list below, and with
 * MOBI_E_NULLREF a ring index whose frame was decoded before motion was switched on.  W, H = the picture's width and height:
 *   MOBI_MOTION_CELLS  dtype MOBI_DTYPE_I16, block 2: per picture int16 [3][H/2][W/2], row-major: dx, dy, ref of every cell.
 *   MOBI_MOTION_MB     dtype MOBI_DTYPE_I32, block 16: per picture int32 [5][H/16][W/16]: type (0 inter, 1 intra); the quantiser field of the
 *                      command list (63: the frame's residual words are literal coefficient values, 62: no quantiser table was ever set
 *                      up); cbp6 (coded 8x8 areas: bits 0-3 luma, 4 U, 5 V); the number of coded levels; the sum of their magnitudes.
 *   MOBI_MOTION_FLOW   dtype MOBI_DTYPE_F32 or MOBI_DTYPE_F16, block 2, 4, 8 or 16: per picture [2][H/block][W/block]: x, y.  Per cell
 *                      nx = dx * (60 / ref), ny = dy * (60 / ref) (integers), 0 for intra cells; Sx, Sy = their int32 sums over the block's
 *                      cells = (block / 2)^2 cells; k = (float)((double)scale / (120.0 * cells)); float32 = (float)Sx * k, one conversion and
 *                      one product, each rounded once; float16 = that value rounded to nearest-even.  scale = 1: the mean displacement in
 *                      pixels per frame, pointing from the block to its source.  scale must be finite; the other formats ignore it. */
#define MOBI_MOTION_CELLS 0
#define MOBI_MOTION_MB 1
#define MOBI_MOTION_FLOW 2
#define MOBI_DTYPE_I16 3 /* int16 */
#define MOBI_DTYPE_I32 4 /* int32 */
int mobi_batch_set_motion(mobi_batch *b, int on);
long mobi_batch_motion_launches(const mobi_batch *b); /* launches of mobi_motion_field so far */
size_t mobi_batch_motion_bytes(const mobi_batch *b);  /* device memory the motion ring holds (0: motion is off) */
int mobi_batch_export_motion(mobi_batch *b, int format, int dtype, int block, float scale, int ring_idx, int n_frames, int clip0, int n_clips,
                             void *dst, size_t dst_bytes, void *stream);
/* ---- the clip sink: frame steps write chosen frames into one (N, T, ...) tensor ------------------------------------------------------
 * The exports above reach the six pictures of the ring, frame-major.  A video model wants T frames of every clip, every s-th frame, from a
 * start that differs per clip, as (N, T, 3, H, W), (N, 3, T, H, W) or (N, T, H, W, 3).  An armed sink rides along with the batch's frame
 * steps: behind the reconstruction of a step, on the batch's own stream, one more kernel (mobi_sink) writes the pictures that step
 * contributes straight to their place in the tensor.
 *   STEPS:     step numbers count the frame steps the batch runs after arming: step 0 is the next one.  Every path counts: decode,
 *              submit / wait, each frame of a group, replay.
 *   SELECTION: clip c contributes picture t at step start[c] + t * stride, t = 0 .. n_frames - 1.
 *   VALUES:    picture (c, t) holds exactly what mobi_batch_export_device_boxes(..., ring_idx 0, n_frames 1, ...) would write for clip c if
 *              it were called right after that step, with the same box, size, dtype and scale_bias (boxes NULL: the whole picture, no
 *              flip).  A clip whose frame was refused or idle gets whatever its slot holds, as that export would give.  The sink follows
 *              batch steps, not streams: mobi_batch_reset_clips does not touch it.
 *   ADDRESSES: in ELEMENTS of the dtype.  Planar: element (c, t, ch, y, x) is at dst + (c * clip_stride + t * frame_stride + ch * chan_stride
 *              + y * out_w + x) * esize; packed: (c * clip_stride + t * frame_stride + (y * out_w + x) * 3 + ch) * esize, chan_stride 0.
 *              That covers (N,T,3,H,W), (N,3,T,H,W), (N,T,H,W,3), the exports' frame-major order and strided views of them.
 *   REFUSED:   MOBI_E_ARG, changing and enqueuing nothing: every geometry refusal of mobi_batch_export_device_boxes (format, dtype /
 *              scale_bias combination, a box outside the picture, flag bits, out_w not a multiple of 4, D > 2^23); n_frames < 1 or
 *              stride < 1; a negative start or start + (n_frames - 1) * stride beyond int32; dst not 16-byte aligned; a stride that is not
 *              a multiple of 4 elements; pictures that overlap or leave [dst, dst + dst_bytes) -- the rule: order the (extent, stride)
 *              pairs of clips, frames and (planar) channels by stride; each stride must be at least the span of everything with a smaller
 *              stride, and the whole span must fit --; dst not device memory of the batch's device; arming, replacing or disarming while
 *              a submitted step or a group is outstanding; a poisoned batch.
 *   LIFETIME:  boxes and start are copied before the call returns.  dst stays valid until mobi_batch_sink_pending is 0 and the call that
 *              reports the last contributing frame has returned, or until the sink is disarmed (mobi_batch_set_sink(b, NULL), which
 *              waits for the batch's stream).  With its last picture written the sink disarms itself: later steps write nothing and
 *              launch nothing.
 *   ORDER:     when the call that reports a frame returns (decode, wait, gop_finish, gop_finish_all; mobi_batch_sync after replay) that
 *              frame's sink pictures are complete.  A clip repaired in mobi_batch_wait has its pictures of the repaired steps written
 *              again: the same words, or the repaired frame's.
 * A batch that never arms a sink runs the code it ran before: no allocation, no launch (mobi_batch_sink_launches stays 0). */
typedef struct mobi_sink {
  int format;               /* MOBI_EXPORT_RGB_PLANAR or MOBI_EXPORT_RGB_PACKED */
  int dtype;                /* MOBI_DTYPE_U8 / _F16 / _F32; scale_bias as mobi_batch_export_device (NULL for U8) */
  const float *scale_bias;
  const int32_t *boxes;     /* host, n_clips x {x, y, w, h, flags} as mobi_batch_export_device_boxes; NULL: the whole picture, no flip */
  int out_w, out_h;
  int n_frames;             /* T >= 1: pictures every clip contributes */
  int stride;               /* s >= 1: every s-th step */
  const int32_t *start;     /* host, n_clips, each >= 0: the step of the clip's first picture; NULL: all 0 */
  int64_t clip_stride, frame_stride, chan_stride;   /* in ELEMENTS */
  void *dst; size_t dst_bytes;                      /* device memory of the batch's device */
} mobi_sink;
int mobi_batch_set_sink(mobi_batch *b, const mobi_sink *spec); /* NULL: disarm */
int mobi_batch_sink_pending(const mobi_batch *b);   /* (clip, t) pictures the armed sink has not written yet; 0: none armed or complete */
long mobi_batch_sink_launches(const mobi_batch *b); /* launches of mobi_sink so far */
/* host only, no GPU: every refusal above that needs no batch state and no look at dst's memory */
int mobi_sink_check(const mobi_sink *spec, int n_clips, uint32_t width, uint32_t height);
/* host only: the clips selected in `step` (ascending, into clips_out) and the element offset of their picture's first element (into
 * elem_off_out); either may be NULL.  Returns the count, or MOBI_E_ARG for a spec mobi_sink_check could not read (spec NULL, n_clips < 1,
 * n_frames < 1, stride < 1) */
int mobi_sink_plan(const mobi_sink *spec, int n_clips, int64_t step, int32_t *clips_out, int64_t *elem_off_out);
/* Encoder-side analysis: Analyzer.InterPredict2x2 (Analyzer.cs:608-681) for every 2x2 luma block of
 * every macroblock of every clip, as SolveInterPredictionPuzzle calls it (:683-693): three-step search (6, 3, 1 pels) in up
 * to five past frames = ring slots 0..4 of this batch (the encoder's PastFramesY, MobiEncoder.cs:138-144).
 * src_y[clip]: the picture to analyse, width*height luma bytes, pitch = width.  out[((clip * n_mbs + mb) * 64) + Y*8 + X] =
 * (Delta.X & 0xFF) | (Delta.Y & 0xFF) << 8 | Frame << 16 | score << 20 (Delta in half pels, as the reference stores it;
 * score = 0xFFF when the ring is empty). */
int mobi_batch_motion_search(mobi_batch *b, const uint8_t *const *src_y, uint32_t *out);
/* The encoder's forward transforms: MobiEncoder.DCT64 (Encoder/MobiEncoder.cs:962-1010, n = 8) and DCT16
 * (:1146-1178, n = 4) of n_blocks residual blocks (Block - CompVals, Encoder/MacroBlock.cs:584-588), n*n int32 each, back to back;
 * out as the reference returns it (the second pass stores transposed).  Integer arithmetic, truncating divisions: bit-exact.
 * The quantiser, bit cost and reconstruction behind it are mobi_transform_code below. */
int mobi_forward_dct(int device, int n, const int32_t *in, int32_t *out, size_t n_blocks);
/* The encoder's transform coding of residual blocks: MacroBlock.EncodeDecode8x8Block / EncodeDecode4x4Block
 * (Encoder/MacroBlock.cs:577-597, 605-626) and the SAD the analyzer scores a candidate with (Analyzer.GetScore8x8 / 4x4, Analyzer.cs:1201,
 * 1269), for every source block against its prediction at one or more quantisers.  For one block of n x n pixels (n = 8 or 4), src and
 * pred u8 row-major (the reference's Block and CompVals), quantiser q in [0, 53]:
 *   Q       SetupQuantizationTables (MobiEncoder.cs:930-960): T[k] = (dq4[qmod6[q] * 16 + k] << (qdiv6[q] + 8)) >> 8 for n = 4,
 *           (dq8[qmod6[q] * 64 + k] << (qdiv6[q] + 6)) >> 8 for n = 8; Q[zz[k]] = T[k] (zz = the decoder's scan order).  Integers.
 *   levels  d = DCT64 / DCT16 (src - pred) as mobi_forward_dct computes it, lev[i] = round_half_even(d[i] / Q[i]) -- what
 *           (int)Math.Round(d / QTable) gives (MacroBlock.cs:591-595): |d| <= 23 500 and Q is an integer, so the float quotient rounds
 *           as the exact one does ("Transform coding").  Out in scan order, levels[k] = lev[zz[k]] (EncodeDct); |lev| < 2^15.
 *   bits    CalculateNrBitsDCT(EncodeDct, 0) (MobiEncoder.cs:767-858): 0 when every level is 0; else the sum over the nonzero levels up to
 *           the last one of the code length of (|level|, zeros since the previous nonzero level, is it the last), VLC table 0 with its
 *           two escapes (+9 shorter run, +8 smaller value) and the 28-bit fallback.
 *   recon   dequantised lev[i] * Q[i] through IDCT64 / IDCT16 (MobiEncoder.cs:1012, 1180) in int32, each pixel Vx2MinMaxTable[0x40 +
 *           pred + (t >> 6)].  All-zero levels give recon == pred.
 *   sad     sum |src - recon| (GetScore8x8 / 4x4).
 *   flags   MOBI_TC_CODED: some level is nonzero (YUseComplex8x8 / YUseDCT4x4 stays set).  MOBI_TC_CLAMP: an index of the clamp table
 *           fell outside [0, 384), where the reference throws IndexOutOfRangeException; that entry's recon and sad are unspecified,
 *           its levels and bits are exact.  A clamp fault is not an error of the call.
 * n_blocks blocks x n_q quantisers (1 <= n_q <= 54, each in [0, 53]); entry e = qi * n_blocks + b.  src / pred: n_blocks * n * n bytes.
 * Per entry: levels_out n * n int16 (scan order), recon_out n * n bytes (row-major), bits_out / sad_out one int32, flags_out one byte.
 * levels_out, recon_out and sad_out may be NULL (not computed out); bits_out and flags_out may not.  MOBI_E_ARG for a bad n, n_q or
 * quantiser, a required NULL pointer while n_blocks > 0, or n_blocks * n_q >= 2^32; MOBI_E_DEVICE for a HIP failure; n_blocks == 0 is
 * MOBI_OK.  The C# caller of one block is in INTEGRATION.md. */
#define MOBI_TC_CODED 1
#define MOBI_TC_CLAMP 2
/* SetupQuantizationTables: QTable4x4 (16) / QTable8x8 (64) in natural DCT order, as the reference's float[] (either may be NULL).
 * MOBI_E_ARG for a quantizer outside [0, 53].  Host only: needs no device. */
int mobi_encoder_qtables(int quantizer, float *qtable4x4, float *qtable8x8);
/* Host pointers; synchronous. */
int mobi_transform_code(int device, int n, const int *quantizers, int n_q, const uint8_t *src, const uint8_t *pred, size_t n_blocks,
                        int16_t *levels_out, uint8_t *recon_out, int32_t *bits_out, int32_t *sad_out, uint8_t *flags_out);
/* The same on device pointers, enqueued on `stream` (a hipStream_t; NULL = the null stream); returns after the enqueue.  Allocates
 * nothing per call (the per-device constant tables are uploaded once, at the first call on that device). */
int mobi_transform_code_async(int device, void *stream, int n, const int *quantizers, int n_q, const uint8_t *src, const uint8_t *pred,
                              size_t n_blocks, int16_t *levels_out, uint8_t *recon_out, int32_t *bits_out, int32_t *sad_out, uint8_t *flags_out);
/* For batches made of copies (clip c was given the same stream as clip c mod modulus: a benchmark, a soak run): compares the newest frame
 * (ring slot 0) of EVERY clip with that of its source clip on the device, byte for byte, and returns how many clips differ (0 = none; < 0 =
 * MOBI_E_*).  n_diff_out, if not NULL, receives the number of differing 16-byte words per clip (n_clips entries).  Checking the `modulus`
 * source clips against the reference decoder then vouches for all of them (the reference has no counterpart: one decoder, one stream). */
int mobi_batch_compare_clips(mobi_batch *b, int modulus, uint32_t *n_diff_out);
uint32_t mobi_batch_quantizer(const mobi_batch *b, int clip);
uint32_t mobi_batch_yuv_format(const mobi_batch *b, int clip);
int mobi_batch_stride(const mobi_batch *b);
int mobi_batch_n_clips(const mobi_batch *b);

/* Pre-parsed replay: keep the command lists of whole clips resident in HBM so that a timed region
 * contains reconstruction only (SURVEY.md 8(d) "GPU timing").
 *  preload : parse all n_frames of `clip` (frame f = data[frame_off[f] .. frame_off[f+1])) and
 *            stage their command lists on the host; rc per frame optional.
 *  preload_clone: give `clip` a private copy of another clip's staged command lists (its own HBM
 *            bytes, same content) -- lets a benchmark run more clips than it generated streams.
 *  commit  : upload everything staged; builds the per-level launch lists across clips.
 *  replay  : one frame step for every clip: ring rotate + reconstruction kernels for frame
 *            `frame_idx`, asynchronously on the batch stream.  No host parse, no H2D.
 *  sync    : wait for the stream; returns MOBI_E_CLAMP if any clip flagged a clamp-domain fault. */
int mobi_batch_preload(mobi_batch *b, int clip, const uint8_t *data, size_t len, const uint32_t *frame_off,
                       int n_frames, int *rc_per_frame);
int mobi_batch_preload_clone(mobi_batch *b, int clip, int src_clip);
int mobi_batch_commit(mobi_batch *b);
int mobi_batch_replay(mobi_batch *b, int frame_idx);
int mobi_batch_sync(mobi_batch *b);
/* command-list bytes the kernels read for frame `frame_idx`, summed over clips (roofline accounting) */
uint64_t mobi_batch_cmd_bytes(const mobi_batch *b, int frame_idx);
/* of frame `frame_idx`, summed over clips: intra macroblocks, and the command-list bytes that belong to them (descriptor, block
 * records, level words).  mobi_recon_inter8 neither reads those bytes nor touches those macroblocks' pixels: bench.py leaves them
 * out of its algorithmic bytes */
int mobi_batch_intra_stats(const mobi_batch *b, int frame_idx, uint64_t *n_intra_mbs, uint64_t *intra_cmd_bytes);
/* milliseconds between two internally recorded HIP events bracketing the replay launches of the last
 * `mobi_batch_time_begin` .. `mobi_batch_time_end` region, measured on the batch's own stream */
int mobi_batch_time_begin(mobi_batch *b);
int mobi_batch_time_end(mobi_batch *b, float *ms_out);
/* per-kernel-class device time (ms) accumulated since the last time_begin: [0] inter MC+IDCT kernel,
 * [1] intra kernel launches; measured with HIP events around launches on the batch's stream.
 * level 0: off; 1: the inter launches only (the dominant kernel -- what a roofline needs; the events themselves cost a
 * few microseconds per launch); 2: every launch */
int mobi_batch_set_kernel_timing(mobi_batch *b, int level);
int mobi_batch_kernel_ms(mobi_batch *b, float *inter_ms, float *intra_ms, int *inter_launches, int *intra_launches);

const char *mobi_error_string(int rc);
/* library self-description: "libmobiclip_hip <ver> gfx950 ..." */
const char *mobi_build_info(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
