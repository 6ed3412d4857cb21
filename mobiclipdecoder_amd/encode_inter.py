"""The inter encoder (include/mobiclip_encode_inter.h): a batch of I420 pictures, each with the reconstruction of the frame before it, to
Mobiclip P-frames, one stream per picture, on the GPU; and encode_clips, which chains it behind the intra encoder over whole clips.
Every stream decodes -- in the reference decoder and in MobiclipBatch, behind the frame that was its reference -- to exactly the
reconstruction the encoder reports; decisions and bits are only ever produced by the HIP kernels (mobi_encode_inter.hip).  DESIGN.md,
"Inter encoder", has the rules."""
import ctypes as C

import numpy as np

from .binding import bind
from .decoder import MobiclipError, check_rc, load_library
from .encode import MobiclipIntraEncoder, _Encoder

# mobi_enc_inter_stats, one per picture
STATS_DTYPE = np.dtype([("bits", "<u8"), ("sad", "<u8"), ("mv_bits", "<u8"), ("coded_blocks", "<u4"), ("fallback_clamp", "<u4"),
                        ("fallback_level", "<u4"), ("code0", "<u4"), ("nonzero_mv", "<u4"), ("halfpel_mv", "<u4"), ("reserved", "<u4", 4)])

_P = C.c_void_p
# names must match include/mobiclip_encode_inter.h (tests/test_encode_inter_model.py checks header, library and this table)
_SIGS = {
    "mobi_enc_inter_create": (C.c_void_p, [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int]),
    "mobi_enc_inter_destroy": (None, [C.c_void_p]),
    "mobi_enc_inter_stream_bound": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "mobi_enc_inter_check": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, _P, C.c_size_t]),
    "mobi_enc_inter_async": (C.c_int, [C.c_void_p, _P, C.c_int, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _P, _P, _P]),
    "mobi_enc_inter": (C.c_int, [C.c_void_p, C.c_int, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _P, _P, _P]),
}


# the partition mode; names must match include/mobiclip_encode_parts.h (tests/test_encode_parts_model.py checks header, library and this table)
_PARTS_SIGS = {
    "mobi_enc_inter_set_partitions": (C.c_int, [C.c_void_p, C.c_int]),
    "mobi_enc_inter_get_partitions": (C.c_int, [C.c_void_p]),
    "mobi_enc_inter_stream_bound_partitions": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_int]),
}
# mobi_enc_inter_stats.reserved in the partition mode (MOBI_ENC_PARTS_STAT_*): macroblocks sent split, leaves sent
STAT_SPLIT, STAT_LEAVES = 0, 1

# the intra mode; names must match include/mobiclip_encode_pintra.h (tests/test_encode_pintra_model.py checks header, library and this table)
_PINTRA_SIGS = {
    "mobi_enc_inter_set_intra": (C.c_int, [C.c_void_p, C.c_int]),
    "mobi_enc_inter_get_intra": (C.c_int, [C.c_void_p]),
}
# mobi_enc_inter_stats.reserved in the intra mode (MOBI_ENC_PINTRA_STAT_INTRA): macroblocks sent intra
STAT_INTRA = 2


def _lib():
    return bind(bind(bind(load_library(), _SIGS), _PARTS_SIGS), _PINTRA_SIGS)


def stream_bound(width, height, partitions=False):
    """mobi_enc_inter_stream_bound[_partitions]: no P-frame of a width x height picture is longer (bytes, a multiple of 4); 0 for refused
    dimensions"""
    return int(_lib().mobi_enc_inter_stream_bound_partitions(width, height, int(bool(partitions))))


class MobiclipInterEncoder(_Encoder):
    """mobi_enc_inter_ctx: P-frames of width x height pictures for MobiclipVersion.Moflex3DS or .ModsDS, up to max_pictures per call.
    partitions=True: macroblocks may be split into 16x8, 8x16 and 8x8 leaves with a vector each (include/mobiclip_encode_parts.h).
    intra=True: a macroblock is sent intra where that is cheaper (include/mobiclip_encode_pintra.h).  The two modes exclude each other."""
    _destroy = "mobi_enc_inter_destroy"
    _sigs, _prefix, _call, _what, _stats, _no_extra = _SIGS, "mobi_enc_inter", "mobi_enc_inter", ("pictures", "references"), STATS_DTYPE, ()

    def __init__(self, width, height, version, max_pictures, device=None, partitions=False, intra=False):
        self._h = None
        if partitions and intra:
            raise ValueError("partitions and intra exclude each other")
        super().__init__(width, height, version, max_pictures, device)
        bind(bind(self._lib, _PARTS_SIGS), _PINTRA_SIGS)
        self.partitions = self.intra = False
        if partitions:
            self.set_partitions(True)
        if intra:
            self.set_intra(True)

    def set_intra(self, on):
        """mobi_enc_inter_set_intra: holds for the calls of encode() and encode_target() after it; refused (MobiclipError) while partitions are on"""
        if not self._h:
            raise MobiclipError("encoder is closed")
        check_rc(self._lib.mobi_enc_inter_set_intra(self._h, int(bool(on))))
        self.intra = bool(self._lib.mobi_enc_inter_get_intra(self._h))

    def set_partitions(self, on):
        """mobi_enc_inter_set_partitions: holds for the calls of encode() after it; stream_bound follows the mode"""
        if not self._h:
            raise MobiclipError("encoder is closed")
        check_rc(self._lib.mobi_enc_inter_set_partitions(self._h, int(bool(on))))
        self.partitions = bool(self._lib.mobi_enc_inter_get_partitions(self._h))
        self.stream_bound = int(self._lib.mobi_enc_inter_stream_bound_partitions(self.width, self.height, int(self.partitions)))

    def encode(self, pictures, references, prev_quantizer, quantizer, recon=False, stats=False, slot_bytes=None, stream=None):
        """pictures, references: (N, width * height * 3 / 2) uint8 each, packed I420 -- torch tensors on the encoder's device (encoded
        where they lie, on `stream` or torch's current one) or numpy arrays (the synchronous host entry point).  references[i] is the
        reconstruction of the frame before pictures[i], as an encoder reported it (`recon`).  prev_quantizer, quantizer: that frame's and
        this one's, ints in [12, 52] or one per picture.  slot_bytes: the room of one stream (a multiple of 4; default: the bound).

        Returns what MobiclipIntraEncoder.encode returns: a list of N bytes objects; for a torch input with slot_bytes given
        (streams, sizes), enqueued and not waited for; with recon and / or stats a dict as the last element ("recon" (N, frame) uint8,
        "stats" (N,) STATS_DTYPE, for the unsynchronised torch form an (N, 64) uint8 tensor)."""
        return self._encode([pictures, references], [(prev_quantizer, "prev_quantizer"), (quantizer, "quantizer")], (), recon, stats, slot_bytes, stream)

    def encode_target(self, pictures, references, prev_quantizer, target_bytes, qmin=12, qmax=52, recon=False, stats=False, slot_bytes=None, stream=None):
        """encode() with a byte target per picture in place of the quantiser (include/mobiclip_encode_rate.h), in either partition mode: the
        quantiser is found on the GPU by a bisection of [qmin, qmax] over trial encodes; the stream is no longer than its target, or its
        quantiser is qmax.  pictures, references: torch tensors on the encoder's device only.  prev_quantizer: an int, one per picture, or
        an (N,) uint8 tensor on the device -- the "quantizer" of the call that made the references, not waited for.  target_bytes: an int,
        one per picture, or an (N,) int32 tensor on the device.

        Returns what encode() returns for tensors, the dict always present and holding "quantizer": the (N,) uint8 chosen quantisers (a
        device tensor in the unsynchronised form, i.e. with slot_bytes given)."""
        from .encode_rate import encode_target
        return encode_target(self, "mobi_enc_inter_target_async", [pictures, references], prev_quantizer, target_bytes, qmin, qmax, (), recon, stats, slot_bytes, stream)


def encode_clips(frames, quantizer, gop, version, width, height, recon=False, partitions=False, target_bytes=None, carry_bytes=0, qmin=12, qmax=52,
                 quantizers=False, intra=False, container=None, file_bytes=None, fps=(30, 1, 0x18000000), audio=None, audio_codec="ima", audio_rate=None):
    """frames: an (N, T, width * height * 3 / 2) uint8 torch tensor on a GPU, packed I420 (what a clip sink or export_tensor("i420")
    writes).  Frame 0 and every gop-th frame of every clip go through the intra encoder, the rest through the inter encoder; the
    reconstructions stay on the device and become the next frame's reference.  quantizer: an int in [12, 52] or T of them, one per frame.
    partitions, intra: the inter encoder's modes (MobiclipInterEncoder); they exclude each other.  intra=True lets the P-frames behind a scene
    cut, or content no earlier frame shows, send those macroblocks intra.

    Exactly one of quantizer and target_bytes is given (the other is None).  target_bytes: an int or T of them, one per frame index: rate
    control (encode_target, quantisers from [qmin, qmax]).  Frame t of every clip gets target_t + carry; carry starts at 0 and becomes,
    after each frame, clamp(target given - bytes produced, 0, carry_bytes): what a frame leaves of its budget the next may spend, up to
    carry_bytes.  Targets, carry and the chosen quantisers stay on the device; the whole clip still waits once.

    Returns, per clip, the list of its T frame streams (bytes); with recon=True also the (N, T, frame) uint8 tensor of reconstructions:
    what a decoder fed the streams of clip i in order holds after each; with quantizers=True also the (N, T) uint8 tensor of the frames'
    quantisers.

    container: None, or "moflex" / "mods" (mux.py; the version must be the one the container carries: Moflex3DS / ModsDS).  Then each clip
    comes back as ONE bytes object, its file, in place of the list of frame streams: every frame is appended to the clip's file image on
    the device behind its encode call (key frames at t % gop == 0), its slots are dropped at once, and the one wait is the muxer's finish,
    which brings only the files' own bytes to the host.  file_bytes: the room of one file (default: head, tail and index plus T frames of
    the size of a raw picture; a clip that needs more raises MobiclipError naming file_bytes).  fps: (fps_rate, fps_scale) for the Moflex
    stream chunk and the raw fps word of the Mods header.

    audio: None, or an (N, C, S_total) int16 tensor on the frames' device, the clips' sound at audio_rate Hz (what MobiclipAudio.decode
    wrote, planar); needs container="moflex".  The files then carry a second stream (mux.MobiclipMuxer(audio=)): behind video frame t
    one audio frame of b_t = floor((t + 1) R) - floor(t R) blocks of 256 samples, R = audio_rate * fps_scale / (fps_rate * 256) in exact
    integer arithmetic, encoded on the GPU (audio_enc.MobiclipAudioEncoder, audio_codec "ima" or "pcm16") from the next blocks of
    `audio`; nothing is appended where b_t = 0.  `audio` must hold the 256 * floor(T R) samples the T frames take (ValueError); samples
    behind them are NOT sent: sound is cut to whole blocks at the pace of the pictures.  The default file_bytes grows by the audio
    frames' framed bytes; there is still one wait.  With recon=True the result ends with one more element, the (N, C, 256 * floor(T R))
    int16 tensor a decoder returns for the audio frames in order."""
    import torch
    if not type(frames).__module__.startswith("torch") or frames.ndim != 3 or frames.dtype != torch.uint8 or not frames.is_cuda:
        raise ValueError("frames must be an (N, T, frame_bytes) uint8 tensor on a GPU")
    n, t_n = int(frames.shape[0]), int(frames.shape[1])
    if partitions and intra:
        raise ValueError("partitions and intra exclude each other")
    if int(gop) < 1 or n < 1 or t_n < 1:
        raise ValueError("gop, clips and frames must be at least 1")
    if (quantizer is None) == (target_bytes is None):
        raise ValueError("exactly one of quantizer and target_bytes")
    per_frame = quantizer if target_bytes is None else target_bytes
    qs = [int(per_frame)] * t_n if np.isscalar(per_frame) else [int(q) for q in per_frame]
    if len(qs) != t_n:
        raise ValueError(f"one {'quantizer' if target_bytes is None else 'target_bytes'}, or one per frame")
    if int(carry_bytes) < 0:
        raise ValueError("carry_bytes must be at least 0")
    device = frames.device.index or 0
    if container is not None:
        from . import mux
        if container not in mux.CONTAINERS:
            raise ValueError(f"container must be None or one of {sorted(mux.CONTAINERS)}, not {container!r}")
        if int(version) != int(mux.CONTAINER_VERSION[container]):
            raise ValueError(f"a {container} file carries {mux.CONTAINER_VERSION[container].name} streams, not version {int(version)}")
        if len(fps) != 3:
            raise ValueError("fps must be (fps_rate, fps_scale, fps_raw)")
    a_blocks = None
    if audio is not None:
        if container != "moflex":
            raise ValueError("audio needs container='moflex': only a moflex file carries an audio stream here")
        if not isinstance(audio, torch.Tensor) or audio.ndim != 3 or audio.dtype != torch.int16 or audio.device != frames.device or int(audio.shape[0]) != n:
            raise ValueError(f"audio must be an ({n}, C, S_total) int16 tensor on {frames.device}")
        if audio_rate is None or isinstance(audio_rate, bool) or int(audio_rate) != audio_rate or not 1 <= int(audio_rate) <= 1 << 24:
            raise ValueError("audio_rate must be an int in [1, 2**24]")
        if int(fps[0]) < 1 or int(fps[1]) < 1:
            raise ValueError("fps_rate and fps_scale must be at least 1 to pace the audio")
        num, den = int(audio_rate) * int(fps[1]), int(fps[0]) * 256
        a_blocks = [(t + 1) * num // den - t * num // den for t in range(t_n)]
        if int(audio.shape[2]) < 256 * sum(a_blocks):
            raise ValueError(f"audio holds {int(audio.shape[2])} samples per channel; {t_n} frames at {audio_rate} Hz take {256 * sum(a_blocks)}")
        if not audio.is_contiguous():
            audio = audio.contiguous()
    intra_mode = bool(intra)  # the name serves the I-frame encoder below
    intra = MobiclipIntraEncoder(width, height, version, n, device=device)
    inter = MobiclipInterEncoder(width, height, version, n, device=device, partitions=partitions, intra=intra_mode) if t_n > 1 and int(gop) > 1 else None
    slot = max(intra.stream_bound, inter.stream_bound if inter else 0)
    held, rec_all, q_all, ref = [], [], [], None
    carry = q_dev = muxer = files = a_enc = None
    a_rec, a_at = [], 0
    try:
        given_file_bytes = file_bytes
        if container is not None:
            n_keys = (t_n + int(gop) - 1) // int(gop)
            muxer = mux.MobiclipMuxer(container, width, height, n, fps_rate=fps[0], fps_scale=fps[1], fps_raw=fps[2], max_key_frames=n_keys, device=device)
            if file_bytes is None:
                file_bytes = mux.fixed_bytes(container, n_keys) + t_n * mux.framed_bytes(container, intra.frame_bytes)
            if a_blocks is not None:
                from .audio_enc import MobiclipAudioEncoder
                a_enc = MobiclipAudioEncoder(n, int(audio.shape[1]), audio_codec, max(1, max(a_blocks)), device=device)
                muxer.set_audio(a_enc.codec_id, int(audio_rate), a_enc.n_channels)
                if given_file_bytes is None:
                    file_bytes += mux.fixed_bytes(container, n_keys, audio=True) - mux.fixed_bytes(container, n_keys)
                    file_bytes += sum(mux.framed_bytes(container, a_enc.frame_bytes(b)) for b in a_blocks if b)
            muxer.begin(n, file_bytes)
        for t in range(t_n):
            pics = frames[:, t].contiguous()
            if target_bytes is not None:
                given = torch.full((n,), qs[t], dtype=torch.int32, device=frames.device) if carry is None else carry + qs[t]
                if t % int(gop) == 0:
                    out, sizes, ex = intra.encode_target(pics, given, qmin, qmax, recon=True, slot_bytes=slot)
                else:
                    out, sizes, ex = inter.encode_target(pics, ref, q_dev, given, qmin, qmax, recon=True, slot_bytes=slot)
                carry = torch.clamp(given - sizes, 0, int(carry_bytes))
                q_dev = ex["quantizer"]
            elif t % int(gop) == 0:
                out, sizes, ex = intra.encode(pics, qs[t], recon=True, slot_bytes=slot)
            else:
                out, sizes, ex = inter.encode(pics, ref, qs[t - 1], qs[t], recon=True, slot_bytes=slot)
            ref = ex["recon"]
            if muxer is not None:
                muxer.append(out, sizes, t % int(gop) == 0)
                del out  # the frame is in the file: the device need not hold T x N slots
                if a_enc is not None and a_blocks[t]:
                    res_a = a_enc.encode(audio[:, :, 256 * a_at:256 * (a_at + a_blocks[t])], recon=recon)
                    muxer.append_audio(res_a[0], res_a[1])
                    a_at += a_blocks[t]
                    if recon:
                        a_rec.append(res_a[2]["recon"])
                    del res_a
            else:
                held.append((out, sizes))
            if quantizers:
                q_all.append(q_dev if target_bytes is not None else torch.full((n,), qs[t], dtype=torch.uint8, device=frames.device))
            if recon:
                rec_all.append(ref)
        if muxer is not None:
            files = muxer.finish()  # the one wait
        else:
            torch.cuda.current_stream(frames.device).synchronize()
    finally:
        intra.close()
        if inter:
            inter.close()
        if muxer is not None:
            muxer.close()
        if a_enc is not None:
            a_enc.close()
    clips = files if files is not None else [[] for _ in range(n)]
    for out, sizes in held:
        out, sizes = out.cpu().numpy(), sizes.cpu().numpy()
        for i in range(n):
            clips[i].append(out[i, :sizes[i]].tobytes())
    res = [clips] + ([torch.stack(rec_all, 1)] if recon else []) + ([torch.stack(q_all, 1)] if quantizers else [])
    if a_blocks is not None and recon:
        res.append(torch.cat(a_rec, 2) if a_rec else audio[:, :, :0])
    return tuple(res) if len(res) > 1 else clips
