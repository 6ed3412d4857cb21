"""Batched audio decode (include/mobiclip_audio.h, include/mobiclip_sx.h): the FastAudio, IMA-ADPCM, PCM16 and Sx sound of many .moflex /
.mods streams into one torch tensor on the GPU, bit-exact with LibMobiclip's FastAudioDecoder and SxDecoder and the converter's
IMAADPCMDecoder.  The packets come from the container readers (demux.MoLiveDemux frames with chunk_id 2, demux.ModsDemuxer.ReadFrame),
Sx's codebooks from demux.ModsDemuxer.AudioCodebooks; samples are only ever produced by the HIP kernels (mobi_audio.hip, mobi_sx.hip)."""
import ctypes as C

import numpy as np

from .binding import Handle, as_u8, bind
from .decoder import MobiclipError, check_out, check_rc, check_stream, default_device, dtype_name, error_string, load_library, stream_and_out, tensor_bytes

MOBI_E_INDEX = -1  # include/mobiclip_hip.h: where the reference would throw
MOBI_E_UNSUPPORTED = -6

FRAMINGS = {"moflex": 0, "mods": 1}
CODECS = {"fastaudio": 0, "ima": 1, "pcm16": 2, "sx": 3}
MOFLEX_CODEC_IDS = {0: "fastaudio", 1: "ima", 2: "pcm16"}   # MoLiveStreamAudio.CodecId (Program.cs:83-157)
MODS_AUDIO_CODECS = {1: "sx", 2: "fastaudio", 3: "ima"}     # ModsHeader.AudioCodec (Program.cs:253-300)
DTYPES = {"int16": 0, "float32": 1}
LAYOUTS = {"planar": 0, "interleaved": 1}
MAX_CHANNELS = 8
TABLES = ("k01", "k2", "k3", "k4", "k5", "k6", "k7", "pulse", "ima_index", "ima_step")


class AudioBlock(C.Structure):
    """mobi_audio_block"""
    _fields_ = [("offset", C.c_uint32), ("header_offset", C.c_uint32), ("channel", C.c_uint16), ("header", C.c_uint16)]


# names must match include/mobiclip_audio.h (tests/test_audio_model.py checks header, library and this table)
_SIGS = {
    "mobi_audio_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.POINTER(C.c_int), C.c_void_p,
                                  C.POINTER(AudioBlock), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    "mobi_audio_table": (C.c_int, [C.c_int, C.POINTER(C.c_int32)]),
    "mobi_audio_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mobi_audio_destroy": (None, [C.c_void_p]),
    "mobi_audio_reset": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int]),
    "mobi_audio_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int)]),
}
# names must match include/mobiclip_sx.h (tests/test_sx_model.py checks header, library and this table)
_SX_SIGS = {
    "mobi_sx_plan": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.POINTER(C.c_int), C.POINTER(AudioBlock), C.c_size_t,
                               C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    "mobi_sx_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "mobi_sx_reset": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_void_p)]),
}
SX_PACKET_SAMPLES = 128
SX_CODEBOOK_BYTES = 0xC34  # MOBI_MODS_CODEBOOK_BYTES


def _lib():
    return bind(load_library(), _SIGS, _SX_SIGS)


def _codec(codec, framing):
    """a name of CODECS, or the container's own number: Moflex codec_id 0..2, Mods audio_codec 1..3"""
    if isinstance(codec, str):
        if codec not in CODECS:
            raise ValueError(f"codec must be one of {sorted(CODECS)} or the container's number, not {codec!r}")
        return codec
    names = MOFLEX_CODEC_IDS if framing == "moflex" else MODS_AUDIO_CODECS
    if isinstance(codec, bool) or not isinstance(codec, (int, np.integer)) or int(codec) not in names:
        raise ValueError(f"codec must be one of {sorted(CODECS)} or a {framing} codec number in {sorted(names)}, not {codec!r}")
    return names[int(codec)]


def _framing_codec_channels(framing, codec, n_channels):
    if framing not in FRAMINGS:
        raise ValueError(f"framing must be 'moflex' or 'mods', not {framing!r}")
    name = _codec(codec, framing)
    if name == "pcm16" and framing != "moflex":
        raise ValueError("pcm16 exists in Moflex framing only")
    if isinstance(n_channels, bool) or not isinstance(n_channels, (int, np.integer)) or not 1 <= int(n_channels) <= MAX_CHANNELS:
        raise ValueError(f"n_channels must be an int in [1, {MAX_CHANNELS}], not {n_channels!r}")
    return FRAMINGS[framing], name, int(n_channels)


def tables():
    """The constants of the formats as int32 arrays, by the names of TABLES.  Needs no device."""
    lib, out = _lib(), {}
    for i, name in enumerate(TABLES):
        a = np.empty(lib.mobi_audio_table(i, None), np.int32)
        lib.mobi_audio_table(i, a.ctypes.data_as(C.POINTER(C.c_int32)))
        out[name] = a
    return out


def plan(framing, codec, n_channels, data, offset=0, n_packets=0, cursor=0, fresh=None):
    """mobi_audio_plan: the blocks one frame of one stream yields, by the reference's framing rules.  Needs no device.
    -> (rc, blocks as a list of (offset, channel, header, header_offset), samples per channel as an int32 array, the cursor afterwards)."""
    fr, name, nc = _framing_codec_channels(framing, codec, n_channels)
    buf = as_u8(data)
    lib = _lib()
    fresh_a = None if fresh is None else np.ascontiguousarray(np.asarray(fresh, np.uint8))
    if fresh_a is not None and fresh_a.shape != (nc,):
        raise ValueError(f"fresh must hold {nc} flags")
    cur, n, ns = C.c_int(int(cursor)), C.c_size_t(), np.zeros(nc, np.int32)
    args = (fr, CODECS[name], nc, buf.ctypes.data if buf.size else None, buf.size, int(offset), int(n_packets), C.byref(cur),
            None if fresh_a is None else fresh_a.ctypes.data)
    rc = lib.mobi_audio_plan(*args, None, 0, C.byref(n), ns.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        return rc, [], ns, int(cursor)
    blocks = (AudioBlock * max(1, n.value))()
    cur = C.c_int(int(cursor))
    rc = lib.mobi_audio_plan(*args[:7], C.byref(cur), args[8], blocks, n.value, C.byref(n), ns.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, [(b.offset, b.channel, b.header, b.header_offset) for b in blocks[:n.value]], ns, cur.value


def sx_plan(n_channels, data, offset=0, n_packets=0, cursor=0):
    """mobi_sx_plan: the Sx packets one Mods frame of one stream yields.  Needs no device.
    -> (rc, packets as a list of (offset, channel), samples per channel as an int32 array, the cursor afterwards)."""
    nc = _framing_codec_channels("mods", "sx", n_channels)[2]
    buf = as_u8(data)
    lib = _lib()
    ptr = buf.ctypes.data if buf.size else None
    cur, n, ns = C.c_int(int(cursor)), C.c_size_t(), np.zeros(nc, np.int32)
    rc = lib.mobi_sx_plan(nc, ptr, buf.size, int(offset), int(n_packets), C.byref(cur), None, 0, C.byref(n), ns.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        return rc, [], ns, cur.value
    blocks = (AudioBlock * max(1, n.value))()
    cur = C.c_int(int(cursor))
    rc = lib.mobi_sx_plan(nc, ptr, buf.size, int(offset), int(n_packets), C.byref(cur), blocks, n.value, C.byref(n), ns.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, [(b.offset, b.channel) for b in blocks[:n.value]], ns, cur.value


def _codebook_rows(codebooks, n_rows, n_channels, what):
    """`codebooks` as n_rows * n_channels contiguous uint8 arrays of SX_CODEBOOK_BYTES each, or ValueError"""
    try:
        rows = [list(r) for r in codebooks]
    except TypeError:
        raise ValueError(f"codebooks must be a sequence of {what} sequences of {n_channels} buffers") from None
    if len(rows) != n_rows or any(len(r) != n_channels for r in rows):
        raise ValueError(f"codebooks must hold {n_rows} ({what}) sequences of {n_channels} buffers each")
    flat = []
    for r in rows:
        for b in r:
            try:
                a = as_u8(b)
            except (TypeError, ValueError):
                raise ValueError("a codebook must be a byte buffer") from None
            if a.size != SX_CODEBOOK_BYTES:
                raise ValueError(f"a codebook is {SX_CODEBOOK_BYTES} bytes, not {a.size}")
            flat.append(np.ascontiguousarray(a))
    return flat


class MobiclipAudio(Handle):
    """n_streams decoders of n_channels channels each, decoded side by side on one GPU: one lane per (stream, channel), the decoder states
    in device memory.  codec: "fastaudio", "ima", "pcm16", or the container's number (Moflex codec_id / Mods audio_codec); framing:
    "moflex" (frames of MoLiveDemux with chunk_id 2) or "mods" (ModsDemuxer.ReadFrame packets).  "sx" (Mods audio_codec 1) needs
    codebooks: n_streams sequences of n_channels buffers of 0xC34 bytes (per stream: ModsDemuxer.AudioCodebooks)."""
    _destroy = "mobi_audio_destroy"

    def __init__(self, n_streams, n_channels, codec, framing, device=None, codebooks=None):
        self.framing = framing
        fr, self.codec, self.n_channels = _framing_codec_channels(framing, codec, n_channels)
        if isinstance(n_streams, bool) or not isinstance(n_streams, (int, np.integer)) or int(n_streams) < 1 \
                or int(n_streams) * self.n_channels >= 1 << 24:
            raise ValueError(f"n_streams must be a positive int with n_streams * n_channels < 2**24, not {n_streams!r}")
        self.n_streams = int(n_streams)
        self._lib = _lib()
        if self.codec != "sx" and codebooks is not None:
            raise ValueError("codebooks belong to codec 'sx' only")
        if self.codec == "sx":
            if framing != "mods":
                raise ValueError("sx exists in Mods framing only")
            if codebooks is None:
                raise MobiclipError("Sx audio needs the file's codebooks (codebooks=[ModsDemuxer.AudioCodebooks, ...])")
            books = _codebook_rows(codebooks, self.n_streams, self.n_channels, "n_streams")
        self.device = int(default_device() if device is None else device)
        if self.codec == "sx":
            ptrs = (C.c_void_p * len(books))(*[b.ctypes.data for b in books])
            self._h = self._lib.mobi_sx_create(self.device, self.n_streams, self.n_channels, ptrs)
        else:
            self._h = self._lib.mobi_audio_create(self.device, fr, CODECS[self.codec], self.n_streams, self.n_channels)
        if not self._h:
            raise MobiclipError(f"mobi_{'sx' if self.codec == 'sx' else 'audio'}_create failed: {error_string(-8)}")

    def reset(self, streams, keep_cursor=False, codebooks=None):
        """New decoders for the listed streams (a refilled slot; a Mods key frame with codec 3: keep_cursor=True).  Takes effect in the next
        decode(), on its stream; waits for nothing.  Sx: codebooks = one sequence of n_channels buffers per listed stream gives them new
        codebooks as well (mobi_sx_reset; the cursor goes to 0); without, the decoders keep theirs."""
        try:
            idx = [int(s) for s in streams]
        except (TypeError, ValueError):
            raise ValueError(f"streams must be a sequence of ints, not {streams!r}") from None
        if any(s < 0 or s >= self.n_streams for s in idx):
            raise ValueError(f"streams must lie in [0, {self.n_streams})")
        arr = (C.c_int32 * max(1, len(idx)))(*idx)
        if codebooks is not None:
            if self.codec != "sx":
                raise ValueError("codebooks belong to codec 'sx' only")
            if keep_cursor:
                raise ValueError("new codebooks set the cursor to 0: keep_cursor does not go with codebooks")
            books = _codebook_rows(codebooks, len(idx), self.n_channels, "len(streams)")
            ptrs = (C.c_void_p * max(1, len(books)))(*[b.ctypes.data for b in books])
            check_rc(self._lib.mobi_sx_reset(self._h, arr, len(idx), ptrs))
            return
        check_rc(self._lib.mobi_audio_reset(self._h, arr, len(idx), int(bool(keep_cursor))))

    def decode(self, frames, offsets=None, n_packets=None, dtype=None, layout="planar", out=None, max_samples=None, stream=None):
        """One frame per stream -> (tensor, n_samples, rc).

        frames: n_streams byte buffers (None or empty: that stream decodes nothing and keeps its state) -- Moflex: the completed audio frame
        with its two appended zero bytes; Mods: the frame packet, with offsets[s] = where its audio starts (the video decode's returned
        offset - 2, + 4 for tag 0x334E packets whose first word has bit 15 set: Program.cs:250-252) and n_packets[s] = NrAudioPackets.
        tensor: on the device, (n_streams, n_channels, max_samples) for layout "planar", (n_streams, max_samples, n_channels) for
        "interleaved"; dtype torch.int16 (default) or torch.float32 = sample / 32768.  Samples beyond a row's count are not written.
        n_samples: int32 numpy (n_streams, n_channels), known when the call returns.  rc: int32 numpy (n_streams,), 0 or MOBI_E_INDEX
        where the reference would throw: that stream gets no samples and keeps its state.
        out: a contiguous tensor of that shape and dtype to fill (default: a new one of max_samples -- default: the length of the call's
        longest row, at least 1 -- allocated on `stream`).  stream: a torch.cuda.Stream of the device (default: its current stream); the call enqueues and does
        not wait.  Every argument is checked before the library is called (ValueError); a refused call enqueues nothing."""
        import torch
        S, nc = self.n_streams, self.n_channels
        if dtype is None:
            dtype = torch.int16
        dname = dtype_name(dtype, DTYPES, f"dtype must be torch.int16 or torch.float32, not {dtype!r}")
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be 'planar' or 'interleaved', not {layout!r}")
        try:
            frames = list(frames)
        except TypeError:
            raise ValueError("frames must be a sequence of byte buffers") from None
        if len(frames) != S:
            raise ValueError(f"frames must hold {S} buffers, not {len(frames)}")
        try:
            bufs = [as_u8(f) for f in frames]
        except (TypeError, ValueError):
            raise ValueError("frames must be byte buffers or None") from None
        mods = self.framing == "mods"
        if mods != (offsets is not None) or mods != (n_packets is not None):
            raise ValueError("offsets and n_packets are required in Mods framing and not allowed in Moflex framing")
        offs = pk = None
        if mods:
            try:
                offs = [int(v) for v in offsets]
                pk = [int(v) for v in n_packets]
            except (TypeError, ValueError):
                raise ValueError("offsets and n_packets must be sequences of ints") from None
            if len(offs) != S or len(pk) != S or any(v < 0 for v in offs) or any(v < 0 or v >= 1 << 32 for v in pk):
                raise ValueError(f"offsets and n_packets must hold {S} non-negative ints each")
        dev = torch.device("cuda", self.device)
        check_stream(stream, dev)
        if max_samples is not None and (isinstance(max_samples, bool) or not isinstance(max_samples, (int, np.integer))
                                        or not 0 < int(max_samples) < 1 << 31):
            raise ValueError(f"max_samples must be a positive int below 2**31, not {max_samples!r}")
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dim() != 3:
                raise ValueError("out must be a 3-d torch tensor")
            ms = out.shape[2] if layout == "planar" else out.shape[1]
            if max_samples is not None and int(max_samples) != ms:
                raise ValueError(f"max_samples = {max_samples} does not match out's {ms}")
            max_samples = ms
        if max_samples is None:
            max_samples = max(1, self._longest_row(bufs, pk))
        max_samples = int(max_samples)
        shape = (S, nc, max_samples) if layout == "planar" else (S, max_samples, nc)
        check_out(out, dev, dtype, shape, aligned=False)
        stream, out = stream_and_out(stream, out, dev, dtype, shape)
        ptrs = (C.c_void_p * S)(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_size_t * S)(*[b.size for b in bufs])
        n_samples, rc = np.zeros((S, nc), np.int32), np.zeros(S, np.int32)
        check_rc(self._lib.mobi_audio_decode(self._h, stream.cuda_stream, ptrs, lens, (C.c_size_t * S)(*offs) if mods else None,
                                             (C.c_uint32 * S)(*pk) if mods else None, DTYPES[dname], LAYOUTS[layout],
                                             out.data_ptr(), tensor_bytes(out), max_samples,
                                             n_samples.ctypes.data_as(C.POINTER(C.c_int32)), rc.ctypes.data_as(C.POINTER(C.c_int))))
        return out, n_samples, rc

    def _longest_row(self, bufs, n_packets):
        """the samples of the longest row of a call: Moflex by the framing itself (mobi_audio_plan, counting only; a frame it rejects
        has none), Mods from the round robin (ceil(n_packets / C) blocks -- Sx: packets of 128 samples -- for some channel, whatever the cursor)"""
        nc = self.n_channels
        if self.framing == "mods":
            per = SX_PACKET_SAMPLES if self.codec == "sx" else 256
            return max(-(-n // nc) * per if b.size else 0 for b, n in zip(bufs, n_packets))
        longest, n, ns = 0, C.c_size_t(), np.zeros(nc, np.int32)
        for b in bufs:
            if b.size and self._lib.mobi_audio_plan(FRAMINGS["moflex"], CODECS[self.codec], nc, b.ctypes.data, b.size, 0, 0, None, None, None,
                                                    0, C.byref(n), ns.ctypes.data_as(C.POINTER(C.c_int32))) == 0:
                longest = max(longest, int(ns.max()))
        return longest
