"""The audio encoder (include/mobiclip_audio_enc.h): int16 samples on the GPU -- what MobiclipAudio.decode wrote, planar -- to Moflex audio
frames, IMA-ADPCM or PCM16, one frame per stream and call, left on the GPU for the muxer (mux.MobiclipMuxer.append_audio).  Frames are
only ever produced by the HIP kernels (mobi_audio_enc.hip); DESIGN.md, "Audio encoder", has the rule."""
import ctypes as C

import numpy as np

from .binding import Handle, bind
from .decoder import MobiclipError, check_rc, check_stream, default_device, load_library

CODECS = {"ima": 1, "pcm16": 2}            # MOBI_AUDIO_IMA, MOBI_AUDIO_PCM16: also the Moflex codec ids
REFUSED = {"fastaudio": 0, "sx": 3}        # MOBI_E_UNSUPPORTED
BLOCK_SAMPLES = 256
MAX_BLOCKS = 65535
# mobi_audio_enc_stats, one per (stream, channel)
STATS_DTYPE = np.dtype([("sse", "<u8"), ("clamped", "<u4"), ("start_index", "<u4")])

_P = C.c_void_p
# names must match include/mobiclip_audio_enc.h (tests/test_audio_enc_model.py checks header, library and this table)
_SIGS = {
    "mobi_audio_enc_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mobi_audio_enc_destroy": (None, [C.c_void_p]),
    "mobi_audio_enc_frame_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mobi_audio_enc_check": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.c_int, _P, C.c_size_t, C.c_size_t, _P, _P, C.c_size_t, _P]),
    "mobi_audio_enc_async": (C.c_int, [C.c_void_p, _P, C.c_int, _P, C.c_size_t, C.c_int, _P, C.c_size_t, C.c_size_t, _P, _P, C.c_size_t, _P]),
}


def _lib():
    return bind(load_library(), _SIGS)


def _codec(codec):
    if codec in REFUSED or codec in tuple(REFUSED.values()):
        raise MobiclipError(f"no encoder for audio codec {codec!r}: IMA-ADPCM ('ima') and PCM16 ('pcm16') are written")
    if codec in CODECS:
        return CODECS[codec]
    if isinstance(codec, bool) or not isinstance(codec, (int, np.integer)) or int(codec) not in CODECS.values():
        raise ValueError(f"codec must be one of {sorted(CODECS)} or a Moflex codec id in {sorted(CODECS.values())}, not {codec!r}")
    return int(codec)


def frame_bytes(codec, n_channels, blocks):
    """mobi_audio_enc_frame_bytes: 4 C + 128 C blocks (IMA), 512 C blocks (PCM16)"""
    return int(_lib().mobi_audio_enc_frame_bytes(_codec(codec), int(n_channels), int(blocks)))


class MobiclipAudioEncoder(Handle):
    """mobi_audio_enc: Moflex audio frames of n_channels channels for up to n_streams streams per call, up to max_blocks blocks of 256
    samples per channel and call.  codec: "ima" or "pcm16" (or the Moflex codec id, 1 or 2).  The encoder keeps no state between calls:
    a Moflex frame is read by decoders made new for it."""
    _destroy = "mobi_audio_enc_destroy"

    def __init__(self, n_streams, n_channels, codec, max_blocks, device=None):
        self._h = None
        self._lib = _lib()
        self.codec_id = _codec(codec)
        self.n_streams, self.n_channels, self.max_blocks = int(n_streams), int(n_channels), int(max_blocks)
        if not 1 <= self.n_channels <= 8 or self.n_streams < 1 or self.n_streams * self.n_channels >= 1 << 24 or not 1 <= self.max_blocks <= MAX_BLOCKS:
            raise ValueError(f"n_channels must be in [1, 8], n_streams * n_channels in [1, 2**24) and max_blocks in [1, {MAX_BLOCKS}]")
        self.device = default_device() if device is None else int(device)
        self._h = self._lib.mobi_audio_enc_create(self.device, self.codec_id, self.n_streams, self.n_channels, self.max_blocks)
        if not self._h:
            raise MobiclipError("mobi_audio_enc_create failed: no usable HIP device, or out of device memory")

    def frame_bytes(self, blocks):
        return int(self._lib.mobi_audio_enc_frame_bytes(self.codec_id, self.n_channels, int(blocks)))

    def encode(self, samples, recon=False, stats=False, slot_bytes=None, stream=None):
        """samples: an (N, n_channels, S) int16 torch tensor on the encoder's device, N <= n_streams, S = 256 B with B <= max_blocks; a
        view whose last axis is a slice of longer rows (a planar MobiclipAudio.decode output with max_samples > S) is encoded where it
        lies.  slot_bytes: the room of one frame (a multiple of 4; default: the frame's length rounded up to 4).

        Returns (frames, sizes[, dict]): frames (N, slot_bytes) uint8 with a frame at the start of each row, sizes (N,) int32 their
        lengths -- what MobiclipMuxer.append_audio takes --, enqueued on `stream` (default: torch's current one) and NOT waited for, as
        the video encoders' tensor form.  With recon and / or stats the dict holds "recon", an (N, n_channels, S) int16 tensor: what a
        decoder returns for the frames (for PCM16 with one channel the decoder also returns one more sample, 0, made by the two zero
        bytes the demuxer appends), and "stats", an (N * n_channels, 16) uint8 tensor of STATS_DTYPE records."""
        import torch
        if not self._h:
            raise MobiclipError("encoder is closed")
        dev = torch.device("cuda", self.device)
        check_stream(stream, dev)
        if not isinstance(samples, torch.Tensor) or samples.dtype != torch.int16 or samples.device != dev or samples.ndim != 3:
            raise ValueError(f"samples must be an (N, {self.n_channels}, S) int16 tensor on {dev}")
        n, nc, S = (int(v) for v in samples.shape)
        if nc != self.n_channels or not 1 <= n <= self.n_streams or S < BLOCK_SAMPLES or S % BLOCK_SAMPLES or S // BLOCK_SAMPLES > self.max_blocks:
            raise ValueError(f"samples must be (N <= {self.n_streams}, {self.n_channels}, 256 B) with B in [1, {self.max_blocks}], not {tuple(samples.shape)}")
        # sample k of channel c of stream s lies at (s C + c) pitch + k (the stride of an axis of length 1 says nothing)
        pitch = int(samples.stride(1)) if nc > 1 else int(samples.stride(0)) if n > 1 else S
        if samples.stride(2) != 1 or pitch < S or (nc > 1 and n > 1 and samples.stride(0) != nc * pitch):
            raise ValueError("samples must be contiguous, or a slice of the last axis of a contiguous (N, C, longer) tensor")
        blocks = S // BLOCK_SAMPLES
        need = self.frame_bytes(blocks)
        slot = (need + 3) & ~3 if slot_bytes is None else int(slot_bytes)
        if slot % 4 or slot < need:
            raise ValueError(f"slot_bytes must be a multiple of 4 and at least the frame's {need} bytes")
        s = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.stream(s):
            frames = torch.empty((n, slot), dtype=torch.uint8, device=dev)
            sizes = torch.empty((n,), dtype=torch.int32, device=dev)
            rec = torch.empty((n, nc, S), dtype=torch.int16, device=dev) if recon else None
            st = torch.empty((n * nc, STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev) if stats else None
        check_rc(self._lib.mobi_audio_enc_async(self._h, s.cuda_stream, n, samples.data_ptr(), pitch, blocks, frames.data_ptr(), slot, slot, sizes.data_ptr(),
                                                rec.data_ptr() if recon else None, S, st.data_ptr() if stats else None))
        if s != torch.cuda.current_stream(dev):
            samples.record_stream(s)
        extra = {}
        if recon:
            extra["recon"] = rec
        if stats:
            extra["stats"] = st
        return (frames, sizes, extra) if extra else (frames, sizes)
