"""The muxer (include/mobiclip_mux.h): the streams an encoder call left on the GPU, framed into .moflex / .mods file images that grow in
device memory frame by frame and cross to the host once, at finish(), and only as long as they are.  The framing is only ever done by the
HIP kernels (mobi_mux.hip); DESIGN.md, "Muxing", has the rule."""
import ctypes as C

import numpy as np

from .binding import Handle, bind
from .decoder import MobiclipError, MobiclipVersion, _check_one_hip_runtime, check_rc, check_stream, default_device, load_library

MOBI_MUX_MOFLEX, MOBI_MUX_MODS = 0, 1
CONTAINERS = {"moflex": MOBI_MUX_MOFLEX, "mods": MOBI_MUX_MODS}
# the stream version a container carries
CONTAINER_VERSION = {"moflex": MobiclipVersion.Moflex3DS, "mods": MobiclipVersion.ModsDS}
# MOBI_MUX_ST_*
STATUS_BITS = {1: "capacity: file_bytes is too small", 2: "stream: a length outside its slot", 4: "frame: 2^18 bytes or more", 8: "keys: max_key_frames is too small"}

_P = C.c_void_p
# names must match include/mobiclip_mux.h (tests/test_mux_model.py checks header, library and this table)
_SIGS = {
    "mobi_mux_create": (C.c_void_p, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int]),
    "mobi_mux_destroy": (None, [C.c_void_p]),
    "mobi_mux_framed_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "mobi_mux_fixed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mobi_mux_begin_async": (C.c_int, [C.c_void_p, _P, C.c_int, _P, C.c_size_t, C.c_size_t]),
    "mobi_mux_append_async": (C.c_int, [C.c_void_p, _P, C.c_int, _P, C.c_size_t, C.c_size_t, _P, C.c_int]),
    "mobi_mux_finish_async": (C.c_int, [C.c_void_p, _P, C.c_int, _P, _P]),
}

# the audio stream; names must match include/mobiclip_mux_audio.h (tests/test_mux_audio_model.py checks header, library and this table)
_AUDIO_SIGS = {
    "mobi_mux_set_audio": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_int]),
    "mobi_mux_fixed_bytes_audio": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mobi_mux_append_audio_async": (C.c_int, [C.c_void_p, _P, C.c_int, _P, C.c_size_t, C.c_size_t, _P]),
}
AUDIO_CODEC_IDS = {"fastaudio": 0, "ima": 1, "pcm16": 2}  # MoLiveStreamAudio.CodecId


def _lib():
    return bind(load_library(), _SIGS, _AUDIO_SIGS)


def _container(container):
    if container not in CONTAINERS:
        raise ValueError(f"container must be one of {sorted(CONTAINERS)}, not {container!r}")
    return CONTAINERS[container]


def framed_bytes(container, stream_bytes):
    """mobi_mux_framed_bytes: what a frame of stream_bytes occupies in a file of this container"""
    return int(_lib().mobi_mux_framed_bytes(_container(container), int(stream_bytes)))


def fixed_bytes(container, key_frames=0, audio=False):
    """mobi_mux_fixed_bytes: head plus tail (Moflex), header plus an index of key_frames entries (Mods); audio=True
    (mobi_mux_fixed_bytes_audio, Moflex): with the audio stream's chunk in the head"""
    if audio:
        if container != "moflex":
            raise ValueError("only a moflex file carries an audio stream")
        return int(_lib().mobi_mux_fixed_bytes_audio(_container(container), int(key_frames), 1))
    return int(_lib().mobi_mux_fixed_bytes(_container(container), int(key_frames)))


def status_names(status):
    return ", ".join(name for bit, name in STATUS_BITS.items() if status & bit) or hex(status)


class MobiclipMuxer(Handle):
    """mobi_mux: up to max_clips files of one container ("moflex" or "mods") side by side.  begin(), one append() per frame
    behind the encode call that made it, finish(); then the object takes the next session.  audio=(codec, frequency, channels): the
    Moflex files carry one audio stream as well (include/mobiclip_mux_audio.h), its frames brought by append_audio()."""
    _destroy = "mobi_mux_destroy"

    def __init__(self, container, width, height, max_clips, fps_rate=30, fps_scale=1, fps_raw=0x18000000, max_key_frames=1024, device=None, audio=None):
        self._h = None
        self._lib = _lib()
        self.container, self.width, self.height, self.max_clips = container, int(width), int(height), int(max_clips)
        self.device = default_device() if device is None else int(device)
        self._files = self._n = None
        _check_one_hip_runtime()
        self._h = self._lib.mobi_mux_create(_container(container), self.width, self.height, int(fps_rate), int(fps_scale), int(fps_raw), self.max_clips,
                                            int(max_key_frames), self.device)
        if not self._h:
            raise MobiclipError("mobi_mux_create failed: refused arguments, no usable HIP device, or out of device memory")
        self.audio = None
        if audio is not None:
            self.set_audio(*audio)

    def set_audio(self, codec, frequency, channels):
        """mobi_mux_set_audio, between sessions: the files of the sessions begun after it carry an audio stream (Moflex only) -- codec
        "fastaudio", "ima", "pcm16" or the Moflex codec id, frequency in [1, 2**24] Hz, channels in [1, 8]; append_audio() brings its
        frames.  frequency 0 switches audio off again."""
        if not self._h:
            raise MobiclipError("muxer is closed")
        if codec not in AUDIO_CODEC_IDS and (isinstance(codec, (str, bool)) or int(codec) not in AUDIO_CODEC_IDS.values()):
            raise ValueError(f"codec must be one of {sorted(AUDIO_CODEC_IDS)} or a Moflex codec id, not {codec!r}")
        cid = AUDIO_CODEC_IDS.get(codec, codec)
        check_rc(self._lib.mobi_mux_set_audio(self._h, int(cid), int(frequency), int(channels)))
        self.audio = (int(cid), int(frequency), int(channels)) if int(frequency) else None

    def _stream(self, stream):
        import torch
        if not self._h:
            raise MobiclipError("muxer is closed")
        dev = torch.device("cuda", self.device)
        check_stream(stream, dev)
        return dev, torch.cuda.current_stream(dev) if stream is None else stream

    def begin(self, n, file_bytes, stream=None):
        """Starts n files of at most file_bytes each: allocates the (n, file_bytes) uint8 tensor they grow in and enqueues the heads."""
        import torch
        dev, s = self._stream(stream)
        n, file_bytes = int(n), int(file_bytes)
        if not 1 <= n <= self.max_clips or file_bytes < 1:
            raise ValueError(f"n must be in [1, {self.max_clips}] and file_bytes at least 1")
        with torch.cuda.stream(s):  # torch's allocator then knows which stream uses the rows
            files = torch.empty((n, file_bytes), dtype=torch.uint8, device=dev)
        self._files = self._n = None
        check_rc(self._lib.mobi_mux_begin_async(self._h, s.cuda_stream, n, files.data_ptr(), file_bytes, file_bytes))
        self._files, self._n = files, n
        return files

    def append_audio(self, slots, sizes, stream=None):
        """One audio frame for every clip, as stream index 1: slots (n, slot_bytes) uint8 and sizes (n,) int32, the tensors
        MobiclipAudioEncoder.encode returned, read on the device behind that call.  Needs audio=(codec, frequency, channels)."""
        if self._h and self.audio is None:
            raise MobiclipError("append_audio on a muxer without an audio stream (audio=, set_audio)")
        self._append(slots, sizes, False, stream, True)

    def append(self, slots, sizes, key_frame, stream=None):
        """One frame for every clip: slots (n, slot_bytes) uint8 and sizes (n,) int32, the tensors an encoder call returned with slot_bytes
        given, read on the device behind that call.  key_frame: whether the frame is one, for every clip (Mods' index)."""
        self._append(slots, sizes, key_frame, stream, False)

    def _append(self, slots, sizes, key_frame, stream, audio):
        import torch
        dev, s = self._stream(stream)
        if self._files is None:
            raise MobiclipError("append before begin")
        for t, dtype, what in ((slots, torch.uint8, "slots"), (sizes, torch.int32, "sizes")):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous {dtype} tensor on {dev}")
        if slots.ndim != 2 or tuple(sizes.shape) != (self._n,) or int(slots.shape[0]) != self._n:
            raise ValueError(f"slots must be ({self._n}, slot_bytes) and sizes ({self._n},)")
        slot = int(slots.shape[1])
        if audio:
            check_rc(self._lib.mobi_mux_append_audio_async(self._h, s.cuda_stream, self._n, slots.data_ptr(), slot, slot, sizes.data_ptr()))
        else:
            check_rc(self._lib.mobi_mux_append_async(self._h, s.cuda_stream, self._n, slots.data_ptr(), slot, slot, sizes.data_ptr(), int(bool(key_frame))))
        if s != torch.cuda.current_stream(dev):
            slots.record_stream(s)
            sizes.record_stream(s)

    def finish(self, stream=None, to_host=True):
        """Ends the files.  to_host=False: (files, lengths, status) -- the (n, file_bytes) uint8 rows, (n,) int64 and (n,) int32 -- as
        device tensors, enqueued and not waited for; a clip with a status has length 0.  Otherwise the one wait: MobiclipError naming the
        first clip with a status and its bits, else a list of n bytes objects; only the files' own bytes cross to the host."""
        import torch
        dev, s = self._stream(stream)
        if self._files is None:
            raise MobiclipError("finish before begin")
        files, n = self._files, self._n
        with torch.cuda.stream(s):
            lengths = torch.empty((n,), dtype=torch.int64, device=dev)
            status = torch.empty((n,), dtype=torch.int32, device=dev)
        self._files = self._n = None
        check_rc(self._lib.mobi_mux_finish_async(self._h, s.cuda_stream, n, lengths.data_ptr(), status.data_ptr()))
        if not to_host:
            return files, lengths, status
        return files_to_host(files, lengths, status, s)


def files_to_host(files, lengths, status, stream=None):
    """what finish(to_host=False) returned -> the list of files as bytes; the used prefixes of the rows are gathered on the device and
    copied once"""
    import torch
    s = torch.cuda.current_stream(files.device) if stream is None else stream
    with torch.cuda.stream(s):
        host = torch.stack([lengths, status.to(torch.int64)]).cpu().numpy()  # waits: the lengths decide what is copied
        ln, st = host[0], host[1]
        bad = np.flatnonzero(st)
        if bad.size:
            raise MobiclipError(f"clip {int(bad[0])} could not be muxed: status {int(st[bad[0]]):#x} ({status_names(int(st[bad[0]]))}); "
                                f"{bad.size} of {len(st)} clips have a status")
        ends = np.cumsum(ln)
        packed = torch.cat([files[i, :int(ln[i])] for i in range(len(ln))]).cpu().numpy()
    return [packed[int(e - l):int(e)].tobytes() for e, l in zip(ends, ln)]
