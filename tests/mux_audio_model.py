"""What tests/test_mux_audio_model.py and tests/test_mux_audio_gpu.py share: a restatement of the reference's Moflex writer for a file with
a video stream (index 0) and an audio stream (index 1), built on tests/containers.py's _ep, _varbyte and _synchro_header
(MoflexMuxer.cs:21-95, MoLiveStreamAudio.cs:29-37); sessions of video and audio append calls; and the binding of the
host model for such sessions (tests/tools/mobi_mux_audio_host.cpp, csrc/mobi_mux.h on the CPU)."""
import ctypes as C
import functools
import struct

import numpy as np

from tests import mux_model as M
from tests.containers import _ep, _synchro_header, _varbyte

AUDIO = (1, 32000, 2)  # codec id, frequency, channels
N = 3
B = M.B
AUDIO_LENS = (1, 2, 17, 3967, 3968, 3969, 7936, 7937)
# the append calls of a session: 0 a video frame for every clip, 1 an audio frame for every clip
KINDS = (0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 1)
VIDEO_LENS = ((12001, 5, 3968, 100), (7, 3969, 4, 7937), (64, 2, 3967, 11))  # clip 0 is longer than the others by more than a tail


def head(width, height, fps_rate, fps_scale, audio):
    video = bytes([0, 0]) + struct.pack(">HHHH", fps_rate, fps_scale, width, height) + bytes([1, 1])
    out = _synchro_header() + _varbyte(1) + _varbyte(12) + video
    if audio is not None:
        codec, frequency, channels = audio
        out += _varbyte(2) + _varbyte(6) + bytes([1, codec]) + (frequency - 1).to_bytes(3, "big") + bytes([channels - 1])
    return out + _varbyte(0) + _varbyte(0)


def frame(stream_index, data):
    """MoflexSimpleVideoMuxer's block loop for one frame of the given stream"""
    data, lim, out = bytes(data), 0x1000 - 0x80, bytearray()
    if len(data) <= lim:
        return b"\x01" + _ep(stream_index, data, True) + _ep(0, None, False)
    pos, left = 0, len(data)
    while left >= lim:
        out += b"\x01" + _ep(stream_index, data[pos:pos + lim], left == lim) + _ep(0, None, False)
        pos += lim
        left -= lim
    if left > 0:
        out += b"\x01" + _ep(stream_index, data[pos:pos + left], True) + _ep(0, None, False)
    return bytes(out)


def write(frames, width, height, fps_rate=30, fps_scale=1, audio=AUDIO, tail=True):
    """frames: (stream index, bytes) in file order"""
    return head(width, height, fps_rate, fps_scale, audio) + b"".join(frame(i, d) for i, d in frames) + (bytes(0x1000) if tail else b"")


@functools.lru_cache(maxsize=None)
def session():
    """sizes (T, N) int32, slots (T, N, slot) uint8 -- random behind each length too --, kinds (T,) uint8"""
    kinds = np.array(KINDS, np.uint8)
    sizes = np.zeros((len(KINDS), N), np.int32)
    for c in range(N):
        a = list(AUDIO_LENS[3 * c:] + AUDIO_LENS[:3 * c])
        v = list(VIDEO_LENS[c])
        for t, k in enumerate(KINDS):
            sizes[t, c] = a.pop(0) if k else v.pop(0)
    slot = (int(sizes.max()) + 3) & ~3
    slots = np.random.default_rng(20250).integers(0, 256, size=sizes.shape + (slot,), dtype=np.uint8)
    for arr in (sizes, slots, kinds):
        arr.setflags(write=False)
    return sizes, slots, kinds


def frames_of(sizes, slots, kinds, clip, upto=None):
    T = sizes.shape[0] if upto is None else upto
    return [(int(kinds[t]), slots[t, clip, :int(sizes[t, clip])].tobytes()) for t in range(T)]


def reference(sizes, slots, kinds, clip, upto=None, audio=AUDIO, tail=True):
    return np.frombuffer(write(frames_of(sizes, slots, kinds, clip, upto), M.W, M.H, M.FPS[0], M.FPS[1], audio, tail), np.uint8)


def ends(sizes, slots, kinds):
    """per clip: where its frames end (the tail follows)"""
    return [len(reference(sizes, slots, kinds, c, tail=False)) for c in range(sizes.shape[1])]


@functools.lru_cache(maxsize=None)
def host():
    from mobiclipdecoder_amd import build
    lib = C.CDLL(build.build_muxaudiohost())
    P = C.c_void_p
    lib.mux_host_run_audio.restype = C.c_int
    lib.mux_host_run_audio.argtypes = [C.c_int] + [C.c_uint32] * 5 + [C.c_int] * 3 + [P, C.c_size_t, C.c_size_t, P, C.c_size_t, C.c_size_t, P, P, P, P, C.c_int, C.c_uint32, C.c_int, P]
    lib.mux_host_fixed_bytes_audio.restype = C.c_uint64
    lib.mux_host_fixed_bytes_audio.argtypes = [C.c_int] * 3
    return lib


def run_host(sizes, slots, kinds, capacity, audio=AUDIO, guard=M.GUARD, container=M.MOFLEX):
    """-> (rc, files (n, capacity + guard) uint8 that were FILL, lengths (n,) int64, status (n,) int32)"""
    T, n = sizes.shape
    sizes, slots = np.ascontiguousarray(sizes, np.int32), np.ascontiguousarray(slots)
    kinds = None if kinds is None else np.ascontiguousarray(kinds, np.uint8)
    keys = np.zeros(T, np.uint8)
    files = np.full((n, capacity + guard), M.FILL, np.uint8)
    ln, st = np.zeros(n, np.int64), np.zeros(n, np.int32)
    slot = slots.shape[2]
    codec, freq, ch = audio if audio is not None else (0, 0, 0)
    rc = host().mux_host_run_audio(container, M.W, M.H, *M.FPS, 0, n, T, files.ctypes.data, capacity + guard, capacity, slots.ctypes.data, slot, slot,
                                   sizes.ctypes.data, keys.ctypes.data, ln.ctypes.data, st.ctypes.data, codec, freq, ch, None if kinds is None else kinds.ctypes.data)
    return rc, files, ln, st


def status_cases():
    """name -> (sizes, slots, kinds, capacity, expect): the smallest input at which an AUDIO frame raises each bit.  expect: per clip
    (status, append calls written before the refusal -- None for a clean clip)"""
    sizes, slots, kinds = session()
    T = sizes.shape[0]
    assert kinds[-1] == 1 and kinds[4] == 1
    e = ends(sizes, slots, kinds)
    assert e[0] > max(e[1:]) + 0x1000
    big = max(e) + 0x1000
    cases = {"capacity_last_audio_frame": (sizes, slots, kinds, e[0] - 1, [(M.ST_CAPACITY, T - 1), (0, None), (0, None)])}
    for name, value in (("audio_size_zero", 0), ("audio_size_above_slot", slots.shape[2] + 4)):
        s2 = sizes.copy()
        s2[4, 1] = value
        cases[name] = (s2, slots, kinds, big, [(0, None), (M.ST_STREAM, 4), (0, None)])
    return cases


def check_session(case, files, ln, st, guard=M.GUARD):
    sizes, slots, kinds, capacity, expect = case
    n = sizes.shape[1]
    assert files.shape == (n, capacity + guard)
    for c in range(n):
        status, written = expect[c]
        assert int(st[c]) == status, (c, int(st[c]), status)
        assert (files[c, capacity:] == M.FILL).all(), f"clip {c}: a byte at or behind the capacity was written"
        if status == 0:
            want = reference(sizes, slots, kinds, c)
            assert int(ln[c]) == len(want) and np.array_equal(files[c, :len(want)], want), f"clip {c} differs from the writer's file"
            continue
        assert int(ln[c]) == 0
        want = reference(sizes, slots, kinds, c, upto=written, tail=False)
        assert np.array_equal(files[c, :len(want)], want), f"clip {c}: the frames before the refusal differ"
        assert (files[c, len(want):] == M.FILL).all(), f"clip {c}: written behind the point of refusal"
