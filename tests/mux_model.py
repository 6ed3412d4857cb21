"""What tests/test_mux_model.py and tests/test_mux_gpu.py share: the clips (frame lengths, random slots, key flags), the binding of the
host model (tests/tools/mobi_mux_host.cpp, csrc/mobi_mux.h on the CPU) and the files tests/containers.py's writers make of the same clips."""
import ctypes as C
import functools

import numpy as np

from tests import containers

MOFLEX, MODS = 0, 1
ST_CAPACITY, ST_STREAM, ST_FRAME, ST_KEYS = 1, 2, 4, 8
W, H = 48, 32
FPS = (30, 1, 0x18000000)
N = 5                 # clips of a session, in a muxer of MAX_CLIPS
MAX_CLIPS = 8
GUARD = 64            # bytes between the rows: pitch = capacity + GUARD
FILL = 0xA5
B = 0xF80
# the lengths the issue names: around one, two and three Moflex blocks
LENS = (1, 2, 17, 3967, 3968, 3969, 7936, 7937, 11904, 12001)
MODS_LONGEST = (1 << 18) - 1
# behind a rotation of LENS every clip gets lengths that move the next frame's start through the residues mod 16 (test_coverage in
# tests/test_mux_model.py), and clip 0 enough to be longer than the others by more than a Moflex tail: the capacity cases refuse it alone
EXTRA = ((15, 12001, 6, 12001), (12, 7937, 4, 11904), (8, 3969, 3, 7937), (3, 12001, 3, 3968), (13, 7936, 11, 3969))


def lengths(container):
    """(T, N) int32: clip c's lengths are LENS rotated by 2 c, then EXTRA[c]; in Mods clip 1 also has the longest frame the format takes"""
    rows = []
    for c in range(N):
        seq = list(LENS[2 * c:] + LENS[:2 * c]) + list(EXTRA[c])
        if container == MODS and c == 1:
            seq[5] = MODS_LONGEST
        rows.append(seq)
    return np.array(rows, np.int32).T.copy()


def key_flags(T):
    return np.array([t % 3 == 0 for t in range(T)], np.uint8)


@functools.lru_cache(maxsize=None)
def clips(container):
    """sizes (T, N) int32, slots (T, N, slot) uint8 -- random behind each stream's length too --, keys (T,) uint8"""
    sizes = lengths(container)
    slot = (int(sizes.max()) + 3) & ~3
    rng = np.random.default_rng(20240 + container)
    slots = rng.integers(0, 256, size=sizes.shape + (slot,), dtype=np.uint8)
    for a in (sizes, slots):
        a.setflags(write=False)
    return sizes, slots, key_flags(sizes.shape[0])


# Moflex frames of more than 32 blocks: mobi_mux_append walks a frame's pieces with a grid of at most 32 workgroups, so these are the
# lengths at which a workgroup takes a second piece (LENS ends at four blocks) -- 32 blocks exactly, one byte more, 33 and a part, 64
# blocks (every workgroup a second piece), 65 and a part (the first a third) --, with short frames between them that move the next
# frame's start through the residues mod 16
LONG_LENS = (32 * B, 1, 32 * B + 1, 17, 33 * B + 17, 1, 64 * B, 17, 65 * B + 3)
LONG_N = 2


@functools.lru_cache(maxsize=None)
def long_moflex():
    """a Moflex session of LONG_N clips, clip 0 with LONG_LENS and clip 1 with LONG_LENS backwards, as clips() gives its own: sizes
    (T, 2) int32, slots (T, 2, slot) uint8 -- random behind each stream's length too --, keys (T,) uint8"""
    sizes = np.array([LONG_LENS, LONG_LENS[::-1]], np.int32).T.copy()
    slot = (int(sizes.max()) + 3) & ~3
    slots = np.random.default_rng(20242).integers(0, 256, size=sizes.shape + (slot,), dtype=np.uint8)
    for a in (sizes, slots):
        a.setflags(write=False)
    return sizes, slots, key_flags(sizes.shape[0])


def frames_of(sizes, slots, clip, upto=None):
    T = sizes.shape[0] if upto is None else upto
    return [slots[t, clip, :int(sizes[t, clip])].tobytes() for t in range(T)]


def reference(container, sizes, slots, keys, clip, upto=None):
    """the file tests/containers.py writes from the clip's first `upto` frames"""
    frames = frames_of(sizes, slots, clip, upto)
    if container == MOFLEX:
        return containers.write_moflex(frames, W, H, FPS[0], FPS[1], stream_index=0)
    return containers.write_mods(frames, W, H, [t for t in range(len(frames)) if keys[t]], audio_tail=b"", fps=FPS[2])


def frame_starts(container, sizes, clip):
    """where each frame of the clip starts in its file, from the writers' own output lengths"""
    if container == MOFLEX:
        per = [len(containers.write_moflex([bytes(int(n))], W, H)) - 30 - 0x1000 for n in sizes[:, clip]]
        pos = 30
    else:
        per = [4 + int(n) for n in sizes[:, clip]]
        pos = 0x30
    out = []
    for p in per:
        out.append(pos)
        pos += p
    return out, pos


@functools.lru_cache(maxsize=None)
def host():
    from mobiclipdecoder_amd import build
    lib = C.CDLL(build.build_muxhost())
    P = C.c_void_p
    lib.mux_host_run.restype = C.c_int
    lib.mux_host_run.argtypes = [C.c_int] + [C.c_uint32] * 5 + [C.c_int] * 3 + [P, C.c_size_t, C.c_size_t, P, C.c_size_t, C.c_size_t, P, P, P, P]
    lib.mux_host_framed_bytes.restype = lib.mux_host_fixed_bytes.restype = C.c_uint64
    lib.mux_host_framed_bytes.argtypes = [C.c_int, C.c_uint64]
    lib.mux_host_fixed_bytes.argtypes = [C.c_int, C.c_int]
    return lib


def run_host(container, sizes, slots, keys, capacity, max_keys, guard=GUARD, slot_bytes=None):
    """the host model over one session -> (rc, files (n, capacity + guard) uint8 that were FILL, lengths (n,) int64, status (n,) int32)"""
    T, n = sizes.shape
    sizes, slots, keys = np.ascontiguousarray(sizes, np.int32), np.ascontiguousarray(slots), np.ascontiguousarray(keys, np.uint8)
    files = np.full((n, capacity + guard), FILL, np.uint8)
    ln, st = np.zeros(n, np.int64), np.zeros(n, np.int32)
    slot = slots.shape[2]
    rc = host().mux_host_run(container, W, H, *FPS, max_keys, n, T, files.ctypes.data, capacity + guard, capacity, slots.ctypes.data, slot,
                             slot if slot_bytes is None else slot_bytes, sizes.ctypes.data, keys.ctypes.data, ln.ctypes.data, st.ctypes.data)
    return rc, files, ln, st


def capacity_of(container, sizes, keys):
    """room for the longest clip of the session"""
    return max(frame_starts(container, sizes, c)[1] for c in range(sizes.shape[1])) + (0x1000 if container == MOFLEX else 8 * int(keys.sum()))


def status_cases(container):
    """name -> (sizes, slots, keys, capacity, max_keys, expect): the smallest input that raises each status bit.  expect: per clip
    (status, frames written before the refusal -- None for a clean clip)"""
    sizes, slots, keys = clips(container)
    T, n = sizes.shape
    n_keys = int(keys.sum())
    tail = 0x1000 if container == MOFLEX else 8 * n_keys
    ends = [frame_starts(container, sizes, c)[1] for c in range(n)]
    longest = int(np.argmax(ends))
    assert sorted(ends)[-1] > sorted(ends)[-2]  # one clip is the longest: the capacity cases refuse it alone
    clean = [(0, None)] * n
    cases = {}

    def one(clip, status, written):
        e = list(clean)
        e[clip] = (status, written)
        return e
    cases["capacity_last_frame"] = (sizes, slots, keys, ends[longest] - 1, n_keys, one(longest, ST_CAPACITY, T - 1))
    cases["capacity_tail_only"] = (sizes, slots, keys, ends[longest] + tail - 1, n_keys, one(longest, ST_CAPACITY, T))
    big = capacity_of(container, sizes, keys)
    for name, value in (("size_zero", 0), ("size_above_slot", slots.shape[2] + 4)):
        s2 = sizes.copy()
        s2[4, 2] = value
        cases[name] = (s2, slots, keys, big, n_keys, one(2, ST_STREAM, 4))
    if container == MODS:
        s2 = sizes.copy()
        s2[5, 1] = 1 << 18  # the slot is exactly that long: the length itself is what is refused
        assert slots.shape[2] == 1 << 18
        cases["frame_2_18"] = (s2, slots, keys, big + 1, n_keys, one(1, ST_FRAME, 5))
        last_key = int(np.flatnonzero(keys)[-1])
        cases["one_key_too_many"] = (sizes, slots, keys, big, n_keys - 1, [(ST_KEYS, last_key)] * n)
    return cases


def check_session(container, case, files, ln, st, guard=GUARD):
    """files, lengths and status of a session against the writers' files and the case's expectation"""
    sizes, slots, keys, capacity, max_keys, expect = case
    n = sizes.shape[1]
    assert files.shape == (n, capacity + guard)
    for c in range(n):
        status, written = expect[c]
        assert int(st[c]) == status, (c, int(st[c]), status)
        assert (files[c, capacity:] == FILL).all(), f"clip {c}: a byte at or behind the capacity was written"
        if status == 0:
            want = reference(container, sizes, slots, keys, c)
            assert int(ln[c]) == len(want), (c, int(ln[c]), len(want))
            assert np.array_equal(files[c, :len(want)], want), f"clip {c} differs from the writer's file"
            continue
        assert int(ln[c]) == 0
        starts, end = frame_starts(container, sizes, c)
        stop = end if written == sizes.shape[0] else starts[written]  # the point of refusal
        assert (files[c, stop:] == FILL).all(), f"clip {c}: written behind the point of refusal"
        want = reference(container, sizes, slots, keys, c, upto=written)
        head = 30 if container == MOFLEX else 0x30
        assert np.array_equal(files[c, head:stop], want[head:stop]), f"clip {c}: the frames before the refusal differ"
        if container == MODS:
            assert (files[c, :head] == FILL).all()  # the header is finish's, and finish wrote nothing
