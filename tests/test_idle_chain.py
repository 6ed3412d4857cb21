"""Idle frame slots in the frame-parallel chain (mobiclipdecoder_amd/csrc/mobi_gop.h) on the CPU: the bodies of mobi_gop_prepare and
mobi_gop_chain (mobi_gop_prepare_clip / mobi_gop_chain_clip) compiled for the host (tests/tools/mobi_idle_host.cpp), over a group in which
clips carry the same stream and go idle at different frames.  A clip's first idle frame ends its chain CLEANLY: the verdict for its live
frames is that of a shorter group without idle frames, the start slot of the first idle frame and the batch's state ring get the state
behind the last live frame (the host parser's, in stream order), and nothing is flagged for the host parser."""
import ctypes as C

import numpy as np
import pytest

from mobiclipdecoder_amd import MobiclipBatch, build, default_params, generate_clip
from mobiclipdecoder_amd.streamgen import BASE_SEED

STATE, TAIL = 64, 1056  # sizeof(MobiDevState), sizeof(MobiDevTail): mobi_state.h


def tail_eq(a, b, p):
    """MobiDevTail: Internal[90..217] (512 bytes) and the MV row cache of a picture this wide, 2 * (mbw + 2) words; the rest is padding"""
    used = 512 + 4 * 2 * (p.width // 16 + 2)
    return np.array_equal(a[:used], b[:used])


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(build.build_idlehost())
    L.mobi_idle_chain_run.argtypes = [C.c_uint, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_void_p] * 6
    return L


def run(L, p, data, fo, pre, n, K, idle_from):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    fo = np.ascontiguousarray(fo, dtype=np.uint32)
    idle = None if idle_from is None else np.ascontiguousarray(idle_from, dtype=np.uint8)
    rc = np.zeros(K * n, np.int32)
    sin = np.zeros((K * n, STATE), np.uint8)
    ring, rtail = np.zeros((n, STATE), np.uint8), np.zeros((n, TAIL), np.uint8)
    ts, tt = np.zeros((K + 1, STATE), np.uint8), np.zeros((K + 1, TAIL), np.uint8)
    e = L.mobi_idle_chain_run(p.width, p.height, p.version, data.ctypes.data, fo.ctypes.data, pre, n, K, None if idle is None else idle.ctypes.data,
                              rc.ctypes.data, sin.ctypes.data, ring.ctypes.data, rtail.ctypes.data, ts.ctypes.data, tt.ctypes.data)
    assert e == 0
    return rc.reshape(K, n), sin.reshape(K, n, STATE), ring, rtail, ts, tt


STREAMS = [  # (config, seed, generator arguments): P-frames with quantiser deltas, an I-frame inside the group, both versions
    ("A", 7100, dict(width=96, height=64, version=2, qdelta_prob=600, pm_intra=150, pm_multiref=200)),
    ("B", 7101, dict(width=128, height=96, version=1, quantizer=30, qdelta_prob=400, iframe_interval=3, pm_intra=200)),
    ("A", 7102, dict(width=256, height=192, version=2, iframe_interval=4, qdelta_prob=800, table1_prob=500)),
]


@pytest.mark.parametrize("K", [3, 6])
@pytest.mark.parametrize("pre", [0, 2])
@pytest.mark.parametrize("idx", range(len(STREAMS)))
def test_idle_suffix_ends_the_chain_cleanly(lib, idx, pre, K):
    cfg, seed, kw = STREAMS[idx]
    p = default_params(cfg, BASE_SEED + seed, **dict(kw, n_frames=pre + K))
    data, fo = generate_clip(p)
    # clip 0: every frame live (the control); then clips idle from frame 0, 1, K - 1 and from the group's middle
    idle_from = [K, 0, 1, K - 1, K // 2]
    n = len(idle_from)
    rc, sin, ring, rtail, ts, tt = run(lib, p, data, fo, pre, n, K, idle_from)
    full = run(lib, p, data, fo, pre, 1, K, None)
    assert not full[0].any() and np.array_equal(full[2][0], ts[K]) and tail_eq(full[3][0], tt[K], p)  # the harness itself: a group without idle slots
    assert np.array_equal(ring[0], ts[K]) and tail_eq(rtail[0], tt[K], p) and np.array_equal(sin[:, 0], ts[:K])
    for c, j in enumerate(idle_from):
        # nothing is flagged for the host parser: no failed prediction, no unfinished frame, in the live frames or the idle ones
        assert not rc[:, c].any(), (c, j, rc[:, c])
        # the live frames: their true start states, equal to the control clip's
        assert np.array_equal(sin[:j, c], ts[:j]) and np.array_equal(sin[:j, c], sin[:j, 0]), (c, j)
        # the state ring gets the state behind the last live frame, and so does the slot of the first idle frame
        assert np.array_equal(ring[c], ts[j]) and tail_eq(rtail[c], tt[j], p), (c, j)
        if j < K:
            assert np.array_equal(sin[j, c], ts[j]), (c, j)
            assert (sin[j + 1:, c] == 0xAB).all(), "start slots behind the first idle frame are nobody's to write"
        # ... which is the verdict of the same clip in a shorter group without idle frames
        if j > 0:
            s_rc, s_sin, s_ring, s_rtail, _, _ = run(lib, p, data, fo, pre, 1, j, None)
            assert np.array_equal(s_rc[:, 0], rc[:j, c]) and np.array_equal(s_sin[:, 0], sin[:j, c])
            assert np.array_equal(s_ring[0], ring[c]) and tail_eq(s_rtail[0], rtail[c], p)


def test_all_intra_group_with_idle_middle(lib):
    """a stream of I-frames only (every frame sets YuvFormat and the quantiser anew), one clip live throughout, one idle from the middle"""
    p = default_params("A", BASE_SEED + 7103, width=96, height=64, version=2, n_frames=4, iframe_interval=1)
    data, fo = generate_clip(p)
    rc, sin, ring, rtail, ts, tt = run(lib, p, data, fo, 0, 2, 4, [4, 2])
    assert not rc.any()
    assert np.array_equal(ring[1], ts[2]) and np.array_equal(ring[0], ts[4]) and np.array_equal(sin[2, 1], ts[2])


# ---- the Python layer: shapes are checked with ValueError before the library is called -----------------------------------------------
EMPTY = np.zeros(0, np.uint8)


def test_python_checks_the_mask_and_the_group_shape_before_any_library_call():
    class Recorder:
        calls = 0

        def __getattr__(self, name):
            def f(*a):
                Recorder.calls += 1
                return 0
            return f
    b = MobiclipBatch.__new__(MobiclipBatch)
    b._lib, b._h, b.n = Recorder(), None, 4
    for bad in (np.zeros(3), np.zeros((2, 3)), np.zeros((2, 2, 4)), np.zeros((0, 4)), np.zeros((129, 4))):
        with pytest.raises(ValueError):
            b.set_idle(bad)
    with pytest.raises(ValueError):
        b.gop_begin([[EMPTY] * 4, [EMPTY] * 3])
    with pytest.raises(ValueError):
        b.decode_gop([[EMPTY] * 4], offsets=[[0] * 4, [0] * 4])
    assert Recorder.calls == 0
    b.set_idle(np.zeros(4))
    b.set_idle(np.zeros((3, 4)))
    b.set_idle(None)
    assert Recorder.calls == 3
