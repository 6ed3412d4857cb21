"""Restarting single clips of a batch with a new stream (mobi_batch_reset_clips, mobi_batch_clip_frames; mobi_reset.hip).

A reset gives a clip a new MobiclipDecoder (MD.cs:41-54) from the next frame step handed over on.  Every frame of a reset clip must then be
what a fresh decoder gives for the new stream -- the oracle, and a fresh batch in the same parse mode -- on every path (decode, submit / wait
with two steps in flight, decode_gop, pipelined gop_begin / gop_finish in parts), in every parse mode, in both versions; the clips that were
never reset must not notice (bit for bit what a batch without the reset gives); the same schedule without the reset call must fail the check.
New streams are (a) another stream from its first frame, (b) a suffix from a mid-stream I-frame (a seek), (c) a suffix from a P-frame (a fresh
decoder answers MOBI_E_NULLREF for the references it lacks)."""
import ctypes as C

import numpy as np
import pytest

from mobiclipdecoder_amd import MobiclipBatch, default_params, generate_clip
from mobiclipdecoder_amd.streamgen import BASE_SEED
from tests.gpu_streams import COVERAGE_SUITE
from tests.oracle_binding import OracleDecoder

W, H = 64, 48
N = 20  # parse mode 2: the hybrid share is the last N // 5 clips (16..19)
RESET = [1, 4, 5, 7, 10, 13, 16, 17, 18, 19]
EMPTY = np.zeros(0, np.uint8)


# ---- CPU: the interface ---------------------------------------------------------------------------------------------------------------
def test_header_library_and_bindings_declare_both_entry_points():
    import os
    import re
    from mobiclipdecoder_amd import decoder
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mobiclip_hip.h")).read(), flags=re.S)
    assert re.search(r"int mobi_batch_reset_clips\(mobi_batch \*b, const int32_t \*clips, int count\);", hdr)
    assert re.search(r"int mobi_batch_clip_frames\(const mobi_batch \*b, int32_t \*out\);", hdr)
    lib = decoder.load_library()
    for name in ("mobi_batch_reset_clips", "mobi_batch_clip_frames"):
        assert hasattr(lib, name) and name in decoder._SIGS
    assert decoder._SIGS["mobi_batch_reset_clips"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int])
    assert decoder._SIGS["mobi_batch_clip_frames"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)])
    assert hasattr(MobiclipBatch, "reset_clips") and hasattr(MobiclipBatch, "clip_frames")


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def mobi_batch_reset_clips(self, h, ptr, count):
        self.calls.append([ptr[i] for i in range(count)])
        return 0


def test_python_checks_indices_before_any_library_call():
    b = MobiclipBatch.__new__(MobiclipBatch)  # no device: the library is a recorder
    b._lib, b._h, b.n = _RecordingLib(), None, 6
    for bad in ([6], [-1], [0, 7], np.zeros(5, bool), np.zeros(7, bool), [1.5]):
        with pytest.raises(ValueError):
            b.reset_clips(bad)
    assert b._lib.calls == []
    b.reset_clips([3, 3, 0])
    b.reset_clips(np.array([True, False, False, False, False, True]))
    b.reset_clips([])
    assert b._lib.calls == [[3, 3, 0], [0, 5], []]


# ---- streams and schedules ------------------------------------------------------------------------------------------------------------
def _packets(p):
    d, fo = generate_clip(p)
    return [d[fo[f]:fo[f + 1]] for f in range(p.n_frames)]


def _stream(i, version, salt, n_frames):
    cfg, seed, kw = COVERAGE_SUITE[i % len(COVERAGE_SUITE)]
    kw = dict(kw, n_frames=n_frames, width=W, height=H, version=version, iframe_interval=6)
    return _packets(default_params(cfg, BASE_SEED + 31000 + 97 * seed + salt, **kw))


def _new_stream(kind, c, version, j):
    salt = 1000 * (j + 1) + c
    if kind == "a":  # another stream from its first frame
        return _stream(c + 3 * j + 1, version, salt, 12)
    if kind == "b":  # a seek: the suffix from the I-frame at frame 6
        s = _stream(c + 3 * j + 2, version, salt, 16)[6:]
        assert s[0][1] & 0x80
        return s
    s = _stream(c + 3 * j, version, salt, 12)[3:]  # a suffix from a P-frame
    assert not s[0][1] & 0x80
    return s


def _plan(version, units):
    """-> segments[c] = [(first step, packets, kind)], resets_before[u] = clips reset before unit u.  Resets sit on unit boundaries."""
    starts = np.concatenate([[0], np.cumsum(units)]).astype(int)
    segments = [[(0, _stream(c, version, c, 10 + c % 5), "-")] for c in range(N)]
    resets_before = [[] for _ in units]
    for i, c in enumerate(RESET):
        if len(units) > 6:  # single steps: first resets spread over steps 2..19, some clips reset again seven steps later
            us = [2 + (3 * i) % (len(units) - 4)]
            step = 7
        else:               # groups: any boundary, some clips at the next one again
            us = [1 + i % (len(units) - 1)]
            step = 1
        if c % 2 == 0 and us[0] + step < len(units):
            us.append(us[0] + step)
        for j, u in enumerate(us):
            kind = "abc"[(i + j) % 3]
            segments[c].append((int(starts[u]), _new_stream(kind, c, version, j), kind))
            resets_before[u].append(c)
    return segments, resets_before, starts


def _packet(segments, c, t):
    t0, pk, _ = max((s for s in segments[c] if s[0] <= t), key=lambda s: s[0])
    return pk[t - t0] if t - t0 < len(pk) else EMPTY


def _seg_of(segments, c, t):
    return max(i for i, s in enumerate(segments[c]) if s[0] <= t)


# ---- expectations: a fresh oracle and a fresh batch per stream --------------------------------------------------------------------------
def _oracle(segments, T, version):
    """[(c, t)] -> (rc, offset, planes or None, quantizer, yuv format, comparable): the taint rule of tests/test_gop.py per stream"""
    exp = {}
    for c in range(N):
        for i, (t0, pk, _) in enumerate(segments[c]):
            t1 = segments[c][i + 1][0] if i + 1 < len(segments[c]) else T
            o = OracleDecoder(W, H, version)
            hist = []
            for t in range(t0, t1):
                o.Data, o.Offset = _packet(segments, c, t), 0
                pl = o.DecodeFrame()
                ok = o.last_error == 0
                comparable = ok and (bool(o.Data[1] & 0x80) or all(hist[-5:]))
                hist.append(comparable)
                exp[(c, t)] = (o.last_error, o.Offset, pl, o.Quantizer, o.YuvFormat, comparable)
            o.close()
    return exp


def _fresh_batch(segments, T, version, mode):
    """every stream decoded from its first frame by a batch of its own clips, in the same parse mode: [(c, t)] -> (rc, offset, Y, UV)"""
    segs = [(c, i) for c in range(N) for i in range(len(segments[c]))]
    span = {}
    for c, i in segs:
        t1 = segments[c][i + 1][0] if i + 1 < len(segments[c]) else T
        span[(c, i)] = (segments[c][i][0], t1)
    L = max(t1 - t0 for t0, t1 in span.values())
    b = MobiclipBatch(len(segs), W, H, version, device_parse=mode)
    out = {}
    for s in range(L):
        row = [_packet(segments, c, span[(c, i)][0] + s) if span[(c, i)][0] + s < span[(c, i)][1] else EMPTY for c, i in segs]
        rcs, offs = b.decode(row, [0] * len(segs))
        for j, (c, i) in enumerate(segs):
            t = span[(c, i)][0] + s
            if t < span[(c, i)][1]:
                y, uv = b.planes(j, 0)
                out[(c, t)] = (rcs[j], offs[j], y.copy(), uv.copy())
    b.close()
    return out


# ---- the batch under test ------------------------------------------------------------------------------------------------------------
def _collect(segments, resets_before, units, version, mode, path, do_reset=True):
    """drive one batch through the schedule: [(c, t)] -> (rc, offset, Y, UV); [(c, t)] -> (quantizer, yuv format) where the call reported
    the frame t last; clip_frames checked against the schedule after every call"""
    b = MobiclipBatch(N, W, H, version, device_parse=mode)
    res, quant = {}, {}
    counted = np.zeros(N, np.int64)  # clip_frames as the schedule says
    epoch = np.zeros(N, np.int64)    # resets before unit epoch[c] apply to it and to the units behind it
    pending = []                     # (unit, t0, K) begun and not finished

    def report(t, rcs, offs, ring_idx, last=True):
        for c in range(N):
            y, uv = b.planes(c, ring_idx)
            res[(c, t)] = (rcs[c], offs[c], y.copy(), uv.copy())
            if last:
                quant[(c, t)] = (b.quantizer(c), b.yuv_format(c))

    def check_counts():
        assert np.array_equal(b.clip_frames(), counted), (b.clip_frames().tolist(), counted.tolist())

    def finish_oldest():
        u, t0, K = pending.pop(0)
        done = 0
        while done < K:
            rcs, offs = b.gop_finish()
            P = len(rcs)
            counted[epoch <= u] += P
            check_counts()
            for j in range(P):
                report(t0 + done + j, rcs[j], offs[j], P - 1 - j, last=j == P - 1)
            done += P

    t = 0
    for u, K in enumerate(units):
        if resets_before[u] and do_reset:
            b.reset_clips(resets_before[u])
            counted[resets_before[u]] = 0
            epoch[resets_before[u]] = u
            check_counts()
        frames = [[_packet(segments, c, t + k) for c in range(N)] for k in range(K)]
        if path == "decode":
            rcs, offs = b.decode(frames[0], [0] * N)
            counted += 1
            check_counts()
            report(t, rcs, offs, 0)
        elif path == "submit":
            b.submit(frames[0], [0] * N)
            counted += 1
            check_counts()
            pending.append(t)
            if len(pending) == 2:
                rcs, offs = b.wait()
                report(pending.pop(0), rcs, offs, 1)  # (the step behind it is in flight: the reported frame is ring index 1)
        elif path == "decode_gop":
            rcs, offs = b.decode_gop(frames)
            counted += K
            check_counts()
            for k in range(K):
                report(t + k, rcs[k], offs[k], K - 1 - k, last=k == K - 1)
        else:
            b.gop_begin(frames)
            check_counts()  # (a group's frames count when they turn the ring: in gop_finish)
            pending.append((u, t, K))
            if len(pending) == 2:
                finish_oldest()
        t += K
    while pending:
        if path == "submit":
            rcs, offs = b.wait()
            report(pending.pop(0), rcs, offs, len(pending))
        else:
            finish_oldest()
    hc = b.host_clips()
    b.close()
    return res, quant, hc


PATHS = [("decode", m) for m in (0, 1, 2, 3)] + [("submit", m) for m in (1, 2, 3)] + [("decode_gop", m) for m in (0, 1, 2, 3)] + \
        [("pipelined", m) for m in (1, 2, 3)]
UNITS = {"decode": [1] * 22, "submit": [1] * 22, "decode_gop": [6, 5, 6, 5], "pipelined": [5, 32, 12, 7]}


@pytest.mark.gpu
@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("path,mode", PATHS)
def test_gpu_reset_clips_decode_their_new_streams_exactly(path, mode, version):
    units = UNITS[path]
    segments, resets_before, _ = _plan(version, units)
    T = int(sum(units))
    exp = _oracle(segments, T, version)
    fresh = _fresh_batch(segments, T, version, mode)
    got, quant, _ = _collect(segments, resets_before, units, version, mode, path)
    twin, _, _ = _collect(segments, resets_before, units, version, mode, path, do_reset=False)
    assert len(got) == N * T
    for (c, t), (rc, off, y, uv) in sorted(got.items()):
        erc, eoff, epl, eq, ey, comparable = exp[(c, t)]
        frc, foff, fy, fuv = fresh[(c, t)]
        where = (path, mode, version, c, t, segments[c][_seg_of(segments, c, t)][2])
        # 1. every clip against a fresh decoder of its current stream, and against a fresh batch fed that stream from its start
        assert rc == erc == frc, (where, rc, erc, frc)
        assert off == foff, (where, off, foff)
        if rc == 0:
            assert off == eoff, (where, off, eoff)
            if (c, t) in quant:
                assert quant[(c, t)] == (eq, ey), (where, quant[(c, t)], (eq, ey))
        if comparable:
            assert np.array_equal(y, epl[0]) and np.array_equal(uv, epl[1]), ("planes differ from the oracle",) + where
            assert np.array_equal(y, fy) and np.array_equal(uv, fuv), ("planes differ from the fresh batch",) + where
        # 2. no cross-talk: a clip never reset is bit for bit what the batch without the reset gives
        if c not in RESET:
            trc, toff, ty, tuv = twin[(c, t)]
            assert (rc, off) == (trc, toff) and np.array_equal(y, ty) and np.array_equal(uv, tuv), ("cross-talk",) + where
    # 3. the check has power: without the reset call, every suffix that starts at a P-frame disagrees with the fresh oracle
    for c in RESET:
        for i, (t0, _, kind) in enumerate(segments[c]):
            if kind != "c":
                continue
            t1 = segments[c][i + 1][0] if i + 1 < len(segments[c]) else T
            bad = [t for t in range(t0, t1) if twin[(c, t)][0] != exp[(c, t)][0] or
                   (exp[(c, t)][5] and not np.array_equal(twin[(c, t)][2], exp[(c, t)][2][0]))]
            assert bad, (path, mode, version, c, t0)


# ---- repairs across the boundary ---------------------------------------------------------------------------------------------------
def _damaged_then_new(c, version=1):
    """ModsDS: an old stream whose last frame (an I-frame) is re-headed to quantiser 5 -- a frame the device parsers always hand to the host
    parser -- and a new stream"""
    from tests.test_internal_walk import _set_quantizer
    p = default_params("A", BASE_SEED + 32000 + c, n_frames=7, width=W, height=H, version=version, quantizer=12, pm_intra=150, cbp_prob=500,
                       iframe_interval=6)
    old = [x.copy() for x in _packets(p)]
    assert old[6][1] & 0x80
    _set_quantizer(old[6], 5)
    new = _packets(default_params("A", BASE_SEED + 32500 + c, n_frames=8, width=W, height=H, version=version, quantizer=14, pm_intra=150,
                                  cbp_prob=500))
    return old, new


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("pipelined", [False, True])
def test_gpu_repair_of_the_old_stream_in_flight_leaves_the_new_one_alone(mode, pipelined):
    n = 10
    share = n // 5 if mode == 2 else 0
    reset = [0, 3, 8, 9]  # (8, 9: the hybrid share in mode 2)
    streams = [_damaged_then_new(c) for c in range(n)]
    L = 7
    # the new stream of a clip that is not reset goes on as its old stream's continuation would: it is not, so its frames are just packets
    rows = [[streams[c][0][t] if t < L else streams[c][1][t - L] for c in range(n)] for t in range(L + 8)]

    def run(do_reset):
        b = MobiclipBatch(n, W, H, 1, device_parse=mode)
        out = {}
        hcs = []

        def rep(t, rcs, offs, ring):
            for c in range(n):
                y, uv = b.planes(c, ring)
                out[(c, t)] = (rcs[c], offs[c], y.copy(), uv.copy())

        if not pipelined:
            b.submit(rows[0], [0] * n)
            for t in range(1, len(rows)):
                b.submit(rows[t], [0] * n)  # two steps in flight
                if t == L - 1 and do_reset:
                    b.reset_clips(reset)  # two steps in flight, the second the damaged last frame of the old stream
                rcs, offs = b.wait()
                rep(t - 1, rcs, offs, 1)
                if t - 1 == L - 1:  # the damaged frame is reported (repaired behind the new stream's first step)
                    hcs.append(b.host_clips())
            rcs, offs = b.wait()
            rep(len(rows) - 1, rcs, offs, 0)
        else:
            b.gop_begin(rows[0:L])
            if do_reset:
                b.reset_clips(reset)  # the group holding the damaged frames is begun and not finished
            b.gop_begin(rows[L:L + 8])
            t = 0
            for K in (L, 8):
                t1 = t + K
                while t < t1:
                    rcs, offs = b.gop_finish()
                    P = len(rcs)
                    for j in range(P):
                        rep(t + j, rcs[j], offs[j], P - 1 - j)
                    t += P
                hcs.append(b.host_clips())
        cf = b.clip_frames()
        b.close()
        return out, hcs[0], cf

    got, hc, cf = run(True)
    ref, _, _ = run(False)
    for c in range(n):
        o = OracleDecoder(W, H, 1)
        for t in range(len(rows)):
            if t == L and c in reset:
                o.close()
                o = OracleDecoder(W, H, 1)
            rc, off, y, uv = got[(c, t)]
            if t < L or c not in reset:  # the old stream (and clips never reset) report what the batch without the reset reports
                rrc, roff, ry, ruv = ref[(c, t)]
                assert (rc, off) == (rrc, roff) and np.array_equal(y, ry) and np.array_equal(uv, ruv), (mode, pipelined, c, t)
            if t < L or c in reset:  # ... which is the oracle's; and the new stream is exact
                o.Data, o.Offset = rows[t][c], 0
                pl = o.DecodeFrame()
                assert rc == o.last_error == 0 and off == o.Offset, (mode, pipelined, c, t, rc, o.last_error)
                assert np.array_equal(y, pl[0]) and np.array_equal(uv, pl[1]), (mode, pipelined, c, t)
        o.close()
    # the damaged frame sends every clip to the host parser, except the reset ones: they are back with the device parsers (the hybrid share
    # stays with the host parser)
    assert hc == n - len([c for c in reset if c < n - share]), (mode, pipelined, hc)
    assert [int(x) for x in cf] == [8 if c in reset else L + 8 for c in range(n)]


# ---- counting and pixels ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_gpu_reset_moves_no_pixel(mode):
    n = 4
    olds = [_stream(c, 2, 500 + c, 8) for c in range(n)]
    new = _stream(9, 2, 777, 6)
    b = MobiclipBatch(n, W, H, 2, device_parse=mode)
    for t in range(8):
        b.decode([olds[c][t] for c in range(n)], [0] * n)
    before = [b.planes(1, r) for r in range(6)]
    exp_before = b.export("i420", ring_idx=5, n_frames=6, clips=range(1, 2))
    assert b.clip_frames().tolist() == [8] * n
    b.reset_clips([1])
    assert b.clip_frames().tolist() == [8, 0, 8, 8]
    for r in range(6):  # the call itself touches nothing
        assert all(np.array_equal(x, y) for x, y in zip(b.planes(1, r), before[r]))
    if mode:
        b.submit([olds[0][0], new[0], olds[2][0], olds[3][0]], [0] * n)  # the new stream's first frame enqueued
        assert b.clip_frames().tolist() == [9, 1, 9, 9]
        after = b.export("i420", ring_idx=5, n_frames=5, clips=range(1, 2))  # ring indices 5..1: the old stream's frames
        assert np.array_equal(after, exp_before[1:])
        rcs, _ = b.wait()
    else:
        rcs, _ = b.decode([olds[0][0], new[0], olds[2][0], olds[3][0]], [0] * n)
        assert b.clip_frames().tolist() == [9, 1, 9, 9]
    assert rcs[1] == 0
    for r in range(1, 6):  # ring index r >= min(6, clip_frames) = 1: the old stream's pictures, untouched
        assert all(np.array_equal(x, y) for x, y in zip(b.planes(1, r), before[r - 1]))
    o = OracleDecoder(W, H, 2)
    o.Data, o.Offset = new[0], 0
    pl = o.DecodeFrame()
    assert all(np.array_equal(x, y) for x, y in zip(b.planes(1, 0), pl))
    o.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_gpu_clip_frames_counts_groups_and_steps_in_flight(mode):
    n = 5
    st = [_stream(c, 1, 800 + c, 24) for c in range(n)]
    b = MobiclipBatch(n, W, H, 1, device_parse=mode)
    b.reset_clips([0, 1, 2, 3, 4])  # before the first frame: nothing changes
    assert b.clip_frames().tolist() == [0] * n
    b.gop_begin([[st[c][k] for c in range(n)] for k in range(8)])
    b.reset_clips([2])
    assert b.clip_frames().tolist() == [0] * n  # (the group has not turned the ring yet)
    b.gop_begin([[st[c][8 + k] for c in range(n)] for k in range(4)])
    b.gop_finish()
    assert b.clip_frames().tolist() == [6, 6, 0, 6, 6]  # a part of six: six ring turns, none of them the new stream's
    b.reset_clips([3])
    b.gop_finish()
    assert b.clip_frames().tolist() == [8, 8, 0, 0, 8]
    b.gop_finish()
    assert b.clip_frames().tolist() == [12, 12, 4, 0, 12]
    b.gop_begin([[st[c][12 + k] for c in range(n)] for k in range(2)])
    b.gop_finish()
    assert b.clip_frames().tolist() == [14, 14, 6, 2, 14]
    b.close()


# ---- refusals and no-ops ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gpu_refusals_and_noops_change_nothing(mode):
    from mobiclipdecoder_amd.decoder import load_library
    lib = load_library()
    n = 6
    st = [_stream(c, 2, 900 + c, 8) for c in range(n)]
    a = MobiclipBatch(n, W, H, 2, device_parse=mode)
    r = MobiclipBatch(n, W, H, 2, device_parse=mode)
    a.reset_clips([])
    a.reset_clips([0, 5])  # before the first frame
    for t in range(8):
        if t in (2, 5):
            arr = (C.c_int32 * 3)(1, 2, n)
            assert lib.mobi_batch_reset_clips(a._h, arr, 3) == -7        # an index outside [0, n): nothing of the list is recorded
            arr = (C.c_int32 * 2)(0, -1)
            assert lib.mobi_batch_reset_clips(a._h, arr, 2) == -7
            assert lib.mobi_batch_reset_clips(a._h, None, 2) == -7       # clips NULL, count > 0
            assert lib.mobi_batch_reset_clips(a._h, arr, -1) == -7       # count < 0
            assert lib.mobi_batch_reset_clips(None, arr, 1) == -7        # no batch
            assert lib.mobi_batch_clip_frames(None, None) == -7
            assert lib.mobi_batch_reset_clips(a._h, None, 0) == 0        # count == 0 does nothing
        ra, oa = a.decode([st[c][t] for c in range(n)], [0] * n)
        rr, orr = r.decode([st[c][t] for c in range(n)], [0] * n)
        assert (ra, oa) == (rr, orr), t
        assert np.array_equal(a.clip_frames(), r.clip_frames())
        for c in range(n):
            assert all(np.array_equal(x, y) for x, y in zip(a.planes(c), r.planes(c))), (t, c)
            assert (a.quantizer(c), a.yuv_format(c)) == (r.quantizer(c), r.yuv_format(c))
    assert a.host_clips() == r.host_clips()
    a.close()
    r.close()
