"""The motion ring and its export on the GPU against the ORACLE's motion trace (oracle/mobi_oracle.h, mobi_oracle_motion_trace; the CPU side
of the comparison is tests/test_motion_oracle.py), on the decode paths and through the life-cycle events that tests/test_motion_export_gpu.py
does not reach with motion switched on: Moflex streams, reset_clips, a repair inside a group and in wait with a non-zero first clip, the
hybrid parse mode, a host-parsed batch of more than one upload chunk.

Every comparison is exact: "cells" against the trace's cells brought to the canonical member in numpy (canonical_cells), "mb" against the
trace's five values, "flow" bit for bit against the header's arithmetic applied to the TRACE's cells.  A clip whose frame is refused keeps an
unspecified slot; no stream here has such a frame, and every test asserts that it skipped none.
"""
import types

import numpy as np
import pytest

from mobiclipdecoder_amd.streamgen import BASE_SEED, default_params, generate_clip
from tests.test_motion_export_gpu import _flow_mirror, _np
from tests.test_motion_oracle import FAMILIES, canonical_cells, family, family_trace, oracle_motion


def _trace(clip):
    """(params, data, frame_off) -> per frame (canonical cells, mbs); every frame decodes"""
    frames, S = oracle_motion(*clip)
    assert all(fr[0] == 0 for fr in frames)
    return [(canonical_cells(cells, S), mbs) for _, cells, mbs in frames]


def _packet(clip, f):
    return clip[1][clip[2][f]:clip[2][f + 1]]


def _packets(clips, f):
    return [_packet(c, f) for c in clips], [0] * len(clips)


def _batch(clips, mode):
    import torch  # noqa: F401  (before the library: one HIP runtime)
    from mobiclipdecoder_amd import MobiclipBatch
    p = clips[0][0]
    assert all((c[0].width, c[0].height, c[0].version) == (p.width, p.height, p.version) for c in clips)
    b = MobiclipBatch(len(clips), p.width, p.height, p.version, device_parse=mode)
    b.set_motion(True)
    return b


def _run(path, clips, n_frames):
    """frames 0 .. n_frames - 1 of `clips` through one decode path with motion on -> the batch; every rc is 0 (no slot is skipped)"""
    b = _batch(clips, {"host": 0, "device": 1, "gop": 1, "lockstep": 3, "submit": 1}[path])
    ok = [0] * len(clips)
    if path in ("host", "device", "lockstep"):
        for f in range(n_frames):
            assert b.decode(*_packets(clips, f))[0] == ok, (path, f)
    elif path == "submit":
        b.submit(*_packets(clips, 0))
        for f in range(1, n_frames):
            b.submit(*_packets(clips, f))
            assert b.wait()[0] == ok, (path, f - 1)
        assert b.wait()[0] == ok
    else:
        for f0 in range(0, n_frames, 3):
            K = min(3, n_frames - f0)
            assert b.decode_gop([_packets(clips, f0 + k)[0] for k in range(K)])[0] == [ok] * K, (path, f0)
    return b


def _check_ring(b, want, what, flow=False):
    """want[c] = the (cells, mbs) of the frames clip c's ring holds, OLDEST first (all of one length K <= 6): ring indices K - 1 .. 0"""
    import torch
    K, n = len(want[0]), len(want)
    assert all(len(w) == K for w in want) and 1 <= K <= 6
    cells, mbs = _np(b.export_motion("cells", ring_idx=K - 1, n_frames=K)), _np(b.export_motion("mb", ring_idx=K - 1, n_frames=K))
    assert cells.dtype == np.int16 and mbs.dtype == np.int32 and cells.shape[:2] == mbs.shape[:2] == (K, n)
    for j in range(K):
        for c in range(n):
            wc, wm = want[c][j]
            assert np.array_equal(cells[j, c], wc), (what, "cells", j, c, np.argwhere(cells[j, c] != wc)[:4].tolist(), cells[j, c][cells[j, c] != wc][:4].tolist(), wc[cells[j, c] != wc][:4].tolist())
            assert np.array_equal(mbs[j, c], wm), (what, "mb", j, c, np.argwhere(mbs[j, c] != wm)[:4].tolist(), mbs[j, c][mbs[j, c] != wm][:4].tolist(), wm[mbs[j, c] != wm][:4].tolist())
    if flow:
        tc = np.stack([np.stack([want[c][j][0] for c in range(n)]) for j in range(K)])  # the trace's cells, [K, n, 3, h, w]
        for block in (2, 16):
            for dtype, bits in ((torch.float32, np.uint32), (torch.float16, np.uint16)):
                got = _np(b.export_motion("flow", ring_idx=K - 1, n_frames=K, block=block, dtype=dtype, scale=0.37))
                mirror = _flow_mirror(tc, block, 0.37, dtype == torch.float16)
                assert got.shape == mirror.shape and np.array_equal(got.view(bits), mirror.view(bits)), (what, "flow", block, dtype, np.argwhere(got != mirror)[:4].tolist())
    return cells, mbs


def _groups(name, pick=None):
    """a family's clips (at most six of them) with their traces, grouped by geometry and version: one batch each"""
    clips, traces = family(name), family_trace(name)
    idx = list(range(len(clips))) if pick is None else pick
    assert len(idx) <= 6
    out = {}
    for i in idx:
        p = clips[i][0]
        out.setdefault((p.width, p.height, p.version), []).append((clips[i], [(c, m) for c, m, _ in traces[i]]))
    return list(out.values())


# Pictures here are at most 512x64, with two exceptions that come with the families themselves: the coverage suite's streams have the
# sizes tests/gpu_streams.py gives them (four ModsDS streams of 256x192: rich, deep trees, intra-heavy, escapes; two Moflex of 640x480:
# rich, deep trees), and "resid" keeps the 640x32 of test_residual_rounds_16_bit_and_32_bit_by_quantizer.  Few clips, few frames: the
# whole file runs in about five seconds.
PICK = {"suite": [3, 5, 7, 10, 4, 6]}


# ---------------------------------------------------------------------------------------------------------------- 1, 2: families x paths
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["device", "host", "gop"])
@pytest.mark.parametrize("name", FAMILIES)
def test_gpu_every_ring_slot_is_the_oracles_trace(name, path):
    """the stream families of tests/test_motion_oracle.py: cells and mb of every ring slot equal the trace, and flow (float32 and float16,
    blocks 2 and 16, scale 0.37) is the header's arithmetic on the trace's cells, bit for bit"""
    for group in _groups(name, PICK.get(name)):  # (_run asserts rc 0 for every clip and frame: no slot is skipped)
        clips, traces = [g[0] for g in group], [g[1] for g in group]
        nf = min(8, min(len(t) for t in traces))
        b = _run(path, clips, nf)
        try:
            assert b.motion_launches() >= nf
            K = min(nf, 6)
            _check_ring(b, [t[nf - K:nf] for t in traces], (name, path, clips[0][0].width), flow=True)
        finally:
            b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["lockstep", "submit"])
def test_gpu_moflex_streams_in_lock_step_and_asynchronous_steps(path):
    """version 2 (the Moflex partition tables, the quantiser clamp): deep trees at Width == Stride, vectors that leave the picture, long
    level runs, hand-made far vectors"""
    n_batches = 0
    for name in ("deep", "edge", "resid", "alias", "far"):
        for group in _groups(name):
            clips, traces = [g[0] for g in group], [g[1] for g in group]
            if clips[0][0].version != 2:
                continue
            nf = min(8, min(len(t) for t in traces))
            b = _run(path, clips, nf)
            try:
                K = min(nf, 6)
                _check_ring(b, [t[nf - K:nf] for t in traces], (name, path, clips[0][0].width))
            finally:
                b.close()
            n_batches += 1
    assert n_batches == 6  # deep 512x32, edge 512x32, resid 640x32, alias 64x64 and 272x64, far 32x32: none skipped


# ---------------------------------------------------------------------------------------------------------------- 3: reset_clips
def _w80(i, n_frames=8):
    return default_params("A", BASE_SEED + 7320 + i, width=80, height=48, n_frames=n_frames, pm_deep=300, pm_multiref=400, pm_intra=100, cbp_prob=500,
                          t8_prob=500, max_coefs=10, scan_span=40, dense_prob=150)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["device", "host", "gop", "gop_pipelined", "submit"])
def test_gpu_a_reset_moves_no_motion_word(path):
    """four frames, reset_clips on clips 0, 2 and 4 (the first and the last) -- between two groups, behind a group begun and not yet
    finished, or with a step in flight --, three more frames.  Ring indices 0..2 of a reset clip hold the NEW stream's motion (its first frame all intra: ref 0, type 1), ring indices 3..5
    still hold the old stream's words exactly as exported before the reset, and the other clips hold their own throughout."""
    n, reset = 5, [0, 2, 4]
    olds = [(p,) + tuple(generate_clip(p)) for p in (_w80(i) for i in range(n))]
    news = {c: (p,) + tuple(generate_clip(p)) for c, p in zip(reset, (_w80(5 + i) for i in range(3)))}
    told, tnew = [_trace(c) for c in olds], {c: _trace(news[c]) for c in reset}
    ok = [0] * n
    after = lambda f: ([_packet(news[c], f - 4) if c in reset else _packet(olds[c], f) for c in range(n)], [0] * n)
    b = _batch(olds, {"device": 1, "host": 0, "gop": 1, "gop_pipelined": 1, "submit": 1}[path])
    try:
        if path == "gop":
            assert b.decode_gop([_packets(olds, f)[0] for f in range(4)])[0] == [ok] * 4
            before = _check_ring(b, [t[1:4] for t in told], (path, "before"))
            b.reset_clips(reset)
            assert b.decode_gop([after(f)[0] for f in range(4, 7)])[0] == [ok] * 3
        elif path == "gop_pipelined":
            b.gop_begin([_packets(olds, f)[0] for f in range(4)])
            b.reset_clips(reset)  # the group in flight is the old stream's
            b.gop_begin([after(f)[0] for f in range(4, 7)])
            assert b.gop_finish()[0] == [ok] * 4
            before = _check_ring(b, [t[1:4] for t in told], (path, "before"))  # (behind the reset call, before any of the new stream's steps)
            assert b.gop_finish()[0] == [ok] * 3
        elif path == "submit":
            b.submit(*_packets(olds, 0))
            for f in range(1, 4):
                b.submit(*_packets(olds, f))
                assert b.wait()[0] == ok
            b.reset_clips(reset)  # frame 3 is in flight: it is the old stream's
            cells, mbs = _np(b.export_motion("cells", ring_idx=2, n_frames=2)), _np(b.export_motion("mb", ring_idx=2, n_frames=2))  # frames 1 and 2
            for f in range(4, 7):
                b.submit(*after(f))
                assert b.wait()[0] == ok
            assert b.wait()[0] == ok
            before = None
        else:
            for f in range(4):
                assert b.decode(*_packets(olds, f))[0] == ok
            before = _check_ring(b, [t[1:4] for t in told], (path, "before"))
            b.reset_clips(reset)
            for f in range(4, 7):
                assert b.decode(*after(f))[0] == ok
        assert b.clip_frames().tolist() == [3 if c in reset else 7 for c in range(n)]
        want = [told[c][1:4] + (tnew[c][0:3] if c in reset else told[c][4:7]) for c in range(n)]
        got = _check_ring(b, want, (path, "after"), flow=True)
        if before is not None:  # the old stream's words, as they were
            assert np.array_equal(got[0][:3], before[0]) and np.array_equal(got[1][:3], before[1])
        else:
            assert np.array_equal(got[0][:2], cells) and np.array_equal(got[1][:2], mbs)
        for c in reset:  # the new stream's first frame: an I-frame
            assert not got[0][3, c].any() and (got[1][3, c, 0] == 1).all() and (got[0][4:, c, 2] > 0).any()
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 4, 5: repairs
def _far_group(n=4, far_clips=(1, 2), far_at=3):
    """32x32 Moflex clips of six hand-made frames; clips `far_clips` carry tests/test_parse_fallback.py's far vector (+8192, 0) -- a frame the
    device parsers hand to the host parser, and which decodes -- as frame `far_at`.  Different near vectors everywhere else."""
    from tests.test_parse_fallback import _DC_MB, _frame, _part_code, _se_code, _ue_code
    ver = 2
    iframe = _frame("1" + "0" + "0" + format(20, "06b") + _DC_MB * 4)
    skip = _part_code(ver, 0, 0) + _ue_code(0)
    leaf = lambda dx, dy, ref=1: _part_code(ver, 0, ref) + _se_code(dx) + _se_code(dy) + _ue_code(0)
    clips = []
    for c in range(n):
        frames = [iframe]
        for f in range(1, 6):
            first = leaf(8192, 0) if (c in far_clips and f == far_at) else leaf(1 + (3 * c + f) % 7, 2 * ((c + 2 * f) % 5), 1 + (c + f) % min(f, 3))
            frames.append(_frame("0" + _se_code(0) + first + skip * 3))
        p = types.SimpleNamespace(width=32, height=32, version=ver, n_frames=6)
        clips.append((p, np.concatenate(frames), np.concatenate([[0], np.cumsum([x.size for x in frames])])))
    return clips


@pytest.mark.gpu
def test_gpu_clips_repaired_inside_a_group_get_their_motion():
    """one group of six frames, device parse: clips 1 and 2 (adjacent, not the first) are handed to the host parser at frame 3 and the
    group's remaining steps are reconstructed for them again -- every slot of every clip is the trace"""
    clips = _far_group()
    traces = [_trace(c) for c in clips]
    assert all((t[3][0][:, :8, :8] == np.array([0, 32, 1]).reshape(3, 1, 1)).all() for t in traces[1:3])  # (+8192, 0) = sixteen rows down
    b = _batch(clips, 1)
    try:
        rcs = b.decode_gop([_packets(clips, f)[0] for f in range(6)])[0]
        assert rcs == [[0] * 4] * 6  # none refused, none skipped
        assert b.host_clips() == 2, "the far vectors were meant to hand clips 1 and 2 to the host parser inside the group"
        _check_ring(b, traces, "group repair", flow=True)
    finally:
        b.close()


@pytest.mark.gpu
def test_gpu_two_adjacent_clips_repaired_in_wait_get_their_motion():
    """the same clips in asynchronous steps: mobi_batch_wait repairs clips 1 and 2 in one run whose first clip is not clip 0 (and the step
    already in flight behind it); the neighbours on both sides keep theirs"""
    clips = _far_group()
    traces = [_trace(c) for c in clips]
    b = _batch(clips, 1)
    try:
        b.submit(*_packets(clips, 0))
        for f in range(1, 6):
            b.submit(*_packets(clips, f))
            assert b.wait()[0] == [0] * 4, f - 1
            assert b.host_clips() == (2 if f - 1 >= 3 else 0), (f, b.host_clips())
        assert b.wait()[0] == [0] * 4
        _check_ring(b, traces, "wait repair")
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 6: hybrid parse
@pytest.mark.gpu
def test_gpu_hybrid_parse_writes_both_shares_motion(monkeypatch):
    """parse mode 2, eight clips of which the last three are the host pool's (payload offsets relative to the arena, the host-parsed clips'
    lists behind the others)"""
    monkeypatch.setenv("MOBI_HYBRID_HOST_CLIPS", "3")  # (read when a batch is created)
    clips = [(p,) + tuple(generate_clip(p)) for p in (_w80(i, 6) for i in range(8))]
    traces = [_trace(c) for c in clips]
    b = _batch(clips, 2)
    try:
        for f in range(6):
            assert b.decode(*_packets(clips, f))[0] == [0] * 8, f
        assert b.host_clips() == 3
        _check_ring(b, traces, "hybrid")
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 7: upload chunks
@pytest.mark.gpu
def test_gpu_a_host_parsed_batch_of_three_upload_chunks():
    """768 clips of 32x32 parsed on the host, five frames, sixteen different streams: every clip holds its own stream's motion.
    mobi_batch_decode takes a host-parsed step in chunks of mobi_batch::host_chunk = 256 clips (parse, stage and upload overlapped) when
    the batch has at least two chunks -- 768 clips are three -- and the step's payload fits the buffers as the steps before left them
    (mobi_step_host.cpp); the first frame never does, and a step no larger than one before it always does.  The library has no
    counter for the path taken, so the sizes are checked here, from the host parser's own command lists: at least three of the four
    P-frame steps are no larger than a step before them."""
    from tests.test_motion_field import host_motion
    n, distinct, nf = 768, 16, 5
    src = [(p,) + tuple(generate_clip(p)) for p in (default_params("A", BASE_SEED + 7400 + i, width=32, height=32, n_frames=nf, pm_deep=300, pm_multiref=400,
                                                                 pm_intra=100, cbp_prob=500, mv_range=8) for i in range(distinct))]
    traces = [_trace(c) for c in src]
    assert len({t[2][0].tobytes() for t in traces}) == distinct  # (really different)
    words = np.sum([[fr[4].size for fr in host_motion(*c)] for c in src], 0) * (n // distinct)  # payload words of each step
    fits = [f for f in range(1, nf) if words[f] <= words[:f].max()]
    assert len(fits) >= 3, (words.tolist(), fits)
    clips = [src[c % distinct] for c in range(n)]
    b = _batch(clips, 0)
    try:
        for f in range(nf):
            assert b.decode(*_packets(clips, f))[0] == [0] * n, f
        _check_ring(b, [traces[c % distinct] for c in range(n)], "chunks")
    finally:
        b.close()
