"""The motion ring and its export (mobi_batch_set_motion / mobi_batch_export_motion, mobi_motion.hip) on the GPU.

What the kernels must give is said on the CPU: the scripted clips' own vectors, and tests/tools/libmobi_motionhost.so (csrc/mobi_motion.h's
host build) over the host parser's command list -- tests/test_motion_field.py, which has checked the one against the other.
(That tool shares the header with the kernel.  The comparison with a side that does not -- the oracle's motion trace -- and the life-cycle
paths with motion on are tests/test_motion_oracle.py and tests/test_motion_trace_gpu.py.)
"""
import functools

import numpy as np
import pytest

from mobiclipdecoder_amd.streamgen import generate_clip
from tests.test_motion_field import N_FRAMES, WIDTHS, host_motion, scripted_case, seeded_params

MOBI_E_NULLREF, MOBI_E_ARG = -2, -7
CELLS, MB, FLOW = 0, 1, 2
F16, F32, I16, I32 = 1, 2, 3, 4


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _scripted_host(W, H):
    """-> per clip, per frame the CPU tool's mbs picture from the host parser's command list (computed once)"""
    p, clips, want = scripted_case(W, H)
    return [[fr[2] for fr in host_motion(p, data, fo)] for data, fo in clips]


@functools.lru_cache(maxsize=None)
def _seeded(n_clips=16, n_frames=8):
    """-> (params, clips, cells[clip][frame], mbs[clip][frame]) of the seeded streams through the host parser and the CPU tool"""
    ps = [seeded_params(i, n_frames) for i in range(n_clips)]
    clips = [generate_clip(p) for p in ps]
    host = [host_motion(p, data, fo) for p, (data, fo) in zip(ps, clips)]
    assert all(fr[0] == 0 for h in host for fr in h)
    return ps[0], clips, [[fr[1] for fr in h] for h in host], [[fr[2] for fr in h] for h in host]


def _frames(clips, f):
    return [d[fo[f]:fo[f + 1]] for d, fo in clips], [0] * len(clips)


def _run_path(path, p, clips, n_frames, monkeypatch):
    """every frame of `clips` through one decode path of a batch with motion on -> the batch"""
    import torch  # noqa: F401  (before the library: one HIP runtime)
    from mobiclipdecoder_amd import MobiclipBatch
    if path == "host_two_launches":
        monkeypatch.setenv("MOBI_FUSED_STEP_MBS", "0")  # (read when a batch is created)
    mode = {"host": 0, "host_two_launches": 0, "replay": 0, "device": 1, "lockstep": 3, "submit": 1, "submit_lockstep": 3, "gop": 1}[path]
    b = MobiclipBatch(len(clips), p.width, p.height, p.version, device_parse=mode)
    b.set_motion(True)
    assert b.motion_bytes() == len(clips) * 6 * (p.width // 16) * (p.height // 16) * 288 and b.motion_launches() == 0
    ok = [0] * len(clips)
    if path in ("host", "host_two_launches", "device", "lockstep"):
        for f in range(n_frames):
            assert b.decode(*_frames(clips, f))[0] == ok, (path, f)
    elif path in ("submit", "submit_lockstep"):
        b.submit(*_frames(clips, 0))
        for f in range(1, n_frames):
            b.submit(*_frames(clips, f))
            assert b.wait()[0] == ok, (path, f)
        assert b.wait()[0] == ok
    elif path == "gop":
        for f0 in range(0, n_frames, 3):
            K = min(3, n_frames - f0)
            assert b.decode_gop([_frames(clips, f0 + k)[0] for k in range(K)])[0] == [ok] * K, (path, f0)
    else:
        for c, (data, fo) in enumerate(clips):
            assert b.preload(c, data, fo) == [0] * n_frames
        b.commit()
        for f in range(n_frames):
            b.replay(f)
        b.sync()
    assert b.motion_launches() >= n_frames
    return b


PATHS = ["host", "host_two_launches", "device", "lockstep", "submit", "submit_lockstep", "gop", "replay"]


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("W,H", WIDTHS)
def test_gpu_scripted_vectors_on_every_decode_path(W, H, path, monkeypatch):
    """the scripted clips as one batch: "cells" is the script, "mb" the CPU tool's reading of the host parser's command list, whichever
    parser wrote the list the kernel read and whichever entry point launched the step"""
    p, clips, want = scripted_case(W, H)
    b = _run_path(path, p, clips, N_FRAMES, monkeypatch)
    try:
        cells = _np(b.export_motion("cells", ring_idx=N_FRAMES - 1, n_frames=N_FRAMES))
        mbs = _np(b.export_motion("mb", ring_idx=N_FRAMES - 1, n_frames=N_FRAMES))
        assert cells.shape == (N_FRAMES, len(clips), 3, H // 2, W // 2) and cells.dtype == np.int16
        assert mbs.shape == (N_FRAMES, len(clips), 5, H // 16, W // 16) and mbs.dtype == np.int32
        tool = _scripted_host(W, H)
        for f in range(N_FRAMES):
            for c in range(len(clips)):
                assert np.array_equal(cells[f, c], want[c][f]), (W, path, f, c, np.argwhere(cells[f, c] != want[c][f])[:4].tolist())
                assert np.array_equal(mbs[f, c], tool[c][f]), (W, path, f, c)
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["device", "host", "gop"])
def test_gpu_seeded_streams_ring_order_and_clip_ranges(path, monkeypatch):
    """16 clips x 8 frames with deep trees, several references and intra macroblocks: cells and mb are the CPU tool's; every ring index,
    every n_frames in the ring's order (oldest first), a clips= sub-range"""
    p, clips, hc, hm = _seeded()
    n, nf = len(clips), 8
    b = _run_path(path, p, clips, nf, monkeypatch)
    try:
        for r in range(6):
            cells, mbs = _np(b.export_motion("cells", ring_idx=r)), _np(b.export_motion("mb", ring_idx=r))
            for c in range(n):
                assert np.array_equal(cells[0, c], hc[c][nf - 1 - r]), (path, r, c)
                assert np.array_equal(mbs[0, c], hm[c][nf - 1 - r]), (path, r, c)
        for k in range(2, 7):
            cells = _np(b.export_motion("cells", ring_idx=k - 1, n_frames=k))
            for j in range(k):
                for c in range(n):
                    assert np.array_equal(cells[j, c], hc[c][nf - k + j]), (path, k, j, c)
        sub = _np(b.export_motion("mb", ring_idx=3, n_frames=2, clips=slice(3, 9)))
        assert sub.shape[:2] == (2, 6)
        for j in range(2):
            for c in range(3, 9):
                assert np.array_equal(sub[j, c - 3], hm[c][nf - 4 + j]), (path, j, c)
        sub = _np(b.export_motion("cells", ring_idx=0, clips=range(15, 16)))
        assert np.array_equal(sub[0, 0], hc[15][nf - 1])
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["device", "host"])
def test_gpu_a_clip_of_more_macroblocks_than_a_workgroup_takes(path, monkeypatch):
    """176x112 = 77 macroblocks: mobi_motion_field's workgroups take 64, so a clip is two of them, the second with 13 macroblocks in its first
    round and none in the others; the clips before and behind it must keep their own"""
    from tests.test_motion_field import host_motion as hm
    ps = [seeded_params(40 + i, 3, 176, 112) for i in range(3)]
    clips = [generate_clip(p) for p in ps]
    host = [hm(p, d, fo) for p, (d, fo) in zip(ps, clips)]
    assert all(fr[0] == 0 for h in host for fr in h)
    b = _run_path(path, ps[0], clips, 3, monkeypatch)
    try:
        cells, mbs = _np(b.export_motion("cells", 2, 3)), _np(b.export_motion("mb", 2, 3))
        assert (cells[1:, :, 2] > 0).any() and (mbs[:, :, 4] > 0).any()
        for f in range(3):
            for c in range(3):
                assert np.array_equal(cells[f, c], host[c][f][1]), (path, f, c)
                assert np.array_equal(mbs[f, c], host[c][f][2]), (path, f, c)
    finally:
        b.close()


def _flow_mirror(cells, block, scale, half):
    """include/mobiclip_hip.h's arithmetic on exported cells [..., 3, h, w] -> [..., 2, h / cb, w / cb]"""
    dx, dy, ref = (cells[..., i, :, :].astype(np.int64) for i in range(3))
    wgt = np.where(ref > 0, 60 // np.maximum(ref, 1), 0)
    cb = block // 2
    k = np.float32(np.float64(np.float32(scale)) / (120.0 * cb * cb))
    out = []
    for v in (dx * wgt, dy * wgt):
        s = v.reshape(v.shape[:-2] + (v.shape[-2] // cb, cb, v.shape[-1] // cb, cb)).sum((-3, -1))
        assert np.abs(s).max() < 2 ** 31
        out.append(s.astype(np.int32).astype(np.float32) * k)
    out = np.stack(out, -3)
    assert out.dtype == np.float32
    return out.astype(np.float16) if half else out


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["seeded_128", "scripted_80"])
def test_gpu_flow_is_the_header_arithmetic_bit_for_bit(which, monkeypatch):
    """blocks 2, 4, 8, 16, float32 and float16, scale 1 and 0.37, against the numpy mirror computed from the exported cells.  Width 80: rows
    of five floats, no 16-byte multiples"""
    import torch
    if which == "seeded_128":
        p, clips, _, _ = _seeded()
        nf = 8
    else:
        p, clips, _ = scripted_case(80, 48)
        nf = N_FRAMES
    b = _run_path("device", p, clips, nf, monkeypatch)
    try:
        k = min(nf, 6)
        cells = _np(b.export_motion("cells", ring_idx=k - 1, n_frames=k))
        assert (cells[:, :, 2] > 1).any() and (cells[:, :, 0] < 0).any() and (cells[:, :, 1] > 0).any()
        nonzero = 0
        for block in (2, 4, 8, 16):
            for dtype, bits in ((torch.float32, np.uint32), (torch.float16, np.uint16)):
                for scale in (1.0, 0.37):
                    got = _np(b.export_motion("flow", ring_idx=k - 1, n_frames=k, block=block, dtype=dtype, scale=scale))
                    want = _flow_mirror(cells, block, scale, dtype == torch.float16)
                    assert got.shape == want.shape == (k, len(clips), 2, p.height // block, p.width // block)
                    assert np.array_equal(got.view(bits), want.view(bits)), (which, block, dtype, scale, np.argwhere(got != want)[:4].tolist())
                    nonzero += int((got != 0).sum())
        assert nonzero > 1000
        # scale 1, block 2, one cell: dx / 2 pixels over ref frames
        one = _np(b.export_motion("flow", ring_idx=0, block=2))
        c0 = cells[-1].astype(np.float64)
        assert np.allclose(one[0, :, 0], np.where(c0[:, 2] > 0, c0[:, 0] / 2 / np.maximum(c0[:, 2], 1), 0), rtol=1e-6, atol=0)
    finally:
        b.close()


@pytest.mark.gpu
def test_gpu_a_clip_repaired_in_wait_gets_the_host_paths_motion():
    """an asynchronous step in which one clip's frame is not the device parser's to finish (a vector beyond the command list's fields:
    tests/test_parse_fallback.py's far frames): mobi_batch_wait repairs the clip, and its motion slot with it; the neighbours keep theirs"""
    import torch  # noqa: F401  (before the library: one HIP runtime)
    from mobiclipdecoder_amd import MobiclipBatch
    from tests.interp_binding import InterpDecoder
    from tests.test_motion_field import cells_picture, frame_motion, mbs_picture
    from tests.test_parse_fallback import _DC_MB, _frame, _part_code, _se_code, _ue_code
    ver = 2
    iframe = _frame("1" + "0" + "0" + format(20, "06b") + _DC_MB * 4)
    skip = _part_code(ver, 0, 0) + _ue_code(0)
    near = lambda dx, dy: _part_code(ver, 0, 1) + _se_code(dx) + _se_code(dy) + _ue_code(0)
    pframes = [_frame("0" + _se_code(0) + first + skip * 3) for first in (near(4, 2), near(8192, 0), near(-3, 6))]
    want = []
    for pf in pframes:
        d = InterpDecoder(32, 32, ver)
        for data in (iframe, pf):
            d.Data, d.Offset = data, 0
            d.DecodeFrame()
            assert d.last_error == 0
        cells, mbs = frame_motion(d.command_list()[0], d.payload(), 2, d.Stride)
        want.append((cells_picture(cells, 2), mbs_picture(mbs, 2)))
        d.close()
    assert (want[1][0][:, :8, :8] == np.array([0, 32, 1]).reshape(3, 1, 1)).all()
    b = MobiclipBatch(3, 32, 32, ver, device_parse=1)
    try:
        b.set_motion(True)
        b.submit([iframe] * 3, [0] * 3)
        b.submit(pframes, [0] * 3)
        assert b.wait()[0] == [0] * 3 and b.host_clips() == 0
        assert b.wait()[0] == [0] * 3
        assert b.host_clips() == 1, "the far vector was meant to hand clip 1 to the host parser in wait"
        cells, mbs = _np(b.export_motion("cells")), _np(b.export_motion("mb"))
        for c in range(3):
            assert np.array_equal(cells[0, c], want[c][0]), (c, cells[0, c, :, 0, 0])
            assert np.array_equal(mbs[0, c], want[c][1]), c
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_gpu_an_idle_slot_leaves_the_live_clips_fields_alone(mode):
    import torch  # noqa: F401  (before the library: one HIP runtime)
    from mobiclipdecoder_amd import MobiclipBatch
    p, clips, want = scripted_case(128, 48)
    n = len(clips)
    b = MobiclipBatch(n, p.width, p.height, p.version, device_parse=mode)
    try:
        b.set_motion(True)
        for f in range(2):
            assert b.decode(*_frames(clips, f))[0] == [0] * n
        datas, offs = _frames(clips, 2)
        datas[2] = None
        b.set_idle([0, 0, 1, 0])
        rcs = b.decode(datas, offs)[0]
        assert rcs == [0, 0, 1, 0]  # MOBI_IDLE
        cells = _np(b.export_motion("cells", ring_idx=1, n_frames=2))
        for c in range(n):
            assert np.array_equal(cells[0, c], want[c][1]), c
            if c != 2:
                assert np.array_equal(cells[1, c], want[c][2]), c
    finally:
        b.close()


@pytest.mark.gpu
def test_gpu_motion_enabled_late():
    """switched on after two frames: ring index 0 works after the next frame; the older ones were never produced"""
    import torch
    from mobiclipdecoder_amd import MobiclipBatch, MobiclipError
    p, clips, hc, hm = _seeded()
    clips, n = clips[:4], 4
    b = MobiclipBatch(n, p.width, p.height, p.version, device_parse=0)
    try:
        for f in range(2):
            b.decode(*_frames(clips, f))
        assert b.motion_launches() == 0 and b.motion_bytes() == 0
        b.set_motion(True)
        out = torch.zeros((3, n, 3, p.height // 2, p.width // 2), dtype=torch.int16, device=torch.device("cuda", b.device))
        call = lambda r, nf: b._lib.mobi_batch_export_motion(b._h, CELLS, I16, 2, 1.0, r, nf, 0, n, out.data_ptr(), out.numel() * 2,
                                                             torch.cuda.current_stream(out.device).cuda_stream)
        assert call(0, 1) == MOBI_E_NULLREF and call(1, 2) == MOBI_E_NULLREF
        b.decode(*_frames(clips, 2))
        assert b.motion_launches() == 1
        assert call(1, 1) == MOBI_E_NULLREF and call(1, 2) == MOBI_E_NULLREF and call(2, 3) == MOBI_E_NULLREF and call(3, 1) == MOBI_E_NULLREF
        with pytest.raises(MobiclipError):
            b.export_motion("cells", ring_idx=1)
        assert not _np(out).any()
        cells = _np(b.export_motion("cells"))
        for c in range(n):
            assert np.array_equal(cells[0, c], hc[c][2]), c
        b.decode(*_frames(clips, 3))
        assert call(1, 2) == 0 and call(2, 1) == MOBI_E_NULLREF
        got = _np(out)
        for c in range(n):
            assert np.array_equal(got[0, c], hc[c][2]) and np.array_equal(got[1, c], hc[c][3]), c
        # off and on again: the frames decoded in between have no slot
        b.set_motion(False)
        assert b.motion_bytes() == 0
        b.decode(*_frames(clips, 4))
        b.set_motion(True)
        assert call(0, 1) == MOBI_E_NULLREF
        b.decode(*_frames(clips, 5))
        cells = _np(b.export_motion("mb"))
        for c in range(n):
            assert np.array_equal(cells[0, c], hm[c][5]), c
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_gpu_motion_never_enabled_costs_nothing(mode):
    """export_motion raises, set_motion(False) is a no-op, and decoding allocates no ring and launches no mobi_motion_field"""
    import torch
    from mobiclipdecoder_amd import MobiclipBatch, MobiclipError
    p, clips, want = scripted_case(128, 48)
    n = len(clips)
    b = MobiclipBatch(n, p.width, p.height, p.version, device_parse=mode)
    try:
        b.set_motion(False)
        for f in range(N_FRAMES):
            assert b.decode(*_frames(clips, f))[0] == [0] * n
        b.set_motion(False)
        assert b.motion_launches() == 0 and b.motion_bytes() == 0
        for fmt in ("cells", "mb", "flow"):
            with pytest.raises(MobiclipError):
                b.export_motion(fmt)
        out = torch.zeros(1 << 16, dtype=torch.uint8, device=torch.device("cuda", b.device))
        assert b._lib.mobi_batch_export_motion(b._h, CELLS, I16, 2, 1.0, 0, 1, 0, 1, out.data_ptr(), out.numel(), None) == MOBI_E_ARG
        assert not _np(out).any()
    finally:
        b.close()


@pytest.mark.gpu
def test_gpu_motion_export_refusals_enqueue_nothing():
    """tests/test_export_device.py::test_device_export_refusals_enqueue_nothing for mobi_batch_export_motion; set_motion with work in flight"""
    import torch
    from mobiclipdecoder_amd import MobiclipBatch, MobiclipError, host_empty
    p, clips, want = scripted_case(128, 48)
    n, W, H = 3, p.width, p.height
    clips = clips[:n]
    b = MobiclipBatch(n, W, H, p.version, device_parse=True)
    lib, h = b._lib, b._h
    dev = torch.device("cuda", b.device)
    cells_pic, mb_pic = 3 * (H // 2) * (W // 2) * 2, 5 * (H // 16) * (W // 16) * 4
    out = torch.full((6 * n * cells_pic + 64,), 0xAB, dtype=torch.uint8, device=dev)
    ptr, nb = out.data_ptr(), out.numel()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ex = lambda fmt, dt, blk, r, nf, c0, nc, d=ptr, nbytes=nb, scale=1.0: lib.mobi_batch_export_motion(h, fmt, dt, blk, scale, r, nf, c0, nc, d, nbytes, stream)
    try:
        b.set_motion(True)
        assert ex(CELLS, I16, 2, 0, 1, 0, n) == MOBI_E_NULLREF
        b.decode(*_frames(clips, 0))
        b.decode(*_frames(clips, 1))
        assert ex(CELLS, I16, 2, 2, 1, 0, n) == MOBI_E_NULLREF
        host, pinned = np.zeros(nb, np.uint8), host_empty(nb, np.uint8)
        flow_pic = lambda blk, es: 2 * (H // blk) * (W // blk) * es
        refused = [
            ex(CELLS, I16, 2, 0, 1, 0, n, d=host.ctypes.data), ex(MB, I32, 16, 0, 1, 0, n, d=pinned.ctypes.data),  # host memory
            ex(CELLS, I16, 2, 0, 1, 0, n, d=ptr + 2), ex(FLOW, F32, 16, 0, 1, 0, n, d=ptr + 8),                     # misaligned
            ex(CELLS, I16, 2, 1, 2, 0, n, nbytes=2 * n * cells_pic - 1), ex(MB, I32, 16, 0, 1, 0, n, nbytes=n * mb_pic - 1),
            ex(FLOW, F32, 4, 0, 1, 0, n, nbytes=n * flow_pic(4, 4) - 1), ex(FLOW, F16, 2, 0, 1, 0, n, nbytes=n * flow_pic(2, 2) - 1),
            ex(CELLS, I32, 2, 0, 1, 0, n), ex(CELLS, F32, 2, 0, 1, 0, n), ex(CELLS, I16, 4, 0, 1, 0, n), ex(CELLS, I16, 16, 0, 1, 0, n),  # dtype / block
            ex(MB, I16, 16, 0, 1, 0, n), ex(MB, I32, 2, 0, 1, 0, n), ex(MB, I32, 8, 0, 1, 0, n),
            ex(FLOW, I16, 16, 0, 1, 0, n), ex(FLOW, 0, 16, 0, 1, 0, n), ex(FLOW, F32, 1, 0, 1, 0, n), ex(FLOW, F32, 3, 0, 1, 0, n), ex(FLOW, F32, 32, 0, 1, 0, n),
            ex(FLOW, F32, 0, 0, 1, 0, n), ex(FLOW, F32, 16, 0, 1, 0, n, scale=float("inf")), ex(FLOW, F16, 16, 0, 1, 0, n, scale=float("nan")),
            ex(3, I16, 2, 0, 1, 0, n), ex(-1, I16, 2, 0, 1, 0, n),
            ex(CELLS, I16, 2, 6, 1, 0, n), ex(CELLS, I16, 2, -1, 1, 0, n), ex(CELLS, I16, 2, 0, 2, 0, n), ex(CELLS, I16, 2, 1, 0, 0, n),
            ex(CELLS, I16, 2, 0, 1, -1, 1), ex(CELLS, I16, 2, 0, 1, 0, n + 1), ex(CELLS, I16, 2, 0, 1, n, 1), ex(CELLS, I16, 2, 0, 1, 0, 0),
            lib.mobi_batch_export_motion(h, CELLS, I16, 2, 1.0, 0, 1, 0, n, None, nb, stream),
        ]
        assert refused == [MOBI_E_ARG] * len(refused), refused
        # the Python layer refuses before any library call
        for kw in (dict(fmt="mv"), dict(fmt="cells", block=4), dict(fmt="mb", block=8), dict(fmt="flow", block=3), dict(fmt="flow", block=True),
                   dict(fmt="cells", dtype=torch.int32), dict(fmt="flow", dtype=torch.int16), dict(fmt="flow", scale=float("nan")), dict(fmt="flow", scale="x"),
                   dict(fmt="cells", scale=2.0), dict(fmt="cells", ring_idx=6), dict(fmt="cells", n_frames=0), dict(fmt="cells", ring_idx=0, n_frames=2),
                   dict(fmt="cells", clips=range(0, n + 1)), dict(fmt="cells", out=torch.zeros(3, device=dev)), dict(fmt="cells", stream=7)):
            with pytest.raises(ValueError):
                b.export_motion(**kw)
        # steps in flight: their ring indices are refused, and so is switching motion
        b.submit(*_frames(clips, 2))
        for r, nf in ((0, 1), (1, 2)):
            assert ex(CELLS, I16, 2, r, nf, 0, n) == MOBI_E_ARG, (r, nf)
        assert lib.mobi_batch_set_motion(h, 0) == MOBI_E_ARG and lib.mobi_batch_set_motion(h, 1) == 0  # (on already: nothing to do)
        with pytest.raises(MobiclipError):
            b.set_motion(False)
        torch.cuda.synchronize()
        assert bool((out == 0xAB).all())  # nothing was written
        assert b.wait()[0] == [0] * n
        assert ex(CELLS, I16, 2, 2, 3, 0, n) == 0
        t = b.export_motion("cells", 2, 3)
        got = _np(t)
        assert np.array_equal(_np(out)[:3 * n * cells_pic].view(np.int16).reshape(t.shape), got)
        for f in range(3):
            for c in range(n):
                assert np.array_equal(got[f, c], want[c][f]), (f, c)
        b.set_motion(False)  # (the exports above have run: torch.cuda.synchronize in _np)
        assert ex(CELLS, I16, 2, 0, 1, 0, n) == MOBI_E_ARG
    finally:
        b.close()
