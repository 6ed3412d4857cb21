"""The clip sink on the GPU (mobi_batch_set_sink, mobi_sink.hip; mobi_batch_gop_finish_all).  The expected tensor never comes from the code
under test: a TWIN batch decodes the same streams with decode(), one frame per call, on the host parser, and calls
export_tensor("rgb", boxes=..., flip=..., size=..., ring_idx=0) after every step -- the path the existing tests pin against numpy on the
Bitmap --; torch indexing puts the selected pictures in place.  Comparison is on the raw bits, without a tolerance.
Pictures are 64 x 48 (golden case mods_64x48_rich, ten frames, walked round and round: its first frame is an I-frame); every frame of every
step returns rc 0, which every test asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.test_export_device import AFFINES, GOLD, MAN, MOBI_E_ARG, PLANAR, ROOT, U8, _bits, _golden

pytestmark = pytest.mark.gpu

NAME = "mods_64x48_rich"
N = 5
BOXES = [(17, 9, 8, 6), (3, 2, 61, 45), (13, 5, 16, 12), (1, 1, 62, 46), (0, 0, 64, 48)]  # enlarging, shrinking, a pure crop, flipped, the whole picture
FLIPS = [False, False, False, True, False]
SIZE = (12, 16)
START = [0, 1, 2, 3, 0]
PKG = os.path.join(ROOT, "mobiclipdecoder_amd")


def _case():
    return next(c for c in MAN["cases"] if c["name"] == NAME)


def _frames(count, first=0):
    g = _golden(_case())
    return [g[(first + i) % len(g)] for i in range(count)]


def _batch(n=N, **kw):
    import torch  # noqa: F401  (before the library: one HIP runtime)
    from mobiclipdecoder_amd import MobiclipBatch
    c = _case()
    return MobiclipBatch(n, c["width"], c["height"], c["version"], **kw)


def _kw(dname, aff):
    import torch
    sb = AFFINES[aff]
    kw = dict(dtype=getattr(torch, dname))
    if sb is not None:
        kw.update(scale=sb[0].tolist(), bias=sb[1].tolist())
    return kw


_TWINS = {}


def _twin(steps, planar, dname, aff, boxes=BOXES, flips=FLIPS, size=SIZE, reset_at=None):
    """[step][clip] pictures (torch, on the GPU) of `steps` decode() steps, and the six ring pictures at the end [6][clip]; computed once per
    variant and never changed.  reset_at: (step, clip): the clip restarts with the stream's first frame at that step."""
    import torch
    key = (steps, planar, dname, aff, tuple(boxes), tuple(flips), size, reset_at)
    if key not in _TWINS:
        b = _batch(len(boxes), device_parse=False)
        n = len(boxes)
        pics = []
        fr = _frames(steps)
        for f in range(steps):
            per = [fr[f]] * n
            if reset_at and f >= reset_at[0]:
                if f == reset_at[0]:
                    b.reset_clips([reset_at[1]])
                per[reset_at[1]] = _frames(steps)[f - reset_at[0]]
            rcs, _ = b.decode([d for d, _ in per], [o for _, o in per])
            assert rcs == [0] * n, (f, rcs)
            pics.append(b.export_tensor("rgb", 0, 1, boxes=boxes, flip=flips, size=size, layout="nchw" if planar else "nhwc", **_kw(dname, aff))[0].clone())
        ring = b.export_tensor("rgb", min(5, steps - 1), min(6, steps)).clone()
        torch.cuda.synchronize()
        b.close()
        _TWINS[key] = (torch.stack(pics), ring)
    return _TWINS[key]


def _plan(T, s, start, step):
    return [c for c in range(len(start)) if step >= start[c] and (step - start[c]) % s == 0 and (step - start[c]) // s < T]


def _expected(pics, layout, T, s, start, steps, fill=0xA5):
    """the sink tensor of `steps` steps from the twin's pictures: layout "ntchw" / "nthwc" first, then permuted; what no step wrote holds `fill` bytes"""
    import torch
    n = len(start)
    base = torch.empty((n, T) + tuple(pics.shape[2:]), dtype=torch.uint8, device=pics.device).fill_(fill) if pics.dtype == torch.uint8 else None
    if base is None:
        raw = torch.empty((n, T) + tuple(pics.shape[2:]) + (pics.element_size(),), dtype=torch.uint8, device=pics.device).fill_(fill)
        base = raw.view(pics.dtype).squeeze(-1)
    for c in range(n):
        for t in range(T):
            if start[c] + t * s < steps:
                base[c, t] = pics[start[c] + t * s, c]
    perm = {"ntchw": None, "nthwc": None, "ncthw": (0, 2, 1, 3, 4), "tnchw": (1, 0, 2, 3, 4), "tnhwc": (1, 0, 2, 3, 4)}[layout]
    return base if perm is None else base.permute(*perm)


def _same(got, want, what):
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want.cpu().numpy())), what


LAYOUTS = ["ntchw", "ncthw", "nthwc", "tnchw", "tnhwc"]
DTYPES = [("uint8", "unit"), ("float16", "imagenet"), ("float32", "imagenet")]


def _run_decode(b, steps, T, s, start, check_pending=True):
    fr = _frames(steps)
    pend, launches = len(start) * T, b.sink_launches()
    for f in range(steps):
        rcs, _ = b.decode([fr[f][0]] * b.n, [fr[f][1]] * b.n)
        assert rcs == [0] * b.n
        sel = _plan(T, s, start, f)
        pend -= len(sel)
        launches += 1 if sel else 0
        if check_pending:
            assert b.sink_pending() == pend, (f, b.sink_pending(), pend)
            assert b.sink_launches() == launches, (f, b.sink_launches(), launches)
    return pend


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dname,aff", DTYPES)
def test_schedule_and_layouts(layout, dname, aff):
    """9 decode steps, T = 3, stride 2, start 0 1 2 3 0, five kinds of box: pending and launches after every step against the plan (host parse:
    no repairs), the tensor against the twin's, disarmed at the end"""
    planar = not layout.endswith("c")
    pics, _ = _twin(9, planar, dname, aff)
    b = _batch(device_parse=False)
    out = b.set_sink(size=SIZE, n_frames=3, stride=2, start=START, boxes=BOXES, flip=FLIPS, layout=layout, **_kw(dname, aff))
    assert b.sink_pending() == 15 and b.sink_launches() == 0
    assert _run_decode(b, 9, 3, 2, START) == 0
    assert b.sink_pending() == 0 and b.sink_launches() == 8  # (steps 0 .. 7: step 8 selects nobody)
    _same(out, _expected(pics, layout, 3, 2, START, 9), (layout, dname))
    b.close()


def test_canaries_gaps_completion_and_a_start_beyond_the_steps():
    import torch
    pics, _ = _twin(9, True, "uint8", "unit")
    for start, left in (([0, 1, 2, 3, 100], 3), (START, 0)):
        b = _batch(device_parse=False)
        big = torch.full((N + 1, 4, 4, 12, 16), 0xA5, dtype=torch.uint8, device="cuda")
        out = big[:N, :3, :3]  # a view with gaps between channels' ends, frames and clips
        got = b.set_sink(size=SIZE, n_frames=3, stride=2, start=start, boxes=BOXES, flip=FLIPS, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert _run_decode(b, 9, 3, 2, start) == left
        want = torch.full_like(big, 0xA5)
        want[:N, :3, :3] = _expected(pics, "ntchw", 3, 2, start, 9)
        _same(big, want, ("gaps", start))  # (clip 4 with start 100 keeps 0xA5, and so does every byte between the pictures)
        assert b.sink_pending() == left
        if left == 0:  # complete: the sink has disarmed itself, and two more steps write and launch nothing
            big.fill_(0x5A)
            torch.cuda.synchronize()
            launches = b.sink_launches()
            for d, o in _frames(2, first=9):
                assert b.decode([d] * N, [o] * N)[0] == [0] * N
            torch.cuda.synchronize()
            assert bool((big == 0x5A).all()) and b.sink_launches() == launches and b.sink_pending() == 0
        else:
            b.set_sink(None)
            assert b.sink_pending() == 0
        b.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_where_the_parse_runs(mode):
    pics, _ = _twin(9, True, "uint8", "unit")
    b = _batch(device_parse=mode)
    out = b.set_sink(size=SIZE, n_frames=3, stride=2, start=START, boxes=BOXES, flip=FLIPS)
    assert _run_decode(b, 9, 3, 2, START, check_pending=mode == 0) == 0
    assert b.sink_pending() == 0
    _same(out, _expected(pics, "ntchw", 3, 2, START, 9), mode)
    b.close()


def _gop_args(frames):
    return [[d] * N for d, _ in frames], [[o] * N for _, o in frames]


def test_groups_six_at_a_time_and_all_at_once():
    """two groups of 8 in flight through one sink (T = 8, stride 2: it spans both): parts of six, gop_finish_all, and gop_finish_all after one
    ordinary part give the twin's tensor, the same rc and offsets, and the twin's last six pictures in the ring"""
    import torch
    T, s, start = 8, 2, [0, 1, 0, 1, 0]
    pics, ring = _twin(16, False, "float16", "imagenet")
    want = _expected(pics, "nthwc", T, s, start, 16)
    fr = _frames(16)
    results = []
    for how in ("parts", "all", "part then all"):
        b = _batch(device_parse=True)
        out = b.set_sink(size=SIZE, n_frames=T, stride=s, start=start, boxes=BOXES, flip=FLIPS, layout="nthwc", **_kw("float16", "imagenet"))
        b.gop_begin(*_gop_args(fr[:8]))
        b.gop_begin(*_gop_args(fr[8:]))
        rcs, offs = [], []
        for g in range(2):
            assert b.gop_frames_pending() == 8
            if how == "part then all" and g == 0:
                r, o = b.gop_finish()
                assert len(r) == 6 and b.gop_frames_pending() == 2
                rcs += r; offs += o
            if how == "parts":
                for want_rows in (6, 2):  # (the group behind reports its own 8 as pending once this one is done)
                    r, o = b.gop_finish()
                    assert len(r) == want_rows
                    rcs += r; offs += o
            else:
                k = b.gop_frames_pending()
                r, o = b.gop_finish_all()
                assert len(r) == k and b.gop_frames_pending() == (8 if g == 0 else 0)
                rcs += r; offs += o
        assert len(rcs) == 16 and all(r == [0] * N for r in rcs)
        assert b.sink_pending() == 0
        _same(out, want, how)
        _same(b.export_tensor("rgb", 5, 6), ring, (how, "ring"))
        results.append((rcs, offs))
        b.close()
    assert results[0] == results[1] == results[2]
    torch.cuda.synchronize()


def test_repairs_rewrite_the_pictures_of_the_repaired_steps():
    """submit / wait with two steps in flight over the streams with which tests/test_parse_fallback.py makes a clip fall back to the host
    parser in the middle (three clips with a glitch in their first four frames, two that never leave the device parsers; every frame
    decodes): the glitch is found in wait and repaired there, with the step already in flight behind it, and the sink's pictures of those
    steps are written again.  The tensor equals the twin's for every clip."""
    import torch
    from mobiclipdecoder_amd import MobiclipBatch, default_params, generate_clip
    from mobiclipdecoder_amd.streamgen import BASE_SEED
    from tests.test_parse_fallback import _glitch_then_clean
    n_clean, nfr = 4, 8
    clips = [_glitch_then_clean(BASE_SEED + 7700 + i, n_clean) for i in range(3)]
    for i in range(2):
        y, fo = generate_clip(default_params("B", BASE_SEED + 7750 + i, n_frames=nfr, width=64, height=48, version=2, pm_intra=80))
        clips.append([y[fo[f]:fo[f + 1]] for f in range(nfr)])
    T, s, start = 4, 2, [0, 1, 0, 1, 0]
    twin = MobiclipBatch(N, 64, 48, 2, device_parse=False)
    pics = []
    for f in range(nfr):
        assert twin.decode([c[f] for c in clips], [0] * N)[0] == [0] * N
        pics.append(twin.export_tensor("rgb", 0, 1, boxes=BOXES, flip=FLIPS, size=SIZE)[0].clone())
    twin.close()
    b = MobiclipBatch(N, 64, 48, 2, device_parse=1)
    out = b.set_sink(size=SIZE, n_frames=T, stride=s, start=start, boxes=BOXES, flip=FLIPS)
    on_host = []
    b.submit([c[0] for c in clips], [0] * N)
    for f in range(1, nfr):
        b.submit([c[f] for c in clips], [0] * N)
        assert b.wait()[0] == [0] * N
        on_host.append(b.host_clips())
    assert b.wait()[0] == [0] * N
    assert max(on_host) == 3, on_host  # (the three clips were handed over: their frames were repaired in wait)
    assert b.sink_pending() == 0
    _same(out, _expected(torch.stack(pics), "ntchw", T, s, start, nfr), "repairs")
    b.close()


def test_replay_with_a_sink():
    case = _case()
    data = np.fromfile(os.path.join(GOLD, NAME + ".bin"), dtype=np.uint8)
    fo = case["frame_off"]
    pics, _ = _twin(7, True, "uint8", "unit")
    b = _batch()
    assert b.preload(0, data[:fo[7]], fo[:8]) == [0] * 7
    for c in range(1, N):
        b.preload_clone(c, 0)
    b.commit()
    out = b.set_sink(size=SIZE, n_frames=4, stride=2, boxes=BOXES, flip=FLIPS, layout="ncthw")
    for f in range(7):
        b.replay(f)
    assert b.sync() == 0
    assert b.sink_pending() == 0 and b.sink_launches() == 4
    _same(out, _expected(pics, "ncthw", 4, 2, [0] * N, 7), "replay")
    b.close()


def test_reset_in_the_middle():
    """reset_clips([2]) after step 3 of 8: the sink follows batch steps, so clip 2's later pictures are the new stream's and the others'
    are what they were"""
    T, s, start = 4, 2, [0, 1, 0, 1, 0]
    plain, _ = _twin(9, True, "uint8", "unit")
    pics, _ = _twin(8, True, "uint8", "unit", reset_at=(4, 2))
    b = _batch(device_parse=False)
    out = b.set_sink(size=SIZE, n_frames=T, stride=s, start=start, boxes=BOXES, flip=FLIPS)
    fr = _frames(8)
    for f in range(8):
        per = [fr[f]] * N
        if f == 4:
            b.reset_clips([2])
        if f >= 4:
            per[2] = fr[f - 4]
        assert b.decode([d for d, _ in per], [o for _, o in per])[0] == [0] * N
    assert b.sink_pending() == 0
    want = _expected(pics, "ntchw", T, s, start, 8)
    _same(out, want, "reset")
    old = _expected(plain, "ntchw", T, s, start, 8)
    keep = [0, 1, 3, 4]
    assert np.array_equal(out[keep].cpu().numpy(), old[keep].cpu().numpy()) and np.array_equal(out[2, :2].cpu().numpy(), old[2, :2].cpu().numpy())
    assert not np.array_equal(out[2, 2:].cpu().numpy(), old[2, 2:].cpu().numpy())
    b.close()


def test_refusals_change_nothing():
    import torch
    from mobiclipdecoder_amd import decoder
    from tests.test_sink import _spec
    lib = decoder.load_library()
    fr = _frames(4)
    b = _batch(device_parse=True)
    out = b.set_sink(size=SIZE, n_frames=3, stride=1)
    keep = out.clone()
    need = out.numel()
    fresh = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")

    def spec(dst, dst_bytes=None):
        return _spec(n=N, T=3, s=1, dst=dst, dst_bytes=dst_bytes)

    def refused(sp, what, pending=15):
        assert lib.mobi_batch_set_sink(b._h, C.byref(sp)) == MOBI_E_ARG, what
        assert b.sink_pending() == pending, what

    host = np.zeros(need + 64, np.uint8)
    refused(spec(host.ctypes.data + (-host.ctypes.data) % 16), "host memory")
    pinned = decoder.host_empty(need + 64)
    refused(spec(pinned.ctypes.data + (-pinned.ctypes.data) % 16), "mobi_host_alloc memory")
    refused(spec(fresh.data_ptr(), need - 1), "one picture short")
    assert lib.mobi_batch_set_sink(b._h, C.byref(spec(fresh.data_ptr()))) == 0 and b.sink_pending() == 15  # (the same spec with room: replaced)
    out = b.set_sink(size=SIZE, n_frames=3, stride=1, out=out)
    b.submit([fr[0][0]] * N, [fr[0][1]] * N)
    refused(spec(fresh.data_ptr()), "a step submitted", 10)  # (the step's five pictures are enqueued)
    assert lib.mobi_batch_set_sink(b._h, None) == MOBI_E_ARG and b.sink_pending() == 10
    assert b.wait()[0] == [0] * N and b.sink_pending() == 10
    b.gop_begin(*_gop_args(fr[1:3]))
    assert lib.mobi_batch_set_sink(b._h, C.byref(spec(fresh.data_ptr()))) == MOBI_E_ARG and b.sink_pending() == 10
    assert lib.mobi_batch_set_sink(b._h, None) == MOBI_E_ARG and b.sink_pending() == 10
    assert all(r == [0] * N for r in b.gop_finish_all()[0]) and b.sink_pending() == 0
    torch.cuda.synchronize()
    assert bool((fresh == 0).all())
    assert not torch.equal(out, keep)
    b.close()


def test_a_batch_that_never_arms_launches_nothing():
    case = _case()
    fr = _frames(10)
    b = _batch(device_parse=True)
    for d, o in fr[:2]:
        assert b.decode([d] * N, [o] * N)[0] == [0] * N
    b.submit([fr[2][0]] * N, [fr[2][1]] * N)
    b.submit([fr[3][0]] * N, [fr[3][1]] * N)
    assert b.wait()[0] == [0] * N and b.wait()[0] == [0] * N
    b.gop_begin(*_gop_args(fr[4:6]))
    assert all(r == [0] * N for r in b.gop_finish()[0])
    b.gop_begin(*_gop_args(fr[6:10]))
    assert all(r == [0] * N for r in b.gop_finish_all()[0])
    assert b.sink_launches() == 0 and b.sink_pending() == 0
    b.set_sink(None)
    b.close()
    data = np.fromfile(os.path.join(GOLD, NAME + ".bin"), dtype=np.uint8)
    r = _batch(device_parse=False)
    assert r.decode([fr[0][0]] * N, [fr[0][1]] * N)[0] == [0] * N
    r.close()
    r = _batch()
    assert r.preload(0, data[:case["frame_off"][3]], case["frame_off"][:4]) == [0] * 3
    for c in range(1, N):
        r.preload_clone(c, 0)
    r.commit()
    for f in range(3):
        r.replay(f)
    assert r.sync() == 0 and r.sink_launches() == 0
    r.close()


def _fnv(a):
    h = 1469598103934665603
    for v in np.ascontiguousarray(a).reshape(-1).tolist():
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_sink_and_finish_all_from_plain_c(tmp_path):
    from mobiclipdecoder_amd import build
    exe = str(tmp_path / "sink_caller")
    rocm_lib = os.path.join(build.ROCM, "lib")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", os.path.join(ROOT, "tests", "tools", "sink_caller.c"), "-L" + PKG, "-lmobiclip_hip", "-L" + rocm_lib,
                    "-lamdhip64", "-Wl,-rpath," + PKG, "-Wl,-rpath," + rocm_lib, "-o", exe], check=True)
    case = _case()
    T, s = 4, 2
    start = [c % 2 for c in range(N)]
    pics, _ = _twin(8, True, "uint8", "unit", boxes=[(0, 0, 64, 48)] * N, flips=[False] * N)
    want = _expected(pics, "ntchw", T, s, start, 8)
    args = [exe, os.path.join(GOLD, NAME + ".bin"), "64", "48", str(case["version"]), str(N), "8"] + [str(o) for o in case["frame_off"][:9]] + [str(T), str(s)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    words = r.stdout.split()
    assert words[0] == "fnv" and int(words[1]) == _fnv(want.cpu().numpy()), r.stdout
    assert words[2:] == ["pending", "0", "launches", "8"], r.stdout
