"""Export of decoded pictures to host memory (mobi_batch_export, include/mobiclip_hip.h; mobi_export.h / mobi_export.hip / mobi_export.cpp).

CPU: the pack kernel's addressing (csrc/mobi_export.h) compiled with g++ against numpy crops of tiled random planes; the header and the
binding; argument errors.  GPU (-m gpu): parity with get_planes / get_argb_at and the oracle, the snapshot rule, groups, asynchronous steps,
staging chunks used over and over, errors and lifetime."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mobiclipdecoder_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")
MAN = json.load(open(os.path.join(GOLD, "golden.json")))
MOBI_E_NULLREF, MOBI_E_ARG = -2, -7


def _stride(w):  # MD.cs:50-52
    s = 256
    while s < w:
        s *= 2
    return s


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
_PACK_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mobi_export.h"
// argv: width height stride in.bin out.bin.  in.bin = the reference's linear Y[stride*height] then UV[stride*height/2]; the slot is built
// with mobi_ty / mobi_tc (mobi_tile.h) and packed lane by lane with mobi_export_lane, as mobi_export_i420 does
int main(int argc, char **argv) {
  const uint32_t w = atoi(argv[1]), h = atoi(argv[2]), S = atoi(argv[3]);
  int lg = 0;
  while ((1u << lg) < S) lg++;
  const uint32_t ysz = S * h;
  std::vector<uint8_t> lin(ysz * 3 / 2), slot(ysz * 3 / 2, 0xEE), pic(mobi_export_i420_bytes(w, h), 0xEE);
  FILE *f = fopen(argv[4], "rb");
  if (fread(lin.data(), 1, lin.size(), f) != lin.size()) return 2;
  fclose(f);
  for (uint32_t a = 0; a < ysz; a++) slot[mobi_ty(a, lg)] = lin[a];
  for (uint32_t a = 0; a < ysz / 2; a++) slot[ysz + mobi_tc(a, lg)] = lin[ysz + a];
  const uint32_t mbw = w / 16;
  for (uint32_t L = 0; L < mobi_export_lanes(h, mbw); L++) {
    uint32_t src[2], dst[2];
    if (mobi_export_lane(L, w, h, mbw, lg, src, dst)) {
      for (int i = 0; i < 8; i++) { pic.at(dst[0] + i) = slot.at(src[0] + i); pic.at(dst[0] + 8 + i) = slot.at(src[1] + i); }
    } else {
      for (int i = 0; i < 8; i++) { pic.at(dst[0] + i) = slot.at(src[0] + i); pic.at(dst[1] + i) = slot.at(src[1] + i); }
    }
  }
  f = fopen(argv[5], "wb");
  fwrite(pic.data(), 1, pic.size(), f);
  fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def pack_tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("export_pack")
    src, exe = d / "pack.cpp", d / "pack"
    src.write_text(_PACK_CPP)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def _crop_i420(y, uv, w, h, S):
    return np.concatenate([y[:h, :w].ravel(), uv[:h // 2, :w // 2].ravel(), uv[:h // 2, S // 2:S // 2 + w // 2].ravel()])


@pytest.mark.parametrize("w,h", [(32, 32), (64, 48), (256, 192), (528, 48), (640, 480), (848, 480)])
def test_pack_addressing_equals_the_crop(pack_tool, tmp_path, w, h):
    """the addressing the kernel runs (mobi_export.h), on the CPU: tiled slot -> packed I420 == the numpy crop of the linear planes.
    256x192 is Stride == Width; 528, 848 have an odd number of macroblocks per row, 32 too (two)"""
    S = _stride(w)
    rng = np.random.default_rng(w * 1000 + h)
    y = rng.integers(0, 256, (h, S), dtype=np.uint8)
    uv = rng.integers(0, 256, (h // 2, S), dtype=np.uint8)
    (tmp_path / "in.bin").write_bytes(y.tobytes() + uv.tobytes())
    subprocess.run([pack_tool, str(w), str(h), str(S), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    assert got.size == w * h * 3 // 2
    assert np.array_equal(got, _crop_i420(y, uv, w, h, S))


def test_header_declares_the_export_and_the_binding_binds_it():
    from mobiclipdecoder_amd import decoder
    text = open(os.path.join(ROOT, "include", "mobiclip_hip.h")).read()
    for name in ("mobi_batch_export", "mobi_batch_export_wait", "mobi_batch_export_query", "mobi_host_alloc", "mobi_host_free"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in decoder._SIGS, name
    assert re.search(r"#define MOBI_EXPORT_I420 0\b", text) and re.search(r"#define MOBI_EXPORT_ARGB 1\b", text)
    assert decoder.EXPORT_FORMATS == {"i420": 0, "argb": 1}


def test_null_batch_is_refused():
    from mobiclipdecoder_amd import decoder
    lib = decoder.load_library()
    t = C.c_uint64(0)
    buf = np.zeros(64, np.uint8)
    assert lib.mobi_batch_export(None, 0, 0, 1, 0, 1, buf.ctypes.data, buf.nbytes, C.byref(t)) == MOBI_E_ARG
    assert lib.mobi_batch_export(None, 1, 0, 1, 0, 1, buf.ctypes.data, buf.nbytes, None) == MOBI_E_ARG
    assert lib.mobi_batch_export_wait(None, 1) == MOBI_E_ARG
    assert lib.mobi_batch_export_query(None, 1) == MOBI_E_ARG
    lib.mobi_host_free(None)  # (a no-op)


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"library called ({name}) for an argument the binding must refuse")


def _fake_batch(n=4, W=64, H=48):
    from mobiclipdecoder_amd import MobiclipBatch
    b = MobiclipBatch.__new__(MobiclipBatch)
    b._lib, b._h, b.n, b.Width, b.Height = _NoLib(), None, n, W, H
    return b


@pytest.mark.parametrize("kw", [
    dict(fmt="nv12"), dict(fmt=0), dict(ring_idx=6), dict(ring_idx=-1), dict(ring_idx=1.0), dict(ring_idx=True),
    dict(n_frames=0), dict(ring_idx=1, n_frames=3), dict(n_frames=2), dict(clips=range(0, 5)), dict(clips=range(2, 2)),
    dict(clips=range(0, 4, 2)), dict(clips=slice(0, 4, 2)), dict(clips=[0, 1]), dict(clips=range(-1, 2)),
    dict(out=np.zeros((1, 4, 64 * 48 * 3 // 2), np.uint16)), dict(out=np.zeros((1, 3, 64 * 48 * 3 // 2), np.uint8)),
    dict(fmt="argb", out=np.zeros((1, 4, 64 * 48), np.uint32)), dict(out=np.zeros((1, 4, 64 * 48 * 3), np.uint8)[:, :, ::2]),
    dict(out=[0] * 4608),
])
def test_export_argument_errors_raise_value_error_before_any_library_call(kw):
    b = _fake_batch()
    with pytest.raises(ValueError):
        b.export(**kw)


def test_split_i420_views():
    from mobiclipdecoder_amd import split_i420
    W, H = 32, 16
    a = np.arange(2 * 3 * W * H * 3 // 2, dtype=np.int64).astype(np.uint8).reshape(2, 3, -1)
    Y, U, V = split_i420(a, W, H)
    assert Y.shape == (2, 3, H, W) and U.shape == V.shape == (2, 3, H // 2, W // 2)
    assert np.shares_memory(Y, a) and np.shares_memory(V, a)
    assert np.array_equal(V[1, 2].ravel(), a[1, 2, W * H + W * H // 4:])
    with pytest.raises(ValueError):
        split_i420(a[..., :-1], W, H)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _golden(case):
    data = np.fromfile(os.path.join(GOLD, case["name"] + ".bin"), dtype=np.uint8)
    fo = case["frame_off"]
    return [(data[:fo[f + 1]], fo[f]) for f in range(len(case["frames"]))], [bool(fr.get("rejected")) for fr in case["frames"]]


def _generated(cfg, seed, n_frames, **kw):
    from mobiclipdecoder_amd import default_params, generate_clip
    from mobiclipdecoder_amd.streamgen import BASE_SEED
    p = default_params(cfg, BASE_SEED + seed, n_frames=n_frames, **kw)
    data, fo = generate_clip(p)
    return p, [(data[fo[f]:fo[f + 1]], 0) for f in range(n_frames)]


def _crop(b, clip, idx):
    y, uv = b.planes(clip, idx)
    return _crop_i420(y, uv, b.Width, b.Height, b.Stride)


def _check_ring(b, oras, rejected_at, frames_done, alloc):
    """every export shape the ring allows right now against get_planes / get_argb_at (and the oracle where it keeps the same picture)"""
    from mobiclipdecoder_amd import split_i420
    n, W, H = b.n, b.Width, b.Height
    top = min(5, frames_done - 1)
    want = {(c, r): _crop(b, c, r) for c in range(n) for r in range(top + 1)}
    bm = {(c, r): b.bitmap(c, r) for c in range(n) for r in range(top + 1)}
    for c in range(n):
        for r in range(top + 1):
            if not rejected_at(frames_done - 1 - r):
                o = oras[c]
                S = o.Stride
                assert np.array_equal(want[c, r], _crop_i420(o.y(r), o.uv(r), W, H, S)), (c, r, "get_planes vs oracle")
    for ring_idx in range(top + 1):
        for nf in range(1, ring_idx + 2):
            for clips in (range(n), range(1, n)) if n > 1 else (range(n),):
                shape = (nf, len(clips), W * H * 3 // 2)
                got = b.export("i420", ring_idx, nf, clips, out=alloc(shape, np.uint8))
                for j in range(nf):
                    for i, c in enumerate(clips):
                        assert np.array_equal(got[j, i], want[c, ring_idx - j]), ("i420", ring_idx, nf, clips, j, c)
                Y, U, V = split_i420(got, W, H)
                assert Y.shape == (nf, len(clips), H, W)
    for ring_idx in range(top + 1):
        nf = ring_idx + 1
        got = b.export("argb", ring_idx, nf, range(n), out=alloc((nf, n, H, W), np.uint32))
        for j in range(nf):
            for c in range(n):
                assert np.array_equal(got[j, c], bm[c, ring_idx - j]), ("argb", ring_idx, nf, j, c)
    for c in range(n):  # ring 0: the oracle's Bitmap
        if not rejected_at(frames_done - 1):
            assert np.array_equal(b.export("argb", 0, 1, range(c, c + 1), out=alloc((1, 1, H, W), np.uint32))[0, 0], oras[c].argb())


def _allocators():
    from mobiclipdecoder_amd import host_empty
    return {"host_empty": host_empty, "np_empty": lambda s, d: np.empty(s, d)}


@pytest.mark.gpu
@pytest.mark.parametrize("dest", ["host_empty", "np_empty"])
@pytest.mark.parametrize("case", MAN["cases"], ids=[c["name"] for c in MAN["cases"]])
def test_export_parity_golden(case, dest):
    from mobiclipdecoder_amd import MobiclipBatch
    from tests.oracle_binding import OracleDecoder
    frames, rejected = _golden(case)
    n = 3
    b = MobiclipBatch(n, case["width"], case["height"], case["version"])
    oras = [OracleDecoder(case["width"], case["height"], case["version"]) for _ in range(n)]
    alloc = _allocators()[dest]
    t = C.c_uint64(0)
    buf = np.zeros(16, np.uint8)
    assert b._lib.mobi_batch_export(b._h, 0, 0, 1, 0, 1, buf.ctypes.data, 1 << 30, C.byref(t)) == MOBI_E_NULLREF
    for f, (d, off) in enumerate(frames):
        rcs, _ = b.decode([d] * n, [off] * n)
        for o in oras:
            o.Data, o.Offset = d, off
            o.DecodeFrame()
        assert all((rc != 0) == rejected[f] for rc in rcs), (f, rcs)
        _check_ring(b, oras, lambda k: k >= 0 and rejected[k], f + 1, alloc)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["A", "B", "C"])
def test_export_parity_generated(cfg):
    """generated streams of the three configurations (640x480, 848x480: odd macroblocks per row), 4 different clips, through decode groups"""
    from mobiclipdecoder_amd import MobiclipBatch
    from tests.oracle_binding import OracleDecoder
    streams = [_generated(cfg, 300 + c, 8) for c in range(4)]
    p = streams[0][0]
    b = MobiclipBatch(4, p.width, p.height, p.version, device_parse=True)
    oras = [OracleDecoder(p.width, p.height, p.version) for _ in range(4)]
    for k0, K in ((0, 1), (1, 4), (5, 3)):
        rcs, _ = b.decode_gop([[streams[c][1][k][0] for c in range(4)] for k in range(k0, k0 + K)])
        assert all(r == [0] * 4 for r in rcs)
        for c, o in enumerate(oras):
            for k in range(k0, k0 + K):
                o.Data, o.Offset = streams[c][1][k]
                assert o.DecodeFrame() is not None
        _check_ring(b, oras, lambda k: False, k0 + K, _allocators()["host_empty"])
    b.close()


def _ring_copy(b, top):
    return {(c, r): _crop(b, c, r) for c in range(b.n) for r in range(top)}


@pytest.mark.gpu
def test_export_is_a_snapshot_decode():
    """six frames exported without waiting, then six more decoded at once (every exported slot written again): dst holds the old six"""
    from mobiclipdecoder_amd import MobiclipBatch
    p, fr = _generated("B", 11, 12)
    n = 8
    b = MobiclipBatch(n, p.width, p.height, p.version)
    for f in range(6):
        b.decode([fr[f][0]] * n, [0] * n)
    want = _ring_copy(b, 6)
    bm = {(c, r): b.bitmap(c, r) for c in range(n) for r in range(6)}
    hi = b.export("i420", 5, 6, wait=False)
    ha = b.export("argb", 5, 6, wait=False)
    for f in range(6, 12):
        b.decode([fr[f][0]] * n, [0] * n)
    got, gota = hi.wait(), ha.wait()
    assert hi.done() and ha.done()
    for j in range(6):
        for c in range(n):
            assert np.array_equal(got[j, c], want[c, 5 - j]), (j, c)
            assert np.array_equal(gota[j, c], bm[c, 5 - j]), (j, c)
    assert not np.array_equal(_crop(b, 0, 0), want[0, 0])  # (the ring did move on)
    b.close()


# The ring-slot guard.  An export larger than the staging pool (4 x 64 MiB) is packed chunk by chunk behind the copies, so its last frames
# are read out of the ring tens of milliseconds after the call returns; the steps below are enqueued at once and write every exported slot
# within a few milliseconds.  Only the guard (mobi_batch::guard_slot) makes them wait for the packs: without it the export would hold the
# new frames.
_GUARD_CLIPS, _GUARD_SRC = 1024, 8  # 1024 clips x 6 frames of 640x480 I420: 2.8 GB, eleven times the pool


def _check_old_six(got, streams, p, argb=False):
    from tests.oracle_binding import OracleDecoder
    n, m = got.shape[1], len(streams)
    assert got.shape[0] == 6
    for c in range(m):
        o = OracleDecoder(p.width, p.height, p.version)
        for f in range(6):
            o.Data, o.Offset = streams[c][f], 0
            assert o.DecodeFrame() is not None
            want = o.argb() if argb else _crop_i420(o.y(0), o.uv(0), p.width, p.height, o.Stride)
            assert np.array_equal(got[f, c], want), (c, f)
    for c in range(m, n):
        assert np.array_equal(got[:, c], got[:, c % m]), c


@pytest.mark.gpu
def test_slot_guard_holds_replayed_steps_behind_a_large_export():
    from mobiclipdecoder_amd import MobiclipBatch
    n, m = _GUARD_CLIPS, _GUARD_SRC
    gen = [_generated("B", 80 + c, 12) for c in range(m)]
    p = gen[0][0]
    b = MobiclipBatch(n, p.width, p.height, p.version)
    for c in range(m):
        data = np.concatenate([d for d, _ in gen[c][1]])
        fo = np.cumsum([0] + [d.size for d, _ in gen[c][1]])
        assert b.preload(c, data, fo) == [0] * 12
    for c in range(m, n):
        b.preload_clone(c, c % m)
    b.commit()
    for f in range(6):
        b.replay(f)
    assert b.sync() == 0
    h = b.export("i420", 5, 6, wait=False)
    for f in range(6, 12):  # six reconstruction steps enqueued in microseconds, each writing a slot the export reads
        b.replay(f)
    assert b.sync() == 0
    got = h.wait()
    _check_old_six(got, [[d for d, _ in g[1]] for g in gen], p)
    new = b.export("i420", 0, 1, range(0, 1), out=np.empty((1, 1, got.shape[2]), np.uint8))
    assert not np.array_equal(new[0, 0], got[5, 0])  # (the ring did move on)
    b.close()


@pytest.mark.gpu
def test_slot_guard_holds_a_gop_finish_part_behind_a_large_export():
    import time
    from mobiclipdecoder_amd import MobiclipBatch, host_empty
    n, m = _GUARD_CLIPS, _GUARD_SRC
    gen = [_generated("B", 90 + c, 12) for c in range(m)]
    p = gen[0][0]
    b = MobiclipBatch(n, p.width, p.height, p.version, device_parse=True)
    b.gop_begin([[gen[c % m][1][k][0] for c in range(n)] for k in range(6)])
    rcs, _ = b.gop_finish()
    assert all(r == [0] * n for r in rcs)
    out = host_empty((6, n, p.height, p.width), np.uint32)  # ARGB: 7.5 GB, packed over ~140 ms of copies
    b.gop_begin([[gen[c % m][1][k][0] for c in range(n)] for k in range(6, 12)])
    time.sleep(1.0)  # (the group's parse is done: gop_finish below enqueues its six steps at once)
    h = b.export("argb", 5, 6, out=out, wait=False)
    rcs, _ = b.gop_finish()
    assert all(r == [0] * n for r in rcs)
    _check_old_six(h.wait(), [[d for d, _ in g[1]] for g in gen], p, argb=True)
    b.close()


@pytest.mark.gpu
def test_export_is_a_snapshot_gop_finish():
    """the same with a 6-frame part of a group (mobi_batch_gop_begin / gop_finish) behind the export"""
    from mobiclipdecoder_amd import MobiclipBatch
    p, fr = _generated("B", 12, 12)
    n = 8
    b = MobiclipBatch(n, p.width, p.height, p.version, device_parse=True)
    b.gop_begin([[fr[k][0]] * n for k in range(6)])
    rcs, _ = b.gop_finish()
    assert all(r == [0] * n for r in rcs)
    want = _ring_copy(b, 6)
    h = b.export("i420", 5, 6, wait=False)
    b.gop_begin([[fr[k][0]] * n for k in range(6, 12)])
    rcs, _ = b.gop_finish()
    assert all(r == [0] * n for r in rcs)
    got = h.wait()
    for j in range(6):
        for c in range(n):
            assert np.array_equal(got[j, c], want[c, 5 - j]), (j, c)
    b.close()


@pytest.mark.gpu
def test_export_groups_every_part_without_waiting():
    """12-frame groups with the next group begun; every part gop_finish reports goes out as ONE export (P - 1, P) and is not waited for
    until the end: every frame of every clip equals the oracle"""
    from mobiclipdecoder_amd import MobiclipBatch
    from tests.oracle_binding import OracleDecoder
    n, G, NG = 6, 12, 3
    streams = [_generated("B", 40 + c, G * NG, iframe_interval=12) for c in range(3)]
    p = streams[0][0]
    b = MobiclipBatch(n, p.width, p.height, p.version, device_parse=True)
    group = lambda g: [[streams[c % 3][1][k][0] for c in range(n)] for k in range(g * G, (g + 1) * G)]
    handles = []  # (first frame, handle)
    b.gop_begin(group(0))
    done = 0
    for g in range(NG):
        if g + 1 < NG:
            b.gop_begin(group(g + 1))
        while True:
            rcs, _ = b.gop_finish()
            P = len(rcs)
            assert all(r == [0] * n for r in rcs)
            handles.append((done, b.export("i420", P - 1, P, wait=False)))
            done += P
            if done % G == 0:
                break
    assert done == G * NG
    W, H = p.width, p.height
    oras = [OracleDecoder(W, H, p.version) for _ in range(3)]
    want = [[None] * (G * NG) for _ in range(3)]
    for c, o in enumerate(oras):
        for k in range(G * NG):
            o.Data, o.Offset = streams[c][1][k]
            assert o.DecodeFrame() is not None
            want[c][k] = _crop_i420(o.y(0), o.uv(0), W, H, o.Stride)
    for f0, h in reversed(handles):  # (the last ticket first: it covers all before it)
        got = h.wait()
        for j in range(got.shape[0]):
            for c in range(n):
                assert np.array_equal(got[j, c], want[c % 3][f0 + j]), (f0 + j, c)
    b.close()


@pytest.mark.gpu
def test_export_with_steps_in_flight():
    """submit / wait with two steps in flight: ring indices below mobi_batch_in_flight are refused; those at or above it equal what
    get_planes shows after the last wait"""
    from mobiclipdecoder_amd import MobiclipBatch, MobiclipError, host_empty
    p, fr = _generated("B", 13, 6)
    n = 4
    b = MobiclipBatch(n, p.width, p.height, p.version, device_parse=True)
    b.submit([fr[0][0]] * n, [0] * n)
    b.wait()
    b.submit([fr[1][0]] * n, [0] * n)
    b.wait()
    b.submit([fr[2][0]] * n, [0] * n)
    b.submit([fr[3][0]] * n, [0] * n)
    assert b._lib.mobi_batch_in_flight(b._h) == 2
    dst = host_empty((4, n, p.width * p.height * 3 // 2), np.uint8)
    t = C.c_uint64(0)
    for ring_idx, nf in ((0, 1), (1, 1), (1, 2), (2, 2), (3, 3)):
        t.value = 0
        assert b._lib.mobi_batch_export(b._h, 0, ring_idx, nf, 0, n, dst.ctypes.data, dst.nbytes, C.byref(t)) == MOBI_E_ARG, (ring_idx, nf)
        assert t.value == 0  # (no ticket)
        with pytest.raises(MobiclipError):
            b.export("i420", ring_idx, nf)
    h = b.export("i420", 3, 2, wait=False)      # frames 0, 1: ring 3, 2
    ha = b.export("argb", 2, 1, wait=False)
    b.wait()
    assert b._lib.mobi_batch_in_flight(b._h) == 1
    h1 = b.export("i420", 2, 2, wait=False)     # frames 1, 2: ring 2, 1
    b.wait()
    got, gota, got1 = h.wait(), ha.wait(), h1.wait()
    for c in range(n):
        assert np.array_equal(got[0, c], _crop(b, c, 3)) and np.array_equal(got[1, c], _crop(b, c, 2))
        assert np.array_equal(got1[0, c], _crop(b, c, 2)) and np.array_equal(got1[1, c], _crop(b, c, 1))
        assert np.array_equal(gota[0, c], b.bitmap(c, 2))
    b.close()


@pytest.mark.gpu
def test_export_recycles_the_staging_chunks():
    """one export over four times the staging pool (800 clips x 640x480 x 3 frames, 1.1 GB against 4 x 64 MiB): every clip equals its source
    clip (8 streams, cloned), and the sources equal the oracle -- into pinned memory and into ordinary memory"""
    from mobiclipdecoder_amd import MobiclipBatch, host_empty
    from tests.oracle_binding import OracleDecoder
    n, m, F = 800, 8, 3
    streams = [_generated("B", 60 + c, F) for c in range(m)]
    p = streams[0][0]
    W, H = p.width, p.height
    b = MobiclipBatch(n, W, H, p.version)
    for f in range(F):
        rcs, _ = b.decode([streams[c % m][1][f][0] for c in range(n)], [0] * n)
        assert rcs == [0] * n
    pic = W * H * 3 // 2
    assert F * n * pic >= 4 * (4 * 64 << 20)
    oras = []
    for c in range(m):
        o = OracleDecoder(W, H, p.version)
        for f in range(F):
            o.Data, o.Offset = streams[c][1][f]
            assert o.DecodeFrame() is not None
        oras.append(o)
    for out in (host_empty((F, n, pic), np.uint8), np.empty((F, n, pic), np.uint8)):
        out[:] = 0xAB
        got = b.export("i420", F - 1, F, out=out)
        for c in range(m, n):
            assert np.array_equal(got[:, c], got[:, c % m]), c
        for c, o in enumerate(oras):
            for j in range(F):
                assert np.array_equal(got[j, c], _crop_i420(o.y(F - 1 - j), o.uv(F - 1 - j), W, H, o.Stride)), (c, j)
        del got
    b.close()


@pytest.mark.gpu
def test_export_refusals_and_tickets():
    from mobiclipdecoder_amd import MobiclipBatch, host_empty
    p, fr = _generated("A", 14, 3)
    n = 3
    b = MobiclipBatch(n, p.width, p.height, p.version)
    lib, h = b._lib, b._h
    pic = p.width * p.height * 3 // 2
    dst = host_empty((6 * n, pic * 4), np.uint8)
    big = dst.nbytes
    t = C.c_uint64(0)
    ex = lambda fmt, r, nf, c0, nc, nbytes=big, d=dst.ctypes.data: lib.mobi_batch_export(h, fmt, r, nf, c0, nc, d, nbytes, C.byref(t))
    assert ex(0, 0, 1, 0, n) == MOBI_E_NULLREF
    assert lib.mobi_batch_export_wait(h, 1) == MOBI_E_ARG  # (no export yet)
    b.decode([fr[0][0]] * n, [0] * n)
    b.decode([fr[1][0]] * n, [0] * n)
    assert ex(0, 2, 1, 0, n) == MOBI_E_NULLREF            # ring index 2: two frames so far
    assert ex(0, 2, 3, 0, n) == MOBI_E_NULLREF
    for args in ((2, 0, 1, 0, n), (-1, 0, 1, 0, n), (0, 6, 1, 0, n), (0, -1, 1, 0, n), (0, 0, 2, 0, n), (0, 1, 0, 0, n), (0, 0, 1, -1, 1),
                 (0, 0, 1, 0, n + 1), (0, 0, 1, n, 1), (0, 0, 1, 1, n), (0, 0, 1, 0, 0)):
        assert ex(*args) == MOBI_E_ARG, args
    assert ex(0, 1, 2, 0, n, nbytes=2 * n * pic - 1) == MOBI_E_ARG     # dst too small
    assert ex(1, 0, 1, 0, n, nbytes=n * p.width * p.height * 4 - 1) == MOBI_E_ARG
    assert ex(0, 0, 1, 0, n, d=None) == MOBI_E_ARG
    t.value = 0
    assert ex(0, 1, 2, 0, n, nbytes=2 * n * pic) == 0 and t.value >= 1
    assert lib.mobi_batch_export_wait(h, t.value + 1) == MOBI_E_ARG   # a ticket never issued
    assert lib.mobi_batch_export_query(h, t.value + 100) == MOBI_E_ARG
    assert lib.mobi_batch_export_wait(h, 0) == MOBI_E_ARG
    assert lib.mobi_batch_export_wait(h, t.value) == 0 and lib.mobi_batch_export_query(h, t.value) == 1
    first = t.value
    assert ex(0, 0, 1, 0, n) == 0 and t.value == first + 1         # a refused export issued no ticket
    assert lib.mobi_batch_export_wait(h, first) == 0               # (an old ticket: done)
    # the batch goes on after all of it, and the getters are untouched
    b.decode([fr[2][0]] * n, [0] * n)
    assert np.array_equal(b.export("i420", 0, 1, range(1, 2))[0, 0], _crop(b, 1, 0))
    b.close()


@pytest.mark.gpu
def test_destroy_with_an_export_outstanding_is_clean(tmp_path):
    """a process that destroys its batch with exports in flight (and one it never waits for) exits 0, the data in place"""
    script = tmp_path / "destroy.py"
    script.write_text(textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        import numpy as np
        from mobiclipdecoder_amd import MobiclipBatch, default_params, generate_clip, host_empty
        from mobiclipdecoder_amd.streamgen import BASE_SEED
        p = default_params("B", BASE_SEED + 15, n_frames=3)
        data, fo = generate_clip(p)
        n = 256
        b = MobiclipBatch(n, p.width, p.height, p.version)
        for f in range(3):
            b.decode([data[fo[f]:fo[f + 1]]] * n, [0] * n)
        want = b.export("i420", 0, 1, range(0, 1))[0, 0].copy()
        hs = [b.export("i420", 2, 3, wait=False) for _ in range(3)]
        loose = host_empty((3, n, p.width * p.height * 3 // 2), np.uint8)
        b.export("i420", 2, 3, out=loose, wait=False)
        b.close()  # waits for all four
        assert np.array_equal(hs[0].out[2, 0], want) and np.array_equal(loose[2, 0], want)
        assert all(h.done() for h in hs)
        print("ok")
    """))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr[-2000:])
