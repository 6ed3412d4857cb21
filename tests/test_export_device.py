"""Export of decoded pictures into device memory on the caller's stream (mobi_batch_export_device, include/mobiclip_hip.h;
mobi_export_rgb.h / mobi_export_rgb.hip / mobi_export.cpp; MobiclipBatch.export_tensor).

CPU: the header, the binding and the exported symbol; the RGB kernel's addressing (csrc/mobi_export_rgb.h) compiled with g++ and walked for
every layout and element size; argument errors.  GPU (-m gpu): parity of every format, layout and dtype with the host export and the Bitmap,
stream order without a host sync, the snapshot rule and the ring-slot guard with readers on several streams, group parts, refusals, and no
staging for a batch that only exports to device memory."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mobiclipdecoder_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")
MAN = json.load(open(os.path.join(GOLD, "golden.json")))
MOBI_E_NULLREF, MOBI_E_ARG = -2, -7
I420, ARGB, PLANAR, PACKED = 0, 1, 2, 3
U8, F16, F32 = 0, 1, 2


def _stride(w):  # MD.cs:50-52
    s = 256
    while s < w:
        s *= 2
    return s


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_device_export_and_the_library_exports_it():
    from mobiclipdecoder_amd import build, decoder
    text = open(os.path.join(ROOT, "include", "mobiclip_hip.h")).read()
    assert re.search(r"\bint mobi_batch_export_device\s*\(", text)
    for name, v in (("MOBI_EXPORT_RGB_PLANAR", 2), ("MOBI_EXPORT_RGB_PACKED", 3), ("MOBI_DTYPE_U8", 0), ("MOBI_DTYPE_F16", 1), ("MOBI_DTYPE_F32", 2)):
        assert re.search(r"#define %s %d\b" % (name, v), text), name
    assert "mobi_batch_export_device" in decoder._SIGS
    assert decoder.DEVICE_EXPORT_FORMATS == {("i420", None): 0, ("argb", None): 1, ("rgb", "nchw"): 2, ("rgb", "nhwc"): 3}
    assert decoder.DEVICE_EXPORT_DTYPES == {"uint8": 0, "float16": 1, "float32": 2}
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], capture_output=True, text=True, check=True).stdout
    assert "mobi_batch_export_device" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert hasattr(decoder.load_library(), "mobi_batch_export_device")


def test_null_batch_is_refused():
    from mobiclipdecoder_amd import decoder
    lib = decoder.load_library()
    buf = np.zeros(64, np.uint8)
    for fmt, dt in ((I420, U8), (ARGB, U8), (PLANAR, U8), (PACKED, F32)):
        assert lib.mobi_batch_export_device(None, fmt, dt, None, 0, 1, 0, 1, buf.ctypes.data, buf.nbytes, None) == MOBI_E_ARG


_ADDR_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mobi_export_rgb.h"
// argv: width height stride.  Walks every lane of every unit of one picture for both layouts and the three element sizes, as
// mobi_export_rgb does, and checks the reads against mobi_ty / mobi_tc (mobi_tile.h) and the writes against the layout.
static int fail(const char *what, unsigned a, unsigned b, unsigned c) { printf("FAIL %s %u %u %u\n", what, a, b, c); return 1; }
int main(int argc, char **argv) {
  const uint32_t w = atoi(argv[1]), h = atoi(argv[2]), S = atoi(argv[3]), mbw = w / 16, mbh = h / 16;
  int lg = 0;
  while ((1u << lg) < S) lg++;
  auto ytile_ok = [&](uint32_t off) { const uint32_t t = off >> 8; return (t & ((S >> 4) - 1)) < mbw && (t >> (lg - 4)) < mbh; };
  auto ctile_ok = [&](uint32_t off) { const uint32_t t = off >> 7; return (off & 15u) == 0 && (t & ((S >> 4) - 1)) < mbw && (t >> (lg - 4)) < mbh; };
  const uint32_t units = mobi_rgb_units(w, h);
  if (units * 256u != w * h) return fail("units", units, w, h);
  for (int planar = 0; planar < 2; planar++)
    for (uint32_t e = 1; e <= 4; e *= 2) {
      std::vector<int> count(3 * w * h, 0);
      if (mobi_rgb_picture_bytes(w, h, e) != 3 * w * h * e) return fail("picture bytes", w, h, e);
      for (uint32_t u = 0; u < units; u++)
        for (uint32_t l = 0; l < 64; l++) {
          MobiRgbSrc s;
          mobi_rgb_lane(u, l, w, h, lg, &s);
          const uint32_t x = s.x, y = s.y, cx = x / 2, cy = y / 2;
          if (x % 4 || x >= w || y >= h || y * w + x != u * 256 + l * 4) return fail("pixel", u, l, x);
          if ((uint32_t)s.odd != (y & 1) || (bool)s.lastcol != (x + 4 == w) || (bool)s.lastrow != ((y | 1) == h - 1)) return fail("flags", u, l, y);
          for (uint32_t t = 0; t < 4; t++)
            if (mobi_ty(y * S + x + t, lg) != s.luma + t) return fail("luma", u, l, t);
          if (!ytile_ok(s.luma)) return fail("luma tile", u, l, s.luma);
          if (!ctile_ok(s.c0) || !ctile_ok(s.c1) || !ctile_ok(s.n0) || !ctile_ok(s.n1)) return fail("chroma tile", u, l, s.c0);
          const uint32_t half = S / 2;
          // a, b under the pixels; V 8 bytes further
          for (uint32_t k = 0; k < 2; k++) {
            if (mobi_tc(cy * S + cx + k, lg) != s.c0 + s.sel + k) return fail("chroma a/b", u, l, k);
            if (mobi_tc(cy * S + half + cx + k, lg) != s.c0 + 8 + s.sel + k) return fail("chroma V", u, l, k);
          }
          // e, the sample right of b (not in the last column)
          if (!s.lastcol) {
            const uint32_t want = mobi_tc(cy * S + cx + 2, lg);
            if (s.sel < 6 ? want != s.c0 + s.sel + 2 : (!s.next || want != s.n0)) return fail("chroma e", u, l, s.sel);
          } else if (s.next) return fail("next in the last column", u, l, 0);
          // the row below (odd rows, not the last)
          if (s.odd && !s.lastrow) {
            if (!s.below || mobi_tc((cy + 1) * S + cx, lg) != s.c1 + s.sel) return fail("chroma below", u, l, y);
            if (!s.lastcol && (s.sel < 6 ? mobi_tc((cy + 1) * S + cx + 2, lg) != s.c1 + s.sel + 2 : mobi_tc((cy + 1) * S + cx + 2, lg) != s.n1))
              return fail("chroma below e", u, l, y);
          } else if (s.below || s.c1 != s.c0) return fail("below read", u, l, y);
          for (uint32_t t = 0; t < 4; t++)
            for (uint32_t ch = 0; ch < 3; ch++) {
              const uint32_t r = mobi_rgb_stage_off(planar, e, l, t, ch);
              if (r % e || r + e > mobi_rgb_chunks(e) * 16) return fail("stage", l, t, ch);
              const uint32_t d = mobi_rgb_chunk_dst(planar, e, w, h, u, r / 16) + r % 16;
              const uint32_t want = planar ? ((ch * h + y) * w + x + t) * e : ((y * w + x + t) * 3 + ch) * e;
              if (d != want) return fail("dst", d, want, ch);
              count[d / e]++;
            }
        }
      for (size_t i = 0; i < count.size(); i++)
        if (count[i] != 1) return fail("written", (unsigned)i, count[i], e);
      // one store instruction of a wave = 64 consecutive chunks (the last one fewer): its runs of contiguous bytes
      for (uint32_t u : {0u, units - 1})
        for (uint32_t k0 = 0; k0 < mobi_rgb_chunks(e); k0 += 64) {
          uint32_t run = 16;
          for (uint32_t k = k0 + 1; k <= k0 + 64 && k <= mobi_rgb_chunks(e); k++) {
            const bool end = k == k0 + 64 || k == mobi_rgb_chunks(e);
            if (!end && mobi_rgb_chunk_dst(planar, e, w, h, u, k) == mobi_rgb_chunk_dst(planar, e, w, h, u, k - 1) + 16) { run += 16; continue; }
            if (run < 256) return fail("store run", u, k, run);
            run = 16;
          }
        }
    }
  printf("ok\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def addr_tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("export_rgb_addr")
    src, exe = d / "addr.cpp", d / "addr"
    src.write_text(_ADDR_CPP)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("w,h", [(32, 32), (64, 48), (256, 192), (528, 48), (640, 480), (848, 480)])
def test_rgb_addressing_covers_every_element_once_and_reads_inside_the_picture(addr_tool, w, h):
    """the addressing the kernel runs (mobi_export_rgb.h), on the CPU, for planar / packed x 1, 2, 4 bytes: every element of the picture written
    exactly once at the place its (x, y, channel) has in the layout; every store instruction's runs at least 256 contiguous bytes; luma and
    chroma reads are the samples mobi_tile.h puts there, inside the picture's tiles.  256x192 is Stride == Width; 528, 848 have an odd number of macroblocks per row, 32 two"""
    r = subprocess.run([addr_tool, str(w), str(h), str(_stride(w))], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"library called ({name}) for an argument the binding must refuse")


def _fake_batch(n=4, W=64, H=48):
    from mobiclipdecoder_amd import MobiclipBatch
    b = MobiclipBatch.__new__(MobiclipBatch)
    b._lib, b._h, b.n, b.Width, b.Height, b.device = _NoLib(), None, n, W, H, 0
    return b


def _bad_kwargs():
    import torch
    cpu = torch.zeros((1, 4, 3, 48, 64), dtype=torch.uint8)
    return [
        dict(fmt="nv12"), dict(fmt=2), dict(layout="chw"), dict(layout=None), dict(dtype=torch.bfloat16), dict(dtype=np.uint8),
        dict(dtype=torch.int32), dict(fmt="i420", dtype=torch.float16), dict(fmt="argb", dtype=torch.float32),
        dict(scale=(1, 1, 1)), dict(bias=(0, 0, 0)), dict(fmt="i420", scale=(1, 1, 1)), dict(dtype=torch.float32, scale=(1, 1)),
        dict(dtype=torch.float32, bias=(0, 0, 0, 0)), dict(dtype=torch.float32, scale=(1, float("nan"), 1)), dict(dtype=torch.float32, scale="abc"),
        dict(dtype=torch.float32, bias=(0, float("inf"), 0)),
        dict(ring_idx=6), dict(ring_idx=-1), dict(ring_idx=1.0), dict(ring_idx=True), dict(n_frames=0), dict(ring_idx=1, n_frames=3),
        dict(n_frames=2), dict(clips=range(0, 5)), dict(clips=range(2, 2)), dict(clips=range(0, 4, 2)), dict(clips=slice(0, 4, 2)),
        dict(clips=[0, 1]), dict(clips=range(-1, 2)),
        dict(out=cpu), dict(out=np.zeros((1, 4, 3, 48, 64), np.uint8)), dict(stream="default"), dict(stream=0),
    ]


@pytest.mark.parametrize("k", range(34))
def test_export_tensor_argument_errors_raise_value_error_before_any_library_call(k):
    kws = _bad_kwargs()
    assert len(kws) == 34
    b = _fake_batch()
    with pytest.raises(ValueError):
        b.export_tensor(**kws[k])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
IMAGENET_MEAN = np.array([0.485, 0.456, 0.406]) * 255.0
IMAGENET_STD = np.array([0.229, 0.224, 0.225]) * 255.0
AFFINES = {"unit": None, "imagenet": ((1.0 / IMAGENET_STD).astype(np.float32), (-IMAGENET_MEAN / IMAGENET_STD).astype(np.float32))}


def _golden(case):
    data = np.fromfile(os.path.join(GOLD, case["name"] + ".bin"), dtype=np.uint8)
    fo = case["frame_off"]
    return [(data[:fo[f + 1]], fo[f]) for f in range(len(case["frames"]))]


def _generated(cfg, seed, n_frames, **kw):
    from mobiclipdecoder_amd import default_params, generate_clip
    from mobiclipdecoder_amd.streamgen import BASE_SEED
    p = default_params(cfg, BASE_SEED + seed, n_frames=n_frames, **kw)
    data, fo = generate_clip(p)
    return p, [(data[fo[f]:fo[f + 1]], 0) for f in range(n_frames)]


def _rgb_from_argb(bm, layout):
    """(F, N, H, W) uint32 Bitmaps -> uint8 R, G, B in the layout"""
    ch = [((bm >> s) & 0xFF).astype(np.uint8) for s in (16, 8, 0)]
    return np.stack(ch, axis=2) if layout == "nchw" else np.stack(ch, axis=-1)


def _affine(v8, layout, sb, np_dtype):
    """numpy's float32 v * s + b (two roundings), then np_dtype"""
    s, b = (np.ones(3, np.float32), np.zeros(3, np.float32)) if sb is None else sb
    shape = (3, 1, 1) if layout == "nchw" else (3,)
    f = v8.astype(np.float32) * s.reshape(shape) + b.reshape(shape)
    assert f.dtype == np.float32
    return f.astype(np_dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _check_all(b, ring_idx, nf, clips, stream=None):
    """every format x layout x dtype of one export shape against the host export (mobi_batch_export) and numpy"""
    import torch
    h420 = b.export("i420", ring_idx, nf, clips)
    harg = b.export("argb", ring_idx, nf, clips)
    d = b.export_tensor("i420", ring_idx, nf, clips, stream=stream)
    assert d.dtype == torch.uint8 and tuple(d.shape) == h420.shape
    assert np.array_equal(d.cpu().numpy(), h420), ("i420", ring_idx, nf, clips)
    d = b.export_tensor("argb", ring_idx, nf, clips, stream=stream)
    assert d.dtype == torch.int32 and tuple(d.shape) == harg.shape
    assert np.array_equal(d.cpu().numpy().view(np.uint32), harg), ("argb", ring_idx, nf, clips)
    for layout in ("nchw", "nhwc"):
        v8 = _rgb_from_argb(harg, layout)
        d = b.export_tensor("rgb", ring_idx, nf, clips, layout=layout, stream=stream)
        assert d.dtype == torch.uint8 and tuple(d.shape) == v8.shape
        assert np.array_equal(d.cpu().numpy(), v8), ("rgb u8", layout, ring_idx, nf, clips)
        for name, sb in AFFINES.items():
            kw = {} if sb is None else dict(scale=sb[0].tolist(), bias=sb[1].tolist())
            for tdt, ndt in ((torch.float32, np.float32), (torch.float16, np.float16)):
                d = b.export_tensor("rgb", ring_idx, nf, clips, layout=layout, dtype=tdt, stream=stream, **kw)
                want = _affine(v8, layout, sb, ndt)
                assert d.dtype == tdt and tuple(d.shape) == want.shape
                assert np.array_equal(_bits(d.cpu().numpy()), _bits(want)), ("rgb", layout, name, ndt, ring_idx, nf, clips)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MAN["cases"], ids=[c["name"] for c in MAN["cases"]])
def test_device_export_parity_golden(case):
    import torch  # noqa: F401  (before the library: one HIP runtime)
    from mobiclipdecoder_amd import MobiclipBatch
    frames = _golden(case)
    n = 3
    b = MobiclipBatch(n, case["width"], case["height"], case["version"])
    for f, (d, off) in enumerate(frames):
        b.decode([d] * n, [off] * n)
        top = min(5, f)
        _check_all(b, top, top + 1, range(n))
        if n > 1:
            _check_all(b, 0, 1, range(1, n))
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["A", "B", "C"])
def test_device_export_parity_generated(cfg):
    """generated streams of the three configurations (640x480 ModsDS / Moflex, 848x480: odd macroblocks per row), 5 different clips, six frames
    at once, clip0 > 0, on the current stream and on a side stream"""
    import torch
    from mobiclipdecoder_amd import MobiclipBatch
    streams = [_generated(cfg, 500 + c, 7) for c in range(5)]
    p = streams[0][0]
    b = MobiclipBatch(5, p.width, p.height, p.version)
    for f in range(7):
        rcs, _ = b.decode([streams[c][1][f][0] for c in range(5)], [0] * 5)
        assert rcs == [0] * 5
    _check_all(b, 5, 6, range(5))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # (the reads of the tensors -- .cpu() -- go on the export's stream, behind it)
        _check_all(b, 5, 6, range(2, 5), stream=side)
    _check_all(b, 3, 2, range(1, 4))
    b.close()


@pytest.mark.gpu
def test_device_export_is_ordered_on_the_stream_without_a_host_sync():
    """a torch reduction enqueued on the export's stream right behind it -- the current stream, and a side stream held busy first -- sees the
    pictures"""
    import torch
    from mobiclipdecoder_amd import MobiclipBatch
    p, fr = _generated("B", 21, 3)
    n = 64
    b = MobiclipBatch(n, p.width, p.height, p.version)
    for f in range(3):
        b.decode([fr[f][0]] * n, [0] * n)
    want8 = _rgb_from_argb(b.export("argb", 2, 3), "nchw")
    want = int(want8.astype(np.int64).sum())
    wantc = want8.astype(np.int64).sum(axis=(0, 1, 3, 4))
    dev = torch.device("cuda", b.device)
    out = torch.zeros(want8.shape, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    b.export_tensor("rgb", 2, 3, out=out)
    total = out.sum(dtype=torch.int64)  # (same stream, no sync in between)
    assert int(total) == want
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        a = torch.randn(4096, 4096, device=dev)
        for _ in range(10):
            a = a @ a / 64.0
        outf = b.export_tensor("rgb", 2, 3, dtype=torch.float32, stream=side)
        sums = outf.double().sum(dim=(0, 1, 3, 4))
    side.synchronize()
    assert np.array_equal(sums.cpu().numpy().astype(np.int64), wantc)
    b.close()


# The ring-slot guard with readers on streams the library does not own.  A side stream is held busy for a few hundred milliseconds, the
# export goes behind that work, and six reconstruction steps that write every exported slot are enqueued at once.  Only the guard makes
# the steps wait for the export's kernel: without it the tensor would hold the new frames.
_GUARD_CLIPS, _GUARD_SRC = 1024, 8


def _busy(stream, dev, ms_hint=300):
    """enqueue ~ms_hint of dense matrix products on stream (nothing waits for them here)"""
    import torch
    with torch.cuda.stream(stream):
        a = torch.randn(8192, 8192, device=dev)
        for _ in range(max(1, ms_hint // 8)):
            a = torch.mm(a, a)
            a.mul_(1e-4)
    return a


def _guard_batch(seed):
    from mobiclipdecoder_amd import MobiclipBatch
    n, m = _GUARD_CLIPS, _GUARD_SRC
    gen = [_generated("B", seed + c, 12) for c in range(m)]
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
    return b, p, [[d for d, _ in g[1]] for g in gen]


def _old_six(streams, p):
    """the oracle's Bitmaps of frames 0..5 of every source stream: [c][f] -> (H, W) uint32"""
    from tests.oracle_binding import OracleDecoder
    out = []
    for s in streams:
        o = OracleDecoder(p.width, p.height, p.version)
        fr = []
        for f in range(6):
            o.Data, o.Offset = s[f], 0
            assert o.DecodeFrame() is not None
            fr.append(o.argb())
        out.append(fr)
    return out


def _check_old_six_rgb(got, old, layout):
    """got: (6, n, ...) uint8 RGB of clips 0..n-1; clip c holds source c % m"""
    m = len(old)
    assert got.shape[0] == 6
    for c in range(got.shape[1]):
        for f in range(6):
            want = _rgb_from_argb(old[c % m][f][None, None], layout)[0, 0]
            assert np.array_equal(got[f, c], want), (c, f)


@pytest.mark.gpu
def test_slot_guard_holds_replayed_steps_behind_a_device_export_on_a_busy_stream():
    import torch
    b, p, streams = _guard_batch(700)
    dev = torch.device("cuda", b.device)
    side = torch.cuda.Stream(device=dev)
    keep = _busy(side, dev)
    out = b.export_tensor("rgb", 5, 6, range(0, 16), layout="nhwc", stream=side)
    for f in range(6, 12):  # six steps enqueued at once, each writing a slot the export has not read yet
        b.replay(f)
    assert b.sync() == 0
    torch.cuda.synchronize()
    _check_old_six_rgb(out.cpu().numpy(), _old_six(streams, p), "nhwc")
    new = b.export_tensor("rgb", 0, 1, range(0, 1), layout="nhwc")
    assert not np.array_equal(new.cpu().numpy()[0, 0], out.cpu().numpy()[5, 0])  # (the ring did move on)
    del keep
    b.close()


@pytest.mark.gpu
def test_slot_guard_holds_steps_behind_a_device_export_and_a_host_export_at_once():
    """a device export on a busy side stream, then a large host export of the same slots (its pack is the slots' newest reader), then six
    steps that write every slot: both hold the old frames.  With one event per slot (the last reader) the steps would wait for the host
    export's pack only and overwrite the slots before the side stream reaches the device export."""
    import torch
    from mobiclipdecoder_amd import host_empty
    b, p, streams = _guard_batch(720)
    dev = torch.device("cuda", b.device)
    side = torch.cuda.Stream(device=dev)
    keep = _busy(side, dev)
    out = b.export_tensor("rgb", 5, 6, range(0, 16), layout="nchw", stream=side)
    h = b.export("i420", 5, 6, out=host_empty((6, b.n, p.width * p.height * 3 // 2), np.uint8), wait=False)
    for f in range(6, 12):
        b.replay(f)
    assert b.sync() == 0
    torch.cuda.synchronize()
    got = h.wait()
    old = _old_six(streams, p)
    _check_old_six_rgb(out.cpu().numpy(), old, "nchw")
    from tests.oracle_binding import OracleDecoder
    for c in range(_GUARD_SRC):
        o = OracleDecoder(p.width, p.height, p.version)
        for f in range(6):
            o.Data, o.Offset = streams[c][f], 0
            assert o.DecodeFrame() is not None
            y, uv = o.y(0), o.uv(0)
            S, W, H = o.Stride, p.width, p.height
            want = np.concatenate([y[:H, :W].ravel(), uv[:H // 2, :W // 2].ravel(), uv[:H // 2, S // 2:S // 2 + W // 2].ravel()])
            assert np.array_equal(got[f, c], want), (c, f)
    for c in range(_GUARD_SRC, b.n, 97):
        assert np.array_equal(got[:, c], got[:, c % _GUARD_SRC]), c
    del keep
    b.close()


@pytest.mark.gpu
def test_device_export_of_every_group_part_without_waiting():
    """an 18-frame group finished in three parts; every part goes out as ONE device export (P - 1, P) on the current stream, with no wait in
    between: every frame of every clip equals the oracle's Bitmap"""
    import torch
    from mobiclipdecoder_amd import MobiclipBatch
    from tests.oracle_binding import OracleDecoder
    n, G = 6, 18
    streams = [_generated("B", 740 + c, G) for c in range(3)]
    p = streams[0][0]
    b = MobiclipBatch(n, p.width, p.height, p.version, device_parse=True)
    b.gop_begin([[streams[c % 3][1][k][0] for c in range(n)] for k in range(G)])
    parts, done = [], 0
    while done < G:
        rcs, _ = b.gop_finish()
        P = len(rcs)
        assert all(r == [0] * n for r in rcs)
        parts.append((done, b.export_tensor("rgb", P - 1, P)))
        done += P
    assert len(parts) == 3
    torch.cuda.synchronize()
    for c in range(3):
        o = OracleDecoder(p.width, p.height, p.version)
        want = []
        for k in range(G):
            o.Data, o.Offset = streams[c][1][k]
            assert o.DecodeFrame() is not None
            want.append(o.argb())
        for f0, t in parts:
            got = t.cpu().numpy()
            for j in range(got.shape[0]):
                for cl in range(c, n, 3):
                    assert np.array_equal(got[j, cl], _rgb_from_argb(want[f0 + j][None, None], "nchw")[0, 0]), (f0 + j, cl)
    b.close()


@pytest.mark.gpu
def test_device_export_refusals_enqueue_nothing():
    import torch
    from mobiclipdecoder_amd import MobiclipBatch, MobiclipError, host_empty
    p, fr = _generated("A", 31, 4)
    n = 3
    b = MobiclipBatch(n, p.width, p.height, p.version, device_parse=True)
    lib, h = b._lib, b._h
    dev = torch.device("cuda", b.device)
    W, H = p.width, p.height
    pic = 3 * W * H
    out = torch.full((6 * n * pic * 4 + 64,), 0xAB, dtype=torch.uint8, device=dev)
    ptr, nb = out.data_ptr(), out.numel()
    stream = torch.cuda.current_stream(dev).cuda_stream
    sb = (C.c_float * 6)(1, 1, 1, 0, 0, 0)
    ex = lambda fmt, dt, r, nf, c0, nc, d=ptr, nbytes=nb, s=None: lib.mobi_batch_export_device(h, fmt, dt, s, r, nf, c0, nc, d, nbytes, stream)
    assert ex(PLANAR, U8, 0, 1, 0, n) == MOBI_E_NULLREF
    b.decode([fr[0][0]] * n, [0] * n)
    b.decode([fr[1][0]] * n, [0] * n)
    assert ex(PLANAR, U8, 2, 1, 0, n) == MOBI_E_NULLREF
    host = np.zeros(nb, np.uint8)
    pinned = host_empty(nb, np.uint8)
    refused = [
        ex(PLANAR, U8, 0, 1, 0, n, d=host.ctypes.data), ex(I420, U8, 0, 1, 0, n, d=pinned.ctypes.data),  # host memory
        ex(PLANAR, U8, 0, 1, 0, n, d=ptr + 1), ex(PACKED, F32, 0, 1, 0, n, d=ptr + 8),                     # misaligned
        ex(PLANAR, U8, 1, 2, 0, n, nbytes=2 * n * pic - 1), ex(PLANAR, F16, 0, 1, 0, n, nbytes=n * pic * 2 - 1),
        ex(ARGB, U8, 0, 1, 0, n, nbytes=n * W * H * 4 - 1), ex(I420, U8, 0, 1, 0, n, nbytes=n * W * H * 3 // 2 - 1),
        ex(I420, F16, 0, 1, 0, n), ex(ARGB, F32, 0, 1, 0, n), ex(I420, U8, 0, 1, 0, n, s=sb), ex(PLANAR, U8, 0, 1, 0, n, s=sb),
        ex(PACKED, 3, 0, 1, 0, n), ex(PLANAR, -1, 0, 1, 0, n), ex(4, U8, 0, 1, 0, n), ex(-1, U8, 0, 1, 0, n),
        ex(PLANAR, U8, 6, 1, 0, n), ex(PLANAR, U8, -1, 1, 0, n), ex(PLANAR, U8, 0, 2, 0, n), ex(PLANAR, U8, 1, 0, 0, n),
        ex(PLANAR, U8, 0, 1, -1, 1), ex(PLANAR, U8, 0, 1, 0, n + 1), ex(PLANAR, U8, 0, 1, n, 1), ex(PLANAR, U8, 0, 1, 0, 0),
        lib.mobi_batch_export_device(h, PLANAR, U8, None, 0, 1, 0, n, None, nb, stream),
    ]
    assert refused == [MOBI_E_ARG] * len(refused), refused
    # ring indices of steps in flight
    b.submit([fr[2][0]] * n, [0] * n)
    b.submit([fr[3][0]] * n, [0] * n)
    for r, nf in ((0, 1), (1, 1), (1, 2), (2, 2), (3, 3)):
        assert ex(PLANAR, U8, r, nf, 0, n) == MOBI_E_ARG, (r, nf)
        with pytest.raises(MobiclipError):
            b.export_tensor("rgb", r, nf)
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())  # nothing was written
    b.wait()
    b.wait()
    # the same buffer is accepted once the request is right, and the batch goes on
    assert ex(PLANAR, U8, 0, 1, 0, n) == 0
    t = b.export_tensor("rgb", 0, 1)
    torch.cuda.synchronize()
    assert np.array_equal(out[:n * pic].cpu().numpy().reshape(t.shape), t.cpu().numpy())
    b.close()


@pytest.mark.gpu
def test_device_only_batch_allocates_no_staging():
    """a batch that only exports to device memory holds no staging chunks (4 x 64 MiB) and no bounce chunks"""
    import torch
    from mobiclipdecoder_amd import MobiclipBatch
    p, fr = _generated("A", 32, 1)
    n = 8
    b = MobiclipBatch(n, p.width, p.height, p.version)
    b.decode([fr[0][0]] * n, [0] * n)
    dev = torch.device("cuda", b.device)
    out = torch.empty((1, n, 3, p.height, p.width), dtype=torch.float32, device=dev)
    i420 = torch.empty((1, n, p.width * p.height * 3 // 2), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    b.export_tensor("rgb", 0, 1, dtype=torch.float32, out=out)
    b.export_tensor("i420", 0, 1, out=i420)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(dev)[0]
    assert free0 - free1 < (64 << 20), (free0, free1)
    assert np.array_equal(i420.cpu().numpy(), b.export("i420", 0, 1))  # (the host export then sets up its own staging)
    b.close()
