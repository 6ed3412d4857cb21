"""Cropped, area-downscaled RGB tensors from the ring in one kernel (mobi_batch_export_device_scaled, include/mobiclip_hip.h;
mobi_export_scale.h / mobi_export_scale.hip; MobiclipBatch.export_tensor(crop=, size=)).

CPU: the header, the binding and the exported symbol; the weights, the band geometry and the exact division of csrc/mobi_export_scale.h
compiled with g++ and walked; argument errors.  GPU (-m gpu), bit-exact against numpy: the fmt="argb" tensor of the same slot (which
test_export_device.py checks against the host export and the oracle), Wy @ V @ Wx.T in int64, (S + D // 2) // D, then the affine of
test_export_device.py::_affine."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_export_device import (AFFINES, CSRC, MAN, MOBI_E_ARG, MOBI_E_NULLREF, PACKED, PLANAR, ROOT, F16, F32, U8, _affine, _bits, _busy,
                                      _fake_batch, _generated, _golden, _guard_batch, _old_six)

I420, ARGB = 0, 1
SHAPES = [(64, 48, 64, 48), (61, 45, 20, 12), (640, 480, 224, 224), (640, 480, 4, 4), (528, 48, 132, 7), (33, 17, 32, 17), (5, 3, 4, 1)]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_scaled_export_and_the_library_exports_it():
    from mobiclipdecoder_amd import build, decoder
    text = open(os.path.join(ROOT, "include", "mobiclip_hip.h")).read()
    assert re.search(r"\bint mobi_batch_export_device_scaled\s*\(", text)
    res, args = decoder._SIGS["mobi_batch_export_device_scaled"]
    assert res is C.c_int and len(args) == 17 and args[4:14] == [C.c_int] * 10 and args[14:] == [C.c_void_p, C.c_size_t, C.c_void_p]
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], capture_output=True, text=True, check=True).stdout
    assert "mobi_batch_export_device_scaled" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    lib = decoder.load_library()
    buf = np.zeros(64, np.uint8)
    assert lib.mobi_batch_export_device_scaled(None, PLANAR, U8, None, 0, 0, 4, 4, 4, 4, 0, 1, 0, 1, buf.ctypes.data, buf.nbytes, None) == MOBI_E_ARG


_GEOM_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mobi_export_scale.h"
// argv: cw ch ow oh.  The weights against the definition, the work split, the division by D = cw * ch.
static int fail(const char *what, long a, long b, long c) { printf("FAIL %s %ld %ld %ld\n", what, a, b, c); return 1; }
static long formula(long o, long s, long out_n, long in_n) { // max(0, min((s+1) out_n, (o+1) in_n) - max(s out_n, o in_n))
  const long hi = (s + 1) * out_n < (o + 1) * in_n ? (s + 1) * out_n : (o + 1) * in_n, lo = s * out_n > o * in_n ? s * out_n : o * in_n;
  return hi > lo ? hi - lo : 0;
}
static int axis(uint32_t out_n, uint32_t in_n) {
  std::vector<long> sum(out_n, 0);
  for (uint32_t s = 0; s < in_n; s++) {
    uint32_t o, w, touched = 0;
    mobi_scale_tap(s, out_n, in_n, &o, &w);
    for (uint32_t x = 0; x < out_n; x++) {
      const long f = formula(x, s, out_n, in_n);
      if ((long)mobi_scale_weight(x, s, out_n, in_n) != f) return fail("weight", x, s, f);
      const long tap = x == o ? (long)w : x == o + 1 ? (long)out_n - (long)w : 0; // what the kernel adds
      if (tap != f) return fail("tap", x, s, f);
      touched += f != 0;
      sum[x] += f;
    }
    if (touched < 1 || touched > 2) return fail("outputs of one source", s, touched, 0);
    if (o >= out_n || w < 1 || w > out_n || (o + 1 == out_n && w != out_n)) return fail("tap range", s, o, w);
  }
  for (uint32_t x = 0; x < out_n; x++)
    if (sum[x] != (long)in_n) return fail("row sum", x, sum[x], in_n);
  return 0;
}
// every span of outputs [o0, o1): its sources are inside [0, in_n), tight, and hold all the weight
static int span(uint32_t o0, uint32_t o1, uint32_t out_n, uint32_t in_n) {
  uint32_t s0, s1;
  mobi_scale_span(o0, o1, out_n, in_n, &s0, &s1);
  if (s0 >= s1 || s1 > in_n) return fail("span range", o0, s0, s1);
  for (uint32_t s = 0; s < in_n; s++) {
    long w = 0;
    for (uint32_t o = o0; o < o1; o++) w += formula(o, s, out_n, in_n);
    const bool inside = s >= s0 && s < s1;
    if (!inside && w) return fail("weight outside the span", o0, s, w);
    if ((s == s0 || s == s1 - 1) && !w) return fail("span not tight", o0, s, 0);
  }
  return 0;
}
int main(int argc, char **argv) {
  if (argc != 5) return 2;
  const uint32_t cw = atoi(argv[1]), ch = atoi(argv[2]), ow = atoi(argv[3]), oh = atoi(argv[4]);
  if (axis(ow, cw) || axis(oh, ch)) return 1;
  const MobiScalePlan p = mobi_scale_plan(3, 2, cw, ch, ow, oh);
  if (p.cx != 3 || p.cy != 2 || p.cw != cw || p.ch != ch || p.ow != ow || p.oh != oh || p.half != cw * ch / 2) return fail("plan", 0, 0, 0);
  if (p.strip_w % 4 || p.strip_w < 4 || p.strip_w > kMobiScaleStripMax || p.band_rows < 1) return fail("tile size", p.strip_w, p.band_rows, 0);
  if (mobi_scale_lds_bytes(&p) > kMobiScaleLdsBytes || mobi_scale_lds_bytes(&p) != p.band_rows * p.strip_w * 12) return fail("lds", mobi_scale_lds_bytes(&p), 0, 0);
  if (mobi_scale_picture_bytes(ow, oh, 2) != (size_t)6 * ow * oh) return fail("picture bytes", 0, 0, 0);
  std::vector<int> rows(oh, 0), cols(ow, 0);
  for (uint32_t b = 0; b < p.n_bands; b++)
    for (uint32_t s = 0; s < p.n_strips; s++) {
      uint32_t r0, r1, c0, c1;
      mobi_scale_tile(&p, b, s, &r0, &r1, &c0, &c1);
      if (r0 >= r1 || r1 > oh || r1 - r0 > p.band_rows || c0 >= c1 || c1 > ow || c1 - c0 > p.strip_w || (c0 | c1) % 4) return fail("tile", b, s, r0);
      if (s == 0) for (uint32_t r = r0; r < r1; r++) rows[r]++;
      if (b == 0) for (uint32_t c = c0; c < c1; c++) cols[c]++;
      if (span(r0, r1, oh, ch) || span(c0, c1, ow, cw)) return 1;
    }
  for (uint32_t r = 0; r < oh; r++) if (rows[r] != 1) return fail("row covered", r, rows[r], 0);
  for (uint32_t c = 0; c < ow; c++) if (cols[c] != 1) return fail("column covered", c, cols[c], 0);
  // the division: where the quotient of (S + D / 2) / D changes, one to either side, and the largest S
  const uint64_t D = (uint64_t)cw * ch, up = (D + 1) / 2;
  const MobiScaleDiv dv = mobi_scale_div_make((uint32_t)D);
  if (dv.m != p.div.m || dv.sh != p.div.sh) return fail("plan div", dv.m, dv.sh, 0);
  long checked = 0;
  for (uint64_t k = 0; k <= 255; k++)
    for (int d = -1; d <= 1; d++) {
      const int64_t S = (int64_t)(k * D) - (int64_t)up + d;
      if (S < 0 || (uint64_t)S > 255 * D) continue;
      const uint64_t n = (uint64_t)S + D / 2;
      if (n >> 31) return fail("sum range", k, d, 0);
      if (mobi_scale_div((uint32_t)n, dv) != n / D) return fail("division", k, d, (long)(n / D));
      checked++;
    }
  if (mobi_scale_div((uint32_t)(255 * D + D / 2), dv) != 255) return fail("division at 255 D", 0, 0, 0);
  if (checked < 255 * 3) return fail("division points", checked, 0, 0);
  printf("ok\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def geom_tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("export_scale_geom")
    src, exe = d / "geom.cpp", d / "geom"
    src.write_text(_GEOM_CPP)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("cw,ch,ow,oh", SHAPES)
def test_weights_bands_and_division_of_the_scale_header(geom_tool, cw, ch, ow, oh):
    """the code the kernel runs (mobi_export_scale.h), on the CPU: the two weights a source gets equal the definition's for every (output,
    source) pair, an output's weights sum to the source count, a source has weight in one or two outputs; the tiles cover every output row
    and column once, within the LDS budget; a tile's source span lies inside the crop, is tight and holds all of the tile's weight; the
    multiply-and-shift division equals (S + D / 2) // D at every S where the quotient changes, one to either side, and at 255 D"""
    r = subprocess.run([geom_tool, str(cw), str(ch), str(ow), str(oh)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def test_division_constant_for_every_shape_is_32_bit():
    """m = ceil(2^(31 + l) / D) < 2^32 for D up to the 2^23 the entry point accepts (python integers)"""
    for D in [cw * ch for cw, ch, _, _ in SHAPES] + [1, 2, 3, 4, 15, (1 << 23) - 1, 1 << 23, (1 << 22) + 1]:
        l = (D - 1).bit_length()
        m = -(-(1 << (31 + l)) // D)
        assert m < 1 << 32 and (1 << (31 + l)) <= m * D <= (1 << (31 + l)) + (1 << l), D


_BAD = [
    dict(crop=(1, 0, 64, 48)), dict(crop=(0, 1, 64, 48)), dict(crop=(-1, 0, 4, 4)), dict(crop=(0, -1, 4, 4)), dict(crop=(0, 0, 0, 4)),
    dict(crop=(0, 0, 4, 0)), dict(crop=(60, 0, 8, 8)),                                                                   # outside / empty
    dict(crop=(0, 0, 32, 32), size=(33, 32)), dict(crop=(0, 0, 32, 32), size=(32, 36)), dict(size=(49, 64)), dict(size=(48, 68)),
    dict(size=(0, 64)), dict(size=(48, 0)),                                                                              # larger than the crop / < 1
    dict(size=(24, 30)), dict(crop=(3, 2, 61, 45)), dict(crop=(0, 0, 32, 32), size=(16, 18)),                             # out_w % 4
    dict(fmt="i420", crop=(0, 0, 32, 32)), dict(fmt="argb", size=(24, 32)), dict(fmt="i420", size=(48, 64)),              # not RGB
    dict(crop=(0, 0, 64)), dict(crop=5), dict(crop=(0, 0, 64.0, 48)), dict(crop="abcd"), dict(crop=(0, 0, True, 4)),
    dict(size=(24,)), dict(size="ab"), dict(size=(True, 4)), dict(size=(24, 32, 3)), dict(size=24), dict(size=(24.0, 32)),  # tuples
]


@pytest.mark.parametrize("k", range(len(_BAD)))
def test_export_tensor_crop_and_size_errors_raise_value_error_before_any_library_call(k):
    b = _fake_batch()  # 4 clips of 64x48; any library call raises AssertionError
    with pytest.raises(ValueError):
        b.export_tensor(**_BAD[k])


def test_export_tensor_refuses_a_crop_of_more_than_2_23_pixels():
    b = _fake_batch(1, 4096, 2064)
    with pytest.raises(ValueError):
        b.export_tensor(size=(224, 224))
    with pytest.raises(ValueError):
        b.export_tensor(crop=(0, 0, 4096, 2049), size=(224, 224))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _weights(out_n, in_n):
    o, s = np.arange(out_n, dtype=np.int64)[:, None], np.arange(in_n, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((s + 1) * out_n, (o + 1) * in_n) - np.maximum(s * out_n, o * in_n))


def _model(bm, crop, size):
    """(..., H, W) uint32 Bitmaps -> (..., 3, oh, ow) uint8: the definition"""
    cx, cy, cw, ch = crop
    oh, ow = size
    v = np.stack([(bm >> s) & 0xFF for s in (16, 8, 0)], axis=-3).astype(np.int64)[..., cy:cy + ch, cx:cx + cw]
    S = _weights(oh, ch) @ v @ _weights(ow, cw).T
    D = cw * ch
    q = (S + D // 2) // D
    assert q.min() >= 0 and q.max() <= 255
    return q.astype(np.uint8)


def _want(bm, crop, size, layout, sb, ndt):
    q = _model(bm, crop, size)
    if layout == "nhwc":
        q = np.moveaxis(q, -3, -1)
    return q if ndt == np.uint8 else _affine(q, layout, sb, ndt)


def _argb(b, ring_idx=0, nf=1, clips=None):
    return b.export_tensor("argb", ring_idx, nf, clips).cpu().numpy().view(np.uint32)


def _check(b, bm, crop, size, layout, tdt, aff, ring_idx=0, nf=1, clips=None, stream=None):
    import torch
    sb = AFFINES[aff]
    kw = {} if sb is None or tdt == torch.uint8 else dict(scale=sb[0].tolist(), bias=sb[1].tolist())
    ndt = {torch.uint8: np.uint8, torch.float16: np.float16, torch.float32: np.float32}[tdt]
    got = b.export_tensor("rgb", ring_idx, nf, clips, layout=layout, dtype=tdt, crop=crop, size=size, stream=stream, **kw)
    H, W = b.Height, b.Width
    full_crop = (0, 0, W, H) if crop is None else crop
    want = _want(bm, full_crop, (full_crop[3], full_crop[2]) if size is None else size, layout, sb, ndt)
    assert got.dtype == tdt and tuple(got.shape) == want.shape, (got.shape, want.shape)
    g = got.cpu().numpy()
    if not np.array_equal(_bits(g), _bits(want)):
        bad = np.argwhere(_bits(g) != _bits(want))
        raise AssertionError((crop, size, layout, str(tdt), aff, len(bad), bad[:4].tolist(), g[tuple(bad[0])], want[tuple(bad[0])]))
    return got


def _decoded(name, n=2, frames=3):
    import torch  # noqa: F401  (before the library: one HIP runtime)
    from mobiclipdecoder_amd import MobiclipBatch
    case = next(c for c in MAN["cases"] if c["name"] == name)
    b = MobiclipBatch(n, case["width"], case["height"], case["version"])
    for d, off in _golden(case)[:frames]:
        b.decode([d] * n, [off] * n)
    return b


VARIANTS = [("nchw", "uint8", "unit"), ("nhwc", "uint8", "unit"), ("nchw", "float16", "unit"), ("nhwc", "float16", "imagenet"),
            ("nchw", "float32", "imagenet"), ("nhwc", "float32", "unit")]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mods_64x48_rich", "moflex_64x48_rich_iint"])
def test_whole_picture_at_its_own_size_is_the_full_size_export(name):
    import torch
    b = _decoded(name)
    W, H = b.Width, b.Height
    bm = _argb(b, 2, 3)
    for layout in ("nchw", "nhwc"):
        for tdt in (torch.uint8, torch.float16, torch.float32):
            for aff in (("unit",) if tdt == torch.uint8 else ("unit", "imagenet")):
                sb = AFFINES[aff]
                kw = {} if sb is None else dict(scale=sb[0].tolist(), bias=sb[1].tolist())
                full = b.export_tensor("rgb", 2, 3, layout=layout, dtype=tdt, **kw)
                for ckw in (dict(crop=(0, 0, W, H), size=(H, W)), dict(crop=(0, 0, W, H)), dict(size=(H, W))):
                    got = b.export_tensor("rgb", 2, 3, layout=layout, dtype=tdt, **ckw, **kw)
                    assert got.dtype == full.dtype and got.shape == full.shape
                    assert np.array_equal(_bits(got.cpu().numpy()), _bits(full.cpu().numpy())), (layout, tdt, aff, ckw)
                _check(b, bm, (0, 0, W, H), (H, W), layout, tdt, aff, 2, 3)  # (and the model agrees with both)
    b.close()


def _sizes(cw, ch):
    """(out_h, out_w): the crop's own size (the width rounded down to a multiple of 4), half of it, and a non-integer factor"""
    s = [(ch, cw & ~3), (max(1, ch // 2), max(4, (cw // 2) & ~3)), (max(1, ch * 4 // 15), max(4, (cw // 3) & ~3))]
    return sorted(set(s), reverse=True)


# odd x and y; ending on the last row / column and one short of them; across macroblock (16) and quadrant (8) boundaries; 4 wide
_CROPS_64x48 = [(0, 0, 64, 48), (3, 2, 61, 45), (3, 3, 61, 45), (1, 1, 62, 46), (13, 5, 22, 30), (17, 9, 4, 7), (60, 41, 4, 7), (7, 15, 12, 2)]
PLACEMENTS = {
    "mods_64x48_rich": _CROPS_64x48,
    "moflex_64x48_rich_iint": _CROPS_64x48,
    "r05_far_mv_moflex_32x32": [(0, 0, 32, 32), (3, 1, 29, 31), (1, 1, 30, 30), (5, 5, 22, 22), (13, 9, 4, 7), (28, 25, 4, 7)],
    "moflex_528x48_edge_pad": [(0, 0, 528, 48), (3, 2, 525, 45), (3, 3, 525, 45), (1, 1, 526, 46), (250, 5, 30, 30), (515, 9, 4, 7), (9, 7, 517, 33)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_crop_placement_and_scale_factors(name):
    """every crop at its own size, at half and at a non-integer factor: uint8 planar and one float packed variant each.  528 wide is 33
    macroblocks per row; (3, 2, 61, 45) -> 20 x 12 and 528 x 48 -> 132 x 7 are among them"""
    import torch
    b = _decoded(name)
    bm = _argb(b)
    n = 0
    for crop in PLACEMENTS[name]:
        sizes = _sizes(crop[2], crop[3]) + ([(7, 132)] if crop == (0, 0, 528, 48) else [])
        for size in sizes:
            _check(b, bm, crop, size, "nchw", torch.uint8, "unit")
            _check(b, bm, crop, size, "nhwc", (torch.float16, torch.float32)[n % 2], "imagenet")
            n += 1
    if name == "mods_64x48_rich":
        assert (12, 20) in _sizes(61, 45)
        for layout, dt, aff in VARIANTS:  # every variant once on an awkward crop
            _check(b, bm, (3, 2, 61, 45), (12, 20), layout, getattr(torch, dt), aff)
        _check(b, bm, (4, 4, 56, 40), None, "nchw", torch.uint8, "unit")  # crop alone: a pure crop
        _check(b, bm, None, (12, 20), "nhwc", torch.uint8, "unit")        # size alone: the whole picture
    b.close()


@pytest.mark.gpu
def test_stride_equal_to_width():
    import torch
    b = _decoded("mods_256x192_A")
    bm = _argb(b)
    for size in ((48, 64), (75, 100)):
        for layout, dt, aff in VARIANTS[:4]:
            _check(b, bm, None, size, layout, getattr(torch, dt), aff)
    _check(b, bm, (1, 1, 255, 191), (75, 100), "nchw", torch.uint8, "unit")
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,crop,size", [("moflex_640x480_B", None, (4, 4)), ("moflex_640x480_B", None, (224, 224)),
                                            ("moflex_848x480_C", (184, 0, 480, 480), (224, 224))])
def test_large_ratio_and_the_real_shapes(name, crop, size):
    """640x480 -> 4x4 is 160 source columns and 120 rows per output (D = 307 200); the others are the shapes a consumer asks for"""
    import torch
    b = _decoded(name, n=1, frames=2)
    bm = _argb(b)
    for layout, dt, aff in VARIANTS:
        _check(b, bm, crop, size, layout, getattr(torch, dt), aff)
    b.close()


@pytest.mark.gpu
def test_several_frames_and_clips_in_one_call():
    """3 different clips x 4 frames, clips 1..2: picture (j * n_clips + c) is frame j (ring slot of ring index 3 - j) of clip 1 + c"""
    import torch
    from mobiclipdecoder_amd import MobiclipBatch
    streams = [_generated("A", 900 + c, 4) for c in range(3)]
    p = streams[0][0]
    b = MobiclipBatch(3, p.width, p.height, p.version)
    for f in range(4):
        rcs, _ = b.decode([streams[c][1][f][0] for c in range(3)], [0] * 3)
        assert rcs == [0] * 3
    assert (p.width, p.height) == (256, 192)
    crop, size = (33, 1, 222, 190), (90, 104)
    bm = _argb(b, 3, 4, range(1, 3))
    assert not np.array_equal(bm[0], bm[1]) and not np.array_equal(bm[:, 0], bm[:, 1])  # (frames and clips do differ)
    _check(b, bm, crop, size, "nchw", torch.uint8, "unit", 3, 4, range(1, 3))
    _check(b, bm, crop, size, "nhwc", torch.float16, "imagenet", 3, 4, range(1, 3))
    _check(b, bm[1:3, 1:], crop, size, "nchw", torch.float32, "imagenet", 2, 2, range(2, 3))
    b.close()


@pytest.mark.gpu
def test_scaled_export_refusals_enqueue_nothing():
    import torch
    from mobiclipdecoder_amd import MobiclipBatch
    p, fr = _generated("B", 31, 3)
    n = 2
    b = MobiclipBatch(n, p.width, p.height, p.version, device_parse=True)
    assert (p.width, p.height) == (640, 480)
    lib, h = b._lib, b._h
    dev = torch.device("cuda", b.device)
    W, H = p.width, p.height
    out = torch.full((2 * n * 3 * W * H + 64,), 0xAB, dtype=torch.uint8, device=dev)
    ptr, nb = out.data_ptr(), out.numel()
    stream = torch.cuda.current_stream(dev).cuda_stream
    sb = (C.c_float * 6)(1, 1, 1, 0, 0, 0)

    def ex(fmt=PLANAR, dt=U8, crop=(80, 0, 480, 480), size=(224, 224), r=0, nf=1, c0=0, nc=n, d=ptr, nbytes=nb, s=None):  # size = (out_w, out_h)
        return lib.mobi_batch_export_device_scaled(h, fmt, dt, s, crop[0], crop[1], crop[2], crop[3], size[0], size[1], r, nf, c0, nc, d, nbytes, stream)
    assert ex() == MOBI_E_NULLREF
    b.decode([fr[0][0]] * n, [0] * n)
    assert ex(r=1) == MOBI_E_NULLREF
    pic = 3 * 224 * 224
    refused = [
        ex(fmt=I420), ex(fmt=ARGB), ex(fmt=4), ex(fmt=-1),                                                                # not RGB
        ex(crop=(161, 0, 480, 480)), ex(crop=(0, 1, 480, 480)), ex(crop=(-1, 0, 480, 480)), ex(crop=(0, -1, 480, 480)),   # not inside
        ex(crop=(0, 0, 0, 480)), ex(crop=(0, 0, 480, 0)), ex(crop=(0, 0, -4, 480)), ex(crop=(0, 0, W + 1, H)),            # empty / too large
        ex(crop=(0x7FFFFFF0, 0, 480, 480)), ex(crop=(0, 0, 0x7FFFFFFF, 480)),
        ex(size=(0, 224)), ex(size=(224, 0)), ex(size=(-4, 224)),                                                         # below 1
        ex(size=(484, 224)), ex(size=(224, 481)), ex(crop=(0, 0, 8, 8), size=(12, 8)),                                    # upscaling
        ex(size=(222, 224)), ex(size=(1, 224)), ex(crop=(0, 0, 61, 45), size=(61, 45)),                                   # out_w % 4
        ex(dt=U8, s=sb), ex(dt=3), ex(dt=-1),                                                                             # dtype / scale_bias
        ex(d=ptr + 4), ex(nbytes=n * pic - 1), ex(dt=F16, nbytes=2 * n * pic - 1), ex(dt=F32, nbytes=4 * n * pic - 1),     # dst
        ex(r=6), ex(r=-1), ex(nf=2), ex(nf=0), ex(c0=-1, nc=1), ex(nc=n + 1), ex(c0=n, nc=1), ex(nc=0),                   # ring / clips
        lib.mobi_batch_export_device_scaled(h, PLANAR, U8, None, 80, 0, 480, 480, 224, 224, 0, 1, 0, n, None, nb, stream),
    ]
    assert refused == [MOBI_E_ARG] * len(refused), refused
    # (crop_w * crop_h > 2^23 cannot be asked of a real batch: mobi_batch_create takes pictures of at most 8191 macroblocks, 2^21 pixels, and
    # a crop lies inside the picture.  The binding's check of it runs on the CPU, above.)
    b.submit([fr[1][0]] * n, [0] * n)  # ring index 0 is a step in flight
    assert ex() == MOBI_E_ARG
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())  # nothing was written
    b.wait()
    # the same buffer is accepted once the request is right
    assert ex() == 0
    t = b.export_tensor("rgb", crop=(80, 0, 480, 480), size=(224, 224))
    torch.cuda.synchronize()
    assert np.array_equal(out[:n * pic].cpu().numpy().reshape(t.shape), t.cpu().numpy())
    assert bool((out[n * pic:] == 0xAB).all())
    b.close()


@pytest.mark.gpu
def test_scaled_export_is_ordered_on_the_stream_without_a_host_sync():
    """a torch reduction enqueued on the export's stream right behind it, a side stream held busy first, sees the pictures"""
    import torch
    from mobiclipdecoder_amd import MobiclipBatch
    p, fr = _generated("B", 21, 2)
    n = 32
    b = MobiclipBatch(n, p.width, p.height, p.version)
    for f in range(2):
        b.decode([fr[f][0]] * n, [0] * n)
    crop, size = (80, 0, 480, 480), (224, 224)
    want = _model(_argb(b, 1, 2, range(0, 1)), crop, size).astype(np.int64).sum(axis=(3, 4)).repeat(n, axis=1)  # (F, n, 3)
    dev = torch.device("cuda", b.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        a = torch.randn(4096, 4096, device=dev)
        for _ in range(10):
            a = a @ a / 64.0
        out = b.export_tensor("rgb", 1, 2, dtype=torch.float32, stream=side, crop=crop, size=size)
        sums = out.double().sum(dim=(3, 4))
    side.synchronize()
    assert np.array_equal(sums.cpu().numpy().astype(np.int64), want)
    b.close()


@pytest.mark.gpu
def test_slot_guard_holds_replayed_steps_behind_a_scaled_export_on_a_busy_stream():
    """test_export_device.py's guard test with the scaled export as the reader: the export sits behind a few hundred milliseconds of work on
    a side stream, six steps that write every exported slot are enqueued at once, and the tensor holds the old frames"""
    import torch
    b, p, streams = _guard_batch(760)
    dev = torch.device("cuda", b.device)
    side = torch.cuda.Stream(device=dev)
    keep = _busy(side, dev)
    crop, size = (80, 0, 480, 480), (224, 224)
    out = b.export_tensor("rgb", 5, 6, range(0, 16), layout="nhwc", stream=side, crop=crop, size=size)
    for f in range(6, 12):  # six steps enqueued at once, each writing a slot the export has not read yet
        b.replay(f)
    assert b.sync() == 0
    torch.cuda.synchronize()
    old = _old_six(streams, p)  # [source][frame] -> (H, W) uint32, the oracle's Bitmaps
    got = out.cpu().numpy()
    m = len(old)
    want = [[np.moveaxis(_model(old[c][f], crop, size), 0, -1) for f in range(6)] for c in range(m)]
    for c in range(got.shape[1]):
        for f in range(6):
            assert np.array_equal(got[f, c], want[c % m][f]), (c, f)
    new = b.export_tensor("rgb", 0, 1, range(0, 1), layout="nhwc", crop=crop, size=size)
    assert not np.array_equal(new.cpu().numpy()[0, 0], got[5, 0])  # (the ring did move on)
    del keep
    b.close()
