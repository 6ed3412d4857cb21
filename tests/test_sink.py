"""The clip sink without a GPU (mobi_batch_set_sink, mobi_sink_check, mobi_sink_plan, mobi_batch_gop_finish_all; csrc/mobi_sink.h): the header,
the binding and the exports; every refusal of mobi_sink_check and an accepted case per layout; mobi_sink_plan against a few lines of Python;
mobi_sink.h under the host compiler -- every element address of every layout, none twice, none outside -- plain and under the address and
undefined-behaviour sanitizers (a stand-alone program, run as a child); the Python argument errors on a fake batch."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_export_device import CSRC, MOBI_E_ARG, PACKED, PLANAR, ROOT, F16, F32, U8, _fake_batch

SYMBOLS = ("mobi_batch_set_sink", "mobi_batch_sink_pending", "mobi_batch_sink_launches", "mobi_sink_check", "mobi_sink_plan", "mobi_batch_gop_finish_all")
W, H = 64, 48  # the picture of the checks below


def _lib():
    from mobiclipdecoder_amd import decoder
    return decoder.load_library()


def _spec(n=5, T=3, s=2, ow=16, oh=12, fmt=PLANAR, dtype=U8, layout="ntchw", start=None, boxes=None, sb=None, gap=0, dst=1 << 20, dst_bytes=None, **over):
    """a mobi_sink of layout `layout` (gap: elements between neighbours of every outer dimension: a view with gaps), and what keeps its arrays alive"""
    from mobiclipdecoder_amd.decoder import SinkSpec
    esize = {U8: 1, F16: 2, F32: 4}.get(dtype, 1)
    plane = ow * oh
    ext = {"n": n, "t": T, "c": 3}
    if fmt == PLANAR:
        order = {"ntchw": "ntc", "ncthw": "nct", "tnchw": "tnc"}[layout]
        inner = plane
    else:
        order = {"nthwc": "nt", "tnhwc": "tn"}[layout]
        inner = plane * 3
    strides = {}
    for d in reversed(order):
        strides[d] = inner + gap
        inner = strides[d] * ext[d]
    keep = []
    st = None
    if start is not None:
        st = (C.c_int32 * n)(*start)
        keep.append(st)
    bx = None
    if boxes is not None:
        bx = (C.c_int32 * (5 * n))(*[v for row in boxes for v in row])
        keep.append(bx)
    sbp = None
    if sb is not None:
        sbp = (C.c_float * 6)(*sb)
        keep.append(sbp)
    sp = SinkSpec(fmt, dtype, sbp, bx, ow, oh, T, s, st, strides["n"], strides["t"], strides.get("c", 0), dst, inner * esize if dst_bytes is None else dst_bytes)
    for k, v in over.items():
        setattr(sp, k, v)
    sp._keep = keep
    return sp


def test_header_declares_the_sink_and_the_library_exports_it():
    from mobiclipdecoder_amd import build, decoder
    hdr = open(os.path.join(ROOT, "include", "mobiclip_hip.h")).read()
    assert re.search(r"int\s+mobi_batch_set_sink\(mobi_batch \*b, const mobi_sink \*spec\);", hdr)
    assert re.search(r"int\s+mobi_batch_sink_pending\(const mobi_batch \*b\);", hdr)
    assert re.search(r"long mobi_batch_sink_launches\(const mobi_batch \*b\);", hdr)
    assert re.search(r"int\s+mobi_sink_check\(const mobi_sink \*spec, int n_clips, uint32_t width, uint32_t height\);", hdr)
    assert re.search(r"int\s+mobi_sink_plan\(const mobi_sink \*spec, int n_clips, int64_t step, int32_t \*clips_out, int64_t \*elem_off_out\);", hdr)
    assert re.search(r"int\s+mobi_batch_gop_finish_all\(mobi_batch \*b, int32_t \*offsets_out, int \*rc\);", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert re.search(r"\bT " + name + r"\b", out), name
        assert name in decoder._SIGS
    # struct mobi_sink: the binding's layout is the header's (14 fields, in order)
    body = re.search(r"typedef struct mobi_sink \{(.*?)\} mobi_sink;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*[;,]", body)
    assert names == [f[0] for f in decoder.SinkSpec._fields_], names


def test_null_handles_are_refused():
    lib = _lib()
    sp = _spec()
    assert lib.mobi_batch_set_sink(None, C.byref(sp)) == MOBI_E_ARG
    assert lib.mobi_batch_set_sink(None, None) == MOBI_E_ARG
    assert lib.mobi_batch_gop_finish_all(None, None, None) == MOBI_E_ARG
    assert lib.mobi_batch_sink_pending(None) == 0
    assert lib.mobi_batch_sink_launches(None) == 0
    assert lib.mobi_sink_check(None, 5, W, H) == MOBI_E_ARG
    assert lib.mobi_sink_plan(None, 5, 0, None, None) == MOBI_E_ARG


ACCEPTED = [dict(layout="ntchw"), dict(layout="ncthw"), dict(layout="tnchw"), dict(layout="nthwc", fmt=PACKED), dict(layout="tnhwc", fmt=PACKED),
            dict(layout="ncthw", gap=8), dict(layout="nthwc", fmt=PACKED, gap=4), dict(layout="ntchw", dtype=F16, sb=(1, 1, 1, 0, 0, 0), gap=12),
            dict(layout="ntchw", dtype=F32), dict(n=1, T=1, s=1), dict(start=[0, 1, 2, 3, 2**31 - 1 - 4]),
            dict(boxes=[(0, 0, 64, 48, 0), (3, 2, 8, 6, 1), (60, 40, 4, 8, 0), (1, 1, 62, 46, 1), (17, 9, 16, 12, 0)])]


@pytest.mark.parametrize("k", range(len(ACCEPTED)))
def test_sink_check_accepts(k):
    kw = dict(ACCEPTED[k])
    n = kw.get("n", 5)
    assert _lib().mobi_sink_check(C.byref(_spec(**kw)), n, W, H) == 0, kw


_PLANE = 16 * 12
REFUSED = {
    "format i420": dict(format=0), "format argb": dict(format=1), "format 7": dict(format=7),
    "dtype 5": dict(dtype=5), "u8 with an affine": dict(sb=(1, 1, 1, 0, 0, 0)), "dtype i16": dict(dtype=3),
    "box right of the picture": dict(boxes=[(0, 0, 64, 48, 0)] * 4 + [(1, 0, 64, 48, 0)]),
    "box below the picture": dict(boxes=[(0, 0, 64, 48, 0)] * 4 + [(0, 41, 4, 8, 0)]),
    "empty box": dict(boxes=[(0, 0, 64, 48, 0)] * 4 + [(0, 0, 0, 8, 0)]),
    "negative box origin": dict(boxes=[(-1, 0, 8, 8, 0)] + [(0, 0, 64, 48, 0)] * 4),
    "flag bits": dict(boxes=[(0, 0, 64, 48, 2)] + [(0, 0, 64, 48, 0)] * 4),
    "out_w % 4": dict(ow=18), "out_w 0": dict(out_w=0), "out_h 0": dict(out_h=0),
    "D > 2^23": dict(ow=2048, oh=1028),  # (2 * 2048) * (2 * 1028) > 2^23: both axes grow
    "T 0": dict(n_frames=0), "T negative": dict(n_frames=-1), "stride 0": dict(stride=0), "stride negative": dict(stride=-2),
    "negative start": dict(start=[0, 1, -1, 3, 0]), "start beyond int32": dict(start=[0, 0, 0, 0, 2**31 - 4]),
    "reach beyond int32": dict(T=3, s=2**30),
    "dst unaligned": dict(dst=(1 << 20) + 8), "dst null": dict(dst=0),
    "clip stride % 4": dict(gap=2), "frame stride % 4": dict(frame_stride=3 * _PLANE + 2), "chan stride % 4": dict(chan_stride=_PLANE + 1),
    "packed with a channel stride": dict(layout="nthwc", fmt=PACKED, chan_stride=4),
    "channels overlap": dict(chan_stride=_PLANE - 4), "frames overlap": dict(frame_stride=3 * _PLANE - 4), "clips overlap": dict(clip_stride=9 * _PLANE - 4),
    "negative stride": dict(frame_stride=-3 * _PLANE),
    "clips inside frames": dict(layout="tnchw", clip_stride=4),
    "one picture short": dict(dst_bytes=15 * 3 * _PLANE - 1), "dst_bytes 0": dict(dst_bytes=0),
    "f16 one element short": dict(dtype=F16, dst_bytes=2 * 15 * 3 * _PLANE - 2),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_sink_check_refuses(name):
    assert _lib().mobi_sink_check(C.byref(_spec(**REFUSED[name])), 5, W, H) == MOBI_E_ARG, name


def test_sink_check_refuses_by_the_batch_geometry():
    lib = _lib()
    sp = _spec(n=5)
    assert lib.mobi_sink_check(C.byref(sp), 5, W, H) == 0
    assert lib.mobi_sink_check(C.byref(sp), 6, W, H) == MOBI_E_ARG      # a sixth clip's pictures leave dst
    assert lib.mobi_sink_check(C.byref(sp), 0, W, H) == MOBI_E_ARG
    bx = _spec(boxes=[(0, 0, 64, 48, 0)] * 5)
    assert lib.mobi_sink_check(C.byref(bx), 5, W, H) == 0
    assert lib.mobi_sink_check(C.byref(bx), 5, 48, 48) == MOBI_E_ARG    # the same boxes in a narrower picture


def _python_plan(n, T, s, start, step, clip_stride, frame_stride):
    out = []
    for c in range(n):
        d = step - start[c]
        if d >= 0 and d % s == 0 and d // s < T:
            out.append((c, c * clip_stride + (d // s) * frame_stride))
    return out


@pytest.mark.parametrize("n,T,s", list(itertools.product((1, 5), (1, 3), (1, 2, 3))))
@pytest.mark.parametrize("layout", ["ntchw", "ncthw", "tnhwc"])
def test_sink_plan_is_the_python_plan(n, T, s, layout):
    lib = _lib()
    for start in ([0] * n, [0, 1, 2, 3, 0][:n], [4, 4, 0, 4, 40][:n]):  # all 0; mixed; equal starts and one beyond every other clip's last step
        sp = _spec(n=n, T=T, s=s, layout=layout, fmt=PACKED if layout.endswith("c") else PLANAR, start=start, gap=4)
        assert lib.mobi_sink_check(C.byref(sp), n, W, H) == 0
        span = 16 * 12 * 3 if sp.format == PACKED else 2 * sp.chan_stride + 16 * 12
        seen, total = set(), 0
        clips, offs = (C.c_int32 * n)(), (C.c_int64 * n)()
        for step in range(-1, max(start) + T * s + 2):
            k = lib.mobi_sink_plan(C.byref(sp), n, step, clips, offs)
            want = _python_plan(n, T, s, start, step, sp.clip_stride, sp.frame_stride)
            assert k == len(want) and [(clips[i], offs[i]) for i in range(k)] == want, (start, step)
            assert lib.mobi_sink_plan(C.byref(sp), n, step, None, None) == k
            for i in range(k):
                assert offs[i] not in seen and 0 <= offs[i] and (offs[i] + span) <= sp.dst_bytes
                seen.add(offs[i])
            total += k
        assert total == n * T
        assert lib.mobi_sink_plan(C.byref(sp), n, 2**40, clips, offs) == 0


_ADDR_CPP = r"""
// every element address of every (c, t, ch, y, x) of a sink tensor through mobi_sink.h: none twice, none outside, and the layout rule agrees
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "mobi_sink.h"
static int fail(const char *what, long a, long b) { printf("FAIL %s %ld %ld\n", what, a, b); return 1; }
int main(int argc, char **argv) {
  if (argc != 10) return 2;
  const int planar = atoi(argv[1]), n = atoi(argv[2]), T = atoi(argv[3]), stride = atoi(argv[4]);
  const uint32_t ow = (uint32_t)atoi(argv[5]), oh = (uint32_t)atoi(argv[6]);
  const int64_t cs = atoll(argv[7]), fs = atoll(argv[8]), chs = atoll(argv[9]);
  int64_t span = 0;
  if (!mobi_sink_layout_ok(planar, (uint32_t)n, T, ow, oh, cs, fs, chs, (uint64_t)1 << 40, &span)) return fail("layout refused", 0, 0);
  if (mobi_sink_layout_ok(planar, (uint32_t)n, T, ow, oh, cs, fs, chs, (uint64_t)span - 1, nullptr)) return fail("one element short accepted", span, 0);
  std::vector<unsigned char> seen((size_t)span, 0); // (exactly the span: the sanitizers see an address outside it)
  const uint32_t start[5] = {0, 1, 2, 3, 0};
  long marked = 0;
  for (int64_t step = 0; step < 3 + (int64_t)T * stride + 1; step++) {
    const MobiSinkSched sch{step, stride, T, cs, fs, chs};
    for (int c = 0; c < n; c++) {
      const int32_t t = mobi_sink_select(step, start[c % 5], stride, T);
      if (t < 0) continue;
      if ((int64_t)start[c % 5] + (int64_t)t * stride != step) return fail("select", c, t);
      const int64_t pic = mobi_sink_picture(&sch, (uint32_t)c, t);
      if (pic + mobi_sink_picture_span(planar, chs, ow, oh) > span) return fail("picture span", pic, span);
      for (uint32_t ch = 0; ch < 3; ch++)
        for (uint32_t y = 0; y < oh; y++)
          for (uint32_t x = 0; x < ow; x++) {
            const int64_t a = pic + mobi_sink_element(planar, chs, ow, ch, y, x);
            if (a < 0 || a >= span) return fail("outside", a, span);
            if (seen[(size_t)a]++) return fail("twice", a, c);
            marked++;
          }
    }
  }
  if (marked != (long)n * T * 3 * ow * oh) return fail("count", marked, (long)n * T * 3 * ow * oh);
  // the last element of the tensor is the span's last
  if (!seen[(size_t)span - 1]) return fail("span not tight", span, 0);
  // what must be refused
  if (mobi_sink_layout_ok(planar, (uint32_t)n, T, ow, oh, cs + 2, fs, chs, (uint64_t)1 << 40, nullptr)) return fail("stride % 4", 0, 0);
  if (n > 1 && T > 1 && mobi_sink_layout_ok(planar, (uint32_t)n, T, ow, oh, cs, cs, chs, (uint64_t)1 << 40, nullptr)) return fail("equal strides", 0, 0);
  if (mobi_sink_layout_ok(planar, (uint32_t)n, T, ow, oh, INT64_MAX & ~3ll, fs, chs, UINT64_MAX, nullptr) && n > 1) return fail("overflow", 0, 0);
  printf("ok %ld\n", marked);
  return 0;
}
"""


def _layout_strides(layout, n, T, ow, oh, gap):
    plane = ow * oh
    planar = not layout.endswith("c")
    ext = {"n": n, "t": T, "c": 3}
    order = layout[:3] if planar else layout[:2]
    inner, st = (plane if planar else 3 * plane), {}
    for d in reversed(order):
        st[d] = inner + gap
        inner = st[d] * ext[d]
    return int(planar), st["n"], st["t"], st.get("c", 0)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def addr_tool(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("sink_addr_" + request.param)
    src, exe = d / "sink_addr.cpp", d / "sink_addr"
    src.write_text(_ADDR_CPP)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O1"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I" + CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("layout", ["ntchw", "ncthw", "nthwc", "tnchw", "tnhwc"])
@pytest.mark.parametrize("gap", [0, 8])
def test_every_element_address_of_the_sink_header(addr_tool, layout, gap):
    """(the element size scales every address alike: the three sizes are the three alignments of the check, test_sink_check_*)"""
    for n, T, s, ow, oh in ((5, 3, 2, 16, 12), (1, 1, 1, 4, 1), (3, 4, 3, 8, 5)):
        planar, cs, fs, chs = _layout_strides(layout, n, T, ow, oh, gap)
        r = subprocess.run([addr_tool] + [str(v) for v in (planar, n, T, s, ow, oh, cs, fs, chs)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok"), (layout, gap, n, T, r.stdout, r.stderr[-2000:])


def _bad_sink_kwargs():
    import torch
    ok = dict(size=(12, 16), n_frames=3)
    return [
        dict(ok, layout="nchw"), dict(ok, layout=None), dict(ok, layout="ntcwh"),
        dict(ok, out=torch.zeros((4, 3, 3, 12, 16), dtype=torch.uint8)[:, :2]),                      # wrong shape
        dict(ok, out=torch.zeros((4, 3, 12, 16, 3), dtype=torch.uint8)),                             # another layout's shape
        dict(ok, out=torch.zeros((4, 3, 3, 12, 16), dtype=torch.float32)),                           # wrong dtype
        dict(ok, out=torch.zeros((4, 3, 3, 12, 32), dtype=torch.uint8)[..., ::2]),                   # W not contiguous
        dict(ok, out=torch.zeros((4, 3, 3, 16, 12), dtype=torch.uint8).transpose(3, 4)),             # H, W swapped
        dict(ok, layout="nthwc", out=torch.zeros((4, 3, 12, 16, 4), dtype=torch.uint8)[..., :3]),    # packed pixels 4 apart
        dict(ok, start=[0, 1, 2]), dict(ok, start=[0, 1, 2, 3, 4]), dict(ok, start=[0, 1, 2, -1]), dict(ok, start=[0.0, 1, 2, 3]), dict(ok, start=7),
        dict(ok, start=[0, 0, 0, 2**31 - 2], stride=1),
        dict(size=(12, 16)), dict(size=(12, 16), n_frames=0), dict(ok, stride=0), dict(ok, stride=1.5), dict(n_frames=3), dict(size=(12, 18), n_frames=3),
        dict(ok, flip=[True] * 4), dict(ok, boxes=[(0, 0, 64, 48)] * 3), dict(ok, boxes=[(0, 0, 65, 48)] * 4),
        dict(ok, dtype=torch.int32), dict(ok, scale=(1, 1, 1)), dict(ok, dtype=torch.float16, bias=(0, 0)),
    ]


@pytest.mark.parametrize("k", range(27))
def test_set_sink_argument_errors_raise_value_error_before_any_library_call(k):
    kws = _bad_sink_kwargs()
    assert len(kws) == 27
    with pytest.raises(ValueError):
        _fake_batch().set_sink(**kws[k])
