"""Per-clip boxes, flips and upscaling in the tensor export (mobi_batch_export_device_boxes, include/mobiclip_hip.h;
mobi_export_resample.h / mobi_export_resample.hip; the exporter's parameter blocks, mobi_export.cpp; MobiclipBatch.export_tensor(boxes=, flip=,
size=)).

CPU: the header, the binding and the exported symbol; the runs, spans, tiles and the exact division of csrc/mobi_export_resample.h compiled
with g++ and walked against the definition; the definition itself (numpy, int64) against torch's float64 bilinear; argument errors.
GPU (-m gpu), bit-exact: the old scaled kernel where the two overlap, and numpy on the fmt="argb" tensor of the same slot -- Wy @ V @ Wx.T in
int64, (S + D // 2) // D, the flip, then the affine of test_export_device.py::_affine."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_export_device import (AFFINES, CSRC, MOBI_E_ARG, MOBI_E_NULLREF, PACKED, PLANAR, ROOT, F16, F32, U8, _affine, _bits, _busy, _fake_batch,
                                      _generated, _guard_batch, _old_six)
from tests.test_export_scaled import _CROPS_64x48, VARIANTS, _argb, _decoded, _sizes, _weights

I420, ARGB = 0, 1
FLIP_X = 1
# (in, out) per axis: linear (out > in), then area
AXES = [(4, 8), (7, 9), (22, 224), (1, 4), (2, 5), (45, 48), (61, 64), (192, 224), (64, 64), (61, 20), (640, 224), (640, 4), (5, 4)]
# both axes enlarging: (w, h, ow, oh)
ENLARGING = [(22, 30, 224, 224), (157, 133, 224, 224), (4, 7, 8, 9), (1, 1, 4, 3), (31, 17, 32, 18)]


# ---- the definition, in numpy ------------------------------------------------------------------------------------------------------
def _axis(out_n, in_n):
    """-> (W[out_n][in_n] int64, d)"""
    if out_n <= in_n:
        return _weights(out_n, in_n), in_n
    W = np.zeros((out_n, in_n), np.int64)
    for o in range(out_n):
        n = (2 * o + 1) * in_n - out_n
        i0 = n // (2 * out_n)  # floor
        f = n - i0 * 2 * out_n
        W[o, min(max(i0, 0), in_n - 1)] += 2 * out_n - f
        W[o, min(max(i0 + 1, 0), in_n - 1)] += f
    return W, 2 * out_n


def _sums(v, size):
    """(..., h, w) int64 -> S (..., oh, ow), D"""
    oh, ow = size
    Wy, dy = _axis(oh, v.shape[-2])
    Wx, dx = _axis(ow, v.shape[-1])
    assert (Wy.sum(axis=1) == dy).all() and (Wx.sum(axis=1) == dx).all()
    # (the products in float64, where BLAS does them: every partial sum is an integer below 255 * 2^23, so exact)
    S = Wy.astype(np.float64) @ v.astype(np.float64) @ Wx.T.astype(np.float64)
    assert S.max() <= 255 * dx * dy < 2 ** 53
    return S.astype(np.int64), dx * dy


def _model(bm, box, size, flip=False):
    """(..., H, W) uint32 Bitmaps -> (..., 3, oh, ow) uint8"""
    x, y, w, h = box
    v = np.stack([(bm >> s) & 0xFF for s in (16, 8, 0)], axis=-3).astype(np.int64)[..., y:y + h, x:x + w]
    S, D = _sums(v, size)
    q = (S + D // 2) // D
    assert q.min() >= 0 and q.max() <= 255
    return (q[..., ::-1] if flip else q).astype(np.uint8)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_boxes_export_and_the_library_exports_it():
    from mobiclipdecoder_amd import build, decoder
    text = open(os.path.join(ROOT, "include", "mobiclip_hip.h")).read()
    assert re.search(r"\bint mobi_batch_export_device_boxes\s*\(", text)
    assert re.search(r"#define MOBI_BOX_FLIP_X 1\b", text)
    res, args = decoder._SIGS["mobi_batch_export_device_boxes"]
    assert res is C.c_int and len(args) == 14 and args[4] == C.POINTER(C.c_int32) and args[5:11] == [C.c_int] * 6
    assert args[11:] == [C.c_void_p, C.c_size_t, C.c_void_p]
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], capture_output=True, text=True, check=True).stdout
    assert "mobi_batch_export_device_boxes" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    lib = decoder.load_library()
    buf = np.zeros(64, np.uint8)
    box = (C.c_int32 * 5)(0, 0, 4, 4, 0)
    assert lib.mobi_batch_export_device_boxes(None, PLANAR, U8, None, box, 4, 4, 0, 1, 0, 1, buf.ctypes.data, buf.nbytes, None) == MOBI_E_ARG


_GEOM_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mobi_export_resample.h"
// argv: in out.  The runs of the axis against the definition; the axis as the rows (and, where out is a multiple of 4, the columns) of the
// tilings of boxes of several sizes under one grid; the division by every D they have.
static int fail(const char *what, long a, long b, long c) { printf("FAIL %s %ld %ld %ld\n", what, a, b, c); return 1; }
static long clampl(long v, long lo, long hi) { return v < lo ? lo : v > hi ? hi : v; }
// W[o][s] of the definition
static std::vector<std::vector<long>> matrix(long out_n, long in_n, long *d) {
  std::vector<std::vector<long>> W(out_n, std::vector<long>(in_n, 0));
  for (long o = 0; o < out_n; o++) {
    if (out_n <= in_n) {
      for (long s = 0; s < in_n; s++) {
        const long hi = (s + 1) * out_n < (o + 1) * in_n ? (s + 1) * out_n : (o + 1) * in_n, lo = s * out_n > o * in_n ? s * out_n : o * in_n;
        W[o][s] = hi > lo ? hi - lo : 0;
      }
    } else {
      const long n = (2 * o + 1) * in_n - out_n;
      long i0 = n / (2 * out_n);
      if (n < 0 && i0 * 2 * out_n != n) i0--; // floor
      const long f = n - i0 * 2 * out_n;
      W[o][clampl(i0, 0, in_n - 1)] += 2 * out_n - f;
      W[o][clampl(i0 + 1, 0, in_n - 1)] += f;
    }
  }
  *d = out_n <= in_n ? in_n : 2 * out_n;
  return W;
}
static int axis(uint32_t out_n, uint32_t in_n) {
  long d;
  const auto W = matrix(out_n, in_n, &d);
  if ((long)mobi_axis_den(out_n, in_n) != d || (mobi_axis_kind(out_n, in_n) == MOBI_AXIS_LINEAR) != (out_n > in_n)) return fail("den", out_n, in_n, d);
  uint32_t last_first = 0, last_end = 0;
  for (uint32_t o = 0; o < out_n; o++) {
    const MobiAxisTap t = mobi_axis_tap(o, out_n, in_n);
    if (t.count < 1 || t.first + t.count > in_n) return fail("run range", o, t.first, t.count);
    if (out_n > in_n && t.count > 2) return fail("linear taps", o, t.count, 0);
    if (t.first < last_first || t.first + t.count < last_end) return fail("runs move right", o, t.first, t.count);
    last_first = t.first; last_end = t.first + t.count;
    long sum = 0;
    for (uint32_t s = 0; s < in_n; s++) {
      const bool in = s >= t.first && s < t.first + t.count;
      const long w = in ? (long)mobi_axis_tap_weight(&t, s - t.first) : 0;
      if (w != W[o][s]) return fail("weight", o, s, W[o][s]);
      if (in && w == 0) return fail("run not tight", o, s, 0);
      sum += w;
    }
    if (sum != d) return fail("row sum", o, sum, d);
  }
  // no n consecutive outputs have more sources than the bound the plan sizes its chunks with
  for (uint32_t n = 1; n <= out_n; n = n < 4 ? n + 1 : n * 2)
    for (uint32_t o0 = 0; o0 + n <= out_n; o0++) {
      uint32_t s0, s1;
      mobi_axis_span(o0, o0 + n, out_n, in_n, &s0, &s1);
      if (s1 - s0 > mobi_axis_span_max(n, out_n, in_n)) return fail("span bound", n, o0, s1 - s0);
    }
  return 0;
}
// outputs [o0, o1): their sources are inside [0, in_n), tight, and hold all the weight
static int span(uint32_t o0, uint32_t o1, uint32_t out_n, uint32_t in_n) {
  long d;
  const auto W = matrix(out_n, in_n, &d);
  uint32_t s0, s1;
  mobi_axis_span(o0, o1, out_n, in_n, &s0, &s1);
  if (s0 >= s1 || s1 > in_n) return fail("span range", o0, s0, s1);
  for (uint32_t s = 0; s < in_n; s++) {
    long w = 0;
    for (uint32_t o = o0; o < o1; o++) w += W[o][s];
    const bool inside = s >= s0 && s < s1;
    if (!inside && w) return fail("weight outside the span", o0, s, w);
    if ((s == s0 || s == s1 - 1) && !w) return fail("span not tight", o0, s, 0);
  }
  return 0;
}
static int division(uint64_t D, const MobiResampleClip &k) {
  const uint64_t up = (D + 1) / 2;
  const MobiScaleDiv dv = mobi_scale_div_make((uint32_t)D);
  if (dv.m != k.div.m || dv.sh != k.div.sh || k.half != D / 2) return fail("plan div", dv.m, dv.sh, 0);
  long checked = 0;
  for (uint64_t q = 0; q <= 255; q++)
    for (int e = -1; e <= 1; e++) {
      const int64_t S = (int64_t)(q * D) - (int64_t)up + e;
      if (S < 0 || (uint64_t)S > 255 * D) continue;
      const uint64_t n = (uint64_t)S + D / 2;
      if (n >> 31) return fail("sum range", q, e, 0);
      if (mobi_scale_div((uint32_t)n, dv) != n / D) return fail("division", q, e, (long)(n / D));
      checked++;
    }
  if (mobi_scale_div((uint32_t)(255 * D + D / 2), dv) != 255) return fail("division at 255 D", 0, 0, 0);
  if (checked < 255 * 3) return fail("division points", checked, 0, 0);
  return 0;
}
// boxes of the sizes ws x hs, all to ow x oh, under one grid
static int tilings(const std::vector<uint32_t> &ws, const std::vector<uint32_t> &hs, uint32_t ow, uint32_t oh, bool check_x, bool want_leave = false) {
  std::vector<MobiResampleClip> ks;
  uint32_t grid = 0, lds = 0;
  for (uint32_t w : ws)
    for (uint32_t h : hs) {
      if (mobi_resample_den(w, h, ow, oh) > (1u << 23)) return fail("D", w, h, 0);
      ks.push_back(mobi_resample_plan(3, 2, w, h, (uint32_t)ks.size() & 1u, ow, oh));
      const MobiResampleClip &k = ks.back();
      if (k.x != 3 || k.y != 2 || k.w != w || k.h != h || k.flags != ((ks.size() - 1) & 1u)) return fail("plan box", w, h, 0);
      if (k.strip_w % 4 || k.strip_w < 4 || k.strip_w > kMobiResampleStripMax || k.band_rows < 1) return fail("tile size", k.strip_w, k.band_rows, 0);
      if ((k.strip_w / 4) * k.band_rows > kMobiResampleLanes) return fail("owners", k.strip_w, k.band_rows, 0);
      if (k.chunk_rows < 2 || k.chunk_rows % 2 || k.chunk_cols < 4 || k.chunk_cols % 4) return fail("chunk", k.chunk_rows, k.chunk_cols, 0);
      if (mobi_resample_lds_bytes(&k) > kMobiResampleLdsBytes) return fail("lds", mobi_resample_lds_bytes(&k), 0, 0);
      if (mobi_resample_lds_bytes(&k) != 16 * k.strip_w + k.chunk_rows * (4 * k.chunk_cols + 12 * k.strip_w)) return fail("lds layout", 0, 0, 0);
      if (division(mobi_resample_den(w, h, ow, oh), k)) return 1;
      if (mobi_resample_blocks(&k) > grid) grid = mobi_resample_blocks(&k);
      if (mobi_resample_lds_bytes(&k) > lds) lds = mobi_resample_lds_bytes(&k);
    }
  bool some_leave = false;
  for (const MobiResampleClip &k : ks) {
    std::vector<int> cover(ow * oh, 0);
    for (uint32_t b = 0; b < grid + 2; b++) {
      uint32_t r0, r1, c0, c1;
      if (!mobi_resample_tile(&k, ow, oh, b, &r0, &r1, &c0, &c1)) {
        if (b < mobi_resample_blocks(&k)) return fail("tile missing", b, 0, 0);
        some_leave |= b < grid;
        continue;
      }
      if (b >= mobi_resample_blocks(&k)) return fail("tile past the tiling", b, 0, 0);
      if (r0 >= r1 || r1 > oh || r1 - r0 > k.band_rows || c0 >= c1 || c1 > ow || c1 - c0 > k.strip_w || (c0 | c1) % 4) return fail("tile", b, r0, c0);
      for (uint32_t r = r0; r < r1; r++)
        for (uint32_t c = c0; c < c1; c++) cover[r * ow + c]++;
      if (span(r0, r1, oh, k.h)) return 1;
      if (check_x && span(c0, c1, ow, k.w)) return 1;
    }
    for (uint32_t i = 0; i < ow * oh; i++)
      if (cover[i] != 1) return fail("covered", i / ow, i % ow, cover[i]);
  }
  if (want_leave && !some_leave) return fail("one tiling for every box", grid, 0, 0);
  return 0;
}
// The kernel's walk on the CPU, lane by lane in the kernel's order of steps, over a picture of W x H random bytes per channel: chunks, the
// column runs cut at chunk edges, the sums along x, the owners' row runs, the division, the flip -- against the definition's matrices.
static int walk(uint32_t W, uint32_t H, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t ow, uint32_t oh, uint32_t flags) {
  std::vector<uint32_t> pic(W * H);
  uint32_t seed = 12345u + W + 7u * w + 13u * ow;
  for (auto &p : pic) { seed = seed * 1664525u + 1013904223u; p = seed >> 8; }
  const MobiResampleClip k = mobi_resample_plan(x, y, w, h, flags, ow, oh);
  std::vector<uint32_t> lds(mobi_resample_lds_bytes(&k) / 4), got(3 * ow * oh, 0xFFFFFFFFu);
  uint32_t *coltap = lds.data(), *rgb = coltap + 4 * k.strip_w, *hs = rgb + k.chunk_rows * k.chunk_cols;
  for (uint32_t b = 0; b < mobi_resample_blocks(&k); b++) {
    uint32_t r0, r1, c0, c1;
    if (!mobi_resample_tile(&k, ow, oh, b, &r0, &r1, &c0, &c1)) return fail("walk tile", b, 0, 0);
    const uint32_t rows = r1 - r0, sw = c1 - c0, nq = sw / 4;
    for (uint32_t i = 0; i < sw; i++) {
      const MobiAxisTap t = mobi_axis_tap(c0 + i, ow, k.w);
      coltap[4 * i] = t.first; coltap[4 * i + 1] = t.count; coltap[4 * i + 2] = t.wf; coltap[4 * i + 3] = t.wl;
    }
    if (rows * nq > kMobiResampleLanes) return fail("walk owners", rows, nq, 0);
    std::vector<uint32_t> acc(rows * nq * 12, 0);
    uint32_t t0, t1, s0, s1;
    mobi_axis_span(r0, r1, oh, k.h, &t0, &t1);
    mobi_axis_span(c0, c1, ow, k.w, &s0, &s1);
    const uint32_t py0 = (k.y + t0) & ~1u, py1 = (k.y + t1 + 1u) & ~1u, px0 = (k.x + s0) & ~3u, px1 = (k.x + s1 + 3u) & ~3u;
    if (py1 > H || px1 > W) return fail("walk span outside the picture", py1, px1, 0);
    for (uint32_t ra = py0; ra < py1; ra += k.chunk_rows) {
      const uint32_t rb = ra + k.chunk_rows < py1 ? ra + k.chunk_rows : py1, nrows = rb - ra;
      for (uint32_t ca = px0; ca < px1; ca += k.chunk_cols) {
        const uint32_t cb = ca + k.chunk_cols < px1 ? ca + k.chunk_cols : px1;
        for (uint32_t r = 0; r < k.chunk_rows; r++)
          for (uint32_t c = 0; c < k.chunk_cols; c++) rgb[r * k.chunk_cols + c] = 0xDEADBEEFu; // (what the chunk does not fill is never read)
        for (uint32_t r = ra; r < rb; r++)
          for (uint32_t c = ca; c < cb; c++) rgb[(r - ra) * k.chunk_cols + (c - ca)] = pic[r * W + c];
        for (uint32_t row = 0; row < nrows; row++)
          for (uint32_t col = 0; col < sw; col++) {
            const uint32_t *t = coltap + 4 * col, base = k.x + t[0];
            const uint32_t ka = base < ca ? ca - base : 0u, kb = cb > base ? (cb - base < t[1] ? cb - base : t[1]) : 0u;
            uint32_t s[3] = {0, 0, 0};
            for (uint32_t kk = ka; kk < kb; kk++) {
              const uint32_t wt = kk == 0u ? t[2] : kk + 1u == t[1] ? t[3] : ow, word = rgb[row * k.chunk_cols + base + kk - ca];
              if (word == 0xDEADBEEFu) return fail("walk read of an unfilled word", row, col, kk);
              for (int ch = 0; ch < 3; ch++) s[ch] += wt * ((word >> (16 - 8 * ch)) & 0xFFu);
            }
            for (int ch = 0; ch < 3; ch++) {
              uint32_t *hp = hs + (row * 3 + ch) * k.strip_w + col;
              *hp = ca == px0 ? s[ch] : *hp + s[ch];
            }
          }
        if (ca + k.chunk_cols < px1) continue;
        for (uint32_t tid = 0; tid < rows * nq; tid++) {
          const uint32_t orow = tid / nq, q4 = (tid - orow * nq) * 4;
          const MobiAxisTap rt = mobi_axis_tap(r0 + orow, oh, k.h);
          const uint32_t base = k.y + rt.first;
          const uint32_t ka = base < ra ? ra - base : 0u, kb = rb > base ? (rb - base < rt.count ? rb - base : rt.count) : 0u;
          for (uint32_t kk = ka; kk < kb; kk++) {
            const uint32_t wt = kk == 0u ? rt.wf : kk + 1u == rt.count ? rt.wl : oh;
            for (int ch = 0; ch < 3; ch++)
              for (int t = 0; t < 4; t++) acc[tid * 12 + ch * 4 + t] += wt * hs[((base + kk - ra) * 3 + ch) * k.strip_w + q4 + t];
          }
        }
      }
    }
    for (uint32_t tid = 0; tid < rows * nq; tid++) {
      const uint32_t orow = tid / nq, q4 = (tid - orow * nq) * 4, col = (flags & MOBI_RESAMPLE_FLIP_X) ? ow - 4 - (c0 + q4) : c0 + q4;
      for (int ch = 0; ch < 3; ch++)
        for (int t = 0; t < 4; t++) {
          const uint32_t a = (flags & MOBI_RESAMPLE_FLIP_X) ? acc[tid * 12 + ch * 4 + 3 - t] : acc[tid * 12 + ch * 4 + t];
          uint32_t &g = got[(ch * oh + r0 + orow) * ow + col + t];
          if (g != 0xFFFFFFFFu) return fail("walk output written twice", ch, r0 + orow, col + t);
          g = mobi_scale_div(a + k.half, k.div);
        }
    }
  }
  long dx, dy;
  const auto Wx = matrix(ow, w, &dx), Wy = matrix(oh, h, &dy);
  for (int ch = 0; ch < 3; ch++)
    for (uint32_t oy = 0; oy < oh; oy++)
      for (uint32_t ox = 0; ox < ow; ox++) {
        long S = 0;
        for (uint32_t t = 0; t < h; t++) {
          if (!Wy[oy][t]) continue;
          long hsum = 0;
          for (uint32_t s = 0; s < w; s++) hsum += Wx[ox][s] * (long)((pic[(y + t) * W + x + s] >> (16 - 8 * ch)) & 0xFFu);
          S += Wy[oy][t] * hsum;
        }
        const long want = (S + dx * dy / 2) / (dx * dy);
        const uint32_t at = (flags & MOBI_RESAMPLE_FLIP_X) ? ow - 1 - ox : ox;
        if ((long)got[(ch * oh + oy) * ow + at] != want) return fail("walk value", ch, oy, ox);
      }
  return 0;
}
int main(int argc, char **argv) {
  if (argc == 11 && argv[1][0] == 'w') {
    if (walk(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]), atoi(argv[9]), atoi(argv[10]))) return 1;
    printf("ok\n");
    return 0;
  }
  if (argc == 2 && argv[1][0] == 'e') { // the example DESIGN.md works through: the centre 480 x 480 of 640 x 480 to 224 x 224
    const MobiResampleClip k = mobi_resample_plan(80, 0, 480, 480, 0, 224, 224);
    printf("%u %u %u %u %u %u %u\n", k.n_strips, k.strip_w, k.n_bands, k.band_rows, k.chunk_rows, k.chunk_cols, mobi_resample_lds_bytes(&k));
    return 0;
  }
  if (argc != 3) return 2;
  const uint32_t in_n = atoi(argv[1]), out_n = atoi(argv[2]);
  if (axis(out_n, in_n)) return 1;
  if (sizeof(MobiResampleClip) != 64) return fail("record size", sizeof(MobiResampleClip), 0, 0);
  // the axis as the rows: boxes 640, 157, 22 and 4 wide to 224 columns
  if (tilings({640, 157, 22, 4}, {in_n}, 224, out_n, true)) return 1;
  if (tilings({640, 40}, {in_n}, 4, out_n, true)) return 1;
  // ... and as the columns: boxes 480, 133, 30 and 1 high to 224 rows (and to 3)
  if (out_n % 4 == 0) {
    if (tilings({in_n}, {480, 133, 30, 1}, out_n, 224, true)) return 1;
    if (tilings({in_n}, {480, 7}, out_n, 3, true)) return 1;
  }
  // a large and a small box to 4 x 4: the large one is cut into more workgroups, and the small one's extra workgroups leave
  if (tilings({640, 64}, {480, 48}, 4, 4, true, true)) return 1;
  printf("ok\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def geom_tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("export_resample_geom")
    src, exe = d / "geom.cpp", d / "geom"
    src.write_text(_GEOM_CPP)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("in_n,out_n", AXES)
def test_runs_spans_tiles_and_division_of_the_resample_header(geom_tool, in_n, out_n):
    """the code the kernel runs (mobi_export_resample.h), on the CPU: an output's run of sources and its first / middle / last weight equal
    the definition's W[o][s] for every (o, s), rows sum to d, a linear output has at most 2 taps; with the axis as rows and as columns of
    boxes of several sizes under one grid: the tiles of every clip cover every output once, workgroups past a clip's tiling leave, the LDS
    stays inside the budget, a tile's source span lies inside the box, is tight and holds all of the tile's weight; the multiply-and-shift
    division equals (S + D / 2) // D at every S where the quotient changes, one to either side, and at 255 D, for every D of those boxes"""
    r = subprocess.run([geom_tool, str(in_n), str(out_n)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


# picture W, H; box x, y, w, h; output ow, oh; flags
WALKS = [(640, 480, 80, 0, 480, 480, 224, 224, 0), (640, 480, 0, 0, 640, 480, 4, 4, 1), (640, 480, 17, 9, 100, 60, 224, 224, 1),
         (256, 192, 0, 0, 256, 192, 224, 224, 0), (256, 192, 33, 1, 222, 190, 64, 48, 1), (256, 192, 17, 9, 20, 30, 64, 48, 0),
         (64, 48, 63, 47, 1, 1, 64, 48, 1), (64, 48, 3, 5, 21, 13, 36, 33, 1), (528, 48, 0, 0, 528, 48, 132, 7, 0), (4096, 16, 1, 0, 4095, 16, 4, 3, 0),
         (4096, 16, 3, 1, 4000, 2, 8, 40, 1)]


@pytest.mark.parametrize("k", range(len(WALKS)))
def test_the_kernels_walk_on_the_cpu(geom_tool, k):
    """the chunk loops, the cut of a column run at a chunk's edge, the sums along x, the owners' row runs, the division and the flip, in the
    kernel's order of steps with the header's functions, against the definition: 4095 -> 4 needs several column chunks per row chunk,
    640x480 -> 4x4 thirty row chunks; no word of LDS is read that its chunk did not fill, and every output is written once"""
    r = subprocess.run([geom_tool, "walk"] + [str(v) for v in WALKS[k]], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def test_the_tiling_example_of_the_design_document(geom_tool):
    """DESIGN.md, "Resampled export": 480x480 -> 224x224 is 4 strips of 56 columns x 13 bands of 18 rows, chunks of 16 rows x 124 columns in
    19 584 bytes of LDS (19.1 KiB); a band's 18 rows have at most 40 source rows, 42 as whole row pairs: three chunks"""
    r = subprocess.run([geom_tool, "example"], capture_output=True, text=True)
    assert r.returncode == 0 and [int(v) for v in r.stdout.split()] == [4, 56, 13, 18, 16, 124, 19584], r.stdout


@pytest.mark.parametrize("w,h,ow,oh", ENLARGING)
def test_the_linear_rule_is_torch_bilinear(w, h, ow, oh):
    """S / D of the integer definition against torch.nn.functional.interpolate(mode="bilinear", align_corners=False) in float64"""
    import torch
    v = np.random.default_rng(w * 1000 + h).integers(0, 256, (3, h, w)).astype(np.int64)
    S, D = _sums(v, (oh, ow))
    ref = torch.nn.functional.interpolate(torch.from_numpy(v)[None].double(), size=(oh, ow), mode="bilinear", align_corners=False)[0].numpy()
    err = np.abs(S / D - ref).max()
    assert err < 1e-6, err


@pytest.mark.parametrize("w,h", [(64, 48), (4, 7), (1, 1), (61, 45)])
def test_a_box_at_its_own_size_is_a_pure_crop(w, h):
    bm = np.random.default_rng(w).integers(0, 1 << 32, (2, 48, 64), dtype=np.uint64).astype(np.uint32)
    x, y = 64 - w, 48 - h
    want = np.stack([(bm >> s) & 0xFF for s in (16, 8, 0)], axis=-3)[..., y:y + h, x:x + w].astype(np.uint8)
    assert np.array_equal(_model(bm, (x, y, w, h), (h, w)), want)
    assert np.array_equal(_model(bm, (x, y, w, h), (h, w), True), want[..., ::-1])


_ONE = [[0, 0, 64, 48]] * 4
_BAD = [
    dict(boxes=[[0, 0, 64, 48]] * 3), dict(boxes=[0, 0, 64, 48]), dict(boxes=[[0, 0, 64]] * 4), dict(boxes=np.zeros((4, 4), np.float32) + 4),
    dict(boxes=[[0, 0, 8.0, 8]] * 4), dict(boxes=np.ones((4, 4), bool)), dict(boxes="abcd"), dict(boxes=[[0, 0, 8, 8, 0]] * 4),     # shape / dtype
    dict(boxes=_ONE, flip=[True] * 3), dict(boxes=_ONE, flip=[0, 1, 0, 1]), dict(boxes=_ONE, flip=True), dict(boxes=_ONE, flip=[[True] * 4]),
    dict(boxes=_ONE, flip=np.zeros(4, np.float32)), dict(flip=[True] * 4),
    dict(boxes=[[0, 0, 64, 48]] * 3 + [[1, 0, 64, 48]]), dict(boxes=[[0, 1, 64, 48]] + [[0, 0, 64, 48]] * 3), dict(boxes=[[-1, 0, 4, 4]] * 4),
    dict(boxes=[[0, -1, 4, 4]] * 4), dict(boxes=[[0, 0, 0, 4]] * 4), dict(boxes=[[0, 0, 4, 0]] * 4), dict(boxes=[[60, 0, 8, 8]] * 4),
    dict(boxes=[[0, 0, 4, -4]] * 4), dict(boxes=[[0, 0, 1 << 40, 4]] * 4),                                                  # outside / empty
    dict(boxes=_ONE, crop=(0, 0, 64, 48)), dict(boxes=_ONE, size=None), dict(boxes=_ONE, size=(48, 62)), dict(boxes=_ONE, size=(48, 1)),
    dict(boxes=_ONE, size=(0, 64)), dict(boxes=_ONE, size=(48, 0)), dict(boxes=_ONE, size=(48,)), dict(boxes=_ONE, size=(48.0, 64)),
    dict(boxes=_ONE, size=(True, 64)), dict(boxes=_ONE, fmt="i420"), dict(boxes=_ONE, fmt="argb"),
    dict(boxes=[[0, 0, 8, 8]] * 4, size=(1028, 2048)), dict(boxes=[[0, 0, 8, 8]] * 3 + [[0, 0, 64, 1]], size=(66000, 64)),   # D > 2^23
]


@pytest.mark.parametrize("k", range(len(_BAD)))
def test_export_tensor_boxes_errors_raise_value_error_before_any_library_call(k):
    b = _fake_batch()  # 4 clips of 64x48; any library call raises AssertionError
    kw = dict(size=(48, 64))
    kw.update(_BAD[k])
    with pytest.raises(ValueError):
        b.export_tensor(**kw)


def test_the_crop_path_keeps_its_refusals():
    b = _fake_batch()
    for kw in (dict(size=(49, 64)), dict(crop=(0, 0, 32, 32), size=(33, 32)), dict(crop=(0, 0, 8, 8), size=(8, 12))):  # no upscaling without boxes
        with pytest.raises(ValueError):
            b.export_tensor(**kw)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _tdt(name):
    import torch
    return getattr(torch, name)


def _export(b, boxes, flips, size, layout, dt, aff, ring_idx=0, nf=1, clips=None, stream=None):
    sb = AFFINES[aff]
    kw = {} if sb is None or dt == "uint8" else dict(scale=sb[0].tolist(), bias=sb[1].tolist())
    return b.export_tensor("rgb", ring_idx, nf, clips, layout=layout, dtype=_tdt(dt), boxes=boxes, flip=flips, size=size, stream=stream, **kw)


def _want(bm, boxes, flips, size, layout, dt, aff):
    """bm (F, N, H, W) -> the tensor's array"""
    flips = [False] * len(boxes) if flips is None else flips
    q = np.stack([_model(bm[:, c], boxes[c], size, bool(flips[c])) for c in range(len(boxes))], axis=1)  # (F, N, 3, oh, ow)
    if layout == "nhwc":
        q = np.moveaxis(q, -3, -1)
    return q if dt == "uint8" else _affine(q, layout, AFFINES[aff], {"float16": np.float16, "float32": np.float32}[dt])


def _same(got, want, what):
    g = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert g.dtype == want.dtype and g.shape == want.shape, (g.dtype, g.shape, want.dtype, want.shape)
    if not np.array_equal(_bits(g), _bits(want)):
        bad = np.argwhere(_bits(g) != _bits(want))
        raise AssertionError((what, len(bad), bad[:4].tolist(), g[tuple(bad[0])], want[tuple(bad[0])]))


def _check(b, bm, boxes, flips, size, layout, dt, aff, ring_idx=0, nf=1, clips=None, stream=None):
    got = _export(b, boxes, flips, size, layout, dt, aff, ring_idx, nf, clips, stream)
    _same(got, _want(bm, boxes, flips, size, layout, dt, aff), (boxes, flips, size, layout, dt, aff))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mods_64x48_rich", "moflex_64x48_rich_iint", "moflex_528x48_edge_pad", "moflex_640x480_B"])
def test_the_scaled_kernel_is_the_oracle_where_both_axes_shrink(name):
    """the same box for every clip, no flip: byte for byte export_tensor(crop=, size=), in every layout x dtype x affine.  640x480 -> 4x4 is
    many chunks of source rows per workgroup; 528 -> 132 x 7 three strips"""
    b = _decoded(name, n=2, frames=2)
    cases = {"moflex_528x48_edge_pad": [((0, 0, 528, 48), (7, 132))], "moflex_640x480_B": [((0, 0, 640, 480), (4, 4))]}.get(name)
    if cases is None:
        cases = [(crop, size) for crop in _CROPS_64x48 for size in _sizes(crop[2], crop[3])]
    for crop, size in cases:
        for layout, dt, aff in VARIANTS:
            sb = AFFINES[aff]
            kw = {} if sb is None or dt == "uint8" else dict(scale=sb[0].tolist(), bias=sb[1].tolist())
            old = b.export_tensor("rgb", layout=layout, dtype=_tdt(dt), crop=crop, size=size, **kw)
            new = _export(b, [list(crop)] * 2, None, size, layout, dt, aff)
            _same(new, old.cpu().numpy(), (crop, size, layout, dt, aff))
    b.close()


@pytest.mark.gpu
def test_per_clip_boxes_in_one_call():
    """3 different clips x 4 frames: a box shrinking on both axes, one enlarging on both, one mixed; flips off, on, on; then clips 1..2"""
    from mobiclipdecoder_amd import MobiclipBatch
    streams = [_generated("A", 900 + c, 4) for c in range(3)]
    p = streams[0][0]
    b = MobiclipBatch(3, p.width, p.height, p.version)
    for f in range(4):
        rcs, _ = b.decode([streams[c][1][f][0] for c in range(3)], [0] * 3)
        assert rcs == [0] * 3
    assert (p.width, p.height) == (256, 192)
    boxes, flips, size = [(33, 1, 222, 190), (17, 9, 20, 30), (0, 0, 256, 40)], [False, True, True], (48, 64)
    bm = _argb(b, 3, 4)
    assert not np.array_equal(bm[0], bm[1]) and not np.array_equal(bm[:, 0], bm[:, 1])  # (frames and clips do differ)
    for layout, dt, aff in (("nchw", "uint8", "unit"), ("nhwc", "float16", "imagenet")):
        _check(b, bm, boxes, flips, size, layout, dt, aff, 3, 4)
        _check(b, bm[:, 1:], boxes[1:], flips[1:], size, layout, dt, aff, 3, 4, range(1, 3))
    _check(b, bm[2:, 1:], boxes[1:], None, size, "nchw", "float32", "imagenet", 1, 2, range(1, 3))
    b.close()


def _edge_boxes(W, H):
    return [(W - 20, H - 30, 20, 30), (W - 21, H - 31, 20, 30),      # ending on the last row and column; one short of them
            (3, 5, 21, 13), (1, 1, 30, 30),                           # odd origins
            (7, 9, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, 1, 1),         # 1 x 1
            (13, 9, 4, 7), (1, 17, 30, 1), (W - 2, 0, 2, 19),         # 4 wide, 1 high, 2 wide on the last column
            (6, 6, 12, 12), (10, 10, 20, 20), (15, 7, 2, 2)]          # across macroblock (16) and quadrant (8) boundaries


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mods_64x48_rich", "moflex_64x48_rich_iint", "r05_far_mv_moflex_32x32", "moflex_528x48_edge_pad"])
def test_edges_enlarged(name):
    b0 = _decoded(name, n=1, frames=1)
    boxes = _edge_boxes(b0.Width, b0.Height)
    assert all(x >= 0 and y >= 0 and x + w <= b0.Width and y + h <= b0.Height and w < 64 and h < 48 for x, y, w, h in boxes)
    b0.close()
    b = _decoded(name, n=len(boxes), frames=2)
    bm = _argb(b)
    flips = [bool(i & 1) for i in range(len(boxes))]
    _check(b, bm, boxes, None, (48, 64), "nchw", "uint8", "unit")
    _check(b, bm, boxes, flips, (48, 64), "nhwc", "float32", "imagenet")
    _check(b, bm, boxes, flips, (33, 36), "nhwc", "float16", "unit")  # (odd height, out_w no multiple of 8)
    b.close()


@pytest.mark.gpu
def test_flip_is_torch_flip():
    import torch
    b = _decoded("mods_64x48_rich", n=3, frames=2)
    boxes = [(3, 2, 61, 45), (13, 5, 22, 30), (0, 0, 64, 20)]
    for layout, axis in (("nchw", 4), ("nhwc", 3)):
        for dt, aff in (("uint8", "unit"), ("float16", "imagenet")):
            plain = _export(b, boxes, None, (24, 40), layout, dt, aff)
            flipped = _export(b, boxes, [True] * 3, (24, 40), layout, dt, aff)
            mixed = _export(b, boxes, [False, True, False], (24, 40), layout, dt, aff)
            assert torch.equal(flipped, torch.flip(plain, (axis,)))
            assert torch.equal(mixed[:, 0], plain[:, 0]) and torch.equal(mixed[:, 1], flipped[:, 1]) and torch.equal(mixed[:, 2], plain[:, 2])
            assert not torch.equal(flipped, plain)
    b.close()


@pytest.mark.gpu
def test_the_second_format_at_224():
    """a ModsDS picture is 256 x 192: 224 x 224 shrinks it along x and enlarges it along y"""
    b = _decoded("mods_256x192_A", n=2, frames=2)
    bm = _argb(b)
    for layout, dt, aff in VARIANTS:
        _check(b, bm, [(0, 0, 256, 192)] * 2, [False, True], (224, 224), layout, dt, aff)
    b.close()


def _loader_boxes(W, H):
    """boxes of 8, 25, 60 and 100 % of the area at 3:4 and 4:3, cut to the picture where they do not fit (100 % at 3:4 is H x H)"""
    out = []
    for i, frac in enumerate((0.08, 0.25, 0.60, 1.0)):
        for ar in (3 / 4, 4 / 3):
            a = frac * W * H
            w, h = min(W, int(round((a * ar) ** 0.5))), min(H, int(round((a / ar) ** 0.5)))
            out.append(((W - w) * (i + 1) // 5, (H - h) * (4 - i) // 5, w, h))
    return out


@pytest.mark.gpu
def test_random_resized_crop_shapes_at_640x480():
    b = _decoded("moflex_640x480_B", n=8, frames=2)
    boxes = _loader_boxes(640, 480)
    assert [bx[2:] for bx in boxes[-2:]] == [(480, 480), (640, 480)] and min(w * h for _, _, w, h in boxes) < 224 * 224 < max(w * h for _, _, w, h in boxes)
    flips = [bool(i % 3 == 0) for i in range(8)]
    bm = _argb(b)
    for layout, dt, aff in VARIANTS:
        _check(b, bm, boxes, flips, (224, 224), layout, dt, aff)
    b.close()


@pytest.mark.gpu
def test_parameter_blocks_are_not_reused_early():
    """two exports with different boxes enqueued back to back behind a busy stream, no host sync between them: each kernel must find its own
    records when it runs at last; a third after a synchronize takes a block that is free again"""
    import torch
    b = _decoded("mods_64x48_rich", n=4, frames=2)
    dev = torch.device("cuda", b.device)
    bm = _argb(b)
    sets = [([(0, 0, 64, 48), (3, 2, 20, 30), (13, 5, 22, 30), (60, 41, 4, 7)], [False, True, False, True]),
            ([(17, 9, 4, 7), (0, 0, 64, 48), (1, 1, 62, 46), (7, 15, 12, 2)], [True, True, False, False]),
            ([(5, 5, 50, 40), (7, 9, 1, 1), (0, 0, 33, 48), (3, 3, 61, 45)], [False, False, True, True])]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    keep = _busy(side, dev, 100)
    got = [_export(b, bx, fl, (48, 64), "nchw", "uint8", "unit", stream=side) for bx, fl in sets[:2]]
    torch.cuda.synchronize()
    got.append(_export(b, sets[2][0], sets[2][1], (48, 64), "nchw", "uint8", "unit", stream=side))
    side.synchronize()
    for g, (bx, fl) in zip(got, sets):
        _same(g, _want(bm, bx, fl, (48, 64), "nchw", "uint8", "unit"), bx)
    del keep
    b.close()


@pytest.mark.gpu
def test_boxes_export_refusals_enqueue_nothing():
    import torch
    from mobiclipdecoder_amd import MobiclipBatch
    p, fr = _generated("B", 31, 3)
    n = 2
    b = MobiclipBatch(n, p.width, p.height, p.version, device_parse=True)
    assert (p.width, p.height) == (640, 480)
    lib, h = b._lib, b._h
    dev = torch.device("cuda", b.device)
    W, H = p.width, p.height
    out = torch.full((4 * n * 3 * 224 * 224 + 64,), 0xAB, dtype=torch.uint8, device=dev)
    ptr, nb = out.data_ptr(), out.numel()
    stream = torch.cuda.current_stream(dev).cuda_stream
    sb = (C.c_float * 6)(1, 1, 1, 0, 0, 0)
    good = [(80, 0, 480, 480, 0), (17, 9, 100, 60, FLIP_X)]

    def ex(fmt=PLANAR, dt=U8, boxes=good, size=(224, 224), r=0, nf=1, c0=0, nc=n, d=ptr, nbytes=nb, s=None, box1=None):  # size = (out_w, out_h)
        rows = [tuple(r_) for r_ in boxes]
        if box1 is not None:
            rows[-1] = box1
        arr = None if boxes is None else (C.c_int32 * (5 * len(rows)))(*[v for r_ in rows for v in r_])
        return lib.mobi_batch_export_device_boxes(h, fmt, dt, s, arr, size[0], size[1], r, nf, c0, nc, d, nbytes, stream)
    assert ex() == MOBI_E_NULLREF
    b.decode([fr[0][0]] * n, [0] * n)
    assert ex(r=1) == MOBI_E_NULLREF
    pic = 3 * 224 * 224
    refused = [
        ex(fmt=I420), ex(fmt=ARGB), ex(fmt=4), ex(fmt=-1),                                                                # not RGB
        lib.mobi_batch_export_device_boxes(h, PLANAR, U8, None, None, 224, 224, 0, 1, 0, n, ptr, nb, stream),             # boxes == NULL
        ex(box1=(161, 0, 480, 480, 0)), ex(box1=(0, 1, 480, 480, 0)), ex(box1=(-1, 0, 480, 480, 0)), ex(box1=(0, -1, 480, 480, 0)),  # not inside
        ex(box1=(0, 0, 0, 480, 0)), ex(box1=(0, 0, 480, 0, 0)), ex(box1=(0, 0, -4, 480, 0)), ex(box1=(0, 0, W + 1, H, 0)),  # empty / too large
        ex(box1=(0x7FFFFFF0, 0, 480, 480, 0)), ex(box1=(0, 0, 0x7FFFFFFF, 480, 0)),
        ex(box1=(0, 0, 64, 64, 2)), ex(box1=(0, 0, 64, 64, 3)), ex(box1=(0, 0, 64, 64, -1)), ex(box1=(0, 0, 64, 64, 0x100)),  # unknown flag bits
        ex(size=(0, 224)), ex(size=(224, 0)), ex(size=(-4, 224)),                                                         # below 1
        ex(size=(222, 224)), ex(size=(1, 224)), ex(size=(61, 45)),                                                        # out_w % 4
        ex(boxes=[(0, 0, 100, 480, 0), (0, 0, 640, 1, 0)], size=(4, 16384)), ex(box1=(0, 0, 640, 480, 0), size=(8, 8192)),  # D > 2^23 in one clip
        ex(dt=U8, s=sb), ex(dt=3), ex(dt=-1),                                                                             # dtype / scale_bias
        ex(d=ptr + 4), ex(nbytes=n * pic - 1), ex(dt=F16, nbytes=2 * n * pic - 1), ex(dt=F32, nbytes=4 * n * pic - 1),     # dst
        ex(r=6), ex(r=-1), ex(nf=2), ex(nf=0), ex(c0=-1, nc=1), ex(nc=n + 1), ex(c0=n, nc=1), ex(nc=0),                   # ring / clips
        lib.mobi_batch_export_device_boxes(h, PLANAR, U8, None, (C.c_int32 * 10)(*[v for r_ in good for v in r_]), 224, 224, 0, 1, 0, n, None, nb, stream),
    ]
    assert refused == [MOBI_E_ARG] * len(refused), refused
    b.submit([fr[1][0]] * n, [0] * n)  # ring index 0 is a step in flight
    assert ex() == MOBI_E_ARG
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())  # nothing was written
    b.wait()
    # the same buffer is accepted once the request is right
    assert ex() == 0
    t = b.export_tensor("rgb", boxes=[g[:4] for g in good], flip=[False, True], size=(224, 224))
    torch.cuda.synchronize()
    assert np.array_equal(out[:n * pic].cpu().numpy().reshape(t.shape), t.cpu().numpy())
    assert bool((out[n * pic:] == 0xAB).all())
    _same(t, _want(_argb(b), [g[:4] for g in good], [False, True], (224, 224), "nchw", "uint8", "unit"), "accepted")
    b.close()


def _varied_boxes(n, W, H, seed):
    """n boxes of 8 - 100 % of the area, and flips"""
    rng = np.random.default_rng(seed)
    boxes = []
    for _ in range(n):
        a, ar = rng.uniform(0.08, 1.0) * W * H, np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
        w, h = min(W, int(round((a * ar) ** 0.5))), min(H, int(round((a / ar) ** 0.5)))
        boxes.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return boxes, [bool(v) for v in rng.integers(0, 2, n)]


@pytest.mark.gpu
def test_boxes_export_is_ordered_on_the_stream_without_a_host_sync():
    """a torch reduction enqueued on the export's stream right behind it, a side stream held busy first, sees the pictures"""
    import torch
    from mobiclipdecoder_amd import MobiclipBatch
    p, fr = _generated("B", 21, 2)
    n = 32
    b = MobiclipBatch(n, p.width, p.height, p.version)
    for f in range(2):
        b.decode([fr[f][0]] * n, [0] * n)
    size = (224, 224)
    boxes, flips = _varied_boxes(8, p.width, p.height, 5)
    boxes, flips = boxes * 4, flips * 2 + [not f for f in flips] * 2
    one = _argb(b, 1, 2, range(0, 1))  # (every clip decodes the same stream)
    sums8 = [_model(one[:, 0], boxes[c], size).astype(np.int64).sum(axis=(2, 3)) for c in range(8)]
    want = np.stack([sums8[c % 8] for c in range(n)], axis=1)  # (F, n, 3); a flip keeps the sum
    dev = torch.device("cuda", b.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        a = torch.randn(4096, 4096, device=dev)
        for _ in range(10):
            a = a @ a / 64.0
        out = b.export_tensor("rgb", 1, 2, dtype=torch.float32, stream=side, boxes=boxes, flip=flips, size=size)
        sums = out.double().sum(dim=(3, 4))
    side.synchronize()
    assert np.array_equal(sums.cpu().numpy().astype(np.int64), want)
    b.close()


@pytest.mark.gpu
def test_slot_guard_holds_replayed_steps_behind_a_boxes_export_on_a_busy_stream():
    """test_export_scaled.py's guard test with per-clip boxes: the export sits behind a few hundred milliseconds of work on a side stream,
    six steps that write every exported slot are enqueued at once, and the tensor holds the old frames"""
    import torch
    b, p, streams = _guard_batch(760)
    dev = torch.device("cuda", b.device)
    side = torch.cuda.Stream(device=dev)
    keep = _busy(side, dev)
    size = (224, 224)
    boxes, flips = _varied_boxes(4, p.width, p.height, 9)
    boxes, flips = [boxes[(c // 2) % 4] for c in range(16)], [flips[c % 4] ^ (c >= 8) for c in range(16)]  # (box and source vary independently)
    out = b.export_tensor("rgb", 5, 6, range(0, 16), layout="nhwc", stream=side, boxes=boxes, flip=flips, size=size)
    for f in range(6, 12):  # six steps enqueued at once, each writing a slot the export has not read yet
        b.replay(f)
    assert b.sync() == 0
    torch.cuda.synchronize()
    old = _old_six(streams, p)  # [source][frame] -> (H, W) uint32, the oracle's Bitmaps
    got = out.cpu().numpy()
    m = len(old)
    models = {}
    for c in range(got.shape[1]):
        key = (c % m, boxes[c])
        if key not in models:
            models[key] = _model(np.stack(old[c % m]), boxes[c], size)  # (6, 3, oh, ow)
        for f in range(6):
            q = models[key][f][..., ::-1] if flips[c] else models[key][f]
            assert np.array_equal(got[f, c], np.moveaxis(q, 0, -1)), (c, f)
    new = b.export_tensor("rgb", 0, 1, range(0, 1), layout="nhwc", boxes=boxes[:1], flip=flips[:1], size=size)
    assert not np.array_equal(new.cpu().numpy()[0, 0], got[5, 0])  # (the ring did move on)
    del keep
    b.close()
