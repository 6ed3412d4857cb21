"""CPU: the hand-written oracle against the mechanical C#->C++ transliteration of the reference (oracle/tools/cs2cpp.py ->
oracle/_ref/libmobi_csref.so).  Bit-exact planes, Offset, Quantizer, and agreement on which frames throw -- on valid streams of every
configuration and on randomly corrupted ones.

The transliteration's results for every case below are recorded in tests/golden/csref_records.npz (tests/golden/make_csref_records.py):
one row per frame (throws, Offset, Quantizer, a 64-bit digest of the Y and UV planes of every ring slot), one row per trial of the unit
sweep.  The oracle is checked against that record everywhere; where the library exists (it can only be generated beside the reference
sources), its results are computed as well and must equal the record."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from mobiclipdecoder_amd import default_params, generate_clip
from mobiclipdecoder_amd.streamgen import BASE_SEED
from tests.oracle_binding import OracleDecoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "oracle", "_ref", "libmobi_csref.so")
RECORD = os.path.join(ROOT, "tests", "golden", "csref_records.npz")
_recording = None  # tests/golden/make_csref_records.py: a dict that takes the library's results instead of checking them


@functools.lru_cache(maxsize=None)
def _lib():
    """the transliteration library, (re)generated when its generator can run here; None where it cannot"""
    gen = os.path.join(ROOT, "oracle", "tools", "cs2cpp.py")
    sys.path.insert(0, os.path.dirname(gen))
    try:
        import cs2cpp
    finally:
        sys.path.pop(0)
    if not os.path.exists(SO) or (os.path.isdir(cs2cpp.REF) and os.path.getmtime(SO) < os.path.getmtime(gen)):
        if not os.path.isdir(cs2cpp.REF):
            return None
        subprocess.check_call([sys.executable, gen])
    L = C.CDLL(SO)
    L.csref_create.restype = C.c_void_p
    L.csref_create.argtypes = [C.c_uint, C.c_uint, C.c_int]
    L.csref_destroy.argtypes = [C.c_void_p]
    L.csref_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.POINTER(C.c_int)]
    L.csref_stride.argtypes = [C.c_void_p]
    L.csref_quantizer.argtypes = [C.c_void_p]
    L.csref_quantizer.restype = C.c_uint
    for n in ("csref_y", "csref_uv"):
        getattr(L, n).restype = C.POINTER(C.c_uint8)
        getattr(L, n).argtypes = [C.c_void_p, C.c_int]
    L.csref_dec_predict.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int]
    L.csref_enc_compvals.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.csref_enc_plane.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.csref_enc_idct.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.csref_enc_getpblock.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_void_p]
    return L


@functools.lru_cache(maxsize=None)
def _record():
    return dict(np.load(RECORD)) if os.path.exists(RECORD) else {}


def _digest(*parts):
    """64 bits of BLAKE2b over the bytes of the parts, as a signed int64 (0 never stands for a digest: it marks "no output")"""
    h = hashlib.blake2b(digest_size=8)
    for a in parts:
        h.update(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes())
    return int.from_bytes(h.digest(), "little", signed=True) or 1


def _reference(key, live):
    """the transliteration's rows for one case: live(L) where the library exists (and then they must equal the record), else the record"""
    L = _lib()
    if L is not None:
        got = np.asarray(live(L), np.int64)
        if _recording is not None:
            _recording[key] = got
            return got
        assert key in _record() and np.array_equal(_record()[key], got), \
            f"{key}: tests/golden/csref_records.npz does not hold what the transliteration computes (python tests/golden/make_csref_records.py)"
        return got
    assert key in _record(), f"{key}: not in tests/golden/csref_records.npz"
    return _record()[key]


def _slots(get_y, get_uv, f):
    """digest of the ring after frame f: per slot 0..min(5, f) whether it holds a picture, and its Y and UV planes"""
    parts = []
    for r in range(min(6, f + 1)):
        y = get_y(r)
        parts += [b"\0"] if y is None else [b"\1", y, get_uv(r)]
    return _digest(*parts)


def _csref_frames(L, params, data, fo, whole):
    h = L.csref_create(params.width, params.height, params.version)
    S, H = L.csref_stride(h), params.height
    rows = []
    for f in range(params.n_frames):
        buf = np.ascontiguousarray(data if whole else data[: fo[f + 1]])
        off = C.c_int(int(fo[f]))
        rc = L.csref_decode(h, buf.ctypes.data, buf.size, C.byref(off))
        # the frame slot is compared even after a throw: partial frames stay in the ring (MD.cs:325)
        py = lambda r: np.ctypeslib.as_array(L.csref_y(h, r), (H, S)) if L.csref_y(h, r) else None
        puv = lambda r: np.ctypeslib.as_array(L.csref_uv(h, r), (H // 2, S))
        rows.append([int(rc != 0), off.value, L.csref_quantizer(h), _slots(py, puv, f)])
    L.csref_destroy(h)
    return rows


def _diff(key, params, data, fo, whole=False):
    """decode every frame with the oracle and compare it with the transliteration's; return (#frames ok, #frames thrown)"""
    want = _reference(key, lambda L: _csref_frames(L, params, data, fo, whole))
    assert len(want) == params.n_frames, key
    o = OracleDecoder(params.width, params.height, params.version)
    ok = thrown = 0
    for f in range(params.n_frames):
        thr, off, q, planes = (int(v) for v in want[f])
        buf = np.ascontiguousarray(data if whole else data[: fo[f + 1]])
        o.Data, o.Offset = buf, int(fo[f])
        ro = o.DecodeFrame()
        assert bool(thr) == (ro is None), (key, f, thr, o.last_error)
        assert off == o.Offset, (key, f, off, o.Offset)
        assert q == o.Quantizer, (key, f)
        assert planes == _slots(o.y, o.uv, f), (key, f, "Y / UV of the ring differ")
        if thr:
            thrown += 1
        else:
            ok += 1
    return ok, thrown


@pytest.mark.parametrize("cfg", ["A", "B", "C"])
def test_valid_streams(cfg):
    for seed in range(4):
        p = default_params(cfg, BASE_SEED + 500 + seed, n_frames=9, pm_intra=150, pm_deep=150, pm_multiref=300,
                           qdelta_prob=300, table1_prob=500, escape_prob=100, edge_mode=seed & 1,
                           iframe_interval=5 if seed == 3 else 0)
        data, fo = generate_clip(p)
        ok, thrown = _diff(f"valid_{cfg}_{seed}", p, data, fo, whole=bool(seed & 2))
        assert ok == 9 and thrown == 0


def test_small_geometries_and_quantizers():
    for i, (w, h, ver, q) in enumerate([(16, 16, 2, 12), (32, 16, 1, 52), (256, 32, 1, 30), (512, 32, 2, 40), (528, 48, 2, 25), (1024, 32, 2, 18)]):
        p = default_params("A", BASE_SEED + 900 + i, n_frames=8, width=w, height=h, version=ver, quantizer=q, pm_intra=200, mv_range=12)
        data, fo = generate_clip(p)
        assert _diff(f"small_{i}", p, data, fo) == (8, 0), (w, h)


def test_corrupted_streams_including_partial_frames():
    """Bit flips: decode garbage or throw -- both executables must do the same thing, down to the partial
    frame a throw leaves behind and the decoder state it leaks into the following frames."""
    rng = np.random.default_rng(11)
    tot_ok = tot_thrown = 0
    for trial in range(150):
        p = default_params("AB"[trial & 1], BASE_SEED + 2000 + trial, n_frames=5, pm_intra=100, width=64, height=48,
                           version=1 + (trial & 1), pm_deep=200)
        data, fo = generate_clip(p)
        data = data.copy()
        for _ in range(int(rng.integers(1, 5))):
            data[int(rng.integers(0, data.size))] ^= 1 << int(rng.integers(0, 8))
        ok, thrown = _diff(f"corrupt_{trial}", p, data, fo, whole=bool(trial & 2))
        tot_ok += ok
        tot_thrown += thrown
    assert tot_ok > 100 and tot_thrown > 30, (tot_ok, tot_thrown)


def test_low_quantizer_aliasing_domain():
    """ModsDS quantizers below 12 make the dequant word leak into its zigzag byte (MD.cs:3907-3911): the product
    refuses those streams, but the oracle must still follow the reference through the Internal[] aliasing."""
    for q in (0, 3, 7, 11):
        p = default_params("A", BASE_SEED + 3000 + q, n_frames=4, width=64, height=48, quantizer=12)
        data, fo = generate_clip(p)
        data = data.copy()
        # I-frame header: bit0=1, yuv, table, then 6-bit quantizer in bits 12..7 of the first 16-bit LE word
        w = int(data[0]) | (int(data[1]) << 8)
        w = (w & ~(0x3F << 7)) | (q << 7)
        data[0], data[1] = w & 0xFF, w >> 8
        _diff(f"lowq_{q}", p, data, fo)


@pytest.mark.parametrize("cfg", ["A", "B", "C"])
def test_bench_streams(cfg):
    """The exact streams bench.py times (mobiclipdecoder_amd.sharding.stream_seed(config, rank 0, index 0..3), 1 I + 32 P
    frames, SURVEY 8(d) mix) and the streams of the GPU coverage suite: oracle and transliteration agree on every frame."""
    from mobiclipdecoder_amd import sharding
    for i in range(4 if cfg == "B" else 2):
        p = default_params(cfg, sharding.stream_seed(cfg, 0, i), n_frames=33)
        data, fo = generate_clip(p)
        ok, thrown = _diff(f"bench_{cfg}_{i}", p, data, fo)
        assert ok == 33 and thrown == 0


def test_coverage_suite_streams():
    from tests.gpu_streams import suite_params
    for j, p in enumerate(suite_params()):
        data, fo = generate_clip(p)
        ok, thrown = _diff(f"suite_{j}", p, data, fo)
        assert ok == p.n_frames and thrown == 0


S_UNIT, ROWS_UNIT = 256, 40


def _sweep_cases():
    """the unit sweep's random inputs, trial by trial (one seeded generator: the same draws in the same order on every machine)"""
    rng = np.random.default_rng(2024)
    S, ROWS = S_UNIT, ROWS_UNIT
    for trial in range(3000):
        t = {"plane": rng.integers(0, 256, S * ROWS, dtype=np.uint8), "four": bool(trial & 1)}
        t["m"] = int(rng.choice([0, 1, 3, 4, 5, 6, 7, 8])) + (10 if t["four"] else 0)
        t["n"] = n = 4 if t["four"] else 8
        t["x"] = x = int(rng.choice([0, n, 2 * n, 128, 128 + n, 64])); t["y"] = int(rng.choice([0, n, 2 * n, 24]))
        t["uv"] = uv = int(x >= 128 or (trial % 5 == 0))
        t["eoff"] = S // 2 if (uv and x >= S // 2) else 0
        # planes
        t["size"] = int(rng.choice([16, 8, 4])); t["px"] = int(rng.choice([t["size"], 2 * t["size"], 48])); t["py"] = int(rng.choice([t["size"], 16]))
        t["param"] = int(rng.integers(-40, 41))
        # CopyBlock
        t["w"], t["h"] = int(rng.choice([2, 4, 8, 16])), int(rng.choice([2, 4, 8, 16]))
        t["dx"], t["dy"] = int(rng.integers(-20, 21)), int(rng.integers(-20, 21))
        # inverse transforms (encoder statement = the full transform)
        t["nn"] = nn = 16 if t["four"] else 64
        c = np.zeros(nn, np.int32)
        k = int(rng.integers(1, nn + 1))
        pos = rng.choice(nn, size=k, replace=False)
        c[pos] = rng.integers(-60, 61, k) * int(rng.choice([16, 40, 64, 104, 160]))
        t["coef"], t["pred"] = c, rng.integers(0, 256, nn, dtype=np.uint8)
        yield t


_COPY_BASE = 12 * S_UNIT + 32


def _csref_sweep(L):
    """per trial: [flags, predicted plane, encoder compvals, plane predictor, GetPBlock, IDCT] -- flags 1: the decoder's PredictIntra
    throws, 2: the encoder's GetCompvals ran (asked only when PredictIntra did not throw), 4: the IDCT throws; digests, 0 = no output"""
    S = S_UNIT
    dec = L.csref_create(256, 192, 2)
    rows = []
    for t in _sweep_cases():
        plane, n, x, y = t["plane"], t["n"], t["x"], t["y"]
        row = [0, 0, 0, 0, 0, 0]
        b = plane.copy()
        if L.csref_dec_predict(dec, t["m"], b.ctypes.data, b.size, y * S + x, t["uv"]) != 0:
            row[0] |= 1
        else:
            row[1] = _digest(b)
            e, eo = plane.copy(), np.zeros(64, np.uint8)
            if L.csref_enc_compvals(t["m"], e.ctypes.data, e.size, x - t["eoff"], y, S, t["eoff"], eo.ctypes.data) == 0:
                row[0] |= 2
                row[2] = _digest(eo[: n * n])
        size = t["size"]
        e, eo = plane.copy(), np.zeros(256, np.uint8)
        assert L.csref_enc_plane(size, e.ctypes.data, e.size, t["py"] * S + t["px"], S, t["param"], eo.ctypes.data) == 0
        row[3] = _digest(eo[: size * size])
        eo = np.zeros(256, np.uint8)
        assert L.csref_enc_getpblock(plane.ctypes.data, plane.size, t["dx"], t["dy"], t["w"], t["h"], _COPY_BASE, S, eo.ctypes.data) == 0
        row[4] = _digest(eo[: t["w"] * t["h"]])
        eo = np.zeros(t["nn"], np.uint8)
        if L.csref_enc_idct(t["nn"], t["coef"].ctypes.data, t["pred"].ctypes.data, eo.ctypes.data) != 0:
            row[0] |= 4
        else:
            row[5] = _digest(eo)
        rows.append(row)
    return rows


def test_unit_statements_random_sweep():
    """The oracle's unit entry points against BOTH reference statements of each unit (decoder PredictIntra; the encoder's GetCompvals /
    PredictIntraPlane / IDCT / FrameUtil.GetPBlock copies) on thousands of random inputs -- the committed
    tests/golden/unit_vectors.npz is a small sample of this sweep that the GPU tests use too."""
    from tests.oracle_binding import lib as oracle_lib
    OL = oracle_lib()
    want = _reference("unit_sweep", _csref_sweep)
    S, ROWS = S_UNIT, ROWS_UNIT
    stated_twice = 0
    for trial, t in enumerate(_sweep_cases()):
        flags, d_pred, d_compvals, d_plane, d_copy, d_idct = (int(v) for v in want[trial])
        plane, m, n, x, y, uv = t["plane"], t["m"], t["n"], t["x"], t["y"], t["uv"]
        a = plane.copy()
        ra = OL.mobi_oracle_predict(m, a.ctypes.data, a.size, y * S + x, S, uv)
        assert (ra != 0) == bool(flags & 1), (trial, m, x, y, uv)
        if not flags & 1:
            assert _digest(a) == d_pred, (trial, m, x, y, uv)
            if flags & 2:
                assert _digest(a.reshape(ROWS, S)[y:y + n, x:x + n]) == d_compvals, ("encoder statement", trial, m, x, y, uv)
                stated_twice += 1
        # planes
        size, px, py = t["size"], t["px"], t["py"]
        a = plane.copy()
        assert OL.mobi_oracle_plane(size, t["param"], a.ctypes.data, a.size, py * S + px, S) == 0
        assert _digest(a.reshape(ROWS, S)[py:py + size, px:px + size]) == d_plane, (trial, size, px, py, t["param"])
        # CopyBlock
        w, h, dx, dy = t["w"], t["h"], t["dx"], t["dy"]
        dst = np.zeros(S * ROWS, np.uint8)
        assert OL.mobi_oracle_copyblock(plane.ctypes.data, plane.size, dx, dy, w, h, dst.ctypes.data, dst.size, _COPY_BASE, S) == 0
        assert _digest(dst.reshape(ROWS, S)[12:12 + h, 32:32 + w]) == d_copy, (trial, w, h, dx, dy)
        # inverse transforms
        c, p, side = t["coef"], t["pred"], 4 if t["four"] else 8
        d = np.zeros(side * 16, np.uint8)
        d.reshape(side, 16)[:, :side] = p.reshape(side, side)
        fn = OL.mobi_oracle_idct4 if t["four"] else OL.mobi_oracle_idct8
        ro = fn(c.ctypes.data, t["nn"], d.ctypes.data, d.size, 0, 16)
        assert (ro != 0) == bool(flags & 4), trial
        if not flags & 4:
            assert _digest(d.reshape(side, 16)[:, :side]) == d_idct, trial
    assert stated_twice > 1500
