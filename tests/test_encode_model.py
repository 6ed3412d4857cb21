"""The intra encoder without a GPU (include/mobiclip_encode.h; csrc/mobi_encode.h run by tests/tools/mobi_encode_host.cpp, the host model
the kernels are compared against in tests/test_encode_gpu.py).

  1  closed loop: every stream decodes in the oracle to exactly the model's reconstruction, same quantiser and yuv_format, no byte past
     bytes_out read
  2  every decision re-derived independently (tests/enc_model.py: predictors from their formulas, transform coding from
     tests/tools/txcode_ref.c, neighbours from the oracle-decoded picture): modes and cbp are the argmin of J under the tie rule, uncoded
     blocks are exactly the zero-level and fallback ones, the re-derived bits + 9 + padding = 8 * bytes_out
  3  the picture sets cover what they must (see test_coverage_condition for the one demand that CANNOT be met, and why)
  4  shapes 16x16, 48x32, 256x192 (stride = width), 272x208 (stride != width); N = 1 and N = 5 with a quantiser per picture
  5  refusals and the stream bound
  6  the host model as a stand-alone program under -fsanitize=address,undefined
  7  closed loop and parse-back at enc_model.GEOMETRY_SHAPES, and what the GPU comparison there rests on"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import enc_model as E
from tests import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOBI_E_ARG, MOBI_E_VERSION = -7, -4
_CACHE = {}


def encoded(W, H, name):
    """the host model's output for one picture set (version does not enter the encoder's arithmetic: test_versions_encode_alike), once"""
    key = (W, H, name)
    if key not in _CACHE:
        pics, qs = E.picture_sets(W, H)[name]
        _CACHE[key] = (pics, qs, E.host_encode(W, H, 2, pics, qs, yuv_format=1 if name == "sat_q52" else 0))
    return _CACHE[key]


SETS = ("mixed5", "sat_q52", "sat_q12", "hard5")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return E.txref(tmp_path_factory.mktemp("enc_txref"))


def test_header_library_and_binding_agree():
    from mobiclipdecoder_amd import encode, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobiclip_encode.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mobi_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(encode._SIGS) and len(names) == 6
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(names) <= exported
    import mobiclipdecoder_amd as m
    assert m.MobiclipIntraEncoder is encode.MobiclipIntraEncoder
    assert encode.STATS_DTYPE == E.STATS_DTYPE and E.STATS_DTYPE.itemsize == 64


def test_every_symbol_is_written_as_priced_and_reads_back():
    """all (|level| <= 2047, run, last): the writer's length = mobi_tc_cost's price = the cost table's entry; the pattern, read with the
    oracle's tables the way the decoder does, gives the symbol back"""
    L = E.host()
    n = 44 * 64 * 2
    pat, ln, form = np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    assert L.enc_host_symbol_walk(pat.ctypes.data, ln.ctypes.data, form.ctypes.data) == 0
    T = tables.load()
    A, B = T["mobi_vx2table0_a"], T["mobi_vx2table0_b"]
    seen = set()
    for v in range(1, 44):
        for run in range(64):
            for last in (0, 1):
                at = (v * 64 + run) * 2 + last
                bits, nb, f = int(pat[at]), int(ln[at]), int(form[at])
                seen.add(f)
                assert (bits >> (nb - 7)) == 3 if f else (nb < 7 or (bits >> (nb - 7)) != 3), "the escape prefix belongs to the escapes alone"
                if f == 3:
                    assert nb == 28 and bits == (15 << 19 | last << 18 | run << 12 | v)
                    continue
                body = nb - (0, 9, 8)[f]
                assert (bits >> body) == (0, 14, 6)[f]
                e = int(A[(bits & ((1 << body) - 1)) << (12 - body) if body <= 12 else (bits & ((1 << body) - 1)) >> (body - 12)])
                assert (e & 15) == body
                val, r, la = (e >> 4) & 31, (e >> 9) & 63, e >> 15
                if f == 2:
                    val += int(B[e >> 9])
                if f == 1:
                    r += int(B[0x80 + val + (la << 6)])
                assert (val, r, la) == (v, run, last) and not bits & 1
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("W,H", E.SHAPES)
def test_closed_loop_through_the_oracle(W, H):
    for name in SETS:
        pics, qs, r = encoded(W, H, name)
        yuv = 1 if name == "sat_q52" else 0
        for version in E.VERSIONS:
            for i in range(len(qs)):
                n = int(r["bytes"][i])
                assert n % 2 == 0 and n <= r["streams"].shape[1]
                assert not r["streams"][i, n:].any(), "zeros behind the stream"
                dec, used, q, yf = E.oracle_decode(W, H, version, r["streams"][i, :n])
                assert np.array_equal(dec, r["recon"][i]), (name, version, i)
                assert (q, yf) == (int(qs[i]), yuv)
                assert used <= n


@pytest.mark.parametrize("version", E.VERSIONS)
@pytest.mark.parametrize("W,H", E.GEOMETRY_SHAPES)
def test_geometry_shapes_through_the_oracle(W, H, version):
    """enc_model.GEOMETRY_SHAPES, the mixed five: the oracle decodes every stream to the reported reconstruction within its bytes, the
    stream reads back to the model's records, and the pictures meet what the GPU comparison at these shapes rests on"""
    pics, qs = E.picture_sets(W, H)["mixed5"]
    r = E.host_encode(W, H, version, pics, qs)
    mbw, nmb = W // 16, (W // 16) * (H // 16)
    forms = np.zeros(4, np.int64)
    for i in range(len(qs)):
        n = int(r["bytes"][i])
        assert n % 2 == 0 and n <= r["streams"].shape[1] and not r["streams"][i, n:].any()
        dec, used, q, yf = E.oracle_decode(W, H, version, r["streams"][i, :n])
        assert np.array_equal(dec, r["recon"][i]), i
        assert (q, yf) == (int(qs[i]), 0) and used <= n
        ps = E.parse_stream(r["streams"][i, :n], W, H)
        for f in ("lev", "bits", "luma_mode", "chroma_mode", "cbp"):
            assert np.array_equal(ps["mbs"][f], r["mbs"][i][f]), (i, f)
        assert ps["q"] == int(qs[i]) and ps["end"] == int(r["stats"]["bits"][i]) == 9 + int(r["mbs"]["bits"][i].sum())
        assert 8 * n == (ps["end"] + 16 + 15) // 16 * 16
        forms += ps["forms"]
    assert np.array_equal(forms, r["forms"])
    if nmb > 256:
        E.geometry_preconditions(r["mbs"]["bits"], r["stats"]["bits"], (W, H, version, "intra"))
    if H > W:
        # below the main diagonal (mby > mbx: the macroblocks a wrong diagonal range would hand an unfinished border) every mode that can
        # occur is chosen, so a stale border changes bytes.  One column has no left neighbour: mode 1 is not allowed there at all.
        idx = np.arange(nmb)
        seen = np.bincount(r["mbs"]["luma_mode"][:, idx // mbw > idx % mbw].ravel(), minlength=4)
        assert seen[0] > 0 and seen[3] > 0 and seen[2] == 0 and (seen[1] > 0) == (mbw > 1), seen


def test_versions_encode_alike():
    pics, qs = E.picture_sets(48, 32)["mixed5"]
    a, b = E.host_encode(48, 32, 2, pics, qs), E.host_encode(48, 32, 1, pics, qs)
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("W,H", E.SHAPES)
def test_decisions_are_the_argmin_of_the_stated_cost(W, H, ref):
    for name in SETS:
        pics, qs, r = encoded(W, H, name)
        for i in range(len(qs)):
            n = int(r["bytes"][i])
            ps = E.parse_stream(r["streams"][i, :n], W, H)
            dec = E.oracle_decode(W, H, 2, r["streams"][i, :n])[0]
            d = E.rederive(ref, W, H, int(qs[i]), pics[i], dec)
            where = (name, i)
            assert np.array_equal(d["luma_mode"], ps["mbs"]["luma_mode"]), where
            assert np.array_equal(d["chroma_mode"], ps["mbs"]["chroma_mode"]), where
            assert np.array_equal(d["cbp"], ps["mbs"]["cbp"]), where       # uncoded = zero levels or a fallback, nothing else
            assert np.array_equal(d["lev"], ps["mbs"]["lev"]), where
            assert np.array_equal(d["bits"], ps["mbs"]["bits"]), where      # written as priced, macroblock by macroblock
            total = 9 + int(d["bits"].sum())
            assert ps["end"] == total
            assert 8 * n == (total + 16 + 15) // 16 * 16                    # 16 zero bits, then zeros to the word boundary
            st = r["stats"][i]
            assert int(st["bits"]) == total
            assert (int(st["fallback_clamp"]), int(st["fallback_level"])) == (d["clamp"], d["range"])
            assert int(st["coded_blocks"]) == sum(bin(int(c)).count("1") for c in ps["mbs"]["cbp"])
            assert [int(x) for x in st["luma_modes"]] == [int((ps["mbs"]["luma_mode"] == m).sum()) for m in range(4)]
            assert [int(x) for x in st["chroma_modes"]] == [int((ps["mbs"]["chroma_mode"] == m).sum()) for m in range(4)]
            assert int(st["sad"]) == int(np.abs(pics[i].astype(np.int64) - r["recon"][i]).sum())


def test_coverage_condition():
    """Over the picture sets of all shapes: every luma and chroma mode is chosen, coded and uncoded blocks occur in luma and in chroma, each
    of the four code forms is written, a clamp fallback occurs.

    A LEVEL-RANGE fallback cannot occur in any picture, whatever the input: a forward-transform output is at most 23500 in size
    (tests/test_txcode.py, test_dct_output_bound_is_23500) and the smallest quantiser step at q = 12, the lowest quantiser the encoder
    takes, is 18, so |level| <= 23500 / 18 = 1305 < 2047.  The test states that bound, requires the count to be 0 everywhere, and
    test_level_range_rule_below_the_encoders_quantisers runs the rule where it can fire: the block function at table quantisers below 12."""
    luma, chroma, forms = np.zeros(4, np.int64), np.zeros(4, np.int64), np.zeros(4, np.int64)
    clamp = level = 0
    coded = {"luma": set(), "chroma": set()}
    for W, H in E.SHAPES:
        for name in SETS:
            _, _, r = encoded(W, H, name)
            luma += r["stats"]["luma_modes"].sum(0).astype(np.int64)
            chroma += r["stats"]["chroma_modes"].sum(0).astype(np.int64)
            forms += r["forms"].astype(np.int64)
            clamp += int(r["stats"]["fallback_clamp"].sum())
            level += int(r["stats"]["fallback_level"].sum())
            cbp = r["mbs"]["cbp"].ravel()
            coded["luma"] |= {bool(c & (1 << k)) for c in cbp for k in range(4)}
            coded["chroma"] |= {bool(c & (1 << k)) for c in cbp for k in (4, 5)}
    assert all(luma[[0, 1, 3]] > 0) and luma[2] == 0
    assert all(chroma[[0, 1, 3]] > 0) and chroma[2] == 0
    assert coded == {"luma": {True, False}, "chroma": {True, False}}
    assert all(forms > 0), forms
    assert clamp > 0
    T = tables.load()
    for q in range(12, 53):
        step = min((int(v) << (int(T["mobi_qdiv6"][q]) + 6)) >> 8 for v in T["mobi_dq8"].reshape(-1, 64)[int(T["mobi_qmod6"][q])])
        assert 23500 // step < 2047
    assert level == 0


def test_level_range_rule_below_the_encoders_quantisers():
    """the rule the pictures cannot reach: at table quantiser 0 a flat residual of 255 gives a DC level beyond the raw escape's 12 bits;
    the block is then sent uncoded -- reconstruction = prediction, 0 bits, the prediction's SAD -- and counted as a level-range fallback"""
    L = E.host()
    src, pred = np.full(64, 255, np.uint8), np.zeros(64, np.uint8)
    lev, rec, out = np.zeros(64, np.int16), np.zeros(64, np.uint8), np.zeros(5, np.int32)
    hit = 0
    for q in range(0, 12):
        L.enc_host_block(q, src.ctypes.data, pred.ctypes.data, lev.ctypes.data, rec.ctypes.data, out.ctypes.data)
        if out[4]:
            hit += 1
            assert list(out) == [255 * 64, 0, 0, 0, 1] and not lev.any() and np.array_equal(rec, pred)
    assert hit > 0
    L.enc_host_block(30, src.ctypes.data, pred.ctypes.data, lev.ctypes.data, rec.ctypes.data, out.ctypes.data)
    assert out[2] == 1 and out[4] == 0 and lev[0] != 0


def test_one_macroblock_predicts_128():
    """16x16: no neighbours, so only DC is allowed and it predicts 128; a flat 128 picture costs the syntax alone"""
    pic = np.full((1, 384), 128, np.uint8)
    r = E.host_encode(16, 16, 2, pic, [30])
    assert r["mbs"][0, 0]["luma_mode"] == 3 and r["mbs"][0, 0]["chroma_mode"] == 3 and r["mbs"][0, 0]["cbp"] == 0
    assert np.array_equal(r["recon"], pic) and int(r["stats"]["bits"][0]) == 9 + 1 + 1 + 6 and r["bytes"][0] == 6


def test_refusals_need_no_device():
    from mobiclipdecoder_amd import encode
    lib = encode._lib()
    q = np.array([12, 52, 30], np.uint8)

    def both(maxp=4, W=64, H=48, ver=2, n=3, pitch=64 * 48 * 3 // 2, qs=q, yuv=0, slot=4096):
        a = lib.mobi_enc_check(maxp, W, H, ver, n, pitch, qs.ctypes.data if qs is not None else None, yuv, slot)
        b = E.host().enc_host_check(maxp, W, H, ver, n, pitch, qs.ctypes.data if qs is not None else None, yuv, slot)
        assert a == b
        return a
    assert both() == 0
    assert both(ver=0) == MOBI_E_VERSION and both(ver=3) == MOBI_E_VERSION
    for bad in (dict(W=60), dict(H=40), dict(W=0), dict(H=0), dict(W=1040), dict(maxp=0), dict(n=0), dict(n=5), dict(n=-1), dict(pitch=64 * 48 * 3 // 2 - 8),
                dict(pitch=64 * 48 * 3 // 2 + 4), dict(qs=None), dict(qs=np.array([12, 11, 30], np.uint8)), dict(qs=np.array([53, 20, 30], np.uint8)),
                dict(yuv=2), dict(yuv=-1), dict(slot=4094)):
        assert both(**bad) == MOBI_E_ARG, bad
    assert both(pitch=64 * 48 * 3 // 2 + 8) == 0 and both(slot=0) == 0 and both(W=1024, pitch=1024 * 48 * 3 // 2) == 0
    assert lib.mobi_enc_stream_bound(60, 48) == 0 and lib.mobi_enc_stream_bound(64, 48) == E.host().enc_host_bound(64, 48)
    assert lib.mobi_enc_create(0, 64, 48, 2, 0) is None and lib.mobi_enc_create(4, 60, 48, 2, 0) is None and lib.mobi_enc_create(4, 64, 48, 0, 0) is None
    assert lib.mobi_enc_intra(None, 1, None, 0, None, 0, None, 0, None, None, None) == MOBI_E_ARG


def test_stream_bound_holds():
    """>= every length seen, and >= a picture built against it: every block coded, every one of its 64 levels a raw escape, the longest
    cbp code -- which is the bound itself up to the alignment"""
    L = E.host()
    for W, H in E.SHAPES:
        bound = L.enc_host_bound(W, H)
        assert bound % 4 == 0
        for name in SETS:
            assert encoded(W, H, name)[2]["bytes"].max() <= bound
        T = tables.load()
        inv = {int(c): i for i, c in reversed(list(enumerate(T["mobi_cbp_intra"])))}
        assert inv[63] <= 63 and max(inv.values()) == 63
        mbs = np.zeros((W // 16) * (H // 16), E.MB_DTYPE)
        mbs["lev"] = np.where(np.arange(64) % 2, -2047, 1999).astype(np.int16)
        mbs["cbp"] = 63
        mbs["luma_mode"] = mbs["chroma_mode"] = 3
        slot = np.zeros(bound, np.uint8)
        n = L.enc_host_write(W, H, 12, 0, mbs.ctypes.data, slot.ctypes.data, bound)
        assert 0 < n <= bound
        assert (mbs["bits"] == 1 + E._ue_bits(inv[63]) + 6 + 6 * (1 + 64 * 28)).all()
        ps = E.parse_stream(slot[:n], W, H)
        assert np.array_equal(ps["mbs"]["lev"], mbs["lev"]) and ps["forms"][3] == 6 * 64 * len(mbs)
        assert bound - n < 4 + len(mbs) * (13 - E._ue_bits(inv[63])) // 8 + 2


def test_slot_too_small_is_zero_and_length_is_true():
    pics, qs, full = encoded(48, 32, "mixed5")
    small = (int(full["bytes"][0]) - 2) // 4 * 4
    r = E.host_encode(48, 32, 2, pics, qs, slot_bytes=small)
    assert np.array_equal(r["bytes"], full["bytes"]) and not r["streams"][0].any()
    for i in range(1, 5):
        assert np.array_equal(r["streams"][i, : full["bytes"][i]], full["streams"][i, : full["bytes"][i]])


def test_picture_pitch_and_threads():
    pics, qs, full = encoded(48, 32, "hard5")
    wide = np.full((5, pics.shape[1] + 24), 0x55, np.uint8)
    wide[:, : pics.shape[1]] = pics
    r = E.host_encode(48, 32, 2, wide, qs, pitch=wide.shape[1], threads=3)
    assert all(np.array_equal(r[k], full[k]) for k in ("streams", "bytes", "recon", "stats", "mbs", "forms"))


def test_host_model_under_sanitizers(tmp_path):
    """tests/tools/enc_host_main.cpp: a program of its own with -fsanitize=address,undefined (nothing sanitised is loaded into Python)"""
    exe = str(tmp_path / "enc_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-variable", "-fwrapv", "-pthread", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I" + E.CSRC, os.path.join(E.TOOLS, "enc_host_main.cpp"), os.path.join(E.TOOLS, "mobi_encode_host.cpp"),
                    "-o", exe], check=True)
    for W, H in ((48, 32), (256, 192)):
        bound = E.host().enc_host_bound(W, H)
        for name in SETS:
            pics, qs, want = encoded(W, H, name)
            if name == "sat_q52":
                want = E.host_encode(W, H, 2, pics, qs)  # (the cached one was made with yuv_format 1)
            src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
            with open(src, "wb") as f:
                f.write(qs.tobytes() + pics.tobytes())
            p = subprocess.run([exe, str(W), str(H), "2", str(len(qs)), src, dst], capture_output=True, text=True)
            assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
            blob = np.fromfile(dst, np.uint8)
            n = len(qs)
            assert np.array_equal(blob[: 4 * n].view(np.int32), want["bytes"])
            assert np.array_equal(blob[4 * n: 4 * n + n * bound].reshape(n, bound), want["streams"])
            assert np.array_equal(blob[4 * n + n * bound:].reshape(n, -1), want["recon"])
