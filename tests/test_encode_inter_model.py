"""The inter encoder without a GPU (include/mobiclip_encode_inter.h; csrc/mobi_encode_inter.h run by tests/tools/mobi_encode_inter_host.cpp,
the host model the kernels are compared against in tests/test_encode_inter_gpu.py).

  1  closed loop: the oracle decodes I, P, P, P in order; every frame equals the model's reconstruction, the header's delta gives the
     oracle's quantiser, no byte past bytes_out is read
  2  every decision re-derived independently (tests/enc_inter_model.py: interpolation from its formula, v* by brute force over the
     candidate set under the tie rule, the median of the decoded neighbours, code 0 iff equal, cbp and uncoded blocks as ruled, the
     re-derived bits + header + padding = 8 * bytes_out)
  3  the sequences cover what they must (test_coverage_conditions)
  4  on the pure full-pel translation every P-frame is shorter than the I-frame of the same picture at the same quantiser
  5  refusals, the stream bound, a slot too small, header / library / binding
  6  the host model as a stand-alone program under -fsanitize=address,undefined
  7  closed loop and parse-back at enc_model.GEOMETRY_SHAPES, with the still scene, and what the GPU comparison there rests on
Shapes 16x16 (no neighbour, and no vector but (0, 0) fits the rectangle), 48x32, 272x208 (stride != width); N = 1 and N = 5."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import enc_inter_model as M
from tests import enc_model as E
from tests import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOBI_E_ARG, MOBI_E_VERSION = -7, -4
_CACHE = {}


def encoded(W, H, name):
    """the host models' chain for one set (the version enters only the partition code words: test_versions_differ_in_code_words_only)"""
    key = (W, H, name)
    if key not in _CACHE:
        frames, qs = M.sequence_sets(W, H)[name]
        _CACHE[key] = (frames, qs, M.chain(W, H, 2, frames, qs))
    return _CACHE[key]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return E.txref(tmp_path_factory.mktemp("encp_txref"))


def test_header_library_and_binding_agree():
    from mobiclipdecoder_amd import build, encode_inter
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobiclip_encode_inter.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mobi_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(encode_inter._SIGS) and len(names) == 6
    assert set(names) <= set(build.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    import mobiclipdecoder_amd as m
    assert m.MobiclipInterEncoder is encode_inter.MobiclipInterEncoder and m.encode_clips is encode_inter.encode_clips
    assert encode_inter.STATS_DTYPE == M.STATS_DTYPE and M.STATS_DTYPE.itemsize == 64


def test_range_constant():
    """one named constant: the model's, the re-derivation's, and DESIGN.md states it"""
    assert M.host().encp_host_range() == M.RANGE
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"`MOBI_ENCP_RANGE` = {M.RANGE}" in text


@pytest.mark.parametrize("W,H", M.SHAPES)
def test_closed_loop_through_the_oracle(W, H):
    for name in M.SETS:
        frames, qs, _ = encoded(W, H, name)
        for version in M.VERSIONS:
            ch = M.chain(W, H, version, frames, qs)
            for c in range(frames.shape[0]):
                streams = []
                for t in range(M.T):
                    n = int(ch[t]["bytes"][c])
                    assert n % 2 == 0 and n <= ch[t]["streams"].shape[1]
                    assert not ch[t]["streams"][c, n:].any(), "zeros behind the stream"
                    streams.append(ch[t]["streams"][c, :n])
                for t, (dec, used, q) in enumerate(M.oracle_chain(W, H, version, streams)):
                    assert np.array_equal(dec, ch[t]["recon"][c]), (name, version, c, t)
                    assert q == int(qs[c, t]) and used <= len(streams[t]), (name, version, c, t)


@pytest.mark.parametrize("version", M.VERSIONS)
@pytest.mark.parametrize("W,H", E.GEOMETRY_SHAPES)
def test_geometry_shapes_through_the_oracle(W, H, version):
    """enc_model.GEOMETRY_SHAPES, the mixed five and the still scene: the oracle decodes I, P, P, P to the reported reconstructions within
    the streams' bytes; every P-frame reads back to the model's records, its vectors from predictors whose neighbours do NOT wrap round
    the picture's edge (one column: no left, no top-right neighbour); and the sets meet what the GPU comparison at these shapes rests on"""
    mbw, nmb = W // 16, (W // 16) * (H // 16)
    for name in M.GEOMETRY_SETS:
        frames, qs = M.geometry_set(W, H, name)
        ch = M.chain(W, H, version, frames, qs)
        for c in range(frames.shape[0]):
            streams = []
            for t in range(M.T):
                n = int(ch[t]["bytes"][c])
                assert n % 2 == 0 and n <= ch[t]["streams"].shape[1] and not ch[t]["streams"][c, n:].any()
                streams.append(ch[t]["streams"][c, :n])
            for t, (dec, used, q) in enumerate(M.oracle_chain(W, H, version, streams)):
                assert np.array_equal(dec, ch[t]["recon"][c]), (name, c, t)
                assert q == int(qs[c, t]) and used <= len(streams[t]), (name, c, t)
            for t in range(1, M.T):
                r, where = ch[t], (name, c, t)
                ps = M.parse_p_stream(streams[t], W, H, version)
                assert ps["dq"] == int(qs[c, t]) - int(qs[c, t - 1]), where
                for f in ("lev", "bits", "cbp"):
                    assert np.array_equal(ps["mbs"][f], r["mbs"][c][f]), (where, f)
                assert ps["end"] == int(r["stats"]["bits"][c]) == ps["hdr_bits"] + int(r["mbs"]["bits"][c].sum()), where
                assert 8 * len(streams[t]) == (ps["end"] + 16 + 15) // 16 * 16, where
                dx, dy = np.zeros(nmb, np.int64), np.zeros(nmb, np.int64)
                at = lambda a, x, y: int(a[y * mbw + x]) if 0 <= x < mbw and y >= 0 else 0
                for i in range(nmb):
                    x, y = i % mbw, i // mbw
                    dx[i] = M.med3(at(dx, x - 1, y), at(dx, x, y - 1), at(dx, x + 1, y - 1)) + ps["ddx"][i]
                    dy[i] = M.med3(at(dy, x - 1, y), at(dy, x, y - 1), at(dy, x + 1, y - 1)) + ps["ddy"][i]
                mdx, mdy = M.unpack_mv(r["mv"][c])
                assert np.array_equal(dx, mdx) and np.array_equal(dy, mdy), where
                assert np.array_equal(ps["code"], (r["mv"][c] != r["mvp"][c]).astype(np.int64)), where
                assert int(r["stats"]["code0"][c]) == int((ps["code"] == 0).sum()) and int(r["stats"]["mv_bits"][c]) == ps["mv_bits"], where
        for t in range(1, M.T):
            if name == "still":
                # nothing moves and nothing is left to code: a partition code 0 (1 bit on Moflex3DS, 2 on ModsDS) and ue(0) per macroblock,
                # 16 or 10 of them to a 32-bit word, whether or not the header changes the quantiser
                assert (ch[t]["mbs"]["bits"] == (2 if version == 2 else 3)).all() and (ch[t]["stats"]["code0"] == nmb).all(), t
                assert np.array_equal(ch[t]["recon"], ch[0]["recon"]) and np.array_equal(frames[:, t], ch[0]["recon"]), t
            elif nmb > 256:
                E.geometry_preconditions(ch[t]["mbs"]["bits"], ch[t]["stats"]["bits"], (W, H, version, "inter", t))
        if name == "still":
            dq = qs[:, 1:].astype(int) - qs[:, :-1]
            assert (dq != 0).any(1).sum() == 1 and (dq == 0).all(1).sum() == 2  # one clip's headers change the quantiser, two clips' do not


def test_versions_differ_in_code_words_only():
    frames, qs = M.sequence_sets(48, 32)["mixed5"]
    a, b = M.chain(48, 32, 2, frames, qs), M.chain(48, 32, 1, frames, qs)
    for t in range(1, M.T):
        assert all(np.array_equal(a[t][k], b[t][k]) for k in ("recon", "mv", "mvp", "forms"))
        assert np.array_equal(a[t]["mbs"]["lev"], b[t]["mbs"]["lev"]) and np.array_equal(a[t]["mbs"]["cbp"], b[t]["mbs"]["cbp"])


@pytest.mark.parametrize("W,H", M.SHAPES)
def test_decisions_are_the_argmin_of_the_stated_cost(W, H, ref):
    for name in M.SETS:
        frames, qs, ch = encoded(W, H, name)
        mbw = W // 16
        for c in range(frames.shape[0]):
            for t in range(1, M.T):
                r, where = ch[t], (name, c, t)
                n, q = int(r["bytes"][c]), int(qs[c, t])
                reference = ch[t - 1]["recon"][c]  # (= what the oracle decoded: test_closed_loop_through_the_oracle)
                ps = M.parse_p_stream(r["streams"][c, :n], W, H, 2)
                assert ps["dq"] == q - int(qs[c, t - 1]), where
                # the vectors the stream decodes to: predictor (median of the decoded neighbours) + the difference sent
                dx, dy = np.zeros(len(ps["code"]), np.int64), np.zeros(len(ps["code"]), np.int64)
                at = lambda a, x, y: int(a[y * mbw + x]) if 0 <= x < mbw and y >= 0 else 0
                for i in range(len(dx)):
                    x, y = i % mbw, i // mbw
                    dx[i] = M.med3(at(dx, x - 1, y), at(dx, x, y - 1), at(dx, x + 1, y - 1)) + ps["ddx"][i]
                    dy[i] = M.med3(at(dy, x - 1, y), at(dy, x, y - 1), at(dy, x + 1, y - 1)) + ps["ddy"][i]
                # v* is the argmin under the tie rule
                sdx, sdy = M.search_picture(W, H, q, E.planes(frames[c, t].astype(np.int64), W, H)[0], E.planes(reference.astype(np.int64), W, H)[0])[:2]
                assert np.array_equal(dx, sdx) and np.array_equal(dy, sdy), where
                mdx, mdy = M.unpack_mv(r["mv"][c])
                assert np.array_equal(dx, mdx) and np.array_equal(dy, mdy), where
                d = M.rederive(ref, W, H, 2, q, frames[c, t], reference, (dx, dy))
                pdx, pdy = M.unpack_mv(r["mvp"][c])
                assert np.array_equal(d["pdx"], pdx) and np.array_equal(d["pdy"], pdy), where
                assert np.array_equal(d["code"], ps["code"]), where          # code 0 iff the vector is the predictor
                assert np.array_equal(d["cbp"], ps["mbs"]["cbp"]), where     # uncoded = zero levels or a fallback, nothing else
                assert np.array_equal(d["lev"], ps["mbs"]["lev"]), where
                assert np.array_equal(d["bits"], ps["mbs"]["bits"]), where   # written as priced, macroblock by macroblock
                assert np.array_equal(d["recon"], r["recon"][c]), where
                total = ps["hdr_bits"] + int(d["bits"].sum())
                assert ps["end"] == total
                assert 8 * n == (total + 16 + 15) // 16 * 16                 # 16 zero bits, then zeros to the word boundary
                st = r["stats"][c]
                assert int(st["bits"]) == total and int(st["mv_bits"]) == d["mv_bits"] == ps["mv_bits"]
                assert (int(st["fallback_clamp"]), int(st["fallback_level"])) == (d["clamp"], d["range"])
                assert int(st["coded_blocks"]) == sum(bin(int(v)).count("1") for v in ps["mbs"]["cbp"])
                assert int(st["code0"]) == int((ps["code"] == 0).sum())
                assert int(st["nonzero_mv"]) == int(((dx != 0) | (dy != 0)).sum()) and int(st["halfpel_mv"]) == int((((dx | dy) & 1) != 0).sum())
                assert int(st["sad"]) == int(np.abs(frames[c, t].astype(np.int64) - r["recon"][c]).sum())


def test_coverage_conditions():
    """Asserted on the model's output over the sets of all shapes: macroblocks with each half-pel phase (x, y, both); a code-0 macroblock
    with a nonzero vector; a macroblock whose unconstrained SAD winner lies outside the rectangle, so that the constraint decides; vector
    components of +16 and of -16; coded and uncoded blocks in Y, U and V; a clamp fallback; a nonzero and a zero quantiser delta.

    As for the intra encoder (tests/test_encode_model.py, test_coverage_condition) a LEVEL-RANGE fallback cannot occur at the encoder's
    quantisers: |level| <= 23500 / 18 < 2047; the count must be 0."""
    phases, comps, coded, deltas = set(), set(), {k: set() for k in range(6)}, set()
    code0_nonzero = outside = clamp = level = 0
    for W, H in M.SHAPES:
        for name in M.SETS:
            frames, qs, ch = encoded(W, H, name)
            for t in range(1, M.T):
                r = ch[t]
                dx, dy = M.unpack_mv(r["mv"])
                phases |= set(((dx & 1) | (dy & 1) << 1).ravel().tolist())
                comps |= set(dx.ravel().tolist()) | set(dy.ravel().tolist())
                code0_nonzero += int(((r["mv"] == r["mvp"]) & (r["mv"] != 0)).sum())
                clamp += int(r["stats"]["fallback_clamp"].sum())
                level += int(r["stats"]["fallback_level"].sum())
                for k in range(6):
                    coded[k] |= set((((r["mbs"]["cbp"] >> k) & 1) != 0).ravel().tolist())
                deltas |= set((qs[:, t].astype(int) - qs[:, t - 1]).tolist())
            if (W, H, name) == (48, 32, "mixed5"):  # the sharp translated clip: the true motion leaves the picture at its borders
                mbw = W // 16
                got = M.search_picture(W, H, int(qs[0, 1]), E.planes(frames[0, 1].astype(np.int64), W, H)[0], E.planes(ch[0]["recon"][0].astype(np.int64), W, H)[0])
                for i in range(len(got[0])):
                    if not M.vector_ok(W, H, i % mbw, i // mbw, int(got[4][i]), int(got[5][i])):
                        outside += 1
                        assert (int(got[2][i]), int(got[3][i])) != (int(got[4][i]), int(got[5][i]))
    assert phases == {0, 1, 2, 3}
    assert code0_nonzero > 0 and outside > 0
    assert {16, -16} <= comps and max(abs(v) for v in comps) <= M.RANGE + 1
    assert all(coded[k] == {True, False} for k in range(6)), coded
    assert clamp > 0 and level == 0
    assert 0 in deltas and any(d > 0 for d in deltas) and any(d < 0 for d in deltas)


@pytest.mark.parametrize("W,H", M.SHAPES)
def test_p_frames_are_shorter_than_i_frames_on_a_translation(W, H):
    """usefulness, as a condition: the pure full-pel translation, every P-frame against the I-frame of the same picture at the same q.
    (At 16x16 no vector but (0, 0) fits the rectangle: there the condition rests on the content being smooth, so that the difference to
    the frame before still costs less than the picture itself.)"""
    frames, qs, ch = encoded(W, H, "fullpel")
    for t in range(1, M.T):
        intra = E.host_encode(W, H, 2, frames[:, t], qs[:, t])
        assert int(ch[t]["bytes"][0]) < int(intra["bytes"][0]), (t, int(ch[t]["bytes"][0]), int(intra["bytes"][0]))


def test_refusals_need_no_device():
    from mobiclipdecoder_amd import encode_inter
    lib = encode_inter._lib()
    q, pq = np.array([12, 52, 30], np.uint8), np.array([52, 12, 30], np.uint8)
    F = 64 * 48 * 3 // 2

    def both(maxp=4, W=64, H=48, ver=2, n=3, pitch=F, rpitch=F, pqs=pq, qs=q, slot=4096):
        args = (maxp, W, H, ver, n, pitch, rpitch, pqs.ctypes.data if pqs is not None else None, qs.ctypes.data if qs is not None else None, slot)
        a, b = lib.mobi_enc_inter_check(*args), M.host().encp_host_check(*args)
        assert a == b
        return a
    assert both() == 0
    assert both(ver=0) == MOBI_E_VERSION and both(ver=3) == MOBI_E_VERSION
    for bad in (dict(W=60), dict(H=40), dict(W=0), dict(H=0), dict(W=1040), dict(maxp=0), dict(maxp=65536), dict(n=0), dict(n=5), dict(n=-1), dict(pitch=F - 8),
                dict(pitch=F + 4), dict(rpitch=F - 8), dict(rpitch=F + 4), dict(qs=None), dict(pqs=None), dict(qs=np.array([12, 11, 30], np.uint8)),
                dict(qs=np.array([53, 20, 30], np.uint8)), dict(pqs=np.array([12, 11, 30], np.uint8)), dict(pqs=np.array([12, 20, 53], np.uint8)), dict(slot=4094)):
        assert both(**bad) == MOBI_E_ARG, bad
    assert both(pitch=F + 8, rpitch=F + 16) == 0 and both(slot=0) == 0 and both(W=1024, pitch=1024 * 48 * 3 // 2, rpitch=1024 * 48 * 3 // 2) == 0
    assert lib.mobi_enc_inter_stream_bound(60, 48) == 0 and lib.mobi_enc_inter_stream_bound(64, 48) == M.host().encp_host_bound(64, 48)
    assert lib.mobi_enc_inter_create(0, 64, 48, 2, 0) is None and lib.mobi_enc_inter_create(4, 60, 48, 2, 0) is None and lib.mobi_enc_inter_create(4, 64, 48, 0, 0) is None
    assert lib.mobi_enc_inter(None, 1, None, 0, None, 0, None, None, None, 0, None, None, None) == MOBI_E_ARG
    assert lib.mobi_enc_inter_async(None, None, 1, None, 0, None, 0, None, None, None, 0, None, None, None) == MOBI_E_ARG


def test_stream_bound_holds():
    """>= every length seen, the hardest set included, and the stated sum: at most 14 header bits, per macroblock 3 + 2 * 13 + 13 bits of
    syntax (a vector difference is at most 2 * (RANGE + 1) in size, its se() 13 bits) and six blocks of 1 + 64 * 28 bits, 16 zero bits"""
    L = M.host()
    assert M.se_bits(2 * (M.RANGE + 1)) <= 13 and M.se_bits(-2 * (M.RANGE + 1)) <= 13 and M.se_bits(40) <= 13 and M.se_bits(-40) <= 13
    Tb = tables.load()
    assert max(int(Tb["mobi_part_bits"][v][0][c]) for v in (0, 1) for c in (0, 1)) <= 3
    for W, H in M.SHAPES:
        bound = L.encp_host_bound(W, H)
        assert bound % 4 == 0
        bits = 14 + (W // 16) * (H // 16) * (3 + 26 + 13 + 6 * (1 + 64 * 28)) + 16
        assert bound == ((bits + 15) // 16 * 2 + 3) // 4 * 4
        for name in M.SETS:
            assert max(int(encoded(W, H, name)[2][t]["bytes"].max()) for t in range(1, M.T)) <= bound
    # the hardest set: saturated noise against an unrelated reference at the lowest quantiser
    rng = np.random.default_rng(9)
    sat = M._saturated(rng, 48, 32)
    r = M.host_encode(48, 32, 2, sat[:2], sat[2:], [52, 12], [12, 12])
    assert r["bytes"].max() <= L.encp_host_bound(48, 32) and r["bytes"].min() > 0


def test_slot_too_small_is_zero_and_length_is_true():
    frames, qs, ch = encoded(48, 32, "mixed5")
    full = ch[1]
    small = (int(full["bytes"][0]) - 2) // 4 * 4
    assert full["bytes"][1:].max() <= small
    r = M.host_encode(48, 32, 2, frames[:, 1], ch[0]["recon"], qs[:, 0], qs[:, 1], slot_bytes=small)
    assert np.array_equal(r["bytes"], full["bytes"]) and not r["streams"][0].any()
    for i in range(1, 5):
        assert np.array_equal(r["streams"][i, : full["bytes"][i]], full["streams"][i, : full["bytes"][i]])


def test_pitches_and_threads():
    frames, qs, ch = encoded(48, 32, "mixed5")
    full, F = ch[2], frames.shape[2]
    wide, rwide = np.full((5, F + 24), 0x55, np.uint8), np.full((5, F + 40), 0x33, np.uint8)
    wide[:, :F], rwide[:, :F] = frames[:, 2], ch[1]["recon"]
    r = M.host_encode(48, 32, 2, wide, rwide, qs[:, 1], qs[:, 2], pitch=F + 24, ref_pitch=F + 40, threads=3)
    assert all(np.array_equal(r[k], full[k]) for k in ("streams", "bytes", "recon", "stats", "mbs", "mv", "mvp", "forms"))


def test_one_macroblock_has_one_candidate():
    """16x16: only (0, 0) fits the rectangle and no neighbour exists; an unchanged picture costs the syntax alone"""
    pic = np.full((1, 384), 77, np.uint8)
    for version, bits in ((2, 1 + 1 + 1 + 1), (1, 1 + 1 + 2 + 1)):  # 0, se(0), code 0 (1 bit / 2 bits), ue(0)
        r = M.host_encode(16, 16, version, pic, pic, [30], [30])
        assert r["mv"][0, 0] == 0 and r["mvp"][0, 0] == 0 and r["mbs"][0, 0]["cbp"] == 0
        assert np.array_equal(r["recon"], pic) and int(r["stats"]["bits"][0]) == bits and r["bytes"][0] == 4


def test_host_model_under_sanitizers(tmp_path):
    """tests/tools/enc_inter_host_main.cpp: a program of its own with -fsanitize=address,undefined (nothing sanitised is loaded into
    Python); its buffers are exactly one picture, one reference and one slot long, so a read outside a window's rectangle is reported"""
    exe = str(tmp_path / "enc_inter_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-variable", "-fwrapv", "-pthread", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I" + E.CSRC, os.path.join(E.TOOLS, "enc_inter_host_main.cpp"),
                    os.path.join(E.TOOLS, "mobi_encode_inter_host.cpp"), "-o", exe], check=True)
    for W, H in ((16, 16), (48, 32)):
        bound = M.host().encp_host_bound(W, H)
        for name in M.SETS:
            frames, qs, ch = encoded(W, H, name)
            n = frames.shape[0]
            for t in (1, 3):
                src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
                with open(src, "wb") as f:
                    f.write(qs[:, t - 1].tobytes() + qs[:, t].tobytes() + frames[:, t].tobytes() + ch[t - 1]["recon"].tobytes())
                p = subprocess.run([exe, str(W), str(H), "2", str(n), src, dst], capture_output=True, text=True)
                assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
                blob = np.fromfile(dst, np.uint8)
                assert np.array_equal(blob[: 4 * n].view(np.int32), ch[t]["bytes"])
                assert np.array_equal(blob[4 * n: 4 * n + n * bound].reshape(n, bound), ch[t]["streams"])
                assert np.array_equal(blob[4 * n + n * bound:].reshape(n, -1), ch[t]["recon"])
