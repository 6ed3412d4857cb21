"""The inter encoder's intra mode on the CPU (include/mobiclip_encode_pintra.h): the host model (tests/enc_pintra_model.py, the product's
csrc/mobi_encode_pintra.h) judged by the oracle, by its own stream read back with the oracle's tables, and by an independent
re-derivation of every decision.  No GPU.

  1  mode 0 equals the inter host model byte for byte: streams, lengths, reconstruction, statistics, records, vectors
  2  every stream of every set decodes in the oracle, chained behind its predecessors, to the model's reconstruction, within its length
  3  the re-derivation (enc_pintra_model.rederive: v* by brute force, Jp and Ji from tests/tools/txcode_ref.c's block coder, the decision
     with its tie, effective-vector predictors, bits, every statistics field) gives the model's decisions and figures
  4  the stream has code 6 exactly where the model's flag says, and the priced bits are the written bits
  5  a picture in which nothing is chosen intra is byte-identical to mode 0 with `reserved` all zero: every picture of `still`, and every
     picture of `fullpel` that chooses none.  (`fullpel`'s frames are one smooth function sampled at moving offsets, so a step brings new
     content in at an edge -- the third step moves 8 samples down -- and the rule sends those macroblocks intra: 3 of 6 macroblocks of
     picture 3 at 48x32, 1, 2 and 17 of 221 in pictures 1..3 at 272x208.  For those pictures the antecedent does not hold; the test
     requires that it does hold for `fullpel` wherever no content enters: all three pictures at 16x16, pictures 1 and 2 at 48x32.)
  6  on `cut`, every P-picture's stream is strictly shorter than mode 0's on the same reference at the same quantiser
  7  header, library and Python table name the same symbols; the stream bound is unchanged; the two modes refuse each other in both orders
  8  closed loop and parse-back at enc_model.GEOMETRY_SHAPES with `cut` and `uncover` as one batch of five, what the GPU comparison there
     rests on, and why: one workgroup's statistics and a carry dropped at macroblock 256 differ from the truth in every picture counted
  +  the conditions that make `cut` and `uncover` worth running, asserted on the model's output"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import enc_inter_model as M
from tests import enc_model as E
from tests import enc_pintra_model as PI
from tests import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOBI_E_ARG = -7
_CACHE = {}


def encoded(W, H, name, version=2, mode=1):
    key = (W, H, name, version, mode)
    if key not in _CACHE:
        frames, qs = PI.sequence_sets(W, H)[name]
        _CACHE[key] = (frames, qs, PI.chain(W, H, version, mode, frames, qs))
    return _CACHE[key]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return E.txref(tmp_path_factory.mktemp("encpi_txref"))


@pytest.mark.parametrize("version", PI.VERSIONS)
@pytest.mark.parametrize("W,H", PI.SHAPES)
def test_mode_0_is_the_inter_host_model(W, H, version):
    for name in ("fullpel", "mixed5"):
        frames, qs = PI.sequence_sets(W, H)[name]
        got, want = PI.chain(W, H, version, 0, frames, qs), M.chain(W, H, version, frames, qs)
        for t in range(1, PI.T):
            for k in ("streams", "bytes", "recon", "stats", "mbs", "mv", "mvp", "forms"):
                assert np.array_equal(got[t][k], want[t][k]), (name, t, k)
            assert not got[t]["stats"]["reserved"].any() and not got[t]["kind"].any()


@pytest.mark.parametrize("version", PI.VERSIONS)
@pytest.mark.parametrize("W,H", PI.SHAPES)
def test_closed_loop_through_the_oracle(W, H, version):
    for name in PI.SETS:
        frames, qs, ch = encoded(W, H, name, version)
        for c in range(frames.shape[0]):
            streams = [ch[t]["streams"][c, : ch[t]["bytes"][c]] for t in range(PI.T)]
            for t, (pic, used, q) in enumerate(M.oracle_chain(W, H, version, streams)):
                assert np.array_equal(pic, ch[t]["recon"][c]), (name, c, t)
                assert used <= len(streams[t]) and q == qs[c, t], (name, c, t)


@pytest.mark.parametrize("version", PI.VERSIONS)
@pytest.mark.parametrize("W,H", PI.SHAPES)
def test_streams_have_code_6_where_the_flag_says(W, H, version):
    intra_n = 0
    for name in PI.SETS:
        frames, qs, ch = encoded(W, H, name, version)
        for t in range(1, PI.T):
            r = ch[t]
            for c in range(frames.shape[0]):
                p = PI.parse_p_stream(r["streams"][c, : r["bytes"][c]], W, H, version)
                flag = PI.is_intra(r)[c]
                where = (name, t, c)
                assert np.array_equal(p["code"] == PI.CODE_INTRA, flag), where
                assert p["dq"] == int(qs[c, t]) - int(qs[c, t - 1]), where
                # the priced bits are the written bits, macroblock by macroblock and in total
                assert np.array_equal(p["mbs"]["bits"], r["mbs"]["bits"][c]), where
                assert p["end"] == int(r["stats"]["bits"][c]) and p["mv_bits"] == int(r["stats"]["mv_bits"][c]), where
                assert int(r["bytes"][c]) == (p["end"] + 16 + 15) // 16 * 2, where
                for f in ("cbp", "lev", "luma_mode", "chroma_mode"):
                    assert np.array_equal(p["mbs"][f], r["mbs"][f][c]), (where, f)
                # an inter macroblock's vector from the stream: predictor + difference; an intra one has none and counts as zero
                dx, dy = M.unpack_mv(r["mv"][c])
                pdx, pdy = M.unpack_mv(r["mvp"][c])
                inter = ~flag
                assert np.array_equal((p["ddx"] + pdx)[inter], dx[inter]) and np.array_equal((p["ddy"] + pdy)[inter], dy[inter]), where
                assert not dx[flag].any() and not dy[flag].any(), where
                assert np.array_equal(p["code"][inter], ((dx != pdx) | (dy != pdy))[inter]), where
                intra_n += int(flag.sum())
    assert intra_n > 0


def _median_of(a, mbw, mbh, i):
    """the median of left, top and top-right of macroblock i in a per-macroblock array, zeros outside the picture"""
    x, y = i % mbw, i // mbw
    at = lambda xx, yy: int(a[yy * mbw + xx]) if 0 <= xx < mbw and 0 <= yy < mbh else 0
    return M.med3(at(x - 1, y), at(x, y - 1), at(x + 1, y - 1))


def _rederive_sets(W, H):
    # the brute-force search is the slow part: at the largest shape the new sets only, where both kinds of macroblock meet
    return PI.NEW_SETS if W * H > 48 * 32 else PI.SETS


@pytest.mark.parametrize("version", PI.VERSIONS)
@pytest.mark.parametrize("W,H", PI.SHAPES)
def test_decisions_are_the_argmin_of_the_stated_costs(W, H, version, ref):
    ties = zeroed = 0
    for name in _rederive_sets(W, H):
        frames, qs, ch = encoded(W, H, name, version)
        for t in range(1, PI.T):
            r = ch[t]
            for c in range(frames.shape[0]):
                where = (name, t, c)
                d = PI.rederive(ref, W, H, version, qs[c, t - 1], qs[c, t], frames[c, t], ch[t - 1]["recon"][c], r["recon"][c])
                flag = PI.is_intra(r)[c]
                assert np.array_equal(d["Jp"], r["jp"][c]), where
                assert np.array_equal(d["intra"], flag), where
                ties += int((d["Ji"] == d["Jp"]).sum())
                dx, dy = M.unpack_mv(r["mv"][c])
                pdx, pdy = M.unpack_mv(r["mvp"][c])
                assert np.array_equal(d["dx"], dx) and np.array_equal(d["dy"], dy), where
                assert np.array_equal(d["pdx"], pdx) and np.array_equal(d["pdy"], pdy), where
                for f in ("cbp", "lev", "luma_mode", "chroma_mode", "bits"):
                    assert np.array_equal(d[f], r["mbs"][f][c]), (where, f)
                assert np.array_equal(d["recon"], r["recon"][c]), where
                for f, v in d["stats"].items():
                    assert np.array_equal(np.asarray(v), r["stats"][f][c]), (where, f, v, r["stats"][f][c])
                # where the zeroing matters: an inter macroblock whose predictor is not the median of the raw v*
                raw = np.array([[_median_of(a, W // 16, H // 16, i) for a in (d["raw_dx"], d["raw_dy"])] for i in range(len(flag))])
                zeroed += int((~flag & ((raw[:, 0] != pdx) | (raw[:, 1] != pdy))).sum())
    print(f"{W}x{H} version {version}: {ties} ties of Ji and Jp, {zeroed} inter macroblocks whose predictor the zeroing changed")
    if (W, H) != (16, 16):
        assert zeroed > 0


def _logical_bits(data):
    """a stream's bits in the order they are read: 16-bit little-endian words, most significant bit first"""
    return np.unpackbits(np.frombuffer(bytes(data), "<u2").byteswap().view(np.uint8))


REDERIVE_GEOMETRY = ((32, 80), (1024, 16))  # where the brute-force re-derivation is cheap enough: 10 and 64 macroblocks
# pictures of the 15 (three P-frame calls of five) that must hold an intra AND an inter macroblock at index >= 256 -- at one column: whose
# macroblocks 255 and 256 differ in kind --: one below, or at, what the model gives (9, 15 and 2 in both versions)
BOTH_KINDS_BEHIND_256 = {(272, 256): 8, (1024, 144): 15, (16, 4112): 2}


@pytest.mark.parametrize("version", PI.VERSIONS)
@pytest.mark.parametrize("W,H", E.GEOMETRY_SHAPES)
def test_geometry_shapes_through_the_oracle(W, H, version, ref):
    """enc_model.GEOMETRY_SHAPES and the five clips of `cut` and `uncover` as one batch: the oracle decodes I, P, P, P to the reported
    reconstructions within the streams' bytes; every P-frame reads back to the model's records, code 6 exactly where the flag says, its
    vectors from predictors whose neighbours do NOT wrap round the picture's edge and in which an intra neighbour counts as zero; and
    the batch meets what the GPU comparison at these shapes (tests/test_encode_pintra_geometry_gpu.py) rests on.

    The last part is shown to be what makes a device-only mistake visible, on the model's output alone: statistics summed over the first
    256 macroblocks only (one workgroup of mobi_encpi_finish instead of two) and a stream written with the running sum of the bit lengths
    restarted at macroblock 256 (a carry dropped between two scan rounds) both differ from the true ones in every picture counted, and the
    second still ends inside the true stream's length, so that nothing but a byte comparison would see it."""
    mbw, mbh = W // 16, H // 16
    nmb = mbw * mbh
    frames, qs = PI.geometry_set(W, H)
    n = frames.shape[0]
    assert n == 5
    ch = PI.chain(W, H, version, 1, frames, qs, threads=n)
    at = lambda a, x, y: int(a[y * mbw + x]) if 0 <= x < mbw and y >= 0 else 0
    for c in range(n):
        streams = []
        for t in range(PI.T):
            nb = int(ch[t]["bytes"][c])
            assert nb % 2 == 0 and nb <= ch[t]["streams"].shape[1] and not ch[t]["streams"][c, nb:].any()
            streams.append(ch[t]["streams"][c, :nb])
        for t, (dec, used, q) in enumerate(M.oracle_chain(W, H, version, streams)):
            assert np.array_equal(dec, ch[t]["recon"][c]), (c, t)
            assert q == int(qs[c, t]) and used <= len(streams[t]), (c, t)
        for t in range(1, PI.T):
            r, where = ch[t], (c, t)
            flag = PI.is_intra(r)[c]
            ps = PI.parse_p_stream(streams[t], W, H, version)
            assert ps["dq"] == int(qs[c, t]) - int(qs[c, t - 1]), where
            assert np.array_equal(ps["code"] == PI.CODE_INTRA, flag), where
            for f in ("lev", "bits", "cbp", "luma_mode", "chroma_mode"):
                assert np.array_equal(ps["mbs"][f], r["mbs"][c][f]), (where, f)
            assert ps["end"] == int(r["stats"]["bits"][c]) == ps["hdr_bits"] + int(r["mbs"]["bits"][c].sum()), where
            assert 8 * len(streams[t]) == (ps["end"] + 16 + 15) // 16 * 16, where
            dx, dy = np.zeros(nmb, np.int64), np.zeros(nmb, np.int64)
            pdx, pdy = np.zeros(nmb, np.int64), np.zeros(nmb, np.int64)
            for i in range(nmb):
                if flag[i]:  # no vector is sent, and the neighbours take it for zero
                    assert ps["ddx"][i] == 0 and ps["ddy"][i] == 0
                    continue
                x, y = i % mbw, i // mbw
                pdx[i] = M.med3(at(dx, x - 1, y), at(dx, x, y - 1), at(dx, x + 1, y - 1))
                pdy[i] = M.med3(at(dy, x - 1, y), at(dy, x, y - 1), at(dy, x + 1, y - 1))
                dx[i], dy[i] = pdx[i] + ps["ddx"][i], pdy[i] + ps["ddy"][i]
            mdx, mdy = M.unpack_mv(r["mv"][c])
            assert np.array_equal(dx, mdx) and np.array_equal(dy, mdy), where
            mpx, mpy = M.unpack_mv(r["mvp"][c])
            assert np.array_equal(pdx[~flag], mpx[~flag]) and np.array_equal(pdy[~flag], mpy[~flag]), where
            assert np.array_equal(ps["code"][~flag], ((dx != pdx) | (dy != pdy))[~flag].astype(np.int64)), where
            assert int(r["stats"]["mv_bits"][c]) == ps["mv_bits"], where
            if (W, H) in REDERIVE_GEOMETRY:
                d = PI.rederive(ref, W, H, version, qs[c, t - 1], qs[c, t], frames[c, t], ch[t - 1]["recon"][c], r["recon"][c])
                assert np.array_equal(d["intra"], flag) and np.array_equal(d["Jp"], r["jp"][c]), where
                assert np.array_equal(d["dx"], mdx) and np.array_equal(d["dy"], mdy) and np.array_equal(d["bits"], r["mbs"]["bits"][c]), where
                assert np.array_equal(d["recon"], r["recon"][c]), where
                for f, v in d["stats"].items():
                    assert np.array_equal(np.asarray(v), r["stats"][f][c]), (where, f)
    # ---- what the GPU comparison rests on ----
    counted = wide_diagonal = 0
    for t in range(1, PI.T):
        r = ch[t]
        flag, bits, total = PI.is_intra(r), r["mbs"]["bits"].astype(np.int64), r["stats"]["bits"].astype(np.int64)
        n_intra = r["stats"]["reserved"][:, PI.STAT_INTRA].astype(np.int64)
        assert np.array_equal(n_intra, flag.sum(1)) and (n_intra > 0).all(), t
        both = flag.any(1) & ~flag.all(1)
        if (W, H) in ((1024, 16), (16, 4112)):
            assert both.any(), t
        if (W, H) == (1024, 144):  # a diagonal that does not start at column 0 (x_lo = d - mbh + 1 > 0) with both kinds on it
            k = flag.reshape(n, mbh, mbw)
            for d in range(mbh, mbw + mbh - 1):
                xs = np.arange(d - mbh + 1, min(d, mbw - 1) + 1)
                on = k[:, d - xs, xs]
                wide_diagonal += int((on.any(1) & ~on.all(1)).sum())
        if nmb <= 256:
            print(f"{W}x{H} version {version} picture {t}: intra macroblocks {n_intra.tolist()}, both kinds {both.tolist()}")
            continue
        E.geometry_preconditions(bits, total, (W, H, version, "intra mode", t))
        front, behind = flag[:, :256], flag[:, 256:]
        assert (front.sum(1) > 0).all(), t  # the first workgroup of mobi_encpi_finish adds to reserved[STAT_INTRA] in every picture
        mixed = (flag[:, 255] != flag[:, 256]) if mbw == 1 else (behind.any(1) & ~behind.all(1))
        counted += int(mixed.sum())
        print(f"{W}x{H} version {version} picture {t}: intra in front of 256 {front.sum(1).tolist()}, behind {behind.sum(1).tolist()}, counted {mixed.tolist()}")
        # one workgroup's statistics are not the picture's
        hdr = total - bits.sum(1)
        assert (hdr + bits[:, :256].sum(1) != total).all(), t
        cb = np.array([[bin(int(v)).count("1") for v in row] for row in r["mbs"]["cbp"]])
        assert np.array_equal(cb.sum(1), r["stats"]["coded_blocks"])
        for c in range(n):
            if behind[c].any():
                assert front[c].sum() != n_intra[c]
            if mixed[c]:
                assert behind[c].any() and front[c].sum() != n_intra[c], (t, c)
                assert cb[c, :256].sum() != int(r["stats"]["coded_blocks"][c]), (t, c)
            # a carry dropped between the scan rounds: macroblocks from 256 on written where a sum restarted at zero puts them
            start = hdr[c] + np.concatenate([[0], np.cumsum(bits[c])[:-1]])
            dropped = np.concatenate([start[:256], np.concatenate([[0], np.cumsum(bits[c, 256:])[:-1]])])
            assert (dropped[256:] != start[256:]).all(), (t, c)
            true = _logical_bits(r["streams"][c, : r["bytes"][c]])
            wrong = np.zeros_like(true)
            wrong[: start[256]] = true[: start[256]]
            for i in range(256, nmb):
                wrong[dropped[i]: dropped[i] + bits[c, i]] |= true[start[i]: start[i] + bits[c, i]]
            assert not np.array_equal(wrong, true), (t, c)
            assert dropped[-1] + bits[c, -1] <= start[-1] + bits[c, -1] <= len(true), (t, c)  # and it stays inside the stream's own bytes
    if (W, H) in BOTH_KINDS_BEHIND_256:
        print(f"{W}x{H} version {version}: {counted} of {3 * n} pictures counted")
        assert counted >= BOTH_KINDS_BEHIND_256[(W, H)], counted
    if (W, H) == (1024, 144):
        print(f"{W}x{H} version {version}: {wide_diagonal} (picture, diagonal) pairs with x_lo > 0 and both kinds")
        assert wide_diagonal > 0


def test_pictures_without_intra_macroblocks_are_mode_0():
    none_in_fullpel = []
    for W, H in PI.SHAPES:
        for version in PI.VERSIONS:
            for name in ("still", "fullpel"):
                frames, qs, ch = encoded(W, H, name, version)
                for t in range(1, PI.T):
                    r = ch[t]
                    plain = M.host_encode(W, H, version, frames[:, t], ch[t - 1]["recon"], qs[:, t - 1], qs[:, t])
                    for c in range(frames.shape[0]):
                        if PI.is_intra(r)[c].any():
                            assert name == "fullpel", (W, H, version, name, t, c)  # `still` never chooses intra
                            continue
                        for k in ("streams", "bytes", "recon", "stats", "mbs", "mv", "mvp"):
                            assert np.array_equal(r[k][c], plain[k][c]), (W, H, version, name, t, c, k)
                        assert not r["stats"]["reserved"][c].any()
                        if name == "fullpel":
                            none_in_fullpel.append((W, H, version, t))
    for version in PI.VERSIONS:  # wherever no content enters the picture
        assert {(16, 16, version, 1), (16, 16, version, 2), (16, 16, version, 3), (48, 32, version, 1), (48, 32, version, 2)} <= set(none_in_fullpel)


def test_intra_shortens_every_picture_behind_a_cut():
    for W, H in PI.SHAPES:
        for version in PI.VERSIONS:
            frames, qs, ch = encoded(W, H, "cut", version)
            for t in range(1, PI.T):
                plain = M.host_encode(W, H, version, frames[:, t], ch[t - 1]["recon"], qs[:, t - 1], qs[:, t])
                print(f"{W}x{H} version {version} picture {t}: intra mode {ch[t]['bytes'].tolist()} bytes, mode 0 {plain['bytes'].tolist()}")
                assert (ch[t]["bytes"] < plain["bytes"]).all(), (W, H, version, t)
                assert (ch[t]["stats"]["reserved"][:, PI.STAT_INTRA] > 0).all()
            if (W, H) == (16, 16):
                assert all(PI.is_intra(ch[t]).all() for t in range(1, PI.T))  # its one macroblock goes intra


def test_coverage_conditions():
    """what `uncover` must show for the tests above and the GPU comparison to mean something"""
    for W, H in PI.SHAPES[1:]:
        mbw, mbh = W // 16, H // 16
        for version in PI.VERSIONS:
            frames, qs, ch = encoded(W, H, "uncover", version)
            modes, good = set(), 0
            for t in range(1, PI.T):
                for c in range(frames.shape[0]):
                    k = PI.is_intra(ch[t])[c].reshape(mbh, mbw)
                    modes |= set(ch[t]["mbs"]["luma_mode"][c][k.ravel()].tolist())
                    pad = np.zeros((mbh + 1, mbw + 2), bool)
                    pad[1:, 1:-1] = k
                    inter = ~k
                    left, top, tr = inter & pad[1:, :-2], inter & pad[:-1, 1:-1], inter & pad[:-1, 2:]
                    if k.any() and inter.any() and left.any() and top.any() and tr.any() and k[0].any() and k[:, 0].any():
                        good += 1
            print(f"{W}x{H} version {version}: {good} pictures with every neighbour condition, luma modes {sorted(modes)}")
            assert good > 0
            if (W, H) == PI.SHAPES[-1]:
                assert modes == {0, 1, 3}


def test_header_library_and_binding_agree():
    from mobiclipdecoder_amd import build, encode_inter
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobiclip_encode_pintra.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mobi_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(encode_inter._PINTRA_SIGS) == ["mobi_enc_inter_get_intra", "mobi_enc_inter_set_intra"]
    assert set(names) <= set(build.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "MOBI_ENC_PINTRA_STAT_INTRA = 2" in src
    assert encode_inter.STAT_INTRA == PI.STAT_INTRA == PI.host().encpi_host_stat_intra() == 2
    lib = encode_inter._lib()
    assert lib.mobi_enc_inter_set_intra(None, 1) == MOBI_E_ARG and lib.mobi_enc_inter_get_intra(None) == MOBI_E_ARG


def test_stream_bound_is_unchanged():
    """code 6 is 5 bits at 16x16 in both versions' tables (the figure csrc/mobi_encode_pintra.h's static_assert counts, and the one the model
    prices and writes): 5 + 13 + 6 bits in front of an intra macroblock's blocks against the 3 + 2 * 13 + 13 the inter bound counts"""
    L = PI.host()
    Tb = tables.load()
    for version in PI.VERSIONS:
        ver = 0 if version == 2 else 1
        nb = int(Tb["mobi_part_bits"][ver][0][PI.CODE_INTRA])
        assert nb == PI.CODE_INTRA_BITS == L.encpi_host_code_bits(version) == L.encpi_host_code_bits_bound()
        # the code word reads back as code 6 whatever follows it
        word, peek = L.encpi_host_code_word(version), 32 - int(Tb["mobi_part_shift"][ver][0])
        assert all(int(Tb["mobi_part_lut"][ver][0][word << (peek - nb) | rest]) == PI.CODE_INTRA for rest in range(1 << (peek - nb)))
    assert PI.CODE_INTRA_BITS + 13 + 6 <= 3 + 2 * 13 + 13
    for W, H in PI.SHAPES:
        bound = L.encpi_host_bound(W, H)
        assert bound == M.host().encp_host_bound(W, H)
        for name in PI.SETS:
            for version in PI.VERSIONS:
                ch = encoded(W, H, name, version)[2]
                assert ch[1]["streams"].shape[1] == bound and max(int(r["bytes"].max()) for r in ch[1:]) <= bound
    rng = np.random.default_rng(9)  # the hardest: saturated noise against an unrelated reference at the lowest quantiser
    sat = M._saturated(rng, 48, 32)
    r = PI.host_encode(48, 32, 2, 1, sat[:2], sat[2:], [52, 12], [12, 12])
    assert 0 < r["bytes"].min() and r["bytes"].max() <= L.encpi_host_bound(48, 32)


def test_the_two_modes_refuse_each_other():
    """the setters' rule (csrc/mobi_encode_pintra.h, mobi_encpi_set_mode; the entry points call nothing else): modes[0] = partitions,
    modes[1] = intra.  tests/test_encode_pintra_gpu.py repeats both orders on an encoder."""
    import ctypes as C
    L = PI.host()
    for first in (0, 1):
        modes = (C.c_int * 2)(0, 0)
        assert L.encpi_host_set_mode(modes, first, 1) == 0 and list(modes) == [1 - first, first]
        assert L.encpi_host_set_mode(modes, 1 - first, 1) == MOBI_E_ARG and list(modes) == [1 - first, first]  # refused, nothing changed
        assert L.encpi_host_set_mode(modes, 1 - first, 0) == 0 and list(modes) == [1 - first, first]  # turning the other OFF is fine
        assert L.encpi_host_set_mode(modes, first, 2) == MOBI_E_ARG and L.encpi_host_set_mode(modes, first, -1) == MOBI_E_ARG
        assert L.encpi_host_set_mode(modes, first, 0) == 0 and L.encpi_host_set_mode(modes, 1 - first, 1) == 0 and list(modes) == [first, 1 - first]
    # the host model refuses a mode it does not know, and what the inter check refuses
    pic = np.zeros((1, 384), np.uint8)
    q = np.array([30], np.uint8)
    out = np.zeros(4096, np.uint8)
    n = np.zeros(1, np.int32)
    call = lambda W, mode: L.encpi_host_inter(W, 16, 2, mode, 1, pic.ctypes.data, 384, pic.ctypes.data, 384, q.ctypes.data, q.ctypes.data, out.ctypes.data, 4096,
                                              n.ctypes.data, None, None, None, None, None, None, None, None, 1)
    assert call(16, 2) == MOBI_E_ARG and call(16, -1) == MOBI_E_ARG and call(12, 1) == MOBI_E_ARG and call(16, 1) == 0 and call(16, 0) == 0


def test_encode_clips_refuses_both_modes_before_anything_is_created():
    import inspect

    from mobiclipdecoder_amd import encode_inter
    assert inspect.signature(encode_inter.encode_clips).parameters["intra"].default is False
    assert inspect.signature(encode_inter.MobiclipInterEncoder.__init__).parameters["intra"].default is False
    src = inspect.getsource(encode_inter.encode_clips)
    assert src.index("partitions and intra") < src.index("MobiclipIntraEncoder(")  # the refusal stands in front of the first encoder
    with pytest.raises(ValueError):
        encode_inter.MobiclipInterEncoder(16, 16, 2, 1, partitions=True, intra=True)
