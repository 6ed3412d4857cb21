"""The inter encoder's partition mode without a GPU (include/mobiclip_encode_parts.h; csrc/mobi_encode_parts.h run by
tests/tools/mobi_encode_parts_host.cpp, the host model the kernels are compared against in tests/test_encode_parts_gpu.py).

  1   header, library and the binding's table agree
  2   closed loop: the oracle decodes I, P, P, P of every chain to the model's reconstructions within the lengths reported
  3   parse-back with the oracle's tables: tree, leaf order, vectors, code 0 / 1 per leaf, cbp; the predictor is the median of the
      neighbours' last leaves
  4   an independent numpy re-derivation: every leaf's v* by brute force over its own candidate set, the tree from the stated costs and tie
      rules, prediction per quadrant, blocks, bits, statistics
  5   mode 0 is the existing host model byte for byte; in mode 1 an unsplit macroblock has its mode-0 vector
  6   the sets cover what they must (test_coverage_conditions)
  7   on the two-motion set mode 1 is strictly shorter than mode 0 at equal quantisers
  8   the bound; 9 the refusals; 10 the leaf predicate at 16x16 is mobi_encp_vector_ok; 11 the host model under sanitizers
  12  closed loop and parse-back at enc_model.GEOMETRY_SHAPES, with the still scene, and what the GPU comparison there rests on
Shapes 16x16 (sub-blocks have candidates the macroblock lacks), 48x32 (every edge), 64x48 (full reach, all three neighbours)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import enc_inter_model as M
from tests import enc_model as E
from tests import enc_parts_model as Q
from tests import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOBI_E_ARG = -7
_CACHE = {}


def encoded(W, H, name, version=2, mode=1):
    key = (W, H, name, version, mode)
    if key not in _CACHE:
        frames, qs = Q.sequence_sets(W, H)[name]
        _CACHE[key] = (frames, qs, Q.chain(W, H, version, mode, frames, qs))
    return _CACHE[key]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return E.txref(tmp_path_factory.mktemp("encq_txref"))


def _vectors(r, c):
    """picture c of a model's output: trees (M,), dx4, dy4 (M, 4)"""
    dx, dy = M.unpack_mv(r["mv4"][c])
    return r["mbs"]["luma_mode"][c].astype(int), dx, dy


def test_header_library_and_binding_agree():
    from mobiclipdecoder_amd import build, encode_inter
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobiclip_encode_parts.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mobi_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(encode_inter._PARTS_SIGS) and len(names) == 3
    assert set(names) <= set(build.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "MOBI_ENC_PARTS_STAT_SPLIT = 0" in src and "MOBI_ENC_PARTS_STAT_LEAVES = 1" in src
    assert (encode_inter.STAT_SPLIT, encode_inter.STAT_LEAVES) == (Q.STAT_SPLIT, Q.STAT_LEAVES) == (0, 1)


def test_code_8_spells_all_8x8():
    """all-8x8 is reachable through both roots; through code 8 it is never longer (9 against 10 bits on Moflex3DS, 11 against 11 on
    ModsDS), so with ties to code 8 the minimum never spells it through code 9: the model's eight partitions are distinct"""
    nb = tables.load()["mobi_part_bits"]
    got = [(int(nb[v][0][8]) + 2 * int(nb[v][1][9]), int(nb[v][0][9]) + 2 * int(nb[v][4][8])) for v in (0, 1)]
    assert got == [(9, 10), (11, 11)]
    for W, H in Q.SHAPES:
        for name in Q.SETS:
            for version in Q.VERSIONS:
                for r in encoded(W, H, name, version)[2][1:]:
                    assert set(r["mbs"]["luma_mode"].ravel().tolist()) <= set(Q.PARTITIONS)


@pytest.mark.parametrize("W,H", Q.SHAPES)
def test_closed_loop_through_the_oracle(W, H):
    for name in Q.SETS:
        for version in Q.VERSIONS:
            frames, qs, ch = encoded(W, H, name, version)
            for c in range(frames.shape[0]):
                streams = []
                for t in range(Q.T):
                    n = int(ch[t]["bytes"][c])
                    assert n % 2 == 0 and n <= ch[t]["streams"].shape[1]
                    assert not ch[t]["streams"][c, n:].any(), "zeros behind the stream"
                    streams.append(ch[t]["streams"][c, :n])
                for t, (dec, used, q) in enumerate(M.oracle_chain(W, H, version, streams)):
                    assert np.array_equal(dec, ch[t]["recon"][c]), (name, version, c, t)
                    assert q == int(qs[c, t]) and used <= len(streams[t]), (name, version, c, t)


@pytest.mark.parametrize("version", Q.VERSIONS)
@pytest.mark.parametrize("W,H", Q.SHAPES)
def test_streams_parse_back_to_the_models_decisions(W, H, version):
    mbw = W // 16
    for name in Q.SETS:
        frames, qs, ch = encoded(W, H, name, version)
        for c in range(frames.shape[0]):
            for t in range(1, Q.T):
                r, where = ch[t], (name, c, t)
                n = int(r["bytes"][c])
                ps = Q.parse_p_stream(r["streams"][c, :n], W, H, version)
                trees, dx4, dy4 = _vectors(r, c)
                assert ps["dq"] == int(qs[c, t]) - int(qs[c, t - 1]), where
                assert np.array_equal(ps["mbs"]["luma_mode"], trees), where
                assert np.array_equal(ps["mbs"]["cbp"], r["mbs"]["cbp"][c]) and np.array_equal(ps["mbs"]["lev"], r["mbs"]["lev"][c]), where
                assert np.array_equal(ps["mbs"]["bits"], r["mbs"]["bits"][c]), where
                # the decoder's walk: the predictor is the median of the neighbours' LAST leaves; every leaf adds its difference to it
                last = np.zeros((len(trees), 2), np.int64)
                at = lambda k, x, y: int(last[y * mbw + x, k]) if 0 <= x < mbw and y >= 0 else 0
                code0 = leaves = 0
                for i, lv in enumerate(ps["leaves"]):
                    x, y = i % mbw, i // mbw
                    px, py = (M.med3(at(k, x - 1, y), at(k, x, y - 1), at(k, x + 1, y - 1)) for k in (0, 1))
                    pdx, pdy = M.unpack_mv(r["mvp"][c, i: i + 1])
                    assert (px, py) == (int(pdx[0]), int(pdy[0])), where
                    want = [Q.LEAVES[l] for l in Q.tree_leaves(int(trees[i]))]
                    assert [f[:4] for f in lv] == want, (where, i)          # the tree's leaves in pblock's order
                    for (lx, ly, w, h, code, ddx, ddy) in lv:
                        qd = (ly // 8) * 2 + lx // 8
                        vx, vy = px + ddx, py + ddy
                        assert (vx, vy) == (int(dx4[i, qd]), int(dy4[i, qd])), (where, i)
                        assert code == int((ddx, ddy) != (0, 0)), (where, i)  # code 0 iff the vector is the predictor
                        for q2 in range(4):                                  # ... and every quadrant the leaf covers has it
                            if lx <= 8 * (q2 & 1) < lx + w and ly <= 8 * (q2 >> 1) < ly + h:
                                assert (vx, vy) == (int(dx4[i, q2]), int(dy4[i, q2]))
                        last[i] = (vx, vy)
                        code0 += code == 0
                        leaves += 1
                    ldx, ldy = M.unpack_mv(r["mv"][c, i: i + 1])
                    assert tuple(last[i]) == (int(ldx[0]), int(ldy[0])) == (int(dx4[i, 3]), int(dy4[i, 3])), where  # the bottom-right quadrant
                st = r["stats"][c]
                assert int(st["mv_bits"]) == ps["mv_bits"] and int(st["bits"]) == ps["end"] == ps["hdr_bits"] + int(ps["mbs"]["bits"].sum()), where
                assert 8 * n == (ps["end"] + 16 + 15) // 16 * 16, where
                assert int(st["code0"]) == code0 and int(st["reserved"][Q.STAT_LEAVES]) == leaves, where
                assert int(st["reserved"][Q.STAT_SPLIT]) == int((trees != 0).sum()) and not st["reserved"][2:].any(), where


@pytest.mark.parametrize("version", Q.VERSIONS)
@pytest.mark.parametrize("W,H", E.GEOMETRY_SHAPES)
def test_geometry_shapes_through_the_oracle(W, H, version):
    """enc_model.GEOMETRY_SHAPES in mode 1, the mixed five and the still scene: the oracle decodes I, P, P, P to the reported reconstructions
    within the streams' bytes; every P-frame reads back to the model's trees, leaves and vectors, the predictors from neighbours that do
    not wrap round the picture's edge; and the sets meet what the GPU comparison at these shapes rests on"""
    mbw, nmb = W // 16, (W // 16) * (H // 16)
    for name in M.GEOMETRY_SETS:
        frames, qs = M.geometry_set(W, H, name)
        ch = Q.chain(W, H, version, 1, frames, qs)
        split = 0
        for c in range(frames.shape[0]):
            streams = []
            for t in range(Q.T):
                n = int(ch[t]["bytes"][c])
                assert n % 2 == 0 and n <= ch[t]["streams"].shape[1] and not ch[t]["streams"][c, n:].any()
                streams.append(ch[t]["streams"][c, :n])
            for t, (dec, used, q) in enumerate(M.oracle_chain(W, H, version, streams)):
                assert np.array_equal(dec, ch[t]["recon"][c]), (name, c, t)
                assert q == int(qs[c, t]) and used <= len(streams[t]), (name, c, t)
            for t in range(1, Q.T):
                r, where = ch[t], (name, c, t)
                ps = Q.parse_p_stream(streams[t], W, H, version)
                trees, dx4, dy4 = _vectors(r, c)
                assert ps["dq"] == int(qs[c, t]) - int(qs[c, t - 1]), where
                assert np.array_equal(ps["mbs"]["luma_mode"], trees), where
                for f in ("lev", "bits", "cbp"):
                    assert np.array_equal(ps["mbs"][f], r["mbs"][c][f]), (where, f)
                assert ps["end"] == int(r["stats"]["bits"][c]) == ps["hdr_bits"] + int(r["mbs"]["bits"][c].sum()), where
                assert 8 * len(streams[t]) == (ps["end"] + 16 + 15) // 16 * 16, where
                last = np.zeros((nmb, 2), np.int64)
                at = lambda k, x, y: int(last[y * mbw + x, k]) if 0 <= x < mbw and y >= 0 else 0
                pdx, pdy = M.unpack_mv(r["mvp"][c])
                code0 = 0
                for i, lv in enumerate(ps["leaves"]):
                    x, y = i % mbw, i // mbw
                    px, py = (M.med3(at(k, x - 1, y), at(k, x, y - 1), at(k, x + 1, y - 1)) for k in (0, 1))
                    assert (px, py) == (int(pdx[i]), int(pdy[i])), (where, i)
                    assert [f[:4] for f in lv] == [Q.LEAVES[l] for l in Q.tree_leaves(int(trees[i]))], (where, i)
                    for (lx, ly, w, h, code, ddx, ddy) in lv:
                        qd = (ly // 8) * 2 + lx // 8
                        assert (px + ddx, py + ddy) == (int(dx4[i, qd]), int(dy4[i, qd])) and code == int((ddx, ddy) != (0, 0)), (where, i)
                        last[i] = (px + ddx, py + ddy)
                        code0 += code == 0
                assert int(r["stats"]["code0"][c]) == code0 and int(r["stats"]["mv_bits"][c]) == ps["mv_bits"], where
                assert int(r["stats"]["reserved"][c][Q.STAT_SPLIT]) == int((trees != 0).sum()), where
                split += int((trees != 0).sum())
        for t in range(1, Q.T):
            if name == "still":
                # nothing moves: no macroblock is split, each is 2 (Moflex3DS) or 3 (ModsDS) bits, and the stream is mode 0's
                assert (ch[t]["mbs"]["bits"] == (2 if version == 2 else 3)).all() and (ch[t]["stats"]["code0"] == nmb).all(), t
                assert np.array_equal(ch[t]["recon"], ch[0]["recon"]) and np.array_equal(frames[:, t], ch[0]["recon"]), t
                m0 = M.host_encode(W, H, version, frames[:, t], ch[t - 1]["recon"], qs[:, t - 1], qs[:, t])
                assert np.array_equal(m0["bytes"], ch[t]["bytes"]) and np.array_equal(m0["streams"], ch[t]["streams"][:, : m0["streams"].shape[1]]), t
            elif nmb > 256:
                E.geometry_preconditions(ch[t]["mbs"]["bits"], ch[t]["stats"]["bits"], (W, H, version, "parts", t))
        assert (split == 0) == (name == "still"), (name, split)
        if name == "still":
            dq = qs[:, 1:].astype(int) - qs[:, :-1]
            assert (dq != 0).any(1).sum() == 1 and (dq == 0).all(1).sum() == 2


@pytest.mark.parametrize("W,H", Q.SHAPES)
def test_decisions_are_the_argmin_of_the_stated_cost(W, H, ref):
    for name in Q.SETS:
        for version in Q.VERSIONS:
            frames, qs, ch = encoded(W, H, name, version)
            for c in range(frames.shape[0]):
                for t in range(1, Q.T):
                    r, where, q = ch[t], (name, version, c, t), int(qs[c, t])
                    reference = ch[t - 1]["recon"][c]
                    cost, bdx, bdy = Q.search_leaves(W, H, q, E.planes(frames[c, t].astype(np.int64), W, H)[0], E.planes(reference.astype(np.int64), W, H)[0])
                    trees, dx4, dy4 = _vectors(r, c)
                    for i in range(len(trees)):
                        tree = Q.decide_tree(version, q, cost[i])
                        assert tree == trees[i], (where, i)
                        for qd in range(4):
                            l = Q.leaf_of_quadrant(tree, qd)
                            assert (int(bdx[i, l]), int(bdy[i, l])) == (int(dx4[i, qd]), int(dy4[i, qd])), (where, i, qd)
                    d = Q.rederive_blocks(ref, W, H, q, frames[c, t], reference, dx4, dy4)
                    assert np.array_equal(d["cbp"], r["mbs"]["cbp"][c]) and np.array_equal(d["lev"], r["mbs"]["lev"][c]), where
                    assert np.array_equal(d["recon"], r["recon"][c]), where
                    st = r["stats"][c]
                    assert (int(st["fallback_clamp"]), int(st["fallback_level"])) == (d["clamp"], d["range"]), where
                    assert int(st["coded_blocks"]) == sum(bin(int(v)).count("1") for v in d["cbp"]), where
                    assert int(st["sad"]) == int(np.abs(frames[c, t].astype(np.int64) - r["recon"][c]).sum()), where
                    # nonzero and half-pel LEAVES, the bits behind the syntax
                    lv = [(int(dx4[i, (Q.LEAVES[l][1] // 8) * 2 + Q.LEAVES[l][0] // 8]), int(dy4[i, (Q.LEAVES[l][1] // 8) * 2 + Q.LEAVES[l][0] // 8]))
                          for i in range(len(trees)) for l in Q.tree_leaves(int(trees[i]))]
                    assert int(st["nonzero_mv"]) == sum(v != (0, 0) for v in lv) and int(st["halfpel_mv"]) == sum((v[0] | v[1]) & 1 for v in lv), where
                    inv = {int(cb): k for k, cb in reversed(list(enumerate(tables.load()["mobi_cbp_inter"])))}
                    syntax = r["mbs"]["bits"][c].astype(np.int64) - d["bits"] - np.array([E._ue_bits(inv[int(cb)]) for cb in d["cbp"]])
                    assert int(syntax.sum()) == int(st["mv_bits"]), where


@pytest.mark.parametrize("W,H", Q.SHAPES + ((272, 208),))
def test_mode_0_is_the_existing_model_and_unsplit_macroblocks_keep_their_vector(W, H):
    for name in M.SETS:
        frames, qs = M.sequence_sets(W, H)[name]
        for version in Q.VERSIONS:
            old, new = M.chain(W, H, version, frames, qs), Q.chain(W, H, version, 0, frames, qs)
            for t in range(1, Q.T):
                assert all(np.array_equal(old[t][k], new[t][k]) for k in ("streams", "bytes", "recon", "stats", "mbs", "mv", "mvp", "forms")), (name, version, t)
                assert not new[t]["stats"]["reserved"].any() and np.array_equal(new[t]["mv4"], np.repeat(new[t]["mv"][:, :, None], 4, 2))
                assert Q.host().encq_host_bound(W, H, 0) == M.host().encp_host_bound(W, H) == new[t]["streams"].shape[1]
    if (W, H) in Q.SHAPES:
        for name in Q.SETS:
            frames, qs, ch = encoded(W, H, name)
            for t in range(1, Q.T):  # the same reference for both modes: mode 1's chain
                m0 = Q.host_encode(W, H, 2, 0, frames[:, t], ch[t - 1]["recon"], qs[:, t - 1], qs[:, t])
                unsplit = ch[t]["mbs"]["luma_mode"] == 0
                assert np.array_equal(ch[t]["mv"][unsplit], m0["mv"][unsplit]), (name, t)


def test_coverage_conditions():
    """Asserted on the model's output over all sets and shapes, for each version: each of the eight partitions chosen; a leaf whose vector
    is not valid for its whole macroblock; a code-0 leaf with a nonzero vector; a leaf with each half-pel phase; a chroma quadrant with an
    odd chroma component; a macroblock whose last leaf differs from its first, next to a macroblock whose predictor therefore differs
    from what the first leaf would give."""
    for version in Q.VERSIONS:
        parts, phases = set(), set()
        beyond = code0_nonzero = odd_chroma = last_matters = 0
        for W, H in Q.SHAPES:
            mbw, mbh = W // 16, H // 16
            for name in Q.SETS:
                frames, qs, ch = encoded(W, H, name, version)
                for t in range(1, Q.T):
                    r = ch[t]
                    for c in range(frames.shape[0]):
                        trees, dx4, dy4 = _vectors(r, c)
                        pdx, pdy = M.unpack_mv(r["mvp"][c])
                        parts |= set(trees.tolist())
                        first = np.stack([dx4[:, 0], dy4[:, 0]], 1)
                        last = np.stack([dx4[:, 3], dy4[:, 3]], 1)
                        for i in range(len(trees)):
                            x, y = i % mbw, i // mbw
                            for l in Q.tree_leaves(int(trees[i])):
                                qd = (Q.LEAVES[l][1] // 8) * 2 + Q.LEAVES[l][0] // 8
                                vx, vy = int(dx4[i, qd]), int(dy4[i, qd])
                                phases.add((vx & 1) | (vy & 1) << 1)
                                beyond += not M.vector_ok(W, H, x, y, vx, vy)
                                code0_nonzero += (vx, vy) == (int(pdx[i]), int(pdy[i])) and (vx, vy) != (0, 0)
                                odd_chroma += ((vx >> 1) | (vy >> 1)) & 1
                            # the neighbours A of macroblock i (left, top, top-right) with first != last: would i's predictor move?
                            nb = [(x - 1, y), (x, y - 1), (x + 1, y - 1)]
                            vec = lambda a, xy: a[xy[1] * mbw + xy[0]] if 0 <= xy[0] < mbw and 0 <= xy[1] < mbh else np.zeros(2, np.int64)
                            for k, xy in enumerate(nb):
                                if 0 <= xy[0] < mbw and 0 <= xy[1] < mbh and tuple(vec(first, xy)) != tuple(vec(last, xy)):
                                    vs = [vec(first, p) if j == k else vec(last, p) for j, p in enumerate(nb)]
                                    other = tuple(M.med3(int(vs[0][d]), int(vs[1][d]), int(vs[2][d])) for d in (0, 1))
                                    last_matters += other != (int(pdx[i]), int(pdy[i]))
        assert parts == set(Q.PARTITIONS), (version, parts)
        assert phases == {0, 1, 2, 3}
        assert beyond > 0 and code0_nonzero > 0 and odd_chroma > 0 and last_matters > 0, (version, beyond, code0_nonzero, odd_chroma, last_matters)


def test_partitions_shorten_the_two_motion_streams():
    """usefulness, as a condition: at equal quantisers the mode-1 streams of the two-motion set are strictly shorter in total than the
    mode-0 streams of the same pictures (each chain on its own reconstructions), at every shape and for both versions"""
    for W, H in Q.SHAPES:
        for version in Q.VERSIONS:
            ch1, ch0 = encoded(W, H, "two_motion", version, 1)[2], encoded(W, H, "two_motion", version, 0)[2]
            b1, b0 = (sum(int(r["bytes"].sum()) for r in ch[1:]) for ch in (ch1, ch0))
            s1, s0 = (sum(int(r["stats"]["sad"].sum()) for r in ch[1:]) for ch in (ch1, ch0))
            print(f"{W}x{H} version {version}: mode 0 {b0} bytes, SAD {s0}; mode 1 {b1} bytes, SAD {s1}")
            assert b1 < b0, (W, H, version, b1, b0)


def test_stream_bound_holds():
    """>= every length seen, and the stated sum: at most 14 header bits; per macroblock 4 + 2 * 4 bits of split codes, four leaves of
    4 + 2 * 13 bits, 13 of ue(cbp) and six blocks of 1 + 64 * 28 bits; 16 zero bits"""
    L = Q.host()
    nb = tables.load()["mobi_part_bits"]
    assert max(int(nb[v][s][c]) for v in (0, 1) for s in (0, 1, 4, 5) for c in (0, 1)) <= 4
    assert max(int(nb[v][s][c]) for v in (0, 1) for s, c in ((0, 8), (0, 9), (1, 9), (4, 8))) <= 4
    assert L.encq_host_bound(60, 48, 1) == 0 and L.encq_host_bound(64, 48, 2) == 0 and L.encq_host_bound(64, 48, -1) == 0
    for W, H in Q.SHAPES:
        bound = L.encq_host_bound(W, H, 1)
        bits = 14 + (W // 16) * (H // 16) * (4 + 2 * 4 + 4 * (4 + 26) + 13 + 6 * (1 + 64 * 28)) + 16
        assert bound % 4 == 0 and bound == ((bits + 15) // 16 * 2 + 3) // 4 * 4 and bound >= L.encq_host_bound(W, H, 0)
        for name in Q.SETS:
            for version in Q.VERSIONS:
                ch = encoded(W, H, name, version)[2]
                assert ch[1]["streams"].shape[1] == bound and max(int(r["bytes"].max()) for r in ch[1:]) <= bound
    rng = np.random.default_rng(9)  # the hardest: saturated noise against an unrelated reference at the lowest quantiser
    sat = M._saturated(rng, 48, 32)
    r = Q.host_encode(48, 32, 2, 1, sat[:2], sat[2:], [52, 12], [12, 12])
    assert 0 < r["bytes"].min() and r["bytes"].max() <= L.encq_host_bound(48, 32, 1)


def test_refusals_need_no_device():
    from mobiclipdecoder_amd import encode_inter
    lib = encode_inter._lib()
    assert lib.mobi_enc_inter_set_partitions(None, 1) == MOBI_E_ARG and lib.mobi_enc_inter_get_partitions(None) == MOBI_E_ARG
    for W, H, mode in ((64, 48, 0), (64, 48, 1), (16, 16, 1), (1024, 48, 1)):
        assert lib.mobi_enc_inter_stream_bound_partitions(W, H, mode) == Q.host().encq_host_bound(W, H, mode) > 0
    assert lib.mobi_enc_inter_stream_bound_partitions(64, 48, 0) == lib.mobi_enc_inter_stream_bound(64, 48)
    for W, H, mode in ((60, 48, 1), (64, 40, 1), (0, 0, 1), (1040, 48, 1), (64, 48, 2), (64, 48, -1)):
        assert lib.mobi_enc_inter_stream_bound_partitions(W, H, mode) == 0
    assert encode_inter.stream_bound(64, 48, partitions=True) == Q.host().encq_host_bound(64, 48, 1)
    # the host model refuses a mode it does not know, and what the inter check refuses
    pic = np.zeros((1, 384), np.uint8)
    q = np.array([30], np.uint8)
    out = np.zeros(4096, np.uint8)
    n = np.zeros(1, np.int32)
    call = lambda W, mode: Q.host().encq_host_inter(W, 16, 2, mode, 1, pic.ctypes.data, 384, pic.ctypes.data, 384, q.ctypes.data, q.ctypes.data, out.ctypes.data, 4096,
                                                     n.ctypes.data, None, None, None, None, None, None, None, 1)
    assert call(16, 2) == MOBI_E_ARG and call(16, -1) == MOBI_E_ARG and call(12, 1) == MOBI_E_ARG and call(16, 1) == 0


def test_leaf_predicate_at_16x16_is_the_macroblock_predicate():
    """over every macroblock and every vector a search can meet (and one beyond) of a small picture; and the re-derivation's restatement
    equals the product's predicate for every leaf"""
    L = Q.host()
    W, H = 48, 32
    for mby in range(H // 16):
        for mbx in range(W // 16):
            for dy in range(-Q.RANGE - 2, Q.RANGE + 3):
                for dx in range(-Q.RANGE - 2, Q.RANGE + 3):
                    want = L.encq_host_vector_ok(W, H, mbx, mby, dx, dy)
                    assert L.encq_host_leaf_ok(W, H, mbx * 16, mby * 16, 16, 16, dx, dy) == want == int(M.vector_ok(W, H, mbx, mby, dx, dy))
                    for (x, y, w, h) in Q.LEAVES[1:]:
                        got = L.encq_host_leaf_ok(W, H, mbx * 16 + x, mby * 16 + y, w, h, dx, dy)
                        assert got == int(Q.leaf_ok(W, H, mbx * 16 + x, mby * 16 + y, w, h, dx, dy))
                        assert got >= want  # a part of a window that fits, fits
    # 16x16: the macroblock has one candidate, Q0 may point up to 8 samples right and down
    assert [L.encq_host_vector_ok(16, 16, 0, 0, dx, 0) for dx in (0, 1, 2)] == [1, 0, 0]
    assert all(L.encq_host_leaf_ok(16, 16, 0, 0, 8, 8, d, d) for d in range(0, 17)) and not L.encq_host_leaf_ok(16, 16, 0, 0, 8, 8, 17, 0)
    assert not L.encq_host_leaf_ok(16, 16, 0, 0, 8, 8, -1, 0)


def test_host_model_under_sanitizers(tmp_path):
    """tests/tools/enc_parts_host_main.cpp: a program of its own with -fsanitize=address,undefined, linked statically (nothing sanitised is
    loaded into Python); its buffers are exactly one picture, one reference and one slot long, so a read outside a leaf's window is
    reported"""
    exe = str(tmp_path / "enc_parts_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-variable", "-fwrapv", "-pthread", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I" + E.CSRC, os.path.join(E.TOOLS, "enc_parts_host_main.cpp"),
                    os.path.join(E.TOOLS, "mobi_encode_parts_host.cpp"), "-o", exe], check=True)
    for W, H in ((16, 16), (48, 32)):
        for mode in (1, 0):
            bound = Q.host().encq_host_bound(W, H, mode)
            for name in ("mixed5", "two_motion", "half_seams"):
                frames, qs, ch = encoded(W, H, name, 2, mode)
                n = frames.shape[0]
                for t in (1, 3):
                    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
                    with open(src, "wb") as f:
                        f.write(qs[:, t - 1].tobytes() + qs[:, t].tobytes() + frames[:, t].tobytes() + ch[t - 1]["recon"].tobytes())
                    p = subprocess.run([exe, str(W), str(H), "2", str(mode), str(n), src, dst], capture_output=True, text=True)
                    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
                    blob = np.fromfile(dst, np.uint8)
                    assert np.array_equal(blob[: 4 * n].view(np.int32), ch[t]["bytes"])
                    assert np.array_equal(blob[4 * n: 4 * n + n * bound].reshape(n, bound), ch[t]["streams"])
                    assert np.array_equal(blob[4 * n + n * bound:].reshape(n, -1), ch[t]["recon"])
