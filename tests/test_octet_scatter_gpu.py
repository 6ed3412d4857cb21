"""The scatter of mobi_recon_inter8's residual stage at the sizes where its code takes another path.

The level words of a macroblock are scattered by the eight lanes of its column, eight words per pass; how many passes an octet runs is
decided once from its largest word count (batches of 2, 3 and 4 words per lane, the words beyond the 128 that travel in registers in a
loop behind them), one packed round holds 24 coded areas, and an area whose coefficients are too large for 16-bit butterflies sends the
octet through the 32-bit rounds.  The streams here are WRITTEN DOWN (tests.test_residual_edges.Script with the motion rows of
tests.test_inter_addressing_gpu.TileScript): frame 0 a flat I-frame, frame 1 the predictions, frame 2 the case.  Pictures are 128x32 (one
full octet per macroblock row) and 80x32 (a short octet of five).

  words_*     level words per macroblock of 0, 1, 7, 8, 9, 16, 17, 127, 128, 129 and 384 mixed inside one octet, the octet's largest count
              in its first macroblock in one clip and in its last in another; octets whose largest count is 16, 17, 24, 25, 32, 33, 64, 65,
              96 and 97 (every batch boundary);
  areas_*     1, 15, 16, 17, 24, 25 and 48 (80x32: 30) coded areas per octet, all 8x8, all 4x4 and alternating by macroblock: an odd number
              of 8x8 areas (the empty slot) and none; 24 / 25 is the boundary of the packed round;
  fallback_*  one area above MOBI_PK_LIMIT in slot 0, in a slot >= 24 (found by the first round's sums, transformed in a later round), and
              in an octet that also holds a deeper tree and an intra macroblock;
  clamp_128   one clip whose frame 2 leaves the clamp table's domain among clean clips: MOBI_E_CLAMP for it and for no other.

CPU: every script has the word counts, coded areas and transform kinds its name claims, read from the host parser's descriptors
(MbDesc.w1, w2), and the number of slots that decides between the batched scatter (at most 24) and the general pass, so that no GPU case can
pass by missing its path.  GPU: every clip of a family as one batch, bit-exact against the oracle,
under both kinds of frame step.
"""
import functools

import numpy as np
import pytest

from tests import residual_model as rm
from tests.oracle_binding import OracleDecoder
from tests.test_inter_addressing_gpu import N_FRAMES, TileScript, _decode_all
from tests.test_residual_edges import E_CLAMP, E_INDEX, Q0, _block_for_sum, _coef, _place_even, _place_late_slot, _target, _tiny, kind_of_step  # noqa: F401  (kind_of_step: a fixture)

WORDS = [0, 1, 7, 8, 9, 16, 17, 127, 128, 129, 384]
BATCH_EDGES = [16, 17, 24, 25, 32, 33, 64, 65, 96, 97]  # the octet's largest count: 2 | 3 | 4 words per lane, then 8, 12, 16
AREAS = {128: [1, 15, 16, 17, 24, 25, 48], 80: [1, 15, 16, 17, 24, 25, 30]}
DEEP_MB, INTRA_MB, BIG_MB = 5, 2, (6, 2)  # (128x32, the third fall-back case)


def _level(p, a):
    return 1 if (p * 7 + a) % 3 else -1


def _put_words(s, mb, count, n4_areas=()):
    """`count` level words into macroblock `mb` of frame 2: areas filled in order, 64 words each (8x8, or four 4x4 blocks of 16)"""
    left = count
    for area in range(6):
        take, left = min(64, left), left - min(64, left)
        if not take:
            break
        if area in n4_areas:
            for sub in range(4):
                k = min(16, take - 16 * sub)
                if k > 0:
                    s.block(2, mb, area, 4, sub, [(p, _level(p, area + sub)) for p in range(k)])
        else:
            s.block(2, mb, area, 8, 0, [(p, _level(p, area)) for p in range(take)])


def _word_scripts(w):
    """-> [(name, script, claims)]; claims["ncoef"][mb] = level words of macroblock mb in frame 2"""
    nmb, out = w // 16, []

    def add(name, rows):
        s, ncoef = TileScript(w, 32), {}
        for row, counts in enumerate(rows):
            assert len(counts) == nmb
            for g, c in enumerate(counts):
                mb = row * nmb + g
                for sub in range(4):
                    s.flat(mb, 0, sub, 90 + 5 * g)  # (frame 1: predictions of their own, and 4x4 areas for its scatter)
                _put_words(s, mb, c, n4_areas=(1, 4) if g & 1 else ())
                ncoef[mb] = c
        out.append(("words_%d_%s" % (w, name), s, dict(ncoef=ncoef)))

    if nmb == 8:
        add("largest_first", [[384, 0, 1, 7, 8, 9, 16, 17], [129, 128, 127, 17, 9, 1, 0, 16]])
        add("largest_last", [[17, 16, 9, 8, 7, 1, 0, 384], [16, 0, 1, 9, 17, 127, 128, 129]])
    else:
        add("largest_first", [[384, 0, 17, 9, 128], [129, 1, 7, 8, 16]])
        add("largest_last", [[127, 16, 1, 0, 384], [8, 9, 17, 7, 129]])
    for i in range(0, len(BATCH_EDGES), 2):  # two octets per clip, the largest count in a macroblock of its own each time
        rows = []
        for k, top in enumerate(BATCH_EDGES[i:i + 2]):
            counts = [(top * (g + 1)) // (nmb + 2) for g in range(nmb)]  # smaller counts of every size around it
            counts[(i + 3 * k) % nmb] = top
            rows.append(counts)
        add("max_%d_%d" % tuple(BATCH_EDGES[i:i + 2]), rows)
    return out


def _area_scripts(w):
    """-> [(name, script, claims)]; claims["areas"][row] = (coded areas, 8x8 ones among them) of the octet of macroblock row `row`"""
    nmb, out = w // 16, []
    specs = [(n, kind) for kind in ("8", "4", "alt") for n in AREAS[w]]
    for i in range(0, len(specs), 2):
        s, areas = TileScript(w, 32), {}
        for row, (n_areas, kind) in enumerate(specs[i:i + 2]):
            n8 = 0
            for k in range(n_areas):
                g, area = k % nmb, k // nmb
                mb = row * nmb + g
                is8 = kind == "8" or (kind == "alt" and g % 2 == 0)
                n8 += is8
                for sub in range(4):
                    s.flat(mb, area, sub, 70 + 7 * g + 3 * area)
                dc = (3 + k % 5) * (1 if k & 1 else -1)
                if is8:
                    s.block(2, mb, area, 8, 0, [(0, dc), (1 + k % 30, 2 if k & 2 else -2)])
                else:
                    s.block(2, mb, area, 4, k % 4, [(0, dc), (1 + k % 14, 2 if k & 2 else -2)])
            areas[row] = (n_areas, n8)
        out.append(("areas_%d_%s" % (w, "_".join("%d%s" % sp for sp in specs[i:i + 2])), s, dict(areas=areas)))
    return out


def _fallback_scripts(w):
    """-> [(name, script, claims)]; claims["big"] = (macroblock, area, lowest slot it may have)"""
    big = _block_for_sum(20000, 8, 1, 3)
    assert int(np.abs(_coef(8, Q0, big)).sum()) > rm.pk_limit()
    out = []
    s = TileScript(w, 32)
    mb, area = _place_even(s)
    assert _target(s, mb, area, 8, 0, big, Q0, "valid")
    out.append(("fallback_%d_slot0" % w, s, dict(big=(mb, area, 0, 0))))
    if w == 128:
        s = TileScript(w, 32)
        mb, area = _place_late_slot(s)
        assert _target(s, mb, area, 8, 0, big, Q0, "valid")
        out.append(("fallback_%d_late_slot" % w, s, dict(big=(mb, area, 24, 47))))
        s = TileScript(w, 32)
        _tiny(s, 0, 0)
        _tiny(s, 7, 5, 4, 2)
        assert _target(s, BIG_MB[0], BIG_MB[1], 8, 0, big, Q0, "valid")
        s.block(2, INTRA_MB, 0, 8, 0, [(0, 5), (3, -2)], 1)
        s.motion.append([2, DEEP_MB, 3] + [1, 2, 2, 1] + [-3, 2, 0, 5] + [1, 0, 3, -2])  # four 8x8 leaves with vectors of their own
        out.append(("fallback_%d_deep_and_intra" % w, s, dict(big=(BIG_MB[0], BIG_MB[1], 0, 23), deep=DEEP_MB, intra=INTRA_MB)))
    return out


def _clamp_scripts(w):
    """clean clips around ONE whose frame 2 leaves the clamp table's domain (a sum of 320 or -65 in one 4x4 block)"""
    out = [x for x in _word_scripts(w)[:2]] + _area_scripts(w)[:1]
    s = TileScript(w, 32)
    mb, area = _place_even(s)
    assert _target(s, mb, area, 8, 0, _block_for_sum(rm.pk_limit() - 1, 8, -1, 2), Q0, "reject")
    out.insert(2, ("clamp_%d_reject" % w, s, dict(reject=True)))
    return out + _fallback_scripts(w)[:1]


FAMILIES = {"words_128": lambda: _word_scripts(128), "words_80": lambda: _word_scripts(80), "areas_128": lambda: _area_scripts(128), "areas_80": lambda: _area_scripts(80),
            "fallback_128": lambda: _fallback_scripts(128), "fallback_80": lambda: _fallback_scripts(80), "clamp_128": lambda: _clamp_scripts(128)}


@functools.lru_cache(maxsize=None)
def family(name):
    """-> (params, [(name, claims, data, frame_off)]): built once"""
    out, p = [], None
    for n, s, claims in FAMILIES[name]():
        p, (data, fo) = s.clip()
        out.append((n, claims, data, fo))
    return p, out


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """-> per clip, per frame (rc, Offset, y, uv): computed once, shared by the CPU and the GPU tests"""
    p, clips = family(name)
    out = []
    for _, _, data, fo in clips:
        o = OracleDecoder(p.width, p.height, p.version)
        out.append(_decode_all(o, data, fo))
        o.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def _slots(w1, nmb):
    """the kernel's slot order from the descriptors of one octet: 8x8 areas first, then (from an even slot) the areas of 4x4 blocks; inside
    a kind by area, then macroblock -> {(g, area): slot}"""
    coded = [(a, g) for a in range(6) for g in range(nmb) if not w1[g] & 1 and (w1[g] >> (8 + a)) & 1]
    is8 = lambda a, g: (w1[g] >> (14 + a)) & 1
    s8, s4 = [x for x in coded if is8(*x)], [x for x in coded if not is8(*x)]
    first4 = (len(s8) + 1) & ~1
    return {(g, a): k for k, (a, g) in enumerate(s8)} | {(g, a): first4 + k for k, (a, g) in enumerate(s4)}


def _n_slots(w1, nmb):
    """the kernel's n_slots of one octet: the 8x8 areas, rounded up to an even number, and the areas of 4x4 blocks behind them"""
    coded = [(w1[g] >> (14 + a)) & 1 for a in range(6) for g in range(nmb) if not w1[g] & 1 and (w1[g] >> (8 + a)) & 1]
    n8 = sum(coded)
    return ((n8 + 1) & ~1) + len(coded) - n8


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_scripts_have_the_counts_they_claim(name):
    """From the host parser's descriptors of frame 2 (MbDesc.w1: kind, coded areas, 8x8 transforms; w2: level words): what every script's
    name says.  The oracle decodes every frame of every clean script, and rejects frame 2 of the clamp case alone."""
    from tests.interp_binding import InterpDecoder
    p, clips = family(name)
    nmb = p.width // 16
    seen_counts, seen_tops, seen_areas, odd8, none8, kinds, paths = set(), set(), set(), 0, 0, set(), set()
    for (n, claims, data, fo), want in zip(clips, _oracle(name)):
        rcs = [r[0] for r in want]
        assert rcs == ([0, 0, E_INDEX] if claims.get("reject") else [0] * N_FRAMES), (n, rcs)
        if claims.get("reject"):
            continue
        assert not np.array_equal(want[1][2], want[2][2]), n
        d = InterpDecoder(p.width, p.height, p.version)
        for f in range(N_FRAMES):
            d.Data, d.Offset = data[: fo[f + 1]], int(fo[f])
            assert d.DecodeFrame() is not None, (n, f)
        desc = d.command_list()[0]
        d.close()
        w1, w2 = desc[:, 1].astype(np.int64), desc[:, 2].astype(np.int64)
        cbp = (w1 >> 8) & 63
        ncoef = np.where(cbp != 0, w2 & 0x3FF, 0)
        for mb, c in claims.get("ncoef", {}).items():
            assert not w1[mb] & 1 and ncoef[mb] == c, (n, mb, int(ncoef[mb]), c)
            seen_counts.add(c)
        if "ncoef" in claims:
            for r in range(2):  # one packed round holds the octet: its words go through the batches, not through the general pass
                assert _n_slots([int(x) for x in w1[r * nmb:(r + 1) * nmb]], nmb) <= 24, (n, r)
            seen_tops.update(int(ncoef[r * nmb:(r + 1) * nmb].max()) for r in range(2))
            seen_tops.update(("first" if int(ncoef[r * nmb:(r + 1) * nmb].argmax()) == 0 else "last" if int(ncoef[r * nmb:(r + 1) * nmb].argmax()) == nmb - 1 else "inside") for r in range(2))
        for row, (n_areas, n8) in claims.get("areas", {}).items():
            o = slice(row * nmb, (row + 1) * nmb)
            got = sum(bin(int(c)).count("1") for c in cbp[o]), sum(bin(int(c & t)).count("1") for c, t in zip(cbp[o], (w1[o] >> 14) & 63))
            assert got == (n_areas, n8), (n, row, got, (n_areas, n8))
            slots = _n_slots([int(x) for x in w1[o]], nmb)
            assert slots == ((n8 + 1) & ~1) + n_areas - n8 and (slots > 24) == (n_areas > 24), (n, row, slots)  # 24: the batches; 25: the general pass, two rounds
            paths.add(slots > 24)
            seen_areas.add(n_areas)
            odd8 += n8 & 1
            none8 += n8 == 0
            kinds.add("8" if n8 == n_areas else "4" if n8 == 0 else "both")
        if "big" in claims:
            mb, area, lo, hi = claims["big"]
            row, g = divmod(mb, nmb)
            slot = _slots([int(x) for x in w1[row * nmb:(row + 1) * nmb]], nmb)[(g, area)]
            assert lo <= slot <= hi, (n, slot)
            toks = [(t[3], t[4]) for t in FAMILIES[name]()[[c[0] for c in clips].index(n)][1].toks if t[0] == 2 and t[1] == mb and t[2] == area * 4]
            assert int(np.abs(_coef(8, Q0, toks)).sum()) > rm.pk_limit(), n
            others = [(t[1], t[2] // 4) for t in FAMILIES[name]()[[c[0] for c in clips].index(n)][1].toks if t[0] == 2 and (t[1], t[2] // 4) != (mb, area)]
            assert others, n  # (not alone in its octet)
        if "deep" in claims:
            m = claims["deep"]
            assert not w1[m] & 1 and (w1[m] >> 1) & 0x7F > 1 and (w1[m] >> 26) & 3 == 0, (n, hex(int(w1[m])))
            assert w1[claims["intra"]] & 1, n
    if name.startswith("words"):
        assert seen_counts >= set(WORDS) and seen_tops >= set(BATCH_EDGES) | {384, 129, "first", "last"}, (seen_counts, seen_tops)
    if name.startswith("areas"):
        assert seen_areas == set(AREAS[p.width]) and odd8 >= 4 and none8 >= 7 and kinds == {"8", "4", "both"} and paths == {False, True}, (seen_areas, odd8, none8, kinds, paths)
    if name.startswith("clamp"):
        assert sum(bool(c[1].get("reject")) for c in clips) == 1 and len(clips) >= 5


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_gpu_scatter_cases(name, kind_of_step):
    """the clips of a family as ONE batch, frame by frame: rc, Offset and both planes of every clip as the oracle's; the clip that leaves
    the clamp domain reports MOBI_E_CLAMP in frame 2, and no other clip of its batch does"""
    from mobiclipdecoder_amd import MobiclipBatch
    p, clips = family(name)
    want = _oracle(name)
    b = MobiclipBatch(len(clips), p.width, p.height, p.version)
    try:
        for f in range(N_FRAMES):
            rcs, offs = b.decode([d[fo[f]:fo[f + 1]] for _, _, d, fo in clips], [0] * len(clips))
            for k, (n, claims, _, fo) in enumerate(clips):
                if want[k][f][0] != 0:
                    assert claims.get("reject") and rcs[k] == E_CLAMP, (n, kind_of_step, f, rcs[k])
                    continue
                assert rcs[k] == 0 and offs[k] == want[k][f][1] - int(fo[f]), (n, kind_of_step, f, rcs[k], offs[k])
                y, uv = b.planes(k)
                assert np.array_equal(y, want[k][f][2]), (n, kind_of_step, f, "luma differs from the oracle", np.argwhere(y != want[k][f][2])[:4].tolist())
                assert np.array_equal(uv, want[k][f][3]), (n, kind_of_step, f, "chroma differs from the oracle", np.argwhere(uv != want[k][f][3])[:4].tolist())
    finally:
        b.close()
