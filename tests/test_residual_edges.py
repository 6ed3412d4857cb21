"""The residual stage at its edges: the packed int16 limit of mobi_recon_inter8 (MOBI_PK_LIMIT) and the clamp table's domain [-64, 319].

The stream generator redraws every block until its residuals are within +-64 and draws |level| <= 24, so no generated stream comes near
either guard.  The streams here are WRITTEN DOWN (mobi_gen_clip_scripted: exact levels at exact scan positions, raw 12-bit tokens):

  frame 0   an I-frame without residual and with DC prediction only: every sample is 128;
  frame 1   the set-up frame: DC-only 4x4 blocks make the prediction of frame 2 -- any value 0..255, flat per 4x4 block.  (Predictions come
            from the stream, not from a debug hook that writes planes: the same bytes go to the oracle, the transliterated reference, the
            CPU interpreter and the PRODUCT library through every one of its parsers);
  frame 2   the case: a valid twin (prediction + residual touches -64 or 319 and stays inside: pixels are compared) or a reject twin (one
            4x4 block of predictions moved so that one sum is -65 or 320, or a sum whose int16-wrapped transform would look valid: the
            reference throws, the product answers MOBI_E_CLAMP);
  frame 3   copies frame 2 (frame-parallel groups have the reject in the middle).

CPU: the bound behind MOBI_PK_LIMIT checked with tests/residual_model.py (int64 against int16-wrapping butterflies), the oracle against the
transliterated reference and the CPU interpreter on every directed stream, and the verdict of every case.  GPU: every case against the
oracle under both kinds of step, one reject among clean clips of one batch, and a subset through every parser and entry point.
"""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

from mobiclipdecoder_amd.streamgen import BASE_SEED, default_params, generate_scripted
from tests import residual_model as rm
from tests.oracle_binding import OracleDecoder, lib as oracle_lib

W, H, VER = 128, 32, 1      # one octet per macroblock row, two rows (the wide cases: 256 x 32, two octets per row)
Q0 = 12                     # scales: 8x8 {18, 19, 20, 24, 25, 32}, 4x4 {40, 52, 64}: 20a + 19b reaches any sum
E_CLAMP, E_INDEX = -5, -1   # the product's MOBI_E_CLAMP; the oracle's (and the reference's) index fault
LO, HI = -64, 319           # the clamp table's domain (MobiConst.cs:587)
GAIN94 = [(1, 1), (1, 3), (3, 1), (3, 3), (1, 5), (5, 1), (1, 7), (7, 1), (3, 5), (5, 3), (5, 5), (7, 7)]  # odd row and odd column


def _coef(n, q, toks):
    """[(scan position, level)] -> dequantised coefficients in natural order"""
    c = np.zeros(n * n, np.int64)
    sc, z = rm.scales(q, n), rm.zz(n)
    for p, lev in toks:
        c[z[p]] = int(sc[p]) * lev
    return c


def _scan(n, row, col):
    return int(np.flatnonzero(rm.zz(n) == row * n + col)[0])


# ---------------------------------------------------------------------------------------------------------------- the bound (CPU)
def _differ(c, n):
    return (rm.idct(c, n) != rm.idct(c, n, True)).reshape(len(c), -1).any(1)


def _valid(res):
    """per-sample predictions 0..255 exist that keep every sum inside the domain"""
    r = res.reshape(len(res), -1)
    return (r.min(1) >= LO - 255) & (r.max(1) <= HI)


def _singles(n, total):
    c = np.zeros((2 * n * n, n * n), np.int64)
    for pos in range(n * n):
        c[2 * pos, pos], c[2 * pos + 1, pos] = total, -total
    return c


def _pairs(n, total):
    odd = [(r, k) for r in range(1, n, 2) for k in range(1, n, 2)]
    out = []
    for (a, b) in itertools.combinations(odd, 2):
        for first in (total // 2, total // 4):
            for sa, sb in itertools.product((1, -1), (1, -1)):
                c = np.zeros(n * n, np.int64)
                c[a[0] * n + a[1]], c[b[0] * n + b[1]] = sa * first, sb * (total - first)
                out.append(c)
    return np.array(out)


def _random_blocks(rng, n, count, total_lo, total_hi):
    """1..4 coefficients at random places and signs whose magnitudes add up to a total drawn from [total_lo, total_hi]"""
    k = rng.integers(1, 5, count)
    total = rng.integers(total_lo, total_hi + 1, count)
    share = rng.random((count, 4)) * (np.arange(4)[None, :] < k[:, None])
    mags = np.floor(share / share.sum(1, keepdims=True) * total[:, None]).astype(np.int64)
    mags[:, 0] += total - mags.sum(1)
    places = np.argsort(rng.random((count, n * n)), 1)[:, :4]
    c = np.zeros((count, n * n), np.int64)
    np.put_along_axis(c, places, mags * rng.choice((-1, 1), (count, 4)), 1)
    return c


def test_model_is_the_oracles_transform():
    """the int64 model against the oracle's unit entry points (which tests/test_unit_vectors.py pins to the reference's statements)"""
    OL = oracle_lib()
    rng = np.random.default_rng(3)
    for n, fn in ((8, OL.mobi_oracle_idct8), (4, OL.mobi_oracle_idct4)):
        c = _random_blocks(rng, n, 300, 1, 9000)
        res = rm.idct(c, n)
        for ci, ri in zip(c, res):
            if ri.min() < LO - 128 or ri.max() > HI - 128:
                continue
            dst = np.full(n * 16, 128, np.uint8)
            cc = np.ascontiguousarray(ci, np.int32)
            assert fn(cc.ctypes.data, n * n, dst.ctypes.data, dst.size, 0, 16) == 0
            assert np.array_equal(dst.reshape(n, 16)[:, :n], np.clip(128 + ri, 0, 255))


def test_packed_limit_is_below_the_first_wrap():
    """MOBI_PK_LIMIT checked instead of argued: at the limit the int16 butterflies give the int64 result for every single coefficient
    (64 + 16 places, both signs), every pair of gain-9/4 places (all signs, split 1:1 and 1:3) and 20 000 seeded blocks of 1..4
    coefficients.  The first sum at which a single coefficient or such a pair differs is S* (stated beside MOBI_PK_LIMIT and in
    DESIGN.md); it must lie above the limit."""
    limit = rm.pk_limit()
    rng = np.random.default_rng(14000)
    for n in (8, 4):
        assert not _differ(_singles(n, limit), n).any()
        assert not _differ(_pairs(n, limit), n).any()
        assert not _differ(_random_blocks(rng, n, 10000, limit, limit), n).any()
    s_star = first_wrap_sum()
    print("first-wrap sum S* = %d (MOBI_PK_LIMIT = %d, headroom %.1f %%)" % (s_star, limit, 100.0 * (s_star - limit) / limit))
    assert s_star > limit
    assert s_star == S_STAR_RECORDED, "update S_STAR_RECORDED, the comment at MOBI_PK_LIMIT and DESIGN.md"
    text = open(os.path.join(rm.ROOT, "DESIGN.md")).read() + open(os.path.join(rm.CSRC, "mobi_kernels.hip")).read()
    assert text.count(str(S_STAR_RECORDED)) >= 2


S_STAR_RECORDED = 14549


@functools.lru_cache(maxsize=None)
def first_wrap_sum():
    """smallest sum of |coefficient| at which int16 and int64 differ, over single coefficients and pairs of gain-9/4 places (8x8; a 4x4
    block first differs where its coefficient no longer fits int16)"""
    lo, hi = 8000, 33000
    sums = np.arange(lo, hi)
    best = hi
    for pos in range(64):
        for sg in (1, -1):
            c = np.zeros((len(sums), 64), np.int64)
            c[:, pos] = sg * sums
            d = _differ(c, 8)
            if d.any():
                best = min(best, int(sums[d.argmax()]))
    for total in range(best - 1, lo, -1):  # pairs: walk down from the singles' value while something still differs just below
        if not _differ(_pairs(8, total), 8).any():
            if not any(_differ(_pairs(8, t), 8).any() for t in range(total - 1, total - 40, -1)):
                break
        else:
            best = total
    return best


def test_no_valid_block_differs_in_int16():
    """Seeded search for a block that the reference decodes (every residual within reach of some prediction) and that the int16 butterflies
    get wrong, at sums from the limit to three times the limit: none.  The limit therefore guards REJECTED frames only: without it a
    frame the reference throws on could come back as pixels (the aliasing cases below), a valid frame could not come back wrong."""
    limit = rm.pk_limit()
    rng = np.random.default_rng(2718)
    n_diff = n_valid = 0
    for n in (8, 4):
        for _ in range(4):
            c = _random_blocks(rng, n, 25000, limit, 3 * limit)
            a, b = rm.idct(c, n), rm.idct(c, n, True)
            d = (a != b).reshape(len(c), -1).any(1)
            v = _valid(a)
            n_diff += int(d.sum())
            n_valid += int(v.sum())
            assert not (d & v).any(), c[(d & v).argmax()]
    print("int16 != int64 in %d of 200000 blocks, %d valid, none both" % (n_diff, n_valid))
    assert n_diff > 1000 and n_valid > 1000


# ---------------------------------------------------------------------------------------------------------------- scripts
class Script:
    def __init__(self, w=W, h=H):
        self.w, self.h, self.mbs, self.toks, self.qdelta = w, h, {}, [], [0, 0, 0, 0]

    def block(self, frame, mb, area, n, sub, toks, intra=0, form=0):
        m = self.mbs.setdefault((frame, mb), [frame, mb, intra, 0, 0, 0, 0, 0, 0, 0, 0])
        assert m[2] == intra
        m[3] |= 1 << area
        if n == 8:
            m[4] |= 1 << area
        else:
            m[5 + area] |= 1 << sub
        self.toks += [(frame, mb, area * 4 + (sub if n == 4 else 0), p, lev, form) for p, lev in toks]

    def flat(self, mb, area, sub, value):
        """set-up frame: the 4x4 block becomes `value` (from 128)"""
        r = int(value) - 128
        if r:
            s = int(rm.scales(Q0, 4)[0])
            lev = -((32 - 64 * r) // s)
            assert (s * lev + 32) >> 6 == r
            self.block(1, mb, area, 4, sub, [(0, lev)])

    def clip(self, q=Q0):
        p = default_params("A", BASE_SEED + 77, width=self.w, height=self.h, version=VER, n_frames=4, quantizer=Q0, cbp_prob=0, intra_dc_only=1)
        qd = list(self.qdelta)
        qd[2] += q - Q0
        qd[3] -= q - Q0
        return p, generate_scripted(p, list(self.mbs.values()), self.toks, qd)


def _dc_level(n, q, r):
    """DC level whose uniform residual (c00 + 32) >> 6 is r"""
    s = int(rm.scales(q, n)[0])
    lev = -((32 - 64 * r) // s)
    assert (s * lev + 32) >> 6 == r, (n, q, r)
    return lev


def _preds(res, n, verdict):
    """predictions flat per 4x4 block for the residuals of one block: "valid" -> every sum inside, touching 319 or -64 where it can;
    "reject" -> the same with ONE 4x4 block moved so that its extreme sum is 320 or -65.  None where no such predictions exist."""
    out, moved = [], False
    for qd in range(4 if n == 8 else 1):
        r = res[(qd >> 1) * 4:(qd >> 1) * 4 + 4, (qd & 1) * 4:(qd & 1) * 4 + 4] if n == 8 else res
        lo, hi = int(r.min()), int(r.max())
        a, b = max(0, LO - lo), min(255, HI - hi)
        if verdict == "reject" and not moved:
            if 0 <= HI + 1 - hi <= 255:
                out.append(HI + 1 - hi)
                moved = True
                continue
            if 0 <= LO - 1 - lo <= 255:
                out.append(LO - 1 - lo)
                moved = True
                continue
        if a > b:
            return None
        out.append(b if HI - hi <= 255 else a)
    return out if verdict == "valid" or moved else None


@functools.lru_cache(maxsize=None)
def _block_for_sum(total, n, sign, k, both=True):
    """k coefficients at gain-9/4 places and DC whose |coefficient| add up to `total` exactly at quantizer 12 and whose residuals allow
    both twins: [(scan position, level)] (seeded search)"""
    rng = np.random.default_rng(total * 8 + n + k)
    sc = rm.scales(Q0, n)
    places = [_scan(n, r, c) for r, c in GAIN94 if r < n and c < n]
    for _ in range(4000):
        # k - 1 gain-9/4 places, then DC (scale 20; its share moves every residual alike) and one place of scale 19: 20a + 19b reaches any rest
        pos = [int(p) for p in rng.choice(places, k - 1, replace=False)] + [0, int(rng.choice((1, 2)))]
        s = [int(sc[p]) for p in pos]
        sa, sb = s[-2:]  # 8x8: 20 and 19; 4x4: 40 and 52 (sums that are multiples of 4)
        share = rng.dirichlet(np.ones(k)) * total * rng.random()
        lev = [max(1, int(share[i] / s[i])) for i in range(k - 1)]
        rest = total - sum(a * b for a, b in zip(lev, s))
        b = np.arange(1, 20)  # (a small odd-scale coefficient: it is there to make the sum exact)
        ok = ((rest - sb * b) % sa == 0) & (rest - sb * b > 0)
        if not ok.any():
            continue
        b = int(rng.choice(b[ok]))
        lev += [(rest - sb * b) // sa, b]
        if max(lev) > 2047 or min(lev) < 1:
            continue
        toks = [(p, int(v) * (sign if i == 0 else int(rng.choice((-1, 1))))) for i, (p, v) in enumerate(zip(pos, lev))]
        c = _coef(n, Q0, toks)
        assert int(np.abs(c).sum()) == total
        res = rm.idct(c[None], n)[0]
        if _preds(res, n, "valid") and (not both or _preds(res, n, "reject")):
            return tuple(toks)
    raise AssertionError(("no block with both twins", total, n))


@functools.lru_cache(maxsize=None)
def _aliasing():
    """single coefficients whose int16-wrapped transform keeps 128 + residual inside the domain although the true one does not: what comes
    back as pixels if the switch to 32-bit rounds is missed.  -> [(n, quantizer, scan position, level, |coefficient|)], at least one of
    them above 65535 (the saturating term of the per-area sum)"""
    found = []
    for n, q, places in ((8, 12, GAIN94[:4]), (8, 24, GAIN94[:6]), (8, 36, GAIN94[:4] + [(0, 0), (0, 1)]), (4, 12, [(1, 1), (1, 3)]), (4, 30, [(1, 1), (3, 3), (0, 0)]), (8, 48, [(0, 0), (1, 1)])):
        sc = rm.scales(q, n)
        for r, c in places:
            p = _scan(n, r, c)
            lev = np.concatenate((np.arange(32, 2048), -np.arange(32, 2049)))
            co = np.zeros((len(lev), n * n), np.int64)
            co[:, r * n + c] = int(sc[p]) * lev
            a, b = rm.idct(co, n).reshape(len(lev), -1), rm.idct(co, n, True).reshape(len(lev), -1)
            hit = ((128 + b.min(1) >= LO) & (128 + b.max(1) <= HI)) & ((128 + a.min(1) < LO) | (128 + a.max(1) > HI)) & (np.abs(co).sum(1) > rm.pk_limit())
            big = np.flatnonzero(hit & (np.abs(co).sum(1) > 65535))
            for i in list(np.flatnonzero(hit)[:1]) + list(big[:1]):
                found.append((n, q, p, int(lev[i]), int(abs(int(sc[p]) * lev[i]))))
    found.sort(key=lambda a: -a[4])
    return found[:2] + found[2::2][:10]  # the two largest and a spread of the others


def _tiny(s, mb, area, n=8, sub=0, frame=2):
    s.block(frame, mb, area, n, sub, [(0, 4 if (mb + area) & 1 else -4)])


# placements of ONE large area in an octet (each a code path of stage C); -> (macroblock, area) of the target
def _place_even(s):      # slot 0: the low half of a pair tile
    _tiny(s, 1, 0)
    return 0, 0


def _place_odd(s):       # slot 1: the high half
    _tiny(s, 0, 0)
    return 1, 0


def _place_alone(s):     # alone among tiny areas of both kinds: the other seven macroblocks go through the 32-bit rounds with it
    for mb in range(8):
        if mb != 3:
            _tiny(s, mb, mb % 4, 8 if mb & 1 else 4, mb % 3)
            _tiny(s, mb, 4 + (mb & 1))
    return 3, 2


def _place_odd_n8(s):    # three 8x8 areas (slot 3 stays empty) in front of 4x4 areas; the target is the third
    _tiny(s, 0, 0)
    _tiny(s, 1, 0)
    for mb in (4, 5, 6):
        _tiny(s, mb, 1, 4, 2)
    return 2, 0


def _place_late_slot(s):  # 32 coded areas, the target in the last slot: beyond the first scatter of 24
    for mb in range(8):
        for a in range(4):
            if (mb, a) != (7, 3):
                _tiny(s, mb, a)
    return 7, 3


def _place_u(s):
    _tiny(s, 2, 5)
    return 2, 4


def _place_v(s):
    _tiny(s, 5, 0)
    return 5, 5


def _place_late_words(s):  # 192 level words in front of the target's: 128 travel in registers, the target's do not
    for a in range(3):
        s.block(2, 6, a, 8, 0, [(p, 1 if (p * 7 + a) % 3 else -1) for p in range(64)])
    return 6, 3


def _place_second_row(s):  # the octet of the second macroblock row
    _tiny(s, 8, 0)
    return 12, 1


PLACEMENTS = [_place_even, _place_odd, _place_alone, _place_odd_n8, _place_late_slot, _place_u, _place_v, _place_late_words, _place_second_row]


def _target(s, mb, area, n, sub, toks, q, verdict, intra=0, pred=None):
    """the target block into frame 2 and its predictions into frame 1; -> False where the verdict cannot be had"""
    res = rm.idct(_coef(n, q, toks)[None], n)[0]
    pr = [pred] * 4 if pred is not None else _preds(res, n, verdict)
    if pr is None:
        return False
    for qd, v in enumerate(pr[:4 if n == 8 else 1]):
        s.flat(mb, area, qd if n == 8 else sub, v)
    s.block(2, mb, area, n, sub, toks, intra)
    return True


@functools.lru_cache(maxsize=None)
def cases():
    """-> [dict(name, family, verdict, q, script)]"""
    out = []

    def add(name, family, verdict, s, q=Q0):
        out.append(dict(name=name, family=family, verdict=verdict, q=q, script=s))

    limit, s_star = rm.pk_limit(), first_wrap_sum()
    sums = [limit - 1, limit, limit + 1, s_star - 1, s_star, s_star + 1, 20000]
    # ---- family A: the packed limit.  Every sum x placement, both twins; n = 8 (a 4x4 block's coefficients are their own bound)
    for i, total in enumerate(sums):
        for j, place in enumerate(PLACEMENTS):
            toks = _block_for_sum(total, 8, 1 if (i + j) & 1 else -1, 2 + (i + j) % 2)
            for verdict in ("valid", "reject"):
                s = Script()
                mb, area = place(s)
                assert _target(s, mb, area, 8, 0, toks, Q0, verdict)
                add("A_sum%d_%s_%s" % (total, place.__name__[7:], verdict), "A", verdict, s)
    # a 4x4 area whose four blocks are each below the limit while the area's sum is above it
    for total in (4 * (limit // 4 + 100) // 4 * 4, 20000):  # (4x4 scales at quantizer 12 are multiples of 4)
        assert total > limit and total // 4 < limit and total % 16 == 0
        for verdict in ("valid", "reject"):
            s = Script()
            _tiny(s, 0, 0)
            for sub in range(4):
                part = total // 4 + (1200 if sub == 2 else -400)  # (the block that is moved out needs a residual of 65 at least)
                assert _target(s, 4, 1, 4, sub, _block_for_sum(part, 4, 1 if sub & 1 else -1, 2, sub == 2), Q0, "reject" if verdict == "reject" and sub == 2 else "valid")
            add("A_area4x4_sum%d_%s" % (total, verdict), "A", verdict, s)
    # aliasing sums: rejects by construction (prediction 128 everywhere), each in two placements
    al = _aliasing()
    assert len(al) >= 8 and max(a[4] for a in al) > 65535, al
    for i, (n, q, p, lev, mag) in enumerate(al):
        light = [pl for pl in PLACEMENTS if pl is not _place_late_words]  # (its dense filler areas are written for quantizer 12)
        for place in (light[i % len(light)], light[(i + 3) % len(light)]):
            s = Script()
            mb, area = place(s)
            assert _target(s, mb, area, n, 1, [(p, lev)], q, "reject", pred=128)
            add("A_alias%d_n%d_q%d_p%d_c%d_%s" % (i, n, q, p, mag if lev > 0 else -mag, place.__name__[7:]), "A", "reject", s, q)
    # single coefficients at the gain-9/4 places: rejects only (a residual of +-(9/4 * 14000 / 64) has no prediction)
    for total, pos in ((limit, (1, 1)), (s_star, (1, 1)), (20000, (3, 3))):
        s = Script()
        mb, area = _place_even(s)
        lev = total // int(rm.scales(Q0, 8)[_scan(8, *pos)])
        assert _target(s, mb, area, 8, 0, [(_scan(8, *pos), -lev)], Q0, "reject", pred=128)
        add("A_single%d_reject" % total, "A", "reject", s)
    # ---- family B: the clamp domain, exactly.  DC-only blocks: the residual is uniform
    big = _block_for_sum(20000, 8, 1, 3)  # a self-contained large area in the same octet: forces the 32-bit rounds

    def edge(name, mb, area, n, sub, intra=0, wide=False, q=Q0):
        for total, verdict in ((LO, "valid"), (LO - 1, "reject"), (HI, "valid"), (HI + 1, "reject")):
            s = Script()
            r = -74 if total < 0 else 74
            if wide:
                assert _target(s, 6, 2, 8, 0, big, Q0, "valid")
            if intra:  # DC prediction = the mean of the row above and the column to the left: both flat
                for m2, a2 in ((mb - 8, 2), (mb - 8, 3), (mb - 1, 1), (mb - 1, 3), (mb - 9, 3)):
                    for sub2 in range(4):
                        s.flat(m2, a2, sub2, total - r)
                for sub2 in range(4):  # (what the macroblock itself held does not matter: say so by making it something else)
                    s.flat(mb, area, sub2, 77)
                if area >= 4:
                    for m2 in (mb - 8, mb - 1, mb - 9):
                        for sub2 in range(4):
                            s.flat(m2, area, sub2, total - r)
                s.block(2, mb, area, n, sub, [(0, _dc_level(n, q, r))], 1)
            else:
                for sub2 in (range(4) if n == 8 else [sub]):
                    s.flat(mb, area, sub2, total - r)
                s.block(2, mb, area, n, sub, [(0, _dc_level(n, q, r))])
            add("B_%s_at%d_%s" % (name, total, verdict), "B", verdict, s, q)

    edge("packed_A_8x8_luma", 0, 0, 8, 0)
    edge("packed_B_8x8_luma", 1, 3, 8, 0)
    edge("packed_4x4_luma", 2, 1, 4, 3)
    edge("packed_8x8_U", 3, 4, 8, 0)
    edge("packed_4x4_V", 4, 5, 4, 2)
    edge("packed_8x8_V_row1", 13, 5, 8, 0)
    edge("wide_8x8_luma", 0, 0, 8, 0, wide=True)
    edge("wide_4x4_luma", 7, 2, 4, 1, wide=True)
    edge("wide_8x8_U", 3, 4, 8, 0, wide=True)
    edge("wide_4x4_V", 5, 5, 4, 0, wide=True)
    edge("intra_8x8_luma", 9, 0, 8, 0, intra=1)
    edge("intra_4x4_luma", 10, 0, 4, 0, intra=1)
    edge("intra_8x8_U", 11, 4, 8, 0, intra=1)
    edge("intra_4x4_V", 12, 5, 4, 0, intra=1)
    # The intra kernel tracks the range of its 8x8 steps in the two halves of a packed pair: even samples of a row in one, odd samples in the
    # other.  A uniform residual puts every sample on the edge at once; here the extreme sits in columns of ONE parity only (DC plus the
    # highest horizontal frequency), so that each half of the pair has to see it on its own.
    for parity, l7 in (("even", -9), ("odd", 9)):
        for total, verdict in ((LO, "valid"), (LO - 1, "reject"), (HI, "valid"), (HI + 1, "reject")):
            mb, toks = 9, [(0, -230 if total < 0 else 230), (_scan(8, 7, 0), l7 if total < 0 else -l7)]
            res = rm.idct(_coef(8, Q0, toks)[None], 8)[0]
            ext = res.min() if total < 0 else res.max()
            cols = np.unique(np.nonzero(res == ext)[1])
            assert (cols % 2 == (parity == "odd")).all(), (parity, res)  # (the other columns are at least one step inside)
            assert 0 <= total - int(ext) <= 255
            s = Script()
            for m2, a2 in ((mb - 8, 2), (mb - 1, 1)):
                for sub2 in range(4):
                    s.flat(m2, a2, sub2, total - int(ext))
            s.block(2, mb, 0, 8, 0, toks, 1)
            add("B_intra_8x8_%s_columns_at%d_%s" % (parity, total, verdict), "B", verdict, s)
    # a residual that does not fit int16 before the shift (raw 12-bit level at quantizer 52): truncated to int16 it would be small and
    # the sum inside; saturated (or in int32) it is far outside.  With its valid twin: the same path with a level that fits.
    for n, mb, area in ((8, 2, 0), (4, 5, 3), (8, 6, 4)):
        sc = int(rm.scales(52, n)[0])
        lev = next(v for v in range(33, 2048) if abs(rm._w16(np.int64(sc * v))) < 2000 and sc * v > 40000)
        fits = next(v for v in range(1, 40) if (sc * v + 32) >> 6 >= 64)  # prediction + residual = 319 with a prediction <= 255
        for verdict, level, pred in (("reject", lev, 128), ("reject", -lev, 128), ("valid", fits, None)):
            s = Script()
            r = (sc * level + 32) >> 6
            for sub2 in range(4):
                s.flat(mb, area, sub2, pred if pred is not None else HI - r)
            s.block(2, mb, area, n, 1 if n == 4 else 0, [(0, level)], form=3)
            add("B_q52_n%d_area%d_level%d_%s" % (n, area, level, verdict), "B", verdict, s, 52)
    for intra_mb in (9,):  # the same through the intra kernel (its residuals are stored as saturated int16)
        sc = int(rm.scales(52, 8)[0])
        lev = next(v for v in range(33, 2048) if abs(rm._w16(np.int64(sc * v))) < 2000 and sc * v > 40000)
        s = Script()
        s.block(2, intra_mb, 0, 8, 0, [(0, lev)], 1)
        add("B_q52_intra_level%d_reject" % lev, "B", "reject", s, 52)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


N_EXPECTED = {("A", "valid"): 7 * 9 + 2, ("A", "reject"): 7 * 9 + 2 + 2 * len(_aliasing()) + 3, ("B", "valid"): 14 * 2 + 4 + 3, ("B", "reject"): 14 * 2 + 4 + 6 + 1}


@functools.lru_cache(maxsize=None)
def _stream(i):
    c = cases()[i]
    p, (data, fo) = c["script"].clip(c["q"])
    return p, data, fo


def _decode_all(dec, data, fo, n=4):
    """-> per frame (rc, Offset, y, uv)"""
    rows = []
    for f in range(n):
        dec.Data, dec.Offset = data[: fo[f + 1]], int(fo[f])
        r = dec.DecodeFrame()
        rows.append((dec.last_error, dec.Offset, None if r is None else r[0], None if r is None else r[1]))
    return rows


@functools.lru_cache(maxsize=None)
def _oracle(i):
    p, data, fo = _stream(i)
    o = OracleDecoder(p.width, p.height, p.version)
    rows = _decode_all(o, data, fo)
    internal = np.ctypeslib.as_array(oracle_lib().mobi_oracle_internal(o.h), (392,)).copy()
    o.close()
    return rows, internal


def test_every_script_does_what_it_says():
    """Before any GPU is involved: the oracle decodes frames 0 and 1 of every case, frame 0 is flat 128, and frame 2 gets the scripted
    verdict -- rc 0 for a valid twin, the index fault for a reject.  The
    numbers of valid and reject cases per family are what the construction says."""
    count = {}
    for i, c in enumerate(cases()):
        rows, _ = _oracle(i)
        assert rows[0][0] == 0 and rows[1][0] == 0, c["name"]
        assert (rows[0][2][:, :c["script"].w] == 128).all() and (rows[0][3][:, :c["script"].w // 2] == 128).all(), c["name"]
        want = 0 if c["verdict"] == "valid" else E_INDEX
        assert rows[2][0] == want, (c["name"], rows[2][0])
        if want == 0:
            assert rows[3][0] == 0 and np.array_equal(rows[3][2], rows[2][2]), c["name"]
        count[(c["family"], c["verdict"])] = count.get((c["family"], c["verdict"]), 0) + 1
    print("directed cases:", sorted(count.items()))
    assert count == N_EXPECTED, (count, N_EXPECTED)


def test_oracle_equals_the_transliterated_reference_on_directed_streams():
    """The oracle has only ever seen |residual| <= 64 from the generator: its clamp path and its large-coefficient arithmetic against the
    mechanical transliteration of the reference (oracle/_ref, only where the reference's sources are): planes, Offset, rc, Internal[]."""
    from tests.test_csref_differential import _lib
    L = _lib()
    if L is None:
        pytest.skip("no transliterated reference here (it is generated beside the reference's sources)")
    L.csref_internal.restype = C.POINTER(C.c_uint32)
    L.csref_internal.argtypes = [C.c_void_p]
    for i, c in enumerate(cases()):
        p, data, fo = _stream(i)
        rows, internal = _oracle(i)
        h = L.csref_create(p.width, p.height, p.version)
        S = L.csref_stride(h)
        for f in range(4):
            buf = np.ascontiguousarray(data[: fo[f + 1]])
            off = C.c_int(int(fo[f]))
            rc = L.csref_decode(h, buf.ctypes.data, buf.size, C.byref(off))
            assert (rc != 0) == (rows[f][0] != 0) and off.value == rows[f][1], (c["name"], f, rc, rows[f][:2])
            if rc == 0:
                assert np.array_equal(np.ctypeslib.as_array(L.csref_y(h, 0), (p.height, S)), rows[f][2]), (c["name"], f)
                assert np.array_equal(np.ctypeslib.as_array(L.csref_uv(h, 0), (p.height // 2, S)), rows[f][3]), (c["name"], f)
        assert np.array_equal(np.ctypeslib.as_array(L.csref_internal(h), (392,)), internal), c["name"]
        L.csref_destroy(h)


def test_product_parser_and_kernel_arithmetic_on_the_cpu():
    """tests/interp_binding.InterpDecoder (the product's parser + the kernels' per-sample arithmetic on the CPU): the same planes, and
    MOBI_E_CLAMP exactly where the oracle throws."""
    from tests.interp_binding import InterpDecoder
    for i, c in enumerate(cases()):
        p, data, fo = _stream(i)
        rows, _ = _oracle(i)
        d = InterpDecoder(p.width, p.height, p.version)
        got = _decode_all(d, data, fo, 3)
        d.close()
        for f in range(3):
            assert got[f][0] == (E_CLAMP if rows[f][0] == E_INDEX else rows[f][0]), (c["name"], f, got[f][0], rows[f][0])
            if rows[f][0] == 0:
                assert got[f][1] == rows[f][1] and np.array_equal(got[f][2], rows[f][2]) and np.array_equal(got[f][3], rows[f][3]), (c["name"], f)


def test_the_writer_refuses_broken_scripts():
    p = default_params("A", BASE_SEED, width=W, height=H, version=VER, n_frames=3, quantizer=Q0)
    ok_mb, ok_tok = [1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 5, 0]
    generate_scripted(p, [ok_mb], [ok_tok])
    for mbs, toks in (([ok_mb], []),                                        # a coded block without a token
                      ([ok_mb], [ok_tok, [1, 0, 4, 0, 5, 0]]),              # a token for an area that is not coded
                      ([ok_mb], [ok_tok, ok_tok]),                          # one position twice
                      ([ok_mb], [[1, 0, 0, 0, 0, 0]]),                      # level 0
                      ([ok_mb], [[1, 0, 0, 0, 2048, 0]]),                   # beyond 12 bits
                      ([ok_mb], [[1, 0, 0, 64, 5, 0]]),
                      ([[0] + ok_mb[1:]], [[0] + ok_tok[1:]]),              # frame 0 is the I-frame
                      ([[1, 16, 0, 1, 1, 0, 0, 0, 0, 0, 0]], [[1, 16, 0, 0, 5, 0]])):
        with pytest.raises(ValueError):
            generate_scripted(p, mbs, toks)
    with pytest.raises(ValueError):
        generate_scripted(p, [ok_mb], [ok_tok], [0, 41, 0])


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(params=["one_launch", "two_launches"])
def kind_of_step(request, monkeypatch):
    """both kinds of frame step (MOBI_FUSED_STEP_MBS is read when a batch is created), as conftest.step_launches does for its modules"""
    if request.param == "two_launches":
        monkeypatch.setenv("MOBI_FUSED_STEP_MBS", "0")
    else:
        monkeypatch.delenv("MOBI_FUSED_STEP_MBS", raising=False)
    yield request.param


def _check_frame(name, f, rc, off, planes, want):
    assert rc == (E_CLAMP if want[0] == E_INDEX else want[0]), (name, f, rc, want[0])
    if want[0] == 0:
        assert off == want[1], (name, f, off, want[1])
        assert np.array_equal(planes[0], want[2]) and np.array_equal(planes[1], want[3]), (name, f, "pixels differ from the oracle")


def _run_batch(idx, device_parse=None, how="decode"):
    """the cases `idx` as the clips of ONE batch, frame by frame, against the oracle; -> (#valid, #reject) case frames seen"""
    from mobiclipdecoder_amd import MobiclipBatch
    streams = [_stream(i) for i in idx]
    want = [_oracle(i)[0] for i in idx]
    names = [cases()[i]["name"] for i in idx]
    p0 = streams[0][0]
    b = MobiclipBatch(len(idx), p0.width, p0.height, p0.version, device_parse=device_parse)
    frame = lambda f: [d[fo[f]:fo[f + 1]] for _, d, fo in streams]
    n_valid = n_reject = 0
    try:
        if how == "gop":
            rcs, offs = b.decode_gop([frame(0)])
            assert rcs == [[0] * len(idx)]
            rcs, offs = b.decode_gop([frame(1), frame(2), frame(3)])  # the reject sits in the middle frame of the group
            for k, i in enumerate(idx):
                for f in (1, 2, 3) if want[k][2][0] == 0 else (1, 2):
                    w = want[k][f]
                    _check_frame(names[k], f, rcs[f - 1][k], offs[f - 1][k], b.planes(k, 3 - f), (w[0], w[1] - int(streams[k][2][f]), w[2], w[3]))
                n_valid += want[k][2][0] == 0
                n_reject += want[k][2][0] != 0
            return n_valid, n_reject
        for f in range(3):
            if how == "submit":
                b.submit(frame(f), [0] * len(idx))
                rcs, offs = b.wait()
            else:
                rcs, offs = b.decode(frame(f), [0] * len(idx))
            for k in range(len(idx)):
                w = want[k][f]
                _check_frame(names[k], f, rcs[k], offs[k], b.planes(k), (w[0], w[1] - int(streams[k][2][f]), w[2], w[3]))
                if f == 2:
                    n_valid += w[0] == 0
                    n_reject += w[0] != 0
    finally:
        b.close()
    return n_valid, n_reject


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["A", "B"])
def test_gpu_directed_cases(family, kind_of_step):
    """Every directed case against the oracle -- planes, Offset, rc -- sixteen clips to a batch: a reject among clean clips in every step,
    so that fault[clip] is seen to be per clip as well."""
    idx = [i for i, c in enumerate(cases()) if c["family"] == family]
    # interleave valid and reject so that every batch holds both
    idx.sort(key=lambda i: (cases()[i]["name"].rsplit("_", 1)[0], cases()[i]["verdict"]))
    n_valid = n_reject = 0
    for k in range(0, len(idx), 16):
        v, r = _run_batch(idx[k:k + 16])
        n_valid += v
        n_reject += r
    print("family %s, %s: %d valid and %d reject cases decoded" % (family, kind_of_step, n_valid, n_reject))
    assert (n_valid, n_reject) == (N_EXPECTED[(family, "valid")], N_EXPECTED[(family, "reject")])


@pytest.mark.gpu
def test_gpu_one_reject_in_a_batch(kind_of_step):
    """Seven clips, one of them a reject: it alone reports MOBI_E_CLAMP, its neighbours in the same step are bit-exact."""
    by = {c["name"]: i for i, c in enumerate(cases())}
    limit = rm.pk_limit()
    clean = [by["A_sum%d_even_valid" % limit], by["B_packed_A_8x8_luma_at319_valid"], by["B_wide_4x4_V_at-64_valid"]]
    for bad in ("A_sum%d_odd_reject" % (limit + 1), "B_packed_4x4_luma_at320_reject", "B_intra_8x8_luma_at-65_reject", "A_single20000_reject"):
        assert _run_batch(clean + [by[bad]] + clean) == (6, 1)


def _subset():
    by = {c["name"]: i for i, c in enumerate(cases())}
    limit, s_star = rm.pk_limit(), first_wrap_sum()
    names = ["A_sum%d_even_valid" % limit, "A_sum%d_odd_reject" % limit, "A_sum%d_late_slot_valid" % (limit + 1), "A_sum%d_late_words_reject" % s_star,
             "A_sum20000_alone_valid", "A_sum20000_u_reject", "A_area4x4_sum20000_valid", "A_single%d_reject" % s_star,
             "B_packed_A_8x8_luma_at-64_valid", "B_packed_A_8x8_luma_at-65_reject", "B_wide_8x8_U_at319_valid", "B_wide_8x8_U_at320_reject",
             "B_intra_4x4_luma_at319_valid", "B_intra_4x4_luma_at320_reject", "B_intra_8x8_luma_at-64_valid", "B_intra_8x8_luma_at-65_reject"]
    names += [c["name"] for c in cases() if "_q52_" in c["name"]] + [c["name"] for c in cases() if "_alias" in c["name"]][::3]
    return [by[n] for n in names]


@pytest.mark.gpu
@pytest.mark.parametrize("way", ["host_parser", "mobi_parse_frames", "lockstep_parser", "frame_parallel_group", "submit_wait"])
def test_gpu_every_way_in(way, kind_of_step):
    """Family C: valid and reject cases of A and B through every parser and entry point; rc per frame and planes as the oracle's.  (Raw
    12-bit tokens are legal for every parser; a hand-over to the host parser is fine, a different answer is not.)"""
    idx = _subset()
    mode, how = {"host_parser": (False, "decode"), "mobi_parse_frames": (True, "decode"), "lockstep_parser": ("lockstep", "decode"),
                 "frame_parallel_group": ("lockstep", "gop"), "submit_wait": (True, "submit")}[way]
    v, r = _run_batch(idx, mode, how)
    want_v = sum(cases()[i]["verdict"] == "valid" for i in idx)
    print("family C, %s, %s: %d valid and %d reject cases" % (way, kind_of_step, v, r))
    assert (v, r) == (want_v, len(idx) - want_v) and v >= 8 and r >= 12
