"""The reference decoder's own motion against the command-list reading of it (csrc/mobi_motion.h), on the CPU.

tests/test_motion_field.py and tests/test_motion_export_gpu.py compare the export with tests/tools/libmobi_motionhost.so, a host build of the
header the kernel compiles: a misreading both share passes there.  Here the other side is the oracle's motion trace (oracle/mobi_oracle.h,
mobi_oracle_motion_trace): what the restated reference decoder hands to CopyBlock for every leaf and what ReadDCTMatrix reads for every
macroblock, written down where it happens, by code that knows neither the command list nor mobi_motion.h.  The header promises the canonical
member of a vector's class; that rule is applied to the trace below in numpy integers (canonical_cells), not by the header.

  every frame of every stream family: trace cells (canonical) == host_motion cells, trace mbs == host_motion mbs, all five values, exactly
  the scripted clips of tests/test_motion_field.py: the trace is the script (the trace itself is sane)

The stream families and their traces are shared with tests/test_motion_trace_gpu.py.
"""
import functools
import types

import numpy as np
import pytest

from mobiclipdecoder_amd.streamgen import BASE_SEED, default_params, generate_clip
from tests.gpu_streams import suite_params
from tests.oracle_binding import OracleDecoder
from tests.test_motion_field import N_FRAMES, WIDTHS, host_motion, scripted_case


def canonical_cells(cells, S):
    """include/mobiclip_hip.h, VECTORS: the member (dx - 4 t S, dy + 4 t) with -2 S <= dx < 2 S -> int64 [3, h, w]"""
    c = np.asarray(cells).astype(np.int64)
    t = np.floor_divide(c[0] + 2 * S, 4 * S)
    out = np.stack([c[0] - 4 * t * S, c[1] + 4 * t, c[2]])
    assert (out[0] >= -2 * S).all() and (out[0] < 2 * S).all() and ((out[0] - c[0]) % (4 * S) == 0).all()
    return out


def oracle_motion(p, data, fo, n_frames=None):
    """a clip through the oracle with the trace armed -> per frame (rc, raw cells int16 [3, H/2, W/2] or None, mbs int32 [5, H/16, W/16] or
    None), and the decoder's Stride"""
    o = OracleDecoder(p.width, p.height, p.version)
    out = []
    for f in range(len(fo) - 1 if n_frames is None else n_frames):
        o.Data, o.Offset = data[: fo[f + 1]], int(fo[f])
        _, cells, mbs = o.DecodeFrameTraced()
        out.append((o.last_error, cells, mbs))
    S = o.Stride
    o.close()
    return out, S


# ---------------------------------------------------------------------------------------------------------------- the stream families
def _generated(ps):
    return [(p,) + tuple(generate_clip(p)) for p in ps]


def _deep_params(cfg, seed, w, h, **kw):
    """test_deeper_trees_cell_by_cell's parameters (tests/test_gpu_parity.py)"""
    args = dict(n_frames=7, width=w, height=h, pm_deep=900, pm_split1=50, pm_skip=20, pm_intra=10, pm_multiref=500)
    args.update(kw)
    return default_params(cfg, seed, **args)


def _far_clips():
    """tests/test_parse_fallback.py::test_far_motion_vectors_travel's frames as clips of two frames"""
    from tests.test_parse_fallback import _DC_MB, _frame, _part_code, _se_code, _ue_code
    out = []
    for ver in (1, 2):
        iframe = _frame("1" + "0" + "0" + format(20, "06b") + _DC_MB * 4)
        skip = _part_code(ver, 0, 0) + _ue_code(0)
        far = _part_code(ver, 0, 1) + _se_code(8192) + _se_code(0) + _ue_code(0)
        deep = (_part_code(ver, 0, 8) + _part_code(ver, 1, 9) + _part_code(ver, 5, 1) + _se_code(8192) + _se_code(0) +
                _part_code(ver, 5, 1) + _se_code(8190) + _se_code(1) + _part_code(ver, 1, 1) + _se_code(8196) + _se_code(-3) + _ue_code(0))
        for first in (far, deep):
            pframe = _frame("0" + _se_code(0) + first + skip * 3)
            p = types.SimpleNamespace(width=32, height=32, version=ver, n_frames=2)
            out.append((p, np.concatenate([iframe, pframe]), np.array([0, iframe.size, iframe.size + pframe.size])))
    return out


def _alias_clips():
    """Hand-made P-frames whose vectors are far members of a near vector's class: (4 t S + a, -4 t + b), |a|, |b| <= a few half samples,
    t = 1, -1, 2, -3, 3, one t per frame.  The generator never writes such a vector; the reference copies from a few samples away, and the
    export must say the canonical member.  In the top macroblock row the predictor is 0 (two of the three neighbours are the zeroed row
    cache): the LAST leaf of each macroblock there -- the one the row cache keeps -- codes (4 t S, -4 t) outright, its other leaves are near
    vectors pointing down and to the right.  The rows below predict from the row cache, which keeps vectors as they were read, so their
    code-0 leaves (no delta) and their small deltas are far vectors too, with b <= 0: no window starts before the plane or ends behind it,
    and the reference throws nowhere.  One leaf, TOP/BOTTOM, LEFT/RIGHT (leaf records), four 8x8 and deeper trees down to 2x2 (cell maps),
    leaves with and without a delta, references 1..5, every phase; a third of the macroblocks carry residual (1, 3 or 20 levels), so far
    vectors and level sums meet in one macroblock.  A last frame puts dx = 2 S, 2 S - 1, -2 S and -2 S - 1 into cell-map words.  64x64
    (Stride 256) and 272x64 (Stride 512), both versions."""
    from tests.test_parse_fallback import _DC_MB, _frame, _part_code, _se_code, _ue_code
    from tests.tables import load
    part = functools.lru_cache(maxsize=None)(_part_code)
    T = load()
    # residual VLC codes of table 0 (P-frames; ReadDCTMatrix, MD.cs:3330: entry = [3:0] bits with the sign, [8:4] level, [14:9] run, [15] last)
    # without their sign bit: level 1 or 2, run 0, a one among the first three bits (no escape prefix) -> [not last, last]
    level_codes = [[], []]
    for idx in range(512, 4096):
        e = int(T["mobi_vx2table0_a"][idx])
        nb, level, run, last = e & 15, (e >> 4) & 31, (e >> 9) & 63, e >> 15
        if 4 <= nb <= 12 and level in (1, 2) and run == 0 and idx % (1 << (13 - nb)) == 0:
            level_codes[last].append(format(idx >> (13 - nb), "0%db" % (nb - 1)))
    assert level_codes[0] and level_codes[1]
    out = []
    for ver, W, H in ((1, 64, 64), (2, 64, 64), (1, 272, 64), (2, 272, 64)):
        S, mbw, mbh = (256 if W <= 256 else 512), W // 16, H // 16
        rng = np.random.default_rng(1000 * ver + W)
        frames = [_frame("1" + "0" + "0" + format(20, "06b") + _DC_MB * (mbw * mbh))]

        def tree(wi, hi, refs, top):
            """-> the codes of one (sub)tree, in stream order"""
            w, h = 16 >> wi, 16 >> hi
            split = [k for k, ok in ((8, h > 2), (9, w > 2)) if ok]
            if split and rng.random() < (0.75 if w * h > 16 else 0.35):
                k = split[int(rng.integers(len(split)))]
                nwi, nhi = (wi, hi + 1) if k == 8 else (wi + 1, hi)
                return [part(ver, wi * 4 + hi, k)] + tree(nwi, nhi, refs, top) + tree(nwi, nhi, refs, top)
            if not top and rng.random() < 0.3:
                return [part(ver, wi * 4 + hi, 0)]  # the predicted vector as it is: far, with no delta in the stream
            ref = 1 + int(rng.integers(refs))
            if top:  # down and to the right; the macroblock's LAST leaf, which the row cache keeps, becomes the far one (below)
                dx, dy = int(rng.integers(0, 7)), int(rng.integers(0, 7))
            else:
                dx, dy = int(rng.integers(-6, 7)), int(rng.integers(-6, 1))
            return [part(ver, wi * 4 + hi, ref), _se_code(dx), _se_code(dy)]

        def residual():
            """one coded 8x8 area (any of the six) as one 8x8 transform: 1, 3 or 20 levels of +-1 / +-2 at consecutive scan positions"""
            area = int(rng.integers(6))
            codes = [_ue_code(int(np.flatnonzero(T["mobi_cbp_inter"] == 1 << area)[0])), "1"]
            n = (1, 3, 20)[int(rng.integers(3))]
            for i in range(n):
                pool = level_codes[i == n - 1]
                codes.append(pool[int(rng.integers(len(pool)))] + "01"[int(rng.integers(2))])
            return codes

        def macroblock(far, refs, top):
            codes = tree(0, 0, refs, top)
            if top:
                codes[-2:] = [_se_code(far[0]), _se_code(far[1])]
            return codes + (residual() if rng.random() < 0.3 else [_ue_code(0)])

        def arrives(codes, k):
            """The reference's bit window holds 16 + (-k mod 16) bits after k bits of a frame (FillBits, MD.cs:2988: one refill per read): a
            longer code is not read as written.  True when every code of `codes`, starting k bits into the frame, fits its window."""
            for code in codes:
                if len(code) > 16 + (-k) % 16:
                    return False
                k += len(code)
            return True

        for f, t in enumerate((1, -1, 2, -3, 3), start=1):
            head, mbs, budget = "0" + _se_code(0), [], 20000
            while len(mbs) < mbw * mbh:
                k = len(head) + sum(len(m) for m in mbs) - 16
                for _ in range(50):  # (the top row's far codes have 23 to 27 bits: draw trees until one fits where it starts ...)
                    codes = macroblock((4 * t * S, -4 * t), min(f, 5), len(mbs) < mbw)
                    if arrives(codes, k):
                        mbs.append("".join(codes))
                        break
                else:  # (... and where none does, draw the macroblock before it again: another length, another start)
                    mbs.pop()
                budget -= 1
                assert budget > 0, (ver, W, f)
            bits = head + "".join(mbs)
            frames.append(_frame(bits))
        # one more frame: the rule's boundary in cell-map words.  dx = 2 S - 1 and -2 S stay, 2 S and -2 S - 1 move.  Macroblocks 0 and 1 of
        # the second row (predictor 0: the row above is all (0, 0)): TOP/BOTTOM, the top half two 8x8 leaves with the boundary vectors, the
        # bottom half (0, 0), which the row cache keeps.  dy, the references and the row above are drawn until the long codes fit their windows.
        skip, still = part(ver, 0, 0) + _ue_code(0), part(ver, 0, 1) + _se_code(0) + _se_code(0) + _ue_code(0)  # (0, 0) both, of two lengths
        for _ in range(20000):
            bits = "0" + _se_code(0) + "".join((skip, still)[int(rng.integers(2))] for _ in range(mbw))
            for pair in ((2 * S, 2 * S - 1), (-2 * S, -2 * S - 1)):
                leaf = lambda shape, dx, dy: [part(ver, shape, 1 + int(rng.integers(5))), _se_code(dx), _se_code(dy)]
                codes = ([part(ver, 0, 8), part(ver, 1, 9)] + leaf(5, pair[0], int(rng.integers(-24, 49))) + leaf(5, pair[1], int(rng.integers(-24, 49))) +
                         [part(ver, 1, 1), _se_code(0), _se_code(0), _ue_code(0)])
                if not arrives(codes, len(bits) - 16):
                    break
                bits += "".join(codes)
            else:
                break
        else:
            raise AssertionError((ver, W))
        frames.append(_frame(bits + skip * (mbw * (mbh - 1) - 2)))
        p = types.SimpleNamespace(width=W, height=H, version=ver, n_frames=len(frames))
        out.append((p, np.concatenate(frames), np.concatenate([[0], np.cumsum([x.size for x in frames])])))
    return out


@functools.lru_cache(maxsize=None)
def family(name):
    """-> [(params, data, frame_off)]"""
    if name == "suite":  # tests/test_coverage.py: every partition shape x table version x code, reference slots 1-5, all four phases
        return _generated(suite_params())
    if name == "deep":  # deep trees with many references, both versions, Width == Stride; vectors stay inside the picture
        return _generated([_deep_params("A", BASE_SEED + 7300 + i, 256, 32, cbp_prob=300) for i in range(3)] +
                          [_deep_params("B", BASE_SEED + 7310 + i, 512, 32, cbp_prob=300) for i in range(3)])
    if name == "w80":  # five macroblocks per row
        return _generated([default_params("A", BASE_SEED + 7320 + i, width=80, height=48, n_frames=8, pm_deep=300, pm_multiref=400, pm_intra=100,
                                          cbp_prob=500, t8_prob=500, max_coefs=10, scan_span=40, dense_prob=150) for i in range(4)])
    if name == "edge":  # vectors that leave the picture and wrap rows: test_deeper_trees_cell_by_cell's streams themselves
        return _generated([_deep_params("A" if ver == 1 else "B", BASE_SEED + 950 + w + cbp, w, h, mv_range=70, edge_mode=1, cbp_prob=cbp)
                           for w, h, ver in ((64, 48, 1), (256, 32, 1), (512, 32, 2)) for cbp in (0, 400)])
    if name == "far":
        return _far_clips()
    if name == "alias":
        return _alias_clips()
    if name == "resid":  # test_residual_rounds_16_bit_and_32_bit_by_quantizer's streams at two quantisers: long level runs, raw escapes, 8x8 and 4x4 mixed
        return _generated([default_params(cfg, BASE_SEED + 900 + q, n_frames=7, pm_multiref=300, width=w, height=h, quantizer=q, cbp_prob=800, t8_prob=700, dense_prob=150,
                                          escape_prob=60, max_coefs=10, scan_span=40, pm_intra=20, qdelta_prob=300)
                           for q in (22, 41) for cfg, w, h in (("A", 256, 48), ("B", 640, 32))])
    raise KeyError(name)


FAMILIES = ["suite", "deep", "w80", "edge", "far", "alias", "resid"]
# what each family is there for, asserted of the streams themselves (a seed that stopped giving it would leave the comparison standing but
# hollow): every reference slot 1..5 / a vector the canonical rule changes / a macroblock of more than sixteen levels (the kernel sums
# levels in sixteen strided lanes).  The generator writes no vector the rule changes, not even with edge_mode=1 and mv_range=70 (rows wrap
# with |dx| < 2 Stride): that is what the hand-made families are for.  "alias" joins such vectors with long level runs in one macroblock
# and puts vectors on the rule's boundary (both asserted below); "far" has one reference and no residual by construction.
NEEDS = {"suite": ("refs", "levels"), "deep": ("refs", "levels"), "w80": ("refs", "levels"), "edge": ("refs", "levels"), "far": ("moved",), "alias": ("refs", "moved", "shapes"),
         "resid": ("refs", "levels", "kinds")}


@functools.lru_cache(maxsize=None)
def family_trace(name):
    """-> per clip: [(canonical cells int64 [3, H/2, W/2], mbs int32 [5, H/16, W/16], raw cells)] per frame.  Every frame decodes with rc 0."""
    out = []
    for c, (p, data, fo) in enumerate(family(name)):
        frames, S = oracle_motion(p, data, fo)
        assert all(fr[0] == 0 for fr in frames), (name, c, [fr[0] for fr in frames])
        out.append([(canonical_cells(cells, S), mbs, cells) for _, cells, mbs in frames])
    return out


# ---------------------------------------------------------------------------------------------------------------- the comparison
@pytest.mark.parametrize("name", FAMILIES)
def test_the_oracles_motion_is_the_command_lists(name):
    """cells and all five macroblock values of every frame, exact.  The trace has no counterpart for the quantiser fields 62 (no table set
    up) and 63 (literal words): no macroblock of these streams carries one, none is left out of the comparison"""
    clips, traces = family(name), family_trace(name)
    seen = {"refs": set(), "moved": 0, "levels": 0, "mixed": 0, "far one leaf": 0, "far pair": 0, "far cell map": 0, "boundary": set(), "far with levels": 0, "far with > 16 levels": 0, "frames": 0, "intra": 0, "left_out": 0}
    for c, ((p, data, fo), trace) in enumerate(zip(clips, traces)):
        host = host_motion(p, data, fo)
        assert len(host) == len(trace) == len(fo) - 1
        for f, ((rc, hcells, hmbs, desc, pay), (cells, mbs, raw)) in enumerate(zip(host, trace)):
            assert rc == 0, (name, c, f, rc)
            seen["left_out"] += int(((hmbs[1] == 62) | (hmbs[1] == 63)).sum())
            assert np.array_equal(hcells, cells), (name, c, f, "cells [plane, y, x]", np.argwhere(hcells != cells)[:4].tolist(),
                                                   hcells[hcells != cells][:4].tolist(), cells[hcells != cells][:4].tolist())
            assert np.array_equal(hmbs, mbs), (name, c, f, "mbs [value, y, x]", np.argwhere(hmbs != mbs)[:4].tolist(),
                                               hmbs[hmbs != mbs][:4].tolist(), mbs[hmbs != mbs][:4].tolist())
            seen["refs"] |= set(np.unique(cells[2]).tolist())
            seen["moved"] += int((cells[0] != raw[0]).sum())
            seen["levels"] += int((mbs[3] > 16).sum())
            seen["intra"] += int(mbs[0].sum())
            t8 = (desc[:, 1] >> 14) & 63  # (which coded areas are one 8x8 transform: only to see that both kinds meet in long macroblocks)
            coded = (desc[:, 1] >> 8) & 63
            far_mb = (cells[0] != raw[0]).reshape(raw.shape[1] // 8, 8, raw.shape[2] // 8, 8).any((1, 3)).reshape(-1)  # macroblocks the rule changed
            leaves, dual = (desc[:, 1] >> 1) & 0x7F, (desc[:, 1] >> 26) & 3
            seen["far one leaf"] += int((far_mb & (leaves == 1)).sum()); seen["far pair"] += int((far_mb & (dual != 0)).sum())
            seen["far cell map"] += int((far_mb & (leaves > 1) & (dual == 0)).sum())
            S = 256 if p.width <= 256 else 512 if p.width <= 512 else 1024
            in_map = np.repeat(np.repeat(((leaves > 1) & (dual == 0)).reshape(raw.shape[1] // 8, -1), 8, 0), 8, 1)
            seen["boundary"] |= {k for k, v in (("2S", 2 * S), ("2S-1", 2 * S - 1), ("-2S", -2 * S), ("-2S-1", -2 * S - 1)) if (in_map & (raw[0] == v)).any()}
            seen["far with levels"] += int((far_mb & (mbs[3].reshape(-1) > 0)).sum()); seen["far with > 16 levels"] += int((far_mb & (mbs[3].reshape(-1) > 16)).sum())
            seen["mixed"] += int((((t8 & coded) != 0) & ((~t8 & coded) != 0) & (mbs[3].reshape(-1) > 16)).sum())
            seen["frames"] += 1
    print(name, {k: (sorted(v) if isinstance(v, set) else v) for k, v in seen.items()})
    assert seen["left_out"] == 0 and seen["frames"] == sum(len(fo) - 1 for _, _, fo in clips)
    need = NEEDS[name]
    if "refs" in need:
        assert seen["refs"] >= {0, 1, 2, 3, 4, 5}, (name, seen["refs"])
    if "moved" in need:
        assert seen["moved"] > 0, name
    if "levels" in need:
        assert seen["levels"] > 0, name
    if "shapes" in need:  # the rule applied to leaf records (one leaf, a TOP/BOTTOM or LEFT/RIGHT pair) and to cell-map words
        assert min(seen["far one leaf"], seen["far pair"], seen["far cell map"]) > 0, (name, seen)
        assert seen["boundary"] == {"2S", "2S-1", "-2S", "-2S-1"}, (name, seen["boundary"])  # both sides of both ends of [-2 S, 2 S), in cell-map words
        assert seen["far with > 16 levels"] > 0, (name, seen)  # a vector the rule changes and a long level sum in one macroblock
    if "kinds" in need:
        assert seen["mixed"] > 0, (name, seen)  # more than sixteen levels AND both transform sizes in one macroblock


@pytest.mark.parametrize("W,H", WIDTHS)
def test_the_trace_is_the_script(W, H):
    """streams written down (tests/test_motion_field.py, scripted_case): the trace's raw cells are the script's vectors, frame 0 is all
    intra, and no vector there needs the canonical rule"""
    p, clips, want = scripted_case(W, H)
    for c, (data, fo) in enumerate(clips):
        frames, S = oracle_motion(p, data, fo)
        for f in range(N_FRAMES):
            rc, cells, mbs = frames[f]
            assert rc == 0, (W, c, f, rc)
            assert np.array_equal(cells, want[c][f]), (W, c, f, np.argwhere(cells != want[c][f])[:4].tolist())
            assert np.array_equal(canonical_cells(cells, S), want[c][f])
            assert np.array_equal(mbs[0], np.full((H // 16, W // 16), f == 0)), (W, c, f)
            assert (mbs[1] == p.quantizer).all() and ((mbs[3] == 0) == (mbs[4] == 0)).all() and ((mbs[2] == 0) == (mbs[3] == 0)).all()


def test_a_frame_that_throws_leaves_the_trace_invalid():
    """a P-frame with no reference: the oracle throws (ORA_E_NULLREF), the trace says so; without arming there is no trace at all"""
    import ctypes as C
    p, data, fo = family("w80")[0]
    o = OracleDecoder(p.width, p.height, p.version)
    o.Data, o.Offset = data[: fo[2]], int(fo[1])  # the second frame first
    assert not data[fo[1] + 1] & 0x80
    planes, cells, mbs = o.DecodeFrameTraced()
    assert o.last_error != 0 and planes is None and cells is None and mbs is None
    assert o.L.mobi_oracle_motion_trace(None, None) == -1
    o.Data, o.Offset = data[: fo[1]], 0  # not armed: the invalid trace is dropped, none is made
    assert o.DecodeFrame() is not None and o.L.mobi_oracle_motion_trace(None, None) == 0
    buf = np.zeros(3 * (p.height // 2) * (p.width // 2), np.int16)
    assert o.L.mobi_oracle_motion_trace(buf.ctypes.data_as(C.c_void_p), None) == 0 and not buf.any()
    o.close()
