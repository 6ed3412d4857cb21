"""Encoder-side analysis: Analyzer.InterPredict2x2 over every 2x2 luma block (Analyzer.cs:608-693).

CPU: the oracle's restatement against an independent numpy brute-force of the same three-step search, and on inputs whose
answer is known.  GPU (-m gpu): mobi_batch_motion_search against the oracle, bit-exact packed words.

The second half of the file takes the search to its edges: pictures of one macroblock, Width == Stride, odd macroblock counts, several clips
with different rings, inputs on which every candidate ties, the extreme scores, every ring position.  One builder (edge_inputs) makes the
planes and pictures of a (size, case); the CPU tests pin the oracle on exactly these inputs (against _numpy_search and against the answers
the inputs were built to have), the GPU test then compares the kernel with the oracle word for word."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from mobiclipdecoder_amd import default_params, generate_clip, unpack_motion_search
from mobiclipdecoder_amd.streamgen import BASE_SEED
from tests.oracle_binding import OracleDecoder, lib as oracle_lib


def _decoded_oracle(cfg="A", n_frames=4, seed=900, **kw):
    p = default_params(cfg, BASE_SEED + seed, n_frames=n_frames, **kw)
    data, fo = generate_clip(p)
    ora = OracleDecoder(p.width, p.height, p.version)
    for f in range(n_frames):
        ora.Data, ora.Offset = data[fo[f]:fo[f + 1]], 0
        assert ora.DecodeFrame() is not None
    return p, data, fo, ora


def _numpy_search(past, pic):
    """Independent statement of Analyzer.cs:608-681 for one picture: plain loops over blocks, numpy only for the planes."""
    H, W = pic.shape
    out = np.zeros((H // 16, W // 16, 8, 8), np.uint32)
    for by in range(0, H, 2):
        for bx in range(0, W, 2):
            cmp = pic[by:by + 2, bx:bx + 2].astype(np.int32)
            res = (0, 0, 0, None)
            for i, ref in enumerate(past):
                if ref is None:
                    break
                cx = cy = 0
                cscore = 0
                for st in (6, 3, 1):
                    best = (None, 0, 0)
                    for y in (-st, 0, st):
                        if by + y + cy < 0 or by + 2 + y + cy > H:
                            continue
                        for x in (-st, 0, st):
                            if bx + x + cx < 0 or bx + 2 + x + cx > W:
                                continue
                            blk = ref[by + y + cy:by + y + cy + 2, bx + x + cx:bx + x + cx + 2].astype(np.int32)
                            s = int(np.abs(cmp - blk).sum())
                            nx, ny = x + cx, y + cy
                            if best[0] is None or s < best[0] or (s == best[0] and abs(nx) + abs(ny) < abs(best[1]) + abs(best[2])):
                                best = (s, nx, ny)
                    cscore, cx, cy = best
                if res[3] is None or cscore < res[3] or (cscore == res[3] and abs(2 * cx) + abs(2 * cy) < abs(res[0]) + abs(res[1])):
                    res = (2 * cx, 2 * cy, i, cscore)
            sc = 0xFFF if res[3] is None else res[3]
            out[by // 16, bx // 16, (by % 16) // 2, (bx % 16) // 2] = (res[0] & 0xFF) | ((res[1] & 0xFF) << 8) | (res[2] << 16) | (sc << 20)
    return out


def test_oracle_search_matches_an_independent_numpy_statement():
    p, _, _, ora = _decoded_oracle("A", n_frames=3)
    rng = np.random.default_rng(5)
    S = ora.Stride
    past = [ora.y(i) for i in range(5)]
    past = [None if a is None else a[:, :p.width] for a in past]
    # a picture that resembles the last frame (shifted, with noise) so that scores and ties are interesting
    pic = np.roll(past[0], (3, -6), axis=(0, 1)).astype(np.int32) + rng.integers(-3, 4, past[0].shape)
    pic = np.clip(pic, 0, 255).astype(np.uint8)
    pic[:64, :64] = past[1][:64, :64]  # one corner is an exact copy of the frame before
    got = ora.motion_search(pic)
    want = _numpy_search(past, pic)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    assert S >= p.width
    ora.close()


def test_known_answers():
    p, _, _, ora = _decoded_oracle("A", n_frames=2)
    y0 = ora.y(0)[:, :p.width]
    # the frame itself: zero vector, frame 0, score 0 everywhere (ties go to the shorter vector and the earlier frame)
    r = unpack_motion_search(ora.motion_search(y0))
    assert not r["dx"].any() and not r["dy"].any() and not r["frame"].any() and not r["score"].any()
    # no past frame at all: the reference's loop body never runs
    fresh = OracleDecoder(p.width, p.height, p.version)
    r = unpack_motion_search(fresh.motion_search(y0))
    assert (r["score"] == 0xFFF).all() and not r["dx"].any() and not r["frame"].any()
    fresh.close()
    # vectors are even (full pels stored as half pels) and within the reach of 6 + 3 + 1 pels
    pic = np.roll(y0, (-9, 7), axis=(0, 1))
    r = unpack_motion_search(ora.motion_search(pic))
    assert (r["dx"] % 2 == 0).all() and (np.abs(r["dx"]) <= 20).all() and (np.abs(r["dy"]) <= 20).all()
    ora.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_gpu_search_equals_oracle(cfg):
    from mobiclipdecoder_amd import MobiclipBatch
    n, nfr = 3, 7
    ps = [default_params(cfg, BASE_SEED + 910 + i, n_frames=nfr, pm_intra=80) for i in range(n)]
    clips = [generate_clip(p) for p in ps]
    W, H = ps[0].width, ps[0].height
    b = MobiclipBatch(n, W, H, ps[0].version)
    oras = [OracleDecoder(W, H, ps[0].version) for _ in range(n)]
    rng = np.random.default_rng(77)
    for f in range(nfr):
        if f in (0, 2, 6):  # empty ring, partly filled ring (two frames), full ring of five and more
            pics = []
            for i in range(n):
                prev = oras[i].y(0)
                base = rng.integers(0, 256, (H, W), dtype=np.uint8) if prev is None else np.roll(prev[:, :W], (int(rng.integers(-8, 9)), int(rng.integers(-8, 9))), axis=(0, 1))
                pic = np.clip(base.astype(np.int32) + rng.integers(-2, 3, (H, W)), 0, 255).astype(np.uint8)
                if i == 1 and f == 6:
                    pic[: H // 2] = oras[i].y(3)[: H // 2, :W]  # half of the picture comes straight from an older frame
                pics.append(pic)
            got = b.motion_search(pics)["packed"]
            for i in range(n):
                want = oras[i].motion_search(pics[i])
                assert np.array_equal(got[i], want), (f, i, np.argwhere(got[i] != want)[:5].tolist())
            if f == 6:
                assert len(np.unique(unpack_motion_search(got[1])["frame"])) > 1
        rcs, _ = b.decode([c[0][c[1][f]:c[1][f + 1]] for c in clips], [0] * n)
        assert rcs == [0] * n
        for i in range(n):
            oras[i].Data, oras[i].Offset = clips[i][0][clips[i][1][f]:clips[i][1][f + 1]], 0
            assert oras[i].DecodeFrame() is not None
    b.close()


# =====================================================================================================================================
# The search at its edges
# =====================================================================================================================================
# (width, height, clips): 16x16 = one macroblock, the whole reach outside the picture; 32x16 = one row of macroblocks (also as a batch of one
# clip); 48x32 and 80x48 = an odd number of macroblocks per row; 256x16 and 512x32 = Width == Stride, no padding column (strides 256 and 512)
RIGS = [(16, 16, 3), (32, 16, 3), (32, 16, 1), (48, 32, 3), (80, 48, 3), (256, 16, 3), (512, 32, 3)]
# case -> frames decoded before the search: n_past = min(5, frames) planes of the ring are searched, and the newest lies in slot frames % 6
CASES = {"random": 7, "shifts": 2, "flat_a": 2, "flat_b": 2, "stripes2": 3, "stripes3": 3, "stripes6": 3, "same_in_all_slots": 5, "only_in_slot_4": 5,
         "shorter_in_later_frame": 5, "past0": 0, "past1": 1, "past3": 3, "ring_f5": 5, "ring_f6": 6, "ring_f7": 7, "ring_f8": 8, "ring_f9": 9, "ring_f10": 10}
# ring_f5 .. ring_f10 are ONE set of planes and pictures at ring_base 5, 0, 1, 2, 3, 4 (the oracle has no ring position: to it they are one case)
CONTENT = {c: ("ring" if c.startswith("ring_f") else c) for c in CASES}
SHIFT_VALUES = (0, 1, -1, 3, -3, 6, -6, 9, -9, 10, -10)
SHIFTS = [(dx, dy) for dy in SHIFT_VALUES for dx in SHIFT_VALUES]  # full pels
MARGIN = 12  # of the oversized fields pictures are cut from: more than the reach of 6 + 3 + 1
FLAT = {"flat_a": [(7, 7), (200, 13), (0, 255)], "flat_b": [(255, 0), (0, 0), (255, 255)]}  # (picture, every past plane) per clip
LATER = [(1, (6, 0), 3, (0, 0)), (0, (-6, 6), 2, (0, 6)), (2, (6, 6), 4, (-6, 0))]  # per clip: (slot, shift) of the longer match, (slot, shift) of the shorter one


def _smooth_field(rng, h, w):
    """a random field without detail below 8 pels (plus a little noise): the three-step search finds its way on it"""
    gy, gx = h // 8 + 2, w // 8 + 2
    g = rng.integers(0, 256, (gy, gx)).astype(np.float64)
    rows = np.array([np.interp(np.arange(w) / 8.0, np.arange(gx), g[j]) for j in range(gy)])
    f = np.array([np.interp(np.arange(h) / 8.0, np.arange(gy), rows[:, i]) for i in range(w)]).T
    return np.clip(np.rint(f) + rng.integers(-2, 3, (h, w)), 0, 255).astype(np.uint8)


def _cut(field, H, W, dx=0, dy=0):
    """the H x W window of an oversized field, moved by (dx, dy): real content comes in over the border, nothing wraps around"""
    return np.ascontiguousarray(field[MARGIN + dy:MARGIN + dy + H, MARGIN + dx:MARGIN + dx + W])


def _stripes(H, W, p, kind, phase, lo=40, hi=200):
    """period p: 0 = horizontal stripes, 1 = vertical stripes, 2 = checkerboard (cells of (p + 1) // 2 and p // 2 pels)"""
    y, x = np.mgrid[0:H, 0:W]
    on_y, on_x = ((y + (phase if kind == 0 else 0)) % p) < (p + 1) // 2, ((x + phase) % p) < (p + 1) // 2  # (the checkerboard moves along x only)
    return np.where((on_y, on_x, on_y ^ on_x)[kind], hi, lo).astype(np.uint8)


def block_shift(k, clip):
    """the shift the 2x2 block with running number k of clip `clip` is cut with (case "shifts"): every clip starts elsewhere in the list"""
    return SHIFTS[(k + 41 * clip) % len(SHIFTS)]


@functools.lru_cache(maxsize=None)
def edge_inputs(W, H, n_clips, content):
    """-> (pasts, pics): pasts[clip][ring index] and pics[clip], (H, W) uint8 each.  Seeded by its arguments alone."""
    rng = np.random.default_rng([W, H, n_clips, zlib.crc32(content.encode())])
    rnd = lambda: rng.integers(0, 256, (H, W), dtype=np.uint8)  # noqa: E731
    big = lambda: rng.integers(0, 256, (H + 2 * MARGIN, W + 2 * MARGIN), dtype=np.uint8)  # noqa: E731
    n_past = min(5, CASES["ring_f5" if content == "ring" else content])
    pasts, pics = [], []
    for c in range(n_clips):
        if content == "random":  # pasts and picture independent: large scores, arbitrary vectors
            past, pic = [rnd() for _ in range(5)], rnd()
        elif content == "shifts":  # every 2x2 block is an exact copy of the newest plane, moved by its own shift
            field = big() if c == 0 else _smooth_field(rng, H + 2 * MARGIN, W + 2 * MARGIN)
            past, pic = [_cut(field, H, W), rnd()], np.empty((H, W), np.uint8)
            for k, (by, bx) in enumerate((by, bx) for by in range(0, H, 2) for bx in range(0, W, 2)):
                dx, dy = block_shift(k, c)
                pic[by:by + 2, bx:bx + 2] = field[MARGIN + by + dy:MARGIN + by + dy + 2, MARGIN + bx + dx:MARGIN + bx + dx + 2]
        elif content in FLAT:  # every candidate of every step and every frame ties
            a, b = FLAT[content][c]
            past, pic = [np.full((H, W), b, np.uint8)] * 2, np.full((H, W), a, np.uint8)
        elif content.startswith("stripes"):
            # slot 0: the pattern one pel out of phase (many candidates tie at the best score); slot 1: in phase but fainter (vector 0, a worse
            # score); slot 2: the picture itself in the right half (all nine candidates of the first step tie at 0), fainter in the left half
            p, kind = int(content[7:]), c % 3
            pic, faint = _stripes(H, W, p, kind, 0), _stripes(H, W, p, kind, 0, 45, 195)
            half = faint.copy()
            half[:, W // 2:] = pic[:, W // 2:]
            past = [_stripes(H, W, p, kind, 1), faint, half]
        elif content == "same_in_all_slots":
            field = big()
            noisy = np.clip(_cut(field, H, W, -3, 1).astype(np.int32) + rng.integers(-3, 4, (H, W)), 0, 255).astype(np.uint8)
            past, pic = [_cut(field, H, W)] * 5, noisy
        elif content == "only_in_slot_4":
            past = [rnd() for _ in range(5)]
            pic = past[4].copy()
        elif content == "shorter_in_later_frame":
            field = big()
            past, pic = [rnd() for _ in range(5)], _cut(field, H, W)
            sa, (ax, ay), sb, (bx_, by_) = LATER[c]
            past[sa], past[sb] = _cut(field, H, W, -ax, -ay), _cut(field, H, W, -bx_, -by_)  # past[y + ay][x + ax] == pic[y][x]
        else:  # past0, past1, past3, ring: block k is a copy of the plane in slot k % n_past, so every slot has to be the right one
            past, pic = [rnd() for _ in range(n_past)], rnd()
            for k, (by, bx) in enumerate((by, bx) for by in range(0, H, 2) for bx in range(0, W, 2)):
                if n_past:
                    pic[by:by + 2, bx:bx + 2] = past[(k + c) % n_past][by:by + 2, bx:bx + 2]
        assert len(past) == n_past
        pasts.append(past)
        pics.append(pic)
    return pasts, pics


@functools.lru_cache(maxsize=None)
def _ring_filler(W, H):
    """any stream of ten frames (I-frames only: what the ring holds when one is decoded does not matter)"""
    p = default_params("A", BASE_SEED + 930, n_frames=10, width=W, height=H, iframe_interval=1)
    data, fo = generate_clip(p)
    return p.version, [data[fo[f]:fo[f + 1]] for f in range(10)]


def _strided(plane, S):
    out = np.zeros((plane.shape[0], S), np.uint8)  # the padding stays zero
    out[:, :plane.shape[1]] = plane
    return out


@functools.lru_cache(maxsize=None)
def oracle_words(W, H, n_clips, case):
    """the oracle's packed answer per clip: a fresh decoder that has decoded CASES[case] frames, its ring overwritten with the case's planes"""
    pasts, pics = edge_inputs(W, H, n_clips, CONTENT[case])
    version, frames = _ring_filler(W, H)
    OL = oracle_lib()
    out = []
    for c in range(n_clips):
        ora = OracleDecoder(W, H, version)
        for f in range(CASES[case]):
            ora.Data, ora.Offset = frames[f], 0
            assert ora.DecodeFrame() is not None
        assert (ora.y(0) is None) == (CASES[case] == 0)
        for i, plane in enumerate(pasts[c]):
            y = _strided(plane, ora.Stride)
            C.memmove(OL.mobi_oracle_y(ora.h, i), y.ctypes.data, y.size)
        out.append(ora.motion_search(pics[c]))
        ora.close()
    return out


def _blocks(H, W):
    """picture coordinates (by, bx) of every 2x2 block, shaped like the results: (mbh, mbw, 8, 8)"""
    mby, mbx, Y, X = np.meshgrid(np.arange(H // 16), np.arange(W // 16), np.arange(8), np.arange(8), indexing="ij")
    return mby * 16 + 2 * Y, mbx * 16 + 2 * X


def _inside(H, W, dx, dy):
    """blocks whose copy moved by (dx, dy) lies inside the picture"""
    by, bx = _blocks(H, W)
    return (by + dy >= 0) & (by + dy + 2 <= H) & (bx + dx >= 0) & (bx + dx + 2 <= W)


NUMPY_RIGS = [r for r in RIGS if r[0] * r[1] <= 256 * 16]  # the pure-Python statement takes a minute on 512x32; 256x16 has the same property (Width == Stride)
CPU_CASES = [c for c in CASES if c == "ring_f5" or not c.startswith("ring_f")]


@pytest.mark.parametrize("case", CPU_CASES)
@pytest.mark.parametrize("W,H,n_clips", NUMPY_RIGS)
def test_oracle_equals_numpy_on_the_edge_inputs(W, H, n_clips, case):
    """The oracle against _numpy_search on every (size, case) the GPU test uses, so that the GPU test may rely on the oracle.  The numpy
    side runs on the sizes up to 80x48 and on 256x16; 512x32 (Width == Stride again, stride 512) is left to the answers pinned in
    test_edge_inputs_have_the_answers_they_were_built_for: the plain loops would take a minute there.  ring_f6 .. ring_f10 are ring_f5's
    inputs at other ring positions, which the oracle does not have."""
    pasts, pics = edge_inputs(W, H, n_clips, CONTENT[case])
    got = oracle_words(W, H, n_clips, case)
    for c in range(n_clips):
        want = _numpy_search(list(pasts[c]) + [None], pics[c])
        assert np.array_equal(got[c], want), (c, np.argwhere(got[c] != want)[:5].tolist())


@pytest.mark.parametrize("W,H,n_clips", RIGS)
def test_edge_inputs_have_the_answers_they_were_built_for(W, H, n_clips):
    by, bx = _blocks(H, W)
    res = {case: [unpack_motion_search(w) for w in oracle_words(W, H, n_clips, case)] for case in CASES}
    tie_decided = 0
    for case in CASES:
        for r in res[case]:
            assert (r["frame"] < max(1, min(5, CASES[case]))).all() and (np.abs(r["dx"]) <= 20).all() and (np.abs(r["dy"]) <= 20).all()
    for c in range(n_clips):
        # flat: every candidate of every step and both frames tie -> vector 0, frame 0; the score is the extreme one for 0 against 255
        for case in FLAT:
            r, (a, b) = res[case][c], FLAT[case][c]
            assert not r["dx"].any() and not r["dy"].any() and not r["frame"].any() and (r["score"] == 4 * abs(a - b)).all()
        # shifts: where the first step can land on the copy (components 0 or +-6, copy inside the picture) it is found, exactly
        r = res["shifts"][c]
        k = (by // 2) * (W // 2) + bx // 2
        sh = np.array([block_shift(int(i), c) for i in k.ravel()]).reshape(k.shape + (2,))
        sdx, sdy = sh[..., 0], sh[..., 1]
        inside = (by + sdy >= 0) & (by + sdy + 2 <= H) & (bx + sdx >= 0) & (bx + sdx + 2 <= W)
        step6 = inside & np.isin(sdx, (0, 6, -6)) & np.isin(sdy, (0, 6, -6))
        assert step6.any() and (r["score"][step6] == 0).all()
        if c == 0:  # (random bytes: nothing else scores 0)
            assert (r["dx"][step6] == 2 * sdx[step6]).all() and (r["dy"][step6] == 2 * sdy[step6]).all() and not r["frame"][step6].any()
        # stripes: in the right half slot 2 wins with vector 0 although all nine candidates of its first step score 0 -- the winner is the
        # fifth in scan order, neither the first nor the last; in the left half slot 0 wins with a vector that only the tie rule picks
        for p in (2, 3, 6):
            r = res[f"stripes{p}"][c]
            pasts, pics = edge_inputs(W, H, n_clips, f"stripes{p}")
            room = _inside(H, W, -6, -6) & _inside(H, W, 6, 6) & (bx >= W // 2 + 6)
            ties = 0
            for idx in np.argwhere(room):
                y0, x0 = int(by[tuple(idx)]), int(bx[tuple(idx)])
                blk = pics[c][y0:y0 + 2, x0:x0 + 2]
                if all(np.array_equal(blk, pasts[c][2][y0 + d:y0 + d + 2, x0 + e:x0 + e + 2]) for d in (-6, 0, 6) for e in (-6, 0, 6)):
                    first = 0 if np.array_equal(blk, pasts[c][0][y0:y0 + 2, x0:x0 + 2]) else 2  # (a block inside one stripe: slot 0 has it in place too)
                    ties += first == 2
                    assert (r["dx"][tuple(idx)], r["dy"][tuple(idx)], r["frame"][tuple(idx)], r["score"][tuple(idx)]) == (0, 0, first, 0)
                else:
                    assert False, "period p divides 6"
            assert ties > 0 or W < 32
            left = bx + 12 <= W // 2  # (no candidate reaches the right half)
            tie_decided += int((left & (r["frame"] == 0) & (r["score"] == 0) & ((r["dx"] != 0) | (r["dy"] != 0))).sum())
        # frame ties
        r = res["same_in_all_slots"][c]
        assert not r["frame"].any()
        r = res["only_in_slot_4"][c]
        assert (r["frame"] == 4).all() and not r["dx"].any() and not r["dy"].any() and not r["score"].any()
        r = res["shorter_in_later_frame"][c]
        sa, (ax, ay), sb, (bx_, by_) = LATER[c]
        both = _inside(H, W, ax, ay) & _inside(H, W, bx_, by_)
        assert both.any() and sb > sa and abs(bx_) + abs(by_) < abs(ax) + abs(ay)
        assert (r["frame"][both] == sb).all() and (r["dx"][both] == 2 * bx_).all() and (r["dy"][both] == 2 * by_).all() and not r["score"][both].any()
        # the ring cases: block k comes from slot (k + c) % n_past
        assert (res["past0"][c]["score"] == 0xFFF).all() and not (res["past0"][c]["packed"] & 0xFFFFF).any()
        for case, n_past in (("past1", 1), ("past3", 3), ("ring_f5", 5), ("ring_f10", 5)):
            r = res[case][c]
            assert np.array_equal(r["frame"], (k + c) % n_past) and not r["score"].any() and not r["dx"].any() and not r["dy"].any()
    assert tie_decided > 0 or W < 48
    # shifts again, over the clips of the rig: copies one, three, nine and ten pels away are found as well where the path leads to them
    if W * H >= 48 * 32:
        for m in (1, 3, 9, 10):
            found = 0
            for c in range(n_clips):
                r = res["shifts"][c]
                sh = np.array([block_shift(int(i), c) for i in k.ravel()]).reshape(k.shape + (2,))
                far = (np.abs(sh[..., 0]) == m) | (np.abs(sh[..., 1]) == m)
                found += int((far & (r["score"] == 0) & (r["dx"] == 2 * sh[..., 0]) & (r["dy"] == 2 * sh[..., 1]) & (r["frame"] == 0)).sum())
            assert found > 0, m


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,n_clips", RIGS)
def test_gpu_search_at_the_edges(W, H, n_clips, profiling_library):
    """every case of a size on one batch, in the order of the frames they need decoded: the ring position moves through 0, 1, 2, 3, 5, 0, 1, 2, 3, 4"""
    from mobiclipdecoder_amd import MobiclipBatch
    lib = profiling_library
    lib.mobi_debug_write_planes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    version, frames = _ring_filler(W, H)
    b = MobiclipBatch(n_clips, W, H, version)
    uv = np.zeros((H // 2, b.Stride), np.uint8)
    decoded, bases = 0, set()
    for case in sorted(CASES, key=lambda c: CASES[c]):
        while decoded < CASES[case]:
            rcs, _ = b.decode([frames[decoded]] * n_clips, [0] * n_clips)
            assert rcs == [0] * n_clips
            decoded += 1
        bases.add(decoded % 6)
        pasts, pics = edge_inputs(W, H, n_clips, CONTENT[case])
        for c in range(n_clips):
            for i, plane in enumerate(pasts[c]):
                y = _strided(plane, b.Stride)
                assert lib.mobi_debug_write_planes(b._h, c, i, y.ctypes.data, uv.ctypes.data) == 0
        got = b.motion_search(pics)["packed"]
        want = np.array(oracle_words(W, H, n_clips, case))
        if not np.array_equal(got, want):
            g, w = unpack_motion_search(got), unpack_motion_search(want)
            lines = [(tuple(int(v) for v in i), tuple(int(g[f][tuple(i)]) for f in ("dx", "dy", "frame", "score")),
                      tuple(int(w[f][tuple(i)]) for f in ("dx", "dy", "frame", "score"))) for i in np.argwhere(got != want)[:10]]
            pytest.fail(f"{case}: (clip, mby, mbx, Y, X), GPU (dx, dy, frame, score), oracle: {lines}")
    assert bases == {0, 1, 2, 3, 4, 5}
    b.close()
