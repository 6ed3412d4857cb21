"""What the tests of the inter encoder's intra mode share (tests/test_encode_pintra_model.py on the CPU, tests/test_encode_pintra_gpu.py on
the GPU):

  host model     tests/tools/mobi_encode_pintra_host.cpp: the product's csrc/mobi_encode_pintra.h run on the CPU (build.build_encpintrahost)
  sequences      enc_inter_model's sets and `still`, and two of this mode's own: `cut` (every frame smooth content unrelated to the frame
                 before) and `uncover` (a sharp texture in full- and half-pel motion in which rectangles of macroblocks of one P-frame are
                 replaced by new smooth content: one at column 0 and row 0, one at the right and bottom edges, one interior where there is room)
  geometry_set   the five clips of `cut` and `uncover` as one batch, for the shapes of enc_model.GEOMETRY_SHAPES
  chain          the host model over a set in mode 0 or 1
  parse_p_stream a P-frame read back with the ORACLE's tables: per macroblock partition code 0 / 1 / 6, vector difference or intra modes,
                 cbp, levels, bits
  rederive       an independent restatement in numpy: v* by brute force, the inter coding and its cost Jp, the six trials against the
                 DECODED picture's neighbours and Ji, the decision with its tie, effective vectors, predictors, bits, every statistic
  bisect         the rate rule written out again in Python over the model's fixed-quantiser encodes
Nothing here includes the product's encoder headers."""
import ctypes as C

import numpy as np

from tests import enc_inter_model as M
from tests import enc_model as E
from tests import tables

P = C.c_void_p
STATS_DTYPE = M.STATS_DTYPE
STAT_INTRA = 2  # reserved[]: macroblocks sent intra (include/mobiclip_encode_pintra.h)
VERSIONS = M.VERSIONS
SHAPES = M.SHAPES
RANGE, T = M.RANGE, M.T
OLD_SETS = ("fullpel", "mixed5", "still")
NEW_SETS = ("cut", "uncover")
SETS = OLD_SETS + NEW_SETS
CODE_INTRA, CODE_INTRA_BITS = 6, 5  # the partition code of an intra macroblock at 16x16 and its length in both versions' tables
_HOST = None
_SETS = {}


def host():
    global _HOST
    if _HOST is None:
        from mobiclipdecoder_amd import build
        L = C.CDLL(build.build_encpintrahost())
        L.encpi_host_bound.restype = C.c_size_t
        L.encpi_host_bound.argtypes = [C.c_uint32, C.c_uint32]
        L.encpi_host_mb_bytes.restype = C.c_size_t
        L.encpi_host_code_word.restype = C.c_uint32
        L.encpi_host_code_word.argtypes = [C.c_int]
        L.encpi_host_code_bits.argtypes = [C.c_int]
        L.encpi_host_inter.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, P, C.c_size_t, P, C.c_size_t, P, P, P, C.c_size_t, P, P, P, P, P, P, P, P, P, C.c_int]
        assert L.encpi_host_mb_bytes() == E.MB_DTYPE.itemsize
        _HOST = L
    return _HOST


def host_encode(W, H, version, mode, pictures, refs, prev_q, q, slot_bytes=None, threads=1, pitch=None, ref_pitch=None):
    """the host model over a batch -> enc_inter_model.host_encode's dict with kind (N, macroblocks; bit 0: sent intra) and jp (N, macroblocks,
    the inter coding's cost) in front of forms; mode 1 fills both, and mv then holds the EFFECTIVE vectors (zero in intra macroblocks)"""
    L = host()
    pictures, refs = np.ascontiguousarray(pictures, np.uint8), np.ascontiguousarray(refs, np.uint8)
    pq, q = np.ascontiguousarray(prev_q, np.uint8), np.ascontiguousarray(q, np.uint8)
    out, args = E.host_outputs(W, H, pictures.shape[0], L.encpi_host_bound(W, H) if slot_bytes is None else slot_bytes, STATS_DTYPE, mv=np.uint32, mvp=np.uint32,
                               kind=np.uint32, jp=np.int64)
    rc = L.encpi_host_inter(W, H, version, mode, pictures.shape[0], pictures.ctypes.data, pictures.shape[1] if pitch is None else pitch, refs.ctypes.data,
                            refs.shape[1] if ref_pitch is None else ref_pitch, pq.ctypes.data, q.ctypes.data, *args, threads)
    assert rc == 0, rc
    return out


def is_intra(out):
    return (out["kind"] & 1).astype(bool)


# ---------------------------------------------------------------------------------------------------------------- sequences
def _cut(W, H, seeds, shifts):
    """T frames, frame t from enc_inter_model._smooth with seed seeds[t] sampled shifts[t] half-pels off: smooth content, every frame
    unrelated to the one before, so that no vector predicts it and intra codes it cheaply"""
    return np.stack([M._smooth(W, H, [shifts[t]], seeds[t])[0] for t in range(T)])


def rectangles(mbw, mbh):
    """the macroblock rectangles (x0, y0, x1, y1; ends exclusive) of `uncover` with the kind of content each gets: the corner at column 0
    and row 0, the far one at the right and bottom edges, the interior one where there is room.  (At three columns the corner is one
    macroblock: the last step of the third clip moves the texture 3 samples to the left, so the right column has nothing to be predicted
    from and goes intra too, and the three macroblocks left over have an intra neighbour to the left, above and above right.)"""
    if mbw == 1 or mbh == 1:
        return [(0, 0, mbw, mbh, "xy")]
    r = [(0, 0, max(2, mbw // 5) if mbw >= 4 else 1, max(1, mbh // 5), "y"), (mbw - max(1, mbw // 6), mbh - max(1, mbh // 6), mbw, mbh, "xy")]
    if mbw >= 7 and mbh >= 7:
        r.append((mbw // 2 - 1, mbh // 2 - 1, mbw // 2 + 2, mbh // 2 + 2, "x"))
    return r


def _fresh(W, H, kind, seed):
    """new smooth content for a rectangle: "x" varies along x only (its macroblocks below the first row predict vertically), "y" along y
    only (horizontally), "xy" is _smooth's"""
    if kind == "xy":
        return M._smooth(W, H, [(0, 0)], seed)[0]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx = np.mgrid[0:H // 2, 0:W // 2].astype(np.float64) * 2
    f = (lambda x, y, a: 128 + 90 * np.sin(0.17 * x + a)) if kind == "x" else (lambda x, y, a: 128 + 90 * np.sin(0.13 * y + a))
    return E._i420(np.clip(np.rint(f(xx, yy, 0.4 * seed)), 0, 255), np.clip(np.rint(f(cx, cy, 1.0 + seed)), 0, 255), np.clip(np.rint(f(cx, cy, 2.0 + seed)), 0, 255))


def _uncover(rng, W, H, steps, at, seed):
    """T frames: frame 0 a sharp texture on a canvas larger than the picture; frame t is frame t - 1 moved by steps[t - 1] = (dx, dy)
    half-pels -- luma by the interpolation formula at (dx, dy), chroma at (dx >> 1, dy >> 1), so the vector that predicts the source
    exactly from the source before is known --, and in frame `at` the rectangles hold new smooth content in place of the texture"""
    pad = 24
    pl = [M._lattice(rng, H + 2 * pad, W + 2 * pad, 16, 240, 2), M._lattice(rng, H // 2 + pad, W // 2 + pad, 40, 216, 2), M._lattice(rng, H // 2 + pad, W // 2 + pad, 40, 216, 2)]
    crop = lambda p, i: p[pad >> (i > 0): (pad >> (i > 0)) + (H >> (i > 0)), pad >> (i > 0): (pad >> (i > 0)) + (W >> (i > 0))]
    out = []
    for t in range(T):
        if t:
            dx, dy = steps[t - 1]
            new = []
            for i, p in enumerate(pl):
                vx, vy = (dx, dy) if i == 0 else (dx >> 1, dy >> 1)
                e = np.pad(p, 12, mode="edge")
                new.append(M.interp(e, 12, 12, p.shape[1], p.shape[0], vx, vy))
            pl = new
        y, u, v = [crop(p, i).copy() for i, p in enumerate(pl)]
        if t == at:
            for k, (x0, y0, x1, y1, kind) in enumerate(rectangles(W // 16, H // 16)):
                fy, fu, fv = E.planes(_fresh(W, H, kind, seed + k), W, H)
                y[y0 * 16: y1 * 16, x0 * 16: x1 * 16] = fy[y0 * 16: y1 * 16, x0 * 16: x1 * 16]
                u[y0 * 8: y1 * 8, x0 * 8: x1 * 8] = fu[y0 * 8: y1 * 8, x0 * 8: x1 * 8]
                v[y0 * 8: y1 * 8, x0 * 8: x1 * 8] = fv[y0 * 8: y1 * 8, x0 * 8: x1 * 8]
        out.append(E._i420(y, u, v))
    return np.stack(out)


UNCOVER_AT = (1, 2, 3)  # the P-frame of each clip of `uncover` that holds the rectangles
# per clip the steps in half-pels: full-pel ones (even; 4 and 12 keep chroma whole, 2 and 6 give it a phase) and half-pel ones
_UNCOVER_STEPS = ([(4, -4), (3, 1), (-5, 2)], [(-2, 6), (8, -4), (1, -3)], [(5, 5), (-4, 2), (6, 0)])


def sequence_sets(W, H):
    """enc_inter_model's 'fullpel' and 'mixed5', its still scene, and: 'cut' -- two clips of four unrelated smooth frames, one quantiser each
    --, 'uncover' -- three clips, clip c with the rectangles in P-frame UNCOVER_AT[c], a quantiser per picture in the last"""
    if (W, H) not in _SETS:
        rng = np.random.default_rng(9090 + W * 3 + H)
        sets = {k: v for k, v in M.sequence_sets(W, H).items() if k in OLD_SETS}
        sets["still"] = M.still(W, H)
        sets["cut"] = (np.stack([_cut(W, H, (1, 3, 0, 2), [(0, 0), (37, 21), (-26, 45), (61, -18)]), _cut(W, H, (4, 2, 3, 0), [(0, 0), (-44, 9), (15, 58), (-33, -27)])]),
                       np.array([[26, 26, 26, 26], [18, 18, 22, 22]], np.uint8))
        sets["uncover"] = (np.stack([_uncover(rng, W, H, _UNCOVER_STEPS[c], UNCOVER_AT[c], 3 * c) for c in range(3)]),
                           np.array([[20, 20, 20, 20], [26, 26, 26, 26], [16, 22, 22, 30]], np.uint8))
        _SETS[(W, H)] = sets
    return _SETS[(W, H)]


def geometry_set(W, H):
    """what the geometry tests run (enc_model.GEOMETRY_SHAPES): the two clips of `cut` and the three of `uncover` as one batch of five ->
    (frames (5, T, frame), quantizers (5, T))"""
    sets = sequence_sets(W, H)
    return np.concatenate([sets[k][0] for k in NEW_SETS]), np.concatenate([sets[k][1] for k in NEW_SETS])


def chain(W, H, version, mode, frames, qs, **kw):
    """the host models over a set: list of T dicts (entry 0 is the intra model's), each P-frame predicted from the reconstruction before"""
    out = [E.host_encode(W, H, version, frames[:, 0], qs[:, 0])]
    for t in range(1, frames.shape[1]):
        out.append(host_encode(W, H, version, mode, frames[:, t], out[-1]["recon"], qs[:, t - 1], qs[:, t], **kw))
    return out


# ---------------------------------------------------------------------------------------------------------------- the stream, read back
def _ue(r):
    z = 0
    while r.take(1) == 0:
        z += 1
    return (1 << z) - 1 + r.take(z)


def _block(r, Tb, m, k, forms):
    """one coded block's symbols into m["lev"][k] (enc_model.parse_stream's reading of them)"""
    A, B = Tb["mobi_vx2table0_a"], Tb["mobi_vx2table0_b"]
    assert r.take(1) == 1, "4x4 transforms"
    p = 0
    while True:
        form = 0
        if r.peek(7) == 3:
            r.take(7)
            form = 2 if r.take(1) == 0 else 1 if r.take(1) == 0 else 3
        if form == 3:
            last, run, val = r.take(1), r.take(6), r.take(12)
            val -= 4096 if val >= 2048 else 0
        else:
            e = int(A[r.peek(12)])
            nb, val, run, last = e & 15, (e >> 4) & 31, (e >> 9) & 63, e >> 15
            assert nb >= 2 and val >= 1, "no code word here"
            if form == 2:
                val += int(B[e >> 9])
            if form == 1:
                run += int(B[0x80 + val + (last << 6)])
            r.take(nb - 1)
            if r.take(1):
                val = -val
        forms[form] += 1
        p += run
        assert p < 64, "run past the block"
        m["lev"][k][p] = val
        p += 1
        if last:
            break
    assert m["lev"][k].any()


def parse_p_stream(data, W, H, version):
    """-> dict(dq, hdr_bits, end, forms, mv_bits (what stands in front of every macroblock's cbp: partition codes, differences), mbs
    (MB_DTYPE; bits = what the macroblock took; the modes of an intra macroblock), code (0 / 1 / 6), ddx, ddy per macroblock)"""
    Tb = tables.load()
    ver = 0 if version == 2 else 1
    lut, nbits, shift = Tb["mobi_part_lut"][ver][0], Tb["mobi_part_bits"][ver][0], int(Tb["mobi_part_shift"][ver][0])
    r = E._Bits(data)
    assert r.take(1) == 0, "not a P-frame"
    out = {"dq": M._se(r), "forms": np.zeros(4, np.int64)}
    out["hdr_bits"] = r.pos
    n = (W // 16) * (H // 16)
    mbs = np.zeros(n, E.MB_DTYPE)
    code, ddx, ddy, mvb = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), 0
    for i, m in enumerate(mbs):
        start = r.pos
        c = int(lut[r.peek(32 - shift)])
        assert c in (0, 1, CODE_INTRA), "a partition code outside the encoder's subset"
        r.take(int(nbits[c]))
        code[i] = c
        if c == 1:
            ddx[i], ddy[i] = M._se(r), M._se(r)
        mvb += r.pos - start
        if c == CODE_INTRA:  # intra_full: ue(cbp) through mobi_cbp_intra, the modes in front of their blocks
            m["cbp"] = Tb["mobi_cbp_intra"][_ue(r)]
            for k in range(6):
                if k in (0, 4):
                    m["luma_mode" if k == 0 else "chroma_mode"] = r.take(3)
                if (int(m["cbp"]) >> k) & 1:
                    _block(r, Tb, m, k, out["forms"])
        else:
            m["cbp"] = Tb["mobi_cbp_inter"][_ue(r)]
            for k in range(6):
                if (int(m["cbp"]) >> k) & 1:
                    _block(r, Tb, m, k, out["forms"])
        m["bits"] = r.pos - start
    out.update(mbs=mbs, code=code, ddx=ddx, ddy=ddy, mv_bits=mvb, end=r.pos)
    return out


# ---------------------------------------------------------------------------------------------------------------- the decisions, re-derived
def _inter_coding(ref, W, H, q, source, reference, dx, dy):
    """every macroblock coded inter with its vector -> dict(sad, bits (the blocks' alone), cbp, clamp, range (M,), lev (M, 6, 64), rec (M, 6, 8, 8))"""
    mbw, mbh = W // 16, H // 16
    n = mbw * mbh
    sp, rp = E.planes(source.astype(np.int64), W, H), E.planes(reference.astype(np.int64), W, H)
    src_b, pred_b = np.zeros((n, 6, 8, 8), np.int64), np.zeros((n, 6, 8, 8), np.int64)
    for i in range(n):
        x, y, vx, vy = i % mbw, i // mbw, int(dx[i]), int(dy[i])
        for k in range(6):
            pl, bx, by, ux, uy = (0, x * 16 + (k & 1) * 8, y * 16 + (k >> 1) * 8, vx, vy) if k < 4 else (k - 3, x * 8, y * 8, vx >> 1, vy >> 1)
            src_b[i, k] = sp[pl][by: by + 8, bx: bx + 8]
            pred_b[i, k] = M.interp(rp[pl], bx, by, 8, 8, ux, uy)
    b = E._code_blocks(ref, q, src_b.reshape(n * 6, 8, 8), pred_b.reshape(n * 6, 8, 8))
    g = lambda k: b[k].reshape(n, 6)
    return {"sad": g("sad").sum(1), "bits": g("bits").sum(1), "cbp": (g("coded") * (1 << np.arange(6))).sum(1), "clamp": g("clamp").sum(1), "range": g("range").sum(1),
            "lev": b["lev"].reshape(n, 6, 64).astype(np.int16), "rec": b["rec"].reshape(n, 6, 8, 8)}


def _intra_trials(ref, W, H, q, source, decoded):
    """the six trials of every macroblock against the DECODED picture's left and upper neighbours (the macroblocks are independent then and
    run as one numpy batch), the argmin of each half with ties to the smaller mode -> dict(J (winners' costs, luma + chroma), sad, bits
    (the blocks' alone), cbp, clamp, range, luma_mode, chroma_mode (M,), lev (M, 6, 64), rec (M, 6, 8, 8))"""
    mbw, mbh = W // 16, H // 16
    n = mbw * mbh
    mbx, mby = np.tile(np.arange(mbw), mbh), np.repeat(np.arange(mbh), mbw)
    lam = E._lam(q)
    sp, dp = E.planes(source.astype(np.int64), W, H), E.planes(decoded.astype(np.int64), W, H)
    res = {k: np.zeros(n, np.int64) for k in ("J", "sad", "bits", "cbp", "clamp", "range")}
    res["lev"], res["rec"] = np.zeros((n, 6, 64), np.int16), np.zeros((n, 6, 8, 8), np.int64)
    for chroma in (0, 1):
        sz = 8 if chroma else 16
        tiles = lambda a: a.reshape(mbh, sz, mbw, sz).transpose(0, 2, 1, 3).reshape(n, sz, sz)

        def border(a):  # the row above and the column to the left of every tile (zeros where there is none)
            pad = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
            pad[1:, 1:] = a
            return (np.stack([pad[y * sz, 1 + x * sz: 1 + x * sz + sz] for y, x in zip(mby, mbx)]),
                    np.stack([pad[1 + y * sz: 1 + y * sz + sz, x * sz] for y, x in zip(mby, mbx)]))
        best, best_J, keep = np.full(n, -1), np.zeros(n, np.int64), {}
        for mode in (0, 1, 3):
            allowed = (mby > 0) if mode == 0 else (mbx > 0) if mode == 1 else np.ones(n, bool)
            J, blocks = np.zeros(n, np.int64), []
            for p_i in ((1, 2) if chroma else (0,)):
                src_t, (top, left) = tiles(sp[p_i]), border(dp[p_i])
                trial = np.zeros((n, sz, sz), np.int64)
                for k in range(1 if chroma else 4):
                    by, bx = k >> 1, k & 1
                    t = top[:, 8 * bx: 8 * bx + 8] if by == 0 else trial[:, 7, 8 * bx: 8 * bx + 8]
                    l = left[:, 8 * by: 8 * by + 8] if bx == 0 else trial[:, 8 * by: 8 * by + 8, 7]
                    b = E._code_blocks(ref, q, src_t[:, 8 * by: 8 * by + 8, 8 * bx: 8 * bx + 8], E._pred(mode, t, l, (mby > 0) | (by == 1), (mbx > 0) | (bx == 1)))
                    trial[:, 8 * by: 8 * by + 8, 8 * bx: 8 * bx + 8] = b["rec"]
                    J += (b["sad"] << 8) + lam * b["bits"]
                    blocks.append(b)
            take = allowed & ((best < 0) | (J < best_J))  # modes run upwards: a tie keeps the smaller one
            best, best_J = np.where(take, mode, best), np.where(take, J, best_J)
            keep[mode] = blocks
        res["chroma_mode" if chroma else "luma_mode"] = best
        res["J"] += best_J
        for a in range(2 if chroma else 4):
            area = 4 + a if chroma else a
            for mode in (0, 1, 3):
                sel, b = best == mode, keep[mode][a]
                res["cbp"] |= np.where(sel & b["coded"], 1 << area, 0)
                for k in ("sad", "bits", "clamp", "range"):
                    res[k] += np.where(sel, b[k], 0)
                res["lev"][sel, area] = b["lev"][sel]
                res["rec"][sel, area] = b["rec"][sel]
    return res


def _assemble(W, H, rec):
    """(M, 6, 8, 8) blocks -> packed I420"""
    mbw, mbh = W // 16, H // 16
    out = [np.zeros((H, W), np.int64), np.zeros((H // 2, W // 2), np.int64), np.zeros((H // 2, W // 2), np.int64)]
    for i in range(mbw * mbh):
        x, y = i % mbw, i // mbw
        for k in range(4):
            out[0][y * 16 + (k >> 1) * 8: y * 16 + (k >> 1) * 8 + 8, x * 16 + (k & 1) * 8: x * 16 + (k & 1) * 8 + 8] = rec[i, k]
        for k in (4, 5):
            out[k - 3][y * 8: y * 8 + 8, x * 8: x * 8 + 8] = rec[i, k]
    return E._i420(*out)


def rederive(ref, W, H, version, prev_q, q, source, reference, decoded):
    """One P-frame of the intra mode from its source, the DECODED frame before it and the DECODED frame itself (whose macroblocks give the
    trials their borders; the test holds the re-derived reconstruction against it, so nothing is taken on trust) -> dict(raw_dx, raw_dy
    (v* by brute force), Jp, Ji, intra, dx, dy (effective), pdx, pdy, code (0 / 1 / 6), cbp, lev, luma_mode, chroma_mode, bits (per
    macroblock, syntax included), recon, stats (field -> value))"""
    mbw, mbh = W // 16, H // 16
    n = mbw * mbh
    q, prev_q = int(q), int(prev_q)
    Tb = tables.load()
    ver = 0 if version == 2 else 1
    pbits = Tb["mobi_part_bits"][ver][0]
    inv_p = {int(c): i for i, c in reversed(list(enumerate(Tb["mobi_cbp_inter"])))}
    inv_i = {int(c): i for i, c in reversed(list(enumerate(Tb["mobi_cbp_intra"])))}
    lam = E._lam(q)
    sy, ry = E.planes(source.astype(np.int64), W, H)[0], E.planes(reference.astype(np.int64), W, H)[0]
    rdx, rdy = M.search_picture(W, H, q, sy, ry)[:2]
    P_ = _inter_coding(ref, W, H, q, source, reference, rdx, rdy)
    I_ = _intra_trials(ref, W, H, q, source, decoded)
    # the vector priced against the ZERO predictor, as the search prices it
    mv0 = np.array([int(pbits[0]) if not (rdx[i] or rdy[i]) else int(pbits[1]) + M.se_bits(int(rdx[i])) + M.se_bits(int(rdy[i])) for i in range(n)], np.int64)
    Jp = (P_["sad"] << 8) + lam * (P_["bits"] + mv0 + np.array([E._ue_bits(inv_p[int(c)]) for c in P_["cbp"]], np.int64))
    hdr_i = np.array([int(pbits[CODE_INTRA]) + E._ue_bits(inv_i[int(c)]) + 6 for c in I_["cbp"]], np.int64)
    Ji = I_["J"] + lam * hdr_i
    intra = Ji < Jp  # a tie stays inter
    dx, dy = np.where(intra, 0, rdx), np.where(intra, 0, rdy)
    at = lambda a, x, y: int(a[y * mbw + x]) if 0 <= x < mbw and 0 <= y < mbh else 0
    pdx, pdy = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        x, y = i % mbw, i // mbw
        if not intra[i]:
            pdx[i] = M.med3(at(dx, x - 1, y), at(dx, x, y - 1), at(dx, x + 1, y - 1) if y > 0 else 0)
            pdy[i] = M.med3(at(dy, x - 1, y), at(dy, x, y - 1), at(dy, x + 1, y - 1) if y > 0 else 0)
    code = np.where(intra, CODE_INTRA, ((dx != pdx) | (dy != pdy)).astype(np.int64))
    mvb = np.array([int(pbits[c]) + (M.se_bits(int(dx[i] - pdx[i])) + M.se_bits(int(dy[i] - pdy[i])) if c == 1 else 0) for i, c in enumerate(code)], np.int64)
    pick = lambda k: np.where(intra, I_[k], P_[k])
    cbp = pick("cbp")
    bits = np.where(intra, hdr_i + I_["bits"], mvb + np.array([E._ue_bits(inv_p[int(c)]) for c in P_["cbp"]], np.int64) + P_["bits"])
    hdr = 1 + M.se_bits(int(q) - int(prev_q))
    inter = ~intra
    stats = {"bits": hdr + int(bits.sum()), "sad": int(pick("sad").sum()), "mv_bits": int(mvb.sum()), "coded_blocks": int(sum(bin(int(c)).count("1") for c in cbp)),
             "fallback_clamp": int(pick("clamp").sum()), "fallback_level": int(pick("range").sum()), "code0": int((code == 0).sum()),
             "nonzero_mv": int((inter & ((dx != 0) | (dy != 0))).sum()), "halfpel_mv": int((inter & (((dx | dy) & 1) != 0)).sum()),
             "reserved": [0, 0, int(intra.sum()), 0]}
    return {"raw_dx": rdx, "raw_dy": rdy, "Jp": Jp, "Ji": Ji, "intra": intra, "dx": dx, "dy": dy, "pdx": pdx, "pdy": pdy, "code": code, "cbp": cbp,
            "lev": np.where(intra[:, None, None], I_["lev"], P_["lev"]), "luma_mode": np.where(intra, I_["luma_mode"], 0), "chroma_mode": np.where(intra, I_["chroma_mode"], 0),
            "bits": bits, "recon": _assemble(W, H, np.where(intra[:, None, None, None], I_["rec"], P_["rec"])), "stats": stats}


# ---------------------------------------------------------------------------------------------------------------- the rate rule
def rounds(qmin, qmax):
    """the smallest k with 2^k >= qmax - qmin + 1"""
    return int(qmax - qmin).bit_length()


def fixed(W, H, version, pictures, refs, prev_q, q, threads=1):
    """the intra mode's host model at given quantisers (prev_q as the encoder uses it: clamped to [12, 52])"""
    n = pictures.shape[0]
    pq = np.clip(np.broadcast_to(np.asarray(prev_q, np.int64), (n,)), 12, 52).astype(np.uint8)
    return host_encode(W, H, version, 1, pictures, refs, pq, np.broadcast_to(np.asarray(q, np.uint8), (n,)), threads=threads)


def bisect(W, H, version, pictures, refs, prev_q, targets, qmin=12, qmax=52, threads=1):
    """the rate rule in Python over `fixed`, as enc_rate_model.bisect states it: per round the middle of [lo, hi] is tried; a stream that
    fits its target moves hi down to it, one that does not moves lo above it -> (fixed's dict at q_out, q_out (N,))"""
    n = pictures.shape[0]
    tg = np.broadcast_to(np.asarray(targets, np.int64), (n,))
    lo, hi = np.full(n, qmin, np.int64), np.full(n, qmax, np.int64)
    for _ in range(rounds(qmin, qmax)):
        mid = (lo + hi) >> 1
        fits = fixed(W, H, version, pictures, refs, prev_q, mid, threads)["bytes"].astype(np.int64) <= tg
        lo, hi = np.where(fits, lo, np.minimum(mid + 1, hi)), np.where(fits, mid, hi)
    assert np.array_equal(lo, hi)
    return fixed(W, H, version, pictures, refs, prev_q, lo, threads), lo.astype(np.uint8)
