"""What the tests of the inter encoder's partition mode share (tests/test_encode_parts_model.py on the CPU, tests/test_encode_parts_gpu.py on
the GPU):

  host model     tests/tools/mobi_encode_parts_host.cpp: the product's csrc/mobi_encode_parts.h run on the CPU (build.build_encpartshost)
  sequences      enc_inter_model's sets and two of this mode's own: a sharp texture whose regions -- left / right halves, top / bottom
                 halves, quadrants, a seam in one half only -- move by different known full- and half-pel vectors, the seams through the
                 middles of macroblocks (x or y = 8 mod 16)
  chain          the host model over a set in mode 0 or 1
  parse_p_stream a P-frame read back with the ORACLE's tables: per macroblock the tree, its leaves in stream order with code 0 / 1 and the
                 vector difference, cbp, levels, bits
  rederive_*     an independent restatement in numpy: the leaf candidate sets, every leaf's v* by brute force, the tree from the stated
                 costs and tie rules, the prediction per quadrant
Nothing here includes the product's encoder headers."""
import ctypes as C

import numpy as np

from tests import enc_inter_model as M
from tests import enc_model as E
from tests import tables

P = C.c_void_p
STATS_DTYPE = M.STATS_DTYPE
STAT_SPLIT, STAT_LEAVES = 0, 1  # reserved[]: macroblocks sent split, leaves sent (include/mobiclip_encode_parts.h)
VERSIONS = M.VERSIONS
SHAPES = ((16, 16), (48, 32), (64, 48))
RANGE, T = M.RANGE, M.T
OLD_SETS = M.SETS
NEW_SETS = ("two_motion", "half_seams")
SETS = OLD_SETS + NEW_SETS
# the tree byte: root 0 (a 16x16 leaf), 1 (code 8: halves stacked), 2 (code 9: side by side); + 4 / + 8: the first / second half is split
ROOT_8, ROOT_9, SPLIT_FIRST, SPLIT_SECOND = 1, 2, 4, 8
PARTITIONS = (0, 1, 1 | 4, 1 | 8, 1 | 4 | 8, 2, 2 | 4, 2 | 8)  # the eight: all-8x8 is spelled through code 8
# the nine leaves as (x, y, w, h) inside the macroblock: the 16x16, top, bottom, left, right, Q0..Q3; and the shape index s = 4 wi + hi
LEAVES = ((0, 0, 16, 16), (0, 0, 16, 8), (0, 8, 16, 8), (0, 0, 8, 16), (8, 0, 8, 16), (0, 0, 8, 8), (8, 0, 8, 8), (0, 8, 8, 8), (8, 8, 8, 8))
SHAPE = (0, 1, 1, 4, 4, 5, 5, 5, 5)
_HOST = None


def host():
    global _HOST
    if _HOST is None:
        from mobiclipdecoder_amd import build
        L = C.CDLL(build.build_encpartshost())
        L.encq_host_bound.restype = C.c_size_t
        L.encq_host_bound.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
        L.encq_host_mb_bytes.restype = C.c_size_t
        L.encq_host_leaf_ok.argtypes = [C.c_int] * 8
        L.encq_host_vector_ok.argtypes = [C.c_int] * 6
        L.encq_host_inter.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, P, C.c_size_t, P, C.c_size_t, P, P, P, C.c_size_t, P, P, P, P, P, P, P, P, C.c_int]
        assert L.encq_host_mb_bytes() == E.MB_DTYPE.itemsize
        _HOST = L
    return _HOST


def host_encode(W, H, version, mode, pictures, refs, prev_q, q, slot_bytes=None, threads=1, pitch=None, ref_pitch=None):
    """the host model over a batch -> enc_inter_model.host_encode's dict with mv4 (N, macroblocks, 4) packed; the trees are mbs["luma_mode"]"""
    L = host()
    pictures, refs = np.ascontiguousarray(pictures, np.uint8), np.ascontiguousarray(refs, np.uint8)
    pq, q = np.ascontiguousarray(prev_q, np.uint8), np.ascontiguousarray(q, np.uint8)
    n, nmb = pictures.shape[0], (W // 16) * (H // 16)
    out, args = E.host_outputs(W, H, n, L.encq_host_bound(W, H, mode) if slot_bytes is None else slot_bytes, STATS_DTYPE, mv=np.uint32, mvp=np.uint32)
    out["mv4"] = np.zeros((n, nmb, 4), np.uint32)
    args = args[:-1] + [out["mv4"].ctypes.data, args[-1]]  # the quadrants' vectors stand in front of forms
    rc = L.encq_host_inter(W, H, version, mode, n, pictures.ctypes.data, pictures.shape[1] if pitch is None else pitch, refs.ctypes.data,
                           refs.shape[1] if ref_pitch is None else ref_pitch, pq.ctypes.data, q.ctypes.data, *args, threads)
    assert rc == 0, rc
    return out


# ---------------------------------------------------------------------------------------------------------------- sequences
def _regions(W, H, kind):
    """the luma mask of every region (bool (H, W)) and the sign (sx, sy) that points its vectors into the picture; the seams lie at
    xs, ys = 8 mod 16 through the middle macroblock column / row"""
    xs, ys = (W // 16 // 2) * 16 + 8, (H // 16 // 2) * 16 + 8
    yy, xx = np.mgrid[0:H, 0:W]
    L, R, U, D = xx < xs, xx >= xs, yy < ys, yy >= ys
    return {"lr": [(L, (1, 0)), (R, (-1, 0))], "tb": [(U, (0, 1)), (D, (0, -1))],
            "quad": [(L & U, (1, 1)), (R & U, (-1, 1)), (L & D, (1, -1)), (R & D, (-1, -1))],
            "top_only": [(L & U, (1, 1)), (R & U, (-1, 1)), (D, (0, -1))], "bottom_only": [(U, (0, 1)), (L & D, (1, -1)), (R & D, (-1, -1))],
            "left_only": [(L & U, (1, 1)), (L & D, (1, -1)), (R, (-1, 0))], "right_only": [(L, (1, 0)), (R & U, (-1, 1)), (R & D, (-1, -1))]}[kind]


def _moving_regions(rng, W, H, kind, steps):
    """T frames: frame 0 a sharp texture; in frame t every region is frame t - 1 moved by its own vector, steps[t - 1][r] = (|dx|, |dy|)
    half-pels for region r, signed to point into the picture: luma by the interpolation formula at (dx, dy), chroma at (dx >> 1, dy >> 1),
    so the vector that predicts region r of the SOURCE exactly from the source before is known"""
    pl = [M._lattice(rng, H, W, 16, 240, 2), M._lattice(rng, H // 2, W // 2, 40, 216, 2), M._lattice(rng, H // 2, W // 2, 40, 216, 2)]
    regs = _regions(W, H, kind)
    out = [E._i420(*pl)]
    pad = RANGE // 2 + 2
    for t in range(1, T):
        new = [np.zeros_like(p) for p in pl]
        for r, (mask, (sx, sy)) in enumerate(regs):
            ax, ay = steps[t - 1][r % len(steps[t - 1])]
            dx, dy = sx * ax, sy * ay
            for i, p in enumerate(pl):
                vx, vy, m = (dx, dy, mask) if i == 0 else (dx >> 1, dy >> 1, mask[::2, ::2])
                moved = M.interp(np.pad(p, pad, mode="edge"), pad, pad, p.shape[1], p.shape[0], vx, vy)
                new[i][m] = moved[m]
        pl = new
        out.append(E._i420(*pl))
    return np.stack(out)


# per frame step, per region (cycled): full-pel vectors first, then half-pel ones, then both; 2, 3 and 6 give odd chroma components
_STEPS = ([(4, 4), (2, 4), (4, 2), (6, 2)], [(3, 1), (1, 3), (3, 3), (1, 1)], [(6, 3), (2, 5), (5, 2), (3, 6)])


def sequence_sets(W, H):
    """enc_inter_model's sets and: 'two_motion' -- halves and quadrants in different motion, the set the usefulness condition is stated on,
    one quantiser --, 'half_seams' -- a seam in one half of the picture only, a quantiser per picture"""
    rng = np.random.default_rng(4242 + W * 3 + H)
    sets = dict(M.sequence_sets(W, H))
    sets["two_motion"] = (np.stack([_moving_regions(rng, W, H, k, _STEPS) for k in ("lr", "tb", "quad")]), np.full((3, T), 20, np.uint8))
    sets["half_seams"] = (np.stack([_moving_regions(rng, W, H, k, _STEPS) for k in ("top_only", "bottom_only", "left_only", "right_only")]),
                          np.array([[16, 16, 16, 16], [22, 22, 26, 26], [30, 28, 28, 34], [14, 18, 18, 18]], np.uint8))
    return sets


def chain(W, H, version, mode, frames, qs, **kw):
    """the host models over a set: list of T dicts (entry 0 is the intra model's), each P-frame predicted from the reconstruction before"""
    out = [E.host_encode(W, H, version, frames[:, 0], qs[:, 0])]
    for t in range(1, frames.shape[1]):
        out.append(host_encode(W, H, version, mode, frames[:, t], out[-1]["recon"], qs[:, t - 1], qs[:, t], **kw))
    return out


# ---------------------------------------------------------------------------------------------------------------- the stream, read back
def _residual(r, Tb, m, forms):
    """ue(cbp) and the coded blocks of one macroblock into the record m (enc_inter_model.parse_p_stream's reading of them)"""
    A, B, CBP = Tb["mobi_vx2table0_a"], Tb["mobi_vx2table0_b"], Tb["mobi_cbp_inter"]
    z = 0
    while r.take(1) == 0:
        z += 1
    m["cbp"] = CBP[(1 << z) - 1 + r.take(z)]
    for k in range(6):
        if not (int(m["cbp"]) >> k) & 1:
            continue
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
    """-> dict(dq, hdr_bits, end, forms, mv_bits, mbs (MB_DTYPE: bits = what the macroblock took, luma_mode = the tree byte), leaves: per
    macroblock the list of (x, y, w, h, code, ddx, ddy) in stream order).  The partition tree is read as the decoder's pblock reads it:
    shape s = 4 wi + hi, code 8 = two halves stacked (hi + 1), code 9 = side by side (wi + 1)."""
    Tb = tables.load()
    ver = 0 if version == 2 else 1
    LUT, NB, SH = Tb["mobi_part_lut"][ver], Tb["mobi_part_bits"][ver], Tb["mobi_part_shift"][ver]
    r = E._Bits(data)
    assert r.take(1) == 0, "not a P-frame"
    out = {"dq": M._se(r), "forms": np.zeros(4, np.int64)}
    out["hdr_bits"] = r.pos
    n = (W // 16) * (H // 16)
    mbs = np.zeros(n, E.MB_DTYPE)
    all_leaves, mvb = [], 0

    def pblock(wi, hi, x, y, leaves, path):
        s = 4 * wi + hi
        c = int(LUT[s][r.peek(32 - int(SH[s]))])
        assert c in (0, 1, 8, 9), "a partition code outside the encoder's subset"
        r.take(int(NB[s][c]))
        if c <= 1:
            ddx, ddy = (M._se(r), M._se(r)) if c else (0, 0)
            leaves.append((x, y, 16 >> wi, 16 >> hi, c, ddx, ddy))
        else:
            assert 16 >> wi >= 8 and 16 >> hi >= 8 and (wi, hi) != (1, 1), "nothing below 8x8 is split"
            path.append((s, c))
            if c == 8:
                pblock(wi, hi + 1, x, y, leaves, path)
                pblock(wi, hi + 1, x, y + (16 >> hi) // 2, leaves, path)
            else:
                pblock(wi + 1, hi, x, y, leaves, path)
                pblock(wi + 1, hi, x + (16 >> wi) // 2, y, leaves, path)

    for i, m in enumerate(mbs):
        start = r.pos
        leaves, path = [], []
        pblock(0, 0, 0, 0, leaves, path)
        tree = 0
        if path:
            tree = root = ROOT_8 if path[0][1] == 8 else ROOT_9
            for (x, y, w, h, *_rest) in leaves:  # a half that is split shows as 8x8 leaves in it
                second = (y >= 8) if root == ROOT_8 else (x >= 8)
                if w == 8 and h == 8:
                    tree |= SPLIT_SECOND if second else SPLIT_FIRST
        m["luma_mode"] = tree
        mvb += r.pos - start
        _residual(r, Tb, m, out["forms"])
        m["bits"] = r.pos - start
        all_leaves.append(leaves)
    out.update(mbs=mbs, leaves=all_leaves, mv_bits=mvb, end=r.pos)
    return out


def tree_leaves(tree):
    """the leaves (indices into LEAVES) of a tree byte in stream order"""
    if tree == 0:
        return [0]
    out = []
    for half in (0, 1):
        split = tree & (SPLIT_SECOND if half else SPLIT_FIRST)
        if tree & 3 == ROOT_8:
            out += [5 + 2 * half, 6 + 2 * half] if split else [1 + half]
        else:
            out += [5 + half, 7 + half] if split else [3 + half]
    return out


def leaf_of_quadrant(tree, qd):
    return next(l for l in tree_leaves(tree) if LEAVES[l][0] <= 8 * (qd & 1) < LEAVES[l][0] + LEAVES[l][2] and LEAVES[l][1] <= 8 * (qd >> 1) < LEAVES[l][1] + LEAVES[l][3])


# ---------------------------------------------------------------------------------------------------------------- the decisions, re-derived
def leaf_ok(W, H, x, y, w, h, dx, dy):
    """the w x h luma window at pixel (x, y) moved by (dx, dy) half-pels and the (w / 2) x (h / 2) chroma windows at (x / 2, y / 2) moved by
    (dx >> 1, dy >> 1), each with the column / row its phase adds, inside the planes' rectangles.  Works on numpy arrays of x, y."""
    X, Y, cdx, cdy = x + (dx >> 1), y + (dy >> 1), dx >> 1, dy >> 1
    cx, cy = x // 2 + (cdx >> 1), y // 2 + (cdy >> 1)
    return ((X >= 0) & (Y >= 0) & (X + w - 1 + (dx & 1) <= W - 1) & (Y + h - 1 + (dy & 1) <= H - 1) & (cx >= 0) & (cy >= 0) &
            (cx + w // 2 - 1 + (cdx & 1) <= W // 2 - 1) & (cy + h // 2 - 1 + (cdy & 1) <= H // 2 - 1))


def search_leaves(W, H, q, src_y, ref_y):
    """every leaf's best key and vector by brute force -> (cost (M, 9), dx (M, 9), dy (M, 9)): step 1 over every full-pel vector within RANGE
    in the leaf's own candidate set, step 2 over the eight half-pel neighbours of its winner; the order is cost, |dx| + |dy|, dy, dx"""
    mbw, mbh = W // 16, H // 16
    n = mbw * mbh
    lam = E._lam(q)
    pad = RANGE // 2 + 2
    ref = np.pad(ref_y, pad, mode="edge")
    mbx, mby = np.tile(np.arange(mbw), mbh) * 16, np.repeat(np.arange(mbh), mbw) * 16
    big = np.iinfo(np.int64).max
    best = np.full((n, 9), big)
    win = np.zeros((n, 9, 2), np.int64)
    for dy in range(-RANGE, RANGE + 1, 2):
        for dx in range(-RANGE, RANGE + 1, 2):
            q8 = np.abs(src_y - M.interp(ref, pad, pad, W, H, dx, dy)).reshape(mbh, 2, 8, mbw, 2, 8).sum((2, 5))  # (mbh, qy, mbw, qx)
            q8 = q8.transpose(0, 2, 1, 3).reshape(n, 2, 2)
            rate = lam * (M.se_bits(dx) + M.se_bits(dy))
            for l, (x, y, w, h) in enumerate(LEAVES):
                sad = q8[:, y // 8: (y + h) // 8, x // 8: (x + w) // 8].sum((1, 2))
                key = np.where(leaf_ok(W, H, mbx + x, mby + y, w, h, dx, dy), M._order((sad << 8) + rate, dx, dy), big)
                take = key < best[:, l]
                best[take, l], win[take, l] = key[take], (dx, dy)
    out = win.copy()
    for i in range(n):
        for l, (x, y, w, h) in enumerate(LEAVES):
            X, Y, fx, fy = int(mbx[i]) + x, int(mby[i]) + y, int(win[i, l, 0]), int(win[i, l, 1])
            s = src_y[Y: Y + h, X: X + w]
            for j in (-1, 0, 1):
                for k in (-1, 0, 1):
                    if (j or k) and leaf_ok(W, H, X, Y, w, h, fx + k, fy + j):
                        sad = int(np.abs(s - M.interp(ref_y, X, Y, w, h, fx + k, fy + j)).sum())
                        key = M._order((sad << 8) + lam * (M.se_bits(fx + k) + M.se_bits(fy + j)), fx + k, fy + j)
                        if key < best[i, l]:
                            best[i, l], out[i, l] = key, (fx + k, fy + j)
    return best // (64 * 128 * 128), out[:, :, 0], out[:, :, 1]


def decide_tree(version, q, cost):
    """the tree byte from the nine leaves' costs: J_leaf = C + lam * nb(s, 1); a half is its leaf unless the split is strictly cheaper;
    the root is unsplit on a tie, then code 8"""
    nb = tables.load()["mobi_part_bits"][0 if version == 2 else 1]
    lam = E._lam(q)
    J = [int(cost[l]) + lam * int(nb[SHAPE[l]][1]) for l in range(9)]
    t8, J8 = ROOT_8, lam * int(nb[0][8])
    for half, (leaf, qa, qb) in enumerate(((1, 5, 6), (2, 7, 8))):
        parts = lam * int(nb[1][9]) + J[qa] + J[qb]
        t8 |= (SPLIT_SECOND if half else SPLIT_FIRST) if parts < J[leaf] else 0
        J8 += min(J[leaf], parts)
    t9, J9 = ROOT_9, lam * int(nb[0][9])
    for half, (leaf, qa, qb) in enumerate(((3, 5, 7), (4, 6, 8))):
        parts = lam * int(nb[4][8]) + J[qa] + J[qb]
        t9 |= (SPLIT_SECOND if half else SPLIT_FIRST) if parts < J[leaf] else 0
        J9 += min(J[leaf], parts)
    return 0 if J[0] <= J8 and J[0] <= J9 else t8 if J8 <= J9 else t9


def rederive_blocks(ref, W, H, q, source, reference, dx4, dy4):
    """prediction and residual of one P-frame from its source, the decoded frame before and the quadrants' vectors (M, 4): luma block k with
    Qk's vector, the chroma blocks' 4x4 quadrants with (dx >> 1, dy >> 1) of Q0..Q3 -> dict(cbp, lev, bits (blocks only), clamp, range, recon)"""
    mbw, mbh = W // 16, H // 16
    n = mbw * mbh
    sp, rp = E.planes(source.astype(np.int64), W, H), E.planes(reference.astype(np.int64), W, H)
    src_b, pred_b = np.zeros((n, 6, 8, 8), np.int64), np.zeros((n, 6, 8, 8), np.int64)
    for i in range(n):
        x, y = i % mbw, i // mbw
        for k in range(4):
            bx, by = x * 16 + (k & 1) * 8, y * 16 + (k >> 1) * 8
            src_b[i, k] = sp[0][by: by + 8, bx: bx + 8]
            pred_b[i, k] = M.interp(rp[0], bx, by, 8, 8, int(dx4[i, k]), int(dy4[i, k]))
        for k in (4, 5):
            src_b[i, k] = sp[k - 3][y * 8: y * 8 + 8, x * 8: x * 8 + 8]
            for qd in range(4):
                cx, cy = x * 8 + (qd & 1) * 4, y * 8 + (qd >> 1) * 4
                pred_b[i, k, (qd >> 1) * 4: (qd >> 1) * 4 + 4, (qd & 1) * 4: (qd & 1) * 4 + 4] = M.interp(rp[k - 3], cx, cy, 4, 4, int(dx4[i, qd]) >> 1, int(dy4[i, qd]) >> 1)
    b = E._code_blocks(ref, q, src_b.reshape(n * 6, 8, 8), pred_b.reshape(n * 6, 8, 8))
    res = {"cbp": (b["coded"].reshape(n, 6) * (1 << np.arange(6))).sum(1), "lev": b["lev"].reshape(n, 6, 64).astype(np.int16), "bits": b["bits"].reshape(n, 6).sum(1),
           "clamp": int(b["clamp"].sum()), "range": int(b["range"].sum())}
    rec, out = b["rec"].reshape(n, 6, 8, 8), [np.zeros_like(p) for p in sp]
    for i in range(n):
        x, y = i % mbw, i // mbw
        for k in range(4):
            out[0][y * 16 + (k >> 1) * 8: y * 16 + (k >> 1) * 8 + 8, x * 16 + (k & 1) * 8: x * 16 + (k & 1) * 8 + 8] = rec[i, k]
        for k in (4, 5):
            out[k - 3][y * 8: y * 8 + 8, x * 8: x * 8 + 8] = rec[i, k]
    res["recon"] = E._i420(*out)
    return res
