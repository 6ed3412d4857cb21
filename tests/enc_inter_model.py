"""What the inter encoder's tests share (tests/test_encode_inter_model.py on the CPU, tests/test_encode_inter_gpu.py on the GPU):

  host model     tests/tools/mobi_encode_inter_host.cpp: the product's csrc/mobi_encode_inter.h run on the CPU (build.build_encinterhost)
  sequences      N clips of an I-frame and three P-frames each, with a quantiser per picture: a textured picture translated by known full-
                 and half-pel vectors, a noisy sequence, a saturated one (fixed seeds, any multiple-of-16 size); and `still`, a scene
                 that does not move, for the geometry tests (tests/test_encode_geometry_gpu.py)
  chain          the host model over a set: the I-frames from the intra host model, every P-frame against the reconstruction before it
  parse_p_stream a P-frame of the encoder's subset read back with the ORACLE's tables: header delta, per macroblock partition code, vector
                 difference, cbp, levels, bits
  rederive       an independent restatement: the interpolation from its formula in numpy, the search by brute force over the candidate set,
                 the median predictor, the transform coding from tests/tools/txcode_ref.c
Nothing here includes the product's encoder headers."""
import ctypes as C

import numpy as np

from tests import enc_model as E
from tests import tables

P = C.c_void_p
STATS_DTYPE = np.dtype([("bits", "<u8"), ("sad", "<u8"), ("mv_bits", "<u8"), ("coded_blocks", "<u4"), ("fallback_clamp", "<u4"),
                        ("fallback_level", "<u4"), ("code0", "<u4"), ("nonzero_mv", "<u4"), ("halfpel_mv", "<u4"), ("reserved", "<u4", 4)])
VERSIONS = E.VERSIONS
SHAPES = ((16, 16), (48, 32), (272, 208))
RANGE = 16  # half-pels, the full-pel step's reach: DESIGN.md, "Inter encoder" (MOBI_ENCP_RANGE; test_range_constant pins the three)
T = 4       # frames of a sequence: I, P, P, P
_HOST = None


def host():
    global _HOST
    if _HOST is None:
        from mobiclipdecoder_amd import build
        L = C.CDLL(build.build_encinterhost())
        L.encp_host_bound.restype = C.c_size_t
        L.encp_host_bound.argtypes = [C.c_uint32, C.c_uint32]
        L.encp_host_check.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_size_t, C.c_size_t, P, P, C.c_size_t]
        L.encp_host_mb_bytes.restype = C.c_size_t
        L.encp_host_inter.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, P, C.c_size_t, P, C.c_size_t, P, P, P, C.c_size_t, P, P, P, P, P, P, P, C.c_int]
        assert L.encp_host_mb_bytes() == E.MB_DTYPE.itemsize
        _HOST = L
    return _HOST


def unpack_mv(mv):
    """packed vectors (dx low, dy high 16 bits) -> (dx, dy) int arrays"""
    mv = np.asarray(mv, np.uint32)
    return (mv & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64), (mv >> 16).astype(np.uint16).view(np.int16).astype(np.int64)


def host_encode(W, H, version, pictures, refs, prev_q, q, slot_bytes=None, threads=1, pitch=None, ref_pitch=None):
    """the host model over a batch -> the intra model's dict (enc_model.host_outputs) with mv, mvp (N, macroblocks) packed before forms"""
    L = host()
    pictures, refs = np.ascontiguousarray(pictures, np.uint8), np.ascontiguousarray(refs, np.uint8)
    pq, q = np.ascontiguousarray(prev_q, np.uint8), np.ascontiguousarray(q, np.uint8)
    out, args = E.host_outputs(W, H, pictures.shape[0], L.encp_host_bound(W, H) if slot_bytes is None else slot_bytes, STATS_DTYPE, mv=np.uint32, mvp=np.uint32)
    rc = L.encp_host_inter(W, H, version, pictures.shape[0], pictures.ctypes.data, pictures.shape[1] if pitch is None else pitch, refs.ctypes.data,
                           refs.shape[1] if ref_pitch is None else ref_pitch, pq.ctypes.data, q.ctypes.data, *args, threads)
    assert rc == 0, rc
    return out


# ---------------------------------------------------------------------------------------------------------------- sequences
def _lattice(rng, h, w, lo=0, hi=256, cell=1):
    a = rng.integers(lo, hi, ((h + cell - 1) // cell, (w + cell - 1) // cell))
    return np.kron(a, np.ones((cell, cell), np.int64))[:h, :w]


def _translated(rng, W, H, steps, cell=2, amp=(16, 240)):
    """T frames cut from one canvas; frame t = frame t - 1 moved by steps[t - 1] = (vx, vy) FULL pels (even, so that chroma moves whole
    samples too): the vector that predicts it exactly is (2 vx, 2 vy) half-pels"""
    M = 40
    cy, cu, cv = (_lattice(rng, H + 2 * M, W + 2 * M, amp[0], amp[1], cell), _lattice(rng, H // 2 + M, W // 2 + M, 40, 216, cell),
                  _lattice(rng, H // 2 + M, W // 2 + M, 40, 216, cell))
    x = y = 0
    out = []
    for t in range(T):
        if t:
            x, y = x + steps[t - 1][0], y + steps[t - 1][1]
        out.append(E._i420(cy[M + y: M + y + H, M + x: M + x + W], cu[M // 2 + y // 2: M // 2 + y // 2 + H // 2, M // 2 + x // 2: M // 2 + x // 2 + W // 2],
                           cv[M // 2 + y // 2: M // 2 + y // 2 + H // 2, M // 2 + x // 2: M // 2 + x // 2 + W // 2]))
    return np.stack(out)


def _smooth(W, H, shifts, seed):
    """T frames sampled from one smooth function; frame t is sampled shifts[t] = (sx, sy) HALF-pels from frame 0, so a half-pel vector
    predicts it better than any full-pel one"""
    k = 0.11 + 0.013 * (seed % 5)
    f = lambda x, y, a, b, c: 128 + 70 * np.sin(k * a * x + 0.3 * c) * np.cos(k * b * y + 0.2 * c) + 40 * np.sin(k * 0.7 * (x + y) + c)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx = np.mgrid[0:H // 2, 0:W // 2].astype(np.float64) * 2
    out = []
    for sx, sy in shifts:
        out.append(E._i420(np.clip(np.rint(f(xx + sx / 2, yy + sy / 2, 1.0, 1.3, 1)), 0, 255), np.clip(np.rint(f(cx + sx / 2, cy + sy / 2, 0.6, 0.5, 2)), 0, 255),
                           np.clip(np.rint(f(cx + sx / 2, cy + sy / 2, 0.4, 0.7, 3)), 0, 255)))
    return np.stack(out)


def _noisy(rng, W, H):
    base = _translated(rng, W, H, [(2, 0), (0, 2), (-2, -2)], cell=4)
    return np.clip(base.astype(np.int64) + rng.integers(-24, 25, base.shape), 0, 255).astype(np.uint8)


def _saturated(rng, W, H):
    return np.stack([E._i420(rng.integers(0, 2, (H, W)) * 255, rng.integers(0, 2, (H // 2, W // 2)) * 255, rng.integers(0, 2, (H // 2, W // 2)) * 255) for _ in range(T)])


def sequence_sets(W, H):
    """name -> (frames (N, T, frame) uint8, quantizers (N, T) uint8).  'fullpel' is the pure full-pel translation the usefulness condition
    is stated on; 'mixed5' has a quantiser per picture and pictures with and without a change of quantiser."""
    rng = np.random.default_rng(771 + W * 5 + H)
    full = _smooth(W, H, [(0, 0), (8, 4), (-8, 4), (-8, 20)], 1)        # steps (8, 4), (-16, 0), (0, 16): whole samples, smooth content
    full2 = _translated(rng, W, H, [(8, -8), (2, -2), (-6, 4)])        # (16, -16), (4, -4), (-12, 8): a sharp texture, exact matches
    half = _smooth(W, H, [(0, 0), (1, 0), (1, 1), (2, 2)], 1)          # steps (1, 0), (0, 1), (1, 1)
    half2 = _smooth(W, H, [(0, 0), (-1, -1), (-4, -1), (-4, 2)], 2)    # steps (-1, -1), (-3, 0), (0, 3)
    return {
        "fullpel": (full[None], np.array([[26, 26, 26, 26]], np.uint8)),
        "mixed5": (np.stack([full2, half, half2, _noisy(rng, W, H), _saturated(rng, W, H)]),
                   np.array([[14, 14, 17, 12], [20, 20, 20, 20], [24, 30, 30, 22], [31, 40, 40, 52], [52, 52, 45, 45]], np.uint8)),
        "sat_q52": (_saturated(rng, W, H)[None], np.array([[52, 52, 52, 52]], np.uint8)),
    }


SETS = ("fullpel", "mixed5", "sat_q52")
# what the geometry tests run (enc_model.GEOMETRY_SHAPES): the mixed five and the still scene below, which is no member of SETS
GEOMETRY_SETS = ("mixed5", "still")
STILL_Q = np.array([[14, 14, 14, 14], [20, 20, 20, 20], [24, 30, 30, 22]], np.uint8)  # two clips at one quantiser, one that changes it (dq != 0)
_STILL = {}


def still(W, H):
    """-> (frames (3, T, frame), quantizers (3, T)): a scene that does not move.  Frame 0 of the first three clips of 'mixed5'; the source of
    frame t is the model's own reconstruction of frame t - 1, made by chaining the model, so every P-macroblock has the zero vector and no
    residual: 2 bits on Moflex3DS, 3 on ModsDS, and 16 or 10 macroblocks in one 32-bit word of the stream.  (Neither the intra model nor
    an unchanged picture depends on the version or on the partition mode: tests/test_encode_*_model.py, test_geometry_*, assert both.)"""
    if (W, H) not in _STILL:
        first = sequence_sets(W, H)["mixed5"][0][:3, 0]
        frames, rec = [first], E.host_encode(W, H, 2, first, STILL_Q[:, 0])["recon"]
        for t in range(1, T):
            frames.append(rec)
            rec = host_encode(W, H, 2, rec, rec, STILL_Q[:, t - 1], STILL_Q[:, t])["recon"]
        _STILL[(W, H)] = (np.ascontiguousarray(np.stack(frames, 1)), STILL_Q)
    return _STILL[(W, H)]


def geometry_set(W, H, name):
    """one of GEOMETRY_SETS as sequence_sets gives its own: (frames (N, T, frame), quantizers (N, T))"""
    return still(W, H) if name == "still" else sequence_sets(W, H)[name]


def chain(W, H, version, frames, qs, **kw):
    """the host models over a set: list of T dicts (host_encode's keys; entry 0 is the intra model's), each P-frame predicted from the
    reconstruction of the frame before"""
    out = [E.host_encode(W, H, version, frames[:, 0], qs[:, 0])]
    for t in range(1, frames.shape[1]):
        out.append(host_encode(W, H, version, frames[:, t], out[-1]["recon"], qs[:, t - 1], qs[:, t], **kw))
    return out


def oracle_chain(W, H, version, streams):
    """the oracle over one clip's frame streams in order -> list of (packed I420, bytes consumed, quantiser)"""
    from tests.oracle_binding import OracleDecoder
    o = OracleDecoder(W, H, version)
    S, res = o.Stride, []
    for data in streams:
        o.Data, o.Offset = bytes(data), 0
        r = o.DecodeFrame()
        assert r is not None, f"the oracle threw {o.last_error} at offset {o.Offset} in frame {len(res)}"
        res.append((E._i420(r[0][:, :W], r[1][:, : W // 2], r[1][:, S // 2: S // 2 + W // 2]), o.Offset, o.Quantizer))
    o.close()
    return res


# ---------------------------------------------------------------------------------------------------------------- the stream, read back
def _se(r):
    z = 0
    while r.take(1) == 0:
        z += 1
    u = (1 << z) - 1 + r.take(z) + 1
    return (1 - u) >> 1 if u & 1 else u >> 1


def parse_p_stream(data, W, H, version):
    """-> dict(dq, mbs (MB_DTYPE; bits = what the macroblock took), code, ddx, ddy (per macroblock), mv_bits, forms, hdr_bits, end)"""
    Tb = tables.load()
    A, B, CBP = Tb["mobi_vx2table0_a"], Tb["mobi_vx2table0_b"], Tb["mobi_cbp_inter"]
    ver = 0 if version == 2 else 1
    lut, nbits, shift = Tb["mobi_part_lut"][ver][0], Tb["mobi_part_bits"][ver][0], int(Tb["mobi_part_shift"][ver][0])
    r = E._Bits(data)
    assert r.take(1) == 0, "not a P-frame"
    out = {"dq": _se(r), "forms": np.zeros(4, np.int64)}
    out["hdr_bits"] = r.pos
    n = (W // 16) * (H // 16)
    mbs = np.zeros(n, E.MB_DTYPE)
    code, ddx, ddy, mvb = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), 0
    for i, m in enumerate(mbs):
        start = r.pos
        c = int(lut[r.peek(32 - shift)])
        assert c in (0, 1), "a partition code outside the encoder's subset"
        r.take(int(nbits[c]))
        code[i] = c
        if c:
            ddx[i], ddy[i] = _se(r), _se(r)
        mvb += r.pos - start
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
                out["forms"][form] += 1
                p += run
                assert p < 64, "run past the block"
                m["lev"][k][p] = val
                p += 1
                if last:
                    break
            assert m["lev"][k].any()
        m["bits"] = r.pos - start
    out.update(mbs=mbs, code=code, ddx=ddx, ddy=ddy, mv_bits=mvb, end=r.pos)
    return out


# ---------------------------------------------------------------------------------------------------------------- the decisions, re-derived
def se_bits(v):
    return E._ue_bits(2 * v - 1 if v > 0 else -2 * v)


def vector_ok(W, H, mbx, mby, dx, dy):
    """the Y, U and V windows of (dx, dy), the column / row a half-pel phase adds included, inside the planes' rectangles"""
    x, y, cdx, cdy = mbx * 16 + (dx >> 1), mby * 16 + (dy >> 1), dx >> 1, dy >> 1
    cx, cy = mbx * 8 + (cdx >> 1), mby * 8 + (cdy >> 1)
    return (x >= 0 and y >= 0 and x + 15 + (dx & 1) <= W - 1 and y + 15 + (dy & 1) <= H - 1 and cx >= 0 and cy >= 0 and
            cx + 7 + (cdx & 1) <= W // 2 - 1 and cy + 7 + (cdy & 1) <= H // 2 - 1)


def interp(plane, x, y, w, h, vx, vy):
    """the w x h prediction at (x, y) of a plane (int64) for vector (vx, vy) in half-pels, from the formula: whole part = v >> 1; an odd
    component averages two neighbours as (a >> 1) + (b >> 1); both odd: that average of the two rows' averages, truncating at every step"""
    X, Y = x + (vx >> 1), y + (vy >> 1)
    a = plane[Y: Y + h, X: X + w]
    if not (vx & 1) and not (vy & 1):
        return a
    if not (vy & 1):
        return (a >> 1) + (plane[Y: Y + h, X + 1: X + 1 + w] >> 1)
    c = plane[Y + 1: Y + 1 + h, X: X + w]
    if not (vx & 1):
        return (a >> 1) + (c >> 1)
    return (((a >> 1) + (plane[Y: Y + h, X + 1: X + 1 + w] >> 1)) >> 1) + (((c >> 1) + (plane[Y + 1: Y + 1 + h, X + 1: X + 1 + w] >> 1)) >> 1)


def _order(cost, dx, dy):
    """the tie rule as one sortable integer: cost, then |dx| + |dy|, then dy, then dx (every field non-negative and below its radix)"""
    return ((cost * 64 + abs(dx) + abs(dy)) * 128 + dy + 64) * 128 + dx + 64


def search_picture(W, H, q, src_y, ref_y):
    """v* of every macroblock by brute force -> (dx, dy, fdx, fdy, udx, udy) int arrays: the chosen vector, the full-pel step's winner and
    the full-pel winner of the UNCONSTRAINED search (every vector within RANGE on an edge-replicated reference, whatever the rectangle
    says: the coverage condition needs it).  All candidates of all macroblocks are priced, then the smallest under the tie rule is taken."""
    mbw, mbh = W // 16, H // 16
    lam = E._lam(q)
    pad = RANGE // 2 + 2
    ref = np.pad(ref_y, pad, mode="edge")
    mbx, mby = np.tile(np.arange(mbw), mbh), np.repeat(np.arange(mbh), mbw)
    big = np.iinfo(np.int64).max
    best_c, best_u = np.full(mbw * mbh, big), np.full(mbw * mbh, big)
    win_c, win_u = np.zeros((mbw * mbh, 2), np.int64), np.zeros((mbw * mbh, 2), np.int64)
    for dy in range(-RANGE, RANGE + 1, 2):
        for dx in range(-RANGE, RANGE + 1, 2):
            sad = np.abs(src_y - interp(ref, pad, pad, W, H, dx, dy)).reshape(mbh, 16, mbw, 16).sum((1, 3)).ravel()
            key = _order((sad << 8) + lam * (se_bits(dx) + se_bits(dy)), dx, dy)
            ok = np.array([vector_ok(W, H, x, y, dx, dy) for x, y in zip(mbx, mby)])
            for best, win, k in ((best_c, win_c, np.where(ok, key, big)), (best_u, win_u, key)):
                take = k < best
                best[take], win[take] = k[take], (dx, dy)
    out = win_c.copy()
    for i in range(mbw * mbh):
        x, y, fx, fy = int(mbx[i]), int(mby[i]), int(win_c[i, 0]), int(win_c[i, 1])
        s = src_y[y * 16: y * 16 + 16, x * 16: x * 16 + 16]
        best = best_c[i]
        for j in (-1, 0, 1):
            for k in (-1, 0, 1):
                if (j or k) and vector_ok(W, H, x, y, fx + k, fy + j):
                    sad = int(np.abs(s - interp(ref_y, x * 16, y * 16, 16, 16, fx + k, fy + j)).sum())
                    key = _order((sad << 8) + lam * (se_bits(fx + k) + se_bits(fy + j)), fx + k, fy + j)
                    if key < best:
                        best, out[i] = key, (fx + k, fy + j)
    return out[:, 0], out[:, 1], win_c[:, 0], win_c[:, 1], win_u[:, 0], win_u[:, 1]


def med3(a, b, c):
    return max(min(a, b), min(max(a, b), c))


def rederive(ref, W, H, version, q, source, reference, mv):
    """One P-frame from its source, the DECODED frame before it and the decoded vectors mv = (dx, dy) arrays (the search is checked apart):
    -> dict(pdx, pdy (predictors), code, cbp, lev (M, 6, 64), bits (per macroblock, syntax included), mv_bits, clamp, range, recon)"""
    mbw, mbh = W // 16, H // 16
    M = mbw * mbh
    Tb = tables.load()
    ver = 0 if version == 2 else 1
    pbits = Tb["mobi_part_bits"][ver][0]
    inv = {int(c): i for i, c in reversed(list(enumerate(Tb["mobi_cbp_inter"])))}
    sp, rp = E.planes(source.astype(np.int64), W, H), E.planes(reference.astype(np.int64), W, H)
    dx, dy = mv
    at = lambda a, x, y: int(a[y * mbw + x]) if 0 <= x < mbw and 0 <= y < mbh else 0
    res = {"pdx": np.zeros(M, np.int64), "pdy": np.zeros(M, np.int64), "recon": [np.zeros_like(p) for p in sp]}
    src_b, pred_b = np.zeros((M, 6, 8, 8), np.int64), np.zeros((M, 6, 8, 8), np.int64)
    for i in range(M):
        x, y = i % mbw, i // mbw
        res["pdx"][i] = med3(at(dx, x - 1, y), at(dx, x, y - 1), at(dx, x + 1, y - 1) if y > 0 else 0)
        res["pdy"][i] = med3(at(dy, x - 1, y), at(dy, x, y - 1), at(dy, x + 1, y - 1) if y > 0 else 0)
        vx, vy = int(dx[i]), int(dy[i])
        for k in range(6):
            if k < 4:
                pl, bx, by, ux, uy = 0, x * 16 + (k & 1) * 8, y * 16 + (k >> 1) * 8, vx, vy
            else:
                pl, bx, by, ux, uy = k - 3, x * 8, y * 8, vx >> 1, vy >> 1
            src_b[i, k] = sp[pl][by: by + 8, bx: bx + 8]
            pred_b[i, k] = interp(rp[pl], bx, by, 8, 8, ux, uy)
    b = E._code_blocks(ref, q, src_b.reshape(M * 6, 8, 8), pred_b.reshape(M * 6, 8, 8))
    coded = b["coded"].reshape(M, 6)
    res["cbp"] = (coded * (1 << np.arange(6))).sum(1)
    res["lev"] = b["lev"].reshape(M, 6, 64).astype(np.int16)
    res["clamp"], res["range"] = int(b["clamp"].sum()), int(b["range"].sum())
    res["code"] = ((dx != res["pdx"]) | (dy != res["pdy"])).astype(np.int64)
    mvb = np.array([int(pbits[c]) + (se_bits(int(dx[i] - res["pdx"][i])) + se_bits(int(dy[i] - res["pdy"][i])) if c else 0) for i, c in enumerate(res["code"])], np.int64)
    res["mv_bits"] = int(mvb.sum())
    res["bits"] = mvb + np.array([E._ue_bits(inv[int(c)]) for c in res["cbp"]], np.int64) + b["bits"].reshape(M, 6).sum(1)
    rec = b["rec"].reshape(M, 6, 8, 8)
    for i in range(M):
        x, y = i % mbw, i // mbw
        for k in range(6):
            if k < 4:
                res["recon"][0][y * 16 + (k >> 1) * 8: y * 16 + (k >> 1) * 8 + 8, x * 16 + (k & 1) * 8: x * 16 + (k & 1) * 8 + 8] = rec[i, k]
            else:
                res["recon"][k - 3][y * 8: y * 8 + 8, x * 8: x * 8 + 8] = rec[i, k]
    res["recon"] = E._i420(*res["recon"])
    return res
