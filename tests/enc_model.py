"""What the intra encoder's tests share (tests/test_encode_model.py on the CPU, tests/test_encode_gpu.py on the GPU):

  host model     tests/tools/mobi_encode_host.cpp: the product's csrc/mobi_encode.h run on the CPU (built by build.build_enchost)
  picture sets   bars, ramps, flat areas, uniform noise, saturated 0 / 255 noise, with fixed seeds, at any multiple-of-16 size
  parse_stream   an I-frame of the encoder's subset read back with the ORACLE's tables: header, per macroblock modes, cbp, levels, bits
  rederive       an independent restatement of the decisions: predictors from their formulas in numpy, transform coding from the scalar
                 restatement tests/tools/txcode_ref.c (ref_encode_batch), neighbours from the oracle-decoded picture
Nothing here includes the product's encoder header."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mobiclipdecoder_amd", "csrc")
TOOLS = os.path.join(ROOT, "tests", "tools")
VXREF = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "encoder_vlc_ref.npy")).astype(np.int16))
P = C.c_void_p
MB_DTYPE = np.dtype([("lev", "<i2", (6, 64)), ("bits", "<u4"), ("luma_mode", "u1"), ("chroma_mode", "u1"), ("cbp", "u1"), ("pad", "u1")])
STATS_DTYPE = np.dtype([("bits", "<u8"), ("sad", "<u8"), ("luma_modes", "<u4", 4), ("chroma_modes", "<u4", 4), ("coded_blocks", "<u4"),
                        ("fallback_clamp", "<u4"), ("fallback_level", "<u4"), ("reserved", "<u4")])
VERSIONS = (2, 1)  # MOBI_VERSION_MOFLEX3DS, MOBI_VERSION_MODSDS
SHAPES = ((16, 16), (48, 32), (256, 192), (272, 208))
# The shapes of the geometry tests (tests/test_encode_geometry_gpu.py and test_geometry_* of the three model tests), each the smallest that
# reaches what stands beside it.  The scan of the bit lengths (csrc/mobi_encode_write.h) goes over the macroblocks 256 at a time and the
# writer 64 at a time; the host models have neither, they sum and write in raster order.
GEOMETRY_SHAPES = (
    (256, 256),    # 16 x 16 = 256 macroblocks: one scan round exactly full, the writer's fourth workgroup exactly full
    (272, 256),    # 17 x 16 = 272: a second scan round with 16 live lanes, a fifth writer workgroup partly filled
    (1024, 144),   # 64 x 9 = 576: three scan rounds; the widest picture there is (the decoder's stride class 1024); mobi_enc_diag_range
                   #   gives x_lo > 0 on 63 of its 72 diagonals
    (16, 4112),    # 1 x 257 = 257: one column, 257 diagonals of one macroblock, a second round with one live lane, vector predictors
                   #   whose left and top-right neighbours would wrap
    (32, 80),      # 2 x 5 = 10: taller than wide, the width ends four of the six diagonals (x_hi < d) and x_lo > 0 on the last; cheap
    (1024, 16),    # 64 x 1 = 64: one row, no neighbour above anywhere, a search window mostly outside the picture
)
LAM_BASE = (218, 274, 345)
_HOST = None


def geometry_preconditions(bits, total, where):
    """What lets the GPU comparison above 256 macroblocks (tests/test_encode_geometry_gpu.py) fail, asserted on a model's output for the five
    pictures of one call of 'mixed5' (bits: (5, macroblocks) per macroblock, total: (5,) with the header).  For EVERY picture the
    macroblocks from index 256 on have bits.  For at least four of the five -- printed: which -- their lengths are not all the same, and
    for at least four macroblock 256 starts inside a 32-bit word, so that the first word of the second scan round is one that two
    workgroups of the writer share.  Every picture cannot be had for these two from the mixed five: the flat I-frame's last macroblock
    row is sixteen times the same 8 bits, the first P-frame of saturated noise (q = 52 after 52) is 2 or 3 bits everywhere, and in 7 of
    the 42 calls one picture's offset is a multiple of 32.  A picture of 1 x 257 has one macroblock behind the first 256, which cannot
    differ from itself: there macroblocks 255 and 256 must differ."""
    bits = np.asarray(bits).astype(np.int64)
    n, nmb = bits.shape
    assert nmb > 256 and n == 5
    assert (bits[:, 256:] > 0).all(), where
    tail = bits[:, 256:] if nmb > 257 else bits[:, 255:]
    differ = np.array([len(set(t.tolist())) > 1 for t in tail])
    offset = np.asarray(total).astype(np.int64) - bits.sum(1) + bits[:, :256].sum(1)  # the header and what stands before macroblock 256
    inside = offset % 32 != 0
    print(where, "lengths differ:", differ.tolist(), "macroblock 256 inside a word:", inside.tolist())
    assert differ.sum() >= 4 and inside.sum() >= 4, (where, differ, inside)
_REF = None


def host():
    global _HOST
    if _HOST is None:
        from mobiclipdecoder_amd import build
        L = C.CDLL(build.build_enchost())
        L.enc_host_bound.restype = C.c_size_t
        L.enc_host_bound.argtypes = [C.c_uint32, C.c_uint32]
        L.enc_host_check.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_size_t, P, C.c_int, C.c_size_t]
        L.enc_host_mb_bytes.restype = C.c_size_t
        L.enc_host_intra.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, P, C.c_size_t, P, C.c_int, P, C.c_size_t, P, P, P, P, P, C.c_int]
        L.enc_host_symbol_walk.argtypes = [P, P, P]
        L.enc_host_block.argtypes = [C.c_int, P, P, P, P, P]
        L.enc_host_write.restype = C.c_size_t
        L.enc_host_write.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, P, P, C.c_size_t]
        assert L.enc_host_mb_bytes() == MB_DTYPE.itemsize
        _HOST = L
    return _HOST


def txref(tmpdir):
    """the scalar restatement of the transform coding (the one tests/test_txcode.py judges the kernel by)"""
    global _REF
    if _REF is None:
        so = os.path.join(str(tmpdir), "libtxcode_ref.so")
        subprocess.run(["gcc", "-O2", "-std=c99", "-fPIC", "-shared", "-fwrapv", "-ffp-contract=off", "-Wall", "-Wno-unused-const-variable", "-I" + CSRC,
                        os.path.join(TOOLS, "txcode_ref.c"), "-o", so, "-lm"], check=True)
        L = C.CDLL(so)
        L.ref_encode_batch.argtypes = [C.c_int, C.c_int, P, C.c_long, P, P, P, P, P, P, P, P]
        _REF = L
    return _REF


def host_outputs(W, H, n, slot, stats_dtype, **more):
    """what either host model fills -> (dict(streams (N, slot) uint8, bytes (N,), recon (N, frame), stats (N,), mbs (N, macroblocks), one
    (N, macroblocks) array of dtype per name in `more`, forms (4,)), the arguments of the model's entry point from `streams` to `forms`)"""
    nmb = (W // 16) * (H // 16)
    out = {"streams": np.full((n, slot), 0xAA, np.uint8), "bytes": np.zeros(n, np.int32), "recon": np.zeros((n, W * H * 3 // 2), np.uint8),
           "stats": np.zeros(n, stats_dtype), "mbs": np.zeros((n, nmb), MB_DTYPE), **{k: np.zeros((n, nmb), dt) for k, dt in more.items()},
           "forms": np.zeros(4, np.uint32)}
    ptrs = [a.ctypes.data for a in out.values()]  # in the entry points' order; the slot's size follows the slots
    return out, ptrs[:1] + [slot] + ptrs[1:]


def host_encode(W, H, version, pictures, quantizers, yuv_format=0, slot_bytes=None, threads=1, pitch=None):
    """the host model over a batch -> host_outputs' dict"""
    L = host()
    pictures = np.ascontiguousarray(pictures, np.uint8)
    q = np.ascontiguousarray(quantizers, np.uint8)
    out, args = host_outputs(W, H, pictures.shape[0], L.enc_host_bound(W, H) if slot_bytes is None else slot_bytes, STATS_DTYPE)
    rc = L.enc_host_intra(W, H, version, pictures.shape[0], pictures.ctypes.data, pictures.shape[1] if pitch is None else pitch, q.ctypes.data, yuv_format,
                          *args, threads)
    assert rc == 0, rc
    return out


# ---------------------------------------------------------------------------------------------------------------- pictures
def _i420(y, u, v):
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()]).astype(np.uint8)


def picture_sets(W, H):
    """name -> (pictures (N, frame) uint8, quantizers (N,)): one set of five with a quantiser each, and sets of one.  Seeds are fixed:
    tests/test_encode_model.py checks that, over all shapes, the sets meet the coverage condition that makes them worth running."""
    rng = np.random.default_rng(20240 + W * 7 + H)
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = np.mgrid[0:H // 2, 0:W // 2]
    noise = lambda lo, hi, shape: rng.integers(lo, hi, shape)
    vbars = _i420(((xx // 3) % 2) * 200 + 20 + noise(0, 6, (H, W)), ((cx // 2) % 2) * 120 + 60, 128 + noise(-3, 4, cy.shape))
    hbars = _i420(((yy // 5) % 2) * 180 + 40 + noise(0, 4, (H, W)), ((cy // 3) % 2) * 100 + 70 + noise(0, 3, cy.shape), ((cy // 2) % 2) * 90 + 80)
    ramps = _i420((xx * 3 + yy * 2) % 256, (cx * 5) % 256, (cy * 7) % 256)
    flat = _i420(np.where(xx < W // 2, 90, 200) + (yy >= H // 2) * 30, np.full(cy.shape, 77), np.where(cy < H // 4, 30, 220))
    uni = _i420(noise(0, 256, (H, W)), noise(0, 256, cy.shape), noise(64, 192, cy.shape))
    sat = lambda: _i420(noise(0, 2, (H, W)) * 255, noise(0, 2, cy.shape) * 255, noise(0, 2, cy.shape) * 255)
    # black and white macroblock-sized fields: a flat residual of 255 is the largest DC there is (level range at low quantisers)
    fields = _i420(((xx // 16 + yy // 16) % 2) * 255, ((cx // 8) % 2) * 255, ((cy // 8 + cx // 8) % 2) * 255)
    soft = _i420(128 + noise(-12, 13, (H, W)), 128 + noise(-20, 21, cy.shape), 128 + noise(-6, 7, cy.shape))
    return {
        "mixed5": (np.stack([vbars, hbars, ramps, flat, uni]), np.array([14, 23, 31, 40, 52], np.uint8)),
        "sat_q52": (sat()[None], np.array([52], np.uint8)),
        "sat_q12": (sat()[None], np.array([12], np.uint8)),
        "hard5": (np.stack([fields, sat(), soft, uni, fields]), np.array([12, 45, 12, 20, 52], np.uint8)),
    }


def planes(frame, W, H):
    y = frame[: W * H].reshape(H, W)
    u = frame[W * H: W * H * 5 // 4].reshape(H // 2, W // 2)
    v = frame[W * H * 5 // 4:].reshape(H // 2, W // 2)
    return y, u, v


def oracle_decode(W, H, version, data):
    """-> (packed I420 of the decoded picture, bytes consumed, quantiser, yuv_format); raises if the oracle throws"""
    from tests.oracle_binding import OracleDecoder
    o = OracleDecoder(W, H, version)
    o.Data, o.Offset = bytes(data), 0
    r = o.DecodeFrame()
    assert r is not None, f"the oracle threw {o.last_error} at offset {o.Offset}"
    S = o.Stride
    pic = _i420(r[0][:, :W], r[1][:, : W // 2], r[1][:, S // 2: S // 2 + W // 2])
    res = (pic, o.Offset, o.Quantizer, o.YuvFormat)
    o.close()
    return res


# ---------------------------------------------------------------------------------------------------------------- the stream, read back
class _Bits:
    """the stream's 16-bit little-endian words, most significant bit first"""

    def __init__(self, data):
        self.w = [int(x) for x in np.frombuffer(bytes(data), "<u2")] + [0, 0, 0]
        self.size = 16 * (len(self.w) - 3)
        self.pos = 0

    def peek(self, n):  # n <= 28; zeros behind the end
        i, off = self.pos >> 4, self.pos & 15
        return ((self.w[i] << 32 | self.w[i + 1] << 16 | self.w[i + 2]) >> (48 - off - n)) & ((1 << n) - 1)

    def take(self, n):
        assert self.pos + n <= self.size, "read past the stream"
        v = self.peek(n) if n else 0
        self.pos += n
        return v


def parse_stream(data, W, H):
    """-> dict(q, yuv_format, table, mbs (MB_DTYPE array; bits = what the macroblock took), forms (4,), end (bit position))"""
    T = tables.load()
    A, B, CBP = T["mobi_vx2table0_a"], T["mobi_vx2table0_b"], T["mobi_cbp_intra"]
    r = _Bits(data)
    assert r.take(1) == 1, "not an I-frame"
    out = {"yuv_format": r.take(1), "table": r.take(1), "q": r.take(6), "forms": np.zeros(4, np.int64)}
    assert out["table"] == 0
    mbs = np.zeros((W // 16) * (H // 16), MB_DTYPE)
    for m in mbs:
        start = r.pos
        assert r.take(1) == 0, "sub-block syntax"
        z = 0
        while r.take(1) == 0:
            z += 1
        m["cbp"] = CBP[(1 << z) - 1 + r.take(z)]
        for k in range(6):
            if k in (0, 4):
                m["luma_mode" if k == 0 else "chroma_mode"] = r.take(3)
            if not (int(m["cbp"]) >> k) & 1:
                continue
            assert r.take(1) == 1, "4x4 transforms"
            p = 0
            while True:
                form = 0
                if r.peek(7) == 3:
                    r.take(7)
                    if r.take(1) == 0:
                        form = 2
                    elif r.take(1) == 0:
                        form = 1
                    else:
                        form = 3
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
    out["mbs"], out["end"] = mbs, r.pos
    return out


# ---------------------------------------------------------------------------------------------------------------- the decisions, re-derived
def _lam(q):
    return LAM_BASE[(q - 12) % 3] << ((q - 12) // 3)


def _ue_bits(v):
    return 2 * (int(v + 1).bit_length() - 1) + 1


def _pred(mode, top, left, top_av, left_av):
    """(M, 8, 8) prediction of M blocks from their row above (M, 8) and column to the left (M, 8): vertical, horizontal, DC with positional
    availability (both: (sum + 8) / 16; one: (sum + 4) / 8; none: 128)"""
    M = top.shape[0]
    if mode == 0:
        return np.repeat(top[:, None, :], 8, axis=1)
    if mode == 1:
        return np.repeat(left[:, :, None], 8, axis=2)
    st, sl = top.sum(1), left.sum(1)
    dc = np.where(top_av & left_av, (st + sl + 8) // 16, np.where(top_av, (st + 4) // 8, np.where(left_av, (sl + 4) // 8, 128)))
    return np.broadcast_to(dc[:, None, None], (M, 8, 8)).copy()


def _code_blocks(ref, q, src, pred):
    """the block rule over (M, 8, 8) blocks at quantiser q -> dict(rec, lev, bits, sad, coded, clamp, range)"""
    M = src.shape[0]
    s = np.ascontiguousarray(src.reshape(M, 64), np.uint8)
    p = np.ascontiguousarray(pred.reshape(M, 64), np.uint8)
    lev, rec = np.empty((M, 64), np.int16), np.empty((M, 64), np.uint8)
    bits, sad, flags = np.empty(M, np.int32), np.empty(M, np.int32), np.empty(M, np.uint8)
    qa = np.array([q], np.int32)
    ref.ref_encode_batch(8, 1, qa.ctypes.data, M, s.ctypes.data, p.ctypes.data, VXREF.ctypes.data, lev.ctypes.data, rec.ctypes.data, bits.ctypes.data,
                         sad.ctypes.data, flags.ctypes.data)
    nz = (flags & 1) != 0
    clamp = nz & ((flags & 2) != 0)
    rng_ = nz & ~clamp & (np.abs(lev.astype(np.int32)).max(1) > 2047)
    coded = nz & ~clamp & ~rng_
    sad_pred = np.abs(s.astype(np.int32) - p.astype(np.int32)).sum(1)
    return {"rec": np.where(coded[:, None], rec, p).reshape(M, 8, 8).astype(np.int64), "lev": np.where(coded[:, None], lev, 0),
            "bits": np.where(coded, 1 + bits, 0).astype(np.int64), "sad": np.where(coded, sad, sad_pred).astype(np.int64),
            "coded": coded, "clamp": clamp, "range": rng_}


def rederive(ref, W, H, q, source, decoded):
    """Every macroblock of one picture, each against the DECODED picture's neighbours (so the macroblocks are independent and run as one
    numpy batch) -> dict(luma_mode, chroma_mode, cbp, bits (per macroblock, syntax included), lev (M, 6, 64), clamp, range (block counts))"""
    mbw, mbh = W // 16, H // 16
    M = mbw * mbh
    mbx, mby = np.tile(np.arange(mbw), mbh), np.repeat(np.arange(mbh), mbw)
    lam = _lam(q)
    sp, dp = planes(source.astype(np.int64), W, H), planes(decoded.astype(np.int64), W, H)
    res = {"cbp": np.zeros(M, np.int64), "bits": np.zeros(M, np.int64), "lev": np.zeros((M, 6, 64), np.int16), "clamp": 0, "range": 0}
    for chroma in (0, 1):
        n = 8 if chroma else 16
        pl = (1, 2) if chroma else (0,)

        def tiles(a):  # (M, n, n) macroblock tiles of a plane
            return a.reshape(mbh, n, mbw, n).transpose(0, 2, 1, 3).reshape(M, n, n)

        def border(a):  # the row above and the column to the left of every tile (zeros where there is none)
            pad = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
            pad[1:, 1:] = a
            top = np.stack([pad[y * n, 1 + x * n: 1 + x * n + n] for y, x in zip(mby, mbx)])
            left = np.stack([pad[1 + y * n: 1 + y * n + n, x * n] for y, x in zip(mby, mbx)])
            return top, left
        best_J = best = None
        keep = {}
        for mode in (0, 1, 3):
            allowed = (mby > 0) if mode == 0 else (mbx > 0) if mode == 1 else np.ones(M, bool)
            J = np.zeros(M, np.int64)
            blocks = []
            for p_i in pl:
                src_t, (top, left) = tiles(sp[p_i]), border(dp[p_i])
                trial = np.zeros((M, n, n), np.int64)
                for k in range(1 if chroma else 4):
                    by, bx = k >> 1, k & 1
                    t = top[:, 8 * bx: 8 * bx + 8] if by == 0 else trial[:, 7, 8 * bx: 8 * bx + 8]
                    l = left[:, 8 * by: 8 * by + 8] if bx == 0 else trial[:, 8 * by: 8 * by + 8, 7]
                    pred = _pred(mode, t, l, (mby > 0) | (by == 1), (mbx > 0) | (bx == 1))
                    b = _code_blocks(ref, q, src_t[:, 8 * by: 8 * by + 8, 8 * bx: 8 * bx + 8], pred)
                    trial[:, 8 * by: 8 * by + 8, 8 * bx: 8 * bx + 8] = b["rec"]
                    J += (b["sad"] << 8) + lam * b["bits"]
                    blocks.append(b)
            if best is None:
                best, best_J = np.full(M, -1), np.zeros(M, np.int64)
            take = allowed & ((best < 0) | (J < best_J))  # modes run upwards: a tie keeps the smaller one
            best, best_J = np.where(take, mode, best), np.where(take, J, best_J)
            keep[mode] = blocks
        res["chroma_mode" if chroma else "luma_mode"] = best
        for a in range(2 if chroma else 4):
            area = 4 + a if chroma else a
            for mode in (0, 1, 3):
                sel = best == mode
                b = keep[mode][a]
                res["cbp"] |= np.where(sel & b["coded"], 1 << area, 0)
                res["bits"] += np.where(sel, b["bits"], 0)
                res["lev"][sel, area] = b["lev"][sel]
                res["clamp"] += int((sel & b["clamp"]).sum())
                res["range"] += int((sel & b["range"]).sum())
    T = tables.load()
    inv = {int(c): i for i, c in reversed(list(enumerate(T["mobi_cbp_intra"])))}
    res["bits"] += np.array([1 + _ue_bits(inv[int(c)]) + 6 for c in res["cbp"]], np.int64)
    return res
