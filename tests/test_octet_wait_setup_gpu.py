"""mobi_recon_inter8 / mobi_recon_step prepare stage B's window addresses, byte selectors and masks, stage C's slot records and the bases
of the output rows while the octet's windows are in flight (recon_inter_oct, "set-up of stages B, C and D").  A value prepared early can
be the wrong one wherever it depends on the lane's leaf, has to cross the deep trees' fetch, or describes the octet's coded areas; the
cases here are those places.  Pictures are 144x48: 9 macroblocks wide, so every macroblock row has a full octet and an octet of one.
Every case is 3 clips of 1 I-frame + 4 P-frames from the project's generator, bit-exact against OracleDecoder, under both kinds of
frame step.

  whole     only whole 16x16 leaves, wide vectors, several references
  tb / lr   only TOP/BOTTOM pairs, only LEFT/RIGHT pairs (written-down motion rows): every leaf a vector, a phase and a reference of its own
  mixed     whole leaves and both pairs inside one octet, pm_multiref high: leaf B from another ring slot than leaf A
  deep      octets with one, two and three deeper trees beside whole leaves: the prepared values cross deep_fetch / deep_finish
  wrap      256x48, Width == Stride: right-most macroblocks whose windows run over the row's end (slow path) beside fast ones and deep trees
  intra     octets with intra macroblocks mixed in, all-intra octets (the early return), the one-macroblock last octet both ways
  coded     odd and even numbers of 8x8 areas, 4x4 and 8x8 areas in one octet, more than 16 slots
  uncoded   no coded area at all

CPU: every case holds the classes its name claims, read from the host parser's descriptors (MbDesc w1..w6) with the kernel's own
arithmetic -- otherwise the GPU case proves nothing.
"""
import functools

import numpy as np
import pytest

from mobiclipdecoder_amd.streamgen import BASE_SEED, default_params, generate_clip, generate_scripted
from tests.oracle_binding import OracleDecoder
from tests.test_residual_edges import kind_of_step  # noqa: F401  (a fixture)

W, H, N_CLIPS, N_FRAMES = 144, 48, 3, 5
QUIET = dict(pm_skip=0, pm_split1=0, pm_deep=0, pm_intra=0, edge_mode=0, iframe_interval=0)


def _params(seed, width=W, **kw):
    return default_params("A", BASE_SEED + seed, width=width, height=H, version=1, n_frames=N_FRAMES, **{**QUIET, **kw})


def _drawn(seed, width=W, **kw):
    return [generate_clip(_params(seed + 101 * c, width, **kw)) for c in range(N_CLIPS)]


def _pairs(shape, seed):
    """every macroblock of every P-frame a TOP/BOTTOM (shape 1) or LEFT/RIGHT (shape 2) pair; each leaf's window at a place of its own
    inside the picture, its CopyBlock phase and (from the second P-frame on) its reference drawn independently of the other leaf's"""
    clips = []
    for c in range(N_CLIPS):
        rng = np.random.RandomState(seed + c)
        motion = []
        for f in range(1, N_FRAMES):
            for mb in range((W // 16) * (H // 16)):
                x0, y0 = 16 * (mb % (W // 16)), 16 * (mb // (W // 16))
                boxes = [(x0, y0, 16, 8), (x0, y0 + 8, 16, 8)] if shape == 1 else [(x0, y0, 8, 16), (x0 + 8, y0, 8, 16)]
                ref, dx, dy = [0] * 4, [0] * 4, [0] * 4
                for k, (lx, ly, w, h) in enumerate(boxes):
                    sx = rng.randint(max(0, lx - 20), min(W - w - 1, lx + 20) + 1)
                    sy = rng.randint(max(0, ly - 20), min(H - h - 1, ly + 20) + 1)
                    ph = rng.randint(4)
                    dx[k], dy[k] = 2 * (sx - lx) + (ph & 1), 2 * (sy - ly) + (ph >> 1)
                    ref[k] = 1 + rng.randint(min(f, 5))
                if f >= 2 and ref[0] == ref[1] and mb & 1:
                    ref[1] = ref[0] % min(f, 5) + 1
                motion.append([f, mb, shape] + ref + dx + dy)
        clips.append(generate_scripted(_params(seed), [], [], None, motion))
    return clips


CASES = {
    "whole": lambda: (W, _drawn(11, mv_range=40, pm_multiref=500)),
    "tb": lambda: (W, _pairs(1, 21)),
    "lr": lambda: (W, _pairs(2, 31)),
    "mixed": lambda: (W, _drawn(41, pm_split1=600, mv_range=40, pm_multiref=800)),
    "deep": lambda: (W, _drawn(51, pm_deep=300, pm_split1=200, mv_range=24, pm_multiref=500)),
    "wrap": lambda: (256, _drawn(61, 256, pm_deep=150, pm_split1=300, mv_range=40, edge_mode=1)),
    "intra": lambda: (W, _drawn(71, pm_intra=800, pm_split1=100, mv_range=24)),
    "coded": lambda: (W, _drawn(81, pm_split1=300, cbp_prob=550, t8_prob=500, mv_range=16)),
    "uncoded": lambda: (W, _drawn(91, pm_split1=400, pm_deep=100, cbp_prob=0, mv_range=24)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (width, [(data, frame_off)] per clip): built once"""
    return CASES[name]()


def _decode_all(dec, data, fo, each=None):
    rows = []
    for f in range(N_FRAMES):
        dec.Data, dec.Offset = data[: fo[f + 1]], int(fo[f])
        r = dec.DecodeFrame()
        rows.append((dec.last_error, dec.Offset, None if r is None else r[0].copy(), None if r is None else r[1].copy()))
        if each is not None:
            each(f, dec)
    return rows


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """-> per clip, per frame (rc, Offset, y, uv): computed once, shared by the CPU and the GPU tests, never changed"""
    width, clips = case(name)
    out = []
    for data, fo in clips:
        o = OracleDecoder(width, H, 1)
        out.append(_decode_all(o, data, fo))
        o.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def _classes(desc, S, width, seen):
    """what one P-frame's descriptors hold, with recon_inter_oct's arithmetic (stage A and the set-up behind it) -> into `seen`"""
    lgS, mbw = S.bit_length() - 1, width // 16
    w1, w2 = desc[:, 1].astype(np.int64), desc[:, 2].astype(np.int64)
    pos = desc[:, 3:7].astype(np.uint32).view(np.int32).astype(np.int64)  # posA, cposA, posB, cposB
    for row in range(H // 16):
        for o0 in range(0, mbw, 8):
            mbs = list(range(row * mbw + o0, row * mbw + min(o0 + 8, mbw)))
            kinds, n_deep, n8, n4, wraps = [], 0, 0, 0, 0
            for m in mbs:
                if w1[m] & 1:
                    kinds.append("intra")
                    continue
                nl, dual = (w1[m] >> 1) & 0x7F, (w1[m] >> 26) & 3
                if nl > 1 and dual == 0:
                    kinds.append("deep")
                    n_deep += 1
                else:
                    kinds.append(("whole", "tb", "lr")[dual])
                    leaves = [(pos[m, 0], pos[m, 1], (w2[m] >> 10) & 7, (w2[m] >> 16) & 3, (w2[m] >> 18) & 3)]
                    if dual:
                        top, ctop = (pos[m, 2] + (8 << lgS), pos[m, 3] + (4 << lgS)) if dual == 1 else (pos[m, 2] + 8, pos[m, 3] + 4)
                        leaves.append((top, ctop, (w2[m] >> 13) & 7, (w2[m] >> 20) & 3, (w2[m] >> 22) & 3))
                        seen.add(("refs differ", bool(leaves[0][2] != leaves[1][2])))
                        seen.add(("vectors differ", bool(pos[m, 0] != pos[m, 2])))
                    wpx, cwpx = (8, 4) if dual == 2 else (16, 8)
                    over = max(max((t & (S - 1)) + wpx + (ph & 1) - S, (ct & (S - 1)) + cwpx + (cph & 1) - (S >> 1)) for t, ct, _, ph, cph in leaves)
                    wraps += over > 0
                    seen.add(("wrap", kinds[-1], bool(over > 0)))
                    for k, (t, ct, _, ph, cph) in enumerate(leaves):
                        seen.update([("luma phase", int(ph)), ("chroma phase", int(cph)), ("xo", int(t & 7)), ("cxo", int(ct & 7)), ("parity", int((t >> lgS) & 1)),
                                     ("leaf", kinds[-1], k, "xo", int(t & 7)), ("leaf", kinds[-1], k, "parity", int((t >> lgS) & 1))])
                for a in range(6):
                    if (w1[m] >> (8 + a)) & 1:
                        n8 += (w1[m] >> (14 + a)) & 1
                        n4 += 1 - ((w1[m] >> (14 + a)) & 1)
            n_inter = sum(k != "intra" for k in kinds)
            n_slots = ((n8 + 1) & ~1) + n4
            seen.add(("octet of", len(mbs), "all intra" if not n_inter else "mixed" if n_inter < len(mbs) else "all inter"))
            seen.add(("octet kinds", frozenset(kinds)))
            if n_deep and n_inter > n_deep:
                seen.add(("deep beside leaves", min(n_deep, 3)))
            if wraps and n_inter > wraps:
                seen.add(("wrap beside fast",))
            if n_inter:
                seen.add(("coded", "none" if n8 + n4 == 0 else "n8 odd" if n8 & 1 else "n8 even"))
                seen.add(("slots", "over 16" if n_slots > 16 else "up to 16"))
                if n8 and n4:
                    seen.add(("coded", "both kinds"))


@functools.lru_cache(maxsize=None)
def _seen(name):
    from tests.interp_binding import InterpDecoder
    width, clips = case(name)
    seen = set()
    for (data, fo), want in zip(clips, _oracle(name)):
        S = want[0][3].shape[1]  # (a chroma row holds U and V: Stride samples)
        d = InterpDecoder(width, H, 1)
        got = _decode_all(d, data, fo, lambda f, dec: f and _classes(dec.command_list()[0], S, width, seen))
        d.close()
        for f in range(N_FRAMES):
            assert want[f][0] == 0 and got[f][0] == 0 and got[f][1] == want[f][1], (name, f, want[f][0], got[f][:2])
            assert np.array_equal(got[f][2], want[f][2]) and np.array_equal(got[f][3], want[f][3]), (name, f)
        assert not np.array_equal(want[1][2], want[N_FRAMES - 1][2]), name
        seen.add(("stride", S))
    return seen


ALL_PHASES = {("luma phase", p) for p in range(4)} | {("chroma phase", p) for p in range(4)}
ALL_SHIFTS = {("xo", x) for x in range(8)} | {("parity", p) for p in range(2)}
CLAIMS = {
    "whole": ALL_PHASES | ALL_SHIFTS | {("cxo", x) for x in range(8)},
    "tb": ALL_PHASES | ALL_SHIFTS | {("leaf", "tb", k, "xo", x) for k in range(2) for x in range(8)} | {("leaf", "tb", k, "parity", p) for k in range(2) for p in range(2)}
          | {("refs differ", True), ("refs differ", False), ("vectors differ", True)},
    "lr": ALL_PHASES | ALL_SHIFTS | {("leaf", "lr", k, "xo", x) for k in range(2) for x in range(8)} | {("leaf", "lr", k, "parity", p) for k in range(2) for p in range(2)}
          | {("refs differ", True), ("refs differ", False), ("vectors differ", True)},
    "mixed": ALL_PHASES | ALL_SHIFTS | {("refs differ", True), ("octet kinds", frozenset(["whole", "tb", "lr"]))},
    "deep": {("deep beside leaves", n) for n in (1, 2, 3)} | {("octet of", 1, "all inter")},
    "wrap": {("stride", 256), ("wrap beside fast",), ("deep beside leaves", 1)} | {("wrap", k, True) for k in ("whole", "tb", "lr")},
    "intra": {("octet of", 8, "mixed"), ("octet of", 8, "all intra"), ("octet of", 1, "all intra"), ("octet of", 1, "all inter")},
    "coded": {("coded", "n8 odd"), ("coded", "n8 even"), ("coded", "both kinds"), ("slots", "over 16"), ("slots", "up to 16")},
    "uncoded": {("coded", "none")},
}
ONLY = {"whole": {"whole"}, "tb": {"tb"}, "lr": {"lr"}}  # cases that hold nothing but one kind of macroblock


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_hold_the_classes_they_claim(name):
    """the oracle and the host parser with the kernels' arithmetic on the CPU decode every frame alike, and the descriptors hold what the
    case is there for"""
    seen = _seen(name)
    missing = CLAIMS[name] - seen
    assert not missing, (name, sorted(missing, key=str))
    kinds = set().union(*[c[1] for c in seen if c[0] == "octet kinds"])
    if name in ONLY:
        assert kinds == ONLY[name], (name, kinds)
    if name == "uncoded":
        assert not {c for c in seen if c[0] == "coded"} - {("coded", "none")}
    if name != "wrap":
        assert ("stride", 256) in seen  # 144 wide in a stride of 256: nothing wraps
        assert not {c for c in seen if c[0] == "wrap" and c[2]}, name


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_wait_setup_cases(name, kind_of_step):
    """the clips of a case as ONE batch, frame by frame: rc, Offset and every byte of both planes of every clip as the oracle's"""
    from mobiclipdecoder_amd import MobiclipBatch
    width, clips = case(name)
    want = _oracle(name)
    b = MobiclipBatch(len(clips), width, H, 1)
    try:
        for f in range(N_FRAMES):
            rcs, offs = b.decode([d[fo[f]:fo[f + 1]] for d, fo in clips], [0] * len(clips))
            for k, (_, fo) in enumerate(clips):
                assert rcs[k] == 0 and offs[k] == want[k][f][1] - int(fo[f]), (name, kind_of_step, k, f, rcs[k], offs[k])
                y, uv = b.planes(k)
                assert np.array_equal(y, want[k][f][2]), (name, kind_of_step, k, f, "luma differs from the oracle", np.argwhere(y != want[k][f][2])[:4].tolist())
                assert np.array_equal(uv, want[k][f][3]), (name, kind_of_step, k, f, "chroma differs from the oracle", np.argwhere(uv != want[k][f][3])[:4].tolist())
    finally:
        b.close()
