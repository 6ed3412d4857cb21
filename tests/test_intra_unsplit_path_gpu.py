"""mobi_recon_intra and its siblings ask one question per wave -- does any of the four macroblocks have a split area? -- and run a
six-step schedule and step loop without the 4x4 half where the answer is no (recon_intra_quad, `plain`).  The cases here are the places
where that second instance of the code can differ from the general one, and the waves in which the two meet.  Pictures are 64x48, four
by three macroblocks: macroblocks 5, 6, 9, 10 are interior by the kernel's own test, the others are at an edge.  Every case is 3 or 4
clips of 1 I-frame + 3 P-frames, bit-exact against OracleDecoder, under both kinds of frame step and through both launch orders:

  host     the host parser's launch list (LevelPlan, mobi_batch.h).  Batches this small are launched sparse: every macroblock has a wave of
           its own behind three padding rows, so a wave is unsplit exactly when its macroblock is.
  device   the device parser's lists (mobi_recon_intra_cl): a wave is list slot s of four clips -- that is where rows with and without
           split areas share a wave, and where a batch of three clips leaves a padding row in every wave.

  nosplit   no split area anywhere (every coded area an 8x8 transform): every predictor kind on unsplit areas, coded and uncoded -- the seven
            directional modes, DC with each availability combination, the 8x8 plane, the chroma planes' pre-pass in front of mode 9, a 16x16
            plane in front of mode 9
  onesplit  waves of four valid rows of which exactly one has a split area (the whole wave takes the general path), beside unsplit waves of four
  padding   three clips with lists of different lengths: unsplit waves with one, two and three valid rows
  wide      written-down frames: plane parameters beyond int16 on an unsplit 8x8 area, on both chroma pre-passes and on a 16x16 plane (sets the reference
            decodes: most parameters this large leave the clamp table's domain)
  wrap      256x48, Width == Stride: unsplit waves whose macroblocks ask every halo sample who owns it
  clamp     written-down: a coded unsplit 8x8 area whose DC prediction + residual is 319 (valid) or 320 (MOBI_E_CLAMP), as
            tests/test_residual_edges.py has it of the general path

The I-frame of every case is a chain of intra neighbours: its waves wait for tags and publish them.

CPU: every case holds what its name claims, read from the host parser's block records, descriptors and launch items -- in particular
which waves of either launch order are unsplit -- otherwise the GPU cases prove nothing about which path ran.
"""
import functools
import itertools

import numpy as np
import pytest

from mobiclipdecoder_amd.streamgen import BASE_SEED, default_params, generate_clip
from tests.oracle_binding import OracleDecoder
from tests.test_parse_fallback import _DC_MB, _frame, _part_code, _se_code, _ue_code
from tests.test_residual_edges import E_CLAMP, E_INDEX, HI, Q0, Script, _dc_level, kind_of_step  # noqa: F401  (kind_of_step: a fixture)

W, H, VER, N_FRAMES = 64, 48, 1, 4
MBW = W // 16
QUIET = dict(pm_skip=100, pm_split1=100, pm_deep=0, iframe_interval=0, edge_mode=0)


def _drawn(seed, n_clips, width=W, **kw):
    return [generate_clip(default_params("A", BASE_SEED + seed + 101 * c, width=width, height=H, version=VER, n_frames=N_FRAMES, **{**QUIET, **kw})) for c in range(n_clips)]


# ---------------------------------------------------------------------------------------------------------------- written-down frames
def _records(frames, f):
    """the host parser's view of frame f of a written-down clip: (rc, desc, payload)"""
    from tests.interp_binding import InterpDecoder
    d = InterpDecoder(W, H, VER)
    try:
        for k in range(f + 1):
            d.Data, d.Offset = frames[k], 0
            if d.DecodeFrame() is None:
                return d.last_error, None, None
        return 0, d.command_list()[0], d.payload()
    finally:
        d.close()


def _sub_mb(before, head, after, mb, modes, params, chroma):
    """An intra macroblock in DecIntraSubBlockPMode with nothing coded whose four 8x8 areas get `modes` (2: a plane with params[k]).  The
    predicted-mode code depends on the neighbours' modes: one bit where the mode is the predicted one, four bits otherwise, the mode's number
    counted without the predicted one.  The three readings of every area are tried until the host parser's records say `modes`.
    before / after: the frames in front and the bits around the macroblock; -> the macroblock's bits"""
    for pick in itertools.product(range(3), repeat=4):
        bits = _ue_code(0)
        for k, m in enumerate(modes):
            bits += ("1", "0" + format(m, "03b"), "0" + format(max(m - 1, 0), "03b"))[pick[k]]
            if m == 2:
                bits += _se_code(params[k])
        bits += chroma
        rc, desc, pay = _records(before + [_frame(head + bits + after)], len(before))
        if rc == 0 and (desc[mb, 1] & 1) and [int(pay[int(desc[mb, 0]) + 4 * a]) & 15 for a in range(4)] == list(modes):
            return bits
    raise AssertionError(("no reading gives", modes))


@functools.lru_cache(maxsize=None)
def _wide_clips():
    hdr = "1" + "0" + "0" + format(20, "06b")
    skip, n_mbs = _part_code(VER, 0, 0) + _ue_code(0), MBW * (H // 16)
    clips = []
    for c, (p8, pu, pv, p16) in enumerate(((40000, -40000, -40000, -70000), (-40000, -40000, -40000, -70000), (40000, 40000, 40000, -70000), (-32769, -32769, 5, 32768))):
        planes_uv = "010" + _se_code(pu) + _se_code(pv)
        full16 = _ue_code(0) + "010" + _se_code(p16) + "011"  # DecIntraFullBlockPMode: a 16x16 plane, chroma DC
        # the I-frame: macroblock 5 (interior) in sub-block mode with a wide 8x8 plane on area 0 and wide chroma planes, 7 a wide 16x16 plane
        # (its neighbours 2, 3 and 6 stay flat: a parameter this large on anything else leaves the clamp table's domain)
        a, b = 5, 7
        sub = _sub_mb([], hdr + _DC_MB * a + "1", _DC_MB * (n_mbs - a - 1), a, (2, 3, 3, 3), (p8, 0, 0, 0), planes_uv)
        frames = [_frame(hdr + _DC_MB * a + "1" + sub + _DC_MB * (b - a - 1) + "0" + full16 + _DC_MB * (n_mbs - b - 1))]
        # P-frames: everything copies the frame before but macroblocks 5 and 7, which are coded again as they were
        for f in range(1, N_FRAMES):
            head = "0" + _se_code(0) + skip * a + _part_code(VER, 0, 7)
            tail = skip * (b - a - 1) + _part_code(VER, 0, 6) + full16 + skip * (n_mbs - b - 1)
            sub = _sub_mb(frames, head, tail, a, (2, 3, 3, 3), (p8, 0, 0, 0), planes_uv)
            frames.append(_frame(head + sub + tail))
        fo = np.cumsum([0] + [len(x) for x in frames]).astype(np.uint32)
        clips.append((np.concatenate(frames), fo))
    return clips


def _clamp_clips():
    """macroblock 5 of frame 2 an intra one whose area 0 is a coded 8x8 block with a uniform residual of 74 on a DC prediction of
    total - 74: total = 319 stays inside the clamp table's domain, 320 leaves it"""
    clips = []
    for total in (HI, HI + 1, HI, HI + 1):
        s, mb, r = Script(W, H), 5, 74
        for m2, a2 in ((mb - MBW, 2), (mb - MBW, 3), (mb - 1, 1), (mb - 1, 3), (mb - MBW - 1, 3)):
            for sub in range(4):
                s.flat(m2, a2, sub, total - r)
        for sub in range(4):
            s.flat(mb, 0, sub, 77)
        s.block(2, mb, 0, 8, 0, [(0, _dc_level(8, Q0, r))], 1)
        clips.append(s.clip()[1])
    return clips


NOSPLIT = dict(pm_intra=650, t8_prob=1000, intra_sub_prob=500, plane_prob=700, cbp_prob=500)
CASES = {
    "nosplit": lambda: (W, _drawn(11, 4, **NOSPLIT)),
    "onesplit": lambda: (W, _drawn(21, 4, pm_intra=800, t8_prob=880, intra_sub_prob=500, plane_prob=500, cbp_prob=400)),
    "padding": lambda: (W, _drawn(31, 3, **{**NOSPLIT, "pm_intra": 350})),
    "wide": lambda: (W, _wide_clips()),
    "wrap": lambda: (256, _drawn(41, 3, 256, **{**NOSPLIT, "pm_intra": 500, "edge_mode": 1})),
    "clamp": lambda: (W, _clamp_clips()),
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
        if each is not None and dec.last_error in (0, E_CLAMP):  # (a clamp fault is found behind the parse: the command list is there)
            each(f, dec)
        if dec.last_error != 0:
            break
    return rows


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """-> per clip, per frame (rc, Offset, y, uv) up to the first frame the reference throws on: computed once, shared by the CPU and the GPU
    tests, never changed"""
    width, clips = case(name)
    out = []
    for data, fo in clips:
        o = OracleDecoder(width, H, VER)
        out.append(_decode_all(o, data, fo))
        o.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
TAP_MODES = (0, 1, 4, 5, 6, 7, 8)


def _area_kind(r, a, mb, S, mbw):
    """what recon_intra_quad's schedule makes of the first record of unsplit area a (its `build`, with its arithmetic) -> tuples"""
    mode, coded, pre, wide = r & 15, bool((r >> 4) & 1), bool((r >> 6) & 1), bool((r >> 7) & 1)
    out = []
    if pre:
        out.append(("pre-plane", "wide" if wide else "narrow"))
    if mode in TAP_MODES:
        out.append(("directional", mode, coded))
    elif mode == 3:
        mbx, mby = mb % mbw, mb // mbw
        off = mby * 16 * S + mbx * 16
        luma = a < 4
        boff = off + (a >> 1) * 8 * S + (a & 1) * 8 if luma else (off >> 1) + (a - 4) * (S >> 1)
        vfix = (not luma) and (boff & (S - 1)) >= (S >> 1)
        la, ta = ((boff - ((S >> 1) if vfix else 0)) & (S - 1)) != 0, boff >= S
        out.append(("dc", ta, la, coded))
    elif mode == 2:
        out.append(("plane8", coded, "wide" if wide else "narrow"))
    else:
        assert mode == 9, (mode, r)
        out.append(("mode9", coded, "behind a pre-pass" if pre else "bare"))
    return out


def _frame_lists(dec, width):
    """one frame of one clip -> [(mb, split areas, first records, w3 flags of the launch item)] in raster order"""
    desc, mbs, _, items = dec.command_list()
    pay = dec.payload()
    flags = {int(it[0]): int(it[3]) for it in items}
    out = []
    for mb in sorted(int(x) for x in mbs):
        recs = [int(pay[int(desc[mb, 0]) + 4 * a]) for a in range(6)]
        out.append((mb, sum((r >> 5) & 1 for r in recs), recs, flags[mb] | (int(desc[mb, 3]) & 0x11)))
    return out


@functools.lru_cache(maxsize=None)
def _seen(name):
    from tests.interp_binding import InterpDecoder
    width, clips = case(name)
    mbw = width // 16
    lists = []  # [clip][frame]
    seen = set()
    for (data, fo), want in zip(clips, _oracle(name)):
        S = want[0][3].shape[1]  # (a chroma row holds U and V: Stride samples)
        d = InterpDecoder(width, H, VER)
        per_frame = []
        got = _decode_all(d, data, fo, lambda f, dec: per_frame.append(_frame_lists(dec, width)))
        d.close()
        for f in range(len(want)):
            assert got[f][0] == (E_CLAMP if want[f][0] == E_INDEX else want[f][0]), (name, f, got[f][0], want[f][0])
            if want[f][0] == 0:
                assert got[f][1] == want[f][1] and np.array_equal(got[f][2], want[f][2]) and np.array_equal(got[f][3], want[f][3]), (name, f)
        seen.add(("stride", S))
        seen.add(("frames decoded", len(want)) if want[-1][0] == 0 else ("rejected in frame", len(want) - 1))
        lists.append((per_frame, S))
    for f in range(N_FRAMES):
        assert all(len(pf) > f or name == "clamp" for pf, _ in lists)
        rows_of = [pf[f] if len(pf) > f else [] for pf, _ in lists]
        kind = "I" if f == 0 else "P"
        # host order: a batch this small is launched sparse (LevelPlan: at most 4096 intra macroblocks), one macroblock per wave
        assert sum(len(x) for x in rows_of) <= 4096
        waves = [("host", [row]) for x in rows_of for row in x]
        # device order: slot s of the clips 4q .. 4q + 3 (mobi_recon_intra_cl)
        for q in range(0, len(lists), 4):
            quad = rows_of[q:q + 4]
            for s in range(max(len(x) for x in quad)):  # (s: a list slot)
                waves.append(("device", [x[s] for x in quad if s < len(x)]))
        for order, rows in waves:
            n_split = sum(splits > 0 for _, splits, _, _ in rows)
            seen.add((order, kind, "unsplit wave" if n_split == 0 else "general wave", len(rows), "rows"))
            if n_split:
                seen.add((order, kind, "split rows", n_split, "of", len(rows)))
                continue
            for mb, _, recs, flags in rows:
                mbx = mb % mbw
                interior = (mbx >= 1 and mbx + 1 < mbw and mb >= mbw) or width < lists[0][1]
                seen.add((kind, "unsplit:", "interior" if interior else "owner test"))
                seen.add((kind, "unsplit:", "waits" if flags & 2 else "does not wait"))
                seen.add((kind, "unsplit:", "publishes" if flags & 4 else "does not publish"))
                if flags & 1:
                    seen.add((kind, "unsplit:", "plane16", "wide" if flags & 0x10 else "narrow"))
                for a, r in enumerate(recs):
                    for k in _area_kind(r, a, mb, lists[0][1], mbw):
                        seen.add((kind, "unsplit:") + k)
    return seen


def _kinds(kind, coded_too=True):
    both = (False, True) if coded_too else (False,)
    return ({(kind, "unsplit:", "directional", m, c) for m in TAP_MODES for c in both} | {(kind, "unsplit:", "plane8", c, "narrow") for c in both} |
            {(kind, "unsplit:", "mode9", c, w) for c in both for w in ("bare", "behind a pre-pass")} | {(kind, "unsplit:", "pre-plane", "narrow"), (kind, "unsplit:", "plane16", "narrow")})


CLAIMS = {
    "nosplit": _kinds("P") | {("P", "unsplit:", "dc", ta, la, c) for ta in (False, True) for la in (False, True) for c in (False, True)}
               | {("I", "unsplit:", "waits"), ("I", "unsplit:", "publishes"), ("P", "unsplit:", "waits"), ("P", "unsplit:", "publishes"), ("P", "unsplit:", "does not wait"),
                  ("device", "P", "unsplit wave", 4, "rows"), ("device", "I", "unsplit wave", 4, "rows"), ("host", "P", "unsplit wave", 1, "rows")},
    "onesplit": {("device", "P", "split rows", 1, "of", 4), ("device", "I", "split rows", 1, "of", 4), ("device", "P", "unsplit wave", 4, "rows"),
                 ("host", "P", "general wave", 1, "rows"), ("host", "P", "unsplit wave", 1, "rows")},
    "padding": {("device", "P", "unsplit wave", n, "rows") for n in (1, 2, 3)} | {("device", "I", "unsplit wave", 3, "rows")},
    "wide": {(k, "unsplit:", "plane8", False, "wide") for k in "IP"} | {(k, "unsplit:", "pre-plane", "wide") for k in "IP"} | {(k, "unsplit:", "plane16", "wide") for k in "IP"}
            | {("device", "P", "unsplit wave", 4, "rows"), ("P", "unsplit:", "interior")},
    "wrap": {("stride", 256), ("P", "unsplit:", "owner test"), ("P", "unsplit:", "interior"), ("I", "unsplit:", "owner test"), ("device", "P", "unsplit wave", 3, "rows")}
            | {("P", "unsplit:", "directional", m, c) for m in TAP_MODES for c in (False, True)},
    "clamp": {("rejected in frame", 2), ("frames decoded", N_FRAMES), ("P", "unsplit:", "dc", True, True, True), ("device", "P", "unsplit wave", 4, "rows")},
}
NO_SPLIT_AT_ALL = ("nosplit", "padding", "wide", "wrap", "clamp")


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_hold_what_they_claim(name):
    """the oracle and the host parser with the kernels' arithmetic on the CPU decode every frame alike, and records, descriptors and launch
    items hold what the case is there for: which waves are unsplit, and what their areas are"""
    seen = _seen(name)
    missing = CLAIMS[name] - seen
    assert not missing, (name, sorted(missing, key=str))
    general = {s for s in seen if "general wave" in s}
    if name in NO_SPLIT_AT_ALL:
        assert not general, (name, general)
    if name != "wrap":
        assert ("stride", 256) in seen and not {s for s in seen if "owner test" in s}, name  # 64 wide in a stride of 256: nothing wraps


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("order", ["host", "device"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_unsplit_path_cases(name, order, kind_of_step):
    """the clips of a case as ONE batch, frame by frame: rc, Offset and every byte of both planes of every clip as the oracle's; a clip the
    reference throws on answers MOBI_E_CLAMP in that frame (and is not looked at afterwards), its neighbours are bit-exact"""
    from mobiclipdecoder_amd import MobiclipBatch
    width, clips = case(name)
    want = _oracle(name)
    b = MobiclipBatch(len(clips), width, H, VER, device_parse=(order == "device"))
    try:
        for f in range(N_FRAMES):
            live = [k for k in range(len(clips)) if len(want[k]) > f]
            rcs, offs = b.decode([d[fo[f]:fo[f + 1]] if k in live else d[fo[0]:fo[1]] for k, (d, fo) in enumerate(clips)], [0] * len(clips))
            for k in live:
                fo = clips[k][1]
                if want[k][f][0] != 0:
                    assert want[k][f][0] == E_INDEX and rcs[k] == E_CLAMP, (name, order, kind_of_step, k, f, rcs[k])
                    continue
                assert rcs[k] == 0 and offs[k] == want[k][f][1] - int(fo[f]), (name, order, kind_of_step, k, f, rcs[k], offs[k])
                y, uv = b.planes(k)
                assert np.array_equal(y, want[k][f][2]), (name, order, kind_of_step, k, f, "luma differs from the oracle", np.argwhere(y != want[k][f][2])[:4].tolist())
                assert np.array_equal(uv, want[k][f][3]), (name, order, kind_of_step, k, f, "chroma differs from the oracle", np.argwhere(uv != want[k][f][3])[:4].tolist())
    finally:
        b.close()
