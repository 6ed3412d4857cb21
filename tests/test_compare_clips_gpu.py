"""The checker, checked: mobi_batch_compare_clips / mobi_compare_clips (csrc/mobi_analysis.hip) is what certifies all but a handful of the
benchmark's clips ("the copies against their source on the device"), so it has to be seen reporting differences -- every single byte of a
slot, in exactly the clip that holds it, counted in 16-byte words of the private tiled layout.

Each case decodes identical streams into all clips (the comparison reports nothing), overwrites ring slots of chosen clips through the
profiling twin's mobi_debug_write_planes with the clip's own planes plus chosen edits, and computes the expected count here: both clips'
slots are laid out with the luma and chroma tile formulas as tests/test_tile_layout.py writes them out (chroma behind Stride * Height), and
the 16-byte words that differ are counted.  n_diff_out[clip] and the return value (clips with a non-zero count) must be exactly that.

Geometries: the smallest that reach each path of the kernel's walk (one workgroup per 16 KB chunk, 4 iterations x 256 lanes x 16 bytes):
64x16 (6144 B: one chunk that ends inside its second iteration), 64x48 (18432 B: two chunks, the second with 128 live lanes), 512x32
(24576 B: one and a half chunks, Width == Stride), 256x192 (73728 B: four and a half chunks)."""
import ctypes as C
import functools

import numpy as np
import pytest

from mobiclipdecoder_amd import default_params, generate_clip
from mobiclipdecoder_amd.streamgen import BASE_SEED
from tests.oracle_binding import OracleDecoder

GEOMS = [(64, 16), (64, 48), (512, 32), (256, 192)]
MOBI_E_NULLREF, MOBI_E_ARG = -2, -7
UNTOUCHED = 0xDEADBEEF


# ---- the tiled slot, in numpy (mobi_tile.h; the formulas of tests/test_tile_layout.py) ----
@functools.lru_cache(maxsize=None)
def tile_maps(S, H):
    """(ty, tc): tiled offset inside the slot of every byte of the Y plane (Stride * Height) and of the UV plane (Stride * Height / 2)"""
    lg = S.bit_length() - 1
    ysz = S * H
    a = np.arange(ysz, dtype=np.int64)
    row, col = a >> lg, a & (S - 1)
    ty = (((row >> 4) * (S >> 4) + (col >> 4)) << 8) + (((row >> 3) & 1) << 7) + (((col >> 3) & 1) << 6) + ((row & 7) << 3) + (col & 7)
    c = np.arange(ysz // 2, dtype=np.int64)
    crow, ccol = c >> lg, c & (S - 1)
    v, x = ccol >> (lg - 1), ccol & (S // 2 - 1)
    tc = (((crow >> 3) * (S >> 4) + (x >> 3)) << 7) + ((crow & 7) << 4) + (v << 3) + (x & 7)
    return ty, ysz + tc


def tiled(y, uv):
    """the slot as the device holds it"""
    H, S = y.shape
    ty, tc = tile_maps(S, H)
    t = np.zeros(S * H * 3 // 2, np.uint8)
    t[ty] = y.ravel()
    t[tc] = uv.ravel()
    return t


def words_differing(a, b):
    """16-byte words of the tiled slot in which planes a = (y, uv) and b differ"""
    return int((tiled(*a).reshape(-1, 16) != tiled(*b).reshape(-1, 16)).any(1).sum())


def edit_at(planes, offsets, xor):
    """a copy of planes = (y, uv) with the bytes at these tiled offsets of the slot xor-ed"""
    y, uv = planes[0].copy(), planes[1].copy()
    H, S = y.shape
    ty, tc = tile_maps(S, H)
    inv = np.empty(S * H * 3 // 2, np.int64)
    inv[ty] = np.arange(S * H)
    inv[tc] = S * H + np.arange(S * H // 2)
    for o in offsets:
        k = int(inv[o])
        if k < S * H:
            y.reshape(-1)[k] ^= xor
        else:
            uv.reshape(-1)[k - S * H] ^= xor
    return y, uv


# ---- batches ----
def _stream(W, H, seed, n_frames):
    p = default_params("A", BASE_SEED + seed, n_frames=n_frames, width=W, height=H, pm_intra=150)
    data, fo = generate_clip(p)
    return p, [data[fo[f]:fo[f + 1]] for f in range(n_frames)]


class Rig:
    """n clips of one geometry on the profiling twin, all decoding the stream of seeds[clip]"""

    def __init__(self, lib, n, W, H, n_frames=1, seeds=None):
        from mobiclipdecoder_amd import MobiclipBatch
        self.lib, self.n = lib, n
        lib.mobi_debug_write_planes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        seeds = [5100] * n if seeds is None else seeds
        streams = {s: _stream(W, H, s, max(n_frames, 1)) for s in set(seeds)}
        self.b = MobiclipBatch(n, W, H, streams[seeds[0]][0].version)
        self.slot_bytes = self.b.Stride * H * 3 // 2
        for f in range(n_frames):
            rcs, _ = self.b.decode([streams[s][1][f] for s in seeds], [0] * n)
            assert rcs == [0] * n

    def compare(self, modulus):
        """-> (return value, n_diff_out as the call left it)"""
        out = np.full(self.n, UNTOUCHED, np.uint32)
        rc = self.lib.mobi_batch_compare_clips(self.b._h, int(modulus), out.ctypes.data)
        return rc, out

    def expect(self, modulus, counts):
        """the comparison reports exactly these counts {clip: words} and nothing else"""
        want = np.zeros(self.n, np.uint32)
        for c, k in counts.items():
            want[c] = k
        rc, got = self.compare(modulus)
        assert np.array_equal(got, want) and rc == int((want != 0).sum()), (modulus, rc, got.tolist(), want.tolist())

    def planes(self, clip, idx=0):
        y, uv = self.b.planes(clip, idx)
        return y.copy(), uv.copy()

    def write(self, clip, planes, ring_idx=0):
        y, uv = (np.ascontiguousarray(a, np.uint8) for a in planes)
        assert self.lib.mobi_debug_write_planes(self.b._h, clip, ring_idx, y.ctypes.data, uv.ctypes.data) == 0

    def close(self):
        self.b.close()


def probe_offsets(slot_bytes):
    """Tiled offsets of the bytes flipped one at a time: the ends of Y and of the slot, the first chroma byte, one byte in every 16 KB
    chunk, one in each of the four iterations of every chunk (as far as the slot reaches), in varying lanes and bytes of the word."""
    ysz = slot_bytes * 2 // 3
    offs = {0: "first byte of Y", ysz - 1: "last byte of Y", ysz: "first chroma byte", slot_bytes - 1: "last byte of the slot"}
    chunks = (slot_bytes + 16383) // 16384
    for c in range(chunks):
        live = min(16384, slot_bytes - c * 16384)
        offs.setdefault(c * 16384 + (4099 * c + 1225) % live, f"chunk {c}")
        for k in range(4):
            o = c * 16384 + k * 4096 + 16 * ((67 * k + 29 * c + 3) % 256) + (7 * k + 3 * c + 5) % 16
            if o < slot_bytes:
                offs.setdefault(o, f"chunk {c}, iteration {k}")
        if live < 16384:  # the last live word of a partial chunk and its last byte are in `offs` already (the end of the slot); its first too
            offs.setdefault(c * 16384, f"first byte of the partial chunk {c}")
    return offs


def test_probe_offsets_reach_every_chunk_and_iteration():
    """(no device needed: what the single-byte cases below claim to cover)"""
    for W, H in GEOMS:
        S = 256 if W <= 256 else 512
        slot = S * H * 3 // 2
        offs = np.array(sorted(probe_offsets(slot)))
        assert offs.max() == slot - 1 and offs.min() == 0
        chunk, k = offs // 16384, (offs % 16384) // 4096
        live = {(c, i) for c in range((slot + 16383) // 16384) for i in range(4) if c * 16384 + i * 4096 < slot}
        assert set(zip(chunk.tolist(), k.tolist())) == live
        assert {0, 1, 2, 3} <= set(((offs % 16) // 4).tolist())  # every dword of the 16-byte word
    ty, tc = tile_maps(256, 16)
    assert np.array_equal(np.sort(np.concatenate([ty, tc])), np.arange(256 * 16 * 3 // 2))


# ---- one byte at a time ----
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", GEOMS)
def test_every_single_byte_is_one_word_in_its_clip(W, H, profiling_library):
    r = Rig(profiling_library, 4, W, H)
    assert r.slot_bytes == {(64, 16): 6144, (64, 48): 18432, (512, 32): 24576, (256, 192): 73728}[(W, H)]
    r.expect(2, {})
    own = r.planes(3)
    assert np.array_equal(own[0], r.planes(1)[0]) and own[0].any()
    for o, what in probe_offsets(r.slot_bytes).items():
        for xor in (1, 0x80):
            ed = edit_at(own, [o], xor)
            assert words_differing(ed, own) == 1
            r.write(3, ed)
            rc, got = r.compare(2)
            assert rc == 1 and got.tolist() == [0, 0, 0, 1], (what, o, xor, rc, got.tolist())
            r.write(3, own)  # (padding bytes among them: the slot is as it was before anything else happens)
    r.expect(2, {})
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(64, 16), (64, 48)])
def test_padding_is_compared(W, H, profiling_library):
    """"padding included": a kernel that writes outside the picture is a real fault, and the checker reports it"""
    r = Rig(profiling_library, 4, W, H)
    own = r.planes(2)
    S = r.b.Stride
    assert not own[0][:, W:].any() and not own[1][:, W // 2:S // 2].any() and not own[1][:, S // 2 + W // 2:].any()
    for plane, row, col in ((0, 0, W), (0, H - 1, S - 1), (0, H // 2, W + 77), (1, 0, W // 2), (1, H // 2 - 1, S // 2 - 1), (1, 3, S // 2 + W // 2),
                            (1, H // 2 - 1, S - 1)):
        ed = (own[0].copy(), own[1].copy())
        ed[plane][row, col] = 1
        assert words_differing(ed, own) == 1
        r.write(2, ed)
        r.expect(2, {2: 1})
        r.write(2, own)
    r.expect(2, {})
    r.close()  # non-zero padding has been in the ring: nothing is decoded with this batch any more


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(64, 48), (256, 192)])
def test_the_count_is_words_not_bytes(W, H, profiling_library):
    r = Rig(profiling_library, 4, W, H)
    own = r.planes(3)
    base = 16384 + 16 * 40  # in the second chunk
    for offsets, words in (([base, base + 3, base + 15], 1), ([base + 15, base + 16], 2), ([base, base + 16, base + 32, base + 47], 3),
                           ([base - 16 * 41, base - 16 * 41 + 16], 2),  # the last word of chunk 0 and the first of chunk 1
                           ([4095, 4096, 8191, 8192, 12287, 12288], 6),  # either side of every iteration's boundary
                           (list(range(r.slot_bytes - 48, r.slot_bytes)), 3)):
        ed = edit_at(own, offsets, 0xFF)
        assert words_differing(ed, own) == words
        r.write(3, ed)
        r.expect(2, {3: words})
    inv = (own[0] ^ 0xFF, own[1] ^ 0xFF)  # every byte of the slot
    r.write(3, inv)
    r.expect(2, {3: r.slot_bytes // 16})
    r.write(1, inv)  # ... and now its source too: equal again
    r.expect(2, {})
    r.write(0, inv)
    r.expect(2, {2: r.slot_bytes // 16})
    r.close()


# ---- which clip is compared with which ----
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(64, 16), (512, 32)])
def test_modulus_semantics(W, H, profiling_library):
    n = 7
    r = Rig(profiling_library, n, W, H)
    own = r.planes(0)
    rng = np.random.default_rng(W)

    def edited(k):
        """k words of the slot changed"""
        words = rng.choice(r.slot_bytes // 16, k, replace=False)
        ed = edit_at(own, [int(w) * 16 + int(rng.integers(0, 16)) for w in words], int(rng.integers(1, 256)))
        assert words_differing(ed, own) == k
        return ed

    r.expect(3, {})
    r.write(5, edited(2))  # a copy: seen on that clip alone
    r.expect(3, {5: 2})
    r.write(5, own)
    r.write(1, edited(3))  # a source: seen on its copies (clip 4; there is no clip 7), never on itself
    r.expect(3, {4: 3})
    r.write(4, r.planes(1))  # the copy follows its source
    r.expect(3, {})
    # sources that differ from one another are nobody's business
    e0, e2 = edited(4), edited(5)
    for c in (0, 3, 6):
        r.write(c, e0)
    for c in (2, 5):
        r.write(c, e2)
    r.expect(3, {})
    r.expect(1, {1: words_differing(r.planes(1), e0), 2: words_differing(e2, e0), 4: words_differing(r.planes(4), e0), 5: words_differing(e2, e0)})
    # modulus = n: every clip is its own source, whatever the contents
    for c in range(n):
        r.write(c, (rng.integers(0, 256, own[0].shape, dtype=np.uint8), rng.integers(0, 256, own[1].shape, dtype=np.uint8)))
    r.expect(n, {})
    # modulus 1: all clips against clip 0
    for c in range(n):
        r.write(c, own)
    r.expect(1, {})
    r.write(2, edited(1))
    r.write(5, edited(7))
    r.expect(1, {2: 1, 5: 7})
    r.expect(2, {2: 1, 5: 7})  # (clip 2 against 0, clip 5 against 1)
    r.expect(6, {})            # (only clip 6 has a source other than itself: clip 0)
    r.write(0, edited(6))
    rc, got = r.compare(1)
    assert rc == n - 1 and got[0] == 0 and (got[1:] > 0).all() and got[1] == got[3] == got[4] == got[6] == 6, (rc, got.tolist())
    r.close()


# ---- which frame is compared ----
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(64, 16), (64, 48)])
@pytest.mark.parametrize("n_frames", [1, 6, 7])
def test_only_the_newest_frame(W, H, n_frames, profiling_library):
    """after 1, 6 and 7 frames the newest picture lies in slot 1, 0 (the ring has wrapped) and 1 again"""
    r = Rig(profiling_library, 3, W, H, n_frames=n_frames)
    r.expect(1, {})
    for idx in range(1, min(n_frames, 6)):  # older pictures: not the checker's business
        old = r.planes(2, idx)
        r.write(2, (old[0] ^ 0xFF, old[1] ^ 0xFF), ring_idx=idx)
        r.expect(1, {})
    own = r.planes(2)
    ed = edit_at(own, [0, 16, r.slot_bytes - 1], 0x40)
    r.write(2, ed)
    r.expect(1, {2: 3})
    assert np.array_equal(r.planes(2)[0], ed[0]) and np.array_equal(r.planes(2)[1], ed[1])
    r.close()


# ---- no injection: a clip that really decoded something else ----
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(64, 48), (256, 192)])
def test_a_different_stream_is_reported_with_the_oracles_count(W, H, profiling_library):
    n_frames, seeds = 3, [5100, 5101, 5100, 5102]  # clip 3 is handed another stream than clip 3 % 2 = 1
    r = Rig(profiling_library, 4, W, H, n_frames=n_frames, seeds=seeds)
    oras = {}
    for s in (5101, 5102):
        p, frames = _stream(W, H, s, n_frames)
        o = OracleDecoder(W, H, p.version)
        for fr in frames:
            o.Data, o.Offset = fr, 0
            assert o.DecodeFrame() is not None
        oras[s] = (o.y(0), o.uv(0))
        o.close()
    want = words_differing(oras[5102], oras[5101])
    assert 0 < want <= r.slot_bytes // 16
    assert np.array_equal(r.planes(3)[0], oras[5102][0]) and np.array_equal(r.planes(1)[1], oras[5101][1])
    r.expect(2, {3: want})
    r.close()


# ---- refusals ----
@pytest.mark.gpu
def test_refusals_write_nothing(profiling_library):
    n = 3
    r = Rig(profiling_library, n, 64, 16, n_frames=0)
    for modulus, rc_want in ((1, MOBI_E_NULLREF), (n, MOBI_E_NULLREF), (0, MOBI_E_ARG), (n + 1, MOBI_E_ARG), (-1, MOBI_E_ARG)):
        rc, got = r.compare(modulus)
        assert rc == rc_want and (got == UNTOUCHED).all(), (modulus, rc, got.tolist())
    _, frames = _stream(64, 16, 5100, 1)
    assert r.b.decode([frames[0]] * n, [0] * n)[0] == [0] * n
    for modulus in (0, n + 1):
        rc, got = r.compare(modulus)
        assert rc == MOBI_E_ARG and (got == UNTOUCHED).all(), (modulus, rc, got.tolist())
    r.expect(1, {})
    assert r.b.compare_clips(1) == 0  # the wrapper's answer stays what it was
    r.close()
