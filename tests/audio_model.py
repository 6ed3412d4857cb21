"""Reference model of the audio codecs and framings in plain Python integers: the expectation of tests/test_audio_model.py and
tests/test_audio_gpu.py.  Written from the reference's semantics -- FastAudioDecoder.cs keeps an Internal[] array of unpacked fields,
builds the 256-sample excitation, then filters it in place; IMAADPCMDecoder.cs; the converter's loops (Program.cs:75-157, 248-319) --
with unbounded ints wrapped to int32 where C# wraps, and independently of csrc/mobi_audio.h (which computes the excitation on the fly, in
uint32).  The tables come through the library's getter (audio.tables()); the tests pin their CRCs."""
import struct
import zlib

import numpy as np

E_INDEX, E_UNSUPPORTED = -1, -6
TAME_GAIN = 8  # every 6-bit FastAudio gain forced to at most this: the model counts no lattice product outside int32 on the tests' bytes
                # (8 was the first value tried; tests/test_audio_model.py asserts the count)


def wrap32(v):
    """an unbounded int as the int32 C# keeps (unchecked arithmetic)"""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def in_int32(v):
    return -(1 << 31) <= v < (1 << 31)


def lcg_bytes(n, x):
    """x <- (x * 1103515245 + 12345) mod 2^31, byte = (x >> 16) & 0xFF -> (bytes, x)"""
    out = bytearray(n)
    for i in range(n):
        x = (x * 1103515245 + 12345) % (1 << 31)
        out[i] = (x >> 16) & 0xFF
    return bytes(out), x


def tame(block, limit):
    """a FastAudio block with every 6-bit gain field of word 1 forced to at most `limit`"""
    w = list(struct.unpack("<10I", block))
    for sh in (8, 14, 20, 26):
        g = (w[1] >> sh) & 0x3F
        w[1] = (w[1] & ~(0x3F << sh)) | (min(g, limit) << sh)
    return struct.pack("<10I", *w)


def crc_i16(samples):
    return zlib.crc32(np.asarray(samples, "<i2").tobytes())


class FastAudio:
    """new FastAudioDecoder(); Decode() per 40-byte block"""

    def __init__(self, t):
        self.t = t
        self.lat = [0] * 9      # Internal[100..108]
        self.deemph = 0         # Internal[109]
        self.overflows = 0      # lattice products that left int32

    def _mul(self, a, b):
        """a lattice product, counted when it leaves int32"""
        p = a * b
        if not in_int32(p):
            self.overflows += 1
        return wrap32(p)

    _memo = {}  # (block, state) -> (samples, state, overflows): the GPU tests feed many lanes the same few byte sequences

    def decode(self, block):
        key = (bytes(block), tuple(self.lat[:8]), self.deemph)
        hit = FastAudio._memo.get(key)
        if hit is None:
            before = self.overflows
            out = self._decode(block)
            FastAudio._memo[key] = (out, list(self.lat), self.deemph, self.overflows - before)
            return list(out)
        self.lat, self.deemph, self.overflows = list(hit[1]), hit[2], self.overflows + hit[3]
        return list(hit[0])

    def _decode(self, block):
        assert len(block) == 40
        w = struct.unpack("<10I", block)
        t = self.t
        coef = [0] * 8
        coef[0] = int(t["k01"][w[0] >> 26])
        coef[1] = int(t["k01"][(w[0] >> 20) & 0x3F])
        coef[2] = int(t["k2"][(w[0] >> 15) & 0x1F])
        coef[3] = int(t["k3"][(w[0] >> 10) & 0x1F])
        coef[4] = int(t["k4"][(w[0] >> 6) & 0xF])
        coef[6] = int(t["k6"][(w[0] >> 3) & 7])
        coef[7] = int(t["k7"][w[0] & 7])
        coef[5] = int(t["k5"][(w[9] & 1) | ((w[7] & 1) << 1) | ((w[5] & 1) << 2) | ((w[3] & 1) << 3)])
        gains = [(w[1] >> (8 + 6 * i)) & 0x3F for i in range(4)]
        offsets = [(w[1] >> (2 * i)) & 3 for i in range(4)]
        exc = []
        for sub in range(4):
            a, b = w[2 + 2 * sub], w[3 + 2 * sub]
            codes = [(a >> (29 - 3 * i)) & 7 for i in range(10)] + [(b >> (29 - 3 * i)) & 7 for i in range(10)]
            codes.append(((b >> 1) & 1) | ((a & 3) << 1))
            exc += [0] * offsets[sub]
            for i, c in enumerate(codes):
                exc.append(int(t["pulse"][gains[sub] * 8 + c]))
                if i < 20:
                    exc += [0, 0]
            exc += [0] * (3 - offsets[sub])
        assert len(exc) == 256
        out = []
        lat, r9 = self.lat, self.deemph
        for x in exc:
            r5 = x
            for j in range(8):
                r6, r7 = coef[7 - j], lat[7 - j]
                r5 = wrap32(r5 - (wrap32(self._mul(r6, r7) + 0x4000) >> 15))
                lat[8 - j] = wrap32(r7 + (wrap32(self._mul(r6, r5) + 0x4000) >> 15))
            lat[0] = r5
            r9 = wrap32(r5 + (wrap32(wrap32(r9 * 0x6E14) + 0x4000) >> 15))
            out.append(max(-32768, min(32767, wrap32(r9 * 2))))
        self.deemph = r9
        return out


class ImaAdpcm:
    """new IMAADPCMDecoder(); GetWaveData(Data, Offset, Length): the first call reads the 4-byte header"""

    def __init__(self, t, last=None, index=None):
        self.t = t
        self.init = last is not None
        self.last, self.index = last, index

    def get_wave_data(self, data, offset, length):
        out = []
        if not self.init:
            if offset + 4 > len(data):
                raise IndexError
            self.index = struct.unpack_from("<h", data, offset)[0] & 0x7F
            self.last = struct.unpack_from("<h", data, offset + 2)[0]
            offset, length, self.init = offset + 4, length - 4, True
        for i in range(offset, offset + length):
            if i >= len(data):
                raise IndexError
            for nib in (data[i] & 0xF, data[i] >> 4):
                if self.index > 88:
                    raise IndexError
                step = int(self.t["ima_step"][self.index])
                diff = step // 8 + step // 4 * (nib & 1) + step // 2 * ((nib >> 1) & 1) + step * ((nib >> 2) & 1)
                self.last = max(-32768, min(32767, self.last - diff if nib & 8 else self.last + diff))
                self.index = max(0, min(88, self.index + int(self.t["ima_index"][nib & 7])))
                out.append(self.last)
        return out


class Stream:
    """One stream's decoders and what the converter keeps between frames.  frame() -> (rc, [samples per channel]); a frame the reference
    would throw on gives (E_INDEX, empty rows) and leaves the stream as it was (this library's contract: the frame never came)."""

    def __init__(self, t, framing, codec, n_channels):
        self.t, self.framing, self.codec, self.C = t, framing, codec, n_channels
        self.cursor = 0
        self.reset(keep_cursor=False)

    def reset(self, keep_cursor):
        self.fa = [FastAudio(self.t) for _ in range(self.C)]
        self.ima = [ImaAdpcm(self.t) for _ in range(self.C)]
        if not keep_cursor:
            self.cursor = 0

    def _snapshot(self):
        return ([(list(f.lat), f.deemph, f.overflows) for f in self.fa], [(d.init, d.last, d.index) for d in self.ima], self.cursor)

    def _restore(self, snap):
        for f, (lat, de, ov) in zip(self.fa, snap[0]):
            f.lat, f.deemph, f.overflows = lat, de, ov
        for d, (init, last, index) in zip(self.ima, snap[1]):
            d.init, d.last, d.index = init, last, index
        self.cursor = snap[2]

    def frame(self, data, offset=0, n_packets=0):
        data = bytes(data)
        empty = [[] for _ in range(self.C)]
        if self.codec == "sx":
            return E_UNSUPPORTED, empty
        if len(data) == 0 or (self.framing == "mods" and n_packets == 0):
            return 0, empty
        snap = self._snapshot()
        try:
            return 0, (self._moflex(data) if self.framing == "moflex" else self._mods(data, offset, n_packets))
        except IndexError:
            self._restore(snap)
            return E_INDEX, empty

    def _moflex(self, data):
        C, rows = self.C, [[] for _ in range(self.C)]
        if self.codec == "pcm16":
            n = (len(data) - len(data) % (2 * C)) // 2
            v = struct.unpack("<%dh" % n, data[:2 * n])
            return [list(v[c::C]) for c in range(C)]
        if self.codec == "fastaudio":
            off = 0
            while off + 40 < len(data):
                for c in range(C):
                    if off + 40 > len(data):
                        raise IndexError
                    rows[c] += self.fa[c].decode(data[off:off + 40])
                    off += 40
            return rows
        dec = [ImaAdpcm(self.t) for _ in range(C)]  # new decoders every frame
        for c in range(C):
            dec[c].get_wave_data(data, 4 * c, 4)
            if dec[c].index > 88:
                raise IndexError  # this library rejects the header itself; the reference throws at the first sample
        off = 4 * C
        while off + 128 * C < len(data):
            for c in range(C):
                rows[c] += dec[c].get_wave_data(data, off, 128)
                off += 128
        return rows

    def _mods(self, data, off, n_packets):
        C, rows = self.C, [[] for _ in range(self.C)]
        for _ in range(n_packets):
            c = self.cursor
            if self.codec == "ima":
                size = 128 + (0 if self.ima[c].init else 4)
                if off + size > len(data):
                    raise IndexError
                rows[c] += self.ima[c].get_wave_data(data, off, size)
            else:
                size = 40
                if off + size > len(data):
                    raise IndexError
                rows[c] += self.fa[c].decode(data[off:off + 40])
            off += size
            self.cursor = (c + 1) % C
        return rows

    def blocks(self, data, offset=0, n_packets=0):
        """the framing alone, as mobi_audio_plan reports it: (rc, [(offset, channel, header, header_offset)], samples per channel, the
        cursor afterwards).  The stream does not move."""
        log, before = [], self.cursor
        rc, rows = self._trace(bytes(data), offset, n_packets, log)
        after, self.cursor = self.cursor, before
        return rc, (log if rc == 0 else []), [len(r) for r in rows], (after if rc == 0 else before)

    def _trace(self, data, offset, n_packets, log):
        """frame()'s walk over the bytes with every block recorded and no sample decoded; moves nothing but the cursor"""
        C = self.C
        empty = [[] for _ in range(C)]
        if self.codec == "sx":
            return E_UNSUPPORTED, empty
        if len(data) == 0 or (self.framing == "mods" and n_packets == 0):
            return 0, empty
        rows = [[] for _ in range(C)]
        try:
            if self.framing == "moflex" and self.codec == "pcm16":
                return 0, self._moflex(data)
            if self.framing == "moflex" and self.codec == "fastaudio":
                off = 0
                while off + 40 < len(data):
                    for c in range(C):
                        if off + 40 > len(data):
                            raise IndexError
                        log.append((off, c, 0, 0))
                        rows[c] += [0] * 256
                        off += 40
            elif self.framing == "moflex":
                for c in range(C):
                    if 4 * c + 4 > len(data) or (struct.unpack_from("<h", data, 4 * c)[0] & 0x7F) > 88:
                        raise IndexError
                off, first = 4 * C, 1
                while off + 128 * C < len(data):
                    for c in range(C):
                        log.append((off, c, first, 4 * c))
                        rows[c] += [0] * 256
                        off += 128
                    first = 0
            else:
                off = offset
                fresh = [self.codec == "ima" and not d.init for d in self.ima]
                for _ in range(n_packets):
                    c = self.cursor
                    hdr = 4 if fresh[c] else 0
                    size = (128 if self.codec == "ima" else 40) + hdr
                    if off + size > len(data):
                        raise IndexError
                    if hdr and (struct.unpack_from("<h", data, off)[0] & 0x7F) > 88:
                        raise IndexError
                    log.append((off + hdr, c, 1 if hdr else 0, off))
                    rows[c] += [0] * 256
                    fresh[c] = False
                    off += size
                    self.cursor = (c + 1) % C
        except IndexError:
            return E_INDEX, empty
        return 0, rows
