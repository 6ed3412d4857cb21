"""A model of the Sx audio decoder (Mods audio_codec 1) in plain Python integers, for tests.

Written from LibMobiclip/Codec/Sx/SxDecoder.cs, function by function, over the same `Internal` byte array and the same offsets; int32
arithmetic wraps explicitly (`Sx.w`), and every operation whose exact result leaves int32 is counted.  It knows nothing of the
library's own restatement.  `Internal` is kept as its 558 little-endian int32 words (`I[off >> 2]`); the four bytes at 0x68..0x6B are
the four bytes of word 0x68.

    Internal  0x00  the eight coefficient sums          0x60  gain           0x70  the filter's eight last outputs
              0x20  coefficient set, 0x40 the other     0x64  parity         0xB8  buffer 0 (256 words)
              0x68  stage rows 0, 1, 2 and the rate     0x6C  output cursor  0x4B8 buffer 1 (256 words)

Also the Mods framing around it (MobiConverter/Program.cs:275-288): `plan`.
"""
import struct
import zlib

CODEBOOK_BYTES = 0xC34
INTERNAL_WORDS = 0x8B8 // 4
PACKET_BYTES = (0x14, 0xE, 0xC, 0xA)  # table_83E, by rate
PACKET_SAMPLES = 128
TABLE_836 = (0, 0, 5, 0xC, 4, 0x10, 3, 0x14)
SCRATCH_WORDS = (0x68 >> 2, 0x6C >> 2)  # written before they are read in every packet: not state


class OutOfData(Exception):
    """The reference's read past the end of the packet buffer."""


class Sx:
    def __init__(self, codebook):
        assert len(codebook) == CODEBOOK_BYTES
        self.cb = bytes(codebook)
        self.I = [0] * INTERNAL_WORDS
        self.data = b""
        self.off = 0
        self.wraps = 0
        self.clamps = 0

    # ---- int32 ----
    def w(self, v):
        r = ((v + 0x80000000) & 0xFFFFFFFF) - 0x80000000
        if r != v:
            self.wraps += 1
        return r

    def rd(self, off):
        return self.I[off >> 2]

    def wr(self, off, v):
        assert -0x80000000 <= v <= 0x7FFFFFFF and not off & 3
        self.I[off >> 2] = v

    def byte(self, off):
        return (self.I[off >> 2] >> (8 * (off & 3))) & 0xFF

    def set_byte(self, off, b):
        u = self.I[off >> 2] & 0xFFFFFFFF
        sh = 8 * (off & 3)
        u = (u & ~(0xFF << sh)) | ((b & 0xFF) << sh)
        self.I[off >> 2] = u - (1 << 32) if u & 0x80000000 else u

    def u16(self):
        if self.off + 2 > len(self.data):
            raise OutOfData
        v = self.data[self.off] | (self.data[self.off + 1] << 8)
        self.off += 2
        return v

    def cb16(self, off):
        return struct.unpack_from("<h", self.cb, off)[0]

    def cb32(self, off):
        return struct.unpack_from("<i", self.cb, off)[0]

    # ---- Decode ----
    def decode(self, data, offset):
        """One packet at data[offset:]; returns (128 samples, the offset behind the packet)."""
        self.data, self.off = data, offset
        val = self.u16()
        if val >> 9 == 0x7F:
            result = self.sub_8BC(val)
        else:
            result = self.sub_8FC(val)
        self.wr(0x64, self.rd(0x64) ^ 1)
        dst = []
        for i in range(128):
            r7 = self.rd(result + 4 * i)
            if r7 > 32767 or r7 < -32768:
                self.clamps += 1
            dst.append(max(-32768, min(32767, r7)))
        assert self.off - offset == PACKET_BYTES[self.byte(0x6B)]
        return dst, self.off

    def sub_0(self, io):
        for i in range(128):
            self.wr(io + 0x200 + 4 * i, 0)

    def sub_28(self, io, io2, lag):
        io += 0x200
        io2 += (0x7F - lag) * 4
        src = [self.rd(io2 + 4 * i) for i in range(128)]
        out = [src[0] >> 4]
        r1 = 2
        for i in range(1, 7):
            out.append(self.w(src[i] * r1) >> 4)
            r1 += 1
        r1 -= 1  # the seventh increment is commented out in the reference: r1 stays 7
        for i in range(7, 7 + 0x72):
            out.append(src[i] >> 1)
        for i in range(121, 127):
            out.append(self.w(src[i] * r1) >> 4)
            r1 -= 1
        out.append(src[127] >> 4)
        assert len(out) == 128 and r1 == 1
        for i in range(128):
            self.wr(io + 4 * i, out[i])

    def sub_170(self, io, g, pos, words, stride):
        io += 0x200 + pos * 4
        r7 = self.w(-g)
        r6 = self.w(g * 2)
        r7 = self.w(r7 - r6)
        for _ in range(words):
            val = self.u16()
            for sh in range(0xE, -1, -2):
                r2 = self.w(self.w(r6 * ((val >> sh) & 3)) + r7)
                self.wr(io, self.w(self.rd(io) + r2))
                io += stride

    def sub_1B8(self, io, g, pos):
        io += 0x200 + pos * 4
        r7 = self.w(-g)
        r6 = self.w(g << 1)
        r7 = self.w(r7 - self.w(r6 << 1))
        r7 = self.w(r7 - r6)
        r9 = 0
        for _ in range(8):
            val = self.u16()
            for sh in range(0xD, -1, -3):
                r2 = self.w(self.w(r6 * ((val >> sh) & 7)) + r7)
                self.wr(io, self.w(self.rd(io) + r2))
                io += 0xC
            r9 = (r9 << 1) | (val & 1)
        for sh in (5, 2):
            r2 = self.w(self.w(r6 * ((r9 >> sh) & 7)) + r7)
            self.wr(io, self.w(self.rd(io) + r2))
            io += 0xC

    def sub_3B4(self, cbo, c):
        for i in range(8):
            c[i] = self.w(c[i] + self.cb16(cbo + 2 * i))

    def sub_244(self, from_codebook, off):
        w = self.w
        if from_codebook:
            c = [self.cb32(off + 4 * i) for i in range(8)]
        else:
            c = [self.rd(off + 4 * i) for i in range(8)]
        self.sub_3B4(self.byte(0x68) * 16, c)
        self.sub_3B4(self.byte(0x69) * 16 + 0x400, c)
        self.sub_3B4(self.byte(0x6A) * 16 + 0x800, c)
        for i in range(8):
            self.wr(4 * i, c[i])

        def m(a, b):  # (a * b) >> 15
            return w(a * b) >> 15

        c[0] = w(c[0] + m(c[0], c[1]))
        tmp = w(c[0] * c[2])
        c[0] = w(c[0] + m(c[1], c[2]))
        c[1] = w(c[1] + (tmp >> 15))
        tmp = w(c[0] * c[3])
        c[0] = w(c[0] + m(c[2], c[3]))
        c[2] = w(c[2] + (tmp >> 15))
        c[1] = w(c[1] + m(c[1], c[3]))
        tmp = w(c[0] * c[4])
        c[0] = w(c[0] + m(c[3], c[4]))
        c[3] = w(c[3] + (tmp >> 15))
        tmp = w(c[1] * c[4])
        c[1] = w(c[1] + m(c[2], c[4]))
        c[2] = w(c[2] + (tmp >> 15))
        tmp = w(c[0] * c[5])
        c[0] = w(c[0] + m(c[4], c[5]))
        c[4] = w(c[4] + (tmp >> 15))
        tmp = w(c[1] * c[5])
        c[1] = w(c[1] + m(c[3], c[5]))
        c[3] = w(c[3] + (tmp >> 15))
        c[2] = w(c[2] + m(c[2], c[5]))
        tmp = w(c[0] * c[6])
        c[0] = w(c[0] + m(c[5], c[6]))
        c[5] = w(c[5] + (tmp >> 15))
        tmp = w(c[1] * c[6])
        c[1] = w(c[1] + m(c[4], c[6]))
        c[4] = w(c[4] + (tmp >> 15))
        tmp = w(c[2] * c[6])
        c[2] = w(c[2] + m(c[3], c[6]))
        c[3] = w(c[3] + (tmp >> 15))
        tmp = w(c[0] * c[7])
        c[0] = w(c[0] + m(c[6], c[7]))
        c[6] = w(c[6] + (tmp >> 15))
        tmp = w(c[1] * c[7])
        c[1] = w(c[1] + m(c[5], c[7]))
        c[5] = w(c[5] + (tmp >> 15))
        tmp = w(c[2] * c[7])
        c[2] = w(c[2] + m(c[4], c[7]))
        c[4] = w(c[4] + (tmp >> 15))
        c[3] = w(c[3] + m(c[3], c[7]))
        return [w(-(x >> 1)) for x in c]

    def sub_3F8(self, io, n, c):
        """Filters n samples from Internal[io]; returns io behind them."""
        h = 0x70
        r1 = self.rd(0x6C)
        while n:
            for i in range(8):
                r4 = self.w(self.rd(io) << 14)
                io += 4
                idx = (7 + i) & 7
                for i2 in range(8):
                    r4 = self.w(r4 + self.w(self.rd(h + idx * 4) * c[i2]))
                    idx = 7 if idx == 0 else idx - 1
                r4 >>= 14
                self.wr(h + i * 4, r4)
                self.wr(r1, r4)
                r1 += 4
            n -= 8
        self.wr(0x6C, r1)
        return io

    def sub_6C0(self, r2, c):
        for i in range(8):
            c[i] = self.w(c[i] + self.rd(r2 + i * 4)) >> 1

    def sub_728(self, io, io2, c):
        r2 = self.rd(0x64)
        r0 = io + 0x200
        self.wr(0x6C, io2)
        if r2 == 1:
            io2 = 0x20
            io = io2 + 0x20
        else:
            io = 0x20
            io2 = io + 0x20
        for i in range(8):
            self.wr(io + i * 4, c[i])
        self.sub_6C0(io2, c)
        c2 = list(c)
        self.sub_6C0(io2, c)
        r0 = self.sub_3F8(r0, 0x20, c)
        c[:] = c2
        r0 = self.sub_3F8(r0, 0x20, c)
        self.sub_6C0(io, c)
        r0 = self.sub_3F8(r0, 0x20, c)
        for i in range(8):
            c[i] = self.rd(io + i * 4)
        self.sub_3F8(r0, 0x20, c)

    def sub_798(self):
        self.wr(0x60, self.cb32(0xC30))
        self.wr(0x64, 1)
        for i in range(8):
            self.wr(0x70 + 4 * i, 0)

    def sub_844(self, io, val):
        r6 = (val >> 6) & 7
        self.set_byte(0x68, val & 0x3F)
        val = self.u16()
        r7 = (val >> 14) & 3
        r8 = self.cb16(0xC00 + r6 * 2)
        r6 = self.rd(0x60)
        r11 = (val >> 12) & 3
        r6 = self.w(r8 * r6) >> 13
        self.wr(0x60, r6)
        self.set_byte(0x69, (val >> 6) & 0x3F)
        self.set_byte(0x6A, val & 0x3F)
        self.set_byte(0x6B, r11)
        if r11 == 0:
            self.sub_1B8(io, r6, r7)
        else:
            self.sub_170(io, r6, r7, TABLE_836[r11 * 2], TABLE_836[r11 * 2 + 1])

    def sub_8BC(self, val):
        self.sub_798()
        self.sub_0(0x4B8)
        self.sub_844(0x4B8, val)
        c = self.sub_244(True, 0xC10)
        for i in range(8):
            self.wr(0x40 + i * 4, c[i])
        self.wr(0x6C, 0xB8)
        self.sub_3F8(0x6B8, 0x80, c)
        return 0xB8

    def sub_8FC(self, val):
        r2 = self.rd(0x64)
        r3 = r2 * 0x400 + 0xB8
        r4 = (r2 ^ 1) * 0x400 + 0xB8
        r7 = r4 + 0x200
        for i in range(128):
            self.wr(r3 + 4 * i, self.rd(r7 + 4 * i))
        if val >> 9 == 0x7E:
            self.sub_0(r3)
        else:
            self.sub_28(r3, r4, val >> 9)
        self.sub_844(r3, val)
        c = self.sub_244(False, 0)
        self.sub_728(r3, r4, c)
        return r4


def plan(n_channels, data, offset, n_packets, cursor):
    """The Mods framing for Sx: [(packet offset, channel)], samples per channel, the next cursor.  OutOfData where the reference's
    decoder would read past `data`: the packet's two header words, then the pulse words its rate asks for."""
    out, per, off, cur = [], [0] * n_channels, offset, cursor
    for _ in range(n_packets):
        if off + 4 > len(data):
            raise OutOfData
        rate = (data[off + 3] >> 4) & 3
        if off + PACKET_BYTES[rate] > len(data):
            raise OutOfData
        out.append((off, cur))
        per[cur] += PACKET_SAMPLES
        off += PACKET_BYTES[rate]
        cur = cur + 1 if cur + 1 < n_channels else 0
    return out, per, cur


# ---- the recorded cases ----
def codebook(rnd, tame):
    if not tame:
        return bytes(rnd.getrandbits(8) for _ in range(0xC34))
    cb = bytearray(0xC34)
    for i in range(0x600):
        struct.pack_into("<h", cb, 2 * i, rnd.randint(-900, 900))
    for i in range(8):
        struct.pack_into("<h", cb, 0xC00 + 2 * i, rnd.randint(6000, 8600))
    for i in range(8):
        struct.pack_into("<i", cb, 0xC10 + 4 * i, rnd.randint(-6000, 6000))
    struct.pack_into("<i", cb, 0xC30, rnd.randint(40, 400))
    return bytes(cb)


def patch_w0(b, w0):
    if b % 33 in (0, 16):
        return 0x7F << 9 | w0 & 0x1FF
    if b % 11 == 5:
        return 0x7E << 9 | w0 & 0x1FF
    if w0 >> 9 == 0x7F:
        return w0 & ~0x200
    return w0


CASES = {  # (seed, tame): crc, bytes consumed, packets by rate
    (1, True): (0x02927EA7, 1426, (32, 21, 31, 12)),
    (2, True): (0x9FCFE814, 1318, (22, 21, 27, 26)),
    (1, False): (0xF7374740, 1344, (25, 24, 19, 28)),
    (2, False): (0xF3B055E3, 1314, (18, 31, 25, 22)),
}
N_CASE_PACKETS = 96


class Case:
    """One recorded case decoded by the model: the patched bytes, every packet's offset, samples and Internal afterwards."""

    def __init__(self, seed, tame):
        import random

        rnd = random.Random(seed)
        self.cb = codebook(rnd, tame)
        data = bytearray(rnd.getrandbits(8) for _ in range(N_CASE_PACKETS * 20))
        d = Sx(self.cb)
        self.offsets, self.samples, self.states, self.rates = [], [], [], [0, 0, 0, 0]
        off = 0
        for b in range(N_CASE_PACKETS):
            w0 = patch_w0(b, data[off] | data[off + 1] << 8)
            data[off], data[off + 1] = w0 & 0xFF, w0 >> 8
            self.offsets.append(off)
            s, off = d.decode(data, off)
            self.samples.append(s)
            self.states.append(list(d.I))
            self.rates[d.byte(0x6B)] += 1
        self.consumed = off
        self.data = bytes(data[:off])
        self.offsets.append(off)
        self.wraps, self.clamps = d.wraps, d.clamps
        self.crc = zlib.crc32(b"".join(struct.pack("<128h", *s) for s in self.samples))


_cases = {}


def case(seed, tame):
    """Computed once, shared and never changed by the tests."""
    if (seed, tame) not in _cases:
        _cases[(seed, tame)] = Case(seed, tame)
    return _cases[(seed, tame)]


def write_mods(packets, n_audio, key_frames, channels, codebooks=None, audio_codec=1, frequency=32768):
    """A .mods image: header, the frame packets (each behind its u32 size << 14 | NrAudioPackets), the codebooks (0xC34 bytes per channel,
    the header's audio_offset pointing at them; None: audio_offset 0), the key frame index."""
    body, offsets, pos = [], [], 0x30
    for p, n in zip(packets, n_audio):
        offsets.append(pos)
        body.append(struct.pack("<I", (len(p) << 14) | n) + bytes(p))
        pos += 4 + len(p)
    books = b"".join(codebooks) if codebooks is not None else b""
    assert len(books) == (CODEBOOK_BYTES * channels if codebooks is not None else 0)
    index = b"".join(struct.pack("<II", k, offsets[k]) for k in key_frames)
    header = struct.pack("<4sHHIIIIHHIIIII", b"MODS", 0x0A, 0x0C, len(packets), 256, 192, 0x18000000, audio_codec, channels, frequency,
                         max(len(p) for p in packets), pos if codebooks is not None else 0, pos + len(books), len(key_frames))
    return header + b"".join(body) + books + index


E_INDEX = -1


class Stream:
    """One .mods stream's Sx decoders and channel cursor, as the converter keeps them (Program.cs:225-288)."""

    def __init__(self, codebooks):
        self.books = [bytes(b) for b in codebooks]
        self.reset()

    def reset(self, codebooks=None):
        if codebooks is not None:
            self.books = [bytes(b) for b in codebooks]
        self.dec = [Sx(b) for b in self.books]
        self.cursor = 0

    def frame(self, data, offset, n_packets):
        """-> (rc, samples per channel); a frame the reference would throw on leaves everything as it was."""
        data, nc = bytes(data), len(self.dec)
        rows = [[] for _ in range(nc)]
        if not data or not n_packets:
            return 0, rows
        try:
            pk, _, cur = plan(nc, data, offset, n_packets, self.cursor)
        except OutOfData:
            return E_INDEX, rows
        for off, c in pk:
            rows[c] += self.dec[c].decode(data, off)[0]
        self.cursor = cur
        return 0, rows
