"""GPU: Sx audio through MobiclipAudio (mobi_sx.hip) against the model written from SxDecoder.cs (sx_model.py), exactly: the recorded
cases with their state carried over 32 calls, lanes and waves with ragged packet counts in both layouts and dtypes, a cut frame, refills
with new codebooks, and a .mods file end to end.  Every expectation is the model's; rows beyond their counts must keep the sentinel the
output was prefilled with."""
import ctypes
import os
import random
import sys
import zlib

import numpy as np
import pytest
import torch  # noqa: F401 -- before the product library is loaded: torch tensors need torch's HIP runtime to be the library's too

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sx_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu
N_SEQ = 5          # distinct (codebook, packet sequence) pairs; lane g uses sequence g % N_SEQ
SEQ_PACKETS = 12
SENTINEL = -21846
_SEQ = {}


def sequence(k):
    """(codebook, packets): tame codebooks for even k, wild for odd.  Packet 0 is a reset packet except in sequence 3, whose new decoder
    starts from zeros; packets 5 and 9 are reset packets that meet parity 0 and parity 1; packet 3 has no long-term prediction."""
    if k not in _SEQ:
        rnd = random.Random(1000 + k)
        cb, packets = sm.codebook(rnd, k % 2 == 0), []
        for b in range(SEQ_PACKETS):
            p = bytearray(rnd.getrandbits(8) for _ in range(20))
            w0 = p[0] | p[1] << 8
            if b in (5, 9) or (b == 0 and k != 3):
                w0 = 0x7F << 9 | w0 & 0x1FF
            elif b == 3:
                w0 = 0x7E << 9 | w0 & 0x1FF
            elif w0 >> 9 == 0x7F:
                w0 &= ~0x200
            p[0], p[1] = w0 & 0xFF, w0 >> 8
            packets.append(bytes(p[:sm.PACKET_BYTES[(p[3] >> 4) & 3]]))
        _SEQ[k] = (cb, packets)
    return _SEQ[k]


class Feeder:
    """Builds the frames of S streams of nc channels from the lanes' sequences, following the model's cursors, and keeps the model."""

    def __init__(self, S, nc, shift=0):
        self.S, self.nc = S, nc
        self.seq = [(g + shift) % N_SEQ for g in range(S * nc)]
        self.pos = [0] * (S * nc)
        self.model = [sm.Stream(self.books(s)) for s in range(S)]

    def books(self, s):
        return [sequence(self.seq[s * self.nc + c])[0] for c in range(self.nc)]

    def frame(self, s, n, lead, commit=True):
        body, cur, pos = b"", self.model[s].cursor, list(self.pos)
        for _ in range(n):
            g = s * self.nc + cur
            body += sequence(self.seq[g])[1][pos[g]]
            pos[g], cur = pos[g] + 1, (cur + 1) % self.nc
        if commit:
            self.pos = pos
        return bytes([0xEE] * lead) + body + bytes(lead % 3)

    def refill(self, s, shift, keep_cursor=False, new_books=True):
        """new decoders for stream s, from the start of (new_books: other) sequences"""
        cur = self.model[s].cursor
        for c in range(self.nc):
            g = s * self.nc + c
            if new_books:
                self.seq[g] = (self.seq[g] + shift) % N_SEQ
            self.pos[g] = 0
        self.model[s].reset(self.books(s))
        if keep_cursor:
            self.model[s].cursor = cur


def prefilled(S, nc, ms, layout, dtype, device):
    shape = (S, nc, ms) if layout == "planar" else (S, ms, nc)
    fill = SENTINEL if dtype == torch.int16 else SENTINEL / 32768
    return torch.full(shape, fill, dtype=dtype, device=torch.device("cuda", device))


def check(out, n_samples, rc, rows, want_rc, layout, dtype):
    S, nc = len(rows), len(rows[0])
    assert rc.tolist() == want_rc
    assert n_samples.tolist() == [[len(r) for r in st] for st in rows]
    ms = out.shape[2] if layout == "planar" else out.shape[1]
    full = np.full((S, nc, ms), SENTINEL, np.int16)
    for s in range(S):
        for c in range(nc):
            full[s, c, :len(rows[s][c])] = rows[s][c]
    if layout == "interleaved":
        full = np.ascontiguousarray(full.transpose(0, 2, 1))
    want = torch.from_numpy(full)
    if dtype == torch.float32:
        want = want.to(torch.float32) / 32768
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("seed,tame", list(sm.CASES), ids=[f"seed{s}-{'tame' if t else 'wild'}" for s, t in sm.CASES])
def test_recorded_cases_three_packets_a_call(seed, tame):
    import mobiclipdecoder_amd as m
    c = sm.case(seed, tame)
    a = m.MobiclipAudio(1, 1, "sx", "mods", codebooks=[[c.cb]])
    outs = []
    for call in range(32):  # the state -- both reset parities among it -- crosses 31 call boundaries on the device
        out, ns, rc = a.decode([c.data], offsets=[c.offsets[3 * call]], n_packets=[3])
        assert rc.tolist() == [0] and ns.tolist() == [[384]] and out.shape == (1, 1, 384)
        outs.append(out)
    torch.cuda.synchronize()
    got = torch.cat(outs, dim=2).cpu().numpy().reshape(-1)
    want = np.array(c.samples, np.int16).reshape(-1)
    first = np.nonzero(got != want)[0]
    assert first.size == 0, f"first difference in packet {first[0] // 128}, sample {first[0] % 128}"
    assert f"{zlib.crc32(got.astype('<i2').tobytes()):08x}" == f"{sm.CASES[(seed, tame)][0]:08x}"
    a.close()


@pytest.mark.parametrize("S,nc", [(5, 2), (33, 2), (22, 3)])
def test_lanes_and_waves_with_ragged_counts_planar(S, nc):
    """a partial wave; a second, nearly empty workgroup; 63 of 64 lanes in two workgroups.  Per stream another n_packets, 0 and empty
    buffers among them; odd counts carry the cursor, so a stream's channels get different lengths."""
    import mobiclipdecoder_amd as m
    f = Feeder(S, nc)
    a16, a32 = (m.MobiclipAudio(S, nc, "sx", "mods", codebooks=[f.books(s) for s in range(S)]) for _ in range(2))
    for call in range(3):
        counts = [(s + call) % 4 for s in range(S)]          # 0, 1, 2, 3 packets
        counts[S - 1] = 3                                    # the last lanes of the last workgroup work in every call
        frames = [f.frame(s, counts[s], 1 + s % 5) if counts[s] or s % 2 else (None if s % 4 else b"") for s in range(S)]
        offs, npk = [1 + s % 5 for s in range(S)], [counts[s] if s % 8 else counts[s] or 2 for s in range(S)]  # a count with an empty buffer
        res = [st.frame(fr or b"", o, n) for st, fr, o, n in zip(f.model, frames, offs, npk)]
        assert all(r[0] == 0 for r in res)
        rows = [r[1] for r in res]
        if call:
            assert any(len(set(len(r) for r in st)) > 1 for st in rows)
        for a, dtype in ((a16, torch.int16), (a32, torch.float32)):
            out = prefilled(S, nc, 128 * 2 + 3, "planar", dtype, a.device)
            got, ns, rc = a.decode(frames, offsets=offs, n_packets=npk, dtype=dtype, out=out)
            torch.cuda.synchronize()
            assert got is out
            check(out, ns, rc, rows, [0] * S, "planar", dtype)
    with pytest.raises(m.MobiclipError):  # unequal counts over a stream's channels refuse the interleaved layout
        a16.decode([f.frame(s, nc + 1, 0, commit=False) for s in range(S)], offsets=[0] * S, n_packets=[nc + 1] * S, layout="interleaved")
    a16.close(), a32.close()


@pytest.mark.parametrize("S,nc", [(5, 2), (33, 2), (22, 3)])
def test_lanes_and_waves_interleaved(S, nc):
    import mobiclipdecoder_amd as m
    f = Feeder(S, nc, shift=1)
    a16, a32 = (m.MobiclipAudio(S, nc, "sx", "mods", codebooks=[f.books(s) for s in range(S)]) for _ in range(2))
    for call in range(2):
        counts = [nc * ((s + call) % 3) for s in range(S)]   # equal counts over a stream's channels: 0, 1 or 2 packets each
        counts[S - 1] = 2 * nc
        frames = [f.frame(s, counts[s], s % 3) for s in range(S)]
        offs = [s % 3 for s in range(S)]
        rows = [st.frame(fr, o, n)[1] for st, fr, o, n in zip(f.model, frames, offs, counts)]
        for a, dtype in ((a16, torch.int16), (a32, torch.float32)):
            out = prefilled(S, nc, 128 * 2 + 1, "interleaved", dtype, a.device)
            _, ns, rc = a.decode(frames, offsets=offs, n_packets=counts, dtype=dtype, layout="interleaved", out=out)
            torch.cuda.synchronize()
            check(out, ns, rc, rows, [0] * S, "interleaved", dtype)
    a16.close(), a32.close()


def test_a_cut_frame_leaves_its_stream_untouched_and_the_rest_exact():
    import mobiclipdecoder_amd as m
    S, nc = 5, 2
    f = Feeder(S, nc)
    a = m.MobiclipAudio(S, nc, "sx", "mods", codebooks=[f.books(s) for s in range(S)])
    for call, cut in enumerate((None, 2, None)):
        frames = [f.frame(s, 3, 2, commit=(s != cut)) for s in range(S)]
        if cut is not None:
            frames[cut] = frames[cut][:-(2 % 3) - 1]         # the last packet is one byte short
        res = [st.frame(fr, 2, 3) for st, fr in zip(f.model, frames)]
        want_rc = [sm.E_INDEX if s == cut else 0 for s in range(S)]
        assert [r[0] for r in res] == want_rc
        out = prefilled(S, nc, 300, "planar", torch.int16, a.device)
        _, ns, rc = a.decode(frames, offsets=[2] * S, n_packets=[3] * S, out=out)
        torch.cuda.synchronize()
        check(out, ns, rc, [r[1] for r in res], want_rc, "planar", torch.int16)  # call 2: stream 2 decodes as if the cut frame had never come
    a.close()


def test_refills_with_new_codebooks_and_plain_resets_between_calls():
    import mobiclipdecoder_amd as m
    S, nc = 6, 2
    f = Feeder(S, nc)
    a = m.MobiclipAudio(S, nc, "sx", "mods", codebooks=[f.books(s) for s in range(S)])
    for call in range(4):
        if call == 1:  # cursors are 1 everywhere: three packets over two channels
            assert [st.cursor for st in f.model] == [1] * S
            f.refill(1, 1), f.refill(3, 2)
            a.reset([1, 3], codebooks=[f.books(1), f.books(3)])  # new codebooks, cursor 0
            f.refill(4, 0, new_books=False)
            a.reset([4])                                         # mobi_audio_reset: the codebooks stay, cursor 0
            f.refill(0, 0, keep_cursor=True, new_books=False)
            a.reset([0], keep_cursor=True)
            assert [st.cursor for st in f.model] == [1, 0, 1, 0, 0, 1]
        if call == 2:  # a refill whose first frame is empty still takes effect, and a second one before any decode replaces the first
            f.refill(2, 1)
            a.reset([2], codebooks=[[bytes(sm.CODEBOOK_BYTES)] * nc])
            a.reset([2], codebooks=[f.books(2)])
        counts = [0 if (call, s) == (2, 5) else 3 for s in range(S)]
        frames = [f.frame(s, counts[s], 4) for s in range(S)]
        res = [st.frame(fr, 4, n) for st, fr, n in zip(f.model, frames, counts)]
        out = prefilled(S, nc, 260, "planar", torch.int16, a.device)
        _, ns, rc = a.decode(frames, offsets=[4] * S, n_packets=counts, out=out)
        torch.cuda.synchronize()
        check(out, ns, rc, [r[1] for r in res], [0] * S, "planar", torch.int16)
    cb = bytes(sm.CODEBOOK_BYTES)
    for kw in (dict(streams=[0], codebooks=[[cb]]), dict(streams=[0, 1], codebooks=[[cb, cb]]), dict(streams=[S], codebooks=[[cb, cb]]),
               dict(streams=[0], codebooks=[[cb, cb[1:]]]), dict(streams=[0], codebooks=[[cb, cb]], keep_cursor=True)):
        with pytest.raises(ValueError):
            a.reset(**kw)
    a.close()
    b = m.MobiclipAudio(1, 1, "fastaudio", "mods")
    with pytest.raises(ValueError):
        b.reset([0], codebooks=[[cb]])
    book = ctypes.create_string_buffer(cb)
    assert b._lib.mobi_sx_reset(b._h, (ctypes.c_int32 * 1)(0), 1, (ctypes.c_void_p * 1)(ctypes.addressof(book))) == -7  # a handle of another codec
    b.close()


def test_end_to_end_mods_file_with_codebooks():
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.demux import ModsDemuxer
    nc, n_audio, video = 2, [3, 0, 2, 4, 1], [5, 9, 4, 7, 3]
    f = Feeder(1, nc, shift=2)
    packets = []
    for fr, n in enumerate(n_audio):  # the video bits, then the audio packets, then padding
        packets.append(bytes([0x11 * (fr + 1)] * video[fr]) + f.frame(0, n, 0) + bytes(3))
    dm = ModsDemuxer(sm.write_mods(packets, n_audio, [0, 2], nc, f.books(0)))
    assert (dm.Header.audio_codec, dm.Header.nb_channel) == (1, nc) and dm.AudioCodebooks == f.books(0)
    a = m.MobiclipAudio(1, dm.Header.nb_channel, dm.Header.audio_codec, "mods", codebooks=[dm.AudioCodebooks])
    model = sm.Stream(dm.AudioCodebooks)
    total = 0
    for fr in range(len(packets)):
        pkt, na, key = dm.ReadFrame()
        assert na == n_audio[fr]                 # Sx decoders are not renewed at key frames (Program.cs:253-288)
        offset = (video[fr] + 2) - 2             # Program.cs:250: the video decode would return video[fr] + 2
        out, ns, rc = a.decode([pkt], offsets=[offset], n_packets=[na], max_samples=256)
        torch.cuda.synchronize()
        res = model.frame(pkt, offset, na)
        assert res[0] == 0 and rc.tolist() == [0] and ns.tolist() == [[len(r) for r in res[1]]]
        for c in range(nc):
            assert out.cpu()[0, c, :len(res[1][c])].tolist() == res[1][c]
        total += sum(len(r) for r in res[1])
    assert dm.ReadFrame() is None and total == 128 * sum(n_audio)
    a.close()
