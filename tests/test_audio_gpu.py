"""GPU: MobiclipAudio (mobi_audio.hip) against the reference model in plain Python integers (audio_model.py), exactly: torch.equal on
int16, and on float32 against model / 32768.  Lanes share a few byte sequences (the model memoises), so every case takes well under a
second of model time; the rows beyond their counts must keep the sentinel the output was prefilled with."""
import os
import struct
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the product library is loaded: torch tensors need torch's HIP runtime to be the library's too

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_model as am  # noqa: E402
from containers import _ep, _synchro_header, _varbyte  # noqa: E402

pytestmark = pytest.mark.gpu
N_SEQ = 5        # distinct byte sequences; lane g uses sequence g % N_SEQ
SENTINEL = -21846


@pytest.fixture(scope="module")
def tables():
    from mobiclipdecoder_amd import audio
    return audio.tables()


_BLOCKS = {}


def lane_blocks(codec, g, n, tame=False):
    """the first n blocks of lane g's sequence (FastAudio: from x = 1 + g % N_SEQ, sequence 0 is the recorded wild set)"""
    key = (codec, g % N_SEQ, tame)
    have = _BLOCKS.setdefault(key, ([], [(1 if codec == "fastaudio" else 7) + g % N_SEQ]))
    while len(have[0]) < n:
        b, have[1][0] = am.lcg_bytes(40 if codec == "fastaudio" else 128, have[1][0])
        have[0].append(am.tame(b, am.TAME_GAIN) if tame else b)
    return have[0][:n]


def ima_header(g, salt=0):
    return struct.pack("<hh", (g * 17 + salt * 5) % 89 | (0x80 if g & 1 else 0), (g * 1237 + salt * 811) % 65536 - 32768)


def moflex_frame(codec, s, nc, counts, first=0, tame=False, salt=0):
    """stream s's frame with counts blocks per channel (all equal in Moflex), blocks first.. of every lane's sequence, two zeros appended"""
    out = b"".join(ima_header(s * nc + c, salt) for c in range(nc)) if codec == "ima" else b""
    for k in range(counts):
        for c in range(nc):
            out += lane_blocks(codec, s * nc + c, first + counts, tame)[first + k]
    return out + b"\0\0" if counts or codec == "ima" else b""


def expected(tables, framing, codec, S, nc):
    return [am.Stream(tables, framing, codec, nc) for _ in range(S)]


def check(out, n_samples, rc, rows, want_rc, layout, dtype):
    """rows[s][c] = the model's samples; everything else of `out` must still hold the sentinel"""
    import torch
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


def prefilled(S, nc, ms, layout, dtype, device):
    import torch
    shape = (S, nc, ms) if layout == "planar" else (S, ms, nc)
    fill = SENTINEL if dtype == torch.int16 else SENTINEL / 32768
    return torch.full(shape, fill, dtype=dtype, device=torch.device("cuda", device))


@pytest.mark.parametrize("nblk", [1, 2, 5])
@pytest.mark.parametrize("S,nc", [(1, 1), (3, 2), (65, 2), (22, 3)])
@pytest.mark.parametrize("codec", ["fastaudio", "ima"])
def test_moflex_decode_exact_in_every_layout_and_dtype(tables, codec, S, nc, nblk):
    import torch
    import mobiclipdecoder_amd as m
    for tame in ((False, True) if codec == "fastaudio" else (False,)):
        frames = [moflex_frame(codec, s, nc, nblk, tame=tame) for s in range(S)]
        rows = [st.frame(f)[1] for st, f in zip(expected(tables, "moflex", codec, S, nc), frames)]
        for layout in ("planar", "interleaved"):
            for dtype in (torch.int16, torch.float32):
                a = m.MobiclipAudio(S, nc, codec, "moflex")
                out = prefilled(S, nc, 256 * nblk + 3, layout, dtype, a.device)
                got, ns, rc = a.decode(frames, dtype=dtype, layout=layout, out=out)
                torch.cuda.synchronize()
                assert got is out
                check(out, ns, rc, rows, [0] * S, layout, dtype)
                a.close()


@pytest.mark.parametrize("codec,framing", [("fastaudio", "moflex"), ("fastaudio", "mods"), ("ima", "mods")])
def test_state_carries_five_blocks_equal_two_plus_three(tables, codec, framing):
    import torch
    import mobiclipdecoder_amd as m
    S, nc = 3, 2

    def frame(s, first, count):
        if framing == "moflex":
            return moflex_frame(codec, s, nc, count, first), 0, 0
        body = b"".join((ima_header(s * nc + c) if codec == "ima" and first + k == 0 else b"") + lane_blocks(codec, s * nc + c, first + count)[first + k]
                        for k in range(count) for c in range(nc))
        return bytes(3 + s) + body, 3 + s, count * nc

    one, two = m.MobiclipAudio(S, nc, codec, framing), m.MobiclipAudio(S, nc, codec, framing)
    kw = (lambda fr: dict(offsets=[f[1] for f in fr], n_packets=[f[2] for f in fr])) if framing == "mods" else (lambda fr: {})
    whole = [frame(s, 0, 5) for s in range(S)]
    a, ns, rc = one.decode([f[0] for f in whole], max_samples=1280, **kw(whole))
    first, second = [frame(s, 0, 2) for s in range(S)], [frame(s, 2, 3) for s in range(S)]
    b1, ns1, rc1 = two.decode([f[0] for f in first], max_samples=512, **kw(first))
    b2, ns2, rc2 = two.decode([f[0] for f in second], max_samples=768, **kw(second))
    torch.cuda.synchronize()
    assert ns.tolist() == [[1280] * nc] * S and ns1.tolist() == [[512] * nc] * S and ns2.tolist() == [[768] * nc] * S
    assert torch.equal(a, torch.cat([b1, b2], dim=2))
    model = expected(tables, framing, codec, S, nc)
    rows = [st.frame(f[0], f[1], f[2])[1] for st, f in zip(model, whole)]
    assert torch.equal(a.cpu(), torch.tensor(rows, dtype=torch.int16))


def test_ima_in_moflex_framing_restarts_from_its_headers_every_call(tables):
    import torch
    import mobiclipdecoder_amd as m
    S, nc = 3, 2
    a = m.MobiclipAudio(S, nc, "ima", "moflex")
    for salt in (0, 1, 0):
        frames = [moflex_frame("ima", s, nc, 2, salt=salt) for s in range(S)]
        rows = [st.frame(f)[1] for st, f in zip(expected(tables, "moflex", "ima", S, nc), frames)]  # new model decoders: no carry
        out, ns, rc = a.decode(frames)
        torch.cuda.synchronize()
        assert rc.tolist() == [0] * S and torch.equal(out.cpu(), torch.tensor(rows, dtype=torch.int16))


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
@pytest.mark.parametrize("codec", ["fastaudio", "ima"])
def test_ragged_counts_write_rows_exactly_up_to_their_counts(tables, codec, layout):
    import torch
    import mobiclipdecoder_amd as m
    S, nc = 65, 2
    counts = [(0, 1, 4)[s % 3] for s in range(S)]
    counts[64] = 4
    a, model = m.MobiclipAudio(S, nc, codec, "moflex"), expected(tables, "moflex", codec, S, nc)
    for call in range(2):  # the second call: the lanes that sat out keep their state, the others carry theirs
        frames = [moflex_frame(codec, s, nc, counts[s], first=call * counts[s]) if counts[s] else (None if s % 2 else b"") for s in range(S)]
        rows = [st.frame(f or b"")[1] for st, f in zip(model, frames)]
        out = prefilled(S, nc, 1030, layout, torch.int16, a.device)
        _, ns, rc = a.decode(frames, layout=layout, out=out)
        torch.cuda.synchronize()
        check(out, ns, rc, rows, [0] * S, layout, torch.int16)
        counts = counts[1:] + counts[:1]


def test_reset_of_a_subset_restarts_those_streams_only(tables):
    import torch
    import mobiclipdecoder_amd as m
    S, nc = 65, 2
    a, model = m.MobiclipAudio(S, nc, "fastaudio", "moflex"), expected(tables, "moflex", "fastaudio", S, nc)
    for call in range(3):
        if call == 1:
            a.reset([0, 64])
            model[0].reset(False), model[64].reset(False)
        frames = [moflex_frame("fastaudio", s, nc, 2, first=2 * call) for s in range(S)]
        rows = [st.frame(f)[1] for st, f in zip(model, frames)]
        out, ns, rc = a.decode(frames)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.tensor(rows, dtype=torch.int16)), call
        if call == 1:  # on the device too, a stream that was not reset did not restart: its rows are not a new decoder's
            fresh = am.Stream(tables, "moflex", "fastaudio", nc).frame(frames[1])[1]
            assert not torch.equal(out[1].cpu(), torch.tensor(fresh, dtype=torch.int16))
            assert torch.equal(out[64].cpu(), torch.tensor(am.Stream(tables, "moflex", "fastaudio", nc).frame(frames[64])[1], dtype=torch.int16))


@pytest.mark.parametrize("codec", ["fastaudio", "ima"])
def test_reset_keeps_or_rewinds_the_mods_cursor(tables, codec):
    import torch
    import mobiclipdecoder_amd as m
    S, nc = 3, 2
    a, model = m.MobiclipAudio(S, nc, codec, "mods"), expected(tables, "mods", codec, S, nc)
    used = [[0] * nc for _ in range(S)]

    def packet(s):  # three packets from where the model's cursor and decoders stand
        body, cur = b"", model[s].cursor
        new = [codec == "ima" and not d.init for d in model[s].ima]
        for _ in range(3):
            g = s * nc + cur
            body += (ima_header(g, used[s][cur]) if new[cur] else b"") + lane_blocks(codec, g, used[s][cur] + 1)[used[s][cur]]
            used[s][cur], new[cur], cur = used[s][cur] + 1, False, (cur + 1) % nc
        return bytes(2) + body

    for call in range(3):
        if call == 1:
            a.reset([0], keep_cursor=True), a.reset([1], keep_cursor=False)
            model[0].reset(True), model[1].reset(False)
            assert [st.cursor for st in model] == [1, 0, 1]
        frames = [packet(s) for s in range(S)]
        res = [st.frame(f, 2, 3) for st, f in zip(model, frames)]
        out = prefilled(S, nc, 512, "planar", torch.int16, a.device)
        _, ns, rc = a.decode(frames, offsets=[2] * S, n_packets=[3] * S, out=out)
        torch.cuda.synchronize()
        check(out, ns, rc, [r[1] for r in res], [0] * S, "planar", torch.int16)
        assert sorted(ns[2].tolist()) == [256, 512]
        with pytest.raises(m.MobiclipError):  # unequal counts over the channels: no interleaved output, and nothing changes
            a.decode(frames, offsets=[2] * S, n_packets=[3] * S, layout="interleaved", max_samples=512)


def test_errors_leave_their_streams_untouched_and_the_rest_exact(tables):
    import torch
    import mobiclipdecoder_amd as m
    S, nc = 5, 1
    a, model = m.MobiclipAudio(S, nc, "ima", "mods"), expected(tables, "mods", "ima", S, nc)

    def packet(s, first, count, header):
        return bytes(1) + (header if header else b"") + b"".join(lane_blocks("ima", s, first + count)[first:first + count])

    bad_header = struct.pack("<hh", 89, 100)
    frames = [packet(s, 0, 2, ima_header(s)) for s in range(S)]
    frames[1] = packet(1, 0, 2, bad_header)            # header index 89
    frames[3] = frames[3][:-1]                         # the second block is one byte short
    res = [st.frame(f, 1, 2) for st, f in zip(model, frames)]
    assert [r[0] for r in res] == [0, am.E_INDEX, 0, am.E_INDEX, 0]
    out = prefilled(S, nc, 512, "planar", torch.int16, a.device)
    _, ns, rc = a.decode(frames, offsets=[1] * S, n_packets=[2] * S, out=out)
    torch.cuda.synchronize()
    check(out, ns, rc, [r[1] for r in res], [r[0] for r in res], "planar", torch.int16)
    # a later valid call: the failed streams decode as if the bad frame had never come (their decoders are still new: header again)
    frames = [packet(s, 2, 2, None) for s in range(S)]
    frames[1], frames[3] = packet(1, 0, 2, ima_header(1)), packet(3, 0, 2, ima_header(3))
    res = [st.frame(f, 1, 2) for st, f in zip(model, frames)]
    out = prefilled(S, nc, 512, "planar", torch.int16, a.device)
    _, ns, rc = a.decode(frames, offsets=[1] * S, n_packets=[2] * S, out=out)
    torch.cuda.synchronize()
    check(out, ns, rc, [r[1] for r in res], [0] * S, "planar", torch.int16)
    # FastAudio in Moflex framing: an iteration that starts with fewer than 40 C bytes; the stream keeps its lattice state
    a, model = m.MobiclipAudio(3, 2, "fastaudio", "moflex"), expected(tables, "moflex", "fastaudio", 3, 2)
    for call, cut in enumerate((None, 41, None)):
        frames = [moflex_frame("fastaudio", s, 2, 2, first=2 * call) for s in range(3)]
        if cut:
            frames[1] = frames[1][:80 + cut]
        res = [st.frame(f) for st, f in zip(model, frames)]
        out = prefilled(3, 2, 512, "interleaved", torch.float32, a.device)
        _, ns, rc = a.decode(frames, out=out, layout="interleaved", dtype=torch.float32)
        torch.cuda.synchronize()
        check(out, ns, rc, [r[1] for r in res], [0, am.E_INDEX if cut else 0, 0], "interleaved", torch.float32)


@pytest.mark.parametrize("nc", [1, 2])
def test_pcm16_deinterleaves_with_the_appended_zeros_rule(tables, nc):
    import torch
    import mobiclipdecoder_amd as m
    S = 4
    payload = [am.lcg_bytes(n, 5 + s)[0] for s, n in enumerate((2 * nc * 300, 2 * nc * 7 + 1, 0, 2 * nc * 129 + 2 * nc - 2))]
    frames = [p + b"\0\0" if p else b"" for p in payload]  # the last one: the zeros complete a sample pair for C = 2 and are a sample for C = 1
    rows = [st.frame(f)[1] for st, f in zip(expected(tables, "moflex", "pcm16", S, nc), frames)]
    assert len(rows[3][0]) == 130 and len(rows[0][0]) == 300 + (nc == 1) and rows[2] == [[]] * nc
    a = m.MobiclipAudio(S, nc, "pcm16", "moflex")
    for layout in ("planar", "interleaved"):
        for dtype in (torch.int16, torch.float32):
            out = prefilled(S, nc, 333, layout, dtype, a.device)
            _, ns, rc = a.decode(frames, dtype=dtype, layout=layout, out=out)
            torch.cuda.synchronize()
            check(out, ns, rc, rows, [0] * S, layout, dtype)


def test_decode_is_ordered_on_a_non_default_stream(tables):
    import torch
    import mobiclipdecoder_amd as m
    S, nc = 65, 2
    a = m.MobiclipAudio(S, nc, "fastaudio", "moflex")
    frames = [moflex_frame("fastaudio", s, nc, 2) for s in range(S)]
    rows = [st.frame(f)[1] for st, f in zip(expected(tables, "moflex", "fastaudio", S, nc), frames)]
    side = torch.cuda.Stream(device=a.device)
    with torch.cuda.stream(side):
        out, ns, rc = a.decode(frames, stream=side)
        twice = out.to(torch.int32) * 2 + 1     # enqueued behind the kernel, no host wait in between
    side.synchronize()
    want = torch.tensor(rows, dtype=torch.int32)
    assert torch.equal(twice.cpu(), want * 2 + 1)


def test_python_checks_its_arguments(tables):
    import torch
    import mobiclipdecoder_amd as m
    a = m.MobiclipAudio(2, 2, "fastaudio", "moflex")
    frames = [moflex_frame("fastaudio", s, 2, 1) for s in range(2)]
    for kw in (dict(dtype=torch.float16), dict(layout="nchw"), dict(offsets=[0, 0], n_packets=[1, 1]), dict(max_samples=0),
               dict(out=torch.zeros((2, 2, 256), dtype=torch.int16)), dict(stream=0),
               dict(out=torch.zeros((2, 2, 256), dtype=torch.float32, device="cuda"))):
        with pytest.raises(ValueError):
            a.decode(frames, **kw)
    with pytest.raises(ValueError):
        a.decode(frames[:1])
    with pytest.raises(ValueError):
        a.reset([2])
    with pytest.raises(m.MobiclipError):  # a row longer than max_samples refuses the whole call
        a.decode(frames, max_samples=255)
    out, ns, rc = a.decode(frames)
    torch.cuda.synchronize()
    assert out.shape == (2, 2, 256) and ns.tolist() == [[256, 256]] * 2


# ---- end to end: one small file per container, through the container readers ----
def write_moflex_audio(frames, codec_id, frequency, channels, stream_index=0):
    """synchro header, one MoLiveStreamAudio chunk (type 2: stream, codec, (frequency - 1) u24be, (channels - 1) u8), terminator; one data
    block per frame, flagged EndFrame; 0x1000 zero bytes at the end (the layout of tests/containers.write_moflex)"""
    chunk = bytes([stream_index, codec_id]) + (frequency - 1).to_bytes(3, "big") + bytes([channels - 1])
    out = bytearray(_synchro_header() + _varbyte(2) + _varbyte(len(chunk)) + chunk + _varbyte(0) + _varbyte(0))
    for f in frames:
        assert len(f) <= 0x1000 - 0x80
        out += b"\x01" + _ep(stream_index, bytes(f), True) + _ep(0, None, False)
    return np.frombuffer(bytes(out) + bytes(0x1000), np.uint8).copy()


def write_mods_audio(packets, n_audio, key_frames, audio_codec, channels, frequency=32768):
    """tests/containers.write_mods with the header's audio fields set and a packet count per frame"""
    body, offsets, pos = [], [], 0x30
    for p, n in zip(packets, n_audio):
        offsets.append(pos)
        body.append(struct.pack("<I", (len(p) << 14) | n) + bytes(p))
        pos += 4 + len(p)
    index = b"".join(struct.pack("<II", k, offsets[k]) for k in key_frames)
    header = struct.pack("<4sHHIIIIHHIIIII", b"MODS", 0x0A, 0x0C, len(packets), 256, 192, 0x18000000, audio_codec, channels, frequency,
                         max(len(p) for p in packets), 0, pos, len(key_frames))
    return np.frombuffer(header + b"".join(body) + index, np.uint8).copy()


def test_end_to_end_moflex_fastaudio(tables):
    import torch
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.demux import MoLiveDemux
    nc = 2
    payloads = [moflex_frame("fastaudio", 0, nc, n, first=f)[:-2] for n, f in ((3, 0), (2, 3), (3, 5))]  # the demuxer appends the zeros
    dm = MoLiveDemux(write_moflex_audio(payloads, 0, 32000, nc))
    a, model, n = None, None, 0
    for st, data in dm.frames():
        assert st.chunk_id == 2 and (st.codec_id, st.channel, st.frequency) == (0, nc, 32000)
        assert bytes(data) == payloads[n] + b"\0\0"
        if a is None:
            a, model = m.MobiclipAudio(1, st.channel, st.codec_id, "moflex"), am.Stream(tables, "moflex", "fastaudio", st.channel)
        out, ns, rc = a.decode([data], layout="interleaved")
        torch.cuda.synchronize()
        rows = model.frame(data)[1]
        assert rc.tolist() == [0] and ns.tolist() == [[len(rows[0])] * nc]
        assert torch.equal(out.cpu()[0, :len(rows[0])], torch.tensor(rows, dtype=torch.int16).T)
        n += 1
    assert n == 3


def test_end_to_end_mods_ima_with_a_key_frame_in_the_middle(tables):
    import torch
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.demux import ModsDemuxer
    nc, n_audio, video = 2, [3, 2, 3, 1], [5, 9, 4, 7]
    packets, cur, new, used = [], 0, [True] * nc, [0] * nc
    for f, n in enumerate(n_audio):
        if f == 2:
            new = [True] * nc                    # the key frame: new decoders, the cursor stays
        p = bytes([0x11 * (f + 1)] * video[f])   # stands for the video bits; the video decode would return video[f] + 2
        for _ in range(n):
            p += (ima_header(cur, f) if new[cur] else b"") + lane_blocks("ima", cur, used[cur] + 1)[used[cur]]
            used[cur], new[cur], cur = used[cur] + 1, False, (cur + 1) % nc
        packets.append(p + bytes(3))
    dm = ModsDemuxer(write_mods_audio(packets, n_audio, [0, 2], 3, nc))
    assert (dm.Header.audio_codec, dm.Header.nb_channel) == (3, nc)
    a, model = m.MobiclipAudio(1, dm.Header.nb_channel, dm.Header.audio_codec, "mods"), am.Stream(tables, "mods", "ima", nc)
    for f in range(len(packets)):
        pkt, na, key = dm.ReadFrame()
        assert na == n_audio[f] and key == (f == 2)  # the reader starts behind key frame 0: the next one it announces is the second
        if key:                                  # Program.cs:255-265
            a.reset([0], keep_cursor=True)
            model.reset(True)
        offset = (video[f] + 2) - 2              # Program.cs:250
        out, ns, rc = a.decode([pkt], offsets=[offset], n_packets=[na], max_samples=512)
        torch.cuda.synchronize()
        res = model.frame(pkt, offset, na)
        assert res[0] == 0 and rc.tolist() == [0] and ns.tolist() == [[len(r) for r in res[1]]]
        for c in range(nc):
            assert out.cpu()[0, c, :len(res[1][c])].tolist() == res[1][c]
    assert dm.ReadFrame() is None
