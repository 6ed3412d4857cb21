"""CPU: Sx audio (include/mobiclip_sx.h) against the model written from SxDecoder.cs in plain Python integers (sx_model.py): the recorded
checksums, the host build of the arithmetic header (tests/tools/libmobi_sx_host.so) packet by packet in samples AND state, mobi_sx_plan
against the model's framing, the ABI and the Python layer, and a stand-alone sanitizer build run as a child process.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sx_model as sm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INDEX, E_ARG = -1, -7  # include/mobiclip_hip.h
CASE_IDS = [f"seed{s}-{'tame' if t else 'wild'}" for s, t in sm.CASES]
WILD_CLAMPS = {1: 9233, 2: 9197}  # of 12288 samples


@pytest.mark.parametrize("seed,tame", list(sm.CASES), ids=CASE_IDS)
def test_model_reproduces_the_recorded_rows(seed, tame):
    c, (crc, consumed, rates) = sm.case(seed, tame), sm.CASES[(seed, tame)]
    assert (c.consumed, tuple(c.rates)) == (consumed, rates)
    assert f"{c.crc:08x}" == f"{crc:08x}"
    if tame:  # a condition on the inputs: no operation leaves int32, no sample clamps
        assert (c.wraps, c.clamps) == (0, 0)
        assert 1000 < max(abs(v) for s in c.samples for v in s) < 6000
    else:
        assert c.wraps > 100000 and c.clamps == WILD_CLAMPS[seed]
    # the reset packets sit behind an odd and behind an even number of packets: both parities of Internal[0x64] meet one
    before = {c.states[b - 1][0x64 >> 2] for b in range(1, sm.N_CASE_PACKETS) if b % 33 in (0, 16)}
    assert before == {0, 1}


def _host():
    from mobiclipdecoder_amd import build
    lib = C.CDLL(build.LIB_SXHOST)
    lib.mobi_sx_host_packet.restype, lib.mobi_sx_host_packet.argtypes = C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("seed,tame", list(sm.CASES), ids=CASE_IDS)
def test_arithmetic_header_on_the_host_equals_the_model_in_samples_and_state(seed, tame):
    """Every word of Internal after every packet, but the two that hold no state: 0x68 (the packet's rows and rate) and 0x6C (the
    output cursor) are written before they are read in every packet."""
    lib, c = _host(), sm.case(seed, tame)
    internal, out = np.zeros(sm.INTERNAL_WORDS, np.int32), np.zeros(128, np.int16)
    keep = np.ones(sm.INTERNAL_WORDS, bool)
    keep[list(sm.SCRATCH_WORDS)] = False
    for b in range(sm.N_CASE_PACKETS):
        pkt = c.data[c.offsets[b]:c.offsets[b + 1]]
        assert lib.mobi_sx_host_packet(internal.ctypes.data, c.cb, pkt, out.ctypes.data) == len(pkt), b
        assert out.tolist() == c.samples[b], b
        want = np.array(c.states[b], np.int32)
        diff = np.nonzero((internal != want) & keep)[0]
        assert diff.size == 0, (b, [hex(4 * int(i)) for i in diff[:8]])


def test_a_new_decoder_decodes_a_packet_that_is_no_reset_from_zeros():
    lib, c = _host(), sm.case(1, True)
    pkt = c.data[c.offsets[1]:c.offsets[2]]
    assert pkt[1] >> 1 != 0x7F
    want, _ = sm.Sx(c.cb).decode(pkt, 0)
    internal, out = np.zeros(sm.INTERNAL_WORDS, np.int32), np.full(128, 7, np.int16)
    lib.mobi_sx_host_packet(internal.ctypes.data, c.cb, pkt, out.ctypes.data)
    assert want == [0] * 128 and out.tolist() == want and internal[0x64 >> 2] == 1


# ---- framing ----
def packet(rate, fill=0x5A, reset=False):
    n = sm.PACKET_BYTES[rate]
    return bytes([fill, 0xFE if reset else 0x12, fill, (fill & 0xCF) | rate << 4]) + bytes([fill] * (n - 4))


@pytest.mark.parametrize("nc", [2, 3])
def test_plan_deals_packets_round_robin_and_carries_the_cursor(nc):
    from mobiclipdecoder_amd import audio
    rates = [0, 3, 1, 2, 2, 0, 1, 3, 3, 1, 0]
    cursor = 0
    for frame, count in enumerate((5, 4, 1, 0, 7)):  # 5, 1 and 7 are multiples of neither channel count
        lead = 3 + frame
        data = bytes(lead) + b"".join(packet(rates[(frame + i) % len(rates)], 0x11 * (i + 1)) for i in range(count)) + bytes(2)
        want, per, want_cur = sm.plan(nc, data, lead, count, cursor)
        rc, got, ns, cur = audio.sx_plan(nc, data, lead, count, cursor)
        assert rc == 0 and got == want and ns.tolist() == per and cur == want_cur
        assert sum(per) == 128 * count and cur == (cursor + count) % nc
        cursor = cur
    assert cursor == (5 + 4 + 1 + 7) % nc


@pytest.mark.parametrize("rate", [0, 1, 2, 3])
def test_plan_every_packet_size_fitting_exactly_and_one_byte_short(rate):
    from mobiclipdecoder_amd import audio
    data = bytes(6) + packet(1) + packet(rate)
    assert len(packet(rate)) == (20, 14, 12, 10)[rate]
    rc, got, ns, cur = audio.sx_plan(2, data, 6, 2, 1)
    assert rc == 0 and got == [(6, 1), (20, 0)] and ns.tolist() == [128, 128] and cur == 1
    assert sm.plan(2, data, 6, 2, 1) == (got, [128, 128], 1)
    short = data[:-1]
    with pytest.raises(sm.OutOfData):
        sm.plan(2, short, 6, 2, 1)
    rc, got, ns, cur = audio.sx_plan(2, short, 6, 2, 1)
    assert rc == E_INDEX and got == [] and ns.tolist() == [0, 0] and cur == 1  # counts zero, the cursor unchanged
    assert audio.sx_plan(2, short, 6, 1, 1)[0] == 0                            # the first packet alone still fits


def test_plan_fewer_than_four_bytes_at_a_packets_start():
    from mobiclipdecoder_amd import audio
    data = packet(3) + packet(3)[:3]
    for n in (0, 1, 2, 3):
        d = packet(3) + packet(3)[:n]
        with pytest.raises(sm.OutOfData):
            sm.plan(1, d, 0, 2, 0)
        assert audio.sx_plan(1, d, 0, 2, 0)[0] == E_INDEX, n
    rc, got, ns, cur = audio.sx_plan(3, data, len(data) + 5, 1, 2)             # an offset behind the end
    assert (rc, got, ns.tolist(), cur) == (E_INDEX, [], [0, 0, 0], 2)
    rc, got, ns, cur = audio.sx_plan(3, data, 0, 0, 2)
    assert (rc, got, ns.tolist(), cur) == (0, [], [0, 0, 0], 2)                # nothing asked: nothing
    assert audio.sx_plan(3, b"", 0, 4, 2)[0] == 0                             # an empty buffer: the stream sits out


def test_plan_checks_its_arguments():
    from mobiclipdecoder_amd import audio
    lib = audio._lib()
    data = packet(2)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    n, ns, blocks = C.c_size_t(), (C.c_int32 * 8)(), (audio.AudioBlock * 4)()

    def call(nc=2, ptr=buf, size=len(data), cursor=0, bl=blocks, mb=4, pn=C.byref(n), pns=ns, no_cursor=False):
        cur = C.c_int(cursor)
        return lib.mobi_sx_plan(nc, C.addressof(ptr) if ptr is not None else None, size, 0, 1, None if no_cursor else C.byref(cur), bl, mb, pn, pns)

    assert call() == 0 and n.value == 1 and (blocks[0].offset, blocks[0].channel, blocks[0].header) == (0, 0, 0)
    for kw in (dict(nc=0), dict(nc=9), dict(cursor=-1), dict(cursor=2), dict(no_cursor=True), dict(ptr=None), dict(bl=None), dict(pn=None),
               dict(pns=None)):
        assert call(**kw) == E_ARG, kw
    assert call(ptr=None, size=0) == 0 and call(bl=None, mb=0) == 0
    with pytest.raises(ValueError):
        audio.sx_plan(9, data)


# ---- ABI and Python ----
def test_sx_header_symbols_are_exported_and_bound():
    from mobiclipdecoder_amd import audio, build, decoder
    lib = decoder.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobiclip_sx.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mobi_[a-z0-9_]+)\s*\(", src)))
    assert names == ["mobi_sx_create", "mobi_sx_plan", "mobi_sx_reset"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/mobiclip_sx.h but not exported"
    assert set(audio._SX_SIGS) == set(names) and set(names) <= set(build.header_symbols())
    assert sorted(audio._SIGS) == ["mobi_audio_create", "mobi_audio_decode", "mobi_audio_destroy", "mobi_audio_plan", "mobi_audio_reset",
                                   "mobi_audio_table"]
    assert not set(audio._SX_SIGS) & (set(audio._SIGS) | set(decoder._SIGS))


def test_the_old_entry_points_still_refuse_sx():
    from mobiclipdecoder_amd import audio
    assert audio.plan("mods", "sx", 2, bytes(400), 0, 2)[0] == audio.MOBI_E_UNSUPPORTED
    assert not audio._lib().mobi_audio_create(0, 1, audio.CODECS["sx"], 1, 1)
    assert not audio._lib().mobi_sx_create(0, 1, 1, None)


@pytest.mark.parametrize("with_audio", [True, False])
def test_demuxer_hands_out_the_codebooks(with_audio):
    from mobiclipdecoder_amd.demux import ModsDemuxer
    books = [bytes((7 * i + c) & 0xFF for i in range(sm.CODEBOOK_BYTES)) for c in range(2)]
    dm = ModsDemuxer(sm.write_mods([bytes(12), bytes(9)], [2, 1], [0], 2, books if with_audio else None))
    assert (dm.Header.audio_codec, dm.Header.nb_channel, dm.Header.audio_offset != 0) == (1, 2, with_audio)
    assert dm.AudioCodebooks == (books if with_audio else None)
    assert dm.ReadFrame()[1] == 2 and dm.ReadFrame()[1] == 1 and dm.ReadFrame() is None


def test_constructor_checks_the_codebooks_before_the_library():
    import mobiclipdecoder_amd as m
    cb = bytes(sm.CODEBOOK_BYTES)
    for books in ([[cb, cb]], [[cb], [cb]], [[cb, cb], [cb, cb[:-1]]], [[cb, cb], [cb, cb + b"\0"]], [[cb, cb], [cb, None]], 5,
                  [[cb, cb], [cb, "text"]], [[cb, cb], [cb, cb], [cb, cb]]):
        with pytest.raises(ValueError):
            m.MobiclipAudio(2, 2, "sx", "mods", codebooks=books)
    with pytest.raises(ValueError):
        m.MobiclipAudio(2, 2, 1, "moflex", codebooks=[[cb, cb]] * 2)   # codec number 1 is IMA there
    with pytest.raises(ValueError):
        m.MobiclipAudio(2, 2, "sx", "moflex", codebooks=[[cb, cb]] * 2)
    with pytest.raises(ValueError):
        m.MobiclipAudio(2, 2, "fastaudio", "mods", codebooks=[[cb, cb]] * 2)
    with pytest.raises(m.MobiclipError, match="codebooks"):
        m.MobiclipAudio(2, 2, "sx", "mods")
    with pytest.raises(m.MobiclipError, match="codebooks"):
        m.MobiclipAudio(2, 2, 1, "mods")


def test_create_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import mobiclipdecoder_amd as m
    cb = bytes(sm.CODEBOOK_BYTES)
    with pytest.raises(m.MobiclipError):
        m.MobiclipAudio(2, 2, "sx", "mods", codebooks=[[cb, cb]] * 2)


# ---- sanitizers, on a stand-alone program ----
def test_stand_alone_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    """The same host sources (the arithmetic header through the test tool, mobi_sx_plan) with their own main: the four recorded cases,
    every packet from an exactly-sized heap copy, and mobi_sx_plan swept over exactly-sized heap copies.  A child process; nothing of it
    is loaded here."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "sx_host_san")
    csrc = os.path.join(ROOT, "mobiclipdecoder_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-DMOBI_SX_HOST_MAIN",
                           "-I" + csrc, os.path.join(ROOT, "tests", "tools", "mobi_sx_host.cpp"), os.path.join(csrc, "mobi_audio_plan.cpp"),
                           "-o", exe])
    files = []
    for seed, tame in sm.CASES:
        c = sm.case(seed, tame)
        files.append(str(tmp_path / f"case_{seed}_{int(tame)}.bin"))
        with open(files[-1], "wb") as f:
            f.write(c.cb + c.data)
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if " crc " in ln]
    assert len(lines) == len(sm.CASES)
    for ln, ((seed, tame), (crc, consumed, _)) in zip(lines, sm.CASES.items()):
        assert ln.endswith(f"packets {sm.N_CASE_PACKETS} bytes {consumed} crc {crc:08x}"), ln
    assert r.stdout.count("plan calls") == len(sm.CASES)
