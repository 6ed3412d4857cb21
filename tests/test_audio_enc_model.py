"""The audio encoder without a GPU (include/mobiclip_audio_enc.h; csrc/mobi_audio_enc.h run by tests/tools/mobi_audio_enc_host.cpp, the
host model the kernels are compared against in tests/test_audio_enc_gpu.py).

  1  the C++ host model equals the plain-Python model (tests/audio_enc_model.py) byte for byte -- frames, lengths, reconstruction, stats
     -- on silence, full-scale square waves of period 2 and 64 (the clamp domain), silence that jumps to 32767 at sample 1, -32768 followed
     by noise, uniform noise and a sine of amplitude 12, each with C = 1, 2, 8 and B = 1, 2, 3; slots and sample rows at a pitch above
     their length, bytes behind a frame untouched
  2  the decoder model (tests/audio_model.py), fed a frame plus the two zero bytes the demuxer appends through mobi_audio_plan, returns
     exactly B * 256 samples per channel, equal to the reported reconstruction (PCM16 with one channel: one more sample, 0)
  3  a brute force over the 89 indices confirms every header's index and its tie rule; over the 16 nibbles, on 200 seeded states, the
     nibble and its tie rule; the case where the nearest candidate has the other sign
  4  header, library and the binding's table name the same symbols
  5  every refusal, each by the smallest input that raises it
  6  the host model under sanitizers, as a program of its own, over heap buffers of exactly the needed size"""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import audio_enc_model as A
from tests import audio_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tests", "tools")
CSRC = os.path.join(ROOT, "mobiclipdecoder_amd", "csrc")
NAMES = ["mobi_audio_enc_async", "mobi_audio_enc_check", "mobi_audio_enc_create", "mobi_audio_enc_destroy", "mobi_audio_enc_frame_bytes"]
SHAPES = [(nc, B) for nc in (1, 2, 8) for B in (1, 2, 3)]


@pytest.mark.parametrize("name", A.SIGNALS)
def test_host_model_equals_the_python_model(name):
    for nc, B in SHAPES:
        x = A.signal(name, nc, B)[None]
        for codec in (A.IMA, A.PCM16):
            frames, rec, stats = A.encode_batch(codec, x)
            rc, slots, sizes, h_rec, h_stats = A.run_host(codec, x, pitch_extra=64, slot_extra=64)
            assert rc == 0 and int(sizes[0]) == len(frames[0]) == A.frame_bytes(codec, nc, B) == A.host().aenc_host_frame_bytes(codec, nc, B)
            assert slots[0, :len(frames[0])].tobytes() == frames[0], (name, nc, B, codec)
            assert (slots[0, len(frames[0]):] == A.FILL).all()
            assert np.array_equal(h_rec, rec) and np.array_equal(h_stats, stats), (name, nc, B, codec)
            # without recon and stats: the same frames
            rc, s2, z2, _, _ = A.run_host(codec, x, pitch_extra=64, slot_extra=64, recon=False, stats=False)
            assert rc == 0 and np.array_equal(s2, slots) and np.array_equal(z2, sizes)


def test_the_signals_reach_what_they_are_for():
    def st(name):  # the host tool's stats, which test 1 holds to the model's
        rc, _, _, _, stats = A.run_host(A.IMA, A.signal(name, 2, 2)[None])
        assert rc == 0
        return stats
    assert st("square2")["clamped"].min() > 0 and st("square64")["clamped"].min() > 0  # the clamp domain
    assert (st("silence")["sse"] == 0).all() and (st("silence")["start_index"] == 0).all() and (st("silence")["clamped"] == 0).all()
    assert (st("sine12")["start_index"] <= 8).all()
    assert st("jump")["start_index"].min() > 40  # a header that pays: the step must reach 32767 at once
    assert A.signal("neg_noise", 8, 1)[:, 0].tolist() == [-32768] * 8
    # with C = 8 a swap of any two channels must show: the noise has eight different channels, the sine eight phases
    for name in ("noise", "sine12"):
        assert len({A.signal(name, 8, 1)[c].tobytes() for c in range(8)}) == 8
    # over its seven offsets a batch gives every stream position every signal (tests/test_audio_enc_gpu.py runs all seven)
    assert all(np.array_equal(A.batch(1, 2, 1, offset=o)[0], A.signal(A.SIGNALS[o], 2, 1)) for o in range(7))


@pytest.mark.parametrize("codec", ("ima", "pcm16"))
def test_the_decoder_model_returns_the_reconstruction(codec):
    from mobiclipdecoder_amd import audio
    t = audio.tables()
    cid = A.IMA if codec == "ima" else A.PCM16
    for name in A.SIGNALS:
        for nc, B in SHAPES:
            # the frames and the reconstruction the C++ host tool reports (test 1 holds them to the model's)
            rc0, slots, sizes, h_rec, _ = A.run_host(cid, A.signal(name, nc, B)[None])
            assert rc0 == 0 and int(sizes[0]) == A.frame_bytes(cid, nc, B)
            frame, rec = slots[0, :int(sizes[0])].tobytes(), h_rec[0]
            data = frame + b"\x00\x00"
            rc, blocks, ns, _ = audio.plan("moflex", codec, nc, data)
            assert rc == 0
            rc2, rows = audio_model.Stream(t, "moflex", codec, nc).frame(data)
            assert rc2 == 0
            if codec == "pcm16" and nc == 1:  # the appended zero bytes are one more sample: documented, not worked round
                assert ns.tolist() == [256 * B + 1] and rows[0][-1] == 0
                rows = [rows[0][:-1]]
            else:
                assert ns.tolist() == [256 * B] * nc and len(blocks) == (B * nc if codec == "ima" else 0)
            assert np.array_equal(np.array(rows), rec), (name, nc, B)
            if codec == "ima":  # the plan finds the blocks where the frame's layout puts them
                assert [(b[0], b[1]) for b in blocks] == [(4 * nc + 128 * (b * nc + c), c) for b in range(B) for c in range(nc)]


def test_brute_force_confirms_index_and_nibble():
    lib = A.host()
    # every frame of test 1: the header's index is the first least E over the 89, by the host's own trial function and the model's
    seen = set()
    for name in A.SIGNALS:
        x = A.signal(name, 8, 1)
        _, _, stats = A.encode_frame(A.IMA, x)
        for c in range(8):
            blk = np.ascontiguousarray(x[c, :256])
            if blk.tobytes() in seen:
                continue
            seen.add(blk.tobytes())
            errs = [int(lib.aenc_host_trial(blk.ctypes.data, 256, i0)) for i0 in range(89)]
            assert errs == A.trial_errors([int(v) for v in blk])
            assert int(stats["start_index"][c]) == errs.index(min(errs)), (name, c)
    # silence ties on all 89 indices below some step? the first wins
    assert A.encode_frame(A.IMA, A.signal("silence", 1, 1))[2]["start_index"][0] == 0
    # 200 seeded states: the nibble is the first of the nearest candidates
    rng = np.random.default_rng(4242)
    ties = 0
    for i in range(200):
        index = int(rng.integers(0, 89))
        last = int(rng.choice([-32768, 32767, int(rng.integers(-32768, 32768))]))
        x = int(rng.choice([last, -32768, 32767, int(np.clip(last + rng.integers(-300, 300), -32768, 32767)), int(rng.integers(-32768, 32768))]))
        d = [abs(x - A.decode_step(v, last, index)[0]) for v in range(16)]
        want = d.index(min(d))
        ties += d.count(min(d)) > 1
        assert lib.aenc_host_nibble(x, last, index) == want == A.nibble(x, last, index), (x, last, index)
    assert ties > 20  # the tie rule was exercised
    # at the clamp the nearest candidate may carry the other sign: last = x = -32768, a step of 41 (step / 8 = 5)
    assert A.nibble(-32768, -32768, 18) == 8 == lib.aenc_host_nibble(-32768, -32768, 18) and A.decode_step(0, -32768, 18)[0] == -32763


def test_header_library_and_binding_agree():
    from mobiclipdecoder_amd import audio_enc, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobiclip_audio_enc.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mobi_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(audio_enc._SIGS) == NAMES
    assert set(names) <= set(build.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(names) <= exported
    # nothing else new: what leaves the library is what the headers declare, and the audio encoder's part of it is these names
    assert exported == set(build.header_symbols()) and sorted(n for n in exported if n.startswith("mobi_audio_enc")) == NAMES
    lib = audio_enc._lib()
    for name, (res, args) in audio_enc._SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == list(args), name
        proto = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(proto.split(",")) == len(args), name
    import mobiclipdecoder_amd
    assert mobiclipdecoder_amd.MobiclipAudioEncoder is audio_enc.MobiclipAudioEncoder


def test_refusals():
    """each by the smallest input that raises it: one step back and the call is accepted"""
    from mobiclipdecoder_amd import audio_enc
    lib = audio_enc._lib()
    x = np.zeros(2 * 2 * 512 + 8, np.int16)
    slots = np.zeros(4096, np.uint8)
    sizes = np.zeros(4, np.int32)
    rec = np.zeros(2 * 2 * 512 + 8, np.int16)
    st = np.zeros(8, A.STATS_DTYPE)
    frame = A.frame_bytes(A.IMA, 2, 2)
    assert frame == 520 and lib.mobi_audio_enc_frame_bytes(A.IMA, 2, 2) == 520 and lib.mobi_audio_enc_frame_bytes(A.PCM16, 2, 2) == 2048
    base = dict(codec=A.IMA, n_streams=2, nc=2, max_blocks=2, n=2, samples=x.ctypes.data, pitch=512, blocks=2, slots=slots.ctypes.data, slot_pitch=frame,
                slot_bytes=frame, sizes=sizes.ctypes.data, recon=rec.ctypes.data, recon_pitch=512, stats=st.ctypes.data)

    def both(**kw):
        a = dict(base, **kw)
        args = (a["codec"], a["n_streams"], a["nc"], a["max_blocks"], a["n"], a["samples"], a["pitch"], a["blocks"], a["slots"], a["slot_pitch"], a["slot_bytes"],
                a["sizes"], a["recon"], a["recon_pitch"], a["stats"])
        r1, r2 = lib.mobi_audio_enc_check(*args), A.host().aenc_host_check(*args)
        assert r1 == r2
        return r1
    assert both() == 0 and both(recon=None, stats=None, recon_pitch=0) == 0
    assert both(codec=A.FASTAUDIO) == A.E_UNSUPPORTED and both(codec=A.SX) == A.E_UNSUPPORTED and both(codec=4) == A.E_ARG and both(codec=-1) == A.E_ARG
    assert both(codec=A.PCM16, slot_bytes=2048, slot_pitch=2048) == 0 and both(codec=A.PCM16, slot_bytes=2044, slot_pitch=2048) == A.E_ARG
    for key in ("samples", "slots", "sizes"):
        assert both(**{key: None}) == A.E_ARG
    assert both(samples=x.ctypes.data + 1) == A.E_ARG and both(samples=x.ctypes.data + 2) == 0
    assert both(slots=slots.ctypes.data + 2) == A.E_ARG and both(slots=slots.ctypes.data + 4) == 0
    assert both(sizes=sizes.ctypes.data + 2) == A.E_ARG and both(sizes=sizes.ctypes.data + 4) == 0
    assert both(recon=rec.ctypes.data + 1) == A.E_ARG and both(recon=rec.ctypes.data + 2) == 0
    assert both(stats=st.ctypes.data + 4) == A.E_ARG and both(stats=st.ctypes.data + 8) == 0
    assert both(n=0) == A.E_ARG and both(n=1) == 0 and both(n=3) == A.E_ARG
    assert both(blocks=0) == A.E_ARG and both(blocks=1) == 0 and both(blocks=3) == A.E_ARG and both(blocks=3, max_blocks=3, pitch=768, recon_pitch=768,
                                                                                                  slot_bytes=776, slot_pitch=776) == 0
    assert both(pitch=511) == A.E_ARG and both(recon_pitch=511) == A.E_ARG and both(recon_pitch=511, recon=None) == 0
    assert both(slot_bytes=frame - 4) == A.E_ARG and both(slot_bytes=frame + 2, slot_pitch=frame + 4) == A.E_ARG and both(slot_bytes=frame + 4, slot_pitch=frame + 4) == 0
    assert both(slot_pitch=frame - 4) == A.E_ARG and both(slot_pitch=frame + 2) == A.E_ARG
    assert both(nc=0) == A.E_ARG and both(nc=9) == A.E_ARG and both(nc=8, slot_bytes=2080, slot_pitch=2080) == 0 and both(nc=1) == 0
    assert both(n_streams=0) == A.E_ARG and both(max_blocks=0) == A.E_ARG and both(max_blocks=65536) == A.E_ARG and both(max_blocks=65535) == 0
    assert both(n_streams=(1 << 24) // 2) == A.E_ARG and both(n_streams=(1 << 24) // 2 - 1) == 0
    # the entry points themselves, without an object
    assert lib.mobi_audio_enc_async(None, None, 1, x.ctypes.data, 512, 1, slots.ctypes.data, frame, frame, sizes.ctypes.data, None, 0, None) == A.E_ARG
    for args in ((0, A.FASTAUDIO, 1, 1, 1), (0, A.SX, 1, 1, 1), (0, A.IMA, 1, 0, 1), (0, A.IMA, 1, 9, 1), (0, A.IMA, 0, 1, 1), (0, A.IMA, 1, 1, 0)):
        assert not lib.mobi_audio_enc_create(*args), args
    assert lib.mobi_audio_enc_frame_bytes(A.FASTAUDIO, 2, 2) == 0 and lib.mobi_audio_enc_frame_bytes(A.IMA, 9, 2) == 0 and lib.mobi_audio_enc_frame_bytes(A.IMA, 2, 0) == 0
    # the Python class refuses the same before it asks for a device
    import mobiclipdecoder_amd as m
    for codec in ("fastaudio", "sx", 0, 3):
        with pytest.raises(m.MobiclipError, match="no encoder"):
            m.MobiclipAudioEncoder(1, 1, codec, 1)
    for args in ((1, 0, "ima", 1), (1, 9, "ima", 1), (0, 1, "ima", 1), (1, 1, "ima", 0), (1, 1, "mp3", 1)):
        with pytest.raises(ValueError):
            m.MobiclipAudioEncoder(*args)
    # the host model refuses as the entry point does, and writes nothing
    rc, slots2, sizes2, _, _ = A.run_host(A.FASTAUDIO, A.signal("noise", 1, 1)[None])
    assert rc == A.E_UNSUPPORTED and (slots2 == A.FILL).all() and (sizes2 == -1).all()


def test_host_model_under_sanitizers(tmp_path):
    """tests/tools/audio_enc_host_main.cpp: a program of its own with -fsanitize=address,undefined, linked statically (nothing sanitised
    is loaded into Python): the encode rule and the audio mux over heap buffers of exactly the needed size"""
    exe = str(tmp_path / "audio_enc_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(TOOLS, "audio_enc_host_main.cpp"), os.path.join(TOOLS, "mobi_audio_enc_host.cpp"),
                    os.path.join(TOOLS, "mobi_mux_audio_host.cpp"), "-o", exe], check=True)
    for codec, nc, B in ((A.IMA, 2, 2), (A.IMA, 8, 1), (A.PCM16, 1, 3)):
        x = A.batch(3, nc, B)
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        x.tofile(src)
        p = subprocess.run([exe, str(codec), "3", str(nc), str(B), src, dst], capture_output=True, text=True)
        assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
        rc, slots, sizes, rec, st = A.run_host(codec, x)
        frame = int(sizes[0])
        blob = np.fromfile(dst, np.uint8)
        n_f, n_r, n_s = 3 * frame, x.size * 2, 3 * nc * 16
        assert blob[:n_f].tobytes() == b"".join(slots[s, :frame].tobytes() for s in range(3))
        assert blob[n_f:n_f + n_r].tobytes() == rec.tobytes() and blob[n_f + n_r:n_f + n_r + n_s].tobytes() == st.tobytes()
        # behind them: the Moflex file of clip 0 with these frames as its audio stream, read back
        from mobiclipdecoder_amd.demux import MoLiveDemux
        d = MoLiveDemux(blob[n_f + n_r + n_s:].copy())
        got = [(s.chunk_id, bytes(f[:-2])) for s, f in d.frames()]
        d.close()
        assert got == [(2, slots[s, :frame].tobytes()) for s in range(3)]
