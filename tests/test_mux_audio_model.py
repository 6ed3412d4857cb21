"""The muxer's audio stream without a GPU (include/mobiclip_mux_audio.h; csrc/mobi_mux.h run by tests/tools/mobi_mux_audio_host.cpp, the host
model the kernels are compared against in tests/test_mux_audio_gpu.py).

  1  images of video and audio frames equal the restated writer (tests/mux_audio_model.py, on tests/containers.py's _ep, _varbyte and
     _synchro_header) byte for byte, frames in the order of the append calls, audio frames of 1, 2, 17, 3967, 3968, 3969, 7936 and 7937
     random bytes
  2  MoLiveDemux returns the video frames (chunk id 1) and the audio frames (chunk id 2) in append order, with the audio chunk's codec,
     frequency and channel count
  3  mobi_mux_fixed_bytes_audio plus the framed bytes add up to the file length
  4  with audio off the image, and its 30-byte head, are what the video-only model (tests/tools/mobi_mux_host.cpp, as it was) writes
  5  _STREAM and _CAPACITY are raised by an audio frame at the smallest input that raises them; the row is untouched behind the refusal
     and the other clips are exact
  6  header, library and the binding's table agree; the refusals that need no device"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import containers
from tests import mux_audio_model as MA
from tests import mux_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mobi_mux_append_audio_async", "mobi_mux_fixed_bytes_audio", "mobi_mux_set_audio"]
MOBI_E_ARG, MOBI_E_UNSUPPORTED = -7, -6


def _clean():
    sizes, slots, kinds = MA.session()
    return sizes, slots, kinds, max(MA.ends(sizes, slots, kinds)) + 0x1000, [(0, None)] * MA.N


def test_model_equals_the_restated_writer():
    case = _clean()
    sizes, _, kinds = case[:3]
    for c in range(MA.N):
        assert sorted(int(v) for v in sizes[kinds == 1, c]) == sorted(MA.AUDIO_LENS)
    rc, files, ln, st = MA.run_host(*case[:4])
    assert rc == 0
    MA.check_session(case, files, ln, st)
    # the one bit that differs: an audio frame's last block starts F2 00 00 00, a video frame's B2 00 00 00; a block that does not end
    # the frame C0 | len >> 8 against 80 | len >> 8
    assert MA.frame(1, bytes(5))[:6] == bytes([1, 0xF2, 0, 0, 0, 0]) and MA.frame(0, bytes(5))[:6] == bytes([1, 0xB2, 0, 0, 0, 0])
    assert MA.frame(1, bytes(5000))[:3] == bytes([1, 0xC0 | 0xF7F >> 8, 0x7F]) and MA.frame(0, bytes(5000))[:3] == bytes([1, 0x80 | 0xF7F >> 8, 0x7F])
    assert MA.frame(0, bytes(5000)) == bytes(containers.write_moflex([bytes(5000)], 16, 16))[30:-0x1000]
    for codec, freq, ch in ((0, 1, 1), (2, 1 << 24, 8), (1, 44100, 2)):
        rc, files, ln, st = MA.run_host(*case[:4], audio=(codec, freq, ch))
        assert rc == 0 and not st.any()
        assert files[0, :int(ln[0])].tobytes() == MA.reference(*case[:3], 0, audio=(codec, freq, ch)).tobytes()
        assert files[0, 28:38].tobytes() == bytes([2, 6, 1, codec]) + (freq - 1).to_bytes(3, "big") + bytes([ch - 1, 0, 0])


def test_files_read_back():
    from mobiclipdecoder_amd.demux import MoLiveDemux
    case = _clean()
    sizes, slots, kinds = case[:3]
    _, files, ln, _ = MA.run_host(*case[:4])
    for c in range(MA.N):
        d = MoLiveDemux(files[c, :int(ln[c])].copy())
        got = list(d.frames())
        d.close()
        want = MA.frames_of(sizes, slots, kinds, c)
        assert [(s.chunk_id, s.stream_index, bytes(f)) for s, f in got] == [(1 + k, k, f + b"\x00\x00") for k, f in want]
        audio = next(s for s, _ in got if s.chunk_id == 2)
        assert (audio.codec_id, audio.frequency, audio.channel) == MA.AUDIO
        video = got[0][0]
        assert (video.fps_rate, video.fps_scale, video.width, video.height) == (M.FPS[0], M.FPS[1], M.W, M.H)


def test_fixed_and_framed_bytes_add_up():
    from mobiclipdecoder_amd import mux
    sizes, slots, kinds, capacity, _ = _clean()
    _, _, ln, _ = MA.run_host(sizes, slots, kinds, capacity)
    lib = mux._lib()
    assert mux.fixed_bytes("moflex", 0, audio=True) == lib.mobi_mux_fixed_bytes_audio(0, 0, 1) == MA.host().mux_host_fixed_bytes_audio(0, 0, 1) == 38 + 0x1000
    assert lib.mobi_mux_fixed_bytes_audio(0, 3, 0) == mux.fixed_bytes("moflex", 3) == 30 + 0x1000 and lib.mobi_mux_fixed_bytes_audio(1, 3, 0) == mux.fixed_bytes("mods", 3)
    assert lib.mobi_mux_fixed_bytes_audio(1, 3, 1) == 0 and lib.mobi_mux_fixed_bytes_audio(2, 0, 1) == 0 and lib.mobi_mux_fixed_bytes_audio(0, -1, 1) == 0
    with pytest.raises(ValueError):
        mux.fixed_bytes("mods", 0, audio=True)
    for c in range(MA.N):
        assert mux.fixed_bytes("moflex", 0, audio=True) + sum(mux.framed_bytes("moflex", int(v)) for v in sizes[:, c]) == int(ln[c])
    for L in MA.AUDIO_LENS:  # one closed form for both streams
        assert len(MA.frame(1, bytes(L))) == len(MA.frame(0, bytes(L))) == mux.framed_bytes("moflex", L)


def test_audio_off_is_the_parents_image():
    sizes, slots, keys = M.clips(M.MOFLEX)
    capacity = M.capacity_of(M.MOFLEX, sizes, keys)
    rc0, f0, l0, s0 = M.run_host(M.MOFLEX, sizes, slots, keys, capacity, 0)
    for kinds in (None, np.zeros(sizes.shape[0], np.uint8)):
        rc, f1, l1, s1 = MA.run_host(sizes, slots, kinds, capacity, audio=None)
        assert rc == rc0 == 0 and np.array_equal(f0, f1) and np.array_equal(l0, l1) and np.array_equal(s0, s1)
    assert f0[0, :30].tobytes() == MA.head(M.W, M.H, M.FPS[0], M.FPS[1], None) == bytes(containers.write_moflex([], M.W, M.H, *M.FPS[:2]))[:30]
    for c in range(M.N):
        assert np.array_equal(f0[c, :l0[c]], M.reference(M.MOFLEX, sizes, slots, keys, c))
    # video frames alone in a file with an audio stream: only the head differs
    rc, f2, l2, s2 = MA.run_host(sizes, slots, None, capacity + 8)
    assert rc == 0 and not s2.any() and np.array_equal(l2, l0 + 8)
    assert np.array_equal(f2[0, 38:l2[0]], f0[0, 30:l0[0]]) and np.array_equal(f2[0, :28], f0[0, :28])
    # an audio frame without an audio stream, a Mods session with one: refused by the model as by the entry points
    sizes, slots, kinds = MA.session()
    assert MA.run_host(sizes, slots, kinds, 100000, audio=None)[0] == MOBI_E_ARG
    assert MA.run_host(sizes, slots, kinds, 100000, container=M.MODS)[0] == MOBI_E_UNSUPPORTED
    for bad in ((3, 32000, 2), (1, (1 << 24) + 1, 2), (1, 32000, 9), (-1, 32000, 2)):
        assert MA.run_host(sizes, slots, kinds, 100000, audio=bad)[0] == MOBI_E_ARG, bad


@pytest.mark.parametrize("name", sorted(MA.status_cases()))
def test_status_bits_from_audio_frames(name):
    case = MA.status_cases()[name]
    rc, files, ln, st = MA.run_host(*case[:4])
    assert rc == 0
    MA.check_session(case, files, ln, st)
    assert any(s for s, _ in case[4])
    # the smallest input: one byte more room (and the tail's), one byte of stream, and there is no status
    sizes, slots, kinds, capacity, _ = case
    if name.startswith("capacity"):
        assert MA.run_host(sizes, slots, kinds, capacity + 1)[3].tolist() == [M.ST_CAPACITY, 0, 0]  # the frame fits, the tail does not
        assert not MA.run_host(sizes, slots, kinds, capacity + 1 + 0x1000)[3].any()
    else:
        for ok in (1, slots.shape[2]):
            s2 = sizes.copy()
            s2[4, 1] = ok
            assert not MA.run_host(s2, slots, kinds, capacity + slots.shape[2])[3].any(), ok


def test_header_library_and_binding_agree():
    from mobiclipdecoder_amd import build, mux
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobiclip_mux_audio.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mobi_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(mux._AUDIO_SIGS) == NAMES
    assert set(names) <= set(build.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    lib = mux._lib()
    for name, (res, args) in mux._AUDIO_SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == list(args), name
        proto = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(proto.split(",")) == len(args), name
    # the video-only header and its table are as they were
    old = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobiclip_mux.h")).read(), flags=re.S)
    assert not set(names) & set(re.findall(r"\b(mobi_[a-z0-9_]+)\s*\(", old)) and not set(names) & set(mux._SIGS)


def test_refusals_need_no_device():
    from mobiclipdecoder_amd import mux
    lib = mux._lib()
    assert lib.mobi_mux_set_audio(None, 1, 32000, 2) == MOBI_E_ARG
    assert lib.mobi_mux_append_audio_async(None, None, 1, None, 64, 64, None) == MOBI_E_ARG
