"""The muxer without a GPU (include/mobiclip_mux.h; csrc/mobi_mux.h run by tests/tools/mobi_mux_host.cpp, the host model the kernels are
compared against in tests/test_mux_gpu.py).

  1  for both containers the model's images equal tests/containers.py's write_moflex / write_mods byte for byte, on random payloads: five
     clips with different length sequences around one, two and three Moflex blocks (Mods: also 2^18 - 1), key frames at 0 and every third
  2  mobi_mux_framed_bytes / mobi_mux_fixed_bytes add up to the file length; the closed form against the writer for the lengths named
  3  the project's MoLiveDemux / ModsDemuxer read every frame back
  4  every status bit is raised by the smallest input that raises it; the other clips stay exact, the refused row is untouched behind the
     point of refusal, nothing at or behind a capacity is written
  5  header, library and the binding's table agree; the refusals that need no device
  6  the host model under sanitizers, as a program of its own, with buffers exactly one capacity long
  7  the clips cover every alignment of a frame's start mod 16 and of a Moflex block boundary mod 4
  8  Moflex frames of 32 to 66 blocks (mux_model.long_moflex) equal the writer's and read back"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import containers
from tests import mux_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tests", "tools")
CSRC = os.path.join(ROOT, "mobiclipdecoder_amd", "csrc")
MOBI_E_ARG = -7
CONTAINERS = (M.MOFLEX, M.MODS)
NAMES = ["mobi_mux_append_async", "mobi_mux_begin_async", "mobi_mux_create", "mobi_mux_destroy", "mobi_mux_finish_async", "mobi_mux_fixed_bytes",
         "mobi_mux_framed_bytes"]


def _clean(container):
    sizes, slots, keys = M.clips(container)
    return sizes, slots, keys, M.capacity_of(container, sizes, keys), int(keys.sum()), [(0, None)] * M.N


@pytest.mark.parametrize("container", CONTAINERS)
def test_model_equals_the_writers(container):
    case = _clean(container)
    sizes = case[0]
    assert set(M.LENS) <= set(sizes.ravel().tolist()) and (container == M.MOFLEX or M.MODS_LONGEST in sizes)
    assert len({tuple(sizes[:, c]) for c in range(M.N)}) == M.N and list(np.flatnonzero(case[2])) == list(range(0, sizes.shape[0], 3))
    rc, files, ln, st = M.run_host(container, *case[:5])
    assert rc == 0
    M.check_session(container, case, files, ln, st)


@pytest.mark.parametrize("container", CONTAINERS)
def test_framed_and_fixed_bytes_add_up(container):
    from mobiclipdecoder_amd import mux
    name = ("moflex", "mods")[container]
    sizes, slots, keys, capacity, n_keys, _ = _clean(container)
    _, _, ln, _ = M.run_host(container, sizes, slots, keys, capacity, n_keys)
    for c in range(M.N):
        total = mux.fixed_bytes(name, n_keys) + sum(mux.framed_bytes(name, int(v)) for v in sizes[:, c])
        assert total == int(ln[c]) == len(M.reference(container, sizes, slots, keys, c))
    for L in (1, 4, 64, 3968, 3969, 7936, 7937, 11904, 12001, 26336, 100000):
        if container == M.MOFLEX:
            want = len(containers.write_moflex([bytes(L)], 16, 16)) - 30 - 0x1000
            k, r = divmod(L, M.B)
            closed = 8 + L if L <= M.B else k * (M.B + 4) + 8 + r if r else (k - 1) * (M.B + 4) + M.B + 8
            assert closed == want
        else:
            want = len(containers.write_mods([bytes(L)], 16, 16, [])) - 0x30
        assert mux.framed_bytes(name, L) == M.host().mux_host_framed_bytes(container, L) == want, L
    for k in (0, 1, 7):
        assert mux.fixed_bytes(name, k) == M.host().mux_host_fixed_bytes(container, k) == (30 + 0x1000 if container == M.MOFLEX else 0x30 + 8 * k)
    assert mux._lib().mobi_mux_framed_bytes(2, 10) == 0 and mux._lib().mobi_mux_fixed_bytes(-1, 0) == 0


def test_moflex_files_read_back():
    from mobiclipdecoder_amd.demux import MoLiveDemux
    sizes, slots, keys, capacity, n_keys, _ = _clean(M.MOFLEX)
    _, files, ln, _ = M.run_host(M.MOFLEX, sizes, slots, keys, capacity, n_keys)
    for c in range(M.N):
        d = MoLiveDemux(files[c, :int(ln[c])].copy())
        got = list(d.frames())
        d.close()
        assert [bytes(f) for _, f in got] == [f + b"\x00\x00" for f in M.frames_of(sizes, slots, c)]
        st = got[0][0]
        assert (st.chunk_id, st.stream_index, st.fps_rate, st.fps_scale, st.width, st.height) == (1, 0, M.FPS[0], M.FPS[1], M.W, M.H)


def _long_case():
    sizes, slots, keys = M.long_moflex()
    return sizes, slots, keys, M.capacity_of(M.MOFLEX, sizes, keys), int(keys.sum()), [(0, None)] * M.LONG_N


def test_moflex_frames_above_32_blocks():
    """mux_model.long_moflex: the model equals write_moflex byte for byte and MoLiveDemux reads every frame back; the frames are the ones
    the GPU comparison needs (a block count of 32, 33, 34, 64 and 66, each started at more than one residue mod 16, some misaligned)"""
    from mobiclipdecoder_amd.demux import MoLiveDemux
    case = _long_case()
    sizes, slots = case[0], case[1]
    blocks = -(-sizes.astype(np.int64) // M.B)
    assert sorted(set(blocks[blocks > 1].tolist())) == [32, 33, 34, 64, 66] and sizes.shape[1] == M.LONG_N == 2
    assert int(sizes.max()) < M.MODS_LONGEST and slots.shape[2] >= int(sizes.max())
    rc, files, ln, st = M.run_host(M.MOFLEX, *case[:5])
    assert rc == 0
    M.check_session(M.MOFLEX, case, files, ln, st)
    starts = {}
    for c in range(M.LONG_N):
        d = MoLiveDemux(files[c, :int(ln[c])].copy())
        got = [bytes(f) for _, f in d.frames()]
        d.close()
        assert got == [f + b"\x00\x00" for f in M.frames_of(sizes, slots, c)]
        for t, s in enumerate(M.frame_starts(M.MOFLEX, sizes, c)[0]):
            if sizes[t, c] > M.B:
                starts.setdefault(int(sizes[t, c]), set()).add(s % 16)
    print({k: sorted(v) for k, v in starts.items()})
    assert all(len(v) == 2 for v in starts.values()) and any(s % 4 for v in starts.values() for s in v)


def test_mods_files_read_back():
    from mobiclipdecoder_amd.demux import ModsDemuxer
    sizes, slots, keys, capacity, n_keys, _ = _clean(M.MODS)
    _, files, ln, _ = M.run_host(M.MODS, sizes, slots, keys, capacity, n_keys)
    T = sizes.shape[0]
    for c in range(M.N):
        d = ModsDemuxer(files[c, :int(ln[c])].copy())
        h = d.Header
        assert (h.frame_count, h.width, h.height, h.fps, h.biggest_frame, h.keyframe_count) == (T, M.W, M.H, M.FPS[2], int(sizes[:, c].max()), n_keys)
        starts, end = M.frame_starts(M.MODS, sizes, c)
        assert h.keyframe_index_offset == end
        assert d.KeyFrames == [(t, starts[t]) for t in range(T) if keys[t]]
        want = M.frames_of(sizes, slots, c)
        for t in range(T):
            pkt, na, key = d.ReadFrame()
            # (the constructor has jumped to key frame 0, so the reader, like the reference's, announces the key frames behind it)
            assert bytes(pkt) == want[t] and na == 0 and key == bool(keys[t] and t > 0), (c, t)
        assert d.ReadFrame() is None
        d.close()


@pytest.mark.parametrize("container,name", [(c, n) for c in CONTAINERS for n in M.status_cases(c)])
def test_status_bits(container, name):
    case = M.status_cases(container)[name]
    rc, files, ln, st = M.run_host(container, *case[:5])
    assert rc == 0
    M.check_session(container, case, files, ln, st)
    assert any(s for s, _ in case[5])


def test_status_cases_are_the_smallest_inputs():
    """one byte more room, one byte less stream, one more table entry: no status"""
    for container in CONTAINERS:
        cases = M.status_cases(container)
        for name, grow in (("capacity_tail_only", 1), ("capacity_last_frame", 1 + (0x1000 if container == M.MOFLEX else 8 * cases["capacity_last_frame"][4]))):
            sizes, slots, keys, capacity, max_keys, _ = cases[name]
            assert not M.run_host(container, sizes, slots, keys, capacity + grow, max_keys)[3].any(), name
        sizes, slots, keys, capacity, max_keys, _ = cases["size_zero"]
        for ok in (1, min(slots.shape[2], (1 << 18) - 1)):  # (a Mods slot of 2^18 bytes: a stream that fills it is the next case's)
            s2 = sizes.copy()
            s2[4, 2] = ok
            assert not M.run_host(container, s2, slots, keys, capacity + slots.shape[2], max_keys)[3].any(), ok
    cases = M.status_cases(M.MODS)
    sizes, slots, keys, capacity, max_keys, _ = cases["one_key_too_many"]
    assert not M.run_host(M.MODS, sizes, slots, keys, capacity, max_keys + 1)[3].any()
    assert (1 << 18) - 1 in M.clips(M.MODS)[0]  # the longest frame the format takes is in the clean clips


def test_coverage_of_alignments():
    """the kernel's misaligned paths are exercised only if the destinations take every alignment: frame starts every residue mod 16, and
    some boundary between two Moflex blocks every residue mod 4"""
    for container in CONTAINERS:
        sizes = M.clips(container)[0]
        starts = [s for c in range(M.N) for s in M.frame_starts(container, sizes, c)[0]]
        assert {s % 16 for s in starts} == set(range(16)), (container, sorted(set(range(16)) - {s % 16 for s in starts}))
    sizes = M.clips(M.MOFLEX)[0]
    bounds = set()
    for c in range(M.N):
        for t, s in enumerate(M.frame_starts(M.MOFLEX, sizes, c)[0]):
            blocks = -(-int(sizes[t, c]) // M.B)
            bounds |= {(s + b * (M.B + 4)) % 4 for b in range(1, blocks)}
    assert bounds == {0, 1, 2, 3}


def test_header_library_and_binding_agree():
    from mobiclipdecoder_amd import build, mux
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobiclip_mux.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mobi_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(mux._SIGS) == NAMES
    assert set(names) <= set(build.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    lib = mux._lib()
    for name, (res, args) in mux._SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == list(args), name
    for name in names:
        proto = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(proto.split(",")) == len(mux._SIGS[name][1]), name
    demux_h = open(os.path.join(ROOT, "include", "mobiclip_demux.h")).read()
    assert "mobi_mux" not in demux_h
    import mobiclipdecoder_amd
    assert mobiclipdecoder_amd.MobiclipMuxer is mux.MobiclipMuxer


def test_refusals_need_no_device():
    from mobiclipdecoder_amd import mux
    lib = mux._lib()
    assert lib.mobi_mux_begin_async(None, None, 1, None, 64, 64) == MOBI_E_ARG
    assert lib.mobi_mux_append_async(None, None, 1, None, 64, 64, None, 0) == MOBI_E_ARG
    assert lib.mobi_mux_finish_async(None, None, 1, None, None) == MOBI_E_ARG
    for args in ((2, 48, 32, 30, 1, 0, 4, 4, 0), (0, 65536, 32, 30, 1, 0, 4, 4, 0), (0, 48, 65536, 30, 1, 0, 4, 4, 0), (0, 48, 32, 30, 1, 0, 0, 4, 0),
                 (1, 48, 32, 30, 1, 0, 4, -1, 0), (0, 48, 32, 65536, 1, 0, 4, 4, 0)):
        assert not lib.mobi_mux_create(*args), args
    with pytest.raises(ValueError):
        mux.framed_bytes("avi", 1)
    # the model refuses what the entry points refuse of a session's shape
    sizes, slots, keys = M.clips(M.MOFLEX)
    assert M.run_host(M.MOFLEX, sizes, slots, keys, 100000, 5, guard=-1)[0] == MOBI_E_ARG  # a pitch below the capacity
    assert M.run_host(M.MOFLEX, sizes, slots, keys, 100000, 5, slot_bytes=slots.shape[2] + 4)[0] == MOBI_E_ARG  # a pitch below slot_bytes
    files = np.zeros(64, np.uint8)
    ln, st = np.zeros(1, np.int64), np.zeros(1, np.int32)
    assert M.host().mux_host_run(M.MODS, 48, 32, 30, 1, 0, 1, 1, 0, files.ctypes.data, 1 << 32, 1 << 32, None, 0, 0, None, None, ln.ctypes.data, st.ctypes.data) == MOBI_E_ARG
    assert M.host().mux_host_run(3, 48, 32, 30, 1, 0, 1, 1, 0, files.ctypes.data, 64, 64, None, 0, 0, None, None, ln.ctypes.data, st.ctypes.data) == MOBI_E_ARG
    # a session without frames is a file: head and tail, header and an empty index
    assert M.host().mux_host_run(M.MODS, 48, 32, 30, 1, 0, 1, 1, 0, files.ctypes.data, 64, 48, None, 0, 0, None, None, ln.ctypes.data, st.ctypes.data) == 0
    assert ln[0] == 0x30 and st[0] == 0 and bytes(files[:4]) == b"MODS" and not files[48:].any()


def test_host_model_under_sanitizers(tmp_path):
    """tests/tools/mux_host_main.cpp: a program of its own with -fsanitize=address,undefined, linked statically (nothing sanitised is
    loaded into Python); its rows are exactly one capacity long and lie back to back, its slots exactly slot_bytes"""
    exe = str(tmp_path / "mux_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(TOOLS, "mux_host_main.cpp"), os.path.join(TOOLS, "mobi_mux_host.cpp"), "-o", exe], check=True)
    for container in CONTAINERS:
        runs = [_clean(container)] + [M.status_cases(container)[k] for k in ("capacity_last_frame", "capacity_tail_only", "size_above_slot")]
        for sizes, slots, keys, capacity, max_keys, _ in runs:
            T, n = sizes.shape
            _, want, ln, st = M.run_host(container, sizes, slots, keys, capacity, max_keys, guard=0)
            src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
            with open(src, "wb") as f:
                f.write(np.ascontiguousarray(sizes, np.int32).tobytes() + keys.tobytes() + slots.tobytes())
            p = subprocess.run([exe, str(container), str(M.W), str(M.H), str(max_keys), str(n), str(T), str(capacity), str(slots.shape[2]), src, dst],
                               capture_output=True, text=True)
            assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
            blob = np.fromfile(dst, np.uint8)
            assert np.array_equal(np.frombuffer(blob[:8 * n].tobytes(), np.int64), ln)
            assert np.array_equal(np.frombuffer(blob[8 * n:12 * n].tobytes(), np.int32), st)
            assert np.array_equal(blob[12 * n:].reshape(n, capacity), want)
