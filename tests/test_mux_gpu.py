"""The muxer on the GPU (csrc/mobi_mux.hip behind include/mobiclip_mux.h and mobiclipdecoder_amd/mux.py) against the host model
(tests/mux_model.py, tests/tools/mobi_mux_host.cpp), which tests/test_mux_model.py holds against tests/containers.py's writers.

  a  the kernels equal the model byte for byte -- files up to their lengths, the lengths, the status words -- on the model test's clips:
     5 clips in a muxer of 8, slots random behind each stream's length, rows of 0xA5 at a pitch 64 bytes above the capacity: the guard
     bytes and everything at or behind the capacity stay 0xA5
  b  every status case of the CPU test
  c  two sessions on one object with different n; a side stream; finish(to_host=False) followed by the host form
  d  round trips at 48x32, both versions: encode_clips(container=) gives files the demuxers split into frames, MobiclipBatch decodes
     them to the recon tensor the same call returned, and apart from the framing the frames are encode_clips(container=None)'s; the same
     with target_bytes=
  e  the Python refusals
  f  Moflex frames of 32 to 66 blocks (mux_model.long_moflex): a workgroup of mobi_mux_append takes a second and a third block
  g  the round trip at 272x256 with intra=True: slots of the encoders' stream bound, real frames of three and more Moflex blocks"""
import numpy as np
import pytest
import torch

from tests import enc_parts_model as Q
from tests import enc_pintra_model as PI
from tests import mux_model as M

pytestmark = pytest.mark.gpu
CONTAINERS = (M.MOFLEX, M.MODS)
NAME = {M.MOFLEX: "moflex", M.MODS: "mods"}
MOBI_E_ARG = -7


def _dev():
    from mobiclipdecoder_amd.decoder import default_device
    return torch.device("cuda", default_device())


def _up(a):
    return torch.from_numpy(np.array(a)).to(_dev())  # (a copy: the shared clips are read-only)


def _muxer(container, max_keys):
    import mobiclipdecoder_amd as m
    return m.MobiclipMuxer(NAME[container], M.W, M.H, M.MAX_CLIPS, *M.FPS, max_key_frames=max_keys)


def _abi_session(container, case):
    """one session through the C ABI itself, on rows of FILL at a pitch GUARD above the capacity -> files, lengths, status as numpy"""
    sizes, slots, keys, capacity, max_keys, _ = case
    T, n = sizes.shape
    mx = _muxer(container, max_keys)
    lib, s = mx._lib, torch.cuda.current_stream(_dev()).cuda_stream
    files = torch.full((n, capacity + M.GUARD), M.FILL, dtype=torch.uint8, device=_dev())
    d_slots, d_sizes = _up(slots), _up(sizes)
    ln = torch.full((n,), -1, dtype=torch.int64, device=_dev())
    st = torch.full((n,), -1, dtype=torch.int32, device=_dev())
    slot = slots.shape[2]
    assert lib.mobi_mux_begin_async(mx._h, s, n, files.data_ptr(), capacity + M.GUARD, capacity) == 0
    for t in range(T):
        assert lib.mobi_mux_append_async(mx._h, s, n, d_slots[t].data_ptr(), slot, slot, d_sizes[t].data_ptr(), int(keys[t])) == 0
    assert lib.mobi_mux_finish_async(mx._h, s, n, ln.data_ptr(), st.data_ptr()) == 0
    torch.cuda.synchronize()
    mx.close()
    return files.cpu().numpy(), ln.cpu().numpy(), st.cpu().numpy()


def _against_the_model(container, case):
    files, ln, st = _abi_session(container, case)
    rc, h_files, h_ln, h_st = M.run_host(container, *case[:5])
    assert rc == 0
    assert np.array_equal(st, h_st), (st, h_st)
    assert np.array_equal(ln, h_ln), (ln, h_ln)
    capacity = case[3]
    assert (files[:, capacity:] == M.FILL).all(), "a byte at or behind a capacity was written"
    for c in range(files.shape[0]):
        if h_st[c] == 0:
            assert np.array_equal(files[c, :h_ln[c]], h_files[c, :h_ln[c]]), f"clip {c} differs from the model"
        else:  # the model leaves FILL behind the point of refusal: so must the kernels, and equal bytes in front of it
            assert np.array_equal(files[c], h_files[c]), f"refused clip {c} differs from the model"
    M.check_session(container, case, files, ln, st)


def _clean(container):
    sizes, slots, keys = M.clips(container)
    return sizes, slots, keys, M.capacity_of(container, sizes, keys), int(keys.sum()), [(0, None)] * M.N


@pytest.mark.parametrize("container", CONTAINERS)
def test_kernels_equal_the_host_model(container):
    assert M.N == 5 and M.MAX_CLIPS == 8
    _against_the_model(container, _clean(container))


@pytest.mark.parametrize("container,name", [(c, n) for c in CONTAINERS for n in M.status_cases(c)])
def test_status_bits(container, name):
    _against_the_model(container, M.status_cases(container)[name])


def _py_session(mx, sizes, slots, keys, capacity, stream=None, to_host=True):
    T, n = sizes.shape
    d_slots, d_sizes = _up(slots), _up(sizes)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(_dev()))
    mx.begin(n, capacity, stream=stream)
    for t in range(T):
        mx.append(d_slots[t], d_sizes[t], bool(keys[t]), stream=stream)
    return mx.finish(stream=stream, to_host=to_host)


def _model_files(container, sizes, slots, keys, capacity, max_keys):
    rc, files, ln, st = M.run_host(container, sizes, slots, keys, capacity, max_keys, guard=0)
    assert rc == 0 and not st.any()
    return [files[c, :ln[c]].tobytes() for c in range(sizes.shape[1])]


@pytest.mark.parametrize("container", CONTAINERS)
def test_two_sessions_a_side_stream_and_device_results(container):
    sizes, slots, keys, capacity, max_keys, _ = _clean(container)
    mx = _muxer(container, max_keys)
    want = _model_files(container, sizes, slots, keys, capacity, max_keys)
    assert _py_session(mx, sizes, slots, keys, capacity) == want
    # the same object again, fewer clips, other frames, on a stream of its own
    s2, l2 = np.ascontiguousarray(sizes[2:9, 1:4]), np.ascontiguousarray(slots[2:9, 1:4])
    k2 = M.key_flags(7)
    cap2 = M.capacity_of(container, s2, k2) + 5
    side = torch.cuda.Stream(_dev())
    assert _py_session(mx, s2, l2, k2, cap2, stream=side) == _model_files(container, s2, l2, k2, cap2, max_keys)
    # and as device tensors first, the host form behind them
    from mobiclipdecoder_amd import mux
    files, ln, st = _py_session(mx, sizes, slots, keys, capacity, to_host=False)
    assert files.is_cuda and tuple(files.shape) == (M.N, capacity) and ln.dtype == torch.int64 and st.dtype == torch.int32
    assert mux.files_to_host(files, ln, st) == want
    assert [int(v) for v in ln.cpu()] == [len(w) for w in want] and not st.cpu().any()
    mx.close()


def test_finish_names_the_first_clip_with_a_status():
    import mobiclipdecoder_amd as m
    sizes, slots, keys, capacity, max_keys, expect = M.status_cases(M.MOFLEX)["size_zero"]
    mx = _muxer(M.MOFLEX, max_keys)
    with pytest.raises(m.MobiclipError, match=r"clip 2 .*0x2"):
        _py_session(mx, sizes, slots, keys, capacity)
    mx.close()


def _demux(container, blob):
    from mobiclipdecoder_amd.demux import ModsDemuxer, MoLiveDemux
    if container == "moflex":
        d = MoLiveDemux(np.frombuffer(blob, np.uint8))
        frames = [bytes(f[:-2]) for _, f in d.frames()]  # two zero bytes appended
        d.close()
        return frames, None
    d = ModsDemuxer(np.frombuffer(blob, np.uint8))
    frames = []
    while (fr := d.ReadFrame()) is not None:
        frames.append(bytes(fr[0]))
    assert d.Header.frame_count == len(frames)
    keys = [k for k, _ in d.KeyFrames]
    d.close()
    return frames, keys


@pytest.mark.parametrize("rate", (False, True))
@pytest.mark.parametrize("gop", (2, 4))
@pytest.mark.parametrize("container", ("moflex", "mods"))
def test_round_trip(container, gop, rate):
    """gop 4 over five frames is I + 3 P + I; gop 2 is I P I P I"""
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd import mux
    W, H, version = 48, 32, int(mux.CONTAINER_VERSION[container])
    sets = Q.sequence_sets(W, H)
    frames = np.concatenate([sets["mixed5"][0], sets["two_motion"][0]])[:, [0, 1, 2, 3, 1]]
    n, T = frames.shape[:2]
    dev_frames = _up(frames)
    kw = dict(quantizer=None, target_bytes=[400, 150, 150, 300, 400], carry_bytes=32) if rate else dict(quantizer=[24, 30, 30, 18, 24])
    q = kw.pop("quantizer")
    # at these quantisers the noisy clips are longer than their raw pictures, which the default file_bytes does not provide for: the room
    # is given for them, and the default serves the rate-controlled run
    room = None if rate else mux.fixed_bytes(container, T) + T * mux.framed_bytes(container, 4 * W * H)
    files, recon = m.encode_clips(dev_frames, q, gop, version, W, H, recon=True, container=container, file_bytes=room, **kw)
    plain, recon_plain = m.encode_clips(dev_frames, q, gop, version, W, H, recon=True, **kw)
    assert torch.equal(recon, recon_plain) and tuple(recon.shape) == (n, T, W * H * 3 // 2)
    assert len(files) == n and all(isinstance(f, bytes) for f in files)
    split = [_demux(container, f) for f in files]
    for c in range(n):
        assert split[c][0] == plain[c], c
        if container == "mods":
            assert split[c][1] == list(range(0, T, gop))
        assert len(files[c]) == mux.fixed_bytes(container, len(range(0, T, gop))) + sum(mux.framed_bytes(container, len(s)) for s in plain[c])
    b = m.MobiclipBatch(n, W, H, version)
    for t in range(T):
        streams = [split[c][0][t] for c in range(n)]
        rcs, offs = b.decode(streams, [0] * n)
        assert rcs == [0] * n, (t, rcs)
        got = b.export_tensor("i420")[0]
        torch.cuda.synchronize()
        assert torch.equal(got, recon[:, t]), t
    b.close()


def test_moflex_frames_above_32_blocks():
    """mux_model.long_moflex: frames of 32 to 66 Moflex blocks, so that a workgroup of mobi_mux_append's grid of 32 takes a second and a
    third block, each with its own header, the last with the terminator, at a stride of B + 4 in the file"""
    sizes, slots, keys = M.long_moflex()
    assert -(-int(sizes.max()) // M.B) > 2 * 32
    _against_the_model(M.MOFLEX, (sizes, slots, keys, M.capacity_of(M.MOFLEX, sizes, keys), int(keys.sum()), [(0, None)] * M.LONG_N))


@pytest.mark.parametrize("rate", (False, True))
@pytest.mark.parametrize("container", ("moflex", "mods"))
def test_round_trip_at_272x256_with_intra_macroblocks(container, rate):
    """test_round_trip at 272 macroblocks with intra=True: the slots are the encoders' stream bound (93 blocks of room a slot, a grid
    clamped to 32), real frames span three and more Moflex blocks, and the P-frames mix macroblock kinds.  Five clips of five frames
    from enc_pintra_model.geometry_set in the order 0, 1, 3, 2, 1 under gop 4 (I P P P I): in the `cut` clips every P-frame stands behind
    a cut, in the `uncover` clips the motion jumps two steps ahead and one back."""
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd import mux
    W, H, gop, version = 272, 256, 4, int(mux.CONTAINER_VERSION[container])
    frames = PI.geometry_set(W, H)[0][:, [0, 1, 3, 2, 1]]
    n, T = frames.shape[:2]
    assert (n, T) == (5, 5)
    dev_frames = _up(frames)
    kw = dict(quantizer=None, target_bytes=[16000, 6000, 9000, 6000, 12000], carry_bytes=512) if rate else dict(quantizer=[20, 26, 18, 26, 22])
    q = kw.pop("quantizer")
    files, recon = m.encode_clips(dev_frames, q, gop, version, W, H, recon=True, container=container, intra=True, **kw)
    plain, recon_plain = m.encode_clips(dev_frames, q, gop, version, W, H, recon=True, intra=True, **kw)
    assert torch.equal(recon, recon_plain) and tuple(recon.shape) == (n, T, W * H * 3 // 2)
    assert len(files) == n and all(isinstance(f, bytes) for f in files)
    split = [_demux(container, f) for f in files]
    for c in range(n):
        assert split[c][0] == plain[c], c
        if container == "mods":
            assert split[c][1] == list(range(0, T, gop))
        assert len(files[c]) == mux.fixed_bytes(container, len(range(0, T, gop))) + sum(mux.framed_bytes(container, len(s)) for s in plain[c])
    longest = max(len(s) for clip in plain for s in clip)
    print(container, "rate" if rate else "fixed", [[len(s) for s in clip] for clip in plain])
    assert longest > 2 * M.B  # three Moflex blocks or more from real content
    if not rate:  # the model's chain of the P-frames: the same bytes, and macroblocks of both kinds in them
        qs = np.tile(np.array(q, np.uint8), (n, 1))
        ch = PI.chain(W, H, version, 1, frames[:, :gop], qs[:, :gop], threads=n)
        for t in range(gop):
            assert [plain[c][t] for c in range(n)] == [ch[t]["streams"][c, : ch[t]["bytes"][c]].tobytes() for c in range(n)], t
        assert all(PI.is_intra(ch[t]).any() and not PI.is_intra(ch[t]).all() for t in range(1, gop))
    b = m.MobiclipBatch(n, W, H, version)
    b.set_motion(True)
    intra_mbs = 0
    for t in range(T):
        streams = [split[c][0][t] for c in range(n)]
        rcs, offs = b.decode(streams, [0] * n)
        assert rcs == [0] * n, (t, rcs)
        got = b.export_tensor("i420")[0]
        mb = b.export_motion("mb")[0] if t % gop else None
        torch.cuda.synchronize()
        assert torch.equal(got, recon[:, t]), t
        if mb is not None:  # the decoder's own count of the intra macroblocks of a P-frame
            intra_mbs += int((mb[:, 0] == 1).sum())
    assert intra_mbs > 0
    b.close()


def test_python_refusals():
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd import mux
    W, H = 48, 32
    frames = torch.zeros((2, 2, W * H * 3 // 2), dtype=torch.uint8, device=_dev())
    for container, version in (("moflex", m.MobiclipVersion.ModsDS), ("mods", m.MobiclipVersion.Moflex3DS)):
        with pytest.raises(ValueError, match="carries"):
            m.encode_clips(frames, 30, 2, version, W, H, container=container)
    with pytest.raises(ValueError, match="container"):
        m.encode_clips(frames, 30, 2, 2, W, H, container="avi")
    with pytest.raises(m.MobiclipError, match="file_bytes"):
        m.encode_clips(frames, 30, 2, 2, W, H, container="moflex", file_bytes=mux.fixed_bytes("moflex") + 8)
    with pytest.raises(ValueError):
        m.MobiclipMuxer("avi", W, H, 2)
    with pytest.raises(m.MobiclipError):
        m.MobiclipMuxer("moflex", 65536, H, 2)
    mx = m.MobiclipMuxer("mods", W, H, 2, max_key_frames=2)
    slots, sizes = torch.zeros((2, 64), dtype=torch.uint8, device=_dev()), torch.full((2,), 8, dtype=torch.int32, device=_dev())
    with pytest.raises(m.MobiclipError, match="before begin"):
        mx.append(slots, sizes, True)
    with pytest.raises(m.MobiclipError, match="before begin"):
        mx.finish()
    with pytest.raises(ValueError):
        mx.begin(3, 4096)
    # the entry points' own refusals, with a live object: nothing is enqueued
    s = torch.cuda.current_stream(_dev()).cuda_stream
    row = torch.zeros((2, 4096), dtype=torch.uint8, device=_dev())
    ln, st = torch.zeros(2, dtype=torch.int64, device=_dev()), torch.zeros(2, dtype=torch.int32, device=_dev())
    lib = mx._lib
    assert lib.mobi_mux_append_async(mx._h, s, 2, slots.data_ptr(), 64, 64, sizes.data_ptr(), 1) == MOBI_E_ARG      # no begin
    assert lib.mobi_mux_finish_async(mx._h, s, 2, ln.data_ptr(), st.data_ptr()) == MOBI_E_ARG
    assert lib.mobi_mux_begin_async(mx._h, s, 3, row.data_ptr(), 4096, 4096) == MOBI_E_ARG                         # n above max_clips
    assert lib.mobi_mux_begin_async(mx._h, s, 0, row.data_ptr(), 4096, 4096) == MOBI_E_ARG
    assert lib.mobi_mux_begin_async(mx._h, s, 2, row.data_ptr(), 4095, 4096) == MOBI_E_ARG                         # pitch below capacity
    assert lib.mobi_mux_begin_async(mx._h, s, 2, None, 4096, 4096) == MOBI_E_ARG
    assert lib.mobi_mux_begin_async(mx._h, s, 2, row.data_ptr(), 1 << 32, 1 << 32) == MOBI_E_ARG                   # Mods offsets are u32
    mx.begin(2, 4096)
    with pytest.raises(ValueError):
        mx.append(slots[:1], sizes[:1], True)
    with pytest.raises(ValueError):
        mx.append(slots, sizes.to(torch.int64), True)
    assert lib.mobi_mux_append_async(mx._h, s, 2, slots.data_ptr(), 60, 64, sizes.data_ptr(), 1) == MOBI_E_ARG      # pitch below slot_bytes
    assert lib.mobi_mux_append_async(mx._h, s, 2, slots.data_ptr(), 64, 64, None, 1) == MOBI_E_ARG
    assert lib.mobi_mux_append_async(mx._h, s, 3, slots.data_ptr(), 64, 64, sizes.data_ptr(), 1) == MOBI_E_ARG
    mx.append(slots, sizes, True)
    out = mx.finish()
    assert [len(f) for f in out] == [0x30 + 12 + 8] * 2
    mx.close()
    with pytest.raises(m.MobiclipError, match="closed"):
        mx.begin(2, 4096)
    with pytest.raises(m.MobiclipError, match="closed"):
        mx.append(slots, sizes, True)
