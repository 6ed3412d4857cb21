"""The muxer's audio stream on the GPU (csrc/mobi_mux.hip behind include/mobiclip_mux_audio.h and mux.py) against the host model
(tests/mux_audio_model.py, tests/tools/mobi_mux_audio_host.cpp), which tests/test_mux_audio_model.py holds against the restated writer; and
encode_clips(audio=).

  a  the kernels equal the model byte for byte -- files up to their lengths, the lengths, the status words -- on the model test's session
     of video and audio append calls and on its status cases; rows of 0xA5 at a pitch 64 bytes above the capacity
  b  encode_clips(container="moflex", audio=) at 32x32, N = 2, T = 5, gop 2: 32 kHz stereo at 30 fps (4 blocks behind every frame) and
     4 kHz (0, 1, 0, 1, 0 blocks: frames without audio), IMA and PCM16.  MoLiveDemux splits the file into the video frames of the same
     call without audio= and the audio frames MobiclipAudioEncoder.encode makes of the same blocks; MobiclipBatch and MobiclipAudio
     decode the file to the reported video and audio reconstructions
  c  the Python refusals"""
import numpy as np
import pytest
import torch

from tests import mux_audio_model as MA
from tests import mux_model as M

pytestmark = pytest.mark.gpu
MOBI_E_ARG, MOBI_E_UNSUPPORTED = -7, -6


def _dev():
    from mobiclipdecoder_amd.decoder import default_device
    return torch.device("cuda", default_device())


def _up(a):
    return torch.from_numpy(np.array(a)).to(_dev())


def _abi_session(case, audio=MA.AUDIO):
    import mobiclipdecoder_amd as m
    sizes, slots, kinds, capacity, _ = case
    T, n = sizes.shape
    mx = m.MobiclipMuxer("moflex", M.W, M.H, M.MAX_CLIPS, *M.FPS, max_key_frames=0, audio=audio)
    lib, s = mx._lib, torch.cuda.current_stream(_dev()).cuda_stream
    files = torch.full((n, capacity + M.GUARD), M.FILL, dtype=torch.uint8, device=_dev())
    d_slots, d_sizes = _up(slots), _up(sizes)
    ln = torch.full((n,), -1, dtype=torch.int64, device=_dev())
    st = torch.full((n,), -1, dtype=torch.int32, device=_dev())
    slot = slots.shape[2]
    assert lib.mobi_mux_begin_async(mx._h, s, n, files.data_ptr(), capacity + M.GUARD, capacity) == 0
    assert lib.mobi_mux_set_audio(mx._h, 1, 32000, 2) == MOBI_E_ARG  # a session is running
    for t in range(T):
        if kinds[t]:
            assert lib.mobi_mux_append_audio_async(mx._h, s, n, d_slots[t].data_ptr(), slot, slot, d_sizes[t].data_ptr()) == 0
        else:
            assert lib.mobi_mux_append_async(mx._h, s, n, d_slots[t].data_ptr(), slot, slot, d_sizes[t].data_ptr(), 0) == 0
    assert lib.mobi_mux_finish_async(mx._h, s, n, ln.data_ptr(), st.data_ptr()) == 0
    torch.cuda.synchronize()
    mx.close()
    return files.cpu().numpy(), ln.cpu().numpy(), st.cpu().numpy()


def _against_the_model(case):
    files, ln, st = _abi_session(case)
    rc, h_files, h_ln, h_st = MA.run_host(*case[:4])
    assert rc == 0
    assert np.array_equal(st, h_st) and np.array_equal(ln, h_ln), (st, h_st, ln, h_ln)
    for c in range(files.shape[0]):
        if h_st[c] == 0:
            assert np.array_equal(files[c, :h_ln[c]], h_files[c, :h_ln[c]]), f"clip {c} differs from the model"
            assert (files[c, case[3]:] == M.FILL).all()
        else:
            assert np.array_equal(files[c], h_files[c]), f"refused clip {c} differs from the model"
    MA.check_session(case, files, ln, st)


def test_kernels_equal_the_host_model():
    sizes, slots, kinds = MA.session()
    _against_the_model((sizes, slots, kinds, max(MA.ends(sizes, slots, kinds)) + 0x1000, [(0, None)] * MA.N))


@pytest.mark.parametrize("name", sorted(MA.status_cases()))
def test_status_bits_from_audio_frames(name):
    _against_the_model(MA.status_cases()[name])


def _pictures(n, T, W, H):
    """smooth, moving pictures: (n, T, W * H * 3 / 2) uint8"""
    y, x = np.mgrid[0:H, 0:W]
    out = np.zeros((n, T, W * H * 3 // 2), np.uint8)
    for c in range(n):
        for t in range(T):
            luma = (3 * x + 2 * y + 5 * t * (c + 1) + 20 * c) % 200 + 20
            chroma = np.full((H // 2, W), 120 + 4 * t + c, np.int64)
            out[c, t] = np.concatenate([luma.ravel(), chroma.ravel()]).astype(np.uint8)
    return out


def _split(blob):
    from mobiclipdecoder_amd.demux import MoLiveDemux
    d = MoLiveDemux(np.frombuffer(blob, np.uint8))
    got = [(s.chunk_id, s.stream_index, s.codec_id, s.frequency, s.channel, bytes(f[:-2])) for s, f in d.frames()]
    d.close()
    return got


@pytest.mark.parametrize("codec", ("ima", "pcm16"))
@pytest.mark.parametrize("rate,blocks", [(32000, [4, 4, 4, 4, 4]), (4000, [0, 1, 0, 1, 0])])
def test_encode_clips_with_audio(rate, blocks, codec):
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd import mux
    W, H, n, T, gop, nc, version = 32, 32, 2, 5, 2, 2, int(mux.CONTAINER_VERSION["moflex"])
    frames = _up(_pictures(n, T, W, H))
    total = 256 * sum(blocks)
    rng = np.random.default_rng(99)
    sound = (6000 * np.sin(np.arange(total + 300) / 9.0)[None, None] + rng.integers(-3000, 3000, (n, nc, total + 300))).astype(np.int16)
    audio = _up(sound)
    q = [24, 30, 24, 30, 24]
    files, recon, a_recon = m.encode_clips(frames, q, gop, version, W, H, recon=True, container="moflex", audio=audio, audio_codec=codec, audio_rate=rate)
    plain, recon_plain = m.encode_clips(frames, q, gop, version, W, H, recon=True)
    assert torch.equal(recon, recon_plain) and tuple(a_recon.shape) == (n, nc, total) and a_recon.dtype == torch.int16
    # the audio frames a call of the encoder makes of the same blocks
    enc = m.MobiclipAudioEncoder(n, nc, codec, max(blocks))
    want_audio, want_rec, at = [[] for _ in range(n)], [], 0
    for b in blocks:
        if b:
            fr, ln, ex = enc.encode(audio[:, :, 256 * at:256 * (at + b)], recon=True)
            fr, ln = fr.cpu().numpy(), ln.cpu().numpy()
            for c in range(n):
                want_audio[c].append(fr[c, :ln[c]].tobytes())
            want_rec.append(ex["recon"])
            at += b
    enc.close()
    assert torch.equal(a_recon, torch.cat(want_rec, 2))
    cid = mux.AUDIO_CODEC_IDS[codec]
    for c in range(n):
        got = _split(files[c])
        assert [g[5] for g in got if g[0] == 1] == plain[c], c
        assert [g[5] for g in got if g[0] == 2] == want_audio[c], c
        assert all(g[1:5] == (1, cid, rate, nc) for g in got if g[0] == 2)
        assert [g[0] for g in got] == [k for b in blocks for k in ((1, 2) if b else (1,))]  # the order of the append calls
        assert len(files[c]) == mux.fixed_bytes("moflex", 0, audio=True) + sum(mux.framed_bytes("moflex", len(g[5])) for g in got)
    # the decoders: the file's video frames to the video reconstruction, its audio frames to the audio reconstruction
    split = [_split(f) for f in files]
    b = m.MobiclipBatch(n, W, H, version)
    for t in range(T):
        rcs, _ = b.decode([[g[5] for g in split[c] if g[0] == 1][t] for c in range(n)], [0] * n)
        assert rcs == [0] * n, (t, rcs)
        got = b.export_tensor("i420")[0]
        torch.cuda.synchronize()
        assert torch.equal(got, recon[:, t]), t
    b.close()
    dec = m.MobiclipAudio(n, nc, codec, "moflex")
    at = 0
    for i, bl in enumerate(bl for bl in blocks if bl):
        out, n_samples, rc = dec.decode([[g[5] for g in split[c] if g[0] == 2][i] + b"\x00\x00" for c in range(n)])
        torch.cuda.synchronize()
        assert not rc.any() and (n_samples == 256 * bl).all()
        assert torch.equal(out[:, :, :256 * bl], a_recon[:, :, at:at + 256 * bl]), i
        at += 256 * bl
    dec.close()
    if codec == "pcm16":
        assert torch.equal(a_recon, audio[:, :, :total])


def test_python_refusals():
    import mobiclipdecoder_amd as m
    W, H = 32, 32
    dev = _dev()
    frames = torch.zeros((2, 2, W * H * 3 // 2), dtype=torch.uint8, device=dev)
    audio = torch.zeros((2, 2, 4096), dtype=torch.int16, device=dev)
    with pytest.raises(ValueError, match="moflex"):
        m.encode_clips(frames, 30, 2, 2, W, H, audio=audio, audio_rate=32000)
    with pytest.raises(ValueError, match="moflex"):
        m.encode_clips(frames, 30, 2, int(m.MobiclipVersion.ModsDS), W, H, container="mods", audio=audio, audio_rate=32000)
    with pytest.raises(ValueError, match="audio_rate"):
        m.encode_clips(frames, 30, 2, 2, W, H, container="moflex", audio=audio)
    with pytest.raises(ValueError, match="samples"):
        m.encode_clips(frames, 30, 2, 2, W, H, container="moflex", audio=audio[:, :, :2047], audio_rate=32000)  # 2 frames take 8 blocks
    with pytest.raises(ValueError):
        m.encode_clips(frames, 30, 2, 2, W, H, container="moflex", audio=audio[:1], audio_rate=32000)
    with pytest.raises(m.MobiclipError, match="no encoder"):
        m.encode_clips(frames, 30, 2, 2, W, H, container="moflex", audio=audio, audio_rate=32000, audio_codec="fastaudio")
    mods = m.MobiclipMuxer("mods", W, H, 2)
    with pytest.raises(m.MobiclipError):
        mods.set_audio("ima", 32000, 2)
    assert mods._lib.mobi_mux_set_audio(mods._h, 1, 32000, 2) == MOBI_E_UNSUPPORTED
    mods.close()
    mx = m.MobiclipMuxer("moflex", W, H, 2)
    slots, sizes = torch.zeros((2, 64), dtype=torch.uint8, device=dev), torch.full((2,), 8, dtype=torch.int32, device=dev)
    mx.begin(2, 8192)
    with pytest.raises(m.MobiclipError, match="audio"):
        mx.append_audio(slots, sizes)
    s = torch.cuda.current_stream(dev).cuda_stream
    assert mx._lib.mobi_mux_append_audio_async(mx._h, s, 2, slots.data_ptr(), 64, 64, sizes.data_ptr()) == MOBI_E_ARG  # audio is off
    assert [len(f) for f in mx.finish()] == [30 + 0x1000] * 2
    for bad in ((3, 32000, 2), (1, (1 << 24) + 1, 2), (1, 32000, 0), (1, 32000, 9), (-1, 32000, 2)):
        assert mx._lib.mobi_mux_set_audio(mx._h, *bad) == MOBI_E_ARG, bad
    with pytest.raises(ValueError):
        mx.set_audio("mp3", 32000, 2)
    mx.set_audio("pcm16", 1 << 24, 8)
    assert mx.audio == (2, 1 << 24, 8)
    mx.begin(2, 8192)
    mx.append_audio(slots, sizes)
    assert mx._lib.mobi_mux_append_audio_async(mx._h, s, 2, slots.data_ptr(), 60, 64, sizes.data_ptr()) == MOBI_E_ARG  # pitch below slot_bytes
    assert mx._lib.mobi_mux_append_audio_async(mx._h, s, 3, slots.data_ptr(), 64, 64, sizes.data_ptr()) == MOBI_E_ARG
    out = mx.finish()
    assert [len(f) for f in out] == [38 + 16 + 0x1000] * 2 and out[0][28:36] == bytes([2, 6, 1, 2, 0xFF, 0xFF, 0xFF, 7])
    mx.set_audio("ima", 0, 0)  # off again: the next session is video only
    assert mx.audio is None
    mx.begin(2, 8192)
    assert [len(f) for f in mx.finish()] == [30 + 0x1000] * 2
    mx.close()
