"""The audio encoder on the GPU (csrc/mobi_audio_enc.hip behind include/mobiclip_audio_enc.h and mobiclipdecoder_amd/audio_enc.py) against
the plain-Python model (tests/audio_enc_model.py), which tests/test_audio_enc_model.py holds against the C++ host model.

  a  the kernels equal the model byte for byte -- frames, lengths, reconstruction, stats -- on the model test's signals at (N, C, B) =
     (1, 1, 1), (3, 2, 2), (2, 8, 1) and (33, 2, 3): 66 lanes, so the encode kernel's lanes cross a wave and its second wave has two live
     rows.  Stream s carries signal (s + offset) mod 7 and every shape runs with all seven offsets, so every shape, the one-stream
     one too, carries every signal (with C = 8: the noise's eight different channels, the sine's eight phases).  Through the C ABI itself:
     sample rows at a pitch 64 above S, slots of 0xA5 at a pitch 64 above slot_bytes, untouched behind every frame and between the rows;
     every shape once on a side stream; IMA and PCM16
  b  the frames, decoded by MobiclipAudio in Moflex framing on the GPU, are the reported reconstruction (PCM16 with one channel: and one
     more sample, 0); the samples are given as a view of longer rows, as a decode call leaves them
  c  calls without recon and without stats give the same frames
  d  the Python refusals"""
import numpy as np
import pytest
import torch

from tests import audio_enc_model as A

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (3, 2, 2), (2, 8, 1), (33, 2, 3)]
PAD = 64


def _dev():
    from mobiclipdecoder_amd.decoder import default_device
    return torch.device("cuda", default_device())


def _abi(codec, x, recon=True, stats=True, side=False):
    """one call through the C ABI -> slots (n, slot + PAD), sizes, recon, stats as numpy"""
    import mobiclipdecoder_amd as m
    n, nc, S = x.shape
    B = S // 256
    dev = _dev()
    enc = m.MobiclipAudioEncoder(n, nc, codec, B)
    padded = torch.full((n, nc, S + PAD), 0x5A5A, dtype=torch.int16, device=dev)
    padded[:, :, :S] = torch.from_numpy(np.array(x)).to(dev)
    slot = (A.frame_bytes(codec, nc, B) + 3) & ~3
    slots = torch.full((n, slot + PAD), A.FILL, dtype=torch.uint8, device=dev)
    sizes = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rec = torch.zeros((n, nc, S), dtype=torch.int16, device=dev)
    st = torch.zeros((n * nc, 16), dtype=torch.uint8, device=dev)
    cur = torch.cuda.current_stream(dev)
    s = torch.cuda.Stream(dev) if side else cur
    if side:
        s.wait_stream(cur)
    rc = enc._lib.mobi_audio_enc_async(enc._h, s.cuda_stream, n, padded.data_ptr(), S + PAD, B, slots.data_ptr(), slot + PAD, slot, sizes.data_ptr(),
                                       rec.data_ptr() if recon else None, S, st.data_ptr() if stats else None)
    assert rc == 0
    s.synchronize()
    enc.close()
    return slots.cpu().numpy(), sizes.cpu().numpy(), rec.cpu().numpy(), st.cpu().numpy().view(A.STATS_DTYPE).ravel()


def _check(codec, x, got, recon=True, stats=True):
    slots, sizes, rec, st = got
    frames, want_rec, want_st = A.encode_batch(codec, x)
    for s, f in enumerate(frames):
        assert int(sizes[s]) == len(f), (s, int(sizes[s]), len(f))
        assert slots[s, :len(f)].tobytes() == f, f"stream {s}: the frame differs from the model"
        assert (slots[s, len(f):] == A.FILL).all(), f"stream {s}: a byte behind the frame was written"
    if recon:
        assert np.array_equal(rec, want_rec)
    if stats:
        assert np.array_equal(st, want_st), (st, want_st)


@pytest.mark.parametrize("codec", (A.IMA, A.PCM16))
@pytest.mark.parametrize("offset", range(len(A.SIGNALS)))
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_model(shape, offset, codec):
    x = A.batch(*shape, offset=offset)
    _check(codec, x, _abi(codec, x))


@pytest.mark.parametrize("codec", (A.IMA, A.PCM16))
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_model_on_a_side_stream(shape, codec):
    x = A.batch(*shape, offset=3)
    _check(codec, x, _abi(codec, x, side=True))


def test_on_a_side_stream_and_without_recon_and_stats():
    x = A.batch(3, 2, 2)
    full = _abi(A.IMA, x, side=True)
    _check(A.IMA, x, full)
    for recon, stats in ((False, False), (True, False), (False, True)):
        got = _abi(A.IMA, x, recon=recon, stats=stats)
        _check(A.IMA, x, got, recon, stats)
        assert np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1])
        if not recon:
            assert not got[2].any()
        if not stats:
            assert not got[3].view(np.uint8).any()
    pcm = _abi(A.PCM16, x, recon=False, stats=False)
    _check(A.PCM16, x, pcm, False, False)


@pytest.mark.parametrize("codec", ("ima", "pcm16"))
@pytest.mark.parametrize("shape,offset", [((3, 2, 2), 0), ((3, 2, 2), 3), ((33, 2, 3), 0), ((2, 8, 1), 4)] + [((2, 1, 3), o) for o in range(7)])
def test_the_gpu_decoder_returns_the_reconstruction(shape, offset, codec):
    import mobiclipdecoder_amd as m
    n, nc, B = shape
    S = 256 * B
    dev = _dev()
    x = A.batch(n, nc, B, offset=offset)
    rows = torch.zeros((n, nc, S + 100), dtype=torch.int16, device=dev)  # what a decode call with max_samples = S + 100 leaves
    rows[:, :, :S] = torch.from_numpy(np.array(x)).to(dev)
    enc = m.MobiclipAudioEncoder(n, nc, codec, B)
    frames, sizes, ex = enc.encode(rows[:, :, :S], recon=True, stats=True)
    plain = enc.encode(rows[:, :, :S])
    torch.cuda.synchronize()
    assert len(plain) == 2 and torch.equal(plain[0], frames) and torch.equal(plain[1], sizes)
    enc.close()
    cid = A.IMA if codec == "ima" else A.PCM16
    want, want_rec, want_st = A.encode_batch(cid, x)
    host, ln = frames.cpu().numpy(), sizes.cpu().numpy()
    data = [host[s, :ln[s]].tobytes() for s in range(n)]
    assert data == want
    assert np.array_equal(ex["recon"].cpu().numpy(), want_rec) and np.array_equal(ex["stats"].cpu().numpy().view(A.STATS_DTYPE).ravel(), want_st)
    dec = m.MobiclipAudio(n, nc, codec, "moflex")
    out, n_samples, rc = dec.decode([d + b"\x00\x00" for d in data])
    torch.cuda.synchronize()
    dec.close()
    extra = 1 if codec == "pcm16" and nc == 1 else 0  # the appended zero bytes are one more sample: documented, not worked round
    assert not rc.any() and (n_samples == S + extra).all()
    assert torch.equal(out[:, :, :S], ex["recon"])
    if extra:
        assert not out[:, :, S].any()


def test_python_refusals():
    import mobiclipdecoder_amd as m
    dev = _dev()
    enc = m.MobiclipAudioEncoder(2, 2, "ima", 2)
    ok = torch.zeros((2, 2, 512), dtype=torch.int16, device=dev)
    for bad in (ok[:, :1], ok[:, :, :300], torch.zeros((3, 2, 512), dtype=torch.int16, device=dev), torch.zeros((2, 2, 768), dtype=torch.int16, device=dev),
                ok.to(torch.int32), ok.cpu(), ok[:, :, ::2], ok.cpu().numpy()):
        with pytest.raises(ValueError):
            enc.encode(bad)
    with pytest.raises(ValueError):
        enc.encode(ok, slot_bytes=516)
    with pytest.raises(ValueError):
        enc.encode(ok, slot_bytes=522)
    frames, sizes = enc.encode(ok[:1, :, :256], slot_bytes=1024)
    torch.cuda.synchronize()
    assert tuple(frames.shape) == (1, 1024) and sizes.tolist() == [264]
    # the entry point's own refusals, with a live object: nothing is enqueued
    s = torch.cuda.current_stream(dev).cuda_stream
    slots, ln = torch.zeros((2, 520), dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    call = lambda n=2, pitch=512, blocks=2, slot=520: enc._lib.mobi_audio_enc_async(enc._h, s, n, ok.data_ptr(), pitch, blocks, slots.data_ptr(), slot, slot, ln.data_ptr(), None, 0, None)
    assert call() == 0
    assert call(n=3) == A.E_ARG and call(blocks=3) == A.E_ARG and call(pitch=511) == A.E_ARG and call(slot=516) == A.E_ARG
    torch.cuda.synchronize()
    enc.close()
    with pytest.raises(m.MobiclipError, match="closed"):
        enc.encode(ok)
