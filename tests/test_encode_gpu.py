"""The intra encoder on the GPU (include/mobiclip_encode.h, csrc/mobi_encode.hip) against its host model (tests/enc_model.py), which
tests/test_encode_model.py has judged by the oracle and by an independent re-derivation of every decision.

  7   streams (whole slots, the zeros behind each stream included), bytes_out, recon_i420 and every field of stats equal the host
      model's byte for byte, with device pointers on torch's current stream and through the host entry point
  8   the streams decoded by MobiclipBatch give export_tensor("i420") == recon_i420
  9   decode a generated clip, export_tensor("i420") straight into encode, decode again: the encoder's reconstruction
  10  a slot too small for its stream is zero, its bytes_out the true length, the others unaffected; guard bytes stay untouched
  11  n = max_pictures and n = 1 on an encoder created for 5"""
import numpy as np
import pytest
import torch

from tests import enc_model as E

pytestmark = pytest.mark.gpu
SETS = ("mixed5", "sat_q52", "sat_q12", "hard5")
_CACHE = {}


def model(W, H, name):
    key = (W, H, name)
    if key not in _CACHE:
        pics, qs = E.picture_sets(W, H)[name]
        _CACHE[key] = (pics, qs, E.host_encode(W, H, 2, pics, qs))
    return _CACHE[key]


def _dev():
    from mobiclipdecoder_amd.decoder import default_device
    return torch.device("cuda", default_device())


def _same(got_streams, got_bytes, got_recon, got_stats, want, where):
    assert np.array_equal(got_bytes, want["bytes"]), where
    assert np.array_equal(got_streams, want["streams"]), where
    assert np.array_equal(got_recon, want["recon"]), where
    for f in E.STATS_DTYPE.names:
        assert np.array_equal(got_stats[f], want["stats"][f]), (where, f)


@pytest.mark.parametrize("version", E.VERSIONS)
@pytest.mark.parametrize("W,H", E.SHAPES)
def test_bit_exact_against_the_host_model(W, H, version):
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.encode import STATS_DTYPE
    enc = m.MobiclipIntraEncoder(W, H, version, 5)
    for name in SETS:
        pics, qs, want = model(W, H, name)
        slot = want["streams"].shape[1]
        assert slot == enc.stream_bound
        # device pointers, torch's current stream, nothing waited for until the copies below
        t = torch.from_numpy(pics).to(_dev())
        streams, sizes, ex = enc.encode(t, qs, recon=True, stats=True, slot_bytes=slot)
        _same(streams.cpu().numpy(), sizes.cpu().numpy(), ex["recon"].cpu().numpy(), ex["stats"].cpu().numpy().view(STATS_DTYPE).reshape(-1), want,
              (name, "device"))
        # the host entry point
        lst, ex = enc.encode(pics, qs, recon=True, stats=True, slot_bytes=slot)
        _same(ex["slots"], ex["sizes"], ex["recon"], ex["stats"], want, (name, "host"))
        assert lst == [want["streams"][i, : want["bytes"][i]].tobytes() for i in range(len(qs))]
    enc.close()


@pytest.mark.parametrize("version", E.VERSIONS)
@pytest.mark.parametrize("W,H", E.SHAPES)
def test_streams_decode_on_the_gpu_to_the_reconstruction(W, H, version):
    import mobiclipdecoder_amd as m
    enc = m.MobiclipIntraEncoder(W, H, version, 5)
    for name in SETS:
        pics, qs, _ = model(W, H, name)
        streams, ex = enc.encode(torch.from_numpy(pics).to(_dev()), qs, recon=True)
        b = m.MobiclipBatch(len(qs), W, H, version)
        rcs, offs = b.decode(streams, [0] * len(qs))
        assert rcs == [0] * len(qs), (name, rcs)
        assert all(o <= len(s) for o, s in zip(offs, streams))
        got = b.export_tensor("i420")[0]
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), ex["recon"]), name
        b.close()
    enc.close()


def test_transcode_loop():
    """generated clip -> MobiclipBatch -> export_tensor("i420") -> encode -> MobiclipBatch: the encoder's reconstruction, no picture on the host"""
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.streamgen import BASE_SEED
    p = m.default_params("A", BASE_SEED + 77, n_frames=3)
    assert (p.width, p.height) == (256, 192)
    data, fo = m.generate_clip(p)
    dec = m.MobiclipBatch(1, p.width, p.height, p.version)
    frames = []
    for f in range(p.n_frames):
        rcs, _ = dec.decode([data[fo[f]:fo[f + 1]]], [0])
        assert rcs == [0]
        frames.append(dec.export_tensor("i420")[0, 0].clone())
    pictures = torch.stack(frames)
    enc = m.MobiclipIntraEncoder(p.width, p.height, p.version, p.n_frames)
    streams, sizes, ex = enc.encode(pictures, [18, 30, 44], recon=True, slot_bytes=enc.stream_bound)
    sizes = sizes.cpu().numpy()
    again = m.MobiclipBatch(p.n_frames, p.width, p.height, p.version)
    host = streams.cpu().numpy()
    rcs, _ = again.decode([host[i, : sizes[i]].tobytes() for i in range(p.n_frames)], [0] * p.n_frames)
    assert rcs == [0] * p.n_frames
    got = again.export_tensor("i420")[0]
    torch.cuda.synchronize()
    assert torch.equal(got, ex["recon"])
    # and it is an encoding of those pictures, not of something else: at q = 18 the reconstruction is close to its source
    err = (ex["recon"][0].to(torch.int32) - pictures[0].to(torch.int32)).abs().float().mean().item()
    assert err < 4.0, err
    for o in (dec, again, enc):
        o.close()


def test_slots_and_guards():
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd import encode
    W, H = 48, 32
    pics, qs, want = model(W, H, "mixed5")
    n = len(qs)
    order = np.argsort(want["bytes"])
    slot = (int(want["bytes"][order[-1]]) - 2) // 4 * 4  # too small for the longest stream alone
    assert want["bytes"][order[-2]] <= slot < want["bytes"][order[-1]]
    enc = m.MobiclipIntraEncoder(W, H, 2, 5)
    dev = _dev()
    guard = 64
    buf = torch.full((guard + n * slot + guard,), 0xC3, dtype=torch.uint8, device=dev)
    sizes = torch.full((n + 2,), -7, dtype=torch.int32, device=dev)
    t = torch.from_numpy(pics).to(dev)
    rc = encode._lib().mobi_enc_intra_async(enc._h, torch.cuda.current_stream(dev).cuda_stream, n, t.data_ptr(), t.shape[1], qs.ctypes.data, 0,
                                           buf.data_ptr() + guard, slot, sizes.data_ptr() + 4, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    got, sz = buf.cpu().numpy(), sizes.cpu().numpy()
    assert (got[:guard] == 0xC3).all() and (got[guard + n * slot:] == 0xC3).all()
    assert sz[0] == -7 and sz[-1] == -7 and np.array_equal(sz[1:-1], want["bytes"])
    slots = got[guard: guard + n * slot].reshape(n, slot)
    for i in range(n):
        if i == order[-1]:
            assert not slots[i].any()
        else:
            assert np.array_equal(slots[i], want["streams"][i, :slot])
    # the Python form of the same: the true size comes back, the stream does not
    lst, ex = enc.encode(pics, qs, slot_bytes=slot)
    assert lst[order[-1]] == b"" and ex["sizes"][order[-1]] == want["bytes"][order[-1]]
    enc.close()


def test_creation_limits():
    import mobiclipdecoder_amd as m
    W, H = 48, 32
    pics, qs, want = model(W, H, "hard5")
    enc = m.MobiclipIntraEncoder(W, H, 1, 5)
    five = enc.encode(torch.from_numpy(pics).to(_dev()), qs)
    one = enc.encode(torch.from_numpy(pics[3:4]).to(_dev()), int(qs[3]))
    assert five == [want["streams"][i, : want["bytes"][i]].tobytes() for i in range(5)] and one == [five[3]]
    with pytest.raises(m.MobiclipError):
        enc.encode(np.concatenate([pics, pics[:1]]), 30)  # six pictures
    with pytest.raises(m.MobiclipError):
        enc.encode(pics[:1], 11)
    enc.close()
