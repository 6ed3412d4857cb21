"""The inter encoder on the GPU (include/mobiclip_encode_inter.h, csrc/mobi_encode_inter.hip) against its host model
(tests/enc_inter_model.py), which tests/test_encode_inter_model.py has judged by the oracle and by an independent re-derivation.

  7   slots (the zeros behind each stream included), bytes_out, recon_i420, every field of stats and -- through the partition codes and
      vector differences in the streams -- v* equal the host model's byte for byte, for both versions, with device pointers and through
      the host entry point
  8   the I + 3 P chain fed frame by frame to MobiclipBatch gives get_planes / export_tensor("i420") equal to the reported reconstruction
  9   encode_clips on a decoded generated clip (gop = 4 over 8 frames) decodes to its own reconstructions
  10  guard bytes around slots, reconstruction and stats stay untouched; a non-default stream and pitches above the minimum work"""
import numpy as np
import pytest
import torch

from tests import enc_inter_model as M
from tests import enc_model as E

pytestmark = pytest.mark.gpu
_CACHE = {}


def model(W, H, name, version):
    key = (W, H, name, version)
    if key not in _CACHE:
        frames, qs = M.sequence_sets(W, H)[name]
        _CACHE[key] = (frames, qs, M.chain(W, H, version, frames, qs))
    return _CACHE[key]


def _dev():
    from mobiclipdecoder_amd.decoder import default_device
    return torch.device("cuda", default_device())


def _same(got_streams, got_bytes, got_recon, got_stats, want, where):
    assert np.array_equal(got_bytes, want["bytes"]), where
    assert np.array_equal(got_streams, want["streams"]), where
    assert np.array_equal(got_recon, want["recon"]), where
    for f in M.STATS_DTYPE.names:
        assert np.array_equal(got_stats[f], want["stats"][f]), (where, f)


@pytest.mark.parametrize("version", M.VERSIONS)
@pytest.mark.parametrize("W,H", M.SHAPES)
def test_bit_exact_against_the_host_model(W, H, version):
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.encode_inter import STATS_DTYPE
    enc = m.MobiclipInterEncoder(W, H, version, 5)
    dev = _dev()
    for name in M.SETS:
        frames, qs, ch = model(W, H, name, version)
        for t in range(1, M.T):
            want, refs = ch[t], ch[t - 1]["recon"]
            slot = want["streams"].shape[1]
            assert slot == enc.stream_bound
            # device pointers, torch's current stream, nothing waited for until the copies below
            streams, sizes, ex = enc.encode(torch.from_numpy(frames[:, t].copy()).to(dev), torch.from_numpy(refs).to(dev), qs[:, t - 1], qs[:, t], recon=True,
                                            stats=True, slot_bytes=slot)
            _same(streams.cpu().numpy(), sizes.cpu().numpy(), ex["recon"].cpu().numpy(), ex["stats"].cpu().numpy().view(STATS_DTYPE).reshape(-1), want,
                  (name, t, "device"))
            # the vectors the streams carry are the model's v* (its streams were parsed back in tests/test_encode_inter_model.py; here the
            # bytes are equal, so are they), and the statistics count them alike
            dx, dy = M.unpack_mv(want["mv"])
            st = ex["stats"].cpu().numpy().view(STATS_DTYPE).reshape(-1)
            assert np.array_equal(st["nonzero_mv"], ((dx != 0) | (dy != 0)).sum(1)) and np.array_equal(st["halfpel_mv"], (((dx | dy) & 1) != 0).sum(1))
        # the host entry point, once per set
        lst, ex = enc.encode(frames[:, M.T - 1], ch[M.T - 2]["recon"], qs[:, M.T - 2], qs[:, M.T - 1], recon=True, stats=True, slot_bytes=slot)
        _same(ex["slots"], ex["sizes"], ex["recon"], ex["stats"], ch[M.T - 1], (name, "host"))
        assert lst == [ch[M.T - 1]["streams"][i, : ch[M.T - 1]["bytes"][i]].tobytes() for i in range(frames.shape[0])]
    enc.close()


@pytest.mark.parametrize("version", M.VERSIONS)
@pytest.mark.parametrize("W,H", M.SHAPES)
def test_chain_decodes_on_the_gpu_to_the_reconstruction(W, H, version):
    """I, P, P, P of every clip of a set, encoded on the GPU frame by frame (each P-frame from the reconstruction the call before
    reported, on the device) and fed frame by frame to MobiclipBatch"""
    import mobiclipdecoder_amd as m
    dev = _dev()
    for name in M.SETS:
        frames, qs, ch = model(W, H, name, version)
        n = frames.shape[0]
        intra, inter = m.MobiclipIntraEncoder(W, H, version, n), m.MobiclipInterEncoder(W, H, version, n)
        b = m.MobiclipBatch(n, W, H, version)
        ref = None
        for t in range(M.T):
            pics = torch.from_numpy(frames[:, t].copy()).to(dev)
            if t == 0:
                streams, ex = intra.encode(pics, qs[:, 0], recon=True)
            else:
                streams, ex = inter.encode(pics, ref, qs[:, t - 1], qs[:, t], recon=True)
            assert np.array_equal(ex["recon"], ch[t]["recon"]), (name, t)
            ref = torch.from_numpy(ex["recon"]).to(dev)
            rcs, offs = b.decode(streams, [0] * n)
            assert rcs == [0] * n, (name, t, rcs)
            assert all(o <= len(s) for o, s in zip(offs, streams))
            got = b.export_tensor("i420")[0]
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), ex["recon"]), (name, t)
            y, uv = b.planes(0)
            S = y.shape[1]
            assert np.array_equal(E._i420(y[:, :W], uv[:, : W // 2], uv[:, S // 2: S // 2 + W // 2]), ex["recon"][0]), (name, t)
        for o in (b, intra, inter):
            o.close()


def test_encode_clips_transcode_loop():
    """generated clip -> MobiclipBatch -> export_tensor("i420") -> encode_clips (gop = 4 over 8 frames) -> MobiclipBatch: the encoder's own
    reconstructions"""
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.streamgen import BASE_SEED
    T = 8
    p = m.default_params("A", BASE_SEED + 78, n_frames=T)
    assert (p.width, p.height) == (256, 192)
    data, fo = m.generate_clip(p)
    dec = m.MobiclipBatch(1, p.width, p.height, p.version)
    frames = []
    for f in range(T):
        rcs, _ = dec.decode([data[fo[f]:fo[f + 1]]], [0])
        assert rcs == [0]
        frames.append(dec.export_tensor("i420")[0, 0].clone())
    clip = torch.stack(frames)
    clips = torch.stack([clip, clip.flip(0)])  # two clips: the second runs backwards
    qs = [20, 20, 24, 24, 30, 28, 28, 28]
    streams, recon = m.encode_clips(clips, qs, 4, p.version, p.width, p.height, recon=True)
    assert len(streams) == 2 and all(len(s) == T for s in streams) and tuple(recon.shape) == (2, T, clip.shape[1])
    again = m.MobiclipBatch(2, p.width, p.height, p.version)
    for t in range(T):
        rcs, _ = again.decode([streams[0][t], streams[1][t]], [0, 0])
        assert rcs == [0, 0], (t, rcs)
        got = again.export_tensor("i420")[0]
        torch.cuda.synchronize()
        assert torch.equal(got, recon[:, t]), t
        assert (streams[0][t][1] >> 7) == (1 if t % 4 == 0 else 0)  # the frame-type bit: the top of the first little-endian 16-bit word
    # it is an encoding of those pictures: at q = 20 the reconstruction is close to its source
    err = (recon[0, 1].to(torch.int32) - clips[0, 1].to(torch.int32)).abs().float().mean().item()
    assert err < 4.0, err
    for o in (dec, again):
        o.close()


def test_guards_stream_and_pitches():
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd import encode_inter
    W, H, version = 48, 32, 2
    frames, qs, ch = model(W, H, "mixed5", version)
    want, n, F = ch[2], frames.shape[0], frames.shape[2]
    order = np.argsort(want["bytes"])
    slot = (int(want["bytes"][order[-1]]) - 2) // 4 * 4  # too small for the longest stream alone
    assert want["bytes"][order[-2]] <= slot < want["bytes"][order[-1]]
    enc = m.MobiclipInterEncoder(W, H, version, 5)
    dev = _dev()
    guard = 64
    pitch, rpitch = F + 24, F + 40
    pics = torch.full((n, pitch), 0x55, dtype=torch.uint8, device=dev)
    refs = torch.full((n, rpitch), 0x33, dtype=torch.uint8, device=dev)
    pics[:, :F], refs[:, :F] = torch.from_numpy(frames[:, 2].copy()).to(dev), torch.from_numpy(ch[1]["recon"]).to(dev)
    buf = torch.full((guard + n * slot + guard,), 0xC3, dtype=torch.uint8, device=dev)
    rec = torch.full((guard + n * F + guard,), 0xC3, dtype=torch.uint8, device=dev)
    st = torch.full((guard + n * 64 + guard,), 0xC3, dtype=torch.uint8, device=dev)
    sizes = torch.full((n + 2,), -7, dtype=torch.int32, device=dev)
    pq, q = np.ascontiguousarray(qs[:, 1]), np.ascontiguousarray(qs[:, 2])
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    rc = encode_inter._lib().mobi_enc_inter_async(enc._h, side.cuda_stream, n, pics.data_ptr(), pitch, refs.data_ptr(), rpitch, pq.ctypes.data, q.ctypes.data,
                                                 buf.data_ptr() + guard, slot, sizes.data_ptr() + 4, rec.data_ptr() + guard, st.data_ptr() + guard)
    assert rc == 0
    side.synchronize()
    got, sz, grec, gst = buf.cpu().numpy(), sizes.cpu().numpy(), rec.cpu().numpy(), st.cpu().numpy()
    for g_, body in ((got, n * slot), (grec, n * F), (gst, n * 64)):
        assert (g_[:guard] == 0xC3).all() and (g_[guard + body:] == 0xC3).all()
    assert sz[0] == -7 and sz[-1] == -7 and np.array_equal(sz[1:-1], want["bytes"])
    slots = got[guard: guard + n * slot].reshape(n, slot)
    for i in range(n):
        if i == order[-1]:
            assert not slots[i].any()
        else:
            assert np.array_equal(slots[i], want["streams"][i, :slot])
    assert np.array_equal(grec[guard: guard + n * F].reshape(n, F), want["recon"])
    gs = gst[guard: guard + n * 64].view(M.STATS_DTYPE).reshape(-1)
    for f in M.STATS_DTYPE.names:
        assert np.array_equal(gs[f], want["stats"][f]), f
    # the Python form: the true size comes back, the stream does not; n = 1 on an encoder created for 5; refusals raise
    lst, ex = enc.encode(frames[:, 2], ch[1]["recon"], pq, q, slot_bytes=slot)
    assert lst[order[-1]] == b"" and ex["sizes"][order[-1]] == want["bytes"][order[-1]]
    one = enc.encode(torch.from_numpy(frames[3:4, 2].copy()).to(dev), torch.from_numpy(ch[1]["recon"][3:4]).to(dev), int(pq[3]), int(q[3]))
    assert one == [want["streams"][3, : want["bytes"][3]].tobytes()]
    with pytest.raises(m.MobiclipError):
        enc.encode(frames[:1, 2], ch[1]["recon"][:1], 11, 30)
    with pytest.raises(m.MobiclipError):
        enc.encode(np.concatenate([frames[:, 2], frames[:1, 2]]), np.concatenate([ch[1]["recon"], ch[1]["recon"][:1]]), 30, 30)  # six pictures
    enc.close()
