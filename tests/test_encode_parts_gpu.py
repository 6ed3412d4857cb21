"""The inter encoder's partition mode on the GPU (include/mobiclip_encode_parts.h, csrc/mobi_encode_parts.hip) against its host model
(tests/enc_parts_model.py), which tests/test_encode_parts_model.py has judged by the oracle and by an independent re-derivation.

  a  mode 1: slots (the zeros behind each stream included), bytes_out, recon_i420 and every field of stats, reserved included, equal the
     host model's byte for byte, for both versions, with device pointers on torch's stream and through the host entry point
  b  one context switched 1 -> 0 -> 1 gives mode-0 bytes, then mode-1 bytes again
  c  the I + 3 P chain fed frame by frame to MobiclipBatch gives export_tensor("i420") equal to the reported reconstruction, and
     export_motion("cells") of each P-frame has in every 2x2 cell the model's vector of the quadrant it lies in, and ref 1
  d  guard bytes around slots, reconstruction and stats stay untouched; a slot too small for the longest stream alone stays zero with
     the length true; a non-default stream and pitches above the minimum work
  e  encode_clips(partitions=True) on a decoded generated clip decodes to its own reconstructions"""
import numpy as np
import pytest
import torch

from tests import enc_inter_model as M
from tests import enc_parts_model as Q

pytestmark = pytest.mark.gpu
_CACHE = {}


def model(W, H, name, version, mode=1):
    key = (W, H, name, version, mode)
    if key not in _CACHE:
        frames, qs = Q.sequence_sets(W, H)[name]
        _CACHE[key] = (frames, qs, Q.chain(W, H, version, mode, frames, qs))
    return _CACHE[key]


def _dev():
    from mobiclipdecoder_amd.decoder import default_device
    return torch.device("cuda", default_device())


def _same(got_streams, got_bytes, got_recon, got_stats, want, where):
    assert np.array_equal(got_bytes, want["bytes"]), where
    assert np.array_equal(got_streams, want["streams"]), where
    assert np.array_equal(got_recon, want["recon"]), where
    for f in Q.STATS_DTYPE.names:
        assert np.array_equal(got_stats[f], want["stats"][f]), (where, f)


@pytest.mark.parametrize("version", Q.VERSIONS)
@pytest.mark.parametrize("W,H", Q.SHAPES)
def test_bit_exact_against_the_host_model(W, H, version):
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.encode_inter import STATS_DTYPE
    enc = m.MobiclipInterEncoder(W, H, version, 5, partitions=True)
    dev = _dev()
    split = 0
    for name in Q.SETS:
        frames, qs, ch = model(W, H, name, version)
        for t in range(1, Q.T):
            want, refs = ch[t], ch[t - 1]["recon"]
            slot = want["streams"].shape[1]
            assert slot == enc.stream_bound
            streams, sizes, ex = enc.encode(torch.from_numpy(frames[:, t].copy()).to(dev), torch.from_numpy(refs).to(dev), qs[:, t - 1], qs[:, t], recon=True,
                                            stats=True, slot_bytes=slot)
            st = ex["stats"].cpu().numpy().view(STATS_DTYPE).reshape(-1)
            _same(streams.cpu().numpy(), sizes.cpu().numpy(), ex["recon"].cpu().numpy(), st, want, (name, t, "device"))
            assert np.array_equal(st["reserved"][:, Q.STAT_SPLIT], (want["mbs"]["luma_mode"] != 0).sum(1))
            split += int(st["reserved"][:, Q.STAT_SPLIT].sum())
        lst, ex = enc.encode(frames[:, Q.T - 1], ch[Q.T - 2]["recon"], qs[:, Q.T - 2], qs[:, Q.T - 1], recon=True, stats=True, slot_bytes=slot)
        _same(ex["slots"], ex["sizes"], ex["recon"], ex["stats"], ch[Q.T - 1], (name, "host"))
        assert lst == [ch[Q.T - 1]["streams"][i, : ch[Q.T - 1]["bytes"][i]].tobytes() for i in range(frames.shape[0])]
    assert split > 0
    enc.close()


@pytest.mark.parametrize("version", Q.VERSIONS)
def test_mode_switching(version):
    import mobiclipdecoder_amd as m
    W, H, name, t = 64, 48, "half_seams", 2
    frames, qs, ch1 = model(W, H, name, version, 1)
    refs = ch1[t - 1]["recon"]
    want = {1: ch1[t], 0: Q.host_encode(W, H, version, 0, frames[:, t], refs, qs[:, t - 1], qs[:, t])}
    assert not np.array_equal(want[0]["bytes"], want[1]["bytes"])
    enc = m.MobiclipInterEncoder(W, H, version, 4)
    assert enc.partitions is False and enc.stream_bound == M.host().encp_host_bound(W, H)
    for mode in (1, 0, 1):
        enc.set_partitions(bool(mode))
        assert enc.partitions is bool(mode) and enc.stream_bound == want[mode]["streams"].shape[1]
        lst, ex = enc.encode(frames[:, t], refs, qs[:, t - 1], qs[:, t], recon=True, stats=True, slot_bytes=enc.stream_bound)
        _same(ex["slots"], ex["sizes"], ex["recon"], ex["stats"], want[mode], (mode,))
        assert bool(ex["stats"]["reserved"].any()) == bool(mode)
    enc.close()
    with pytest.raises(m.MobiclipError):
        enc.set_partitions(True)


@pytest.mark.parametrize("version", Q.VERSIONS)
@pytest.mark.parametrize("W,H", Q.SHAPES)
def test_chain_decodes_on_the_gpu_with_the_encoders_motion(W, H, version):
    import mobiclipdecoder_amd as m
    dev = _dev()
    mbw, mbh = W // 16, H // 16
    for name in Q.NEW_SETS + ("mixed5",):
        frames, qs, ch = model(W, H, name, version)
        n = frames.shape[0]
        intra, inter = m.MobiclipIntraEncoder(W, H, version, n), m.MobiclipInterEncoder(W, H, version, n, partitions=True)
        b = m.MobiclipBatch(n, W, H, version)
        b.set_motion(True)
        ref = None
        for t in range(Q.T):
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
            cells = b.export_motion("cells")[0] if t else None
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), ex["recon"]), (name, t)
            if t:
                # the decoder's own motion field: every 2x2 cell of quadrant qd of macroblock i holds the model's vector of that quadrant
                dx4, dy4 = M.unpack_mv(ch[t]["mv4"])
                quad = lambda a: np.kron(a.reshape(n, mbh, mbw, 2, 2).transpose(0, 1, 3, 2, 4).reshape(n, 2 * mbh, 2 * mbw), np.ones((4, 4), np.int64))
                cells = cells.cpu().numpy()
                assert np.array_equal(cells[:, 0], quad(dx4)) and np.array_equal(cells[:, 1], quad(dy4)), (name, t)
                assert (cells[:, 2] == 1).all(), (name, t)
        for o in (b, intra, inter):
            o.close()


def test_guards_stream_and_pitches():
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd import encode_inter
    W, H, version = 48, 32, 2
    frames, qs, ch = model(W, H, "half_seams", version)
    want, n, F = ch[2], frames.shape[0], frames.shape[2]
    order = np.argsort(want["bytes"])
    slot = (int(want["bytes"][order[-1]]) - 2) // 4 * 4  # too small for the longest stream alone
    assert want["bytes"][order[-2]] <= slot < want["bytes"][order[-1]]
    enc = m.MobiclipInterEncoder(W, H, version, 5, partitions=True)
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
    gs = gst[guard: guard + n * 64].view(Q.STATS_DTYPE).reshape(-1)
    for f in Q.STATS_DTYPE.names:
        assert np.array_equal(gs[f], want["stats"][f]), f
    enc.close()


def test_encode_clips_with_partitions_transcode_loop():
    """generated clip -> MobiclipBatch -> export_tensor("i420") -> encode_clips(partitions=True) -> MobiclipBatch: the encoder's own
    reconstructions; the streams differ from the unsplit mode's"""
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.streamgen import BASE_SEED
    T = 4
    p = m.default_params("A", BASE_SEED + 78, n_frames=T)
    data, fo = m.generate_clip(p)
    dec = m.MobiclipBatch(1, p.width, p.height, p.version)
    frames = []
    for f in range(T):
        rcs, _ = dec.decode([data[fo[f]:fo[f + 1]]], [0])
        assert rcs == [0]
        frames.append(dec.export_tensor("i420")[0, 0].clone())
    clips = torch.stack(frames)[None]
    streams, recon = m.encode_clips(clips, 24, 4, p.version, p.width, p.height, recon=True, partitions=True)
    plain = m.encode_clips(clips, 24, 4, p.version, p.width, p.height)
    assert streams[0][0] == plain[0][0] and streams[0][1:] != plain[0][1:]
    again = m.MobiclipBatch(1, p.width, p.height, p.version)
    for t in range(T):
        rcs, _ = again.decode([streams[0][t]], [0])
        assert rcs == [0], (t, rcs)
        got = again.export_tensor("i420")[0]
        torch.cuda.synchronize()
        assert torch.equal(got, recon[:, t]), t
    for o in (dec, again):
        o.close()
