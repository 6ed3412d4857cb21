"""The inter encoder's intra mode on the GPU (include/mobiclip_encode_pintra.h, csrc/mobi_encode_pintra.hip) against its host model
(tests/enc_pintra_model.py), which tests/test_encode_pintra_model.py has judged by the oracle and by an independent re-derivation.

  a  slots (the zeros behind each stream included), bytes_out, recon_i420 and every field of stats, reserved included, equal the host
     model's byte for byte, for all sets, shapes and versions, with device pointers on torch's stream and through the host entry point
  b  one context switched 1 -> 0 -> 1 gives intra-mode bytes, mode-0 bytes, then intra-mode bytes again; the two modes refuse each other
  c  the I + 3 P chain fed frame by frame to MobiclipBatch: export_tensor("i420") equals the reported reconstruction, export_motion("mb")
     gives every macroblock the type the model's flag says, export_motion("cells") the model's vector with ref 1 in inter macroblocks
  d  guard bytes around slots, reconstruction and stats stay untouched; a slot too small for the longest stream alone stays zero with
     the length true; a non-default stream and pitches above the minimum work
  e  encode_target in the mode equals a Python bisection of the rate rule over the host model's fixed-quantiser encodes
  f  encode_clips(intra=True) on a clip with a cut at a non-key frame decodes in MobiclipBatch to its own reconstructions, is shorter in
     total than intra=False and identical to it up to the cut"""
import numpy as np
import pytest
import torch

from tests import enc_inter_model as M
from tests import enc_model as E
from tests import enc_pintra_model as PI
from tests import enc_rate_model as R

pytestmark = pytest.mark.gpu
_CACHE = {}


def model(W, H, name, version, mode=1):
    key = (W, H, name, version, mode)
    if key not in _CACHE:
        frames, qs = PI.sequence_sets(W, H)[name]
        _CACHE[key] = (frames, qs, PI.chain(W, H, version, mode, frames, qs))
    return _CACHE[key]


def _dev():
    from mobiclipdecoder_amd.decoder import default_device
    return torch.device("cuda", default_device())


def _same(got_streams, got_bytes, got_recon, got_stats, want, where):
    assert np.array_equal(got_bytes, want["bytes"]), where
    assert np.array_equal(got_streams, want["streams"]), where
    assert np.array_equal(got_recon, want["recon"]), where
    for f in PI.STATS_DTYPE.names:
        assert np.array_equal(got_stats[f], want["stats"][f]), (where, f)


@pytest.mark.parametrize("version", PI.VERSIONS)
@pytest.mark.parametrize("W,H", PI.SHAPES)
def test_bit_exact_against_the_host_model(W, H, version):
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.encode_inter import STAT_INTRA, STATS_DTYPE
    enc = m.MobiclipInterEncoder(W, H, version, 5, intra=True)
    assert enc.intra is True and enc.partitions is False
    dev = _dev()
    intra_n = 0
    for name in PI.SETS:
        frames, qs, ch = model(W, H, name, version)
        for t in range(1, PI.T):
            want, refs = ch[t], ch[t - 1]["recon"]
            slot = want["streams"].shape[1]
            assert slot == enc.stream_bound
            streams, sizes, ex = enc.encode(torch.from_numpy(frames[:, t].copy()).to(dev), torch.from_numpy(refs).to(dev), qs[:, t - 1], qs[:, t], recon=True,
                                            stats=True, slot_bytes=slot)
            st = ex["stats"].cpu().numpy().view(STATS_DTYPE).reshape(-1)
            _same(streams.cpu().numpy(), sizes.cpu().numpy(), ex["recon"].cpu().numpy(), st, want, (name, t, "device"))
            assert np.array_equal(st["reserved"][:, STAT_INTRA], PI.is_intra(want).sum(1))
            intra_n += int(st["reserved"][:, STAT_INTRA].sum())
        lst, ex = enc.encode(frames[:, PI.T - 1], ch[PI.T - 2]["recon"], qs[:, PI.T - 2], qs[:, PI.T - 1], recon=True, stats=True, slot_bytes=slot)
        _same(ex["slots"], ex["sizes"], ex["recon"], ex["stats"], ch[PI.T - 1], (name, "host"))
        assert lst == [ch[PI.T - 1]["streams"][i, : ch[PI.T - 1]["bytes"][i]].tobytes() for i in range(frames.shape[0])]
    assert intra_n > 0
    enc.close()


@pytest.mark.parametrize("version", PI.VERSIONS)
def test_mode_switching_and_mutual_refusal(version):
    import mobiclipdecoder_amd as m
    W, H, name, t = 48, 32, "uncover", 2
    frames, qs, ch1 = model(W, H, name, version, 1)
    refs = ch1[t - 1]["recon"]
    want = {1: ch1[t], 0: M.host_encode(W, H, version, frames[:, t], refs, qs[:, t - 1], qs[:, t])}
    assert (want[1]["bytes"] < want[0]["bytes"]).all()
    enc = m.MobiclipInterEncoder(W, H, version, 4)
    assert enc.intra is False
    for mode in (1, 0, 1):
        enc.set_intra(bool(mode))
        assert enc.intra is bool(mode) and enc.stream_bound == want[mode]["streams"].shape[1]
        lst, ex = enc.encode(frames[:, t], refs, qs[:, t - 1], qs[:, t], recon=True, stats=True, slot_bytes=enc.stream_bound)
        _same(ex["slots"], ex["sizes"], ex["recon"], ex["stats"], want[mode], (mode,))
        assert bool(ex["stats"]["reserved"].any()) == bool(mode)
    # either mode refuses to come on beside the other, and nothing changes
    with pytest.raises(m.MobiclipError):
        enc.set_partitions(True)
    assert enc.intra is True and enc.partitions is False
    enc.set_intra(False)
    enc.set_partitions(True)
    with pytest.raises(m.MobiclipError):
        enc.set_intra(True)
    assert enc.intra is False and enc.partitions is True
    enc.set_intra(False)  # turning off what is off is no refusal
    with pytest.raises(ValueError):
        m.MobiclipInterEncoder(W, H, version, 4, partitions=True, intra=True)
    with pytest.raises(ValueError):
        m.encode_clips(torch.zeros((1, 2, W * H * 3 // 2), dtype=torch.uint8, device=_dev()), 20, 2, version, W, H, partitions=True, intra=True)
    enc.close()
    with pytest.raises(m.MobiclipError):
        enc.set_intra(True)


@pytest.mark.parametrize("version", PI.VERSIONS)
@pytest.mark.parametrize("W,H", PI.SHAPES)
def test_chain_decodes_on_the_gpu_with_the_encoders_kinds_and_motion(W, H, version):
    import mobiclipdecoder_amd as m
    dev = _dev()
    mbw, mbh = W // 16, H // 16
    for name in PI.NEW_SETS + ("mixed5",):
        frames, qs, ch = model(W, H, name, version)
        n = frames.shape[0]
        intra, inter = m.MobiclipIntraEncoder(W, H, version, n), m.MobiclipInterEncoder(W, H, version, n, intra=True)
        b = m.MobiclipBatch(n, W, H, version)
        b.set_motion(True)
        ref = None
        for t in range(PI.T):
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
            cells, mb = (b.export_motion("cells")[0], b.export_motion("mb")[0]) if t else (None, None)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), ex["recon"]), (name, t)
            if t:
                flag = PI.is_intra(ch[t]).reshape(n, mbh, mbw)
                assert np.array_equal(mb.cpu().numpy()[:, 0], flag.astype(np.int32)), (name, t)
                dx, dy = M.unpack_mv(ch[t]["mv"])
                up = lambda a: np.kron(a.reshape(n, mbh, mbw), np.ones((8, 8), np.int64))
                cells, inter_c = cells.cpu().numpy(), ~up(flag).astype(bool)
                assert np.array_equal(cells[:, 0][inter_c], up(dx)[inter_c]) and np.array_equal(cells[:, 1][inter_c], up(dy)[inter_c]), (name, t)
                assert (cells[:, 2][inter_c] == 1).all() and (cells[:, 2][~inter_c] == 0).all(), (name, t)
        for o in (b, intra, inter):
            o.close()


def test_guards_stream_and_pitches():
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd import encode_inter
    W, H, version = 48, 32, 2
    frames, qs, ch = model(W, H, "uncover", version)
    want, n, F = ch[2], frames.shape[0], frames.shape[2]
    assert PI.is_intra(want).any() and not PI.is_intra(want).all()
    order = np.argsort(want["bytes"])
    slot = (int(want["bytes"][order[-1]]) - 2) // 4 * 4  # too small for the longest stream alone
    assert want["bytes"][order[-2]] <= slot < want["bytes"][order[-1]]
    enc = m.MobiclipInterEncoder(W, H, version, 5, intra=True)
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
    gs = gst[guard: guard + n * 64].view(PI.STATS_DTYPE).reshape(-1)
    for f in PI.STATS_DTYPE.names:
        assert np.array_equal(gs[f], want["stats"][f]), f
    enc.close()


def _rate_inputs(W, H, version):
    """frame 1 of the five clips of `cut` and `uncover` with the intra model's reconstruction at enc_rate_model.REF_Q of frame 0 as reference,
    and the bytes by quantiser of the mode's host model: (53, N), rows 12 .. 52 filled"""
    key = ("rate", W, H, version)
    if key not in _CACHE:
        sets = PI.sequence_sets(W, H)
        frames = np.concatenate([sets[k][0] for k in PI.NEW_SETS])
        n = frames.shape[0]
        pq = np.full(n, R.REF_Q, np.uint8)
        refs = E.host_encode(W, H, version, frames[:, 0], pq)["recon"]
        pics = np.ascontiguousarray(frames[:, 1])
        table = np.zeros((R.QMAX + 1, n), np.int64)
        for q in range(R.QMIN, R.QMAX + 1):
            table[q] = PI.fixed(W, H, version, pics, refs, pq, q)["bytes"]
        _CACHE[key] = (pics, refs, pq, table)
    return _CACHE[key]


@pytest.mark.parametrize("version", PI.VERSIONS)
@pytest.mark.parametrize("W,H", R.SHAPES)
def test_encode_target_is_the_bisection_over_the_host_model(W, H, version):
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.encode_inter import STATS_DTYPE
    pics, refs, pq, B = _rate_inputs(W, H, version)
    n, mid = pics.shape[0], (R.QMIN + R.QMAX) >> 1
    # the classes rotated over the pictures: ends at qmin (the longest stream fits), inside the range, at qmax (nothing fits)
    cls = {"qmin": lambda i: int(B[R.QMIN:R.QMAX + 1, i].max()), "inside": lambda i: int(B[mid - 2, i]), "qmax": lambda i: 0}
    names = list(cls)
    enc = m.MobiclipInterEncoder(W, H, version, n, intra=True)
    dev = _dev()
    seen = set()
    for r in range(len(names)):
        tg = np.array([cls[names[(i + r) % len(names)]](i) for i in range(n)], np.int32)
        want, q_want = PI.bisect(W, H, version, pics, refs, pq, tg)
        out, sizes, ex = enc.encode_target(torch.from_numpy(pics).to(dev), torch.from_numpy(refs).to(dev), torch.from_numpy(pq).to(dev), torch.from_numpy(tg).to(dev),
                                           R.QMIN, R.QMAX, recon=True, stats=True, slot_bytes=enc.stream_bound)
        torch.cuda.synchronize()
        assert np.array_equal(ex["quantizer"].cpu().numpy(), q_want), r
        _same(out.cpu().numpy(), sizes.cpu().numpy(), ex["recon"].cpu().numpy(), ex["stats"].cpu().numpy().view(STATS_DTYPE).reshape(-1), want, ("target", r))
        for i in range(n):
            c = names[(i + r) % len(names)]
            assert (c != "qmin" or q_want[i] == R.QMIN) and (c != "qmax" or q_want[i] == R.QMAX)
            seen.add("qmin" if q_want[i] == R.QMIN else "qmax" if q_want[i] == R.QMAX else "inside")
        assert PI.is_intra(want).any()
    assert seen == {"qmin", "inside", "qmax"}
    enc.close()


def test_encode_clips_with_a_cut_at_a_non_key_frame():
    """six frames, one key frame (gop 6): the first three of `fullpel` (no macroblock of which goes intra), then -- the cut -- three of
    unrelated smooth content in slow motion"""
    import mobiclipdecoder_amd as m
    W, H, version, cut, q = 48, 32, 2, 3, 26
    before = PI.sequence_sets(W, H)["fullpel"][0][0][:cut]
    after = M._smooth(W, H, [(40, 30), (41, 30), (41, 31)], 3)
    clip = np.concatenate([before, after])
    frames = torch.from_numpy(clip[None].copy()).to(_dev())
    T = clip.shape[0]
    streams, recon = m.encode_clips(frames, q, T, version, W, H, recon=True, intra=True)
    plain = m.encode_clips(frames, q, T, version, W, H)
    total = lambda s: sum(len(x) for x in s[0])
    print("intra=True", [len(x) for x in streams[0]], "intra=False", [len(x) for x in plain[0]])
    assert streams[0][:cut] == plain[0][:cut]  # identical up to the cut
    assert len(streams[0][cut]) < len(plain[0][cut]) and total(streams) < total(plain)
    ch = PI.chain(W, H, version, 1, clip[None], np.full((1, T), q, np.uint8))
    assert not any(PI.is_intra(ch[t]).any() for t in range(1, cut)) and PI.is_intra(ch[cut]).all()
    assert [bytes(ch[t]["streams"][0, : ch[t]["bytes"][0]]) for t in range(T)] == streams[0]
    b = m.MobiclipBatch(1, W, H, version)
    for t in range(T):
        rcs, _ = b.decode([streams[0][t]], [0])
        assert rcs == [0], (t, rcs)
        got = b.export_tensor("i420")[0]
        torch.cuda.synchronize()
        assert torch.equal(got, recon[:, t]), t
    b.close()
