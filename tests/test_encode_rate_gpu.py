"""The encoders' rate control on the GPU (include/mobiclip_encode_rate.h, csrc/mobi_encode_rate.hip around the encoders' kernels) against
its host model (tests/enc_rate_model.py), which tests/test_encode_rate_model.py has judged by the existing models and by the oracle.

  a  I-frames, P-frames and P-frames with partitions at 16x16 and 48x32 over the coverage calls, and one call at 272x208: slots (the zeros
     behind each stream included), bytes_out, quantizers_out, recon_i420 and every field of stats equal the host model's byte for byte
  b  qmin == qmax equals encode() of the same object byte for byte
  c  a chain I, P, P, P in which every call's prev_quantizer is the call before's device tensor and nothing is waited for until the end
     equals the model's chain, and MobiclipBatch decodes every clip to the reported reconstructions
  d  encode_clips(target_bytes=, carry_bytes=) equals a Python loop over encode_target with the carry kept on the host; with quantizer=
     it equals the loop over encode() it has always been
  e  every new refusal; guard bytes around quantizers_out, bytes_out and the slots; a slot smaller than the final stream stays zero with
     its true size; a numpy input raises"""
import numpy as np
import pytest
import torch

from tests import enc_inter_model as M
from tests import enc_parts_model as Q
from tests import enc_rate_model as R

pytestmark = pytest.mark.gpu
MOBI_E_ARG = -7


def _dev():
    from mobiclipdecoder_amd.decoder import default_device
    return torch.device("cuda", default_device())


def _encoder(W, H, version, kind, n):
    import mobiclipdecoder_amd as m
    return m.MobiclipIntraEncoder(W, H, version, n) if kind == 0 else m.MobiclipInterEncoder(W, H, version, n, partitions=kind == 2)


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _target(enc, kind, pics, refs, pq, tg, qmin, qmax, **kw):
    """encode_target with everything as device tensors, unsynchronised -> (slots, sizes, dict) as numpy, stats as records"""
    args = (_up(pics),) if kind == 0 else (_up(pics), _up(refs), _up(pq))
    out, sizes, ex = enc.encode_target(*args, _up(tg), qmin, qmax, recon=True, stats=True, slot_bytes=enc.stream_bound, **kw)
    assert ex["quantizer"].is_cuda and ex["quantizer"].dtype == torch.uint8
    torch.cuda.synchronize()
    ex = {k: v.cpu().numpy() for k, v in ex.items()}
    ex["stats"] = ex["stats"].view(enc._stats).reshape(-1)
    return out.cpu().numpy(), sizes.cpu().numpy(), ex


def _same(got, want, stats_dtype, where):
    slots, sizes, ex = got
    assert np.array_equal(ex["quantizer"], want["quantizer"]), (where, ex["quantizer"], want["quantizer"])
    assert np.array_equal(sizes, want["bytes"]), where
    assert np.array_equal(slots, want["streams"]), where
    assert np.array_equal(ex["recon"], want["recon"]), where
    for f in stats_dtype.names:
        assert np.array_equal(ex["stats"][f], want["stats"][f]), (where, f)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("version", R.VERSIONS)
@pytest.mark.parametrize("W,H", R.SHAPES)
def test_bit_exact_against_the_host_model(W, H, version, kind):
    pics, refs, _ = R.inputs(W, H, version, kind)
    enc = _encoder(W, H, version, kind, pics.shape[0] + 1)
    assert enc.stream_bound == R.host().encr_host_bound(W, H, kind)
    for name, pq, tg, qmin, qmax in R.calls(W, H, version, kind):
        _same(_target(enc, kind, pics, refs, pq, tg, qmin, qmax), R.model(W, H, version, kind, name), R.STATS[kind], name)
    enc.close()


@pytest.mark.parametrize("kind", R.KINDS)
def test_bit_exact_at_272x208(kind):
    W, H, version = 272, 208, 2
    frames = M.sequence_sets(W, H)["mixed5"][0]
    n = frames.shape[0]
    pics = frames[:, 0] if kind == 0 else frames[:, 1]
    refs = None if kind == 0 else R.fixed(W, H, version, 0, frames[:, 0], None, None, R.REF_Q)["recon"]
    pq = np.array([20, 9, 20, 52, 20], np.uint8)
    # per picture: half of what q = 30 takes; exactly what q = 22 takes; nothing; everything; what q = 45 takes
    at = lambda q: R.fixed(W, H, version, kind, pics, refs, pq, q)["bytes"].astype(np.int64)
    tg = np.array([at(30)[0] // 2, at(22)[1], 0, 1 << 30, at(45)[4]], np.int32)
    want = R.host_target(W, H, version, kind, pics, refs, pq, tg, threads=8)
    assert len(set(want["quantizer"].tolist())) >= 4
    enc = _encoder(W, H, version, kind, n)
    _same(_target(enc, kind, pics, refs, pq, tg, 12, 52), want, R.STATS[kind], kind)
    enc.close()


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_range_of_one_is_encode(kind):
    W, H, version = 48, 32, 2
    pics, refs, pq = R.inputs(W, H, version, kind)
    n = pics.shape[0]
    enc = _encoder(W, H, version, kind, n)
    for q in (12, 31, 52):
        got = _target(enc, kind, pics, refs, pq, np.zeros(n, np.int32), q, q)
        args = (_up(pics), q) if kind == 0 else (_up(pics), _up(refs), pq, q)
        out, sizes, ex = enc.encode(*args, recon=True, stats=True, slot_bytes=enc.stream_bound)
        torch.cuda.synchronize()
        assert (got[2]["quantizer"] == q).all()
        assert np.array_equal(got[0], out.cpu().numpy()) and np.array_equal(got[1], sizes.cpu().numpy())
        assert np.array_equal(got[2]["recon"], ex["recon"].cpu().numpy())
        assert np.array_equal(got[2]["stats"], ex["stats"].cpu().numpy().view(enc._stats).reshape(-1))
    enc.close()


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("version", R.VERSIONS)
def test_chain_on_device_tensors_decodes(version, mode):
    import mobiclipdecoder_amd as m
    W, H = 48, 32
    sets = Q.sequence_sets(W, H)
    frames = np.concatenate([sets["mixed5"][0], sets["two_motion"][0]])
    n = frames.shape[0]
    first = R.fixed(W, H, version, 0, frames[:, 0], None, None, 30)["bytes"].astype(np.int64)
    targets = np.stack([first, first // 2, first // 4, np.where(np.arange(n) % 2, 4, first)], 1).astype(np.int32)
    want = R.chain(W, H, version, mode, frames, targets)
    intra, inter = _encoder(W, H, version, 0, n), _encoder(W, H, version, 1 + mode, n)
    slot = max(intra.stream_bound, inter.stream_bound)
    dev_frames, dev_targets = _up(frames), _up(targets)
    held, ref, q = [], None, None
    for t in range(Q.T):
        if t == 0:
            res = intra.encode_target(dev_frames[:, 0].contiguous(), dev_targets[:, 0].contiguous(), recon=True, slot_bytes=slot)
        else:
            res = inter.encode_target(dev_frames[:, t].contiguous(), ref, q, dev_targets[:, t].contiguous(), recon=True, slot_bytes=slot)
        ref, q = res[2]["recon"], res[2]["quantizer"]
        held.append(res)
    torch.cuda.synchronize()  # the only wait
    b = m.MobiclipBatch(n, W, H, version)
    for t, (out, sizes, ex) in enumerate(held):
        out, sizes = out.cpu().numpy(), sizes.cpu().numpy()
        assert np.array_equal(ex["quantizer"].cpu().numpy(), want[t]["quantizer"]), t
        assert np.array_equal(sizes, want[t]["bytes"]) and np.array_equal(ex["recon"].cpu().numpy(), want[t]["recon"]), t
        streams = [out[i, : sizes[i]].tobytes() for i in range(n)]
        assert streams == [want[t]["streams"][i, : sizes[i]].tobytes() for i in range(n)]
        rcs, offs = b.decode(streams, [0] * n)
        assert rcs == [0] * n and all(o <= len(s) for o, s in zip(offs, streams)), (t, rcs)
        got = b.export_tensor("i420")[0]
        torch.cuda.synchronize()
        assert torch.equal(got, ex["recon"]), t
    for o in (b, intra, inter):
        o.close()


@pytest.mark.parametrize("partitions", (False, True))
def test_encode_clips_with_targets_and_carry(partitions):
    import mobiclipdecoder_amd as m
    W, H, version, gop = 48, 32, 2, 3
    sets = Q.sequence_sets(W, H)
    frames = np.concatenate([sets["mixed5"][0], sets["two_motion"][0]])
    n, T = frames.shape[:2]
    first = R.fixed(W, H, version, 0, frames[:, 0], None, None, 30)["bytes"]
    per_frame, carry_bytes, qmin, qmax = [int(np.median(first)), int(np.median(first)) // 3, 40, int(np.median(first))], 64, 14, 50
    dev_frames = _up(frames)
    clips, recon, qs = m.encode_clips(dev_frames, None, gop, version, W, H, recon=True, partitions=partitions, target_bytes=per_frame, carry_bytes=carry_bytes,
                                      qmin=qmin, qmax=qmax, quantizers=True)
    assert tuple(qs.shape) == (n, T) and qs.dtype == torch.uint8 and qs.is_cuda
    # the same by hand: the carry on the host, a wait per frame
    intra, inter = _encoder(W, H, version, 0, n), _encoder(W, H, version, 2 if partitions else 1, n)
    carry, ref, q, spent = np.zeros(n, np.int64), None, None, 0
    for t in range(T):
        given = (per_frame[t] + carry).astype(np.int32)
        if t % gop == 0:
            streams, ex = intra.encode_target(dev_frames[:, t].contiguous(), given.tolist(), qmin, qmax, recon=True)
        else:
            streams, ex = inter.encode_target(dev_frames[:, t].contiguous(), _up(ref), q.tolist(), given.tolist(), qmin, qmax, recon=True)
        ref, q = ex["recon"], ex["quantizer"]
        sizes = np.array([len(s) for s in streams], np.int64)
        carry = np.clip(given - sizes, 0, carry_bytes)
        spent += int((carry > 0).sum())
        assert [c[t] for c in clips] == streams, t
        assert np.array_equal(recon[:, t].cpu().numpy(), ref) and np.array_equal(qs[:, t].cpu().numpy(), q), t
        assert ((sizes <= given) | (q == qmax)).all() and (q >= qmin).all()
    assert spent > 0  # some frame left bytes for the next
    # the fixed-quantiser form is the loop over encode() it has always been
    per_q = [24, 30, 30, 18]
    clips_q, recon_q = m.encode_clips(dev_frames, per_q, gop, version, W, H, recon=True, partitions=partitions)
    assert m.encode_clips(dev_frames, per_q, gop, version, W, H, partitions=partitions) == clips_q
    ref = None
    for t in range(T):
        if t % gop == 0:
            streams, ex = intra.encode(dev_frames[:, t].contiguous(), per_q[t], recon=True)
        else:
            streams, ex = inter.encode(dev_frames[:, t].contiguous(), _up(ref), per_q[t - 1], per_q[t], recon=True)
        ref = ex["recon"]
        assert [c[t] for c in clips_q] == streams and np.array_equal(recon_q[:, t].cpu().numpy(), ref), t
    for bad in (dict(quantizer=24, target_bytes=100), dict(quantizer=None), dict(quantizer=None, target_bytes=[100] * (T + 1)),
                dict(quantizer=None, target_bytes=100, carry_bytes=-1)):
        with pytest.raises(ValueError):
            m.encode_clips(dev_frames, bad.pop("quantizer"), gop, version, W, H, **bad)
    intra.close()
    inter.close()


def test_refusals_guards_and_small_slots():
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd import encode_rate
    W, H, version, kind = 48, 32, 2, 1
    pics, refs, pq = R.inputs(W, H, version, kind)
    name, _, tg, qmin, qmax = R.calls(W, H, version, kind)[0]
    want = R.model(W, H, version, kind, name)
    n, F = pics.shape
    order = np.argsort(want["bytes"])
    slot = (int(want["bytes"][order[-1]]) - 2) // 4 * 4  # too small for the longest final stream alone
    assert want["bytes"][order[-2]] <= slot < want["bytes"][order[-1]]
    enc, ienc = _encoder(W, H, version, kind, n), _encoder(W, H, version, 0, n)
    dev, guard = _dev(), 64
    d_pics, d_refs, d_pq, d_tg = _up(pics), _up(refs), _up(pq), _up(tg)
    buf = torch.full((guard + n * slot + guard,), 0xC3, dtype=torch.uint8, device=dev)
    qout = torch.full((guard + n + guard,), 0xC3, dtype=torch.uint8, device=dev)
    sizes = torch.full((n + 2,), -7, dtype=torch.int32, device=dev)
    lib = encode_rate._lib()
    s = torch.cuda.current_stream(dev).cuda_stream

    def inter(e=enc._h, count=n, prev=d_pq.data_ptr(), target=d_tg.data_ptr(), lo=qmin, hi=qmax, out=qout.data_ptr() + guard):
        return lib.mobi_enc_inter_target_async(e, s, count, d_pics.data_ptr(), F, d_refs.data_ptr(), F, prev, target, lo, hi, buf.data_ptr() + guard, slot,
                                               sizes.data_ptr() + 4, None, None, out)

    def intra(e=ienc._h, count=n, target=d_tg.data_ptr(), lo=qmin, hi=qmax, out=qout.data_ptr() + guard):
        return lib.mobi_enc_intra_target_async(e, s, count, d_pics.data_ptr(), F, target, lo, hi, 0, buf.data_ptr() + guard, slot, sizes.data_ptr() + 4, None, None, out)
    for call in (inter, intra):
        for kw in (dict(lo=11), dict(hi=53), dict(lo=30, hi=29), dict(lo=0, hi=0), dict(target=None), dict(target=d_tg.data_ptr() + 2), dict(out=None), dict(e=None),
                   dict(count=0), dict(count=n + 1)):
            assert call(**kw) == MOBI_E_ARG, (call.__name__, kw)
    assert inter(prev=None) == MOBI_E_ARG
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xC3).all() and (qout.cpu().numpy() == 0xC3).all() and (sizes.cpu().numpy() == -7).all()  # a refused call enqueues nothing
    # the Python side: the library's refusal, and tensors only
    with pytest.raises(m.MobiclipError):
        enc.encode_target(d_pics, d_refs, d_pq, d_tg, 11, 52)
    with pytest.raises(m.MobiclipError):
        ienc.encode_target(d_pics, d_tg, 30, 29)
    with pytest.raises(ValueError):
        enc.encode_target(pics, refs, pq, tg)
    with pytest.raises(ValueError):
        ienc.encode_target(pics, tg)
    with pytest.raises(ValueError):
        ienc.encode_target(d_pics, d_tg.to(torch.int64))
    with pytest.raises(ValueError):
        enc.encode_target(d_pics, d_refs, d_pq.to(torch.int32), d_tg)
    with pytest.raises(ValueError):
        ienc.encode_target(d_pics, [100] * (n + 1))
    # the accepted call: guards, the small slot
    assert inter() == 0
    torch.cuda.synchronize()
    got, gq, sz = buf.cpu().numpy(), qout.cpu().numpy(), sizes.cpu().numpy()
    assert (got[:guard] == 0xC3).all() and (got[guard + n * slot:] == 0xC3).all()
    assert (gq[:guard] == 0xC3).all() and (gq[guard + n:] == 0xC3).all() and np.array_equal(gq[guard: guard + n], want["quantizer"])
    assert sz[0] == -7 and sz[-1] == -7 and np.array_equal(sz[1:-1], want["bytes"])
    slots = got[guard: guard + n * slot].reshape(n, slot)
    for i in range(n):
        if i == order[-1]:
            assert not slots[i].any()
        else:
            assert np.array_equal(slots[i], want["streams"][i, :slot])
    enc.close()
    ienc.close()
    with pytest.raises(m.MobiclipError):
        enc.encode_target(d_pics, d_refs, d_pq, d_tg)
