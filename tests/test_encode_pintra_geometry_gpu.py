"""The inter encoder's intra mode on the GPU (csrc/mobi_encode_pintra.hip) at the shapes of tests/enc_model.py, GEOMETRY_SHAPES, which
tests/test_encode_pintra_gpu.py does not have: more than 256 macroblocks, one column, one row, the widest picture.  The batch is the
five clips of `cut` and `uncover` (enc_pintra_model.geometry_set); test_geometry_shapes_through_the_oracle of
tests/test_encode_pintra_model.py has judged the host model by the oracle at these shapes and asserted what the comparison rests on:
intra and inter macroblocks (several hundred bits against 2) on both sides of index 256, macroblock 256 inside a 32-bit word, a
diagonal with x_lo > 0 that holds both kinds.  The host model has no scan, no writer workgroups, no diagonals and one thread a picture;
the device decides diagonal by diagonal (mobi_encpi_decide), sums the statistics in workgroups of 256 macroblocks with atomics
(mobi_encpi_finish), scans the lengths 256 at a time with a carry and writes 64 macroblocks to a workgroup.  Only a byte comparison
sees those go wrong.

  a  P-frames 1..3: slots (the zeros behind each stream included), bytes_out, recon_i420 and every field of stats, reserved included,
     equal the host model's byte for byte, with device tensors on torch's stream and once a shape through the host entry point
  b  I, P, P, P fed frame by frame to MobiclipBatch: export_tensor("i420") is the reported reconstruction, export_motion("mb") gives every
     macroblock the type the model's flag says, export_motion("cells") the model's vector with ref 1 in inter macroblocks, ref 0 in intra
  c  at 272x256 encode_target in the mode equals the Python bisection over the host model's fixed-quantiser encodes: two scan rounds a trial
  d  at 272x256 a slot one word too small for the longest stream alone stays zero with its true size, the others are exact, the guard
     bytes around slots, reconstruction, statistics and sizes are untouched, on a side stream with pitches above the minimum
  e  at 272x256 one context switched 1 -> 0 -> 1 gives intra-mode bytes, mode-0 bytes, intra-mode bytes: nothing of the mode's `kind` or
     zeroed vectors behind index 256 is left for mode 0 to find"""
import numpy as np
import pytest
import torch

from tests import enc_inter_model as M
from tests import enc_model as E
from tests import enc_pintra_model as PI
from tests import enc_rate_model as R

pytestmark = pytest.mark.gpu
CHAIN_SHAPES = ((272, 256), (1024, 144), (16, 4112))
THREADS = 5  # of the host model: a thread per picture
_CACHE = {}


def model(W, H, version):
    """(frames, quantizers, the host models' chain I, P, P, P in the intra mode), once per (shape, version)"""
    key = (W, H, version)
    if key not in _CACHE:
        frames, qs = PI.geometry_set(W, H)
        _CACHE[key] = (frames, qs, PI.chain(W, H, version, 1, frames, qs, threads=THREADS))
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
@pytest.mark.parametrize("W,H", E.GEOMETRY_SHAPES)
def test_bit_exact_against_the_host_model(W, H, version):
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.encode_inter import STAT_INTRA, STATS_DTYPE
    frames, qs, ch = model(W, H, version)
    n = frames.shape[0]
    enc = m.MobiclipInterEncoder(W, H, version, n, intra=True)
    dev = _dev()
    for t in range(1, PI.T):
        want, refs = ch[t], ch[t - 1]["recon"]
        slot = want["streams"].shape[1]
        assert slot == enc.stream_bound
        streams, sizes, ex = enc.encode(torch.from_numpy(frames[:, t].copy()).to(dev), torch.from_numpy(refs).to(dev), qs[:, t - 1], qs[:, t], recon=True,
                                        stats=True, slot_bytes=slot)
        st = ex["stats"].cpu().numpy().view(STATS_DTYPE).reshape(-1)
        _same(streams.cpu().numpy(), sizes.cpu().numpy(), ex["recon"].cpu().numpy(), st, want, (t, "device"))
        assert np.array_equal(st["reserved"][:, STAT_INTRA], PI.is_intra(want).sum(1)), t
        assert (st["reserved"][:, STAT_INTRA] > 0).all(), t
    if version == PI.VERSIONS[0]:  # the host entry point, once a shape
        last = ch[PI.T - 1]
        lst, ex = enc.encode(frames[:, PI.T - 1], ch[PI.T - 2]["recon"], qs[:, PI.T - 2], qs[:, PI.T - 1], recon=True, stats=True, slot_bytes=slot)
        _same(ex["slots"], ex["sizes"], ex["recon"], ex["stats"], last, "host")
        assert lst == [last["streams"][i, : last["bytes"][i]].tobytes() for i in range(n)]
    enc.close()


@pytest.mark.parametrize("W,H", CHAIN_SHAPES)
def test_chain_decodes_on_the_gpu_with_the_encoders_kinds_and_motion(W, H):
    """the decoder on P-frames that mix macroblock kinds at stride 1024, at 257 rows and behind macroblock 256"""
    import mobiclipdecoder_amd as m
    dev, version = _dev(), 2
    mbw, mbh = W // 16, H // 16
    frames, qs, ch = model(W, H, version)
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
        assert np.array_equal(ex["recon"], ch[t]["recon"]), t
        assert streams == [ch[t]["streams"][i, : ch[t]["bytes"][i]].tobytes() for i in range(n)], t
        ref = torch.from_numpy(ex["recon"]).to(dev)
        rcs, offs = b.decode(streams, [0] * n)
        assert rcs == [0] * n, (t, rcs)
        assert all(o <= len(s) for o, s in zip(offs, streams))
        got = b.export_tensor("i420")[0]
        cells, mb = (b.export_motion("cells")[0], b.export_motion("mb")[0]) if t else (None, None)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), ex["recon"]), t
        if t:
            flag = PI.is_intra(ch[t]).reshape(n, mbh, mbw)
            assert np.array_equal(mb.cpu().numpy()[:, 0], flag.astype(np.int32)), t
            dx, dy = M.unpack_mv(ch[t]["mv"])
            up = lambda a: np.kron(a.reshape(n, mbh, mbw), np.ones((8, 8), np.int64))
            cells, inter_c = cells.cpu().numpy(), ~up(flag).astype(bool)
            assert np.array_equal(cells[:, 0][inter_c], up(dx)[inter_c]) and np.array_equal(cells[:, 1][inter_c], up(dy)[inter_c]), t
            assert (cells[:, 2][inter_c] == 1).all() and (cells[:, 2][~inter_c] == 0).all(), t
    for o in (b, intra, inter):
        o.close()


@pytest.mark.parametrize("version", PI.VERSIONS)
def test_encode_target_is_the_bisection_over_the_host_model_at_272x256(version):
    """tests/test_encode_pintra_gpu.py, test_encode_target_is_the_bisection_over_the_host_model, with a second scan round in every trial:
    frame 1 of the five clips on the intra model's reconstruction of frame 0 at enc_rate_model.REF_Q; the classes rotated over the
    pictures: ends at qmin (the target is the stream bound, which no stream exceeds, so every trial fits), inside the range (what the
    quantiser two below the middle takes), at qmax (nothing fits)"""
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.encode_inter import STATS_DTYPE
    W, H = 272, 256
    frames = PI.geometry_set(W, H)[0]
    n, mid = frames.shape[0], (R.QMIN + R.QMAX) >> 1
    pq = np.full(n, R.REF_Q, np.uint8)
    refs = E.host_encode(W, H, version, frames[:, 0], pq, threads=THREADS)["recon"]
    pics = np.ascontiguousarray(frames[:, 1])
    at_mid = PI.fixed(W, H, version, pics, refs, pq, mid - 2, threads=THREADS)["bytes"]
    enc = m.MobiclipInterEncoder(W, H, version, n, intra=True)
    cls = {"qmin": lambda i: int(enc.stream_bound), "inside": lambda i: int(at_mid[i]), "qmax": lambda i: 0}
    names = list(cls)
    dev = _dev()
    seen = set()
    for r in range(len(names)):
        tg = np.array([cls[names[(i + r) % len(names)]](i) for i in range(n)], np.int32)
        want, q_want = PI.bisect(W, H, version, pics, refs, pq, tg, threads=THREADS)
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


def test_a_slot_one_word_too_small_and_guards_at_272x256():
    """tests/test_encode_pintra_gpu.py, test_guards_stream_and_pitches, with five workgroups of the writer and two of mobi_encpi_finish a
    picture"""
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd import encode_inter
    W, H, version = 272, 256, 2
    frames, qs, ch = model(W, H, version)
    want, n, F = ch[2], frames.shape[0], frames.shape[2]
    behind = PI.is_intra(want)[:, 256:]
    assert behind.any() and not behind.all()
    order = np.argsort(want["bytes"])
    slot = (int(want["bytes"][order[-1]]) - 2) // 4 * 4  # too small for the longest stream alone, by one word at most
    assert want["bytes"][order[-2]] <= slot < want["bytes"][order[-1]] <= slot + 4
    enc = m.MobiclipInterEncoder(W, H, version, n, intra=True)
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


@pytest.mark.parametrize("version", PI.VERSIONS)
def test_mode_switching_at_272x256(version):
    """P-frame 2: every picture has intra macroblocks, four of the five behind index 256, whose `kind` and zeroed vectors mode 0 must not see"""
    import mobiclipdecoder_amd as m
    W, H, t = 272, 256, 2
    frames, qs, ch1 = model(W, H, version)
    n = frames.shape[0]
    refs = ch1[t - 1]["recon"]
    want = {1: ch1[t], 0: M.host_encode(W, H, version, frames[:, t], refs, qs[:, t - 1], qs[:, t], threads=THREADS)}
    assert PI.is_intra(want[1])[:, 256:].any(1).sum() >= 4 and not np.array_equal(want[1]["mv"], want[0]["mv"])
    enc = m.MobiclipInterEncoder(W, H, version, n)
    for mode in (1, 0, 1):
        enc.set_intra(bool(mode))
        assert enc.intra is bool(mode) and enc.stream_bound == want[mode]["streams"].shape[1]
        lst, ex = enc.encode(frames[:, t], refs, qs[:, t - 1], qs[:, t], recon=True, stats=True, slot_bytes=enc.stream_bound)
        _same(ex["slots"], ex["sizes"], ex["recon"], ex["stats"], want[mode], (mode,))
        assert bool(ex["stats"]["reserved"].any()) == bool(mode)
    enc.close()
