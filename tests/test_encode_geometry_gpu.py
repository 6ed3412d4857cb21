"""The encoders on the GPU at the shapes the other encoder tests do not have (tests/enc_model.py, GEOMETRY_SHAPES): more than 256
macroblocks, taller than wide, one column, one row, the widest picture, and a scene that does not move.  The host models, which
test_geometry_shapes_through_the_oracle of tests/test_encode_model.py, test_encode_inter_model.py and test_encode_parts_model.py have
judged by the oracle at these shapes, sum the macroblocks' lengths and write them in raster order; the device scans them 256 at a time
with a carry (csrc/mobi_encode_write.h) and writes them 64 to a workgroup, neighbours sharing a 32-bit word by atomic OR, and the intra
encoder goes diagonal by diagonal.  Only a byte comparison sees those go wrong: a wrong carry keeps the stream inside its slot.

  a  I-frames of the mixed five: slots (the zeros behind each stream included), bytes_out, recon_i420 and every field of stats equal the
     host model's byte for byte, with device tensors on torch's stream and once through the host entry point
  b  P-frames 1..3 of the mixed five and of the still scene (2 or 3 bits a macroblock: 16 or 10 lanes OR into one word), in mode 0 and
     in partition mode 1: the same, reserved[STAT_SPLIT] included
  c  I, P, P, P encoded frame by frame from the reported reconstruction and fed to MobiclipBatch: export_tensor("i420") is the
     reconstruction and, in mode 1, export_motion("cells") the model's quadrant vectors
  d  the rate rule at 272x256 for the three kinds: every trial's scan goes through two rounds
  e  at 272x256 a slot one word too small for the longest stream alone stays zero with its true size, the others are exact, and the guard
     bytes around slots, reconstruction, statistics and sizes are untouched"""
import numpy as np
import pytest
import torch

from tests import enc_inter_model as M
from tests import enc_model as E
from tests import enc_parts_model as Q
from tests import enc_rate_model as R

pytestmark = pytest.mark.gpu
CHAIN_SHAPES = ((272, 256), (1024, 144), (16, 4112))
THREADS = 5  # of the host models: a thread per picture
_CACHE = {}


def intra_model(W, H, version):
    key = ("intra", W, H, version)
    if key not in _CACHE:
        pics, qs = E.picture_sets(W, H)["mixed5"]
        _CACHE[key] = (pics, qs, E.host_encode(W, H, version, pics, qs, threads=THREADS))
    return _CACHE[key]


def model(W, H, name, version, mode):
    """(frames, quantizers, the host models' chain I, P, P, P in partition mode `mode`), once per (shape, set, version, mode)"""
    key = (W, H, name, version, mode)
    if key not in _CACHE:
        frames, qs = M.geometry_set(W, H, name)
        first = ("first", W, H, name, version)
        if first not in _CACHE:
            _CACHE[first] = E.host_encode(W, H, version, frames[:, 0], qs[:, 0], threads=THREADS)
        ch = [_CACHE[first]]
        for t in range(1, M.T):
            args = (frames[:, t], ch[-1]["recon"], qs[:, t - 1], qs[:, t])
            ch.append(Q.host_encode(W, H, version, 1, *args, threads=THREADS) if mode else M.host_encode(W, H, version, *args, threads=THREADS))
        _CACHE[key] = (frames, qs, ch)
    return _CACHE[key]


def _dev():
    from mobiclipdecoder_amd.decoder import default_device
    return torch.device("cuda", default_device())


def _same(got_streams, got_bytes, got_recon, got_stats, want, names, where):
    assert np.array_equal(got_bytes, want["bytes"]), where
    assert np.array_equal(got_streams, want["streams"]), where
    assert np.array_equal(got_recon, want["recon"]), where
    for f in names:
        assert np.array_equal(got_stats[f], want["stats"][f]), (where, f)


@pytest.mark.parametrize("version", E.VERSIONS)
@pytest.mark.parametrize("W,H", E.GEOMETRY_SHAPES)
def test_intra_bit_exact_against_the_host_model(W, H, version):
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.encode import STATS_DTYPE
    pics, qs, want = intra_model(W, H, version)
    enc = m.MobiclipIntraEncoder(W, H, version, 5)
    slot = want["streams"].shape[1]
    assert slot == enc.stream_bound
    streams, sizes, ex = enc.encode(torch.from_numpy(pics).to(_dev()), qs, recon=True, stats=True, slot_bytes=slot)
    _same(streams.cpu().numpy(), sizes.cpu().numpy(), ex["recon"].cpu().numpy(), ex["stats"].cpu().numpy().view(STATS_DTYPE).reshape(-1), want,
          E.STATS_DTYPE.names, "device")
    lst, ex = enc.encode(pics, qs, recon=True, stats=True, slot_bytes=slot)
    _same(ex["slots"], ex["sizes"], ex["recon"], ex["stats"], want, E.STATS_DTYPE.names, "host")
    assert lst == [want["streams"][i, : want["bytes"][i]].tobytes() for i in range(len(qs))]
    enc.close()


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("version", M.VERSIONS)
@pytest.mark.parametrize("W,H", E.GEOMETRY_SHAPES)
def test_inter_bit_exact_against_the_host_model(W, H, version, mode):
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.encode_inter import STATS_DTYPE
    enc = m.MobiclipInterEncoder(W, H, version, 5, partitions=bool(mode))
    dev = _dev()
    for name in M.GEOMETRY_SETS:
        frames, qs, ch = model(W, H, name, version, mode)
        for t in range(1, M.T):
            want, refs = ch[t], ch[t - 1]["recon"]
            slot = want["streams"].shape[1]
            assert slot == enc.stream_bound
            streams, sizes, ex = enc.encode(torch.from_numpy(frames[:, t].copy()).to(dev), torch.from_numpy(refs).to(dev), qs[:, t - 1], qs[:, t], recon=True,
                                            stats=True, slot_bytes=slot)
            st = ex["stats"].cpu().numpy().view(STATS_DTYPE).reshape(-1)
            _same(streams.cpu().numpy(), sizes.cpu().numpy(), ex["recon"].cpu().numpy(), st, want, M.STATS_DTYPE.names, (name, t, "device"))
            if mode:
                assert np.array_equal(st["reserved"][:, Q.STAT_SPLIT], (want["mbs"]["luma_mode"] != 0).sum(1)), (name, t)
            else:
                dx, dy = M.unpack_mv(want["mv"])
                assert np.array_equal(st["nonzero_mv"], ((dx != 0) | (dy != 0)).sum(1)) and np.array_equal(st["halfpel_mv"], (((dx | dy) & 1) != 0).sum(1))
        # the host entry point, once per set
        lst, ex = enc.encode(frames[:, M.T - 1], ch[M.T - 2]["recon"], qs[:, M.T - 2], qs[:, M.T - 1], recon=True, stats=True, slot_bytes=slot)
        _same(ex["slots"], ex["sizes"], ex["recon"], ex["stats"], ch[M.T - 1], M.STATS_DTYPE.names, (name, "host"))
        assert lst == [ch[M.T - 1]["streams"][i, : ch[M.T - 1]["bytes"][i]].tobytes() for i in range(frames.shape[0])]
    enc.close()


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("W,H", CHAIN_SHAPES)
def test_chain_decodes_on_the_gpu_to_the_reconstruction(W, H, mode):
    """I, P, P, P of every clip, each P-frame from the reconstruction the call before reported, fed frame by frame to MobiclipBatch"""
    import mobiclipdecoder_amd as m
    dev, version = _dev(), 2
    mbw, mbh = W // 16, H // 16
    for name in ("still", "mixed5"):
        frames, qs, ch = model(W, H, name, version, mode)
        n = frames.shape[0]
        intra, inter = m.MobiclipIntraEncoder(W, H, version, n), m.MobiclipInterEncoder(W, H, version, n, partitions=bool(mode))
        b = m.MobiclipBatch(n, W, H, version)
        if mode:
            b.set_motion(True)
        ref = None
        for t in range(M.T):
            pics = torch.from_numpy(frames[:, t].copy()).to(dev)
            if t == 0:
                streams, ex = intra.encode(pics, qs[:, 0], recon=True)
            else:
                streams, ex = inter.encode(pics, ref, qs[:, t - 1], qs[:, t], recon=True)
            assert np.array_equal(ex["recon"], ch[t]["recon"]), (name, t)
            assert streams == [ch[t]["streams"][i, : ch[t]["bytes"][i]].tobytes() for i in range(n)], (name, t)
            ref = torch.from_numpy(ex["recon"]).to(dev)
            rcs, offs = b.decode(streams, [0] * n)
            assert rcs == [0] * n, (name, t, rcs)
            assert all(o <= len(s) for o, s in zip(offs, streams))
            got = b.export_tensor("i420")[0]
            cells = b.export_motion("cells")[0] if mode and t else None
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), ex["recon"]), (name, t)
            if cells is not None:
                # the decoder's own motion field: every 2x2 cell of quadrant qd of macroblock i holds the model's vector of that quadrant
                dx4, dy4 = M.unpack_mv(ch[t]["mv4"])
                quad = lambda a: np.kron(a.reshape(n, mbh, mbw, 2, 2).transpose(0, 1, 3, 2, 4).reshape(n, 2 * mbh, 2 * mbw), np.ones((4, 4), np.int64))
                cells = cells.cpu().numpy()
                assert np.array_equal(cells[:, 0], quad(dx4)) and np.array_equal(cells[:, 1], quad(dy4)), (name, t)
                assert (cells[:, 2] == 1).all(), (name, t)
        for o in (b, intra, inter):
            o.close()


@pytest.mark.parametrize("kind", R.KINDS)
def test_rate_bit_exact_at_272x256(kind):
    """tests/test_encode_rate_gpu.py, test_bit_exact_at_272x208, with a second scan round in every trial"""
    import mobiclipdecoder_amd as m
    W, H, version = 272, 256, 2
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
    enc = m.MobiclipIntraEncoder(W, H, version, n) if kind == 0 else m.MobiclipInterEncoder(W, H, version, n, partitions=kind == 2)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    args = (up(pics),) if kind == 0 else (up(pics), up(refs), up(pq))
    out, sizes, ex = enc.encode_target(*args, up(tg), 12, 52, recon=True, stats=True, slot_bytes=enc.stream_bound)
    torch.cuda.synchronize()
    assert np.array_equal(ex["quantizer"].cpu().numpy(), want["quantizer"]), (ex["quantizer"], want["quantizer"])
    _same(out.cpu().numpy(), sizes.cpu().numpy(), ex["recon"].cpu().numpy(), ex["stats"].cpu().numpy().view(enc._stats).reshape(-1), want, R.STATS[kind].names, kind)
    enc.close()


@pytest.mark.parametrize("mode", (0, 1))
def test_a_slot_one_word_too_small_and_guards_at_272x256(mode):
    """tests/test_encode_inter_gpu.py, test_guards_stream_and_pitches, with five workgroups of the writer a picture"""
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd import encode_inter
    W, H, version = 272, 256, 2
    frames, qs, ch = model(W, H, "mixed5", version, mode)
    want, n, F = ch[2], frames.shape[0], frames.shape[2]
    order = np.argsort(want["bytes"])
    slot = (int(want["bytes"][order[-1]]) - 2) // 4 * 4  # too small for the longest stream alone, by one word at most
    assert want["bytes"][order[-2]] <= slot < want["bytes"][order[-1]] <= slot + 4
    enc = m.MobiclipInterEncoder(W, H, version, 5, partitions=bool(mode))
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
    enc.close()
