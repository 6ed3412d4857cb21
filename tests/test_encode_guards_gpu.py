"""What the two encoders' host sides refuse and say (csrc/mobi_encode.cpp, csrc/mobi_encode_inter.cpp, encode.py, encode_inter.py), pinned
as it is, so that the code the two share can move without moving any of it:

  1  mobi_enc_intra_async / mobi_enc_inter_async: every pointer the entry point tests for alignment, off by 1, 2 or 4, every required
     pointer NULL and a NULL handle are MOBI_E_ARG, and nothing is written.  The intra call takes recon_i420 at a multiple of 4, the
     inter call only at a multiple of 8.
  2  mobi_enc_intra / mobi_enc_inter (encode() with numpy input) equal the host models; one encoder object through slot_bytes = 0, a
     small slot, the bound and the small slot again (the slot alias, the staging slots' growth and their reuse)
  3  the type and the text of every exception of the two constructors and the two encode() methods"""
import numpy as np
import pytest
import torch

from tests import enc_inter_model as M
from tests import enc_model as E

pytestmark = pytest.mark.gpu
E_ARG = -7
_CACHE = {}


def _dev():
    from mobiclipdecoder_amd.decoder import default_device
    return torch.device("cuda", default_device())


def _case(kind, W, H):
    """-> (inputs, quantiser arrays, the host model's outputs) of the mixed5 set: the intra model's pictures, or frame 2 of the inter
    model's sequences behind the reconstruction of frame 1"""
    key = (kind, W, H)
    if key not in _CACHE:
        if kind == "intra":
            pics, qs = E.picture_sets(W, H)["mixed5"]
            _CACHE[key] = ((pics,), (qs,), E.host_encode(W, H, 2, pics, qs))
        else:
            frames, qs = M.sequence_sets(W, H)["mixed5"]
            ch = M.chain(W, H, 2, frames, qs)
            _CACHE[key] = ((np.ascontiguousarray(frames[:, 2]), ch[1]["recon"]), (np.ascontiguousarray(qs[:, 1]), np.ascontiguousarray(qs[:, 2])), ch[2])
    return _CACHE[key]


def _encoder(kind, W, H, n=5):
    import mobiclipdecoder_amd as m
    return (m.MobiclipIntraEncoder if kind == "intra" else m.MobiclipInterEncoder)(W, H, 2, n)


def _stats_dtype(kind):
    return E.STATS_DTYPE if kind == "intra" else M.STATS_DTYPE


# ---------------------------------------------------------------------------------------------------------------- 1: the refusals
# (pointer, offset) pairs the entry point refuses, and those it takes although the other one does not
REFUSED = {
    "intra": [("i420", 1), ("i420", 4), ("streams", 1), ("streams", 2), ("recon_i420", 1), ("recon_i420", 2), ("bytes_out", 1), ("bytes_out", 2),
              ("stats", 1), ("stats", 4)],
    "inter": [("i420", 1), ("i420", 4), ("ref_i420", 1), ("ref_i420", 4), ("streams", 1), ("streams", 2), ("recon_i420", 1), ("recon_i420", 4),
              ("bytes_out", 1), ("bytes_out", 2), ("stats", 1), ("stats", 4)],
}
REQUIRED = {"intra": ("i420", "streams", "bytes_out"), "inter": ("i420", "ref_i420", "streams", "bytes_out")}
TAKEN = {"intra": [("streams", 4), ("recon_i420", 4), ("bytes_out", 4), ("stats", 8)], "inter": [("streams", 4), ("recon_i420", 8), ("bytes_out", 4), ("stats", 8)]}


def _call_async(kind, lib, h, stream, n, F, q, slot, p):
    if kind == "intra":
        return lib.mobi_enc_intra_async(h, stream, n, p["i420"], F, q[0].ctypes.data, 0, p["streams"], slot, p["bytes_out"], p["recon_i420"], p["stats"])
    return lib.mobi_enc_inter_async(h, stream, n, p["i420"], F, p["ref_i420"], F, q[0].ctypes.data, q[1].ctypes.data, p["streams"], slot, p["bytes_out"],
                                    p["recon_i420"], p["stats"])


@pytest.mark.parametrize("kind", ("intra", "inter"))
def test_async_refusals_write_nothing(kind):
    from mobiclipdecoder_amd import encode, encode_inter
    W, H, n, room = 16, 16, 5, 16
    inputs, q, want = _case(kind, W, H)
    F = W * H * 3 // 2
    enc = _encoder(kind, W, H)
    lib = (encode if kind == "intra" else encode_inter)._lib()
    slot = enc.stream_bound
    dev = _dev()
    stream = torch.cuda.current_stream(dev).cuda_stream
    src = {name: torch.zeros(n * F + room, dtype=torch.uint8, device=dev) for name in ("i420", "ref_i420")[: len(inputs)]}
    for t, a in zip(src.values(), inputs):
        t[: n * F] = torch.from_numpy(a.copy()).to(dev).reshape(-1)
    sizes = {"streams": n * slot, "bytes_out": n * 4, "recon_i420": n * F, "stats": n * 64}
    outs = {name: torch.full((b + room,), 0xC3, dtype=torch.uint8, device=dev) for name, b in sizes.items()}
    base = {name: t.data_ptr() for name, t in list(src.items()) + list(outs.items())}
    assert all(v % 256 == 0 for v in base.values())
    # every refused call first: none of them may have written anything by the time the device is idle
    for name, off in REFUSED[kind]:
        assert _call_async(kind, lib, enc._h, stream, n, F, q, slot, dict(base, **{name: base[name] + off})) == E_ARG, (name, off)
    for name in REQUIRED[kind]:
        assert _call_async(kind, lib, enc._h, stream, n, F, q, slot, dict(base, **{name: None})) == E_ARG, name
    assert _call_async(kind, lib, None, stream, n, F, q, slot, base) == E_ARG
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert (t.cpu().numpy() == 0xC3).all(), name
    # ... and the offsets each entry point takes, one at a time (for the input pointers the same offsets as their copies' would need
    # other pictures: the refusals above are their pin), with the model's outputs behind them
    dt = _stats_dtype(kind)
    for name, off in [(None, 0)] + TAKEN[kind]:
        for t in outs.values():
            t.fill_(0xC3)
        p = dict(base) if name is None else dict(base, **{name: base[name] + off})
        assert _call_async(kind, lib, enc._h, stream, n, F, q, slot, p) == 0, (name, off)
        torch.cuda.synchronize()
        got = {k: outs[k].cpu().numpy() for k in outs}
        for k, b in sizes.items():
            o = off if k == name else 0
            assert (got[k][:o] == 0xC3).all() and (got[k][o + b:] == 0xC3).all(), (name, off, k)
            got[k] = got[k][o: o + b]
        assert np.array_equal(got["bytes_out"].view(np.int32), want["bytes"]), (name, off)
        assert np.array_equal(got["streams"].reshape(n, slot), want["streams"]), (name, off)
        assert np.array_equal(got["recon_i420"].reshape(n, F), want["recon"]), (name, off)
        gs = got["stats"].view(dt).reshape(-1)
        for f in dt.names:
            assert np.array_equal(gs[f], want["stats"][f]), (name, off, f)
    enc.close()


# ---------------------------------------------------------------------------------------------------------------- 2: the host-pointer calls
def _encode(kind, enc, inputs, q, **kw):
    return enc.encode(inputs[0], q[0], **kw) if kind == "intra" else enc.encode(inputs[0], inputs[1], q[0], q[1], **kw)


def _same_extras(kind, ex, want, where):
    assert np.array_equal(ex["recon"], want["recon"]), where
    dt = _stats_dtype(kind)
    assert ex["stats"].dtype == dt and ex["stats"].shape == want["stats"].shape
    for f in dt.names:
        assert np.array_equal(ex["stats"][f], want["stats"][f]), (where, f)


@pytest.mark.parametrize("kind", ("intra", "inter"))
def test_host_entry_point_equals_the_model_and_reuses_its_staging(kind):
    W, H = 48, 32
    inputs, q, want = _case(kind, W, H)
    n = inputs[0].shape[0]
    whole = [want["streams"][i, : want["bytes"][i]].tobytes() for i in range(n)]
    enc = _encoder(kind, W, H)
    lst, ex = _encode(kind, enc, inputs, q, recon=True, stats=True)
    assert lst == whole and sorted(ex) == ["recon", "stats"]
    _same_extras(kind, ex, want, "default")
    assert _encode(kind, enc, inputs, q) == whole
    enc.close()
    # a fresh object: the first call has no staging slots at all
    order = np.argsort(want["bytes"])
    small = (int(want["bytes"][order[-1]]) - 2) // 4 * 4  # too small for the longest stream alone
    bound = want["streams"].shape[1]
    assert want["bytes"][order[-2]] <= small < want["bytes"][order[-1]] <= bound
    enc = _encoder(kind, W, H)
    assert bound == enc.stream_bound
    for step, slot in enumerate((0, small, bound, small)):
        lst, ex = _encode(kind, enc, inputs, q, recon=True, stats=True, slot_bytes=slot)
        assert sorted(ex) == ["recon", "sizes", "slots", "stats"] and ex["slots"].shape == (n, slot)
        assert np.array_equal(ex["sizes"], want["bytes"]), (step, slot)
        _same_extras(kind, ex, want, (step, slot))
        for i in range(n):
            if want["bytes"][i] <= slot:
                assert lst[i] == whole[i] and np.array_equal(ex["slots"][i], want["streams"][i, :slot]), (step, slot, i)
            else:
                assert lst[i] == b"" and not ex["slots"][i].any(), (step, slot, i)
    enc.close()


# ---------------------------------------------------------------------------------------------------------------- 3: the messages
def _raises(exc, text, fn, *a, **kw):
    with pytest.raises(exc) as e:
        fn(*a, **kw)
    assert type(e.value) is exc and str(e.value) == text, (type(e.value), str(e.value))


WHAT = {"intra": ("pictures", "a uint8 tensor"), "inter": ("pictures and references", "uint8 tensors")}


@pytest.mark.parametrize("kind", ("intra", "inter"))
def test_python_messages(kind):
    import mobiclipdecoder_amd as m
    W, H = 16, 16
    F = W * H * 3 // 2
    cls = m.MobiclipIntraEncoder if kind == "intra" else m.MobiclipInterEncoder
    name, tensors = WHAT[kind]
    k = 1 if kind == "intra" else 2  # pictures, and references
    dev = _dev()
    # the constructors
    for w, h in ((24, 16), (16, 8), (0, 16), (1040, 16)):
        _raises(m.MobiclipError, "bad argument", cls, w, h, 2, 1)
    _raises(m.MobiclipError, "bad argument", cls, W, H, 2, 0)
    _raises(m.MobiclipError, "unsupported codec version", cls, W, H, 3, 1)
    # (the one raise left, "... create failed", needs a device that fails: not provoked here)
    # encode(); for the inter encoder with the pictures as their own references and 30 before the quantiser named
    enc = cls(W, H, 2, 2)
    pic = np.full((2, F), 128, np.uint8)
    tpic = torch.from_numpy(pic).to(dev)
    enc_q = lambda pics, q, **kw: enc.encode(*([pics] * k), *((q,) if kind == "intra" else (30, q)), **kw)
    assert len(enc_q(pic, 30)) == 2 and len(enc_q(tpic, 30)) == 2
    for bad in (pic.astype(np.int16), pic.astype(np.float32), pic[:, :-1].astype(np.int8)):  # the dtype comes before the shape
        _raises(ValueError, name + " must be uint8", enc_q, bad, 30)
    for bad in (pic[:, :-1], pic[0], pic[None], tpic[:, :-8], tpic[0], np.zeros((2, F + 8), np.uint8)):
        _raises(ValueError, f"{name} must be (N, {F})", enc_q, bad, 30)
    _raises(ValueError, f"{name} must be (N, {F})", enc_q, pic[:, :-1], [30])  # the shape comes before the quantisers
    one = "one quantizer, or one per picture"
    for bad in ([30], [30, 30, 30], [], 256, -1, [30, 256], [-1, 30]):
        _raises(ValueError, one, enc_q, pic, bad)
        _raises(ValueError, one, enc_q, tpic, bad)
    _raises(ValueError, one if kind == "intra" else "one prev_quantizer, or one per picture", enc_q, pic[:0], 30)  # no picture at all
    _raises(ValueError, one, enc_q, tpic.float(), [30])  # the quantisers come before the tensors' dtype and device
    for bad in (tpic.float(), tpic.cpu(), tpic.to(torch.int8)):
        _raises(ValueError, f"{name} must be {tensors} on the encoder's device", enc_q, bad, 30)
    for bad in (11, 53, 0, 255, [30, 11], [53, 30]):  # inside a byte, outside 12..52: the C check's refusal
        _raises(m.MobiclipError, "bad argument", enc_q, pic, bad)
        _raises(m.MobiclipError, "bad argument", enc_q, tpic, bad)
    three = np.full((3, F), 128, np.uint8)
    _raises(m.MobiclipError, "bad argument", enc_q, three, 30)  # more than max_pictures
    _raises(m.MobiclipError, "bad argument", enc_q, torch.from_numpy(three).to(dev), 30)
    _raises(m.MobiclipError, "bad argument", enc_q, pic, 30, slot_bytes=6)
    _raises(m.MobiclipError, "bad argument", enc_q, tpic, 30, slot_bytes=6)
    if kind == "intra":
        _raises(m.MobiclipError, "bad argument", enc.encode, pic, 30, yuv_format=2)
        _raises(m.MobiclipError, "bad argument", enc.encode, tpic, 30, yuv_format=2)
    else:
        both = "pictures and references must both be torch tensors or both numpy arrays"
        _raises(ValueError, both, enc.encode, pic, tpic, 30, 30)
        _raises(ValueError, both, enc.encode, tpic, pic, 30, 30)
        _raises(ValueError, both, enc.encode, tpic, pic.astype(np.int16), 30, 30)  # ... comes first
        # either of the two is enough, and each quantiser array has its own name
        _raises(ValueError, name + " must be uint8", enc.encode, pic, pic.astype(np.int16), 30, 30)
        _raises(ValueError, f"{name} must be (N, {F})", enc.encode, pic, pic[:1], 30, 30)
        _raises(ValueError, f"{name} must be (N, {F})", enc.encode, tpic, tpic[:1], 30, 30)
        _raises(ValueError, f"{name} must be {tensors} on the encoder's device", enc.encode, tpic, tpic.to(torch.int8), 30, 30)
        _raises(ValueError, f"{name} must be {tensors} on the encoder's device", enc.encode, tpic.to(torch.int8), tpic, 30, 30)
        for bad in ([30], 256, -1):
            _raises(ValueError, "one prev_quantizer, or one per picture", enc.encode, pic, pic, bad, 30)
            _raises(ValueError, "one prev_quantizer, or one per picture", enc.encode, pic, pic, bad, bad)  # the previous one's first
            _raises(ValueError, one, enc.encode, pic, pic, 30, bad)
        _raises(m.MobiclipError, "bad argument", enc.encode, pic, pic, 11, 30)
        _raises(m.MobiclipError, "bad argument", enc.encode, tpic, tpic, 30, 53)
    enc.close()
    _raises(m.MobiclipError, "encoder is closed", enc_q, pic, 30)
    _raises(m.MobiclipError, "encoder is closed", enc_q, pic.astype(np.int16), [30])  # ... before anything else is looked at


@pytest.mark.parametrize("kind", ("intra", "inter"))
def test_python_message_for_another_device(kind):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two HIP devices")
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.decoder import default_device
    W, H = 16, 16
    cls = m.MobiclipIntraEncoder if kind == "intra" else m.MobiclipInterEncoder
    name, tensors = WHAT[kind]
    here = default_device()
    other = torch.device("cuda", (here + 1) % torch.cuda.device_count())
    enc = cls(W, H, 2, 1)
    t = torch.full((1, W * H * 3 // 2), 128, dtype=torch.uint8, device=other)
    args = (t, 30) if kind == "intra" else (t, t, 30, 30)
    _raises(ValueError, f"{name} must be {tensors} on the encoder's device", enc.encode, *args)
    enc.close()
