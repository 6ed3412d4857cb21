"""The Python binding's shared parts (mobiclipdecoder_amd/binding.py, and decoder.py's check_rc and tensor-argument helpers).

  1  a library swapped in behind decoder._LIB -- the profiling_library fixture does that -- gets the signature tables of audio, encode
     and demux too, not only decoder's: with a table left out a 64-bit handle comes back as a C int
  2  the words of every argument refusal the entry points share, and which of two refusals comes first, as they were before the checks
     were gathered in one place (the strings are literals on purpose)
  3  GPU: under the fixture an audio decoder, an intra encoder and a Mods reader -- each a handle of the swapped library -- work"""
import struct

import numpy as np
import pytest

from tests.test_export_device import _NoLib, _fake_batch


def _assert_fully_bound(lib):
    from mobiclipdecoder_amd import audio, demux, encode
    for mod, sigs in ((audio, audio._SIGS), (audio, audio._SX_SIGS), (encode, encode._SIGS), (demux, demux._SIGS)):
        assert mod._lib() is lib
        for name, (res, args) in sigs.items():
            fn = getattr(lib, name)
            assert fn.restype == res and fn.argtypes is not None and list(fn.argtypes) == list(args), name


def test_a_swapped_library_is_fully_bound(monkeypatch):
    from mobiclipdecoder_amd import audio, build, decoder, demux, encode
    product = decoder.load_library()
    for mod in (audio, encode, demux):
        assert mod._lib() is product
    twin = decoder.bind_library(build.build_hip(profiling=True))
    assert twin is not product
    monkeypatch.setattr(decoder, "_LIB", twin)
    _assert_fully_bound(twin)
    monkeypatch.setattr(decoder, "_LIB", product)
    _assert_fully_bound(product)


def _fake_audio():
    from mobiclipdecoder_amd.audio import MobiclipAudio
    a = MobiclipAudio.__new__(MobiclipAudio)
    a._lib, a._h, a.n_streams, a.n_channels, a.framing, a.codec, a.device = _NoLib(), None, 1, 1, "moflex", "pcm16", 0
    return a


def _wording():
    import torch
    cpu = torch.zeros((1, 4, 3, 48, 64), dtype=torch.uint8)
    sink = dict(size=(48, 64), n_frames=2)
    silent = dict(frames=[b""])
    dtype3 = "dtype must be torch.uint8, torch.float16 or torch.float32, not "
    return [
        ("export_tensor", dict(dtype=torch.bfloat16), dtype3 + "torch.bfloat16"),
        ("export_tensor", dict(fmt="i420", dtype=torch.float16), "fmt='i420' has bytes only: dtype must be torch.uint8"),
        ("export_tensor", dict(scale=(1, 1, 1)), "scale and bias apply to fmt='rgb' with a float dtype only"),
        ("export_tensor", dict(dtype=torch.float32, scale=(1, 1)), "scale must be three finite floats, not [1.0, 1.0]"),
        ("export_tensor", dict(dtype=torch.float32, bias=(0, float("inf"), 0)), "bias must be three finite floats, not [0.0, inf, 0.0]"),
        ("export_tensor", dict(stream="default"), "stream must be a torch.cuda.Stream of cuda:0, not 'default'"),
        ("export_tensor", dict(out=cpu), "out must be a contiguous, 16-byte aligned torch.uint8 tensor of shape (1, 4, 3, 48, 64) on cuda:0"),
        ("export_motion", dict(fmt="flow", dtype=torch.int16), "fmt='flow': dtype must be torch.float32 or torch.float16, not torch.int16"),
        ("export_motion", dict(scale="x"), "scale must be a float, not 'x'"),
        ("export_motion", dict(stream=0), "stream must be a torch.cuda.Stream of cuda:0, not 0"),
        ("export_motion", dict(out=torch.zeros((1, 4, 3, 24, 31), dtype=torch.int16)),
         "out must be a contiguous, 16-byte aligned torch.int16 tensor of shape (1, 4, 3, 24, 32) on cuda:0"),
        ("set_sink", dict(sink, dtype=torch.int32), dtype3 + "torch.int32"),
        ("set_sink", dict(sink, scale=(1, 1, 1)), "scale and bias apply to a float dtype only"),
        ("set_sink", dict(sink, out=torch.zeros((4, 2, 3, 48, 128), dtype=torch.uint8)[..., ::2]),
         "out: the innermost H, W of layout 'ntchw' must be contiguous, strides are (36864, 18432, 6144, 128, 2)"),
        ("set_sink", dict(sink, out=torch.zeros((4, 2, 3, 48, 60), dtype=torch.uint8)),
         "out must be a torch.uint8 tensor of shape (4, 2, 3, 48, 64) (layout 'ntchw')"),
        ("audio", dict(silent, dtype=torch.uint8), "dtype must be torch.int16 or torch.float32, not torch.uint8"),
        ("audio", dict(silent, stream="s"), "stream must be a torch.cuda.Stream of cuda:0, not 's'"),
        ("audio", dict(silent, out=torch.zeros((1, 8), dtype=torch.int16)), "out must be a 3-d torch tensor"),
        ("audio", dict(silent, out=torch.zeros((1, 1, 8), dtype=torch.int16)), "out must be a contiguous torch.int16 tensor of shape (1, 1, 8) on cuda:0"),
        # two bad arguments: the check that came first still comes first
        ("export_tensor", dict(dtype=torch.bfloat16, stream="default"), dtype3 + "torch.bfloat16"),
        ("export_tensor", dict(stream="default", out=cpu), "stream must be a torch.cuda.Stream of cuda:0, not 'default'"),
        ("export_motion", dict(scale="x", out=cpu), "scale must be a float, not 'x'"),
        ("set_sink", dict(sink, dtype=torch.int32, scale=(1, 1)), dtype3 + "torch.int32"),
        ("audio", dict(silent, stream="s", out=torch.zeros((1, 8), dtype=torch.int16)), "stream must be a torch.cuda.Stream of cuda:0, not 's'"),
    ]


def test_the_wording_of_the_shared_refusals_is_pinned():
    for entry, kwargs, message in _wording():
        call = _fake_audio().decode if entry == "audio" else getattr(_fake_batch(), entry)
        with pytest.raises(ValueError) as e:
            call(**kwargs)
        assert str(e.value) == message, (entry, sorted(kwargs))


@pytest.mark.gpu
def test_handles_of_the_swapped_library_work(profiling_library):
    import torch
    import mobiclipdecoder_amd as m
    from mobiclipdecoder_amd.demux import ModsDemuxer
    from tests.containers import write_mods
    from tests.test_demux import _frames

    samples = [1, -2, 300, -400, 5000, -6000, 32767]  # seven, and the two zero bytes a Moflex frame ends with: the eighth
    a = m.MobiclipAudio(1, 1, "pcm16", "moflex")
    assert a._lib is profiling_library
    out, ns, rc = a.decode([struct.pack("<7h", *samples) + b"\0\0"])
    torch.cuda.synchronize()
    assert rc.tolist() == [0] and ns.tolist() == [[8]] and out[0, 0, :8].cpu().tolist() == samples + [0]
    a.close()

    enc = m.MobiclipIntraEncoder(16, 16, m.MobiclipVersion.Moflex3DS, 1)
    assert enc._lib is profiling_library
    streams = enc.encode(np.full((1, 16 * 16 * 3 // 2), 128, np.uint8), 26)
    enc.close()
    b = m.MobiclipBatch(1, 16, 16, m.MobiclipVersion.Moflex3DS)
    rcs, offs = b.decode(streams, [0])
    assert rcs == [0] and 0 < offs[0] <= len(streams[0])
    b.close()

    p, _, frames = _frames("A", 9, iframe_interval=4)
    d = ModsDemuxer(write_mods(frames, p.width, p.height, [0, 4, 8]))
    assert d._lib is profiling_library and d.Header.keyframe_count == 3 and bytes(d.ReadFrame()[0]) == frames[0]
    d.close()
