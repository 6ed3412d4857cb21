"""The intra encoder (include/mobiclip_encode.h): a batch of I420 pictures to Mobiclip I-frames, one stream per picture, on the GPU.
Every stream decodes -- in the reference decoder and in MobiclipBatch -- to exactly the reconstruction the encoder reports; decisions and
bits are only ever produced by the HIP kernels (mobi_encode.hip).  DESIGN.md, "Intra encoder", has the rules.
_Encoder here is the one Python side of both encoders: this module's MobiclipIntraEncoder and encode_inter.py's MobiclipInterEncoder."""
import ctypes as C

import numpy as np

from .binding import Handle, bind
from .decoder import MobiclipError, _check_one_hip_runtime, check_rc, default_device, load_library

# mobi_enc_stats, one per picture
STATS_DTYPE = np.dtype([("bits", "<u8"), ("sad", "<u8"), ("luma_modes", "<u4", 4), ("chroma_modes", "<u4", 4), ("coded_blocks", "<u4"),
                        ("fallback_clamp", "<u4"), ("fallback_level", "<u4"), ("reserved", "<u4")])

_P = C.c_void_p
# names must match include/mobiclip_encode.h (tests/test_encode_model.py checks header, library and this table)
_SIGS = {
    "mobi_enc_create": (C.c_void_p, [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int]),
    "mobi_enc_destroy": (None, [C.c_void_p]),
    "mobi_enc_stream_bound": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "mobi_enc_check": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_size_t, _P, C.c_int, C.c_size_t]),
    "mobi_enc_intra_async": (C.c_int, [C.c_void_p, _P, C.c_int, _P, C.c_size_t, _P, C.c_int, _P, C.c_size_t, _P, _P, _P]),
    "mobi_enc_intra": (C.c_int, [C.c_void_p, C.c_int, _P, C.c_size_t, _P, C.c_int, _P, C.c_size_t, _P, _P, _P]),
}


def _lib():
    return bind(load_library(), _SIGS)


def stream_bound(width, height):
    """mobi_enc_stream_bound: no stream of a width x height picture is longer (bytes, a multiple of 4); 0 for refused dimensions"""
    return int(_lib().mobi_enc_stream_bound(width, height))


def _quantizers(q, n, what):
    qs = np.full(n, int(q), np.int64) if np.isscalar(q) else np.asarray([int(v) for v in q], np.int64)
    if qs.shape != (n,) or n < 1 or qs.min() < 0 or qs.max() > 255:
        raise ValueError(f"one {what}, or one per picture")
    return qs.astype(np.uint8)


class _Encoder(Handle):
    """What MobiclipIntraEncoder and MobiclipInterEncoder (encode_inter.py) share: creation and the one body of encode().  A subclass
    names its entry points (_prefix + _create / _check / _stream_bound, _call + _async and _call for host pointers) and their table
    (_sigs), its picture arrays as messages call them (_what), its statistics record (_stats) and the C arguments that stand between the
    quantisers and the slots when a call has none of its own to give (_no_extra).  The check and both calls take a pitch and a quantiser
    array per picture array."""
    _sigs = _prefix = _call = _what = _stats = _no_extra = None

    def __init__(self, width, height, version, max_pictures, device=None):
        self._h = None
        self._lib = bind(load_library(), self._sigs)
        self.width, self.height, self.version, self.max_pictures = int(width), int(height), int(version), int(max_pictures)
        self.device = default_device() if device is None else int(device)
        self.frame_bytes = self.width * self.height * 3 // 2
        self._check(1, (self.frame_bytes + 7) & ~7, [np.full(1, 12, np.uint8)] * len(self._what), self._no_extra, 0)
        self._h = getattr(self._lib, self._prefix + "_create")(self.max_pictures, self.width, self.height, self.version, self.device)
        if not self._h:
            raise MobiclipError(self._prefix + "_create failed: no usable HIP device, or out of device memory")
        self.stream_bound = int(getattr(self._lib, self._prefix + "_stream_bound")(self.width, self.height))

    def _check(self, n, pitch, qs, extra, slot):
        check_rc(getattr(self._lib, self._prefix + "_check")(self.max_pictures, self.width, self.height, self.version, n, *[pitch] * len(qs),
                                                             *[q.ctypes.data for q in qs], *extra, slot))

    def _encode(self, inputs, quantizers, extra, recon, stats, slot_bytes, stream):
        """inputs: the picture arrays; quantizers: per array (its quantiser or quantisers, their name in a message); extra: as _no_extra"""
        if not self._h:
            raise MobiclipError("encoder is closed")
        what = " and ".join(self._what)
        is_torch = type(inputs[0]).__module__.startswith("torch")
        if any(type(a).__module__.startswith("torch") != is_torch for a in inputs[1:]):
            raise ValueError(f"{what} must both be torch tensors or both numpy arrays")
        if not is_torch:
            inputs = [np.ascontiguousarray(a) for a in inputs]
            if any(a.dtype != np.uint8 for a in inputs):
                raise ValueError(f"{what} must be uint8")
        F = self.frame_bytes  # as a pitch a multiple of 8: width and height are multiples of 16
        if inputs[0].ndim != 2 or int(inputs[0].shape[1]) != F or any(tuple(a.shape) != tuple(inputs[0].shape) for a in inputs[1:]):
            raise ValueError(f"{what} must be (N, {F})")
        n = int(inputs[0].shape[0])
        qs = [_quantizers(q, n, name) for q, name in quantizers]
        slot = self.stream_bound if slot_bytes is None else int(slot_bytes)
        extras = {}
        if is_torch:
            import torch
            _check_one_hip_runtime()
            for t in inputs:
                if t.dtype != torch.uint8 or not t.is_cuda or (t.device.index or 0) != self.device:
                    raise ValueError(f"{what} must be {'a uint8 tensor' if len(inputs) == 1 else 'uint8 tensors'} on the encoder's device")
            inputs = [t.contiguous() for t in inputs]
            dev = inputs[0].device
            extra = [int(x) for x in extra]
            self._check(n, F, qs, extra, slot)
            s = torch.cuda.current_stream(dev) if stream is None else stream
            with torch.cuda.stream(s):  # torch's allocator then knows which stream uses the outputs
                out = torch.empty((n, slot), dtype=torch.uint8, device=dev)
                sizes = torch.empty((n,), dtype=torch.int32, device=dev)
                if recon:
                    extras["recon"] = torch.empty((n, F), dtype=torch.uint8, device=dev)
                if stats:
                    extras["stats"] = torch.empty((n, self._stats.itemsize), dtype=torch.uint8, device=dev)
            fn, head, ptr = getattr(self._lib, self._call + "_async"), (self._h, s.cuda_stream, n), lambda t: t.data_ptr()
        else:
            out = np.zeros((n, slot), np.uint8)
            sizes = np.zeros(n, np.int32)
            if recon:
                extras["recon"] = np.zeros((n, F), np.uint8)
            if stats:
                extras["stats"] = np.zeros(n, self._stats)
            extra = [int(x) for x in extra]
            fn, head, ptr = getattr(self._lib, self._call), (self._h, n), lambda a: a.ctypes.data
        check_rc(fn(*head, *[x for a in inputs for x in (ptr(a), F)], *[q.ctypes.data for q in qs], *extra, ptr(out), slot, ptr(sizes),
                    ptr(extras["recon"]) if recon else None, ptr(extras["stats"]) if stats else None))
        if is_torch:
            if slot_bytes is not None:
                return (out, sizes, extras) if extras else (out, sizes)
            s.synchronize()
            out, sizes = out.cpu().numpy(), sizes.cpu().numpy()
            if recon:
                extras["recon"] = extras["recon"].cpu().numpy()
            if stats:
                extras["stats"] = extras["stats"].cpu().numpy().view(self._stats).reshape(n)
        streams = [out[i, :sizes[i]].tobytes() if sizes[i] <= slot else b"" for i in range(n)]
        if slot_bytes is not None:
            extras["sizes"] = sizes
            extras["slots"] = out
        return (streams, extras) if extras else streams


class MobiclipIntraEncoder(_Encoder):
    """mobi_enc: I-frames of width x height pictures for MobiclipVersion.Moflex3DS or .ModsDS, up to max_pictures per call."""
    _destroy = "mobi_enc_destroy"
    _sigs, _prefix, _call, _what, _stats, _no_extra = _SIGS, "mobi_enc", "mobi_enc_intra", ("pictures",), STATS_DTYPE, (0,)

    def encode(self, pictures, quantizer, yuv_format=0, recon=False, stats=False, slot_bytes=None, stream=None):
        """pictures: (N, width * height * 3 / 2) uint8, packed I420 as export_tensor("i420") writes it -- a torch tensor on the encoder's
        device (encoded where it lies, on `stream` or torch's current one) or a numpy array (the synchronous host entry point).
        quantizer: an int in [12, 52] or one per picture.  slot_bytes: the room of one stream (a multiple of 4; default: the bound).

        Returns a list of N bytes objects.  For a torch input with slot_bytes given: (streams, sizes) -- an (N, slot_bytes) uint8 and an
        (N,) int32 tensor, enqueued and not waited for; a stream longer than slot_bytes leaves its slot zero and its true size in sizes.
        With recon and / or stats a dict follows as the last element: "recon" (N, frame) uint8, "stats" (N,) STATS_DTYPE (for the
        unsynchronised torch form an (N, 64) uint8 tensor: .cpu().numpy().view(STATS_DTYPE))."""
        return self._encode([pictures], [(quantizer, "quantizer")], (yuv_format,), recon, stats, slot_bytes, stream)

    def encode_target(self, pictures, target_bytes, qmin=12, qmax=52, yuv_format=0, recon=False, stats=False, slot_bytes=None, stream=None):
        """encode() with a byte target per picture in place of the quantiser (include/mobiclip_encode_rate.h): the quantiser is found on the
        GPU by a bisection of [qmin, qmax] over trial encodes; the stream is no longer than its target, or its quantiser is qmax.
        pictures: a torch tensor on the encoder's device only.  target_bytes: an int, one per picture, or an (N,) int32 tensor on the device.

        Returns what encode() returns for a tensor, the dict always present and holding "quantizer": the (N,) uint8 chosen quantisers (a
        device tensor in the unsynchronised form, i.e. with slot_bytes given)."""
        from .encode_rate import encode_target
        return encode_target(self, "mobi_enc_intra_target_async", [pictures], None, target_bytes, qmin, qmax, (yuv_format,), recon, stats, slot_bytes, stream)
