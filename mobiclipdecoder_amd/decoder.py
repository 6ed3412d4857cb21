"""Host-side mirror of the reference decoder class over the C ABI (include/mobiclip_hip.h).

``MobiclipDecoder`` keeps the public surface of LibMobiclip.Codec.Mobiclip.MobiclipDecoder
(MobiclipDecoder.cs:13-61): ctor ``(Width, Height, Version)``, fields ``Data`` / ``Offset`` /
``Width`` / ``Height`` / ``Stride`` / ``Quantizer`` / ``YuvFormat``, plane accessors ``Y[i]`` /
``UV[i]`` and ``DecodeFrame()``.  The callers' contract (MobiConverter/Program.cs:69-71,243-250):

    d.Data = frame; d.Offset = 0; d.DecodeFrame(); audio_start = d.Offset - 2

Differences, on purpose: ``DecodeFrame`` returns the planes (Y, UV) instead of a System.Drawing
Bitmap (the RGB conversion MD.cs:260-323 is outside the graded path), and where the reference
swallows every exception and returns null (MD.cs:325-328) this returns ``None`` and leaves the
reason in ``last_error``.  Reconstruction runs only on the GPU; there is no CPU fallback.
"""
import ctypes as C
import enum
import os
import weakref

import numpy as np

from .binding import Handle, as_u8, bind, byte_arrays

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class MobiclipVersion(enum.IntEnum):  # MD.cs:32-37
    VxDS = 0
    ModsDS = 1
    Moflex3DS = 2


class MobiclipError(RuntimeError):
    pass


MOBI_E_ARG = -7  # include/mobiclip_hip.h
MOBI_IDLE = 1  # rc of a frame slot marked idle (MobiclipBatch.set_idle): not an error


# names must match include/mobiclip_hip.h (tests/test_abi_symbols.py checks the header against the .so)
_SIGS = {
    "mobi_create": (C.c_void_p, [C.c_uint32, C.c_uint32, C.c_int, C.c_int]),
    "mobi_destroy": (None, [C.c_void_p]),
    "mobi_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]),
    "mobi_get_planes": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mobi_get_argb": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mobi_selftest_div239": (C.c_longlong, [C.c_int]),
    "mobi_stride": (C.c_int, [C.c_void_p]),
    "mobi_quantizer": (C.c_uint32, [C.c_void_p]),
    "mobi_yuv_format": (C.c_uint32, [C.c_void_p]),
    "mobi_width": (C.c_uint32, [C.c_void_p]),
    "mobi_height": (C.c_uint32, [C.c_void_p]),
    "mobi_batch_create": (C.c_void_p, [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int]),
    "mobi_batch_destroy": (None, [C.c_void_p]),
    "mobi_batch_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mobi_batch_submit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mobi_batch_wait": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mobi_batch_in_flight": (C.c_int, [C.c_void_p]),
    "mobi_batch_decode_gop": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mobi_batch_gop_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mobi_batch_gop_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mobi_batch_gop_in_flight": (C.c_int, [C.c_void_p]),
    "mobi_batch_gop_frames_pending": (C.c_int, [C.c_void_p]),
    "mobi_batch_host_clips": (C.c_int, [C.c_void_p]),
    "mobi_batch_compare_clips": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mobi_forward_dct": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "mobi_encoder_qtables": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p]),
    "mobi_transform_code": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mobi_transform_code_async": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mobi_batch_get_planes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mobi_batch_convert_argb": (C.c_int, [C.c_void_p]),
    "mobi_batch_get_argb": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mobi_batch_get_argb_at": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mobi_batch_quantizer": (C.c_uint32, [C.c_void_p, C.c_int]),
    "mobi_batch_yuv_format": (C.c_uint32, [C.c_void_p, C.c_int]),
    "mobi_batch_set_parse_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "mobi_batch_lockstep_finished": (C.c_int, [C.c_void_p]),
    "mobi_batch_reset_clips": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "mobi_batch_clip_frames": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mobi_batch_set_idle": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "mobi_batch_clip_idle": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mobi_batch_idle_launches": (C.c_int, [C.c_void_p]),
    "mobi_batch_last_decode_ms": (C.c_float, [C.c_void_p]),
    "mobi_batch_motion_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mobi_batch_stride": (C.c_int, [C.c_void_p]),
    "mobi_batch_n_clips": (C.c_int, [C.c_void_p]),
    "mobi_batch_preload": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    "mobi_batch_preload_clone": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mobi_batch_commit": (C.c_int, [C.c_void_p]),
    "mobi_batch_replay": (C.c_int, [C.c_void_p, C.c_int]),
    "mobi_batch_sync": (C.c_int, [C.c_void_p]),
    "mobi_batch_cmd_bytes": (C.c_uint64, [C.c_void_p, C.c_int]),
    "mobi_batch_intra_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mobi_batch_time_begin": (C.c_int, [C.c_void_p]),
    "mobi_batch_time_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mobi_batch_set_kernel_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "mobi_batch_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mobi_host_alloc": (C.c_void_p, [C.c_size_t]),
    "mobi_host_free": (None, [C.c_void_p]),
    "mobi_batch_export": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "mobi_batch_export_wait": (C.c_int, [C.c_void_p, C.c_uint64]),
    "mobi_batch_export_query": (C.c_int, [C.c_void_p, C.c_uint64]),
    "mobi_batch_export_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_size_t, C.c_void_p]),
    "mobi_batch_export_device_scaled": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)] + [C.c_int] * 10 + [C.c_void_p, C.c_size_t,
                                                                                                                       C.c_void_p]),
    "mobi_batch_export_device_boxes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int32)] + [C.c_int] * 6
                                       + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "mobi_batch_set_motion": (C.c_int, [C.c_void_p, C.c_int]),
    "mobi_batch_motion_launches": (C.c_long, [C.c_void_p]),
    "mobi_batch_motion_bytes": (C.c_size_t, [C.c_void_p]),
    "mobi_batch_export_motion": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_size_t, C.c_void_p]),
    "mobi_batch_set_sink": (C.c_int, [C.c_void_p, C.c_void_p]),  # (a mobi_sink by reference: C.byref(SinkSpec), or None)
    "mobi_batch_sink_pending": (C.c_int, [C.c_void_p]),
    "mobi_batch_sink_launches": (C.c_long, [C.c_void_p]),
    "mobi_sink_check": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32]),
    "mobi_sink_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "mobi_batch_gop_finish_all": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mobi_error_string": (C.c_char_p, [C.c_int]),
    "mobi_build_info": (C.c_char_p, []),
}

LIB_PATH = os.environ.get("MOBI_LIB") or os.path.join(_HERE, "libmobiclip_hip.so")  # MOBI_LIB: A/B-test another build of the library


def bind_library(path):
    """dlopen one build of the library and bind every entry point of include/mobiclip_hip.h"""
    return bind(C.CDLL(path), _SIGS)


def load_library():
    """dlopen libmobiclip_hip.so and bind every entry point.  Raises if it was not built: the HIP
    library is the only implementation, there is nothing to fall back to."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: run `python -m mobiclipdecoder_amd.build` (or __graft_entry__.build())")
        _LIB = bind_library(LIB_PATH)
    return _LIB


def default_device():
    """HIP ordinal used when a caller names none: MOBI_DEVICE (default 0).  Lets a whole test run exercise another GPU of the node --
    MOBI_DEVICE=1 python -m pytest tests -m gpu -- so that no code path is only ever reached with ordinal 0 (the path shards by clip over
    GPUs: SURVEY.md 8(e))."""
    return int(os.environ.get("MOBI_DEVICE", "0"))


def error_string(rc):
    return load_library().mobi_error_string(rc).decode()


def check_rc(rc, counts=False, null_ok=False):
    """The rc of a library call, handed back; MobiclipError with the library's text for it when it is not 0 -- when it is negative, for an
    entry that returns a count (counts) -- and not the MOBI_E_NULLREF of a ring slot never filled, where that is an answer (null_ok)."""
    if (rc < 0 if counts else rc != 0) and not (null_ok and rc == -2):
        raise MobiclipError(error_string(rc))
    return rc


class _PlaneRing:
    """d.Y[i] / d.UV[i] (MD.cs:19-20): device ring slot i copied to a numpy array on access."""

    def __init__(self, dec, which):
        self._dec, self._which = dec, which

    def __getitem__(self, idx):
        return self._dec._plane(idx, self._which)

    def __len__(self):
        return 6


# mobi_batch_export formats (include/mobiclip_hip.h, MOBI_EXPORT_*)
EXPORT_FORMATS = {"i420": 0, "argb": 1}
# mobi_batch_export_device: (fmt, layout) -> MOBI_EXPORT_*; torch dtype name -> MOBI_DTYPE_*
DEVICE_EXPORT_FORMATS = {("i420", None): 0, ("argb", None): 1, ("rgb", "nchw"): 2, ("rgb", "nhwc"): 3}
DEVICE_EXPORT_DTYPES = {"uint8": 0, "float16": 1, "float32": 2}
# mobi_batch_export_motion: fmt -> (MOBI_MOTION_*, channels, the block size it has or None for a choice, torch dtype names: the first is the
# default); torch dtype name -> MOBI_DTYPE_*
MOTION_FORMATS = {"cells": (0, 3, 2, ("int16",)), "mb": (1, 5, 16, ("int32",)), "flow": (2, 2, None, ("float32", "float16"))}
MOTION_DTYPES = {"float16": 1, "float32": 2, "int16": 3, "int32": 4}


class SinkSpec(C.Structure):
    """struct mobi_sink of include/mobiclip_hip.h (mobi_batch_set_sink, mobi_sink_check, mobi_sink_plan)"""
    _fields_ = [("format", C.c_int), ("dtype", C.c_int), ("scale_bias", C.POINTER(C.c_float)), ("boxes", C.POINTER(C.c_int32)),
                ("out_w", C.c_int), ("out_h", C.c_int), ("n_frames", C.c_int), ("stride", C.c_int), ("start", C.POINTER(C.c_int32)),
                ("clip_stride", C.c_int64), ("frame_stride", C.c_int64), ("chan_stride", C.c_int64), ("dst", C.c_void_p),
                ("dst_bytes", C.c_size_t)]


# MobiclipBatch.set_sink: layout -> (planar?, the tensor's dimensions as letters: n clips, t frames, c channels, h, w)
SINK_LAYOUTS = {"ntchw": (True, "ntchw"), "ncthw": (True, "ncthw"), "nthwc": (False, "nthwc"), "tnchw": (True, "tnchw"), "tnhwc": (False, "tnhwc")}


class _HostBlock:
    """One mobi_host_alloc block (pinned, portable host memory) seen by numpy through the array interface; mobi_host_free runs when the
    last array over it is gone."""

    def __init__(self, nbytes):
        lib = load_library()
        self.ptr = lib.mobi_host_alloc(max(1, int(nbytes)))
        if not self.ptr:
            raise MobiclipError(f"mobi_host_alloc({nbytes}) failed (a HIP device is required)")
        self.__array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (self.ptr, False), "version": 3}
        weakref.finalize(self, lib.mobi_host_free, self.ptr)


def host_empty(shape, dtype=np.uint8):
    """np.empty() in memory from mobi_host_alloc: an export into it returns at once (MobiclipBatch.export(..., wait=False))"""
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(d) for d in shape)
    dt = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
    return np.asarray(_HostBlock(n))[:n].view(dt).reshape(shape)


def split_i420(arr, W, H):
    """(Y, U, V) views of packed I420 pictures (MobiclipBatch.export(fmt="i420")): arr[..., W*H*3/2] -> [..., H, W], [..., H/2, W/2] x 2"""
    a = np.asarray(arr)
    ys, cs = W * H, (W // 2) * (H // 2)
    if a.shape[-1] != ys + 2 * cs:
        raise ValueError(f"last dimension {a.shape[-1]} is not a {W}x{H} I420 picture ({ys + 2 * cs} bytes)")
    lead = a.shape[:-1]
    return (a[..., :ys].reshape(lead + (H, W)), a[..., ys:ys + cs].reshape(lead + (H // 2, W // 2)),
            a[..., ys + cs:].reshape(lead + (H // 2, W // 2)))


class ExportHandle:
    """An export in flight (MobiclipBatch.export(..., wait=False)): done() asks, wait() waits and returns the array.  Keeps the destination
    and the batch alive until then."""

    def __init__(self, batch, ticket, out):
        self._batch, self.ticket, self.out = batch, ticket, out

    def done(self):
        if not self._batch._h:
            return True  # (mobi_batch_destroy waited for it)
        return check_rc(self._batch._lib.mobi_batch_export_query(self._batch._h, self.ticket), counts=True) == 1

    def wait(self):
        if self._batch._h:
            check_rc(self._batch._lib.mobi_batch_export_wait(self._batch._h, self.ticket))
        return self.out


class MobiclipDecoder(Handle):
    _destroy = "mobi_destroy"

    def __init__(self, Width, Height, Version, device=None):
        self._lib = load_library()
        self.Width, self.Height, self.Version = int(Width), int(Height), MobiclipVersion(Version)
        device = default_device() if device is None else device
        self._h = self._lib.mobi_create(self.Width, self.Height, int(self.Version), device)
        if not self._h:
            raise MobiclipError(
                f"mobi_create({Width},{Height},{Version},dev={device}) failed: {error_string(-8)} "
                "(dimensions must be multiples of 16; a HIP device is required)")
        self.Data = None
        self.Offset = 0
        self.last_error = 0
        self.Y = _PlaneRing(self, 0)
        self.UV = _PlaneRing(self, 1)

    # -- reference fields -------------------------------------------------------------------
    @property
    def Stride(self):
        return self._lib.mobi_stride(self._h)

    @property
    def Quantizer(self):
        return self._lib.mobi_quantizer(self._h)

    @property
    def YuvFormat(self):
        return self._lib.mobi_yuv_format(self._h)

    # -- reference method -------------------------------------------------------------------
    def DecodeFrame(self):
        """MD.cs:56-61.  Returns (Y, UV) of the new frame, or None where the reference returns null."""
        if self.Data is None:
            self.last_error = -2
            return None
        buf = as_u8(self.Data)
        off = C.c_int32(int(self.Offset))
        rc = self._lib.mobi_decode(self._h, buf.ctypes.data, buf.size, C.byref(off))
        self.Offset = off.value
        self.last_error = rc
        if rc != 0:
            return None
        return self._plane(0, 0), self._plane(0, 1)

    def _plane(self, idx, which):
        S, H = self.Stride, self.Height
        y = np.empty(S * H, np.uint8) if which == 0 else None
        uv = np.empty(S * H // 2, np.uint8) if which == 1 else None
        rc = self._lib.mobi_get_planes(self._h, idx, y.ctypes.data if y is not None else None,
                                       uv.ctypes.data if uv is not None else None)
        if check_rc(rc, null_ok=True):
            return None  # null slot, like the reference's unfilled ring entries
        return (y.reshape(H, S) if which == 0 else uv.reshape(H // 2, S))

    def Bitmap(self):
        """The Bitmap DecodeFrame() returns in the reference (MD.cs:260-323), for the frame just decoded:
        (Height, Width) uint32 array of 0xAARRGGBB; None before the first frame."""
        out = np.empty((self.Height, self.Width), np.uint32)
        return None if check_rc(self._lib.mobi_get_argb(self._h, out.ctypes.data), null_ok=True) else out


def _check_frames(ring_idx, n_frames):
    """the frames of an export: ring indices ring_idx .. ring_idx - n_frames + 1"""
    if isinstance(ring_idx, bool) or not isinstance(ring_idx, (int, np.integer)) or not 0 <= ring_idx <= 5:
        raise ValueError(f"ring_idx must be an int in 0..5, not {ring_idx!r}")
    if isinstance(n_frames, bool) or not isinstance(n_frames, (int, np.integer)) or not 1 <= n_frames <= ring_idx + 1:
        raise ValueError(f"n_frames must be an int in 1..ring_idx + 1 = {ring_idx + 1}, not {n_frames!r}")


def _ints(name, v, n):
    """v, a tuple or list of n ints (no bools), as a list of int"""
    if not isinstance(v, (tuple, list)) or len(v) != n or any(isinstance(i, bool) or not isinstance(i, (int, np.integer)) for i in v):
        raise ValueError(f"{name} must be {n} ints, not {v!r}")
    return [int(i) for i in v]


# -- the arguments an entry point takes from torch, each checked in one place: the entry points differ in which checks they make, in their
# order and in some wording (`refusal`), not in the checks themselves --------------------------------------------------------------------
def dtype_name(dtype, allowed, refusal):
    """the name of a torch.dtype ("float16" for torch.float16) when `allowed` holds it, ValueError(refusal) for anything else"""
    import torch
    name = str(dtype).split(".")[-1] if isinstance(dtype, torch.dtype) else None
    if name not in allowed:
        raise ValueError(refusal)
    return name


def scale_bias(scale, bias, applies, refusal):
    """scale and bias of an RGB export (three floats each; None: 1 and 0) as the library's float[6], None when both are None;
    ValueError(refusal) when one is given where they do not apply"""
    if scale is None and bias is None:
        return None
    if not applies:
        raise ValueError(refusal)
    vals = []
    for name, v, dflt in (("scale", scale, 1.0), ("bias", bias, 0.0)):
        v = [dflt] * 3 if v is None else v
        try:
            v = [float(x) for x in v]
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be three floats, not {v!r}") from None
        if len(v) != 3 or not all(np.isfinite(v)):
            raise ValueError(f"{name} must be three finite floats, not {v!r}")
        vals += v
    return (C.c_float * 6)(*np.asarray(vals, np.float32).tolist())


def check_stream(stream, dev):
    import torch
    if stream is not None and (not isinstance(stream, torch.cuda.Stream) or stream.device != dev):
        raise ValueError(f"stream must be a torch.cuda.Stream of {dev}, not {stream!r}")


def check_out(out, dev, dtype, shape, aligned=True):
    """out, where it is given: a contiguous tensor of this dtype and shape on dev, 16-byte aligned where the kernel stores vectors"""
    import torch
    if out is not None and (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != dtype or tuple(out.shape) != shape
                            or not out.is_contiguous() or (aligned and out.data_ptr() % 16)):
        raise ValueError(f"out must be a contiguous{', 16-byte aligned' if aligned else ''} {dtype} tensor of shape {shape} on {dev}")


def stream_and_out(stream, out, dev, dtype, shape):
    """behind the last argument check: one HIP runtime in the process; no stream = the device's current one; no out = a new tensor,
    allocated on the stream (torch's allocator then knows which stream uses it) -> (stream, out)"""
    import torch
    _check_one_hip_runtime()
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    if out is None:
        with torch.cuda.stream(stream):
            out = torch.empty(shape, dtype=dtype, device=dev)
    return stream, out


def tensor_bytes(t):
    """the bytes of a contiguous tensor: the room the library is told it may write"""
    return t.numel() * t.element_size()


def _rows(flat, K, n):
    """a C array [k * n + c] as K lists of n"""
    return [list(flat[k * n:(k + 1) * n]) for k in range(K)]


def unpack_motion_search(words):
    """Packed results of mobi_batch_motion_search / the oracle -> dict(dx, dy, frame, score)."""
    w = np.asarray(words, dtype=np.uint32)
    return {"dx": (w & 0xFF).astype(np.int8).astype(np.int32), "dy": ((w >> 8) & 0xFF).astype(np.int8).astype(np.int32),
            "frame": ((w >> 16) & 7).astype(np.int32), "score": (w >> 20).astype(np.int32), "packed": w}


class MobiclipBatch(Handle):
    """N independent decoder instances of equal geometry decoded in lock step on one GPU
    (decoder instances share nothing: MD.cs:15-39).  Also the pre-parsed replay path used for
    throughput measurement."""
    _destroy = "mobi_batch_destroy"

    def __init__(self, n_clips, Width, Height, Version, device=None, device_parse=None):
        """device_parse: True = decode() parses the bitstreams on the GPU (one wavefront per clip, mobi_dparse.hip),
        "lockstep" = the same with the lock-step parser in front (clips in lock step, one per lane, mobi_lsparse.hip),
        False = on host threads, "hybrid" = most clips on the GPU and a fixed share (a fifth, at most 1024) on the host pool at the same
        time, None = library default (device parse from 20 clips per host parse thread, 640 at least; env MOBI_DEVICE_PARSE=0/1/2)."""
        self._lib = load_library()
        self.n, self.Width, self.Height, self.Version = int(n_clips), int(Width), int(Height), MobiclipVersion(Version)
        device = default_device() if device is None else device
        self.device = int(device)
        self._h = self._lib.mobi_batch_create(self.n, self.Width, self.Height, int(self.Version), self.device)
        if not self._h:
            raise MobiclipError(f"mobi_batch_create failed: {error_string(-8)}")
        self.Stride = self._lib.mobi_batch_stride(self._h)
        if device_parse is not None:
            if isinstance(device_parse, int) and not isinstance(device_parse, bool):
                mode = device_parse  # the library's own numbering: 0 host, 1 device, 2 hybrid, 3 device with the lock-step parser in front
            else:
                mode = 2 if device_parse == "hybrid" else 3 if device_parse == "lockstep" else int(bool(device_parse))
            check_rc(self._lib.mobi_batch_set_parse_mode(self._h, mode))

    def decode(self, datas, offsets):
        """One DecodeFrame() per clip.  datas: list of byte buffers; offsets: list of ints.
        Returns (rc list, new offsets list)."""
        bufs, ptrs, lens = byte_arrays(datas, self.n)
        offs = (C.c_int32 * self.n)(*[int(o) for o in offsets])
        rcs = (C.c_int * self.n)()
        check_rc(self._lib.mobi_batch_decode(self._h, ptrs, lens, offs, rcs))
        return list(rcs), list(offs)

    def submit(self, datas, offsets):
        """Asynchronous decode(): enqueue one frame step (device parse only, at most two in flight); the buffers may be reused at
        once.  Results come from wait(), oldest step first."""
        bufs, ptrs, lens = byte_arrays(datas, self.n)
        offs = (C.c_int32 * self.n)(*[int(o) for o in offsets])
        check_rc(self._lib.mobi_batch_submit(self._h, ptrs, lens, offs))

    # -- frame-parallel groups: K consecutive frames of every clip per call (mobiclip_hip.h, mobi_batch_decode_gop) -------------
    def _gop_arrays(self, frames, offsets):
        """frames[k][c] = byte buffer of frame k of clip c; offsets[k][c] (or None: all 0) -> the C arrays, [k * n + c]"""
        K = len(frames)
        for k, fr in enumerate(frames):
            if len(fr) != self.n:
                raise ValueError(f"frames[{k}] has {len(fr)} entries, the batch has {self.n} clips")
        if offsets is not None and (len(offsets) != K or any(len(row) != self.n for row in offsets)):
            raise ValueError(f"offsets must have the shape of frames: {K} rows of {self.n}")
        bufs, ptrs, lens = byte_arrays([d for fr in frames for d in fr], K * self.n)
        flat = [0] * (K * self.n) if offsets is None else [int(o) for row in offsets for o in row]
        offs = (C.c_int32 * (K * self.n))(*flat)
        return K, bufs, ptrs, lens, offs

    def decode_gop(self, frames, offsets=None):
        """K = len(frames) <= 6 DecodeFrame() calls per clip in one go, parsed side by side on the GPU.  -> (rc, offsets), each a list of
        K lists of n: exactly what K decode() calls return."""
        K, bufs, ptrs, lens, offs = self._gop_arrays(frames, offsets)
        rcs = (C.c_int * (K * self.n))()
        check_rc(self._lib.mobi_batch_decode_gop(self._h, K, ptrs, lens, offs, rcs))
        return _rows(rcs, K, self.n), _rows(offs, K, self.n)

    def gop_begin(self, frames, offsets=None):
        """first half of decode_gop(): gather, upload (and parse, when no group is in front); at most two groups begun and not finished"""
        K, bufs, ptrs, lens, offs = self._gop_arrays(frames, offsets)
        check_rc(self._lib.mobi_batch_gop_begin(self._h, K, ptrs, lens, offs))

    def _gop_finish(self, entry, K):
        """(rc, offsets) of K frames of the oldest group begun, from mobi_batch_gop_finish or mobi_batch_gop_finish_all"""
        offs = (C.c_int32 * max(1, K * self.n))()
        rcs = (C.c_int * max(1, K * self.n))()
        check_rc(entry(self._h, offs, rcs))
        return _rows(rcs, K, self.n), _rows(offs, K, self.n)

    def gop_finish(self):
        """second half, for the OLDEST group begun: hand-overs, the reconstruction steps; -> (rc, offsets) as decode_gop().  A group of more
        than six frames (gop_begin takes up to 128) is handed out six at a time: call again while gop_frames_pending() > 0."""
        return self._gop_finish(self._lib.mobi_batch_gop_finish, min(6, self._lib.mobi_batch_gop_frames_pending(self._h)))

    def gop_frames_pending(self):
        return self._lib.mobi_batch_gop_frames_pending(self._h)

    def compare_clips(self, modulus):
        """clips whose newest frame differs from that of clip (index mod modulus), compared on the device (batches made of copies)"""
        return check_rc(self._lib.mobi_batch_compare_clips(self._h, int(modulus), None), counts=True)

    def host_clips(self):
        """clips the host parser parses at present: all of them in host mode, else the hybrid share plus every clip that has had a frame
        the device parser could not finish (the result is the same either way: mobiclip_hip.h, mobi_batch_set_parse_mode)"""
        return self._lib.mobi_batch_host_clips(self._h)

    def lockstep_finished(self):
        """device_parse="lockstep": clips of the last finished step the lock-step parser finished itself (-1 in other modes)."""
        return self._lib.mobi_batch_lockstep_finished(self._h)

    def reset_clips(self, clips):
        """A new MobiclipDecoder for each of `clips` (ints, or a bool mask of length n) from the next step handed over on: start the
        next file -- or seek to an I-frame -- in a slot whose stream has ended.  Waits for nothing; steps and groups in flight, and the
        pictures in the ring, are not touched (mobiclip_hip.h, mobi_batch_reset_clips)."""
        arr = np.asarray(clips)
        if arr.dtype == np.bool_:
            if arr.shape != (self.n,):
                raise ValueError(f"a clip mask must have {self.n} entries, not {arr.shape}")
            idx = np.flatnonzero(arr)
        else:
            arr = arr.reshape(-1)
            if arr.size and not np.issubdtype(arr.dtype, np.integer):
                raise ValueError("clips must be integers or a bool mask")
            idx = arr.astype(np.int64)
            if idx.size and (idx.min() < 0 or idx.max() >= self.n):
                raise ValueError(f"clip index outside [0, {self.n})")
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        check_rc(self._lib.mobi_batch_reset_clips(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), int(idx.size)))

    def set_idle(self, mask):
        """Mark frame slots of the NEXT step or group handed over as idle: "this clip has no frame here, its stream has ended".  mask:
        array-like [K][n] (groups) or [n] (decode / submit), nonzero = idle; None drops a mask not consumed yet.  An idle slot is not
        parsed, changes no decoder state and writes no pixel; its rc is MOBI_IDLE and its entry in datas / frames may be None.  The idle
        slots of a clip are a suffix of a group, and the clip takes live frames again only after reset_clips (mobiclip_hip.h,
        mobi_batch_set_idle)."""
        if mask is None:
            e = self._lib.mobi_batch_set_idle(self._h, None, 0)
        else:
            m = np.asarray(mask)
            if m.ndim == 1:
                m = m.reshape(1, -1)
            if m.ndim != 2 or m.shape[1] != self.n or not 1 <= m.shape[0] <= 128:
                raise ValueError(f"an idle mask is [K][{self.n}] or [{self.n}], 1 <= K <= 128, not {np.asarray(mask).shape}")
            m = np.ascontiguousarray(m != 0, dtype=np.uint8)
            e = self._lib.mobi_batch_set_idle(self._h, m.ctypes.data, int(m.shape[0]))
        check_rc(e)

    def clip_idle(self):
        """int32[n]: idle slots handed over per clip since its last live frame or reset (steps and groups in flight included).  Ring
        index r of clip c holds a picture of its current stream iff clip_idle()[c] <= r < min(6, clip_idle()[c] + clip_frames()[c])."""
        out = np.zeros(self.n, np.int32)
        check_rc(self._lib.mobi_batch_clip_idle(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def idle_launches(self):
        """launches of the idle-slot kernel so far (0 for a batch that never had an idle slot)"""
        return self._lib.mobi_batch_idle_launches(self._h)

    def clip_frames(self):
        """int32[n]: LIVE frames handed over per clip since the batch was created or the clip was last reset (steps in flight and every
        frame of a finished group part count; idle slots do not); without idle slots ring index r of clip c holds the current stream's
        picture iff r < min(6, that) -- clip_idle() has the general rule."""
        out = np.zeros(self.n, np.int32)
        check_rc(self._lib.mobi_batch_clip_frames(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def wait(self):
        """(rc list, new offsets list) of the oldest submitted step, when its reconstruction is done."""
        offs = (C.c_int32 * self.n)()
        rcs = (C.c_int * self.n)()
        check_rc(self._lib.mobi_batch_wait(self._h, offs, rcs))
        return list(rcs), list(offs)

    def planes(self, clip, idx=0):
        S, H = self.Stride, self.Height
        y = np.empty(S * H, np.uint8)
        uv = np.empty(S * H // 2, np.uint8)
        if check_rc(self._lib.mobi_batch_get_planes(self._h, clip, idx, y.ctypes.data, uv.ctypes.data), null_ok=True):
            return None
        return y.reshape(H, S), uv.reshape(H // 2, S)

    def convert_argb(self):
        """Bitmaps of every clip's current frame into a device-resident buffer (asynchronous)."""
        check_rc(self._lib.mobi_batch_convert_argb(self._h))

    def bitmap(self, clip, idx=0):
        """the Bitmap of the frame at ring index idx (0 = the newest)"""
        out = np.empty((self.Height, self.Width), np.uint32)
        check_rc(self._lib.mobi_batch_get_argb_at(self._h, clip, idx, out.ctypes.data) if idx else self._lib.mobi_batch_get_argb(self._h, clip, out.ctypes.data))
        return out

    def _clip_range(self, clips):
        """the clips argument of the exports as a range: None = all clips, a slice is taken of them"""
        if clips is None:
            clips = range(self.n)
        elif isinstance(clips, slice):
            clips = range(self.n)[clips]
        if not isinstance(clips, range) or clips.step != 1 or len(clips) < 1 or clips.start < 0 or clips.stop > self.n:
            raise ValueError(f"clips must be a non-empty range / slice of step 1 inside 0..{self.n}, not {clips!r}")
        return clips

    def export(self, fmt="i420", ring_idx=0, n_frames=1, clips=None, out=None, wait=True):
        """Pictures of many clips and frames to host memory in one call (mobi_batch_export): frame j = ring index ring_idx - j (oldest first),
        clips = a range / slice of clip numbers (step 1; None: all).  -> (n_frames, n_clips, W*H*3/2) uint8 (fmt="i420"; split_i420) or
        (n_frames, n_clips, H, W) uint32 Bitmaps (fmt="argb").  out: an array of that shape and type to fill (default: host_empty()); with
        wait=False an ExportHandle is returned at once -- the export runs behind the steps enqueued so far -- when out is host_empty() memory."""
        if fmt not in EXPORT_FORMATS:
            raise ValueError(f"fmt must be one of {sorted(EXPORT_FORMATS)}, not {fmt!r}")
        _check_frames(ring_idx, n_frames)
        clips = self._clip_range(clips)
        W, H = self.Width, self.Height
        shape, dtype = ((n_frames, len(clips), W * H * 3 // 2), np.uint8) if fmt == "i420" else ((n_frames, len(clips), H, W), np.uint32)
        if out is None:
            out = host_empty(shape, dtype)
        elif (not isinstance(out, np.ndarray) or out.shape != shape or out.dtype != dtype or not out.flags.c_contiguous
              or not out.flags.writeable):
            raise ValueError(f"out must be a writeable C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        ticket = C.c_uint64(0)
        check_rc(self._lib.mobi_batch_export(self._h, EXPORT_FORMATS[fmt], int(ring_idx), int(n_frames), clips.start, len(clips), out.ctypes.data,
                                             out.nbytes, C.byref(ticket)))
        h = ExportHandle(self, ticket.value, out)
        return h.wait() if wait else h

    def export_tensor(self, fmt="rgb", ring_idx=0, n_frames=1, clips=None, layout="nchw", dtype=None, scale=None, bias=None, out=None,
                      stream=None, crop=None, size=None, boxes=None, flip=None):
        """Pictures of many clips and frames into a torch tensor on the batch's GPU (mobi_batch_export_device), enqueued on `stream`
        (default: torch.cuda.current_stream of the batch's device) without a host wait: work enqueued on that stream afterwards sees them.
        Frame j = ring index ring_idx - j (oldest first), clips = a range / slice of step 1 (None: all), as in export().

        fmt="i420": (F, N, W*H*3/2) uint8, byte for byte what export() gives (split_i420 works on it).
        fmt="argb": (F, N, H, W) int32 with the bits of the uint32 Bitmap.
        fmt="rgb":  layout "nchw" -> (F, N, 3, H, W), "nhwc" -> (F, N, H, W, 3); dtype torch.uint8 (the Bitmap's R, G, B bytes, the default),
                    torch.float16 or torch.float32: v * scale[ch] + bias[ch] in float32 (a product and a sum, each rounded), float16 rounded
                    from that.  scale, bias: three floats each (default 1 and 0), for float dtypes only.  Normalising with a mean and a
                    standard deviation is scale = 1 / std, bias = -mean / std, rounded to float32 first.
        crop=(x, y, w, h), size=(out_h, out_w) (fmt="rgb" only; mobi_batch_export_device_scaled): the crop of every picture (default: the
                    whole picture), area-averaged down to out_h x out_w (default: the crop's size, a pure crop) in one kernel, exactly (the
                    definition is include/mobiclip_hip.h's); H, W in the shapes above become out_h, out_w.  No upscaling, out_w a multiple
                    of 4, w * h <= 2**23.  With both None the call is the full-size export.
        boxes=(len(clips), 4) ints, rows (x, y, w, h); flip=len(clips) bools or None; size=(out_h, out_w), required (fmt="rgb" only;
                    mobi_batch_export_device_boxes): clip i's box of every frame, resized to out_h x out_w -- area-averaged where an axis
                    shrinks, bilinear (half-pixel centres, clamped at the box's edge) where it grows -- and mirrored left to right where
                    flip[i], in one kernel, exactly (include/mobiclip_hip.h).  out_w a multiple of 4; dx * dy <= 2**23 with d = the box's
                    side where the axis shrinks, twice the output's where it grows.  Not together with crop.
        out: a contiguous, 16-byte aligned tensor of that shape and dtype on the batch's device to fill (default: a new one, allocated on
        `stream`).  Every argument is checked before the library is called (ValueError); a refused export enqueues nothing."""
        import torch
        if fmt not in ("i420", "argb", "rgb"):
            raise ValueError(f"fmt must be 'i420', 'argb' or 'rgb', not {fmt!r}")
        if layout not in ("nchw", "nhwc"):
            raise ValueError(f"layout must be 'nchw' or 'nhwc', not {layout!r}")
        if dtype is None:
            dtype = torch.uint8
        dcode = DEVICE_EXPORT_DTYPES[dtype_name(dtype, DEVICE_EXPORT_DTYPES, f"dtype must be torch.uint8, torch.float16 or torch.float32, not {dtype!r}")]
        if fmt != "rgb" and dtype != torch.uint8:
            raise ValueError(f"fmt={fmt!r} has bytes only: dtype must be torch.uint8")
        sb = scale_bias(scale, bias, fmt == "rgb" and dtype != torch.uint8, "scale and bias apply to fmt='rgb' with a float dtype only")
        _check_frames(ring_idx, n_frames)
        clips = self._clip_range(clips)
        F, N, W, H = int(n_frames), len(clips), self.Width, self.Height
        box_rows = crop_size = None
        if boxes is not None or flip is not None:
            box_rows, W, H = self._box_geometry(fmt, N, crop, size, boxes, flip)
        elif crop is not None or size is not None:
            crop_size = self._crop_geometry(fmt, crop, size)
            W, H = crop_size[4:]
        if fmt == "i420":
            shape, tdtype = (F, N, W * H * 3 // 2), torch.uint8
        elif fmt == "argb":
            shape, tdtype = (F, N, H, W), torch.int32
        else:
            shape, tdtype = ((F, N, 3, H, W) if layout == "nchw" else (F, N, H, W, 3)), dtype
        dev = torch.device("cuda", self.device)
        check_stream(stream, dev)
        check_out(out, dev, tdtype, shape)
        stream, out = stream_and_out(stream, out, dev, tdtype, shape)
        code = DEVICE_EXPORT_FORMATS[(fmt, layout if fmt == "rgb" else None)]
        frames_dst = (int(ring_idx), F, clips.start, N, out.data_ptr(), tensor_bytes(out), stream.cuda_stream)
        if box_rows is not None:
            rc = self._lib.mobi_batch_export_device_boxes(self._h, code, dcode, sb, box_rows.ctypes.data_as(C.POINTER(C.c_int32)), W, H, *frames_dst)
        elif crop_size is not None:
            rc = self._lib.mobi_batch_export_device_scaled(self._h, code, dcode, sb, *crop_size, *frames_dst)
        else:
            rc = self._lib.mobi_batch_export_device(self._h, code, dcode, sb, *frames_dst)
        check_rc(rc)
        return out

    def set_motion(self, on):
        """Keep the motion field and macroblock data of every frame decoded from now on (mobi_batch_set_motion): a motion ring of six slots
        per clip beside the picture ring, written by one more kernel per frame step; set_motion(False) frees it.  Only with nothing in
        flight (no submitted step, no group, no export that may still run).  A batch that never calls this pays nothing."""
        check_rc(self._lib.mobi_batch_set_motion(self._h, 1 if on else 0))

    def motion_launches(self):
        """launches of the motion kernel so far (0 for a batch that never switched motion on)"""
        return int(self._lib.mobi_batch_motion_launches(self._h))

    def motion_bytes(self):
        """device memory the motion ring holds (0: motion is off)"""
        return int(self._lib.mobi_batch_motion_bytes(self._h))

    def export_motion(self, fmt="cells", ring_idx=0, n_frames=1, clips=None, block=None, dtype=None, scale=1.0, out=None, stream=None):
        """The motion the stream carries, of many clips and frames, into a torch tensor [n_frames, n_clips, C, h, w] on the batch's GPU
        (mobi_batch_export_motion; set_motion(True) first), enqueued on `stream` without a host wait, as export_tensor's pictures are.
        Frame j = ring index ring_idx - j (oldest first), clips = a range / slice of step 1 (None: all).

        fmt="cells": int16, C = 3: dx, dy (half samples, from the block to its source) and ref (0 = intra, 1..5 = frames back) of every
                     2x2 cell; h, w = H/2, W/2.
        fmt="mb":    int32, C = 5: type (0 inter, 1 intra), quantiser field, cbp6, coded levels, sum of their magnitudes; h, w = H/16, W/16.
        fmt="flow":  torch.float32 (default) or torch.float16, C = 2: x, y; block = 2, 4, 8 or 16 (default 16), h, w = H/block, W/block:
                     the mean over the block's cells of the displacement per frame back, in pixels, times `scale`, exact up to one
                     rounding (include/mobiclip_hip.h has the arithmetic).
        The vectors are canonical: -2 * Stride <= dx < 2 * Stride (mobiclip_hip.h).  out: a contiguous, 16-byte aligned tensor of that
        shape and dtype on the batch's device.  Every argument is checked before the library is called (ValueError)."""
        import torch
        if fmt not in MOTION_FORMATS:
            raise ValueError(f"fmt must be one of {sorted(MOTION_FORMATS)}, not {fmt!r}")
        code, channels, fixed_block, dnames = MOTION_FORMATS[fmt]
        if block is None:
            block = fixed_block or 16
        if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or (block != fixed_block if fixed_block else block not in (2, 4, 8, 16)):
            raise ValueError(f"fmt={fmt!r}: block must be {fixed_block if fixed_block else '2, 4, 8 or 16'}, not {block!r}")
        block = int(block)
        if dtype is None:
            dtype = getattr(torch, dnames[0])
        dname = dtype_name(dtype, dnames, f"fmt={fmt!r}: dtype must be {' or '.join('torch.' + d for d in dnames)}, not {dtype!r}")
        try:
            scale = float(scale)
        except (TypeError, ValueError):
            raise ValueError(f"scale must be a float, not {scale!r}") from None
        if not np.isfinite(np.float32(scale)):
            raise ValueError(f"scale must be finite in float32, not {scale!r}")
        if fmt != "flow" and scale != 1.0:
            raise ValueError("scale applies to fmt='flow' only")
        _check_frames(ring_idx, n_frames)
        clips = self._clip_range(clips)
        F, N = int(n_frames), len(clips)
        shape = (F, N, channels, self.Height // block, self.Width // block)
        dev = torch.device("cuda", self.device)
        check_stream(stream, dev)
        check_out(out, dev, dtype, shape)
        stream, out = stream_and_out(stream, out, dev, dtype, shape)
        check_rc(self._lib.mobi_batch_export_motion(self._h, code, MOTION_DTYPES[dname], block, scale, int(ring_idx), F, clips.start, N,
                                                    out.data_ptr(), tensor_bytes(out), stream.cuda_stream))
        return out

    # -- the clip sink: frame steps write chosen frames into one (N, T, ...) tensor (mobiclip_hip.h, mobi_batch_set_sink) ----------
    def set_sink(self, size=None, n_frames=None, stride=1, start=None, boxes=None, flip=None, layout="ntchw", dtype=None, scale=None, bias=None,
                 out=None):
        """Arm a clip sink and return its tensor: from the next frame step on -- decode, submit / wait, every frame of a group, replay -- clip
        c's picture t is written at step start[c] + t * stride (t = 0 .. n_frames - 1; steps count from 0 at arming) straight into the tensor,
        by one more kernel behind the step's reconstruction on the batch's stream.  When the call that reports a frame returns, the frame's
        pictures are there; sink_pending() == 0 says all of them are, and the sink has disarmed itself.

        size=(out_h, out_w), boxes=(n, 4) ints (x, y, w, h; None: the whole picture), flip=n bools or None: export_tensor's, a box per clip,
        with the same values (the definition is include/mobiclip_hip.h's).  start: n ints >= 0 (None: all 0).
        layout: "ntchw" (N, T, 3, H, W), "ncthw" (N, 3, T, H, W), "nthwc" (N, T, H, W, 3), "tnchw" (T, N, 3, H, W), "tnhwc" (T, N, H, W, 3).
        dtype, scale, bias: export_tensor's.  out: a tensor of the layout's shape and the dtype on the batch's device whose innermost H, W
        (H, W, 3) are contiguous; the other strides are taken as they are (multiples of 4 elements, no overlap), so a view into a larger buffer
        works; default: a new contiguous tensor.  The batch keeps a reference to the tensor while the sink is armed.
        set_sink(None) disarms.  Arming, replacing and disarming need nothing in flight (no submitted step, no group)."""
        if size is None and n_frames is None and out is None:
            check_rc(self._lib.mobi_batch_set_sink(self._h, None))
            self._sink_out = None
            return None
        import torch
        if layout not in SINK_LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(SINK_LAYOUTS)}, not {layout!r}")
        planar, dims = SINK_LAYOUTS[layout]
        if dtype is None:
            dtype = torch.uint8
        dname = dtype_name(dtype, DEVICE_EXPORT_DTYPES, f"dtype must be torch.uint8, torch.float16 or torch.float32, not {dtype!r}")
        sb = scale_bias(scale, bias, dtype != torch.uint8, "scale and bias apply to a float dtype only")
        N = self.n
        (T,) = _ints("n_frames", (n_frames,), 1)
        (s,) = _ints("stride", (stride,), 1)
        if T < 1 or s < 1:
            raise ValueError(f"n_frames and stride must be at least 1, not {T} and {s}")
        if boxes is None:
            if flip is not None:
                raise ValueError("flip applies to boxes only")
            boxes = np.tile(np.array([0, 0, self.Width, self.Height], np.int64), (N, 1))
        box_rows, ow, oh = self._box_geometry("rgb", N, None, size, boxes, flip)
        if start is None:
            st = np.zeros(N, np.int64)
        else:
            try:
                st = np.asarray(start)
            except (TypeError, ValueError):
                raise ValueError(f"start must be {N} non-negative ints") from None
            if st.dtype == np.bool_ or not np.issubdtype(st.dtype, np.integer) or st.shape != (N,):
                raise ValueError(f"start must be {N} non-negative ints, not {st.dtype} {st.shape}")
            st = st.astype(np.int64)
        if (st < 0).any() or int(st.max()) + (T - 1) * s > 2**31 - 1:
            raise ValueError(f"start must be non-negative, and start + (n_frames - 1) * stride at most 2**31 - 1")
        st = np.ascontiguousarray(st, dtype=np.int32)
        extent = {"n": N, "t": T, "c": 3, "h": oh, "w": ow}
        shape = tuple(extent[d] for d in dims)
        dev = torch.device("cuda", self.device)
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != shape:
                raise ValueError(f"out must be a {dtype} tensor of shape {shape} (layout {layout!r})")
            sd = dict(zip(dims, out.stride()))
            inner = (sd["h"], sd["w"]) == (ow, 1) if planar else (sd["h"], sd["w"], sd["c"]) == (3 * ow, 3, 1)
            if not inner:
                raise ValueError(f"out: the innermost {'H, W' if planar else 'H, W, 3'} of layout {layout!r} must be contiguous, strides are {tuple(out.stride())}")
            if out.device != dev or out.data_ptr() % 16:
                raise ValueError(f"out must be a 16-byte aligned tensor on {dev}")
        _check_one_hip_runtime()
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=dev)
        sd = dict(zip(dims, out.stride()))
        # the bytes from out's first element to the end of the memory it may address: its storage's, which a view does not own alone
        avail = out.untyped_storage().nbytes() - out.storage_offset() * out.element_size()
        spec = SinkSpec(DEVICE_EXPORT_FORMATS[("rgb", "nchw" if planar else "nhwc")], DEVICE_EXPORT_DTYPES[dname], sb,
                        box_rows.ctypes.data_as(C.POINTER(C.c_int32)), ow, oh, T, s, st.ctypes.data_as(C.POINTER(C.c_int32)), sd["n"], sd["t"],
                        sd["c"] if planar else 0, out.data_ptr(), avail)
        torch.cuda.current_stream(dev).synchronize()  # (whatever was filling `out` is done before the batch's stream writes it)
        check_rc(self._lib.mobi_batch_set_sink(self._h, C.byref(spec)))
        self._sink_out = out
        return out

    def sink_pending(self):
        """(clip, t) pictures the armed sink has not written yet; 0: no sink armed, or complete"""
        return int(self._lib.mobi_batch_sink_pending(self._h))

    def sink_launches(self):
        """launches of the sink kernel so far (0 for a batch that never armed one)"""
        return int(self._lib.mobi_batch_sink_launches(self._h))

    def gop_finish_all(self):
        """gop_finish() for every frame of the oldest group that is still pending, in one call with one wait: -> (rc, offsets) as gop_finish(),
        gop_frames_pending() rows each.  The ring holds the group's last six frames afterwards; the earlier ones reach the caller through a
        sink (set_sink)."""
        return self._gop_finish(self._lib.mobi_batch_gop_finish_all, self._lib.mobi_batch_gop_frames_pending(self._h))

    def _box_geometry(self, fmt, N, crop, size, boxes, flip):
        """export_tensor's boxes / flip / size, checked -> the (N, 5) int32 rows (x, y, w, h, flip) of the library call, out_w, out_h"""
        W, H = self.Width, self.Height
        if boxes is None:
            raise ValueError("flip applies to boxes only")
        if crop is not None:
            raise ValueError("boxes and crop exclude each other")
        if fmt != "rgb":
            raise ValueError(f"boxes apply to fmt='rgb' only, not {fmt!r}")
        if size is None:
            raise ValueError("boxes need a size (out_h, out_w)")
        oh, ow = _ints("size", size, 2)
        if oh < 1 or ow < 1 or ow % 4:
            raise ValueError(f"size (out_h, out_w) = {(oh, ow)!r} must be at least 1x1, out_w a multiple of 4")
        try:
            bx = np.asarray(boxes)
        except (TypeError, ValueError):
            raise ValueError(f"boxes must be an integer array of shape ({N}, 4)") from None
        if bx.dtype == np.bool_ or not np.issubdtype(bx.dtype, np.integer) or bx.shape != (N, 4):
            raise ValueError(f"boxes must be an integer array of shape ({N}, 4), not {bx.dtype} {bx.shape}")
        bx = bx.astype(np.int64)
        if flip is None:
            fl = np.zeros(N, np.int64)
        else:
            try:
                fl = np.asarray(flip)
            except (TypeError, ValueError):
                raise ValueError(f"flip must be {N} bools") from None
            if fl.dtype != np.bool_ or fl.shape != (N,):
                raise ValueError(f"flip must be {N} bools, not {fl.dtype} {fl.shape}")
            fl = fl.astype(np.int64)
        x, y, w, h = bx.T
        bad = (w < 1) | (h < 1) | (x < 0) | (y < 0) | (x + w > W) | (y + h > H)
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError(f"boxes[{i}] (x, y, w, h) = {bx[i].tolist()} is empty or not inside the {W}x{H} picture")
        D = np.where(ow > w, 2 * ow, w) * np.where(oh > h, 2 * oh, h)
        if (D > 1 << 23).any():
            i = int(np.argmax(D > 1 << 23))
            raise ValueError(f"boxes[{i}] = {bx[i].tolist()} to {ow}x{oh}: dx * dy = {int(D[i])}, at most 2**23")
        return np.ascontiguousarray(np.concatenate([bx, fl[:, None]], axis=1), dtype=np.int32), ow, oh

    def _crop_geometry(self, fmt, crop, size):
        """export_tensor's crop / size, checked -> (crop_x, crop_y, crop_w, crop_h, out_w, out_h)"""
        W, H = self.Width, self.Height
        if fmt != "rgb":
            raise ValueError(f"crop and size apply to fmt='rgb' only, not {fmt!r}")
        cx, cy, cw, ch = (0, 0, W, H) if crop is None else _ints("crop", crop, 4)
        if cw < 1 or ch < 1 or cx < 0 or cy < 0 or cx + cw > W or cy + ch > H:
            raise ValueError(f"crop (x, y, w, h) = {crop!r} is empty or not inside the {W}x{H} picture")
        oh, ow = (ch, cw) if size is None else _ints("size", size, 2)
        if not (1 <= ow <= cw and 1 <= oh <= ch) or ow % 4:
            raise ValueError(f"size (out_h, out_w) = {(oh, ow)!r} must be at least 1x1, no larger than the crop ({ch}, {cw}), out_w a multiple of 4")
        if cw * ch > 1 << 23:
            raise ValueError(f"crop of {cw}x{ch} pixels: at most 2**23")
        return cx, cy, cw, ch, ow, oh

    def quantizer(self, clip):
        return self._lib.mobi_batch_quantizer(self._h, clip)

    def yuv_format(self, clip):
        return self._lib.mobi_batch_yuv_format(self._h, clip)

    def motion_search(self, pictures):
        """Analyzer.InterPredict2x2 for every 2x2 luma block (Analyzer.cs:608-693) of `pictures` (one (Height, Width) uint8 luma
        picture per clip) against this batch's ring.  -> dict of (n, mbh, mbw, 8, 8) arrays: dx, dy (half pels), frame, score."""
        pics = [np.ascontiguousarray(p, dtype=np.uint8) for p in pictures]
        assert len(pics) == self.n and all(p.shape == (self.Height, self.Width) for p in pics)
        ptrs = (C.c_void_p * self.n)(*[p.ctypes.data for p in pics])
        out = np.empty((self.n, self.Height // 16, self.Width // 16, 8, 8), np.uint32)
        check_rc(self._lib.mobi_batch_motion_search(self._h, ptrs, out.ctypes.data))
        return unpack_motion_search(out)

    def last_decode_ms(self):
        """Wall time the last decode() spent inside the library."""
        return float(self._lib.mobi_batch_last_decode_ms(self._h))

    # -- replay ---------------------------------------------------------------------------------
    def preload(self, clip, data, frame_off):
        buf = as_u8(data)
        fo = np.ascontiguousarray(frame_off, dtype=np.uint32)
        n_frames = fo.size - 1
        rcs = (C.c_int * n_frames)()
        rc = self._lib.mobi_batch_preload(self._h, clip, buf.ctypes.data, buf.size, fo.ctypes.data, n_frames, rcs)
        if rc == MOBI_E_ARG:  # bad clip index / frame offsets: nothing was staged (a stream error comes back per frame instead)
            check_rc(rc)
        return list(rcs)

    def preload_clone(self, clip, src):
        check_rc(self._lib.mobi_batch_preload_clone(self._h, clip, src))

    def commit(self):
        check_rc(self._lib.mobi_batch_commit(self._h))

    def replay(self, frame_idx):
        check_rc(self._lib.mobi_batch_replay(self._h, frame_idx))

    def sync(self):
        return self._lib.mobi_batch_sync(self._h)

    def cmd_bytes(self, frame_idx):
        return int(self._lib.mobi_batch_cmd_bytes(self._h, frame_idx))

    def intra_stats(self, frame_idx):
        """(intra macroblocks, command-list bytes that belong to them) of one frame step, all clips."""
        n, by = C.c_uint64(), C.c_uint64()
        check_rc(self._lib.mobi_batch_intra_stats(self._h, frame_idx, C.byref(n), C.byref(by)))
        return int(n.value), int(by.value)

    def time_begin(self):
        self._lib.mobi_batch_time_begin(self._h)

    def time_end(self):
        ms = C.c_float()
        check_rc(self._lib.mobi_batch_time_end(self._h, C.byref(ms)))
        return ms.value

    def set_kernel_timing(self, level):
        """0 / False: off; 1 / True: HIP events around the inter launches; 2: around every launch."""
        self._lib.mobi_batch_set_kernel_timing(self._h, int(level))

    def kernel_ms(self):
        a, b, na, nb = C.c_float(), C.c_float(), C.c_int(), C.c_int()
        self._lib.mobi_batch_kernel_ms(self._h, C.byref(a), C.byref(b), C.byref(na), C.byref(nb))
        return {"inter_ms": a.value, "intra_ms": b.value, "inter_launches": na.value, "intra_launches": nb.value}


def forward_dct(blocks, device=None):
    """MobiEncoder.DCT64 / DCT16 (Encoder/MobiEncoder.cs:962, 1146) on the GPU: blocks = int32 array (n_blocks, 64) or (n_blocks, 16)
    of residuals -> coefficients of the same shape, as the reference returns them."""
    a = np.ascontiguousarray(blocks, dtype=np.int32)
    if a.ndim != 2 or a.shape[1] not in (64, 16):
        raise ValueError("blocks must be (n, 64) or (n, 16)")
    out = np.empty_like(a)
    check_rc(load_library().mobi_forward_dct(default_device() if device is None else device, 8 if a.shape[1] == 64 else 4, a.ctypes.data, out.ctypes.data, a.shape[0]))
    return out


def quant_tables(q):
    """MobiEncoder.SetupQuantizationTables (Encoder/MobiEncoder.cs:930-960) for quantiser q in [0, 53]: (QTable4x4 float32[16],
    QTable8x8 float32[64]) in natural DCT order, as the reference's float[] holds them.  Needs no device."""
    q4, q8 = np.empty(16, np.float32), np.empty(64, np.float32)
    check_rc(load_library().mobi_encoder_qtables(int(q), q4.ctypes.data, q8.ctypes.data))
    return q4, q8


_ONE_RUNTIME = False


def _check_one_hip_runtime():
    """torch's pointers and streams mean something to this library only if both use the same HIP runtime.  A torch wheel that bundles its own
    libamdhip64 shares it with this library when torch is imported first; loaded the other way round the process holds two runtimes."""
    global _ONE_RUNTIME
    if _ONE_RUNTIME:
        return
    try:
        maps = open("/proc/self/maps").read().split("\n")
    except OSError:
        return
    paths = {ln.split()[-1] for ln in maps if "libamdhip64.so" in ln}
    if len({os.path.realpath(x) for x in paths}) > 1:
        raise MobiclipError("two HIP runtimes in this process (torch's and the one libmobiclip_hip.so was loaded with): import torch before "
                            "the first use of mobiclipdecoder_amd to pass torch tensors")
    _ONE_RUNTIME = True


def transform_code(src, pred, quantizers, levels=True, recon=True, sad=True, device=None):
    """MacroBlock.EncodeDecode8x8Block / EncodeDecode4x4Block (Encoder/MacroBlock.cs:577-626) and the analyzer's SAD on the GPU
    (include/mobiclip_hip.h, mobi_transform_code): every block of src against the same block of pred at every quantiser.

    src, pred: uint8 (n_blocks, 64) or (n_blocks, 16), row-major pixels.  quantizers: an int or a sequence of 1..54 ints in [0, 53].
    Returns a dict of arrays shaped (n_q, n_blocks, ...): "bits" int32, "flags" uint8 (MOBI_TC_CODED 1, MOBI_TC_CLAMP 2), and unless
    switched off "levels" int16 (.., n*n, scan order), "recon" uint8 (.., n*n), "sad" int32.  numpy inputs go through the host entry
    point; torch tensors on the GPU through the asynchronous one, on torch.cuda.current_stream(), and come back as torch tensors (torch
    must have been imported before this library was loaded, so that both use one HIP runtime)."""
    qs = [int(quantizers)] if np.isscalar(quantizers) else [int(q) for q in quantizers]
    if not 1 <= len(qs) <= 54:
        raise ValueError("1 to 54 quantizers")
    is_torch = type(src).__module__.startswith("torch")
    if is_torch:
        import torch
        _check_one_hip_runtime()
        if not (isinstance(pred, torch.Tensor) and src.is_cuda and pred.is_cuda and src.device == pred.device):
            raise ValueError("src and pred must both be torch tensors on the same GPU")
        if src.dtype != torch.uint8 or pred.dtype != torch.uint8:
            raise ValueError("src and pred must be uint8")
    else:
        src, pred = np.asarray(src), np.asarray(pred)
        if src.dtype != np.uint8 or pred.dtype != np.uint8:
            raise ValueError("src and pred must be uint8")
    if src.ndim != 2 or src.shape[1] not in (64, 16) or tuple(pred.shape) != tuple(src.shape):
        raise ValueError("src and pred must be (n_blocks, 64) or (n_blocks, 16), of one shape")
    nb, nn = int(src.shape[0]), int(src.shape[1])
    n, nq = (8 if nn == 64 else 4), len(qs)
    qarr = (C.c_int * nq)(*qs)
    lib = load_library()
    if is_torch:
        src, pred = src.contiguous(), pred.contiguous()
        dev = src.device
        out = {"bits": torch.empty((nq, nb), dtype=torch.int32, device=dev), "flags": torch.empty((nq, nb), dtype=torch.uint8, device=dev)}
        if levels:
            out["levels"] = torch.empty((nq, nb, nn), dtype=torch.int16, device=dev)
        if recon:
            out["recon"] = torch.empty((nq, nb, nn), dtype=torch.uint8, device=dev)
        if sad:
            out["sad"] = torch.empty((nq, nb), dtype=torch.int32, device=dev)
        ptr = {k: v.data_ptr() for k, v in out.items()}
        rc = lib.mobi_transform_code_async(dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream,
                                           n, qarr, nq, src.data_ptr(), pred.data_ptr(), nb, ptr.get("levels"), ptr.get("recon"), ptr["bits"],
                                           ptr.get("sad"), ptr["flags"])
    else:
        src, pred = np.ascontiguousarray(src), np.ascontiguousarray(pred)
        out = {"bits": np.empty((nq, nb), np.int32), "flags": np.empty((nq, nb), np.uint8)}
        if levels:
            out["levels"] = np.empty((nq, nb, nn), np.int16)
        if recon:
            out["recon"] = np.empty((nq, nb, nn), np.uint8)
        if sad:
            out["sad"] = np.empty((nq, nb), np.int32)
        ptr = {k: v.ctypes.data for k, v in out.items()}
        rc = lib.mobi_transform_code(default_device() if device is None else device, n, qarr, nq, src.ctypes.data, pred.ctypes.data, nb,
                                     ptr.get("levels"), ptr.get("recon"), ptr["bits"], ptr.get("sad"), ptr["flags"])
    check_rc(rc)
    return out
