"""The intra encoder (include/mobiclip_encode.h): a batch of I420 pictures to Mobiclip I-frames, one stream per picture, on the GPU.
Every stream decodes -- in the reference decoder and in MobiclipBatch -- to exactly the reconstruction the encoder reports; decisions and
bits are only ever produced by the HIP kernels (mobi_encode.hip).  DESIGN.md, "Intra encoder", has the rules."""
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


class MobiclipIntraEncoder(Handle):
    """mobi_enc: I-frames of width x height pictures for MobiclipVersion.Moflex3DS or .ModsDS, up to max_pictures per call."""
    _destroy = "mobi_enc_destroy"

    def __init__(self, width, height, version, max_pictures, device=None):
        self._h = None
        self._lib = _lib()
        self.width, self.height, self.version, self.max_pictures = int(width), int(height), int(version), int(max_pictures)
        self.device = default_device() if device is None else int(device)
        self.frame_bytes = self.width * self.height * 3 // 2
        q = np.full(1, 12, np.uint8)
        check_rc(self._lib.mobi_enc_check(self.max_pictures, self.width, self.height, self.version, 1, (self.frame_bytes + 7) & ~7, q.ctypes.data, 0, 0))
        self._h = self._lib.mobi_enc_create(self.max_pictures, self.width, self.height, self.version, self.device)
        if not self._h:
            raise MobiclipError("mobi_enc_create failed: no usable HIP device, or out of device memory")
        self.stream_bound = stream_bound(self.width, self.height)

    def encode(self, pictures, quantizer, yuv_format=0, recon=False, stats=False, slot_bytes=None, stream=None):
        """pictures: (N, width * height * 3 / 2) uint8, packed I420 as export_tensor("i420") writes it -- a torch tensor on the encoder's
        device (encoded where it lies, on `stream` or torch's current one) or a numpy array (the synchronous host entry point).
        quantizer: an int in [12, 52] or one per picture.  slot_bytes: the room of one stream (a multiple of 4; default: the bound).

        Returns a list of N bytes objects.  For a torch input with slot_bytes given: (streams, sizes) -- an (N, slot_bytes) uint8 and an
        (N,) int32 tensor, enqueued and not waited for; a stream longer than slot_bytes leaves its slot zero and its true size in sizes.
        With recon and / or stats a dict follows as the last element: "recon" (N, frame) uint8, "stats" (N,) STATS_DTYPE (for the
        unsynchronised torch form an (N, 64) uint8 tensor: .cpu().numpy().view(STATS_DTYPE))."""
        if not self._h:
            raise MobiclipError("encoder is closed")
        is_torch = type(pictures).__module__.startswith("torch")
        if not is_torch:
            pictures = np.ascontiguousarray(pictures)
            if pictures.dtype != np.uint8:
                raise ValueError("pictures must be uint8")
        if pictures.ndim != 2 or int(pictures.shape[1]) != self.frame_bytes:
            raise ValueError(f"pictures must be (N, {self.frame_bytes})")
        n = int(pictures.shape[0])
        qs = np.full(n, int(quantizer), np.int64) if np.isscalar(quantizer) else np.asarray([int(q) for q in quantizer], np.int64)
        if qs.shape != (n,) or n < 1 or qs.min() < 0 or qs.max() > 255:
            raise ValueError("one quantizer, or one per picture")
        qs = qs.astype(np.uint8)
        slot = self.stream_bound if slot_bytes is None else int(slot_bytes)
        extras = {}
        if is_torch:
            import torch
            _check_one_hip_runtime()
            if pictures.dtype != torch.uint8 or not pictures.is_cuda or (pictures.device.index or 0) != self.device:
                raise ValueError("pictures must be a uint8 tensor on the encoder's device")
            pictures = pictures.contiguous()
            dev = pictures.device
            check_rc(self._lib.mobi_enc_check(self.max_pictures, self.width, self.height, self.version, n, self.frame_bytes, qs.ctypes.data, int(yuv_format), slot))
            s = torch.cuda.current_stream(dev) if stream is None else stream
            with torch.cuda.stream(s):  # torch's allocator then knows which stream uses the outputs
                out = torch.empty((n, slot), dtype=torch.uint8, device=dev)
                sizes = torch.empty((n,), dtype=torch.int32, device=dev)
                if recon:
                    extras["recon"] = torch.empty((n, self.frame_bytes), dtype=torch.uint8, device=dev)
                if stats:
                    extras["stats"] = torch.empty((n, STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            check_rc(self._lib.mobi_enc_intra_async(self._h, s.cuda_stream, n, pictures.data_ptr(), self.frame_bytes, qs.ctypes.data, int(yuv_format),
                                                    out.data_ptr(), slot, sizes.data_ptr(), extras["recon"].data_ptr() if recon else None,
                                                    extras["stats"].data_ptr() if stats else None))
            if slot_bytes is not None:
                return (out, sizes, extras) if extras else (out, sizes)
            s.synchronize()
            out, sizes = out.cpu().numpy(), sizes.cpu().numpy()
            if recon:
                extras["recon"] = extras["recon"].cpu().numpy()
            if stats:
                extras["stats"] = extras["stats"].cpu().numpy().view(STATS_DTYPE).reshape(n)
        else:
            out = np.zeros((n, slot), np.uint8)
            sizes = np.zeros(n, np.int32)
            if recon:
                extras["recon"] = np.zeros((n, self.frame_bytes), np.uint8)
            if stats:
                extras["stats"] = np.zeros(n, STATS_DTYPE)
            pitch = self.frame_bytes  # a multiple of 8: width and height are multiples of 16
            check_rc(self._lib.mobi_enc_intra(self._h, n, pictures.ctypes.data, pitch, qs.ctypes.data, int(yuv_format), out.ctypes.data, slot,
                                              sizes.ctypes.data, extras["recon"].ctypes.data if recon else None, extras["stats"].ctypes.data if stats else None))
        streams = [out[i, :sizes[i]].tobytes() if sizes[i] <= slot else b"" for i in range(n)]
        if slot_bytes is not None:
            extras["sizes"] = sizes
            extras["slots"] = out
        return (streams, extras) if extras else streams
