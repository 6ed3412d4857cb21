"""Rate control of both encoders (include/mobiclip_encode_rate.h): a byte target per picture in place of a quantiser.  The quantiser is
found on the GPU, by a bisection over real trial encodes (csrc/mobi_encode_rate.h, mobi_encode_rate.hip around the encoders' own kernels);
nothing is waited for and the host reads no device value, so calls chain: the chosen quantisers of one call are the previous quantisers of
the next as a device tensor.  DESIGN.md, "Rate control", has the rule.  This module is the one body of
MobiclipIntraEncoder.encode_target and MobiclipInterEncoder.encode_target."""
import ctypes as C

import numpy as np

from .binding import bind
from .decoder import MobiclipError, _check_one_hip_runtime, check_rc, check_stream, load_library

_P = C.c_void_p
# names must match include/mobiclip_encode_rate.h (tests/test_encode_rate_model.py checks header, library and this table)
_SIGS = {
    "mobi_enc_rate_rounds": (C.c_int, [C.c_int, C.c_int]),
    "mobi_enc_intra_target_async": (C.c_int, [C.c_void_p, _P, C.c_int, _P, C.c_size_t, _P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, _P, _P, _P]),
    "mobi_enc_inter_target_async": (C.c_int, [C.c_void_p, _P, C.c_int, _P, C.c_size_t, _P, C.c_size_t, _P, _P, C.c_int, C.c_int, _P, C.c_size_t, _P, _P, _P, _P]),
}


def _lib():
    return bind(load_library(), _SIGS)


def rate_rounds(qmin, qmax):
    """mobi_enc_rate_rounds: the trial encodes per picture of a call with this range (0 .. 6); -1 for a range the calls refuse"""
    return int(_lib().mobi_enc_rate_rounds(int(qmin), int(qmax)))


def _row(value, n, dev, dtype, what):
    """one value per picture as an (n,) tensor of dtype on dev: an int, a sequence of n, or such a tensor (taken as it is)"""
    import torch
    if isinstance(value, torch.Tensor):
        if value.dtype != dtype or value.device != dev or tuple(value.shape) != (n,):
            raise ValueError(f"{what} as a tensor must be ({n},) {dtype} on {dev}")
        return value.contiguous()
    vals = [int(value)] * n if np.isscalar(value) else [int(v) for v in value]
    info = torch.iinfo(dtype)
    if len(vals) != n or min(vals) < info.min or max(vals) > info.max:
        raise ValueError(f"one {what}, or one per picture")
    return torch.tensor(vals, dtype=dtype, device=dev)


def encode_target(enc, call, inputs, prev_quantizer, target_bytes, qmin, qmax, extra, recon, stats, slot_bytes, stream):
    """enc: an encode._Encoder; call: its _target_async entry; inputs: its picture tensors; prev_quantizer: None for I-frames; extra: the C
    arguments between the range and the slots -> what _Encoder._encode returns for tensors, the dict always there and with "quantizer" in it"""
    import torch
    if not enc._h:
        raise MobiclipError("encoder is closed")
    what = " and ".join(enc._what)
    F = enc.frame_bytes
    for t in inputs:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or (t.device.index or 0) != enc.device:
            raise ValueError(f"{what} must be {'a uint8 tensor' if len(inputs) == 1 else 'uint8 tensors'} on the encoder's device")
    if inputs[0].ndim != 2 or int(inputs[0].shape[1]) != F or any(tuple(a.shape) != tuple(inputs[0].shape) for a in inputs[1:]):
        raise ValueError(f"{what} must be (N, {F})")
    n, dev = int(inputs[0].shape[0]), inputs[0].device
    check_stream(stream, dev)
    _check_one_hip_runtime()
    lib = bind(enc._lib, _SIGS)
    slot = enc.stream_bound if slot_bytes is None else int(slot_bytes)
    s = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(s):  # torch's allocator then knows which stream uses the rows and the outputs
        inputs = [t.contiguous() for t in inputs]
        rows = ([_row(prev_quantizer, n, dev, torch.uint8, "prev_quantizer")] if prev_quantizer is not None else []) + [_row(target_bytes, n, dev, torch.int32, "target_bytes")]
        out = torch.empty((n, slot), dtype=torch.uint8, device=dev)
        sizes = torch.empty((n,), dtype=torch.int32, device=dev)
        extras = {"quantizer": torch.empty((n,), dtype=torch.uint8, device=dev)}
        if recon:
            extras["recon"] = torch.empty((n, F), dtype=torch.uint8, device=dev)
        if stats:
            extras["stats"] = torch.empty((n, enc._stats.itemsize), dtype=torch.uint8, device=dev)
    check_rc(getattr(lib, call)(enc._h, s.cuda_stream, n, *[x for a in inputs for x in (a.data_ptr(), F)], *[r.data_ptr() for r in rows], int(qmin), int(qmax),
                                *[int(x) for x in extra], out.data_ptr(), slot, sizes.data_ptr(), extras["recon"].data_ptr() if recon else None,
                                extras["stats"].data_ptr() if stats else None, extras["quantizer"].data_ptr()))
    if slot_bytes is not None:
        return out, sizes, extras
    s.synchronize()
    out, sizes = out.cpu().numpy(), sizes.cpu().numpy()
    extras = {k: v.cpu().numpy() for k, v in extras.items()}
    if stats:
        extras["stats"] = extras["stats"].view(enc._stats).reshape(n)
    return [out[i, :sizes[i]].tobytes() if sizes[i] <= slot else b"" for i in range(n)], extras
