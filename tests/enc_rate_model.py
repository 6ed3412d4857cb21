"""What the rate control's tests share (tests/test_encode_rate_model.py on the CPU, tests/test_encode_rate_gpu.py on the GPU):

  host model   tests/tools/mobi_encode_rate_host.cpp: the product's csrc/mobi_encode_rate.h over the three encoders' picture functions
               (built by build.build_encratehost).  kind 0: I-frames, 1: P-frames, 2: P-frames in partition mode 1
  fixed        the EXISTING single-quantiser host models (enc_model, enc_inter_model, enc_parts_model) by kind
  bisect       the rule written out again in Python over `fixed`, one call of it per round: the independent re-derivation
  inputs       per kind and shape, pictures with (for P-frames) the intra model's reconstruction at q = 20 of the frame before as reference
  table        bytes by quantiser of those inputs from `fixed`; calls() takes every target from it
Nothing here includes the product's rate header."""
import ctypes as C

import numpy as np

from tests import enc_inter_model as M
from tests import enc_model as E
from tests import enc_parts_model as Q

P = C.c_void_p
KINDS = (0, 1, 2)
VERSIONS = E.VERSIONS
SHAPES = ((16, 16), (48, 32))
QMIN, QMAX = 12, 52
REF_Q = 20  # the quantiser of the frame before every P-frame of `inputs`
STATS = (E.STATS_DTYPE, M.STATS_DTYPE, M.STATS_DTYPE)
_HOST = None
_CACHE = {}


def host():
    global _HOST
    if _HOST is None:
        from mobiclipdecoder_amd import build
        L = C.CDLL(build.build_encratehost())
        L.encr_host_rounds.argtypes = [C.c_int, C.c_int]
        L.encr_host_bound.restype = C.c_size_t
        L.encr_host_bound.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
        L.encr_host_target.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, P, C.c_size_t, P, C.c_size_t, P, P, C.c_int, C.c_int, C.c_int, P, C.c_size_t,
                                       P, P, P, P, P, C.c_int]
        _HOST = L
    return _HOST


def rounds(qmin, qmax):
    """the closed form: the smallest k with 2^k >= qmax - qmin + 1"""
    return int(qmax - qmin).bit_length()


def host_target(W, H, version, kind, pictures, refs, prev_q, targets, qmin=QMIN, qmax=QMAX, yuv_format=0, slot_bytes=None, threads=1):
    """the host model over a batch -> dict(streams (N, slot), bytes, recon, stats, quantizer (N,), trials (N, 6, 2): (q, bytes) per round, -1 behind them)"""
    L = host()
    pictures = np.ascontiguousarray(pictures, np.uint8)
    n = pictures.shape[0]
    refs = None if kind == 0 else np.ascontiguousarray(refs, np.uint8)
    pq = None if kind == 0 else np.ascontiguousarray(np.broadcast_to(np.asarray(prev_q, np.uint8), (n,)))
    tg = np.ascontiguousarray(np.broadcast_to(np.asarray(targets, np.int32), (n,)))
    slot = L.encr_host_bound(W, H, kind) if slot_bytes is None else slot_bytes
    out = {"streams": np.full((n, slot), 0xAA, np.uint8), "bytes": np.zeros(n, np.int32), "recon": np.zeros((n, W * H * 3 // 2), np.uint8),
           "stats": np.zeros(n, STATS[kind]), "quantizer": np.zeros(n, np.uint8), "trials": np.zeros((n, 6, 2), np.int32)}
    rc = L.encr_host_target(W, H, version, kind, n, pictures.ctypes.data, pictures.shape[1], None if kind == 0 else refs.ctypes.data, 0 if kind == 0 else refs.shape[1],
                            None if kind == 0 else pq.ctypes.data, tg.ctypes.data, qmin, qmax, yuv_format, out["streams"].ctypes.data, slot, out["bytes"].ctypes.data,
                            out["recon"].ctypes.data, out["stats"].ctypes.data, out["quantizer"].ctypes.data, out["trials"].ctypes.data, threads)
    assert rc == 0, rc
    return out


def fixed(W, H, version, kind, pictures, refs, prev_q, q, yuv_format=0):
    """the existing model of the kind at given quantisers (prev_q as the encoder uses it: clamped)"""
    n = pictures.shape[0]
    q = np.broadcast_to(np.asarray(q, np.uint8), (n,))
    if kind == 0:
        return E.host_encode(W, H, version, pictures, q, yuv_format)
    pq = np.clip(np.broadcast_to(np.asarray(prev_q, np.int64), (n,)), QMIN, QMAX).astype(np.uint8)
    if kind == 1:
        return M.host_encode(W, H, version, pictures, refs, pq, q)
    return Q.host_encode(W, H, version, 1, pictures, refs, pq, q)


def bisect(W, H, version, kind, pictures, refs, prev_q, targets, qmin=QMIN, qmax=QMAX, yuv_format=0):
    """the rule in Python over `fixed` -> (fixed's dict at q_out, q_out (N,), trials: list of (mid (N,), bytes (N,)) per round)"""
    n = pictures.shape[0]
    tg = np.broadcast_to(np.asarray(targets, np.int64), (n,))
    lo, hi = np.full(n, qmin, np.int64), np.full(n, qmax, np.int64)
    trials = []
    for _ in range(rounds(qmin, qmax)):
        mid = (lo + hi) >> 1
        b = fixed(W, H, version, kind, pictures, refs, prev_q, mid, yuv_format)["bytes"].astype(np.int64)
        fits = b <= tg
        lo, hi = np.where(fits, lo, np.minimum(mid + 1, hi)), np.where(fits, mid, hi)
        trials.append((mid, b))
    assert np.array_equal(lo, hi)
    return fixed(W, H, version, kind, pictures, refs, prev_q, lo, yuv_format), lo.astype(np.uint8), trials


def inputs(W, H, version, kind):
    """-> (pictures (N, frame), refs (N, frame) or None, prev_q (N,) or None): kind 0 the intra sets' mixed five; kind 1 frame 1 of the
    inter sets' six clips; kind 2 frame 1 of the three two-motion clips and the mixed five"""
    key = ("in", W, H, version, kind)
    if key not in _CACHE:
        if kind == 0:
            _CACHE[key] = (E.picture_sets(W, H)["mixed5"][0], None, None)
        else:
            sets = M.sequence_sets(W, H) if kind == 1 else Q.sequence_sets(W, H)
            frames = np.concatenate([sets[k][0] for k in (("fullpel", "mixed5") if kind == 1 else ("two_motion", "mixed5"))])
            n = frames.shape[0]
            refs = E.host_encode(W, H, version, frames[:, 0], np.full(n, REF_Q, np.uint8))["recon"]
            _CACHE[key] = (np.ascontiguousarray(frames[:, 1]), refs, np.full(n, REF_Q, np.uint8))
    return _CACHE[key]


def table(W, H, version, kind):
    """bytes by quantiser: (53, N) int64, rows 12 .. 52 filled"""
    key = ("tab", W, H, version, kind)
    if key not in _CACHE:
        pics, refs, pq = inputs(W, H, version, kind)
        t = np.zeros((QMAX + 1, pics.shape[0]), np.int64)
        for q in range(QMIN, QMAX + 1):
            t[q] = fixed(W, H, version, kind, pics, refs, pq, q)["bytes"]
        _CACHE[key] = t
    return _CACHE[key]


# what a picture's target is taken from, by class: ends at qmin; ends inside; ends at qmax and fits; fits nothing (0 and 4); exactly the
# first trial's length (fits); one less (does not)
CLASSES = ("qmin", "inside", "qmax_fits", "zero", "four", "trial", "trial_less")


def _target(B, i, cls, qmin, qmax):
    mid = (qmin + qmax) >> 1
    return {"qmin": int(B[qmin:qmax + 1, i].max()), "inside": int(B[mid - 2, i]), "qmax_fits": int(B[qmax, i]), "zero": 0, "four": 4,
            "trial": int(B[mid, i]), "trial_less": int(B[mid, i]) - 1}[cls]


def calls(W, H, version, kind):
    """-> list of (name, prev_q (N,) or None, targets (N,) int32, qmin, qmax): the full range with every picture in every class once
    (seven calls, the classes rotated over the pictures), the range 20 .. 27 (three rounds), a range of one, and for P-frames a call whose
    previous quantisers lie outside [12, 52]"""
    pics, refs, pq = inputs(W, H, version, kind)
    n, B = pics.shape[0], table(W, H, version, kind)
    out = []
    for r in range(len(CLASSES)):
        out.append((f"full{r}", pq, np.array([_target(B, i, CLASSES[(i + r) % len(CLASSES)], QMIN, QMAX) for i in range(n)], np.int32), QMIN, QMAX))
    out.append(("k3", pq, np.array([_target(B, i, CLASSES[(i + 1) % len(CLASSES)], 20, 27) for i in range(n)], np.int32), 20, 27))
    out.append(("one", pq, np.array([_target(B, i, CLASSES[i % len(CLASSES)], 31, 31) for i in range(n)], np.int32), 31, 31))
    if kind:
        wild = np.array([5, 60, 0, 255, 11, 53, 12][:n] + [52] * max(0, n - 7), np.uint8)
        out.append(("clamped", wild, np.array([_target(B, i, "inside", QMIN, QMAX) for i in range(n)], np.int32), QMIN, QMAX))
    return out


def model(W, H, version, kind, name):
    """the host model's output for one of calls(), cached: both test files read it and leave it unchanged"""
    key = ("model", W, H, version, kind, name)
    if key not in _CACHE:
        pics, refs, _ = inputs(W, H, version, kind)
        _, pq, tg, qmin, qmax = next(c for c in calls(W, H, version, kind) if c[0] == name)
        _CACHE[key] = host_target(W, H, version, kind, pics, refs, pq, tg, qmin, qmax)
    return _CACHE[key]


def chain(W, H, version, mode, frames, targets, qmin=QMIN, qmax=QMAX):
    """the host model over clips: frame 0 as an I-frame, the rest as P-frames (partition mode `mode`), each with the frame before's
    reconstruction and chosen quantisers; targets (N, T) -> list of T host_target dicts"""
    out = [host_target(W, H, version, 0, frames[:, 0], None, None, targets[:, 0], qmin, qmax)]
    for t in range(1, frames.shape[1]):
        out.append(host_target(W, H, version, 1 + mode, frames[:, t], out[-1]["recon"], out[-1]["quantizer"], targets[:, t], qmin, qmax))
    return out
