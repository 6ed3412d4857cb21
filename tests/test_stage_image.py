"""The staged bitstream image of a device-parsed hand-over (csrc/mobi_handover.h) against a model of its layout.  CPU only: the header's
planner, header writer, gather and routing are built with g++ (tests/tools/mobi_stage_host.cpp) and run on the smallest shapes at which the
layout can go wrong -- three clips of 2x2 macroblocks, once as a step (K = 1) and once as a group (K = 2) -- into a buffer filled with 0xAA
with guard zones on both sides.

The model below is written from the layout's description, not from the code: [bit_off u64 x lanes][bit_len u32 x lanes], padded to 16; the
bits, every lane that has any 8-aligned with 32 zero bytes (and the alignment's) behind them; zero bytes, 64 at least, up to the reset
list; the idle list; and, for groups with an idle slot, idle_from[n] -- the three of them 16-aligned.  Whatever the layout does not name keeps its 0xAA."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mobiclipdecoder_amd", "csrc")
SKIP = 0xFFFFFFFF
N, N_MBS = 3, 4
BOUND = N_MBS * 4096 + 64  # bytes of a frame beyond which nothing can influence its parse
GUARD = 256


def _frame(size, first=()):
    b = bytearray((i * 37 + 11) & 0xFF for i in range(size))
    return b, first


# a lane: (Data or None, Length, Offset, first bytes of the frame to force).  The lanes between the two cases:
STEP = dict(K=1, group=0, on_host=[0, 1, 0], idle_from=[1, 1, 0], resets=[2, 0], lanes=[
    (8, 8, 3, (0x12, 0x80)),     # 5 bytes, odd: the 8-byte alignment; an I-frame's first bit
    (10, 10, 11, ()),            # the host parser's clip, offset > len: no bytes, and nothing for max_len either
    (None, 0, -5, ()),           # the idle clip: nothing of it is looked at
])
GROUP = dict(K=2, group=1, on_host=[0, 0, 1], idle_from=[2, 1, 2], resets=[1, 2], lanes=[
    (1, 1, 0, (0xFF,)),                          # one byte: no first bit to read (an I-frame needs two)
    (BOUND + 107, BOUND + 107, 7, (0x55, 0x7F)),  # frame_bound + 100 bytes, clamped; a P-frame's first bit
    (4, 4, -1, ()),                              # the host parser's clip, offset < 0: keeps its (empty) place
    (None, 9, 0, ()),                            # Data == null
    (3, 3, 0, ()),                               # idle from frame 1: nothing of it is read
    (6, 6, 6, ()),                               # the host parser's clip, offset == len
])


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("stage_host") / "libmobi_stage_host.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "tools", "mobi_stage_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.mobi_stage_host_build.restype = ctypes.c_int
    lib.mobi_stage_host_build.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6 + [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 3
    return lib


def _align(v, a):
    return (v + a - 1) // a * a


def _model(case, routed):
    """(image bytes, info dict, boff, lens, header bit_len) of the hand-over, from the layout's description"""
    K, group = case["K"], case["group"]
    nv = N * K
    hdr = _align(nv * 12, 16)
    pos, max_len = 0, 0
    boff, lens, bit_len, bits = [], [], [], []
    n_dev = n_iframes = 0
    for v, (size, length, off, first) in enumerate(case["lanes"]):
        c, k = v % N, v // N
        boff.append(pos)
        if k >= case["idle_from"][c]:  # an idle slot: no bytes, skipped
            lens.append(SKIP); bit_len.append(SKIP)
            continue
        frame = b""
        if size is not None and 0 <= off < length:
            data, _ = _frame(size)
            data[off:off + len(first)] = bytes(first)
            frame = bytes(data[off:length][:BOUND])
        max_len = max(max_len, len(frame))
        host = case["on_host"][c]
        if host and not group:  # the step rule: no bytes, skipped at once
            lens.append(SKIP); bit_len.append(SKIP)
            continue
        lens.append(len(frame))  # (the group rule: the host parser's lane keeps bytes and length; the header says so once routed)
        bit_len.append(SKIP if host and routed else len(frame))
        bits.append((pos, frame))
        pos += _align(len(frame) + 32, 8)
        if not host and (routed or not group):
            n_dev += 1
            n_iframes += len(frame) >= 2 and (frame[1] & 0x80) != 0
    idle_clips = [c for c in range(N) if case["idle_from"][c] < K]
    reset_off = _align(hdr + pos + 64, 16)  # zero bytes in front of the lists, 64 at least; the lists are 16-aligned
    idle_off = reset_off + _align(4 * len(case["resets"]), 16)
    idle_from_off = idle_off + _align(4 * len(idle_clips), 16) if group and idle_clips else 0
    total = idle_from_off + _align(N, 16) if idle_from_off else idle_off + _align(4 * len(idle_clips), 16)
    img = bytearray(b"\xAA" * total)
    img[0:nv * 8] = struct.pack("<%dQ" % nv, *boff)
    img[nv * 8:nv * 12] = struct.pack("<%dI" % nv, *bit_len)
    for p, frame in bits:
        span = _align(len(frame) + 32, 8)
        img[hdr + p:hdr + p + span] = frame + bytes(span - len(frame))
    img[hdr + pos:reset_off] = bytes(reset_off - hdr - pos)
    img[reset_off:reset_off + 4 * len(case["resets"])] = struct.pack("<%di" % len(case["resets"]), *case["resets"])
    img[idle_off:idle_off + 4 * len(idle_clips)] = struct.pack("<%di" % len(idle_clips), *idle_clips)
    if idle_from_off:
        img[idle_from_off:idle_from_off + N] = bytes(case["idle_from"])
    if group and not routed:
        n_dev = sum(1 for x in lens if x != SKIP)  # (before the routing is known every live lane counts, and no first bit has been read)
        n_iframes = 0
    info = dict(hdr_bytes=hdr, bytes=total, max_len=max_len, reset_off=reset_off, n_reset=len(case["resets"]), idle_off=idle_off, n_idle=len(idle_clips),
                idle_from_off=idle_from_off, n_dev=n_dev, n_iframes=n_iframes)
    return bytes(img), info, boff, lens, bit_len


def _build(lib, case, route):
    nv = N * case["K"]
    keep, ptrs, lens_in, offs = [], [], [], []
    for size, length, off, first in case["lanes"]:
        if size is None:
            ptrs.append(None)
        else:
            data, _ = _frame(size)
            if first:
                data[off:off + len(first)] = bytes(first)
            a = np.frombuffer(bytes(data), np.uint8).copy()
            keep.append(a)
            ptrs.append(a.ctypes.data)
        lens_in.append(length); offs.append(off)
    data_p = (ctypes.c_void_p * nv)(*ptrs)
    len_p = (ctypes.c_size_t * nv)(*lens_in)
    off_p = np.array(offs, np.int32)
    host, idle, resets = np.array(case["on_host"], np.uint8), np.array(case["idle_from"], np.uint8), np.array(case["resets"], np.int32)
    info, boff, lens = np.zeros(10, np.uint64), np.zeros(nv, np.uint64), np.zeros(nv, np.uint32)
    buf = np.full(GUARD + BOUND + 4096 + GUARD, 0xAA, np.uint8)
    rc = lib.mobi_stage_host_build(N, case["K"], N_MBS, ctypes.addressof(data_p), ctypes.addressof(len_p), off_p.ctypes.data, host.ctypes.data, idle.ctypes.data, resets.ctypes.data,
                                   len(resets), case["group"], route, buf.ctypes.data + GUARD, buf.size - 2 * GUARD, info.ctypes.data, boff.ctypes.data, lens.ctypes.data)
    assert rc == 0
    names = ("hdr_bytes", "bytes", "max_len", "reset_off", "n_reset", "idle_off", "n_idle", "idle_from_off", "n_dev", "n_iframes")
    return buf, dict(zip(names, (int(x) for x in info))), [int(x) for x in boff], [int(x) for x in lens]


# ... and both once more with no clip the host parser's, so that the lanes with offset > len, offset < 0 and offset == len are the GPU's
STEP_DEV, GROUP_DEV = dict(STEP, on_host=[0, 0, 0]), dict(GROUP, on_host=[0, 0, 0])


@pytest.mark.parametrize("name,case,route", [("step", STEP, 0), ("group", GROUP, 0), ("group-routed", GROUP, 1), ("step-dev", STEP_DEV, 0), ("group-dev-routed", GROUP_DEV, 1)])
def test_stage_image_matches_the_layout(lib, name, case, route):
    buf, info, boff, lens = _build(lib, case, route)
    want_img, want, want_boff, want_lens, want_bit_len = _model(case, bool(route))
    K, nv = case["K"], N * case["K"]
    assert info == want  # n_dev, n_iframes, max_len, hdr_bytes, bytes; where the lists sit
    assert boff == want_boff and lens == want_lens
    img = buf[GUARD:GUARD + info["bytes"]].tobytes()
    got_boff = list(struct.unpack_from("<%dQ" % nv, img, 0))
    got_bit_len = list(struct.unpack_from("<%dI" % nv, img, nv * 8))
    assert got_boff == boff and all(o % 8 == 0 for o in got_boff) and info["hdr_bytes"] % 16 == 0
    for v in range(nv):
        c, k = v % N, v // N
        idle, host = k >= case["idle_from"][c], bool(case["on_host"][c])
        skipped = idle or (host and (not case["group"] or route))  # idle lanes; host lanes under the step rule, or once a group is routed
        assert (got_bit_len[v] == SKIP) == skipped, v
        if lens[v] != SKIP:  # a gathered frame: its bytes, then at least 32 zero bytes
            at = info["hdr_bytes"] + boff[v]
            assert not any(img[at + lens[v]:at + lens[v] + 32]), v
            assert idle is False and (case["group"] or not host)
        if case["group"] and host and not idle:
            assert lens[v] != SKIP and lens[v] == want_lens[v]  # the group rule: the host parser's lane keeps its place and its real length
    assert max(x for x in lens if x != SKIP) <= BOUND
    assert not any(img[info["reset_off"] - 64:info["reset_off"]])
    assert info["reset_off"] % 16 == 0 and info["idle_off"] % 16 == 0 and info["idle_from_off"] % 16 == 0
    assert list(struct.unpack_from("<2i", img, info["reset_off"])) == case["resets"]
    idle_clips = [c for c in range(N) if case["idle_from"][c] < K]
    assert info["n_idle"] == len(idle_clips) == 1 and struct.unpack_from("<i", img, info["idle_off"])[0] == idle_clips[0]
    if case["group"]:
        assert info["idle_from_off"] and list(img[info["idle_from_off"]:info["idle_from_off"] + N]) == case["idle_from"]
    else:
        assert info["idle_from_off"] == 0
    # nothing outside [0, bytes) is written, and inside it nothing but what the layout names
    assert img == want_img
    assert (buf[:GUARD] == 0xAA).all() and (buf[GUARD + info["bytes"]:] == 0xAA).all()
