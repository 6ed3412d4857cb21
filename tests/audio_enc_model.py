"""The audio encoder's rule in plain Python integers (include/mobiclip_audio_enc.h; DESIGN.md "Audio encoder"): the expectation of
tests/test_audio_enc_model.py and tests/test_audio_enc_gpu.py, with the signals they share and the binding of the C++ host model
(tests/tools/mobi_audio_enc_host.cpp).  Written from the rule's statement, not from csrc/mobi_audio_enc.h:

  nibble   from a decoder state (last, index) the code of sample x is the val in 0..15 minimising |x - s(val)|, s(val) the clamped sample
           the decoder makes of val from that state; ties to the smallest val -- sixteen trials, literally
  header   last = x[0]; index = the i0 in 0..88 with the least E(i0) = sum over block 0 of (x[k] - r[k])^2, ties to the smallest
  frame    C headers (s16le index, s16le last), then block b of channel c at 4 C + 128 (b C + c), low nibble first
  stats    u64 sse over the frame, u32 samples where the clamp acted, u32 the header's index
  PCM16    the samples interleaved, s16le; the reconstruction is the input

The tables come through the library's getter (audio.tables(); tests/test_audio_model.py pins their CRCs)."""
import ctypes as C
import functools
import math
import struct

import numpy as np

IMA, PCM16, FASTAUDIO, SX = 1, 2, 0, 3
E_ARG, E_UNSUPPORTED = -7, -6
STATS_DTYPE = np.dtype([("sse", "<u8"), ("clamped", "<u4"), ("start_index", "<u4")])
FILL = 0xA5


@functools.lru_cache(maxsize=None)
def _tables():
    from mobiclipdecoder_amd import audio
    t = audio.tables()
    return [int(v) for v in t["ima_step"]], [int(v) for v in t["ima_index"]]


def decode_step(val, last, index):
    """IMAADPCMDecoder's nibble: -> (the clamped sample, the sample before the clamp, the next index)"""
    step_tab, index_tab = _tables()
    step = step_tab[index]
    diff = step // 8 + (step // 4 if val & 1 else 0) + (step // 2 if val & 2 else 0) + (step if val & 4 else 0)
    raw = last - diff if val & 8 else last + diff
    return max(-32768, min(32767, raw)), raw, max(0, min(88, index + index_tab[val & 7]))


def nibble(x, last, index):
    """the sixteen trials"""
    best, best_d = None, None
    for val in range(16):
        d = abs(x - decode_step(val, last, index)[0])
        if best is None or d < best_d:
            best, best_d = val, d
    return best


def code(x, i0):
    """samples x coded from (x[0], i0) -> (nibbles, reconstruction, squared error, samples where the clamp acted)"""
    last, index = int(x[0]), i0
    vals, rec, sse, clamped = [], [], 0, 0
    for v in x:
        v = int(v)
        val = nibble(v, last, index)
        last, raw, index = decode_step(val, last, index)
        clamped += raw != last
        vals.append(val)
        rec.append(last)
        sse += (v - last) ** 2
    return vals, rec, sse, clamped


_channel_memo = {}


def encode_channel(x):
    """one channel of one frame -> (header index, nibble bytes, reconstruction, sse, clamped)"""
    x = [int(v) for v in x]
    key = struct.pack("<%dh" % len(x), *x)
    hit = _channel_memo.get(key)
    if hit is None:
        errors = trial_errors(x[:256])
        i0 = min(range(89), key=lambda i: (errors[i], i))
        vals, rec, sse, clamped = code(x, i0)
        hit = _channel_memo[key] = (i0, bytes(vals[2 * i] | vals[2 * i + 1] << 4 for i in range(len(x) // 2)), rec, sse, clamped)
    return hit


_trial_memo = {}


def trial_errors(block0):
    """E(i0) for the 89 start indices"""
    key = tuple(block0)
    if key not in _trial_memo:
        _trial_memo[key] = [code(block0, i0)[2] for i0 in range(89)]
    return _trial_memo[key]


def encode_frame(codec, x):
    """x: (C, 256 B) ints -> (frame bytes, reconstruction (C, 256 B) int16, stats (C,) STATS_DTYPE)"""
    x = np.asarray(x)
    nc, S = x.shape
    assert S % 256 == 0 and S
    stats = np.zeros(nc, STATS_DTYPE)
    if codec == PCM16:
        return np.ascontiguousarray(x.T, "<i2").tobytes(), x.astype(np.int16), stats
    B = S // 256
    frame = bytearray(4 * nc + 128 * nc * B)
    rec = np.zeros((nc, S), np.int16)
    for c in range(nc):
        i0, data, r, sse, clamped = encode_channel(x[c])
        struct.pack_into("<hh", frame, 4 * c, i0, int(x[c, 0]))
        for b in range(B):
            at = 4 * nc + 128 * (b * nc + c)
            frame[at:at + 128] = data[128 * b:128 * b + 128]
        rec[c] = r
        stats[c] = (sse, clamped, i0)
    return bytes(frame), rec, stats


def frame_bytes(codec, nc, B):
    return 4 * nc + 128 * nc * B if codec == IMA else 512 * nc * B


# ---- the signals: name -> channel variant v, S samples.  Few distinct channels (the model memoises a channel by its samples) ----
SIGNALS = ("silence", "square2", "square64", "jump", "neg_noise", "noise", "sine12")


@functools.lru_cache(maxsize=None)
def _channel(name, v, S):
    k = np.arange(S)
    if name == "silence":
        x = np.zeros(S, np.int64)
    elif name in ("square2", "square64"):  # full scale, the clamp domain; odd variants start low
        half = 1 if name == "square2" else 32
        x = np.where((k // half + v) % 2 == 0, 32767, -32768)
    elif name == "jump":
        x = np.where(k == 0, 0, 32767)
    elif name in ("neg_noise", "noise"):
        # (eight different channels of noise: with C = 8 a swap of any two channels shows; -32768 + noise has four, the trials cost)
        x = np.random.default_rng(7100 + 10 * SIGNALS.index(name) + v % (8 if name == "noise" else 4)).integers(-32768, 32768, S)
        if name == "neg_noise":
            x[0] = -32768
    else:  # the index sits at 0
        x = np.array([int(round(12 * math.sin(2 * math.pi * (i + 5 * (v % 8)) / 50))) for i in range(S)])
    x = x.astype(np.int16)
    x.setflags(write=False)
    return x


def signal(name, nc, B):
    """(C, 256 B) int16: the channels of a longer frame begin as those of a shorter one"""
    return np.stack([_channel(name, c, 256 * 3)[:256 * B] for c in range(nc)])


def batch(n, nc, B, offset=0):
    """(n, C, 256 B) int16: stream s carries signal (s + offset) mod 7, its channels moved on by s // 7: over the seven offsets every
    stream position of a shape, the first of a one-stream shape too, carries every signal"""
    k = len(SIGNALS)
    return np.stack([np.stack([_channel(SIGNALS[(s + offset) % k], c + s // k, 256 * 3)[:256 * B] for c in range(nc)]) for s in range(n)])


def encode_batch(codec, x):
    """the model over (n, C, S) -> (frames as a list of bytes, recon (n, C, S) int16, stats (n * C,) STATS_DTYPE)"""
    out = [encode_frame(codec, x[s]) for s in range(x.shape[0])]
    return [o[0] for o in out], np.stack([o[1] for o in out]), np.concatenate([o[2] for o in out])


# ---- the C++ host model ----
@functools.lru_cache(maxsize=None)
def host():
    from mobiclipdecoder_amd import build
    lib = C.CDLL(build.build_audioenchost())
    P = C.c_void_p
    lib.aenc_host_run.restype = C.c_int
    lib.aenc_host_run.argtypes = [C.c_int] * 5 + [P, C.c_size_t, C.c_int, P, C.c_size_t, C.c_size_t, P, P, C.c_size_t, P, C.c_int]
    lib.aenc_host_check.restype = C.c_int
    lib.aenc_host_check.argtypes = [C.c_int] * 5 + [P, C.c_size_t, C.c_int, P, C.c_size_t, C.c_size_t, P, P, C.c_size_t, P]
    lib.aenc_host_frame_bytes.restype = C.c_uint64
    lib.aenc_host_frame_bytes.argtypes = [C.c_int] * 3
    lib.aenc_host_nibble.restype = C.c_uint32
    lib.aenc_host_nibble.argtypes = [C.c_int] * 3
    lib.aenc_host_trial.restype = C.c_uint64
    lib.aenc_host_trial.argtypes = [P, C.c_int, C.c_int]
    return lib


def run_host(codec, x, pitch_extra=0, slot_extra=0, recon=True, stats=True, threads=1):
    """the host model over (n, C, S) int16 at a sample pitch of S + pitch_extra, slots of FILL at a pitch of slot_bytes + slot_extra
    -> (rc, slots (n, slot_bytes + slot_extra) uint8, sizes (n,) int32, recon (n, C, S) int16 or None, stats (n * C,) or None)"""
    n, nc, S = x.shape
    B = S // 256
    padded = np.full((n, nc, S + pitch_extra), 0x5A5A, np.int16)
    padded[:, :, :S] = x
    slot = (frame_bytes(codec, nc, B) + 3) & ~3
    slots = np.full((n, slot + slot_extra), FILL, np.uint8)
    sizes = np.full(n, -1, np.int32)
    rec = np.zeros((n, nc, S), np.int16) if recon else None
    st = np.zeros(n * nc, STATS_DTYPE) if stats else None
    rc = host().aenc_host_run(codec, n, nc, B, n, padded.ctypes.data, S + pitch_extra, B, slots.ctypes.data, slot + slot_extra, slot, sizes.ctypes.data,
                              rec.ctypes.data if recon else None, S, st.ctypes.data if stats else None, threads)
    return rc, slots, sizes, rec, st
