#!/usr/bin/env python3
"""Throughput of the batched audio decode on one GPU (MobiclipAudio.decode, int16 planar, output allocated once, torch's current stream;
FastAudio and IMA in Moflex framing, Sx in Mods framing); prints ONE JSON line and writes it to --out.

Per codec (FastAudio, IMA, Sx; --codecs): 4096 streams x 2 channels x 4 blocks per call (--streams, --channels, --blocks; an Sx "block" is
a packet of 128 samples, of random rate and lag, every sixth a reset packet, over eight random codebooks).
  call_ms      wall time per call over --iters back-to-back calls ended by one synchronise: plan + gather + one copy + launch on the host,
               overlapped with the previous calls' kernels (a call does not wait for its own) -- what a loader sees
  device_ms    HIP events around ONE call's device work, its copy (h2d_bytes) and kernel, enqueued while the stream is held busy so that
               the host's part of the call is not between the events; median and minimum
  copy_ms      HIP events around a bare pinned-to-device copy of h2d_bytes (median): kernel_ms = device_ms_median - copy_ms, and
               kernel_share_of_call = kernel_ms / call_ms
  device_share_of_call = device_ms_median / call_ms: near 1 the calls are bound by the device, below by the host (Python's per-stream
               handling, plan and gather)
  blocks_per_s, samples_per_s   from call_ms
  ns_per_sample_per_lane = kernel_ms / (256 * blocks) (Sx: 128 * blocks): what one lane's dependent chain takes per sample, write-out and,
               for Sx, the load and store of its 546-word state included
  variants     device_ms_median of the same call as float32 planar (twice the bytes stored), int16 interleaved, and with 2 and 4 times the
               streams (int16 planar): a kernel bound by each lane's dependent chain takes the same time until the SIMDs fill up; one
               bound by its stores takes longer with float32
For scale: --bench-ms takes the project's reconstruction step time of the same session's `python bench.py` (ms per step) into the record.
For `rocprofv3 --kernel-trace --stats -- python tools/exp_audio.py` the kernels are mobi_audio_blocks<0> (FastAudio), <1> (IMA) and mobi_sx_packets.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mobiclipdecoder_amd as m  # noqa: E402


def lcg(n, x):
    out = bytearray(n)
    for i in range(n):
        x = (x * 1103515245 + 12345) % (1 << 31)
        out[i] = (x >> 16) & 0xFF
    return bytes(out)


def frames_for(codec, streams, channels, blocks):
    """eight distinct frames shared by the streams (the kernel's time does not depend on which lanes hold which bytes)"""
    size = 40 if codec == "fastaudio" else 128
    distinct = []
    for k in range(8):
        head = b"".join(bytes([(k * 11 + c) % 89, 0, 0, 0]) for c in range(channels)) if codec == "ima" else b""
        distinct.append(head + lcg(size * channels * blocks, 1 + k) + b"\0\0")
    return [distinct[s % 8] for s in range(streams)]


def sx_setup(streams, channels, blocks):
    """eight distinct (codebook, packets of one lane and call); a stream's frame deals its lanes' packets round robin"""
    lanes = []
    for k in range(8):
        packets = []
        for b in range(blocks):
            p = bytearray(lcg(20, 100 + 8 * b + k))
            p[1] = 0xFE | (p[1] & 1) if (b + k) % 6 == 0 else (p[1] if p[1] >> 1 != 0x7F else p[1] & ~2)
            packets.append(bytes(p[:(20, 14, 12, 10)[(p[3] >> 4) & 3]]))
        lanes.append((lcg(0xC34, 50 + k), packets))
    frames, books = [], []
    for s in range(streams):
        mine = [lanes[(s * channels + c) % 8] for c in range(channels)]
        frames.append(b"".join(mine[c][1][b] for b in range(blocks) for c in range(channels)))
        books.append([mine[c][0] for c in range(channels)])
    return frames, books


def setup(codec, streams, a, dev):
    """-> (decoder, frames, decode()'s framing arguments, samples per block, staged bytes: the blocks and a 16-byte descriptor per lane)"""
    if codec == "sx":
        frames, books = sx_setup(streams, a.channels, a.blocks)
        au = m.MobiclipAudio(streams, a.channels, "sx", "mods", device=dev.index, codebooks=books)
        return au, frames, dict(offsets=[0] * streams, n_packets=[a.channels * a.blocks] * streams), 128, sum(len(f) for f in frames) + 16 * streams * a.channels
    au = m.MobiclipAudio(streams, a.channels, codec, "moflex", device=dev.index)
    h2d = streams * a.channels * a.blocks * (40 if codec == "fastaudio" else 128) + 16 * streams * a.channels
    return au, frames_for(codec, streams, a.channels, a.blocks), {}, 256, h2d


_BLOCKER = {}


def hold_stream(ms, dev):
    """keeps the current stream busy for at least `ms`: what is enqueued meanwhile starts back to back when it ends"""
    if dev not in _BLOCKER:
        t = torch.empty(1 << 28, dtype=torch.float32, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t.add_(1.0)
        e0.record()
        for _ in range(4):
            t.add_(1.0)
        e1.record()
        e1.synchronize()
        _BLOCKER[dev] = (t, e0.elapsed_time(e1) / 4)
    t, each = _BLOCKER[dev]
    for _ in range(int(ms / each) + 1):
        t.add_(1.0)


def device_ms(au, frames, out, iters, dev, host_ms, **kw):
    """median and minimum of the HIP-event time of one call's copy + kernel.  The stream is held busy for three times the call's host
    time first, so that the copy and the kernel are already enqueued when the first event fires: the events bracket device work alone"""
    s = torch.cuda.current_stream(dev)
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        hold_stream(3 * host_ms + 5, dev)
        e0.record(s)
        au.decode(frames, out=out, **kw)
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def copy_ms(n, iters, dev):
    src, dst = torch.empty(n, dtype=torch.uint8).pin_memory(), torch.empty(n, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev)
    ms = []
    for _ in range(iters + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record(s)
        dst.copy_(src, non_blocking=True)
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = sorted(ms[2:])
    return ms[len(ms) // 2]


def variant(codec, a, dev, streams, dtype, layout):
    au, frames, kw, spb, _ = setup(codec, streams, a, dev)
    shape = (streams, a.channels, spb * a.blocks) if layout == "planar" else (streams, spb * a.blocks, a.channels)
    out = torch.empty(shape, dtype=dtype, device=dev)
    for _ in range(a.warmup):
        au.decode(frames, out=out, dtype=dtype, layout=layout, **kw)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    au.decode(frames, out=out, dtype=dtype, layout=layout, **kw)
    torch.cuda.synchronize(dev)
    med = device_ms(au, frames, out, a.iters, dev, (time.perf_counter() - t0) * 1e3, dtype=dtype, layout=layout, **kw)[0]
    au.close()
    return med


def run(codec, a):
    dev = torch.device("cuda", torch.cuda.current_device())
    au, frames, kw, spb, h2d = setup(codec, a.streams, a, dev)
    out = torch.empty((a.streams, a.channels, spb * a.blocks), dtype=torch.int16, device=dev)
    for _ in range(a.warmup):
        au.decode(frames, out=out, **kw)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(a.iters):
        au.decode(frames, out=out, **kw)
    torch.cuda.synchronize(dev)
    call = (time.perf_counter() - t0) / a.iters
    med, low = device_ms(au, frames, out, a.iters, dev, call * 1e3, **kw)
    n_blocks = a.streams * a.channels * a.blocks
    au.close()
    cp = copy_ms(h2d, a.iters, dev)
    res = {"call_ms": call * 1e3, "device_ms_median": med, "device_ms_min": low, "h2d_bytes": h2d, "copy_ms": cp, "kernel_ms": med - cp,
           "kernel_share_of_call": (med - cp) / (call * 1e3), "device_share_of_call": med / (call * 1e3),
           "ns_per_sample_per_lane": (med - cp) * 1e6 / (spb * a.blocks),
           "blocks_per_s": n_blocks / call, "samples_per_s": n_blocks * spb / call}
    if a.variants:
        res["device_ms_float32"] = variant(codec, a, dev, a.streams, torch.float32, "planar")
        res["device_ms_interleaved"] = variant(codec, a, dev, a.streams, torch.int16, "interleaved")
        res["device_ms_streams_x2"] = variant(codec, a, dev, 2 * a.streams, torch.int16, "planar")
        res["device_ms_streams_x4"] = variant(codec, a, dev, 4 * a.streams, torch.int16, "planar")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bench-ms", type=float, default=None, help="ms per reconstruction step from the same session's python bench.py")
    ap.add_argument("--no-variants", dest="variants", action="store_false", help="the headline configuration only")
    ap.add_argument("--codecs", default="fastaudio,ima,sx", help="comma-separated: fastaudio, ima, sx")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"streams": a.streams, "channels": a.channels, "blocks_per_call": a.blocks, "iters": a.iters, "dtype": "int16", "layout": "planar"}
    for codec in a.codecs.split(","):
        for k, v in run(codec, a).items():
            res[f"{codec}_{k}"] = round(v, 4) if isinstance(v, float) and v < 1e6 else (float("%.4g" % v) if isinstance(v, float) else v)
    if a.bench_ms is not None:
        res["bench_step_ms"] = a.bench_ms
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
