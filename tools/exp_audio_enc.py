#!/usr/bin/env python3
"""What the audio encoder costs on one GPU (include/mobiclip_audio_enc.h; DESIGN.md "Audio encoder").  Prints ONE JSON line and, with --out,
appends it to a file.  One process; every figure is the median of --iters single calls behind --warmup calls.

  --kernels   at --streams x --channels x --blocks (default 4096 x 2 x 6), noise over a sine:
                call_ms[B]     mobi_audio_enc_async between two HIP events, for B in 1, --blocks and 2 x --blocks.  The call is the trial
                               kernel (its work does not depend on B) and the encode kernel (linear in B) back to back on one stream, so
                               trials_ms and encode_ms_per_block are the intercept and the slope of the line through the first and the
                               last B; fit_error_ms says how far the middle B lies from it
                trials_kernel_ms, encode_kernel_ms
                               with the profiling twin of the library (MOBI_LIB=.../libmobiclip_hip_prof.so), whose
                               mobi_debug_aenc_select makes a call launch one of the two kernels alone: each kernel between two HIP
                               events at --blocks, the encode kernel reading the indices a whole call left
                pcm16_ms       the PCM16 call at --blocks
                host_ms        the same rule from the host model (tests/tools/mobi_audio_enc_host.cpp) on --host-threads threads, wall clock
                decode_ms      MobiclipAudio.decode of the frames just made (Moflex, IMA): host plan, one copy, mobi_audio_blocks<IMA>
  --clips     encode_clips(container="moflex") at --clips-n clips x --frames frames of 640x480 (tools/exp_encode_inter.py's translated mix),
              wall clock, with and without audio= (32 kHz stereo, IMA), alternating: the share audio adds
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mobiclipdecoder_amd as m  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def event_ms(call, s, iters, warmup):
    """the median of `iters` single calls, each between two events of its own"""
    for _ in range(warmup):
        call()
    s.synchronize()
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        call()
        e1.record(s)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return median(out), out


def sound(n, nc, S, seed=5):
    rng = np.random.default_rng(seed)
    return (8000 * np.sin(np.arange(S) / 11.0)[None, None] + rng.integers(-4000, 4000, (n, nc, S))).astype(np.int16)


def kernels(a, dev, res):
    from tests import audio_enc_model as A
    n, nc = a.streams, a.channels
    s = torch.cuda.current_stream(dev)
    Bs = [1, a.blocks, 2 * a.blocks]
    x_host = sound(n, nc, 256 * Bs[-1])
    x = torch.from_numpy(x_host).to(dev)
    enc = m.MobiclipAudioEncoder(n, nc, "ima", Bs[-1])
    call_ms = {}
    for B in Bs:
        view = x[:, :, :256 * B]
        call_ms[B], every = event_ms(lambda: enc.encode(view), s, a.iters, a.warmup)
        res[f"call_ms_B{B}"] = {"median": call_ms[B], "all": every}
    slope = (call_ms[Bs[2]] - call_ms[Bs[0]]) / (Bs[2] - Bs[0])
    res.update(trials_ms=call_ms[Bs[0]] - slope * Bs[0], encode_ms_per_block=slope, encode_ms=slope * a.blocks,
               fit_error_ms=call_ms[Bs[1]] - (call_ms[Bs[0]] + slope * (Bs[1] - Bs[0])))
    try:
        select = m.load_library().mobi_debug_aenc_select
    except AttributeError:
        select = None  # the product library: no hooks
    if select is not None:
        view = x[:, :, :256 * a.blocks]
        enc.encode(view)  # a whole call: the indices the encode kernel alone will read
        for only, name in ((1, "trials_kernel_ms"), (2, "encode_kernel_ms")):
            select(only)
            med, every = event_ms(lambda: enc.encode(view), s, a.iters, a.warmup)
            res[name] = {"median": med, "all": every}
        select(0)
        res["library"] = "profiling twin"
    with_all, _ = event_ms(lambda: enc.encode(x[:, :, :256 * a.blocks], recon=True, stats=True), s, a.iters, a.warmup)
    res["call_ms_with_recon_and_stats"] = with_all
    frames, sizes = enc.encode(x[:, :, :256 * a.blocks])
    enc.close()
    pcm = m.MobiclipAudioEncoder(n, nc, "pcm16", a.blocks)
    res["pcm16_ms"], _ = event_ms(lambda: pcm.encode(x[:, :, :256 * a.blocks]), s, a.iters, a.warmup)
    pcm.close()
    # the host model, the same samples
    xh = np.ascontiguousarray(x_host[:, :, :256 * a.blocks])
    A.run_host(A.IMA, xh[:64], recon=False, stats=False, threads=a.host_threads)
    ms = []
    for _ in range(max(3, a.iters // 2)):
        t0 = time.perf_counter()
        rc, slots, h_sizes, _, _ = A.run_host(A.IMA, xh, recon=False, stats=False, threads=a.host_threads)
        ms.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0
    res.update(host_ms=median(ms), host_threads=a.host_threads)
    host, ln = frames.cpu().numpy(), sizes.cpu().numpy()
    assert np.array_equal(host[:, :ln[0]], slots[:, :ln[0]]) and (ln == h_sizes).all(), "the kernels and the host model disagree"
    res["frame_bytes"] = int(ln[0])
    # the decoder at the same shape
    data = [host[i, :ln[i]].tobytes() + b"\x00\x00" for i in range(n)]
    dec = m.MobiclipAudio(n, nc, "ima", "moflex")
    out = torch.empty((n, nc, 256 * a.blocks), dtype=torch.int16, device=dev)
    res["decode_ms"], _ = event_ms(lambda: dec.decode(data, out=out), s, a.iters, a.warmup)
    dec.close()


def clips(a, dev, res):
    from exp_encode_inter import H, VERSION, W, pairs
    _, cur = pairs("translated", np.random.default_rng(77))
    src = torch.from_numpy(cur).to(dev)
    n, T = a.clips_n, a.frames
    frames = torch.stack([src[(torch.arange(n, device=dev) + t) % 16] for t in range(T)], 1).contiguous()
    rate, nc = 32000, 2
    need = 256 * (T * rate // (30 * 256))
    audio = torch.from_numpy(sound(n, nc, need)).to(dev)
    runs = {"video": lambda: m.encode_clips(frames, a.quantizer, T, VERSION, W, H, container="moflex"),
            "audio": lambda: m.encode_clips(frames, a.quantizer, T, VERSION, W, H, container="moflex", audio=audio, audio_rate=rate)}
    ms = {k: [] for k in runs}
    for k in runs:
        runs[k]()
    for _ in range(a.iters):
        for k in ("video", "audio"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = runs[k]()
            ms[k].append((time.perf_counter() - t0) * 1e3)
            res[f"clips_{k}_file_bytes"] = sum(len(f) for f in got)
    v, w = median(ms["video"]), median(ms["audio"])
    res.update(clips_n=n, frames=T, clips_video_ms=v, clips_audio_ms=w, clips_video_ms_all=ms["video"], clips_audio_ms_all=ms["audio"], audio_share=(w - v) / w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--clips", action="store_true")
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--clips-n", type=int, default=64)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--quantizer", type=int, default=30)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"streams": a.streams, "channels": a.channels, "blocks": a.blocks, "iters": a.iters}
    if a.kernels:
        kernels(a, dev, res)
    if a.clips:
        clips(a, dev, res)
    line = json.dumps(json.loads(json.dumps(res), parse_float=lambda x: round(float(x), 4)))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
