#!/usr/bin/env python3
"""Rate at which decoded frames reach host memory (mobi_batch_export), one process, one GPU; prints ONE JSON line.

  d2h_ceiling_gbps           a plain 256 MB hipMemcpyAsync device -> mobi_host_alloc memory, HIP events, best of 10
  export_gbps / export_frac  sustained mobi_batch_export into mobi_host_alloc memory, 640x480, 512 clips, >= 8 GB per timed region, per
                             format (GB/s of picture bytes; fraction of the ceiling)
  end_to_end_to_host_gpix_s  decode + I420 export of every frame of 4096 clips x 32-frame groups (gop_begin / gop_finish, the next group
                             begun; ONE export per part gop_finish reports, (P - 1, P), as INTEGRATION.md's loop; nothing waited for until
                             the end); bound = d2h_ceiling_gbps / 1.5
  getter_loop_gpix_s         the same pictures through today's per-clip mobi_batch_get_planes loop, 1024 clips
  --pack-only                exports only (for `rocprofv3 --kernel-trace --stats -- python tools/exp_export.py --pack-only`: the pack
                             kernel's time per launch)
  --export-only              the ceiling and the export rates only
  --e2e-only                 end_to_end only (for a `rocprofv3 --kernel-trace --memory-copy-trace` run of it)
  --prof                     the -DMOBI_PROFILING twin of the library (MOBI_EXPORT_CHUNKS / MOBI_EXPORT_CHUNK_MB: the staging A/B)
"""
import ctypes as C
import json
import os
import sys
import time

if "--prof" in sys.argv:
    import _prof  # noqa: F401
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import mobiclipdecoder_amd as m  # noqa: E402
from mobiclipdecoder_amd import build, sharding  # noqa: E402

W, H, VER = 640, 480, 2
PX = W * H


def streams(n_frames, distinct=8, iframe_interval=None):
    out = []
    for i in range(distinct):
        kw = {"n_frames": n_frames}
        if iframe_interval:
            kw["iframe_interval"] = iframe_interval
        data, fo = m.generate_clip(m.default_params("B", sharding.stream_seed("B", 0, i), **kw))
        out.append([data[fo[f]:fo[f + 1]] for f in range(n_frames)])
    return out


def d2h_ceiling(nbytes=256 << 20, reps=10):
    hip = C.CDLL(os.path.join(build.ROCM, "lib", "libamdhip64.so"))
    lib = m.load_library()
    src, s, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipSetDevice(0) == 0 and hip.hipMalloc(C.byref(src), C.c_size_t(nbytes)) == 0
    assert hip.hipStreamCreate(C.byref(s)) == 0 and hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    dst = lib.mobi_host_alloc(nbytes)
    assert dst
    best = 0.0
    for _ in range(reps):
        hip.hipEventRecord(e0, s)
        assert hip.hipMemcpyAsync(C.c_void_p(dst), src, C.c_size_t(nbytes), 2, s) == 0  # hipMemcpyDeviceToHost
        hip.hipEventRecord(e1, s)
        assert hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), e0, e1)
        best = max(best, nbytes / (ms.value * 1e-3) / 1e9)
    lib.mobi_host_free(dst)
    hip.hipFree(src)
    return best


def export_rate(b, fmt, min_bytes=8e9):
    pic = PX * 3 // 2 if fmt == "i420" else PX * 4
    shape = (1, b.n, pic) if fmt == "i420" else (1, b.n, H, W)
    dst = m.host_empty(shape, np.uint8 if fmt == "i420" else np.uint32)
    b.export(fmt, 0, 1, out=dst)  # (staging allocated, warm)
    reps = int(np.ceil(min_bytes / dst.nbytes))
    t0 = time.perf_counter()
    hs = [b.export(fmt, r % 6, 1, out=dst, wait=False) for r in range(reps)]  # (the same destination over and over: only the rate counts)
    hs[-1].wait()
    dt = time.perf_counter() - t0
    return reps * dst.nbytes / dt / 1e9


def end_to_end(n_clips=4096, G=32, n_groups=3):
    S = streams(G * n_groups, iframe_interval=G)
    b = m.MobiclipBatch(n_clips, W, H, VER, device_parse=True)
    group = lambda g: [[S[c % len(S)][k] for c in range(n_clips)] for k in range(g * G, (g + 1) * G)]
    dst = m.host_empty((6, n_clips, PX * 3 // 2), np.uint8)  # one part (six frames) of every clip: every export goes here (only the rate counts)
    # group 0 untimed (allocations, the I-frame)
    b.gop_begin(group(0))
    b.gop_begin(group(1))
    while True:
        rcs, _ = b.gop_finish()
        if b.gop_frames_pending() == G:
            break
    h = None
    t0 = time.perf_counter()
    frames = 0
    for g in range(1, n_groups):
        if g + 1 < n_groups:
            b.gop_begin(group(g + 1))
        while True:
            rcs, _ = b.gop_finish()
            P = len(rcs)
            h = b.export("i420", P - 1, P, out=dst[:P], wait=False)  # the whole part in one call
            frames += P
            if b.gop_frames_pending() in (0, G):
                break
    h.wait()
    dt = time.perf_counter() - t0
    b.close()
    return frames * n_clips * PX / dt / 1e9, frames


def getter_loop(n_clips=1024):
    S = streams(1)
    b = m.MobiclipBatch(n_clips, W, H, VER)
    b.decode([S[c % len(S)][0] for c in range(n_clips)], [0] * n_clips)
    b.planes(0)
    t0 = time.perf_counter()
    for c in range(n_clips):
        b.planes(c)
    dt = time.perf_counter() - t0
    b.close()
    return n_clips * PX / dt / 1e9


def main():
    S = streams(6)
    b = m.MobiclipBatch(512, W, H, VER)
    for f in range(6):
        b.decode([S[c % len(S)][f] for c in range(512)], [0] * 512)
    if "--e2e-only" in sys.argv:
        b.close()
        e2e, frames = end_to_end()
        print(json.dumps({"end_to_end_to_host_gpix_s": round(e2e, 4), "end_to_end_frames_timed": frames}), flush=True)
        return
    if "--pack-only" in sys.argv:
        for fmt in ("i420", "argb"):
            export_rate(b, fmt, 4e9)
        b.close()
        print(json.dumps({"pack_only": True}))
        return
    res = {"d2h_ceiling_gbps": d2h_ceiling()}
    for fmt in ("i420", "argb"):
        r = export_rate(b, fmt)
        res[f"export_gbps_{fmt}"] = r
        res[f"export_frac_{fmt}"] = r / res["d2h_ceiling_gbps"]
    b.close()
    res["staging"] = {k: os.environ[k] for k in ("MOBI_EXPORT_CHUNKS", "MOBI_EXPORT_CHUNK_MB") if k in os.environ} or "default"
    if "--export-only" in sys.argv:  # (the staging A/B)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
        return
    e2e, frames = end_to_end()
    res["end_to_end_to_host_gpix_s"] = e2e
    res["end_to_end_frames_timed"] = frames
    res["end_to_end_export_calls"] = "one per gop_finish part: (P - 1, P)"
    res["end_to_end_bound_gpix_s"] = res["d2h_ceiling_gbps"] / 1.5
    res["end_to_end_frac_of_bound"] = e2e / res["end_to_end_bound_gpix_s"]
    res["getter_loop_gpix_s"] = getter_loop()
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
