#!/usr/bin/env python3
"""What the motion ring costs (mobi_batch_set_motion, mobi_motion.hip), one process, one GPU; prints JSON lines (profiles/motion_exp.json).

  --step      4096 clips of 640x480, P-frames.  (a) decode(): wall time per frame step with motion off and on, two batches alternating
              frame by frame; (b) replay(): time of a step on the stream (HIP events around six replayed P-frames), off and on,
              alternating over three rounds -- the difference is mobi_motion_field's own time, next to the bytes it moves (the step's
              command list in, 288 B per macroblock out).
  --exports   4096 clips x 6 frames: every export format, time on the stream (HIP events, best of 5 after a warm-up), bytes = the ring
              words read + the output written, fraction of 8 TB/s.
  --clips N   another batch size
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library: one HIP runtime)

import mobiclipdecoder_amd as m  # noqa: E402
from mobiclipdecoder_amd import sharding  # noqa: E402

W, H, VER = 640, 480, 2
N_MBS = (W // 16) * (H // 16)
PEAK = 8e12  # HBM bytes/s
N_FRAMES = 8
DISTINCT = 8


def clips():
    return [m.generate_clip(m.default_params("B", sharding.stream_seed("B", 0, i), n_frames=N_FRAMES)) for i in range(DISTINCT)]


def step(n):
    S = clips()
    frames = lambda f: [S[c % DISTINCT][0][S[c % DISTINCT][1][f]:S[c % DISTINCT][1][f + 1]] for c in range(n)]
    off, on = m.MobiclipBatch(n, W, H, VER), m.MobiclipBatch(n, W, H, VER)
    on.set_motion(True)
    wall = {"off": [], "on": []}
    for f in range(N_FRAMES):
        fr = frames(f)
        for name, b in (("off", off), ("on", on)) if f & 1 else (("on", on), ("off", off)):
            t0 = time.perf_counter()
            rcs, _ = b.decode(fr, [0] * n)
            dt = (time.perf_counter() - t0) * 1e3
            assert not any(rcs)
            if f >= 2:  # (frame 0 is the I-frame, frame 1 the first step of its size)
                wall[name].append(dt)
    res = {"what": "decode() per P-frame step, wall ms", "clips": n, "size": f"{W}x{H}", "motion_off": [round(v, 3) for v in wall["off"]],
           "motion_on": [round(v, 3) for v in wall["on"]], "motion_launches": [off.motion_launches(), on.motion_launches()],
           "motion_ring_bytes": on.motion_bytes()}
    print(json.dumps(res), flush=True)
    off.close(); on.close()
    torch.cuda.empty_cache()
    # (b) replayed steps: the stream's own time
    b = m.MobiclipBatch(n, W, H, VER)
    for c in range(DISTINCT):
        assert not any(b.preload(c, S[c][0], S[c][1]))
    for c in range(DISTINCT, n):
        b.preload_clone(c, c % DISTINCT)
    b.commit()
    cmd = sum(b.cmd_bytes(f) for f in range(2, N_FRAMES)) / (N_FRAMES - 2)
    ms = {"off": [], "on": []}
    for rnd in range(3):
        for name in ("off", "on"):
            b.sync()
            b.set_motion(name == "on")
            b.replay(0); b.replay(1)
            b.time_begin()
            for f in range(2, N_FRAMES):
                b.replay(f)
            ms[name].append(b.time_end() / (N_FRAMES - 2))
    b.sync()
    b.set_motion(False)
    own = min(ms["on"]) - min(ms["off"])
    out_bytes = n * N_MBS * 288
    res = {"what": "replay() per P-frame step, stream ms", "clips": n, "motion_off": [round(v, 4) for v in ms["off"]], "motion_on": [round(v, 4) for v in ms["on"]],
           "mobi_motion_field_ms": round(own, 4), "bytes_in_cmd_list": int(cmd), "bytes_out": out_bytes,
           "gbps": round((cmd + out_bytes) / (own * 1e-3) / 1e9, 1) if own > 0 else None,
           "frac_8tbs": round((cmd + out_bytes) / (own * 1e-3) / PEAK, 4) if own > 0 else None}
    print(json.dumps(res), flush=True)
    b.close()


def exports(n):
    S = clips()
    b = m.MobiclipBatch(n, W, H, VER)
    b.set_motion(True)
    for f in range(6):
        b.decode([S[c % DISTINCT][0][S[c % DISTINCT][1][f]:S[c % DISTINCT][1][f + 1]] for c in range(n)], [0] * n)
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {"what": "export_motion, stream ms", "clips": n, "frames": 6, "size": f"{W}x{H}"}
    variants = [("cells", {}, "cells"), ("mb", {}, "mb")] + [("flow", {"block": blk, "dtype": dt}, f"flow_{blk}_{str(dt).split('.')[-1]}")
                                                             for blk, dt in ((2, torch.float32), (16, torch.float32), (8, torch.float16))]
    for fmt, kw, name in variants:
        out = b.export_motion(fmt, 5, 6, **kw)
        best = 1e30
        for _ in range(5):
            e0.record(s)
            b.export_motion(fmt, 5, 6, out=out, **kw)
            e1.record(s)
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1))
        read = 6 * n * N_MBS * (32 if fmt == "mb" else 256)
        nbytes = read + out.numel() * out.element_size()
        res[name] = {"ms": round(best, 4), "bytes": nbytes, "gbps": round(nbytes / (best * 1e-3) / 1e9, 1), "frac_8tbs": round(nbytes / (best * 1e-3) / PEAK, 4)}
        del out
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    b.close()


if __name__ == "__main__":
    n = int(sys.argv[sys.argv.index("--clips") + 1]) if "--clips" in sys.argv else 4096
    if "--step" in sys.argv:
        step(n)
    if "--exports" in sys.argv:
        exports(n)
