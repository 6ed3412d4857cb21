#!/usr/bin/env python3
"""Export of decoded pictures into device memory (mobi_batch_export_device, MobiclipBatch.export_tensor), one process, one GPU; prints JSON
lines.

  (default)        per variant (i420, argb, rgb nchw / nhwc x uint8 / float16 / float32) at 640x480, 512 .. 4096 clips x 6 frames: time per
                   export on the stream (HIP events, best of 5 after a warm-up), bytes = 1.5 B/px read + the output written, fraction of
                   8 TB/s.  These include launch gaps (argb: one launch per frame); the kernel's own time comes from --kernels.
  --kernels        the same exports at 4096 clips only, 10 per variant, nothing timed: for `rocprofv3 --kernel-trace --stats -- python
                   tools/exp_export_device.py --kernels`, whose kernel_stats.csv --from-stats turns into the table
  --from-stats CSV per variant: the kernel's mean time from rocprofv3's kernel_stats.csv, bytes, fraction of 8 TB/s
  --e2e            decode 4096 clips in 32-frame groups (gop_begin / gop_finish, the next group begun) with one device export per part
                   gop_finish reports, (P - 1, P) -- RGB uint8 NCHW, RGB float16 NCHW -- against decode alone, alternating, two rounds
  --nt             (needs --prof) the RGB kernel's stores plain against nontemporal (MOBI_EXPORT_RGB_NT), each export followed at once by a
                   consumer on the same stream (a torch reduction over the tensor): export + consumer time, alternating
  --scaled         the scaled export (mobi_batch_export_device_scaled): 512 clips x 6 frames of 640x480, centre crop 480x480 -> 224x224,
                   uint8 and float16 NCHW, three legs alternating over two rounds (HIP events, best of 3): (a) the full-size export plus
                   torch's crop and adaptive_avg_pool2d on the same stream, (b) the scaled export, (c) the full-size export alone.
                   --clips N: another batch size (above 512 clips leg (a) hands torch more than 2^31 elements per call: not measured)
  --scaled --kernels   legs (b) and (c) only, 10 each, nothing timed: for a `rocprofv3 --kernel-trace --stats` run of its own
  --scaled --e2e   the --e2e run with the scaled export per part against decode alone and the full-size export
  --boxes          the resampled export (mobi_batch_export_device_boxes) at the 512 clips x 6 frames of 640x480 of --scaled (no --clips: the
                   batch is not made larger), -> 224x224, uint8 and float16 NCHW, legs alternating over two rounds (HIP events, best of 3):
                   (a) the full-size export plus a per-clip loop of torch's crop, interpolate (area / bilinear, antialias off) and flip on the
                   same stream, (b) the resampled export with a random box (8 - 100 % of the area, 3:4 .. 4:3) and a random flip per clip,
                   (c) the resampled export with the centre 480x480 box for every clip, (d) the scaled export at that crop
  --boxes --kernels    legs (b), (c), (d) only, 10 each, nothing timed: for a `rocprofv3 --kernel-trace --stats` run of its own
  --prof           the -DMOBI_PROFILING twin of the library
"""
import json
import os
import sys
import time

if "--prof" in sys.argv:
    import _prof  # noqa: F401
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library: one HIP runtime)

import mobiclipdecoder_amd as m  # noqa: E402
from mobiclipdecoder_amd import sharding  # noqa: E402

W, H, VER = 640, 480, 2
PX = W * H
PEAK = 8e12  # HBM bytes/s
VARIANTS = [("i420", "nchw", torch.uint8), ("argb", "nchw", torch.uint8)] + [
    ("rgb", lay, dt) for lay in ("nchw", "nhwc") for dt in (torch.uint8, torch.float16, torch.float32)]
ESIZE = {torch.uint8: 1, torch.float16: 2, torch.float32: 4}


def name(fmt, layout, dt):
    return fmt if fmt != "rgb" else f"rgb_{layout}_{str(dt).split('.')[-1]}"


def out_bytes_per_px(fmt, dt):
    return 1.5 if fmt == "i420" else 4 if fmt == "argb" else 3 * ESIZE[dt]


def streams(n_frames, distinct=8, iframe_interval=None):
    out = []
    for i in range(distinct):
        kw = {"n_frames": n_frames}
        if iframe_interval:
            kw["iframe_interval"] = iframe_interval
        data, fo = m.generate_clip(m.default_params("B", sharding.stream_seed("B", 0, i), **kw))
        out.append([data[fo[f]:fo[f + 1]] for f in range(n_frames)])
    return out


def resident(n_clips):
    S = streams(6)
    b = m.MobiclipBatch(n_clips, W, H, VER)
    for f in range(6):
        b.decode([S[c % len(S)][f] for c in range(n_clips)], [0] * n_clips)
    return b


def time_exports(b, fmt, layout, dt, out, reps=5):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.export_tensor(fmt, 5, 6, layout=layout, dtype=dt, out=out)  # warm
    best = 1e30
    for _ in range(reps):
        e0.record(s)
        b.export_tensor(fmt, 5, 6, layout=layout, dtype=dt, out=out)
        e1.record(s)
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def rates():
    for n in (512, 1024, 2048, 4096):
        b = resident(n)
        res = {"clips": n, "frames": 6, "size": f"{W}x{H}"}
        for fmt, layout, dt in VARIANTS:
            out = b.export_tensor(fmt, 5, 6, layout=layout, dtype=dt)
            ms = time_exports(b, fmt, layout, dt, out)
            nbytes = 6 * n * PX * (1.5 + out_bytes_per_px(fmt, dt))
            res[name(fmt, layout, dt)] = {"ms": round(ms, 4), "gbps": round(nbytes / (ms * 1e-3) / 1e9, 1),
                                          "frac_8tbs": round(nbytes / (ms * 1e-3) / PEAK, 4)}
            del out
            torch.cuda.empty_cache()
        b.close()
        torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


def kernels(n=4096, reps=10):
    b = resident(n)
    for fmt, layout, dt in VARIANTS:
        out = b.export_tensor(fmt, 5, 6, layout=layout, dtype=dt)
        for _ in range(reps):
            b.export_tensor(fmt, 5, 6, layout=layout, dtype=dt, out=out)
        torch.cuda.synchronize()
        del out
        torch.cuda.empty_cache()
    b.close()
    print(json.dumps({"kernels": True, "clips": n, "frames": 6, "reps": reps + 1}), flush=True)


def from_stats(path, n=4096):
    """rocprofv3's kernel_stats.csv (Name, Calls, ..., AverageNs, ...) -> per variant: mean kernel time, bytes, fraction of 8 TB/s"""
    import csv
    rows = {r["Name"]: r for r in csv.DictReader(open(path))}
    kern = {"i420": "mobi_export_i420", "argb": "mobi_yuv_to_argb"}
    res = {"clips": n, "frames": 6, "size": f"{W}x{H}", "source": os.path.basename(path)}
    for fmt, layout, dt in VARIANTS:
        if fmt == "rgb":
            k = "mobi_export_rgb<%d, %d, false>" % (1 if layout == "nchw" else 0, ESIZE[dt])
        else:
            k = kern[fmt]
        hit = [r for nm, r in rows.items() if k in nm]
        if not hit:
            continue
        ns = float(hit[0]["AverageNs"])
        pics = 6 * n if fmt != "argb" else n  # (argb: one launch per frame)
        nbytes = pics * PX * (1.5 + out_bytes_per_px(fmt, dt))
        res[name(fmt, layout, dt)] = {"kernel": hit[0]["Name"][:60], "calls": int(hit[0]["Calls"]), "mean_ms": round(ns * 1e-6, 4),
                                      "tbs": round(nbytes / (ns * 1e-9) / 1e12, 3), "frac_8tbs": round(nbytes / (ns * 1e-9) / PEAK, 4)}
    print(json.dumps(res), flush=True)


CROP, SIZE = (80, 0, 480, 480), (224, 224)  # --scaled: the centre square of 640x480, the size a vision model takes


def end_to_end(mode, n_clips=4096, G=32, n_groups=3, S=None):
    """decode (+ one device export per part) of groups 1 .. n_groups - 1; group 0 untimed.  -> Gpixels/s of decoded frames"""
    b = m.MobiclipBatch(n_clips, W, H, VER, device_parse=True)
    group = lambda g: [[S[c % len(S)][k] for c in range(n_clips)] for k in range(g * G, (g + 1) * G)]
    dt = {"u8": torch.uint8, "f16": torch.float16}.get(mode.split("_")[0])
    kw = dict(crop=CROP, size=SIZE) if mode.endswith("_scaled") else {}
    out = torch.empty((6, n_clips, 3) + (SIZE if kw else (H, W)), dtype=dt, device="cuda") if dt is not None else None
    b.gop_begin(group(0))
    b.gop_begin(group(1))
    while True:
        b.gop_finish()
        if b.gop_frames_pending() == G:
            break
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frames = 0
    for g in range(1, n_groups):
        if g + 1 < n_groups:
            b.gop_begin(group(g + 1))
        while True:
            rcs, _ = b.gop_finish()
            P = len(rcs)
            if out is not None:
                b.export_tensor("rgb", P - 1, P, dtype=dt, out=out[:P], **kw)  # the whole part in one call, on the current stream
            frames += P
            if b.gop_frames_pending() in (0, G):
                break
    torch.cuda.synchronize()  # (the device: the batch's streams too)
    dt_s = time.perf_counter() - t0
    b.close()
    del out
    torch.cuda.empty_cache()
    return frames * n_clips * PX / dt_s / 1e9


def e2e():
    S = streams(32 * 3, iframe_interval=32)
    for rnd in range(2):
        for mode in ("decode", "u8", "f16"):
            g = end_to_end(mode, S=S)
            print(json.dumps({"round": rnd, "mode": mode if mode == "decode" else f"decode + rgb nchw {mode} export per part",
                              "clips": 4096, "group": 32, "gpix_s": round(g, 2)}), flush=True)


def scaled_legs(b, dt):
    """the three legs of --scaled for one dtype: name -> a function that enqueues it on the current stream"""
    x, y, w, h = CROP
    full = b.export_tensor("rgb", 5, 6, dtype=dt)
    small = b.export_tensor("rgb", 5, 6, dtype=dt, crop=CROP, size=SIZE)

    def parent_route():  # what a caller did before: full size, then the framework's crop and area average (in float16 for uint8)
        t = b.export_tensor("rgb", 5, 6, dtype=dt, out=full)[..., y:y + h, x:x + w].flatten(0, 1)
        return torch.nn.functional.adaptive_avg_pool2d(t if dt != torch.uint8 else t.half(), SIZE)
    return {"a_full_export_plus_torch_crop_pool": parent_route,
            "b_scaled_export": lambda: b.export_tensor("rgb", 5, 6, dtype=dt, crop=CROP, size=SIZE, out=small),
            "c_full_export_alone": lambda: b.export_tensor("rgb", 5, 6, dtype=dt, out=full)}


def scaled(n):
    b = resident(n)
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for dt in (torch.uint8, torch.float16):
        legs = scaled_legs(b, dt)
        if "--kernels" in sys.argv:
            for k in ("b_scaled_export", "c_full_export_alone"):
                for _ in range(10):
                    legs[k]()
            torch.cuda.synchronize()
        else:
            for f in legs.values():  # warm
                f()
            for rnd in range(2):
                for k, f in legs.items():
                    best = 1e30
                    for _ in range(3):
                        e0.record(s)
                        r = f()
                        e1.record(s)
                        e1.synchronize()
                        best = min(best, e0.elapsed_time(e1))
                    del r
                    print(json.dumps({"clips": n, "frames": 6, "crop": CROP, "size": SIZE, "dtype": str(dt).split(".")[-1], "round": rnd,
                                      "leg": k, "ms": round(best, 4)}), flush=True)
        del legs
        torch.cuda.empty_cache()
    b.close()


def random_boxes(n, seed=7):
    """n boxes of 8 - 100 % of the picture's area at aspect ratios 3:4 .. 4:3 (log-uniform), cut to the picture, and flips"""
    import numpy as np
    rng = np.random.default_rng(seed)
    boxes = []
    for _ in range(n):
        a, ar = rng.uniform(0.08, 1.0) * PX, np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
        w, h = min(W, int(round((a * ar) ** 0.5))), min(H, int(round((a / ar) ** 0.5)))
        boxes.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return boxes, [bool(v) for v in rng.integers(0, 2, n)]


def boxes_legs(b, n, dt):
    boxes, flips = random_boxes(n)
    full = b.export_tensor("rgb", 5, 6, dtype=dt)
    small = b.export_tensor("rgb", 5, 6, dtype=dt, crop=CROP, size=SIZE)

    def torch_route():  # what a caller does without the entry point: full size, then per clip crop, resize, flip
        t = b.export_tensor("rgb", 5, 6, dtype=dt, out=full)
        res = torch.empty((6, n, 3) + SIZE, dtype=torch.float16 if dt == torch.uint8 else dt, device=t.device)
        for c, ((x, y, w, h), fl) in enumerate(zip(boxes, flips)):
            v = t[:, c, :, y:y + h, x:x + w]
            v = v.half() if dt == torch.uint8 else v
            # (one mode per clip, as a loader's resize has: area where the box is no smaller than the output, bilinear otherwise)
            r = (torch.nn.functional.interpolate(v, size=SIZE, mode="area") if w >= SIZE[1] and h >= SIZE[0]
                 else torch.nn.functional.interpolate(v, size=SIZE, mode="bilinear", align_corners=False))
            res[:, c] = torch.flip(r, (3,)) if fl else r
        return res
    return {"a_full_export_plus_torch_per_clip_loop": torch_route,
            "b_boxes_export_random": lambda: b.export_tensor("rgb", 5, 6, dtype=dt, boxes=boxes, flip=flips, size=SIZE, out=small),
            "c_boxes_export_centre": lambda: b.export_tensor("rgb", 5, 6, dtype=dt, boxes=[CROP] * n, size=SIZE, out=small),
            "d_scaled_export_centre": lambda: b.export_tensor("rgb", 5, 6, dtype=dt, crop=CROP, size=SIZE, out=small)}


def boxes_run():
    n = 512  # (not larger: DESIGN.md, "Scaled export", records an unexplained memory fault of the 4096-clip run)
    b = resident(n)
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for dt in (torch.uint8, torch.float16):
        legs = boxes_legs(b, n, dt)
        if "--kernels" in sys.argv:
            for k in ("b_boxes_export_random", "c_boxes_export_centre", "d_scaled_export_centre"):
                for _ in range(10):
                    legs[k]()
            torch.cuda.synchronize()
        else:
            for f in legs.values():  # warm
                f()
            for rnd in range(2):
                for k, f in legs.items():
                    best = 1e30
                    for _ in range(3):
                        e0.record(s)
                        r = f()
                        e1.record(s)
                        e1.synchronize()
                        best = min(best, e0.elapsed_time(e1))
                    del r
                    print(json.dumps({"clips": n, "frames": 6, "size": SIZE, "dtype": str(dt).split(".")[-1], "round": rnd, "leg": k,
                                      "ms": round(best, 4)}), flush=True)
        del legs
        torch.cuda.empty_cache()
    b.close()


def scaled_e2e():
    S = streams(32 * 3, iframe_interval=32)
    for rnd in range(2):
        for mode in ("decode", "u8", "u8_scaled", "f16", "f16_scaled"):
            g = end_to_end(mode, S=S)
            print(json.dumps({"round": rnd, "mode": mode, "clips": 4096, "group": 32, "gpix_s": round(g, 2)}), flush=True)


def nt_ab():
    for n, nf in ((64, 1), (512, 6)):
        b = resident(n)
        for dt in (torch.uint8, torch.float16):
            out = b.export_tensor("rgb", nf - 1, nf, dtype=dt)
            s = torch.cuda.current_stream()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for rnd in range(3):
                for nt in ("0", "1"):
                    os.environ["MOBI_EXPORT_RGB_NT"] = nt
                    best = 1e30
                    for _ in range(6):
                        e0.record(s)
                        b.export_tensor("rgb", nf - 1, nf, dtype=dt, out=out)
                        tot = out.sum(dtype=torch.float32 if dt != torch.uint8 else torch.int64)  # the consumer, right behind
                        e1.record(s)
                        e1.synchronize()
                        best = min(best, e0.elapsed_time(e1))
                    del tot
                    print(json.dumps({"clips": n, "frames": nf, "dtype": str(dt).split(".")[-1], "round": rnd, "nontemporal": int(nt),
                                      "export_plus_consumer_ms": round(best, 4)}), flush=True)
            del out
        b.close()
        torch.cuda.empty_cache()


def main():
    if "--from-stats" in sys.argv:
        from_stats(sys.argv[sys.argv.index("--from-stats") + 1])
    elif "--boxes" in sys.argv:
        boxes_run()
    elif "--scaled" in sys.argv:
        if "--e2e" in sys.argv:
            scaled_e2e()
        else:
            scaled(int(sys.argv[sys.argv.index("--clips") + 1]) if "--clips" in sys.argv else 512)
    elif "--kernels" in sys.argv:
        kernels()
    elif "--e2e" in sys.argv:
        e2e()
    elif "--nt" in sys.argv:
        assert "--prof" in sys.argv, "--nt switches MOBI_EXPORT_RGB_NT, which only the profiling twin reads"
        nt_ab()
    else:
        rates()


if __name__ == "__main__":
    main()
