#!/usr/bin/env python3
"""What the clip sink and mobi_batch_gop_finish_all buy, one process, one GPU; prints JSON lines and writes profiles/sink_exp.json.

  clip_tensor    512 clips of 640x480, groups of 32 frames, a random box and flip per clip -> 224x224, T = 8, stride 4, "ncthw", uint8 and
                 float16; wall ms per group from gop_begin's return to the tensor, the arms alternating in one process on the same group:
                   parts  gop_finish six at a time, export_tensor(boxes=...) of each part, the selected frames picked and permuted with
                          torch into the (N, 3, T, 224, 224) tensor (what a loader did before the sink);
                   sink   set_sink + gop_finish_all.
                 Both arms end with a torch.cuda.synchronize(): the tensor is there.
  finish_all     4096 clips x 32 frames, no sink: ms per frame step six at a time against gop_finish_all, interleaved.
  --kernels      one group per arm and dtype only (for `rocprofv3 --kernel-trace --stats -- python tools/exp_sink.py --kernels`: the sums
                 of kernel times, and mobi_sink beside mobi_export_resample per picture)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mobiclipdecoder_amd as m  # noqa: E402
from mobiclipdecoder_amd import sharding  # noqa: E402

W, H, VER, G = 640, 480, 2, 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def streams(n_frames, distinct=8):
    out = []
    for i in range(distinct):
        data, fo = m.generate_clip(m.default_params("B", sharding.stream_seed("B", 0, i), n_frames=n_frames, iframe_interval=G))
        out.append([data[fo[f]:fo[f + 1]] for f in range(n_frames)])
    return out


def group_of(S, n, g):
    return [[S[c % len(S)][k] for c in range(n)] for k in range(g * G, (g + 1) * G)]


def random_boxes(n, rng):
    """RandomResizedCrop's boxes: 8 % .. 100 % of the area, aspect 3/4 .. 4/3"""
    boxes = []
    while len(boxes) < n:
        area = rng.uniform(0.08, 1.0) * W * H
        ar = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
        w, h = int(round(np.sqrt(area * ar))), int(round(np.sqrt(area / ar)))
        if 0 < w <= W and 0 < h <= H:
            boxes.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return np.array(boxes), rng.integers(0, 2, n).astype(bool)


def finish_parts(b, n, boxes, flips, dtype, T, s, size):
    """the loader's way before the sink: every part exported whole, the frames of the schedule picked, one permute at the end"""
    keep, k0 = [], 0
    while True:
        rcs, _ = b.gop_finish()
        P = len(rcs)
        if boxes is not None:
            part = b.export_tensor("rgb", P - 1, P, boxes=boxes, flip=flips, size=size, dtype=dtype)  # (P, N, 3, h, w)
            keep += [part[k - k0] for k in range(k0, k0 + P) if k % s == 0 and k // s < T]
        k0 += P
        if b.gop_frames_pending() in (0, G):
            break
    if boxes is None:
        return None
    return torch.stack(keep, 2).contiguous()  # (N, 3, T, h, w)


def clip_tensor(n=512, T=8, s=4, size=(224, 224), rounds=3, kernels=False):
    """one group in flight at a time (a sink is armed with nothing in flight); every arm decodes the same group again, after a reset of every clip"""
    S = streams(G * 2)
    rng = np.random.default_rng(7)
    boxes, flips = random_boxes(n, rng)
    res = []
    for dtype in (torch.uint8, torch.float16):
        b = m.MobiclipBatch(n, W, H, VER, device_parse=True)
        b.gop_begin(group_of(S, n, 0))
        finish_parts(b, n, None, None, dtype, T, s, size)  # untimed: allocations
        ms = {"parts": [], "sink": []}
        same = None
        for r in range(1 if kernels else rounds):
            outs = {}
            for arm in ("parts", "sink"):
                b.reset_clips(list(range(n)))  # every arm decodes the same group from its I-frame
                if arm == "sink":
                    out = b.set_sink(size=size, n_frames=T, stride=s, boxes=boxes, flip=flips, layout="ncthw", dtype=dtype)
                b.gop_begin(group_of(S, n, 0))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if arm == "parts":
                    out = finish_parts(b, n, boxes, flips, dtype, T, s, size)
                else:
                    b.gop_finish_all()
                torch.cuda.synchronize()
                ms[arm].append((time.perf_counter() - t0) * 1e3)
                outs[arm] = out
            same = bool(torch.equal(outs["parts"], outs["sink"]))
        b.close()
        res.append({"case": "clip_tensor", "n_clips": n, "T": T, "stride": s, "size": list(size), "dtype": str(dtype).split(".")[-1],
                    "ms_per_group": {k: [round(v, 3) for v in vs] for k, vs in ms.items()}, "median_ms": {k: round(float(np.median(vs)), 3) for k, vs in ms.items()},
                    "tensors_equal": same})
    return res


def finish_all(n=4096, rounds=3):
    S = streams(G * 2)
    b = m.MobiclipBatch(n, W, H, VER, device_parse=True)
    b.gop_begin(group_of(S, n, 0))
    finish_parts(b, n, None, None, None, 0, 1, None)
    ms = {"parts": [], "all": []}
    for r in range(rounds):
        for arm in ("parts", "all"):
            b.reset_clips(list(range(n)))
            b.gop_begin(group_of(S, n, 0))
            t0 = time.perf_counter()
            if arm == "parts":
                finish_parts(b, n, None, None, None, 0, 1, None)
            else:
                b.gop_finish_all()
            ms[arm].append((time.perf_counter() - t0) * 1e3 / G)
    b.close()
    return {"case": "finish_all", "n_clips": n, "frames": G, "ms_per_frame_step": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
            "median_ms": {k: round(float(np.median(vs)), 4) for k, vs in ms.items()}}


def main():
    kernels = "--kernels" in sys.argv
    res = clip_tensor(kernels=kernels)
    if not kernels:
        res.append(finish_all())
    for r in res:
        print(json.dumps(r), flush=True)
    if not kernels:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "sink_exp.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
