#!/usr/bin/env python3
"""Continuous batching over a fixed batch (mobi_batch_reset_clips): clips of different lengths, refilled as they end.

4096 Moflex3DS 640x480 clips, each a stream of 12..96 frames (a prefix of one of --pool generated streams: every one starts with an
I-frame).  Pipelined groups of K = 6 frames (gop_begin(g + 1) before gop_finish(g)).  A clip whose stream ends inside a group decodes empty
packets for the rest of it -- or, with --idle, has those slots marked idle (mobi_batch_set_idle: not parsed, not handed to the host parser;
same seed, same streams, same resets) --; before the next group is begun it is reset and handed its next stream.  Reported: Gpixels/s
of live frames, the share of idle frame slots, the host time of the reset calls; --equal feeds every clip streams of one length, a
multiple of K (no idle slot; every clip is reset at the same boundaries).  The kernel's time comes from a rocprofv3 --kernel-trace --stats
run of this script (mobi_reset_state in its stats).

  python tools/exp_refill.py [--clips 4096] [--groups 40] [--equal] [--idle] [--label NAME] [--out profiles/refill_runs.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobiclipdecoder_amd import MobiclipBatch, default_params, generate_clip  # noqa: E402
from mobiclipdecoder_amd.streamgen import BASE_SEED  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--groups", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--min-len", type=int, default=12)
    ap.add_argument("--max-len", type=int, default=96)
    ap.add_argument("--equal", action="store_true", help="every stream --equal-len frames long")
    ap.add_argument("--equal-len", type=int, default=54)
    ap.add_argument("--idle", action="store_true", help="mark the ended clips' slots idle instead of feeding them empty packets")
    ap.add_argument("--label", default=None, help="copied into the result line (which build, which leg)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H, n, K = 640, 480, a.clips, a.k
    pool = []
    for i in range(a.pool):
        d, fo = generate_clip(default_params("B", BASE_SEED + 41000 + i, n_frames=a.max_len))
        pool.append([d[fo[f]:fo[f + 1]] for f in range(a.max_len)])
    rng = np.random.default_rng(7)
    empty = np.zeros(0, np.uint8)

    def new_len():
        return a.equal_len if a.equal else int(rng.integers(a.min_len, a.max_len + 1))

    src = rng.integers(0, a.pool, n)  # the pool stream each clip plays, how long, and how far it is
    length = np.array([new_len() for _ in range(n)])
    pos = np.zeros(n, np.int64)
    b = MobiclipBatch(n, W, H, 2, device_parse=True)
    live_frames = idle_slots = 0
    reset_ms, reset_calls, reset_clips, max_reset = 0.0, 0, 0, 0
    pending = 0

    def group():
        """the next K frames of every clip; clips whose stream ends are reset and refilled BEFORE this group (their next stream starts here)"""
        nonlocal live_frames, idle_slots, reset_ms, reset_calls, reset_clips, max_reset
        ended = np.flatnonzero(pos >= length)
        if ended.size:
            t0 = time.perf_counter()
            b.reset_clips(ended)
            reset_ms += (time.perf_counter() - t0) * 1e3
            reset_calls += 1
            reset_clips += int(ended.size)
            max_reset = max(max_reset, int(ended.size))
            src[ended] = rng.integers(0, a.pool, ended.size)
            length[ended] = [new_len() for _ in range(ended.size)]
            pos[ended] = 0
        frames = []
        if a.idle:
            mask = pos[None, :] + np.arange(K)[:, None] >= length[None, :]
            if mask.any():
                b.set_idle(mask)
        for k in range(K):
            row = []
            for c in range(n):
                f = pos[c] + k
                if f < length[c]:
                    row.append(pool[src[c]][f])
                    live_frames += 1
                else:
                    row.append(None if a.idle else empty)
                    idle_slots += 1
            frames.append(row)
        pos[:] = np.minimum(pos + K, length)
        return frames

    def finish():
        nonlocal pending
        while b.gop_frames_pending():
            b.gop_finish()
        pending -= 1

    for g in range(a.warmup):
        b.gop_begin(group())
        pending += 1
        if pending == 2:
            finish()
    live_frames = idle_slots = 0
    reset_ms, reset_calls, reset_clips, max_reset = 0.0, 0, 0, 0
    t0 = time.perf_counter()
    for g in range(a.groups):
        b.gop_begin(group())
        pending += 1
        if pending == 2:
            finish()
    while pending:
        finish()
    dt = time.perf_counter() - t0
    host_clips_end = b.host_clips()
    b_idle_launches = b.idle_launches() if hasattr(b, "idle_launches") else None
    b.close()
    out = {"label": a.label, "idle_mask": a.idle, "idle_launches": b_idle_launches, "host_clips_end": host_clips_end, "clips": n, "K": K, "groups": a.groups, "equal": a.equal, "lengths": [a.equal_len] * 2 if a.equal else [a.min_len, a.max_len],
           "live_gpixels_s": round(live_frames * W * H / dt / 1e9, 3), "frame_slots_s": round((live_frames + idle_slots) / dt, 1),
           "idle_share": round(idle_slots / max(1, live_frames + idle_slots), 4), "wall_s": round(dt, 3),
           "reset_calls": reset_calls, "reset_clips": reset_clips, "max_clips_per_reset": max_reset,
           "reset_host_ms_total": round(reset_ms, 3), "reset_host_us_per_call": round(1e3 * reset_ms / max(1, reset_calls), 2)}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
