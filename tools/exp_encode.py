#!/usr/bin/env python3
"""Throughput of the intra encoder on one GPU (mobi_enc_intra_async on device-resident torch buffers, everything allocated once, torch's
current stream, warm-up, HIP-event timing over `--iters` calls); prints ONE JSON line and, with --out, writes it to a file.

  pictures   640x480, half of them decoded frames of a generated clip (streamgen class "B"), half synthetic ramps with a little noise,
             repeated to N.  CONTENT MATTERS: bits, coded blocks and with them stage 2's time follow the pictures and the quantiser, and
             no real media exists in this repository -- read the rates as those of this synthetic mix, not of a film.
  per N in (512, 4096) and q in (26, 40):  stage 1 (decide and reconstruct) and stage 2 (scan + write bits) each timed alone by HIP events,
             the whole call, pictures/s and Gpixels/s of the whole call, bytes per picture, coded blocks per picture
  host       the same 512 pictures through the host model (tests/tools/mobi_encode_host.cpp) on 16 threads of the same machine
  shapes     stage 1 as one launch per diagonal (0, the product's) and as one workgroup per picture with a barrier between diagonals
             (1, in the profiling twin only), at N = 8, 512 and 4096, q = 26, one after the other; both must give the same bytes
The stage / shape switch is a hook of the profiling twin (libmobiclip_hip_prof.so, mobi_debug_enc_select), which this tool loads.
For `rocprofv3 --kernel-trace --stats -- python tools/exp_encode.py` the kernels are mobi_enc_decide_loop / mobi_enc_decide_diag /
mobi_enc_scan / mobi_enc_write.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MOBI_LIB", os.path.join(ROOT, "mobiclipdecoder_amd", "libmobiclip_hip_prof.so"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mobiclipdecoder_amd as m  # noqa: E402
from mobiclipdecoder_amd import encode  # noqa: E402

W, H = 640, 480


def pictures(n_distinct, dev):
    """(n_distinct, frame) uint8 on the device: decoded generated frames and ramps, alternating"""
    p = m.default_params("B", 4242, n_frames=n_distinct // 2)
    assert (p.width, p.height) == (W, H)
    data, fo = m.generate_clip(p)
    dec = m.MobiclipBatch(1, W, H, p.version)
    out = []
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = np.mgrid[0:H // 2, 0:W // 2]
    rng = np.random.default_rng(5)
    for f in range(p.n_frames):
        rcs, _ = dec.decode([data[fo[f]:fo[f + 1]]], [0])
        assert rcs == [0]
        out.append(dec.export_tensor("i420")[0, 0].clone())
        ramp = np.concatenate([((xx * (1 + f % 3) + yy * (2 + f % 2)) // 3 % 256 + rng.integers(-2, 3, (H, W))).clip(0, 255).ravel(),
                               ((cx + 3 * f) % 256).ravel(), ((cy * 2 + f) % 256).ravel()]).astype(np.uint8)
        out.append(torch.from_numpy(ramp).to(dev))
    torch.cuda.synchronize(dev)
    dec.close()
    return torch.stack(out), p.version


def timed(call, s, iters, warmup):
    for _ in range(warmup):
        call()
    s.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(iters):
        call()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--quantizers", type=int, nargs="+", default=[26, 40])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-pictures", type=int, default=512)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = encode._lib()
    select = lib.mobi_debug_enc_select  # (stages: 1 decide, 2 scan, 4 write, 7 all; shape: 0 launch per diagonal, 1 barrier loop)
    select.argtypes, select.restype = [C.c_int, C.c_int], None
    dev = torch.device("cuda", torch.cuda.current_device())
    s = torch.cuda.current_stream(dev)
    base, version = pictures(16, dev)
    frame = base.shape[1]
    res = {"width": W, "height": H, "iters": a.iters, "content": "decoded streamgen class B frames + noisy ramps, 16 distinct, repeated"}
    nmax = max(a.counts + [512])
    enc = m.MobiclipIntraEncoder(W, H, version, nmax)
    src = base.repeat((nmax + base.shape[0] - 1) // base.shape[0], 1)[:nmax].contiguous()
    slot = 96 * 1024  # measured below: no stream of this mix comes near it
    out = torch.empty((nmax, slot), dtype=torch.uint8, device=dev)
    sizes = torch.empty(nmax, dtype=torch.int32, device=dev)
    stats = torch.empty((nmax, 64), dtype=torch.uint8, device=dev)

    def call(n, q):
        qs = np.full(n, q, np.uint8)
        rc = lib.mobi_enc_intra_async(enc._h, s.cuda_stream, n, src.data_ptr(), frame, qs.ctypes.data, 0, out.data_ptr(), slot, sizes.data_ptr(), None,
                                      stats.data_ptr())
        assert rc == 0, rc

    default_shape = 0
    for n in a.counts:
        for q in a.quantizers:
            k = f"n{n}_q{q}"
            select(7, default_shape)
            whole = timed(lambda: call(n, q), s, a.iters, a.warmup)
            sz = sizes[:n].cpu().numpy()
            st = stats[:n].cpu().numpy().view(encode.STATS_DTYPE).reshape(-1)
            assert sz.max() <= slot
            select(1, default_shape)
            t1 = timed(lambda: call(n, q), s, a.iters, 1)
            select(6, default_shape)
            t2 = timed(lambda: call(n, q), s, a.iters, 1)
            res[k] = {"whole_ms": whole, "stage1_ms": t1, "stage2_ms": t2, "pictures_per_s": n / whole * 1e3, "gpixels_per_s": n * W * H / whole / 1e6,
                      "bytes_per_picture": float(sz.mean()), "coded_blocks_per_picture": float(st["coded_blocks"].mean()),
                      "fallback_blocks_per_picture": float(st["fallback_clamp"].mean())}
    # the two stage-1 shapes
    for n in (8, 512, max(a.counts)):
        got = {}
        for shape in (0, 1):
            select(7, shape)
            call(n, 26)
            s.synchronize()
            got[shape] = (out[:n].cpu().numpy().copy(), sizes[:n].cpu().numpy().copy())
            select(1, shape)
            res[f"{('diag', 'loop')[shape]}_n{n}_stage1_ms"] = timed(lambda: call(n, 26), s, a.iters * (4 if n == 8 else 1), 2)
        res[f"shapes_agree_n{n}"] = bool(np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]))
    select(7, default_shape)
    # the host model on the same pictures
    sys.path.insert(0, ROOT)
    from tests import enc_model as E
    hp = src[: a.host_pictures].cpu().numpy()
    for q in a.quantizers:
        t0 = time.perf_counter()
        r = E.host_encode(W, H, version, hp, np.full(len(hp), q, np.uint8), slot_bytes=slot, threads=a.host_threads)
        dt = time.perf_counter() - t0
        call(len(hp), q)
        s.synchronize()
        res[f"host_n{len(hp)}_q{q}"] = {"threads": a.host_threads, "ms": dt * 1e3, "pictures_per_s": len(hp) / dt,
                                         "equals_gpu": bool(np.array_equal(r["streams"], out[: len(hp)].cpu().numpy()))}
    enc.close()
    line = json.dumps(json.loads(json.dumps(res), parse_float=lambda x: round(float(x), 4)))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
