#!/usr/bin/env python3
"""Throughput of the encoder's transform coding on one GPU (mobi_transform_code_async on device-resident torch buffers, outputs allocated
once, torch's current stream, warm-up, HIP-event timing over `--iters` calls); prints ONE JSON line.

  (a) one quantiser (24), every output: blocks/s and the share of 8 TB/s that the algorithmic bytes reach -- per entry src + pred + levels
      + recon + bits + sad + flags = 329 B for 8x8, 89 B for 4x4
  (b) the rate-control sweep, 29 quantisers (12..40, the range EncodePrediction clamps to), bits and flags only: blocks/s, entries/s
Blocks: 4 Mi 8x8 and 4 Mi 4x4 (--blocks), "natural" (random prediction, residual of a few levels) so that most blocks code something.
For `rocprofv3 --kernel-trace --stats -- python tools/exp_txcode.py` the kernels are mobi_txcode8 / mobi_txcode4.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mobiclipdecoder_amd as m  # noqa: E402

HBM = 8.0e12


def blocks(nb, nn, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    pred = torch.randint(0, 256, (nb, nn), device=dev, generator=g, dtype=torch.int32)
    res = torch.randint(-12, 13, (nb, nn), device=dev, generator=g, dtype=torch.int32)
    return (pred + res).clamp(0, 255).to(torch.uint8), pred.to(torch.uint8)


def run(lib, n, src, pred, qs, outs, iters, warmup):
    dev = src.device
    nb = src.shape[0]
    qa = (C.c_int * len(qs))(*qs)
    s = torch.cuda.current_stream(dev)
    ptr = {k: (v.data_ptr() if v is not None else None) for k, v in outs.items()}

    def call():
        rc = lib.mobi_transform_code_async(dev.index, s.cuda_stream, n, qa, len(qs), src.data_ptr(), pred.data_ptr(), nb, ptr["levels"],
                                           ptr["recon"], ptr["bits"], ptr["sad"], ptr["flags"])
        assert rc == 0, rc

    for _ in range(warmup):
        call()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(iters):
        call()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1 << 22)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    lib = m.load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"blocks": a.blocks, "iters": a.iters}
    for n in (8, 4):
        nn = n * n
        src, pred = blocks(a.blocks, nn, dev)
        one = {"levels": torch.empty((a.blocks, nn), dtype=torch.int16, device=dev), "recon": torch.empty((a.blocks, nn), dtype=torch.uint8, device=dev),
               "bits": torch.empty(a.blocks, dtype=torch.int32, device=dev), "sad": torch.empty(a.blocks, dtype=torch.int32, device=dev),
               "flags": torch.empty(a.blocks, dtype=torch.uint8, device=dev)}
        t = run(lib, n, src, pred, [24], one, a.iters, a.warmup)
        per = 2 * nn + 2 * nn + nn + 9
        res[f"a_{n}x{n}_ms"] = t * 1e3
        res[f"a_{n}x{n}_blocks_per_s"] = a.blocks / t
        res[f"a_{n}x{n}_bytes_per_entry"] = per
        res[f"a_{n}x{n}_tb_s"] = a.blocks * per / t / 1e12
        res[f"a_{n}x{n}_frac_8tbs"] = a.blocks * per / t / HBM
        res[f"a_{n}x{n}_coded_frac"] = float((one["flags"] & 1).float().mean())
        del one
        qs = list(range(12, 41))
        sweep = {"levels": None, "recon": None, "sad": None, "bits": torch.empty((len(qs), a.blocks), dtype=torch.int32, device=dev),
                 "flags": torch.empty((len(qs), a.blocks), dtype=torch.uint8, device=dev)}
        t = run(lib, n, src, pred, qs, sweep, max(1, a.iters // 4), a.warmup)
        res[f"b_{n}x{n}_ms"] = t * 1e3
        res[f"b_{n}x{n}_blocks_per_s"] = a.blocks / t
        res[f"b_{n}x{n}_entries_per_s"] = a.blocks * len(qs) / t
        res[f"b_{n}x{n}_tb_s"] = (a.blocks * 2 * nn + a.blocks * len(qs) * 5) / t / 1e12
        del sweep, src, pred
        torch.cuda.empty_cache()
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) and v < 1e6 else (float("%.4g" % v) if isinstance(v, float) else v)) for k, v in res.items()}),
          flush=True)


if __name__ == "__main__":
    main()
