#!/usr/bin/env python3
"""What rate control costs and buys on one GPU (include/mobiclip_encode_rate.h): the _target_async calls on device-resident torch buffers,
everything allocated once, torch's current stream, warm-up, HIP-event timing over `--iters` calls; prints ONE JSON line and, with --out,
writes it to a file.  Pictures: tools/exp_encode_inter.py's synthetic 640x480 `translated` mix (16 distinct pairs repeated) -- read the
figures as those of that mix.

  default     per encoder (intra, inter in mode 0 and mode 1), N in --counts, ranges 12..52 (six rounds) and 24..31 (three):
                fixed_ms     the fixed-quantiser call at --quantizer          write_ms   its bit writer alone (profiling twin's stage switch)
                target_ms    the target call, every picture's target the bytes it takes at --quantizer
                expected_ms  (K + 1) x (fixed - write) + write: K trials without the writer, one whole encode
                bytes per picture against the target, the share of pictures within their target, the mean chosen quantiser
              and encode_clips(target_bytes=) against the same clips driven by a bisection ON THE HOST: one encode() and one
              sizes.cpu() per trial (in this tool only) -- wall-clock, what staying on the device buys
  --fixed-ab  only the fixed-quantiser calls of whatever library MOBI_LIB names (the product library of this or of another commit), for
              a job that alternates two builds: one JSON line with "lib" in it
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
if "--fixed-ab" in sys.argv:
    os.environ.setdefault("MOBI_LIB", os.path.join(ROOT, "mobiclipdecoder_amd", "libmobiclip_hip.so"))
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from exp_encode_inter import H, VERSION, W, pairs, timed  # noqa: E402  (sets MOBI_LIB to the profiling twin unless it is set)
import mobiclipdecoder_amd as m  # noqa: E402
from mobiclipdecoder_amd import encode, encode_inter  # noqa: E402

FRAME = W * H * 3 // 2
SLOT = 256 * 1024  # checked: no stream of this mix is longer
KINDS = ("intra", "inter", "inter_parts")


class Bench:
    """the buffers of every call, made once for nmax pictures; pictures, references (the intra encoder's reconstruction of the frame before)"""

    def __init__(self, nmax, q, dev):
        self.dev, self.s, self.q = dev, torch.cuda.current_stream(dev), q
        prev, cur = pairs("translated", np.random.default_rng(77))
        reps = (nmax + 15) // 16
        self.src = torch.from_numpy(cur).to(dev).repeat(reps, 1)[:nmax].contiguous()
        before = torch.from_numpy(prev).to(dev).repeat(reps, 1)[:nmax].contiguous()
        self.ref = torch.empty((nmax, FRAME), dtype=torch.uint8, device=dev)
        self.out = torch.empty((nmax, SLOT), dtype=torch.uint8, device=dev)
        self.sizes = torch.empty(nmax, dtype=torch.int32, device=dev)
        self.qout = torch.empty(nmax, dtype=torch.uint8, device=dev)
        self.prev_q = torch.full((nmax,), q, dtype=torch.uint8, device=dev)
        self.target = torch.empty(nmax, dtype=torch.int32, device=dev)
        self.qs = np.full(nmax, q, np.uint8)
        self.ienc = m.MobiclipIntraEncoder(W, H, VERSION, nmax)
        self.penc = m.MobiclipInterEncoder(W, H, VERSION, nmax)
        self.ilib, self.plib = encode._lib(), encode_inter._lib()
        rc = self.ilib.mobi_enc_intra_async(self.ienc._h, self.s.cuda_stream, nmax, before.data_ptr(), FRAME, self.qs.ctypes.data, 0, self.out.data_ptr(), SLOT,
                                            self.sizes.data_ptr(), self.ref.data_ptr(), None)
        assert rc == 0, rc
        self.s.synchronize()

    def fixed(self, kind, n):
        if kind == "intra":
            rc = self.ilib.mobi_enc_intra_async(self.ienc._h, self.s.cuda_stream, n, self.src.data_ptr(), FRAME, self.qs.ctypes.data, 0, self.out.data_ptr(), SLOT,
                                                self.sizes.data_ptr(), None, None)
        else:
            rc = self.plib.mobi_enc_inter_async(self.penc._h, self.s.cuda_stream, n, self.src.data_ptr(), FRAME, self.ref.data_ptr(), FRAME, self.qs.ctypes.data,
                                                self.qs.ctypes.data, self.out.data_ptr(), SLOT, self.sizes.data_ptr(), None, None)
        assert rc == 0, rc

    def target_call(self, kind, n, qmin, qmax):
        from mobiclipdecoder_amd import encode_rate
        lib = encode_rate._lib()
        if kind == "intra":
            rc = lib.mobi_enc_intra_target_async(self.ienc._h, self.s.cuda_stream, n, self.src.data_ptr(), FRAME, self.target.data_ptr(), qmin, qmax, 0, self.out.data_ptr(),
                                                 SLOT, self.sizes.data_ptr(), None, None, self.qout.data_ptr())
        else:
            rc = lib.mobi_enc_inter_target_async(self.penc._h, self.s.cuda_stream, n, self.src.data_ptr(), FRAME, self.ref.data_ptr(), FRAME, self.prev_q.data_ptr(),
                                                 self.target.data_ptr(), qmin, qmax, self.out.data_ptr(), SLOT, self.sizes.data_ptr(), None, None, self.qout.data_ptr())
        assert rc == 0, rc

    def mode(self, kind):
        self.penc.set_partitions(kind == "inter_parts")


def host_bisect_clips(frames, targets, gop, qmin, qmax):
    """encode_clips(target_bytes=) with the rule driven from the host: per frame and round one encode() of every clip at its own trial
    quantiser and one sizes.cpu() -- the round trip the device-side loop does not make; everything else as encode_clips does it"""
    from mobiclipdecoder_amd import encode_rate
    n, t_n = int(frames.shape[0]), int(frames.shape[1])
    intra, inter = m.MobiclipIntraEncoder(W, H, VERSION, n), m.MobiclipInterEncoder(W, H, VERSION, n)
    slot = max(intra.stream_bound, inter.stream_bound)
    ref, prev, held = None, None, []
    for t in range(t_n):
        pics = frames[:, t].contiguous()
        enc = (lambda q: intra.encode(pics, q, recon=True, slot_bytes=slot)) if t % gop == 0 else (lambda q: inter.encode(pics, ref, prev, q, recon=True, slot_bytes=slot))
        lo, hi = np.full(n, qmin), np.full(n, qmax)
        for _ in range(encode_rate.rate_rounds(qmin, qmax)):
            mid = (lo + hi) >> 1
            fits = enc(mid)[1].cpu().numpy() <= targets[t]
            lo, hi = np.where(fits, lo, np.minimum(mid + 1, hi)), np.where(fits, mid, hi)
        out, sizes, ex = enc(lo)
        ref, prev = ex["recon"], lo
        held.append((out, sizes))
    torch.cuda.current_stream(frames.device).synchronize()
    intra.close()
    inter.close()
    clips = [[] for _ in range(n)]  # the streams to the host as encode_clips brings them
    for out, sizes in held:
        out, sizes = out.cpu().numpy(), sizes.cpu().numpy()
        for i in range(n):
            clips[i].append(out[i, :sizes[i]].tobytes())
    return clips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--quantizer", type=int, default=30)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", type=int, nargs="+", default=[4, 64])
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--fixed-ab", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    nmax = max(a.counts)
    b = Bench(nmax, a.quantizer, dev)
    res = {"width": W, "height": H, "iters": a.iters, "quantizer": a.quantizer, "lib": os.path.relpath(os.environ["MOBI_LIB"], ROOT),
           "content": "synthetic: exp_encode_inter.py's translated mix, 16 distinct pairs repeated"}
    if a.fixed_ab:
        for kind in KINDS:
            b.mode(kind)
            for n in a.counts:
                res[f"{kind}_n{n}_fixed_ms"] = timed(lambda: b.fixed(kind, n), b.s, a.iters, a.warmup)
    else:
        isel, psel = b.ilib.mobi_debug_enc_select, b.plib.mobi_debug_encp_select  # all stages: 7 / 15; the bit writer alone: 4 / 8
        isel.argtypes, isel.restype, psel.argtypes, psel.restype = [C.c_int, C.c_int], None, [C.c_int], None
        for kind in KINDS:
            b.mode(kind)
            for n in a.counts:
                fixed = timed(lambda: b.fixed(kind, n), b.s, a.iters, a.warmup)
                b.target[:n] = b.sizes[:n]  # every picture's target: what it takes at --quantizer
                want = float(b.sizes[:n].float().mean().item())
                isel(4, 0) if kind == "intra" else psel(8)
                write = timed(lambda: b.fixed(kind, n), b.s, a.iters, 1)
                isel(7, 0) if kind == "intra" else psel(15)
                for qmin, qmax, k in ((12, 52, 6), (24, 31, 3)):
                    ms = timed(lambda: b.target_call(kind, n, qmin, qmax), b.s, a.iters, a.warmup)
                    sz, q, tg = b.sizes[:n].cpu().numpy(), b.qout[:n].cpu().numpy(), b.target[:n].cpu().numpy()
                    assert sz.max() <= SLOT
                    res[f"{kind}_n{n}_k{k}"] = {"fixed_ms": fixed, "write_ms": write, "target_ms": ms, "expected_ms": (k + 1) * (fixed - write) + write,
                                                "target_over_fixed": ms / fixed, "target_bytes_per_picture": want, "bytes_per_picture": float(sz.mean()),
                                                "within_target": float((sz <= tg).mean()), "at_qmax": float((q == qmax).mean()), "mean_quantizer": float(q.mean())}
                    print("done", kind, n, k, file=sys.stderr, flush=True)
        b.mode("inter")
        # whole clips: the device-side loop against a host-driven one
        t_n, gop = a.frames, a.frames
        per_frame = int(b.sizes[:16].float().mean().item())
        for n in a.clips:
            frames = torch.stack([b.src[(torch.arange(n, device=dev) + t) % nmax] for t in range(t_n)], 1).contiguous()
            got = {}
            for name, run in (("device", lambda: m.encode_clips(frames, None, gop, VERSION, W, H, target_bytes=per_frame)),
                              ("host", lambda: host_bisect_clips(frames, [per_frame] * t_n, gop, 12, 52))):
                run()  # warm-up: the allocator, the first launches
                ms = []
                for _ in range(a.iters):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got[name] = run()
                    ms.append((time.perf_counter() - t0) * 1e3)
                res[f"clips{n}_{name}_ms"] = sorted(ms)[len(ms) // 2]
            res[f"clips{n}_same_streams"] = got["device"] == got["host"]
            res[f"clips{n}_bytes_per_frame"] = sum(len(s) for c in got["device"] for s in c) / (n * t_n)
        res.update(clip_frames=t_n, clip_target_bytes=per_frame)
    line = json.dumps(json.loads(json.dumps(res), parse_float=lambda x: round(float(x), 4)))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a" if a.fixed_ab else "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
