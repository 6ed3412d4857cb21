#!/usr/bin/env python3
"""Throughput of the inter encoder on one GPU (mobi_enc_inter_async on device-resident torch buffers, everything allocated once, torch's
current stream, warm-up, HIP-event timing over `--iters` calls); prints ONE JSON line and, with --out, writes it to a file.

  pictures   640x480, SYNTHETIC, 16 distinct (picture, reference) pairs repeated to N, two mixes:
               translated  a random texture of softened 8x8 cells moved by whole and half samples (vectors up to 16 half-pels, every phase) with a little
                           noise on top; the reference is the intra encoder's reconstruction of the frame before at the same quantiser
               noisy       the same with strong noise on every frame: the search finds little, the residual is large
             CONTENT MATTERS: vectors, bits and coded blocks follow the pictures and the quantiser, and no real media exists in this
               two_motion  the translated mix with every picture cut into 32x32 tiles in checkerboard order, the tiles' corners at
                           8 mod 16, the two colours moved by different vectors: every other macroblock straddles two motions
             repository -- read the rates as those of these mixes, not of a film.
  per mix, N in (512, 4096) and q in (26, 40):  search, code and write (scan + bits) each timed alone by HIP events, the whole call,
             pictures/s, bytes per picture, macroblocks by vector kind; beside it the INTRA encoder's whole call on the same pictures
  host       the first `--host-pictures` pairs through the host model (tests/tools/mobi_encode_inter_host.cpp) on 16 threads of the
             same machine; its streams must equal the GPU's (equals_gpu)
  --partitions  every configuration twice, side by side: mode 0 (keys as without the switch) and mode 1 (keys + "_parts": partitions
             down to 8x8, include/mobiclip_encode_parts.h), with the share of split macroblocks, the leaves per picture and the search's
             time as a multiple of mode 0's; the host model is then tests/tools/mobi_encode_parts_host.cpp
  --intra    every configuration also in the intra mode (keys + "_pintra": include/mobiclip_encode_pintra.h), with the share of macroblocks
             sent intra and the two stages the mode adds, decide (one launch per anti-diagonal: mbw + mbh - 1 = 69 here) and finish,
             timed alone.  The mix `cut` is made for it: the translated pictures against the reconstruction of an UNRELATED texture, so
             that no macroblock's inter cost is small enough to skip the trials; on `translated` most macroblocks skip them
The stage switch is a hook of the profiling twin (libmobiclip_hip_prof.so, mobi_debug_encp_select), which this tool loads.
For `rocprofv3 --kernel-trace --stats` or `--pmc` runs (--no-host --counts 512 --quantizers 26) the kernels are mobi_encp_search /
mobi_encp_code / mobi_encp_scan / mobi_encp_write (mode 1: mobi_encq_*).
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
from mobiclipdecoder_amd import encode, encode_inter  # noqa: E402

W, H, VERSION = 640, 480, 2
MOVES = [(0, 0), (2, 0), (0, 2), (-4, 6), (1, 0), (0, 1), (1, 1), (-3, 5), (16, -16), (-16, 8), (7, -9), (12, 3), (-1, -1), (6, 6), (-10, 0), (3, -14)]  # half-pels


def pairs(mix, rng):
    """16 (previous frame, frame) pairs as (16, frame) uint8 arrays: frame = the previous one moved by MOVES[i] half-pels"""
    M2 = 24
    if mix == "cut":  # the translated pictures; the frames before them show another texture
        return pairs("translated", np.random.default_rng(1077))[0], pairs("translated", rng)[1]
    def texture(h, w, lo, hi, blur):  # 8x8 cells of random grey, softened: edges stay, an I-frame of it fits the slots below
        a = rng.integers(lo, hi, (h // 8, w // 8)).repeat(8, 0).repeat(8, 1).astype(np.int64)
        for _ in range(blur):
            a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(np.roll(a, 1, 0), 1, 1)) // 4
        return a
    tex = texture(H + 2 * M2, W + 2 * M2, 32, 224, 3)
    ctex = [texture(H // 2 + M2, W // 2 + M2, 64, 192, 2) for _ in range(2)]
    amp = 10 if mix == "noisy" else 3

    def cut(a, x2, y2, w, h, m0):  # the picture at half-pel offset (x2, y2): whole part a shift, an odd part the mean of two neighbours
        x, y = m0 + (x2 >> 1), m0 + (y2 >> 1)
        return (a[y: y + h, x: x + w] + a[y: y + h, x + (x2 & 1): x + (x2 & 1) + w] + a[y + (y2 & 1): y + (y2 & 1) + h, x: x + w] +
                a[y + (y2 & 1): y + (y2 & 1) + h, x + (x2 & 1): x + (x2 & 1) + w]) // 4

    def picture(x2, y2):
        p = np.concatenate([cut(tex, x2, y2, W, H, M2).ravel(), cut(ctex[0], x2 >> 1, y2 >> 1, W // 2, H // 2, M2 // 2).ravel(),
                            cut(ctex[1], x2 >> 1, y2 >> 1, W // 2, H // 2, M2 // 2).ravel()])
        return np.clip(p + rng.integers(-amp, amp + 1, p.shape), 0, 255).astype(np.uint8)
    prev = np.stack([picture(0, 0) for _ in MOVES])
    cur = np.stack([picture(dx, dy) for dx, dy in MOVES])
    if mix == "two_motion":  # the odd tiles from the picture moved by another vector
        yy, xx = np.mgrid[0:H, 0:W]
        odd = (((xx + 8) // 32 + (yy + 8) // 32) & 1).astype(bool)
        mask = np.concatenate([odd.ravel(), odd[::2, ::2].ravel(), odd[::2, ::2].ravel()])
        other = np.stack([picture(*MOVES[(i + 5) % len(MOVES)]) for i in range(len(MOVES))])
        cur[:, mask] = other[:, mask]
    return prev, cur


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
    ap.add_argument("--mixes", nargs="+", default=["translated", "noisy"])
    ap.add_argument("--partitions", action="store_true")
    ap.add_argument("--intra", action="store_true")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-pictures", type=int, default=512)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = encode_inter._lib()
    ilib = encode._lib()
    select = lib.mobi_debug_encp_select  # stages: 1 search, 2 code, 4 scan, 8 write, 16 decide, 32 finish (the intra mode's two), 63 all
    ALL = 63
    variants = [("", 0, 0)] + ([("_parts", 1, 0)] if a.partitions else []) + ([("_pintra", 0, 1)] if a.intra else [])

    def set_modes(enc, parts, intra):  # never both on: off first
        enc.set_partitions(False)
        enc.set_intra(False)
        enc.set_partitions(bool(parts))
        enc.set_intra(bool(intra))
    select.argtypes, select.restype = [C.c_int], None
    dev = torch.device("cuda", torch.cuda.current_device())
    s = torch.cuda.current_stream(dev)
    frame = W * H * 3 // 2
    nmax = max(a.counts + ([a.host_pictures] if not a.no_host else []))
    enc = m.MobiclipInterEncoder(W, H, VERSION, nmax)
    ienc = m.MobiclipIntraEncoder(W, H, VERSION, nmax)
    slot = 256 * 1024  # checked below: no stream of these mixes, intra or inter, is longer
    out = torch.empty((nmax, slot), dtype=torch.uint8, device=dev)
    sizes = torch.empty(nmax, dtype=torch.int32, device=dev)
    stats = torch.empty((nmax, 64), dtype=torch.uint8, device=dev)
    ref = torch.empty((nmax, frame), dtype=torch.uint8, device=dev)
    res = {"width": W, "height": H, "iters": a.iters, "content": "synthetic: a random texture of softened 8x8 cells moved by whole and half samples, 16 distinct pairs repeated"}
    for mix in a.mixes:
        prev, cur = pairs(mix, np.random.default_rng(77))
        reps = (nmax + 15) // 16
        src = torch.from_numpy(cur).to(dev).repeat(reps, 1)[:nmax].contiguous()
        before = torch.from_numpy(prev).to(dev).repeat(reps, 1)[:nmax].contiguous()
        for q in a.quantizers:
            qs = np.full(nmax, q, np.uint8)

            def intra(n, pics=src, rec=None):
                rc = ilib.mobi_enc_intra_async(ienc._h, s.cuda_stream, n, pics.data_ptr(), frame, qs.ctypes.data, 0, out.data_ptr(), slot, sizes.data_ptr(),
                                               rec.data_ptr() if rec is not None else None, None)
                assert rc == 0, rc

            def call(n):
                rc = lib.mobi_enc_inter_async(enc._h, s.cuda_stream, n, src.data_ptr(), frame, ref.data_ptr(), frame, qs.ctypes.data, qs.ctypes.data,
                                              out.data_ptr(), slot, sizes.data_ptr(), None, stats.data_ptr())
                assert rc == 0, rc
            intra(nmax, before, ref)  # the references: what a decoder holds after the frame before
            s.synchronize()
            for n in a.counts:
                k = f"{mix}_n{n}_q{q}"
                t_intra = timed(lambda: intra(n), s, a.iters, a.warmup)
                isz = float(sizes[:n].float().mean().item())
                assert int(sizes[:n].max().item()) <= slot
                for suffix, mode, pintra in variants:
                    set_modes(enc, mode, pintra)
                    select(ALL)
                    whole = timed(lambda: call(n), s, a.iters, a.warmup)
                    sz = sizes[:n].cpu().numpy()
                    st = stats[:n].cpu().numpy().view(encode_inter.STATS_DTYPE).reshape(-1)
                    assert sz.max() <= slot
                    t = {}
                    for name, bit in (("search", 1), ("code", 2), ("write", 12)) + ((("decide", 16), ("finish", 32)) if pintra else ()):
                        select(bit)
                        t[name] = timed(lambda: call(n), s, a.iters, 1)
                    select(ALL)
                    r = {"whole_ms": whole, "search_ms": t["search"], "code_ms": t["code"], "write_ms": t["write"], "pictures_per_s": n / whole * 1e3,
                         "gpixels_per_s": n * W * H / whole / 1e6, "bytes_per_picture": float(sz.mean()), "coded_blocks_per_picture": float(st["coded_blocks"].mean()),
                         "code0_per_picture": float(st["code0"].mean()), "nonzero_mv_per_picture": float(st["nonzero_mv"].mean()),
                         "halfpel_mv_per_picture": float(st["halfpel_mv"].mean()), "sad_per_picture": float(st["sad"].mean()), "intra_whole_ms": t_intra,
                         "intra_pictures_per_s": n / t_intra * 1e3, "intra_bytes_per_picture": isz}
                    if mode:
                        r.update(split_share=float(st["reserved"][:, encode_inter.STAT_SPLIT].mean()) / ((W // 16) * (H // 16)),
                                 leaves_per_picture=float(st["reserved"][:, encode_inter.STAT_LEAVES].mean()), search_vs_mode0=t["search"] / res[k]["search_ms"])
                    if pintra:
                        r.update(decide_ms=t["decide"], finish_ms=t["finish"], decide_launches=W // 16 + H // 16 - 1,
                                 intra_mb_share=float(st["reserved"][:, encode_inter.STAT_INTRA].mean()) / ((W // 16) * (H // 16)), whole_vs_mode0=whole / res[k]["whole_ms"])
                    res[k + suffix] = r
                    print("done", k + suffix, file=sys.stderr, flush=True)
            for suffix, mode, pintra in variants:
                if a.no_host:
                    break
                from tests import enc_inter_model as M
                from tests import enc_parts_model as Q
                hn = a.host_pictures
                hp, hr = src[:hn].cpu().numpy(), ref[:hn].cpu().numpy()
                t0 = time.perf_counter()
                if pintra:
                    from tests import enc_pintra_model as PI
                    r = PI.host_encode(W, H, VERSION, 1, hp, hr, qs[:hn], qs[:hn], slot_bytes=slot, threads=a.host_threads)
                elif a.partitions:
                    r = Q.host_encode(W, H, VERSION, mode, hp, hr, qs[:hn], qs[:hn], slot_bytes=slot, threads=a.host_threads)
                else:
                    r = M.host_encode(W, H, VERSION, hp, hr, qs[:hn], qs[:hn], slot_bytes=slot, threads=a.host_threads)
                dt = time.perf_counter() - t0
                set_modes(enc, mode, pintra)
                print("host done", mix, q, suffix or "mode 0", round(dt, 1), "s", file=sys.stderr, flush=True)
                call(hn)
                s.synchronize()
                res[f"{mix}_host_n{hn}_q{q}" + suffix] = {"threads": a.host_threads, "ms": dt * 1e3, "pictures_per_s": hn / dt,
                                                                              "equals_gpu": bool(np.array_equal(r["streams"], out[:hn].cpu().numpy()) and
                                                                                                 np.array_equal(r["bytes"], sizes[:hn].cpu().numpy()))}
            set_modes(enc, 0, 0)
    enc.close()
    ienc.close()
    line = json.dumps(json.loads(json.dumps(res), parse_float=lambda x: round(float(x), 4)))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
