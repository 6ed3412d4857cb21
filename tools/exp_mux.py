#!/usr/bin/env python3
"""What the muxer costs and buys on one GPU (include/mobiclip_mux.h; DESIGN.md "Muxing").  640x480, tools/exp_encode_inter.py's synthetic
mixes (16 distinct pairs repeated): read the figures as those of these mixes.  Prints ONE JSON line and, with --out, appends it to a file.

  --kernels   per mix (translated, noisy) and N in --counts: the inter encoder's fixed-quantiser call (HIP events, --iters calls) and, fed
              by its slots and lengths in the same run, mobi_mux_append_async (the append kernel and the advance kernel behind it):
              ms, bytes read plus written, their rate as a share of 8 TB/s, and the ratio to the encode call
  --clips     whole clips, wall clock, median of --iters, --frames frames, N in --clips-n, fixed quantiser, translated mix, with the
              library MOBI_LIB names and the package under --package-root (this tree, or another commit's):
                --mode framed   encode_clips() as it always was, then a host loop that frames its streams (tests/containers.write_moflex)
                --mode muxed    encode_clips(container="moflex")
              and the peak device memory of either (torch.cuda.max_memory_allocated); a job alternates the two
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _early(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


PKG_ROOT = os.path.abspath(_early("--package-root", ROOT))
os.environ.setdefault("MOBI_LIB", os.path.join(PKG_ROOT, "mobiclipdecoder_amd", "libmobiclip_hip.so"))
sys.path.insert(0, PKG_ROOT)
import mobiclipdecoder_amd as m  # noqa: E402  (from --package-root: imported before anything else puts this tree in front)

sys.path.insert(1, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from exp_encode_inter import H, VERSION, W, pairs, timed  # noqa: E402

FRAME = W * H * 3 // 2
HBM_BYTES_PER_S = 8e12


def kernels(a, dev, res):
    from mobiclipdecoder_amd import encode, encode_inter, mux
    s = torch.cuda.current_stream(dev)
    nmax = max(a.counts)
    ienc, penc = m.MobiclipIntraEncoder(W, H, VERSION, nmax), m.MobiclipInterEncoder(W, H, VERSION, nmax)
    ilib, plib, mlib = encode._lib(), encode_inter._lib(), mux._lib()
    SLOT = max(ienc.stream_bound, penc.stream_bound)  # the slot encode_clips gives every stream
    out = torch.empty((nmax, SLOT), dtype=torch.uint8, device=dev)
    sizes = torch.empty(nmax, dtype=torch.int32, device=dev)
    ref = torch.empty((nmax, FRAME), dtype=torch.uint8, device=dev)
    qs = np.full(nmax, a.quantizer, np.uint8)
    frames = a.iters + a.warmup + 1
    for mix in ("translated", "noisy"):
        prev, cur = pairs(mix, np.random.default_rng(77))
        reps = (nmax + 15) // 16
        src = torch.from_numpy(cur).to(dev).repeat(reps, 1)[:nmax].contiguous()
        before = torch.from_numpy(prev).to(dev).repeat(reps, 1)[:nmax].contiguous()
        assert ilib.mobi_enc_intra_async(ienc._h, s.cuda_stream, nmax, before.data_ptr(), FRAME, qs.ctypes.data, 0, out.data_ptr(), SLOT, sizes.data_ptr(),
                                         ref.data_ptr(), None) == 0
        for n in a.counts:
            def enc():
                assert plib.mobi_enc_inter_async(penc._h, s.cuda_stream, n, src.data_ptr(), FRAME, ref.data_ptr(), FRAME, qs.ctypes.data, qs.ctypes.data,
                                                 out.data_ptr(), SLOT, sizes.data_ptr(), None, None) == 0
            enc_ms = timed(enc, s, a.iters, a.warmup)
            sz = sizes[:n].cpu().numpy().astype(np.int64)
            assert sz.min() > 0 and sz.max() <= SLOT
            for container in ("moflex", "mods"):
                mx = m.MobiclipMuxer(container, W, H, n, max_key_frames=frames)
                files = mx.begin(n, mux.fixed_bytes(container, frames) + frames * mux.framed_bytes(container, int(sz.max())))

                def app():
                    assert mlib.mobi_mux_append_async(mx._h, s.cuda_stream, n, out.data_ptr(), SLOT, SLOT, sizes.data_ptr(), 1) == 0
                ms = timed(app, s, a.iters, a.warmup)
                _, ln, st = mx.finish(to_host=False)
                assert not st.cpu().any() and int(ln.min()) > 0
                moved = int(sz.sum()) + sum(mux.framed_bytes(container, int(v)) for v in sz)
                res[f"{mix}_n{n}_{container}"] = {"encode_inter_ms": enc_ms, "append_ms": ms, "append_over_encode": ms / enc_ms, "bytes_per_stream": float(sz.mean()),
                                                  "bytes_read_and_written": moved, "share_of_8TBps": moved / (ms * 1e-3) / HBM_BYTES_PER_S}
                mx.close()
                del files
                print("done", mix, n, container, file=sys.stderr, flush=True)
    ienc.close()
    penc.close()


def clips(a, dev, res):
    from tests.containers import write_moflex
    _, cur = pairs("translated", np.random.default_rng(77))
    src = torch.from_numpy(cur).to(dev)
    for n in a.clips_n:
        frames = torch.stack([src[(torch.arange(n, device=dev) + t) % 16] for t in range(a.frames)], 1).contiguous()
        if a.mode == "muxed":
            def run():
                return m.encode_clips(frames, a.quantizer, a.frames, VERSION, W, H, container="moflex")
        else:
            def run():
                return [write_moflex(c, W, H).tobytes() for c in m.encode_clips(frames, a.quantizer, a.frames, VERSION, W, H)]
        run()  # warm-up: the allocator, the first launches
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        ms = []
        for _ in range(a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = run()
            ms.append((time.perf_counter() - t0) * 1e3)
        import hashlib
        res[f"clips{n}"] = {"ms": sorted(ms)[len(ms) // 2], "ms_all": ms, "peak_device_bytes": int(torch.cuda.max_memory_allocated(dev)),
                            "file_bytes_total": sum(len(f) for f in got), "sha256": hashlib.sha256(b"".join(got)).hexdigest()[:16]}
        del frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--clips", action="store_true")
    ap.add_argument("--mode", choices=("framed", "muxed"), default="muxed")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--counts", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--clips-n", type=int, nargs="+", default=[4, 64])
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--quantizer", type=int, default=30)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"width": W, "height": H, "iters": a.iters, "quantizer": a.quantizer, "lib": os.path.relpath(os.environ["MOBI_LIB"], ROOT),
           "package": os.path.relpath(os.path.dirname(m.__file__), ROOT)}
    if a.kernels:
        res["what"] = "kernels"
        kernels(a, dev, res)
    if a.clips:
        res.update(what="clips", mode=a.mode, frames=a.frames)
        clips(a, dev, res)
    line = json.dumps(json.loads(json.dumps(res), parse_float=lambda x: round(float(x), 4)))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
