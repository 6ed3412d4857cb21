"""Randomised GPU-vs-oracle sweep aimed at the inter path: many small streams (every partition shape, deep trees, older references,
all half-pel phases, vectors that leave the picture and read its zero padding, widths that leave the last octet partly empty -- 80,
144, 272, 528, 848 -- so that the zeros the octet kernel stores there are read back by the next frames, width == stride), a few intra
macroblocks in between, batches of 1..7 clips, host-parsed and device-parsed alternately.  Stops at the first difference.
python tools/fuzz_inter_gpu.py [rounds] [seed0]
python tools/fuzz_inter_gpu.py --scripted [rounds] [seed0]: the region the generator's draw avoids -- written-down P-frames
(mobi_gen_clip_scripted) with raw 12-bit levels, coefficient sums on both sides of the packed limit of the residual stage, residuals up to
+-319 and now and then a sample outside the clamp table's domain, over random flat predictions; rc (MOBI_E_CLAMP where the oracle
throws), Offset and planes."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mobiclipdecoder_amd as m
from mobiclipdecoder_amd.streamgen import BASE_SEED
from tests.oracle_binding import OracleDecoder

scripted = "--scripted" in sys.argv
argv = [a for a in sys.argv if a != "--scripted"]
rounds = int(argv[1]) if len(argv) > 1 else 200
seed0 = int(argv[2]) if len(argv) > 2 else 0


def scripted_clip(rng, w, h, seed):
    """I-frame of 128s, a set-up frame of flat 4x4 blocks, then two frames of random directed blocks"""
    from mobiclipdecoder_amd.streamgen import generate_scripted
    from tests import residual_model as rm
    q = int(rng.choice([12, 12, 18, 25, 40, 52]))
    mbs, toks = {}, []

    def block(frame, mb, area, n, sub, tk, intra):
        e = mbs.setdefault((frame, mb), [frame, mb, intra, 0, 0, 0, 0, 0, 0, 0, 0])
        e[3] |= 1 << area
        if n == 8:
            e[4] |= 1 << area
        else:
            e[5 + area] |= 1 << sub
        toks.extend((frame, mb, area * 4 + (sub if n == 4 else 0), p, lev, int(rng.integers(0, 4))) for p, lev in tk)

    n_mb = (w // 16) * (h // 16)
    for mb in range(n_mb):
        for area in range(6):
            if rng.random() < 0.5:
                for sub in range(4):
                    if rng.random() < 0.7:
                        block(1, mb, area, 4, sub, [(0, int(rng.integers(1, 120)) * int(rng.choice((-1, 1))))], 0)
    for frame in (2, 3):
        for mb in range(n_mb):
            intra = int(rng.random() < 0.15)
            for area in range(6):
                if rng.random() > 0.04:
                    continue
                n = 8 if rng.random() < 0.6 else 4
                budget = float(rng.choice([300, 1500, 3000, 6000, 14000, 14600, 20000])) * rng.random() ** 2  # sum of |coefficient| to spend
                for sub in ([0] if n == 8 else [k for k in range(4) if rng.random() < 0.6] or [0]):
                    pos = sorted(set(int(v) for v in rng.integers(0, min(n * n, 12), int(rng.integers(1, 4)))))
                    sc = rm.scales(q, n)
                    tk = []
                    for p_ in pos:
                        lev = int(max(1, min(2047, budget / len(pos) / int(sc[p_])))) * int(rng.choice((-1, 1)))
                        tk.append((p_, lev))
                    block(frame, mb, area, n, sub, tk, intra)
    p = m.default_params("A", seed, width=w, height=h, version=1, n_frames=4, quantizer=12, cbp_prob=0, intra_dc_only=1)
    return p, generate_scripted(p, list(mbs.values()), toks, [0, 0, q - 12, 0])


if scripted:
    rng = np.random.default_rng(4321 + seed0)
    t0, frames, valid, rejected = time.time(), 0, 0, 0
    for it in range(rounds):
        w, h = [(128, 16), (128, 32), (256, 32), (64, 48)][int(rng.integers(4))]
        nclips = int(rng.integers(1, 8))
        clips = [scripted_clip(rng, w, h, BASE_SEED + 7 * it + i) for i in range(nclips)]
        if it & 2:
            os.environ["MOBI_FUSED_STEP_MBS"] = "0"
        else:
            os.environ.pop("MOBI_FUSED_STEP_MBS", None)
        mode = [False, True, "lockstep"][it % 3]
        b = m.MobiclipBatch(nclips, w, h, 1, device_parse=mode)
        oras = [OracleDecoder(w, h, 1) for _ in clips]
        alive = [True] * nclips  # after a reject the two decoders hold different partial frames: the clip is compared no further
        for f in range(4):
            rcs, offs = b.decode([c[1][0][c[1][1][f]:c[1][1][f + 1]] for c in clips], [0] * nclips)
            for i in range(nclips):
                data, fo = clips[i][1]
                oras[i].Data, oras[i].Offset = data[fo[f]:fo[f + 1]], 0
                o = oras[i].DecodeFrame()
                if not alive[i]:
                    continue
                if o is None:
                    ok = oras[i].last_error == -1 and rcs[i] == -5
                    alive[i] = False
                    rejected += 1
                else:
                    y, uv = b.planes(i)
                    ok = rcs[i] == 0 and offs[i] == oras[i].Offset and np.array_equal(y, o[0]) and np.array_equal(uv, o[1])
                    valid += 1
                if not ok:
                    print("DIFFERENCE scripted round", it, "frame", f, "clip", i, "parse", mode, "two_launches", bool(it & 2), "rc", rcs[i], oras[i].last_error, "seed0", seed0)
                    sys.exit(1)
            frames += nclips
        b.close()
        for o in oras:
            o.close()
    print("fuzz_inter_gpu --scripted: %d rounds, %d clip-frames (%d decoded, %d rejected), no difference, %.0f s" % (rounds, frames, valid, rejected, time.time() - t0))
    sys.exit(0 if valid > rounds and rejected > rounds // 20 else 2)

geoms = [(16, 16, 2), (80, 48, 1), (144, 64, 2), (256, 32, 1), (512, 32, 2), (160, 112, 2), (272, 48, 1), (128, 128, 2), (848, 32, 2), (528, 48, 2), (1024, 32, 2), (640, 48, 2)]
rng = np.random.default_rng(1234 + seed0)
t0, frames, mbs = time.time(), 0, 0
for it in range(rounds):
    w, h, ver = geoms[int(rng.integers(len(geoms)))]
    nclips = int(rng.integers(1, 8))
    nfr = int(rng.integers(4, 9))
    kw = dict(width=w, height=h, version=ver, n_frames=nfr, pm_intra=int(rng.choice([0, 50, 200])), pm_deep=int(rng.choice([0, 100, 400])), pm_multiref=int(rng.choice([0, 200, 600])), pm_skip=int(rng.choice([0, 150, 500])), pm_split1=int(rng.choice([100, 400])), intra_sub_prob=int(rng.choice([100, 500, 900])),
              plane_prob=int(rng.choice([0, 300, 700])), iframe_interval=int(rng.choice([0, 0, 4])), mv_range=int(rng.choice([2, 12, 40, 90])),
              cbp_prob=int(rng.choice([100, 300, 700])), dense_prob=int(rng.choice([0, 200])), qdelta_prob=int(rng.choice([0, 300])),
              table1_prob=int(rng.choice([0, 500])), escape_prob=int(rng.choice([0, 80])), quantizer=int(rng.choice([12, 18, 25, 29, 33, 36, 40, 46, 52])),
              intra_dc_only=int(rng.choice([0, 0, 1])), edge_mode=int(rng.choice([0, 1])))
    ps = [m.default_params("A", BASE_SEED + 100000 + 1000 * (seed0 + it) + i, **kw) for i in range(nclips)]
    clips = [m.generate_clip(p) for p in ps]
    dev = bool(it & 1)
    if it & 2:  # host-parsed rounds: a small step is ONE launch (mobi_recon_step) unless the limit is 0; both kinds in turn
        os.environ["MOBI_FUSED_STEP_MBS"] = "0"
    else:
        os.environ.pop("MOBI_FUSED_STEP_MBS", None)
    b = m.MobiclipBatch(nclips, w, h, ver, device_parse=dev)
    oras = [OracleDecoder(w, h, ver) for _ in ps]
    for f in range(nfr):
        rcs, offs = b.decode([c[0][c[1][f]:c[1][f + 1]] for c in clips], [0] * nclips)
        for i in range(nclips):
            oras[i].Data, oras[i].Offset = clips[i][0][clips[i][1][f]:clips[i][1][f + 1]], 0
            o = oras[i].DecodeFrame()
            ok = rcs[i] == 0 and o is not None and offs[i] == oras[i].Offset
            if ok:
                y, uv = b.planes(i)
                ok = np.array_equal(y, o[0]) and np.array_equal(uv, o[1])
            if not ok:
                print("DIFFERENCE round", it, "frame", f, "clip", i, "device_parse", dev, "two_launches", bool(it & 2), "rc", rcs[i], oras[i].last_error, kw, "seed", ps[i].seed)
                sys.exit(1)
        frames += nclips
        mbs += nclips * (w // 16) * (h // 16)
    b.close()
    for o in oras:
        o.close()
print("fuzz_inter_gpu: %d rounds, %d clip-frames, %d macroblocks, no difference, %.0f s" % (rounds, frames, mbs, time.time() - t0))
