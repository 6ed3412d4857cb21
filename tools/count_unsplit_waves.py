"""usage: python tools/count_unsplit_waves.py [--config B] [--clips 24576] [--distinct 16]  (host only, no GPU)

Which waves of mobi_recon_intra take the six-step path (recon_intra_quad, `plain`): those whose four launch items have no split area.
Rebuilds the launch order of bench.py's headline batch on the host -- LevelPlan (mobi_batch.h): per dependency level, per class
(mobi_parse.cpp finish_levels: bits [1:0] = min(split areas, 3)), per clip, levels padded to whole waves -- from the host parser's
command lists (tests/interp_binding.py), and counts per frame kind: the share of waves without a split area, of macroblocks without one,
and of (wave, step) pairs of the unsplit waves in which no row's step is a directional one (what a ballot in front of the tap request
would save)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mobiclipdecoder_amd as m  # noqa: E402
from mobiclipdecoder_amd import sharding  # noqa: E402
from tests.interp_binding import InterpDecoder  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="B")
ap.add_argument("--clips", type=int, default=24576)
ap.add_argument("--distinct", type=int, default=16)
ap.add_argument("--pframes", type=int, default=32)
args = ap.parse_args()


def frame_lists(p, data, fo):
    """per frame: {(level, class): [per macroblock (first records of the six areas)]} of one stream"""
    d = InterpDecoder(p.width, p.height, p.version)
    mbw = p.width // 16
    out = []
    for f in range(p.n_frames):
        d.Data, d.Offset = data[: fo[f + 1]], int(fo[f])
        assert d.DecodeFrame() is not None
        desc, mbs, ls, _ = d.command_list()
        pay = d.payload()
        named = set()
        for mb in mbs:
            w = desc[mb, 4:8]
            for dep in np.concatenate([w & 0xFFFF, w >> 16]):
                if dep != 0xFFFF and not dep & 0x8000:
                    named.add(int(dep & 0x1FFF))
        groups = {}
        for L in range(1, len(ls) - 1):
            for mb in mbs[ls[L]:ls[L + 1]]:
                recs = [int(pay[int(desc[mb, 0]) + 4 * a]) for a in range(6)]
                splits = sum((r >> 5) & 1 for r in recs)
                mbx = int(mb) % mbw
                k = (0 if (mbx >= 1 and mbx + 1 < mbw and mb >= mbw) else 8) + (4 if int(mb) in named else 0) + min(splits, 3)
                groups.setdefault((L, k), []).append(recs)
        out.append(groups)
    d.close()
    return out


streams = []
for i in range(min(args.distinct, args.clips)):
    p = m.default_params(args.config, sharding.stream_seed(args.config, 0, i), n_frames=1 + args.pframes)
    streams.append(frame_lists(p, *m.generate_clip(p)))
copies = [len(range(i, args.clips, len(streams))) for i in range(len(streams))]  # clip c plays stream c mod distinct


def is_tap(r):
    mode = r & 15
    return mode < 2 or 4 <= mode <= 8


tot = {"P": np.zeros(6, np.int64), "I": np.zeros(6, np.int64)}  # waves, unsplit waves, macroblocks, unsplit macroblocks, steps of unsplit waves, those without a tap row
for f in range(1 + args.pframes):
    t = tot["I" if f == 0 else "P"]
    levels = max(L for s in streams for (L, _) in s[f]) if any(s[f] for s in streams) else 0
    for L in range(1, levels + 1):
        # the level's items in launch order: per class, per clip (the clips of one stream are copies of its list)
        items = []
        for k in range(16):
            for si, s in enumerate(streams):
                g = s[f].get((L, k))
                if g:
                    items.append((k, g, copies[si]))
        flat_split, flat_tap = [], []
        for k, g, n in items:
            flat_split += [bool(k & 3)] * (len(g) * n)
            taps = [[is_tap(r) for r in recs] for recs in g]
            flat_tap += taps * n
        n_items = len(flat_split)
        if n_items == 0:
            continue
        sp = np.array(flat_split + [False] * (-n_items % 4)).reshape(-1, 4)
        tp = np.array(flat_tap + [[False] * 6] * (-n_items % 4)).reshape(-1, 4, 6)
        plain = ~sp.any(1)
        t += [len(sp), int(plain.sum()), n_items, n_items - int(np.sum(flat_split)), 6 * int(plain.sum()), int((~tp[plain].any(1)).sum())]
for kind in "PI":
    w, pw, n, pn, st, nt = (int(x) for x in tot[kind])
    if w:
        print("%s-frames, %d clips of config %s: %d waves, %.1f %% without a split area; %d macroblocks, %.1f %% without one; "
              "%.2f %% of the unsplit waves' steps have no directional row" % (kind, args.clips, args.config, w, 100.0 * pw / w, n, 100.0 * pn / n, 100.0 * nt / max(st, 1)))
