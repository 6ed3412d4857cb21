#!/usr/bin/env python3
"""Generates tests/golden/encoder_vlc_ref.npy: the encoder's reverse VLC table MobiConst.VxTable0_A_Ref[32, 64, 2] (int16: for value,
skip, last the index of its code word in Vx2Table0_A, or -1), read from the reference's MobiConst.cs.  Data only; tests/test_txcode.py
checks the product's derivation of the same table (mobi_txcode.h, mobi_tc_build_ref) against it.

    python tests/golden/make_encoder_vlc_ref.py PATH/TO/LibMobiclip/Codec/Mobiclip/MobiConst.cs
"""
import os
import re
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "encoder_vlc_ref.npy")


def parse(text):
    m = re.search(r"VxTable0_A_Ref\s*=\s*\{(.*?)\};", text, re.S)
    if not m:
        raise SystemExit("VxTable0_A_Ref not found")
    nums = [int(v) for v in re.findall(r"-?\d+", m.group(1))]
    if len(nums) != 32 * 64 * 2:
        raise SystemExit(f"VxTable0_A_Ref: {len(nums)} numbers, expected {32 * 64 * 2}")
    return np.array(nums, dtype=np.int16).reshape(32, 64, 2)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    t = parse(open(sys.argv[1], encoding="utf-8-sig").read())
    np.save(OUT, t)
    print(OUT, t.shape, int((t >= 0).sum()), "entries with a code")


if __name__ == "__main__":
    main()
