#!/usr/bin/env python3
"""Generates tests/golden/csref_records.npz: what the C#->C++ transliteration of the reference (oracle/_ref/libmobi_csref.so, made by
oracle/tools/cs2cpp.py, so only where the reference sources are) computes for every case of tests/test_csref_differential.py.

Runs the tests of that module once with the library's results recorded instead of checked against the file -- the oracle is still
checked against them as it goes -- and writes what was recorded.  The record holds only results: per frame whether it throws, Offset,
Quantizer and a 64-bit digest of the ring's planes; per trial of the unit sweep the return codes and digests of the outputs.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from tests import test_csref_differential as t
    if t._lib() is None:
        sys.exit("the transliteration library cannot be built here (oracle/tools/cs2cpp.py needs the reference sources)")
    t._recording = {}
    for cfg in "ABC":
        t.test_valid_streams(cfg)
        t.test_bench_streams(cfg)
    t.test_small_geometries_and_quantizers()
    t.test_corrupted_streams_including_partial_frames()
    t.test_low_quantizer_aliasing_domain()
    t.test_coverage_suite_streams()
    t.test_unit_statements_random_sweep()
    np.savez_compressed(t.RECORD, **t._recording)
    print(t.RECORD, os.path.getsize(t.RECORD), "bytes,", len(t._recording), "cases")


if __name__ == "__main__":
    main()
