"""The encoders' rate control without a GPU (include/mobiclip_encode_rate.h; csrc/mobi_encode_rate.h run by
tests/tools/mobi_encode_rate_host.cpp, the host model the _target_async calls are compared against in tests/test_encode_rate_gpu.py).

  1   an independent re-derivation: the bisection written out in Python over the EXISTING single-quantiser host models, one call of
      them per round, gives the model's quantisers, streams, lengths, reconstructions and statistics, and its every trial; the number of
      rounds is the closed form for all 861 ranges
  2   the guarantee: every stream is no longer than its target, or its quantiser is qmax
  3   the oracle decodes I, P, P, P chains made with targets to the reported reconstructions, and holds q_out after each frame
  4   qmin == qmax is the fixed-quantiser model byte for byte
  5   the calls cover what they must (test_coverage_conditions); how often the bisection misses the exhaustive smallest fitting
      quantiser is printed, not asserted ("Rate control", records it)
  6   header, library and the binding's table agree; the refusals that need no device
  7   the host model under sanitizers, as a program of its own
Shapes 16x16 and 48x32, both versions, I-frames, P-frames and P-frames with partitions."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import enc_inter_model as M
from tests import enc_model as E
from tests import enc_parts_model as Q
from tests import enc_rate_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOBI_E_ARG = -7
KEYS = ("streams", "bytes", "recon", "stats")


def test_rounds_are_the_closed_form_for_every_range():
    from mobiclipdecoder_amd import encode_rate
    n = 0
    for qmin in range(12, 53):
        for qmax in range(qmin, 53):
            k = next(k for k in range(8) if 2 ** k >= qmax - qmin + 1)
            assert R.host().encr_host_rounds(qmin, qmax) == encode_rate.rate_rounds(qmin, qmax) == R.rounds(qmin, qmax) == k <= 6
            n += 1
    assert n == 861
    for qmin, qmax in ((11, 52), (12, 53), (30, 29), (-1, 20), (0, 0), (52, 12)):
        assert R.host().encr_host_rounds(qmin, qmax) == encode_rate.rate_rounds(qmin, qmax) == -1


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("version", R.VERSIONS)
@pytest.mark.parametrize("W,H", R.SHAPES)
def test_the_model_is_the_bisection_over_the_existing_models(W, H, version, kind):
    pics, refs, _ = R.inputs(W, H, version, kind)
    for name, pq, tg, qmin, qmax in R.calls(W, H, version, kind):
        got = R.model(W, H, version, kind, name)
        want, q, trials = R.bisect(W, H, version, kind, pics, refs, pq, tg, qmin, qmax)
        assert np.array_equal(got["quantizer"], q), (name, got["quantizer"], q)
        for k in KEYS:
            assert np.array_equal(got[k], want[k]), (name, k)
        assert len(trials) == R.rounds(qmin, qmax)
        for r, (mid, b) in enumerate(trials):
            assert np.array_equal(got["trials"][:, r, 0], mid) and np.array_equal(got["trials"][:, r, 1], b), (name, r)
        assert (got["trials"][:, len(trials):] == -1).all()
        # (2) the guarantee, and that the range holds
        assert ((got["bytes"] <= tg) | (got["quantizer"] == qmax)).all(), name
        assert (got["quantizer"] >= qmin).all() and (got["quantizer"] <= qmax).all()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("version", R.VERSIONS)
def test_a_range_of_one_is_the_fixed_quantiser_model(version, kind):
    for W, H in R.SHAPES:
        pics, refs, pq = R.inputs(W, H, version, kind)
        for q in (12, 31, 52):
            for target in (0, 1 << 30):
                got = R.host_target(W, H, version, kind, pics, refs, pq, target, q, q, yuv_format=kind == 0)
                want = R.fixed(W, H, version, kind, pics, refs, pq, q, yuv_format=kind == 0)
                assert (got["quantizer"] == q).all() and (got["trials"] == -1).all()
                for k in KEYS:
                    assert np.array_equal(got[k], want[k]), (W, H, q, k)


def test_coverage_conditions():
    """Asserted on the model's output, for every kind, shape and version: a picture that ends at qmin; one strictly inside the range; one
    at qmax that fits; one at qmax that does not (targets 0 and 4); a target equal to a trial's length, which fits, and that target less
    one, which does not; one call with four or more different quantisers; a range of three rounds; a clamped previous quantiser that
    changes the stream.  Printed: how often the bisection is not the exhaustive smallest fitting quantiser."""
    missed = total = 0
    for W, H in R.SHAPES:
        for version in R.VERSIONS:
            for kind in R.KINDS:
                B = R.table(W, H, version, kind)
                seen = set()
                for name, pq, tg, qmin, qmax in R.calls(W, H, version, kind):
                    r = R.model(W, H, version, kind, name)
                    q, b, tr = r["quantizer"].astype(int), r["bytes"].astype(int), r["trials"]
                    if name == "k3":
                        assert R.rounds(qmin, qmax) == 3 and (tr[:, 2, 0] >= 0).all() and (tr[:, 3:] == -1).all()
                        seen.add("k3")
                    if name == "clamped":
                        assert (pq < 12).any() and (pq > 52).any()
                        same = R.host_target(W, H, version, kind, *R.inputs(W, H, version, kind)[:2], np.clip(pq, 12, 52), tg, qmin, qmax)
                        other = R.host_target(W, H, version, kind, *R.inputs(W, H, version, kind)[:2], R.REF_Q, tg, qmin, qmax)
                        assert all(np.array_equal(r[k], same[k]) for k in KEYS + ("quantizer",))
                        assert not np.array_equal(r["streams"], other["streams"])
                        seen.add("clamped")
                        continue
                    if not name.startswith("full"):
                        continue
                    if len(set(q.tolist())) >= 4:
                        seen.add("four_quantisers")
                    for i in range(len(q)):
                        if q[i] == qmin:
                            seen.add("qmin")
                        if qmin < q[i] < qmax:
                            seen.add("inside")
                        if q[i] == qmax:
                            seen.add("qmax_fits" if b[i] <= tg[i] else f"qmax_over_{int(tg[i])}")
                        for k in range(6):
                            if tr[i, k, 0] >= 0 and tr[i, k, 1] == tg[i]:      # it fitted: hi became this trial's quantiser
                                assert q[i] <= tr[i, k, 0]
                                seen.add("equal_fits")
                            if tr[i, k, 0] >= 0 and tr[i, k, 1] == tg[i] + 1:  # it did not: lo went above it (unless lo == hi already)
                                assert q[i] >= tr[i, k, 0]
                                if q[i] > tr[i, k, 0]:
                                    seen.add("one_less_does_not")
                        if tg[i] > 4:  # against the exhaustive search, recorded only
                            fit = [qq for qq in range(qmin, qmax + 1) if B[qq, i] <= tg[i]]
                            total += 1
                            missed += (min(fit) if fit else qmax) != q[i]
                want = {"qmin", "inside", "qmax_fits", "qmax_over_0", "qmax_over_4", "equal_fits", "one_less_does_not", "four_quantisers", "k3"} | ({"clamped"} if kind else set())
                assert seen >= want, (W, H, version, kind, want - seen)
    print(f"bisection differs from the exhaustive smallest fitting quantiser in {missed} of {total} (picture, target) cases")


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("version", R.VERSIONS)
@pytest.mark.parametrize("W,H", R.SHAPES)
def test_chains_decode_in_the_oracle_with_the_chosen_quantisers(W, H, version, mode):
    sets = Q.sequence_sets(W, H)
    frames = np.concatenate([sets["mixed5"][0], sets["two_motion"][0]])
    n = frames.shape[0]
    # a budget per clip from the fixed-quantiser chain at q = 30: the I-frame's length for every frame starves the I-frame's successors
    # of nothing and the I-frame not at all; half of it forces high quantisers; 4 forces qmax
    base = Q.chain(W, H, version, mode, frames, np.full((n, Q.T), 30, np.uint8))
    i_len = base[0]["bytes"].astype(np.int64)
    targets = np.stack([i_len, i_len // 2, np.maximum(base[2]["bytes"], 4), np.where(np.arange(n) % 2, 4, i_len)], 1).astype(np.int32)
    ch = R.chain(W, H, version, mode, frames, targets)
    qs = np.stack([r["quantizer"] for r in ch], 1)
    assert len(set(qs.ravel().tolist())) >= 4 and (qs[:, 1:] != qs[:, :-1]).any()
    for c in range(n):
        streams = [ch[t]["streams"][c, : int(ch[t]["bytes"][c])] for t in range(Q.T)]
        for t, (dec, used, q) in enumerate(M.oracle_chain(W, H, version, streams)):
            assert np.array_equal(dec, ch[t]["recon"][c]), (c, t)
            assert q == int(qs[c, t]) and used <= len(streams[t]), (c, t)
            assert ch[t]["bytes"][c] <= targets[c, t] or q == 52, (c, t)


def test_header_library_and_binding_agree():
    from mobiclipdecoder_amd import build, encode, encode_inter, encode_rate
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobiclip_encode_rate.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mobi_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(encode_rate._SIGS) == ["mobi_enc_inter_target_async", "mobi_enc_intra_target_async", "mobi_enc_rate_rounds"]
    assert set(names) <= set(build.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_HIP], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not set(names) & (set(encode._SIGS) | set(encode_inter._SIGS) | set(encode_inter._PARTS_SIGS))
    lib = encode_rate._lib()
    for name, (res, args) in encode_rate._SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == list(args), name
    # the tables agree with the prototypes' argument counts
    for name in names:
        proto = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(proto.split(",")) == len(encode_rate._SIGS[name][1]), name


def test_refusals_need_no_device():
    """the host model refuses what the calls refuse: a range outside [12, 52] or upside down, no targets, misaligned targets, no room for
    the quantisers; and the entry points refuse a NULL encoder before they look at anything else"""
    from mobiclipdecoder_amd import encode_rate
    lib = encode_rate._lib()
    assert lib.mobi_enc_intra_target_async(None, None, 1, None, 384, None, 12, 52, 0, None, 0, None, None, None, None) == MOBI_E_ARG
    assert lib.mobi_enc_inter_target_async(None, None, 1, None, 384, None, 384, None, None, 12, 52, None, 0, None, None, None, None) == MOBI_E_ARG
    L = R.host()
    pic, out, n, q = np.zeros((1, 384), np.uint8), np.zeros(4096, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.uint8)
    tg = np.zeros(3, np.int32)
    pq = np.array([30], np.uint8)

    def call(kind=0, qmin=12, qmax=52, target=tg.ctypes.data, qout=q.ctypes.data, W=16, prev=pq.ctypes.data):
        return L.encr_host_target(W, 16, 2, kind, 1, pic.ctypes.data, 384, pic.ctypes.data, 384, prev, target, qmin, qmax, 0, out.ctypes.data, 4096, n.ctypes.data,
                                  None, None, qout, None, 1)
    assert call() == 0 and call(1) == 0 and call(2) == 0
    for kw in (dict(qmin=11), dict(qmax=53), dict(qmin=30, qmax=29), dict(target=None), dict(target=tg.ctypes.data + 2), dict(qout=None), dict(W=12),
               dict(kind=3), dict(kind=1, prev=None)):
        assert call(**kw) == MOBI_E_ARG, kw


def test_host_model_under_sanitizers(tmp_path):
    """tests/tools/enc_rate_host_main.cpp: a program of its own with -fsanitize=address,undefined, linked statically (nothing sanitised is
    loaded into Python); its buffers are exactly one picture, one reference, one slot and one row long"""
    exe = str(tmp_path / "enc_rate_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-variable", "-fwrapv", "-pthread", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I" + E.CSRC, os.path.join(E.TOOLS, "enc_rate_host_main.cpp"),
                    os.path.join(E.TOOLS, "mobi_encode_rate_host.cpp"), "-o", exe], check=True)
    for W, H in R.SHAPES:
        for kind in R.KINDS:
            pics, refs, _ = R.inputs(W, H, 2, kind)
            n, bound = pics.shape[0], R.host().encr_host_bound(W, H, kind)
            for name in ("full0", "k3", "one") + (("clamped",) if kind else ()):
                _, pq, tg, qmin, qmax = next(c for c in R.calls(W, H, 2, kind) if c[0] == name)
                want = R.model(W, H, 2, kind, name)
                src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
                with open(src, "wb") as f:
                    f.write(tg.tobytes() + (pq.tobytes() + pics.tobytes() + refs.tobytes() if kind else pics.tobytes()))
                p = subprocess.run([exe, str(W), str(H), "2", str(kind), str(qmin), str(qmax), str(n), src, dst], capture_output=True, text=True)
                assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
                blob = np.fromfile(dst, np.uint8)
                assert np.array_equal(blob[:n], want["quantizer"])
                assert np.array_equal(np.frombuffer(blob[n: 5 * n].tobytes(), np.int32), want["bytes"])
                assert np.array_equal(blob[5 * n: 5 * n + n * bound].reshape(n, bound), want["streams"])
                assert np.array_equal(blob[5 * n + n * bound:].reshape(n, -1), want["recon"])
