"""The encoder's transform coding (include/mobiclip_hip.h, mobi_transform_code; csrc/mobi_txcode.h / .hip / .cpp).

CPU: the product's header compiled for the host (tests/tools/txcode_host.cpp) against the reference's reverse VLC table
(tests/golden/encoder_vlc_ref.npy) and against float32 division + round-half-even for every quantiser; the bound that makes the
quantiser exact and the levels int16; mobi_encoder_qtables; the argument checks; the scalar restatement (tests/tools/txcode_ref.c)
against the oracle's transforms.
GPU: every output and flag of mobi_transform_code / _async bit-exact against the restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 -- before the product library is loaded: torch tensors need torch's HIP runtime to be the library's too

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mobiclipdecoder_amd", "csrc")
TOOLS = os.path.join(ROOT, "tests", "tools")
VXREF = np.load(os.path.join(ROOT, "tests", "golden", "encoder_vlc_ref.npy"))  # MobiConst.VxTable0_A_Ref[32, 64, 2]
MOBI_E_ARG = -7
P = C.c_void_p

# the reference's DCT64 / DCT16 weights and divisors per output (MobiEncoder.cs:970-1008, 1154-1176), for the bound
W8 = np.array([[1, 1, 1, 1, 1, 1, 1, 1], [48, 40, 24, 12, -12, -24, -40, -48], [2, 1, -1, -2, -2, -1, 1, 2], [40, -12, -48, -24, 24, 48, 12, -40],
               [1, -1, -1, 1, 1, -1, -1, 1], [24, -48, 12, 40, -40, -12, 48, -24], [1, -2, 2, -1, -1, 2, -2, 1], [12, -24, 40, -48, 48, -40, 24, -12]])
D8 = np.array([8, 289, 10, 289, 8, 289, 10, 289])
W4 = np.array([[1, 1, 1, 1], [2, 1, -1, -2], [1, -1, -1, 1], [1, -2, 2, -1]])
D4 = np.array([4, 5, 4, 5])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("txcode_host") / "libtxcode_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-variable", "-I" + CSRC, os.path.join(TOOLS, "txcode_host.cpp"),
                    "-o", so], check=True)
    L = C.CDLL(so)
    L.tc_lut_index.restype = C.c_int
    for f, a in (("tc_build_ref", [P]), ("tc_build_lut", [P]), ("tc_lut_index", [C.c_int] * 3), ("tc_qtable", [C.c_int, C.c_int, P]),
                 ("tc_quant_range", [C.c_int, C.c_int, C.c_int, P])):
        getattr(L, f).argtypes = a
    return L


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("txcode_ref") / "libtxcode_ref.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-fPIC", "-shared", "-fwrapv", "-ffp-contract=off", "-Wall", "-Wno-unused-const-variable", "-I" + CSRC,
                    os.path.join(TOOLS, "txcode_ref.c"), "-o", so, "-lm"], check=True)
    L = C.CDLL(so)
    L.ref_qtables.argtypes = [C.c_int, P, P]
    L.ref_dct.argtypes = [C.c_int, P, P]
    L.ref_idct.argtypes = [C.c_int, P, P, P]
    L.ref_coef_bits.argtypes = [C.c_int, C.c_int, C.c_int, P]
    L.ref_encode_batch.argtypes = [C.c_int, C.c_int, P, C.c_long, P, P, P, P, P, P, P, P]
    return L


_VX = np.ascontiguousarray(VXREF.astype(np.int16))


def encode_ref(ref, src, pred, qs):
    """the restatement over a batch: dict shaped as transform_code's"""
    src, pred = np.ascontiguousarray(src, np.uint8), np.ascontiguousarray(pred, np.uint8)
    nb, nn = src.shape
    nq = len(qs)
    out = {"levels": np.empty((nq, nb, nn), np.int16), "recon": np.empty((nq, nb, nn), np.uint8), "bits": np.empty((nq, nb), np.int32),
           "sad": np.empty((nq, nb), np.int32), "flags": np.empty((nq, nb), np.uint8)}
    qa = np.array(qs, np.int32)
    ref.ref_encode_batch(8 if nn == 64 else 4, nq, qa.ctypes.data, nb, src.ctypes.data, pred.ctypes.data, _VX.ctypes.data, out["levels"].ctypes.data,
                         out["recon"].ctypes.data, out["bits"].ctypes.data, out["sad"].ctypes.data, out["flags"].ctypes.data)
    return out


def _q_table(host, q, n):
    t = np.empty(n * n, np.int32)
    host.tc_qtable(q, n, t.ctypes.data)
    return t


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_derived_reverse_table_equals_the_reference_and_the_lut_its_branches(host, ref):
    """1. mobi_tc_build_ref (from mobi_vx2table0_a) is VxTable0_A_Ref in all 4096 entries; the kernel's [2][64][44] cost table, extended
    by 28 bits for every |level| >= 44, equals the literal branches of CalculateNrBitsDCT for every |level| 1..5875, run 0..63, last 0/1."""
    derived = np.empty(32 * 64 * 2, np.int16)
    host.tc_build_ref(derived.ctypes.data)
    assert np.array_equal(derived.reshape(32, 64, 2), VXREF)
    lut = np.empty(2 * 64 * 44, np.uint8)
    host.tc_build_lut(lut.ctypes.data)
    bad = []
    for last in (0, 1):
        for skip in range(64):
            for v in range(1, 5876):
                want = ref.ref_coef_bits(v, skip, last, _VX.ctypes.data)
                got = int(lut[host.tc_lut_index(v, skip, last)]) if v < 44 else 28
                if got != want:
                    bad.append((v, skip, last, got, want))
    assert not bad, bad[:10]


def _qs_distinct(host):
    return sorted({int(x) for q in range(54) for n in (4, 8) for x in _q_table(host, q, n)})


def test_quantiser_is_float32_division_with_round_half_even(host):
    """2. mobi_tc_quant equals (int)Math.Round((float)d / Q) -- float32 division, ties to even -- for every Q of quantisers 0..53 and every
    |d| <= 40 000 (the DCT output is bounded by 23 500).  Exact ties occur; rounding them away from zero would fail."""
    qs = _qs_distinct(host)
    assert len(qs) == 170 and qs[0] == 4 and qs[-1] == 7424
    d = np.arange(-40000, 40001, dtype=np.int32)
    got = np.empty_like(d)
    ties = 0
    for Q in qs:
        host.tc_quant_range(int(d[0]), d.size, Q, got.ctypes.data)
        want = np.rint(d.astype(np.float32) / np.float32(Q)).astype(np.int32)
        assert np.array_equal(got, want), (Q, d[got != want][:5])
        a2 = 2 * np.abs(d)
        tie = (a2 % Q == 0) & ((a2 // Q) % 2 == 1)  # |d| / Q = k + 1/2
        ties += int(tie.sum())
        k_even = tie & (((a2 // Q - 1) // 2) % 2 == 0)
        away = (np.sign(d) * np.floor(np.abs(d) / Q + 0.5)).astype(np.int32)
        assert np.array_equal(away != want, k_even), Q  # half away from zero is wrong exactly on the ties with k even
    assert ties > 100000


def _dct(n, x):
    """the reference's two passes, exactly: numpy int64 with truncating division"""
    W, D = (W8, D8) if n == 8 else (W4, D4)
    x = np.asarray(x, np.int64).reshape(-1, n, n) * 64
    t = np.einsum("uj,bij->biu", W, x)
    t = np.trunc(t / D).astype(np.int64)  # exact: |t| < 2^31, divisors small
    o = np.einsum("uj,bji->biu", W, t)
    return np.trunc(o / D).astype(np.int64).reshape(-1, n * n)


def test_dct_output_bound_is_23500():
    """3. |DCT64| and |DCT16| <= 23 500 for any residual in [-255, 255]: a pass multiplies the largest magnitude by at most
    max_u sum_j |W[u][j]| / D[u] = 1.2, and truncation never increases it, so 64 * 255 = 16 320 -> 19 584 -> 23 500 (floors).  The
    sign pattern of the 1.2 rows reaches it in mobi_oracle_dct8/4; so |level| <= 23 500 / 4 (the smallest Q) fits int16."""
    from tests.oracle_binding import lib as oracle_lib
    L = oracle_lib()
    for n, W, D, f in ((8, W8, D8, L.mobi_oracle_dct8), (4, W4, D4, L.mobi_oracle_dct4)):
        f.argtypes = [P, P]
        f.restype = None
        gain = np.abs(W).sum(1)
        first = max((64 * 255 * int(g)) // int(d) for g, d in zip(gain, D))
        bound = max((first * int(g)) // int(d) for g, d in zip(gain, D))
        assert first == 19584 and bound == 23500
        rng = np.random.default_rng(3)
        best = 0
        u = int(np.argmax(gain / D))
        s = np.sign(W[u])
        patterns = [255 * np.outer(s, s), -255 * np.outer(s, s)] + [255 * rng.choice([-1, 1], (n, n)) for _ in range(20000)]
        for x in patterns:
            a = np.ascontiguousarray(x.reshape(-1), np.int32)
            o = np.empty(n * n, np.int32)
            f(a.ctypes.data, o.ctypes.data)
            best = max(best, int(np.abs(o).max()))
            assert np.array_equal(o, _dct(n, a)[0])
        assert best == 23500
    assert 23500 // 4 < 2 ** 15


def test_encoder_qtables_equal_the_restatement(ref):
    """4. mobi_encoder_qtables = SetupQuantizationTables for every quantiser (no device needed); -1 and 54 are refused."""
    from mobiclipdecoder_amd import MobiclipError, load_library, quant_tables
    for q in range(54):
        w4, w8 = np.empty(16, np.float32), np.empty(64, np.float32)
        ref.ref_qtables(q, w4.ctypes.data, w8.ctypes.data)
        g4, g8 = quant_tables(q)
        assert np.array_equal(g4, w4) and np.array_equal(g8, w8), q
        assert np.all(g4 == np.round(g4)) and g4.min() >= 4 and g8.max() <= 7424
    lib = load_library()
    buf = np.empty(64, np.float32)
    for q in (-1, 54):
        assert lib.mobi_encoder_qtables(q, buf.ctypes.data, buf.ctypes.data) == MOBI_E_ARG
        with pytest.raises(MobiclipError):
            quant_tables(q)


def test_restatement_transforms_equal_the_oracle(ref):
    """5. the restatement's DCT and IDCT (with its clamp check) equal mobi_oracle_dct8/4 and mobi_oracle_idct8(64)/idct4(16)"""
    from tests.oracle_binding import lib as oracle_lib
    L = oracle_lib()
    rng = np.random.default_rng(5)
    faults = 0
    for n, fd, fi, var in ((8, L.mobi_oracle_dct8, L.mobi_oracle_idct8, 64), (4, L.mobi_oracle_dct4, L.mobi_oracle_idct4, 16)):
        fd.argtypes = [P, P]
        fd.restype = None
        for trial in range(4000):
            x = np.ascontiguousarray(rng.integers(-255, 256, n * n), np.int32)
            a, b = np.empty(n * n, np.int32), np.empty(n * n, np.int32)
            fd(x.ctypes.data, a.ctypes.data)
            ref.ref_dct(n, x.ctypes.data, b.ctypes.data)
            assert np.array_equal(a, b), trial
            amp = int(rng.choice([50, 800, 6000, 30000]))
            coef = np.ascontiguousarray(rng.integers(-amp, amp + 1, n * n), np.int32)
            pred = np.ascontiguousarray(rng.integers(0, 256, n * n), np.uint8)
            stride = 32
            dst = np.zeros((n + 2) * stride, np.uint8)
            dst.reshape(n + 2, stride)[1:n + 1, 8:8 + n] = pred.reshape(n, n)
            rc = fi(coef.ctypes.data, var, dst.ctypes.data, dst.size, stride + 8, stride)
            out = np.empty(n * n, np.uint8)
            fault = ref.ref_idct(n, coef.ctypes.data, pred.ctypes.data, out.ctypes.data)
            assert (rc != 0) == (fault != 0), trial
            faults += fault
            if not fault:
                assert np.array_equal(out, dst.reshape(n + 2, stride)[1:n + 1, 8:8 + n].reshape(-1)), trial
    assert faults > 100


def test_argument_checks_need_no_device():
    """11 (the refusals): every MOBI_E_ARG case, on both entry points, is decided before the device is touched"""
    from mobiclipdecoder_amd import load_library
    lib = load_library()
    b = np.zeros(64, np.uint8)
    bits, flags = np.zeros(4, np.int32), np.zeros(4, np.uint8)
    q1, q54 = (C.c_int * 1)(12), (C.c_int * 54)(*range(54))

    def call(n=8, qs=q1, nq=1, src=b.ctypes.data, pred=b.ctypes.data, nb=1, bits_p=bits.ctypes.data, flags_p=flags.ctypes.data):
        r1 = lib.mobi_transform_code(0, n, qs, nq, src, pred, nb, None, None, bits_p, None, flags_p)
        r2 = lib.mobi_transform_code_async(0, None, n, qs, nq, src, pred, nb, None, None, bits_p, None, flags_p)
        assert r1 == r2
        return r1

    assert call(n=5) == MOBI_E_ARG and call(n=16) == MOBI_E_ARG and call(n=0) == MOBI_E_ARG
    assert call(nq=0) == MOBI_E_ARG and call(qs=q54, nq=55) == MOBI_E_ARG and call(qs=None) == MOBI_E_ARG
    assert call(qs=(C.c_int * 1)(-1)) == MOBI_E_ARG and call(qs=(C.c_int * 1)(54)) == MOBI_E_ARG
    assert call(qs=(C.c_int * 2)(3, 60), nq=2) == MOBI_E_ARG
    assert call(src=None) == MOBI_E_ARG and call(pred=None) == MOBI_E_ARG
    assert call(bits_p=None) == MOBI_E_ARG and call(flags_p=None) == MOBI_E_ARG
    assert call(qs=(C.c_int * 2)(3, 4), nq=2, nb=2 ** 31) == MOBI_E_ARG  # 2^32 entries
    assert call(qs=q54, nq=54, nb=2 ** 32 // 54 + 1) == MOBI_E_ARG
    # nothing to do: no pointer needed, no device touched
    assert call(src=None, pred=None, bits_p=None, flags_p=None, nb=0) == 0
    from mobiclipdecoder_amd import transform_code
    for bad in ((np.zeros((3, 64), np.int32), np.zeros((3, 64), np.uint8)), (np.zeros((3, 32), np.uint8),) * 2,
                (np.zeros((3, 64), np.uint8), np.zeros((4, 64), np.uint8)), (np.zeros(64, np.uint8),) * 2):
        with pytest.raises(ValueError):
            transform_code(bad[0], bad[1], 12)
    with pytest.raises(ValueError):
        transform_code(np.zeros((3, 64), np.uint8), np.zeros((3, 64), np.uint8), list(range(54)) + [1])


# ---------------------------------------------------------------------------------------------------------------- GPU


def _blocks(rng, nb, n):
    """half uniform noise, half "natural": a smooth prediction and a small residual"""
    nn = n * n
    h = nb // 2
    src = np.empty((nb, nn), np.uint8)
    pred = np.empty((nb, nn), np.uint8)
    src[:h] = rng.integers(0, 256, (h, nn))
    pred[:h] = rng.integers(0, 256, (h, nn))
    m = nb - h
    yy, xx = np.mgrid[0:n, 0:n]
    base = rng.integers(20, 236, (m, 1, 1)) + rng.integers(-4, 5, (m, 1, 1)) * yy + rng.integers(-4, 5, (m, 1, 1)) * xx
    p = np.clip(base + rng.integers(-2, 3, (m, n, n)), 0, 255)
    sigma = rng.choice([1, 3, 8, 20], (m, 1, 1))
    s = np.clip(p + np.round(rng.normal(0, 1, (m, n, n)) * sigma), 0, 255)
    pred[h:] = p.reshape(m, nn)
    src[h:] = s.reshape(m, nn)
    perm = rng.permutation(nb)
    return src[perm], pred[perm]


def _same(got, want, keys=("levels", "recon", "bits", "sad", "flags")):
    ok = (want["flags"] & 2) == 0  # recon / SAD of a clamp fault are unspecified
    for k in keys:
        if k not in got:
            continue
        g, w = np.asarray(got[k]), want[k]
        if k in ("recon", "sad"):
            assert np.array_equal(g[ok], w[ok]), k
        else:
            assert np.array_equal(g, w), (k, np.argwhere(g != w)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 4])
def test_random_blocks_bit_exact(ref, n):
    """6. 100 000 blocks (noise and natural): 2 000 swept over all 54 quantisers in one call, the rest at one quantiser per call"""
    from mobiclipdecoder_amd import transform_code
    rng = np.random.default_rng(600 + n)
    src, pred = _blocks(rng, 100000, n)
    sweep = list(range(54))
    got = transform_code(src[:2000], pred[:2000], sweep)
    want = encode_ref(ref, src[:2000], pred[:2000], sweep)
    _same(got, want)
    assert got["levels"].shape == (54, 2000, n * n) and got["recon"].shape == (54, 2000, n * n) and got["bits"].shape == (54, 2000)
    assert (want["flags"] & 1).any() and not (want["flags"] & 1).all()
    rest = np.array_split(np.arange(2000, 100000), 54)
    for q, idx in zip(rng.permutation(54), rest):
        got = transform_code(src[idx], pred[idx], [int(q)])
        _same(got, encode_ref(ref, src[idx], pred[idx], [int(q)]))


def _tie_blocks(rng, n, parity, want=300):
    """blocks with some d / Q exactly k + 1/2, k of the given parity, at the quantiser returned beside them"""
    from mobiclipdecoder_amd import quant_tables
    out_s, out_p, out_q = [], [], []
    while len(out_s) < want:
        q = int(rng.integers(0, 24))
        Q = np.asarray(quant_tables(q)[0 if n == 4 else 1], np.int64)
        s = rng.integers(0, 256, (4096, n * n))
        p = np.clip(s + rng.integers(-40, 41, (4096, n * n)), 0, 255)
        d = _dct(n, s - p)
        k2 = (2 * np.abs(d)) // Q
        tie = ((2 * np.abs(d)) % Q == 0) & (k2 % 2 == 1) & (((k2 - 1) // 2) % 2 == parity)
        for b in np.flatnonzero(tie.any(1))[: want - len(out_s)]:
            out_s.append(s[b])
            out_p.append(p[b])
            out_q.append(q)
    return np.array(out_s, np.uint8), np.array(out_p, np.uint8), out_q


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 4])
def test_exact_ties_round_to_even(ref, n):
    """7. blocks with d / Q = k + 1/2 exactly, k even and k odd: the levels are the even neighbour, as Math.Round gives"""
    from mobiclipdecoder_amd import transform_code
    rng = np.random.default_rng(700 + n)
    for parity in (0, 1):
        s, p, qs = _tie_blocks(rng, n, parity)
        for q in sorted(set(qs)):
            idx = [i for i, x in enumerate(qs) if x == q]
            got = transform_code(s[idx], p[idx], [q])
            _same(got, encode_ref(ref, s[idx], p[idx], [q]))


def _clamp_cases(ref, rng, n, want=200):
    s_all, p_all, q_all = [], [], []
    found = 0
    while found < want:
        q = int(rng.integers(36, 54))
        nb = 4096
        p = rng.choice([0, 1, 2, 253, 254, 255], (nb, n * n)).astype(np.uint8)
        s = np.where(rng.random((nb, n * n)) < 0.5, 255 - p, p).astype(np.uint8)
        r = encode_ref(ref, s, p, [q])
        hit = np.flatnonzero(r["flags"][0] & 2)[: want - found]
        if hit.size:
            s_all.append(s[hit])
            p_all.append(p[hit])
            q_all += [q] * hit.size
            found += hit.size
    return np.concatenate(s_all), np.concatenate(p_all), q_all


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 4])
def test_clamp_faults_are_flagged_exactly(ref, n):
    """8. entries whose reconstruction leaves the clamp table (found by CPU search at high quantisers) carry MOBI_TC_CLAMP, and only
    they; their levels and bits are still exact.  Mixed with clean blocks in one call."""
    from mobiclipdecoder_amd import transform_code
    rng = np.random.default_rng(800 + n)
    s, p, qs = _clamp_cases(ref, rng, n)
    cs, cp = _blocks(rng, 4 * len(qs), n)
    for q in sorted(set(qs)):
        idx = [i for i, x in enumerate(qs) if x == q]
        S, Pr = np.concatenate([s[idx], cs]), np.concatenate([p[idx], cp])
        got = transform_code(S, Pr, [q, 12, 53])
        want = encode_ref(ref, S, Pr, [q, 12, 53])
        _same(got, want)
        assert (got["flags"][0, : len(idx)] & 2).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 4])
def test_uncoded_blocks(ref, n):
    """9. src == pred, and residuals of +-1 at quantiser 53: no level, 0 bits, flags 0, recon == pred, SAD = the residual"""
    from mobiclipdecoder_amd import transform_code
    rng = np.random.default_rng(900 + n)
    p = rng.integers(1, 255, (500, n * n)).astype(np.uint8)
    s = (p.astype(np.int16) + rng.integers(-1, 2, p.shape)).astype(np.uint8)
    for src, qs in ((p, list(range(54))), (s, [53])):
        got = transform_code(src, p, qs)
        _same(got, encode_ref(ref, src, p, qs))
        assert not got["levels"].any() and not got["bits"].any() and not got["flags"].any()
        assert np.array_equal(got["recon"], np.broadcast_to(p, got["recon"].shape))
        assert np.array_equal(got["sad"][0], np.abs(src.astype(np.int32) - p).sum(1))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 4])
def test_block_counts_off_the_workgroup_size(ref, n):
    """10. block counts that are not a multiple of the blocks per workgroup (32 / 64); optional outputs off give the same bits / flags;
    n_blocks = 0 (11)"""
    from mobiclipdecoder_amd import transform_code
    rng = np.random.default_rng(1000 + n)
    for nb in (1, 7, 33, 63, 65, 100, 1025):
        s, p = _blocks(rng, nb, n)
        qs = [int(x) for x in rng.choice(54, 3, replace=False)]
        got = transform_code(s, p, qs)
        want = encode_ref(ref, s, p, qs)
        _same(got, want)
        lean = transform_code(s, p, qs, levels=False, recon=False, sad=False)
        assert set(lean) == {"bits", "flags"}
        _same(lean, want)
    z = transform_code(np.zeros((0, n * n), np.uint8), np.zeros((0, n * n), np.uint8), [5, 6])
    assert z["bits"].shape == (2, 0) and z["levels"].shape == (2, 0, n * n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 4])
def test_async_on_torch_tensors_orders_after_the_stream(ref, n):
    """12. torch GPU tensors go through mobi_transform_code_async on torch's current stream: the same as the host entry point, and it
    reads what a torch kernel enqueued just before it on that stream wrote (also on a side stream)"""
    import torch
    from mobiclipdecoder_amd import transform_code
    rng = np.random.default_rng(1200 + n)
    nb = 1 << 18
    s, p = _blocks(rng, nb, n)
    qs = [12, 30, 40]
    want = transform_code(s, p, qs)
    dev = torch.device("cuda", torch.cuda.current_device())
    side = torch.cuda.Stream(dev)
    for stream in (torch.cuda.current_stream(dev), side):
        with torch.cuda.stream(stream):
            pt = torch.from_numpy(p).to(dev)
            s32 = torch.from_numpy(s.astype(np.int32)).to(dev)
            st = torch.zeros(s.shape, dtype=torch.uint8, device=dev)
            slow = torch.ones((2048, 2048), device=dev) / 2048
            for _ in range(8):
                slow = slow @ slow
            # src is written by a torch kernel that waits for the matrix products; no synchronisation before the call
            st.copy_((s32 + (slow[0, 0] * 0).to(torch.int32)).to(torch.uint8))
            got = transform_code(st, pt, qs)
        stream.synchronize()
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got.values())
        for k in want:
            assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    _same({k: v[:, :4096] for k, v in want.items()}, encode_ref(ref, s[:4096], p[:4096], qs))
