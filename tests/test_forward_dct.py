"""mobi_fwd_dct8 / mobi_fwd_dct4 (csrc/mobi_analysis.hip) on EVERY block of runs whose block count does and does not fill the workgroups.

The passes themselves are pinned through mobi_txcode; what is pinned here is these two kernels' own indexing: the block of a lane inside
its workgroup (32 blocks of 8 lanes, 64 blocks of 4), the LDS transpose and its pitch, and the `on` predicate of a workgroup that is only
partly occupied.

  * CPU: a vectorised int64 numpy statement of MobiEncoder.DCT64 / DCT16 (input x 64, the row pass with C#'s truncating division, the
    column pass with the result stored transposed) equals the reference's vectors (tests/golden/unit_vectors.npz) and the oracle's scalar
    restatement on a few thousand random blocks and on every special block used below.
  * GPU: that statement is the reference for all blocks of every run.  The input lies in the middle of a larger sentinel-filled host array
    and the output array is longer than the run: neither the caller's input nor the words behind the last block may change.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests.oracle_binding import lib as oracle_lib
from tests.test_txcode import D4, D8, W4, W8  # the reference's weights and divisors per output (MobiEncoder.cs:970-1008, 1154-1176)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPZ = os.path.join(ROOT, "tests", "golden", "unit_vectors.npz")
COUNTS = [1, 7, 31, 32, 33, 63, 64, 65, 100, 3001]  # around 32 blocks (dct8) and 64 blocks (dct4) per workgroup; 3001 = 93 * 32 + 25 = 46 * 64 + 57
SENTINEL_IN, SENTINEL_OUT = 0x5A5A1234, 0x7B7B4321
PAD = 4096  # words of sentinel on either side of the input: more than a workgroup's worth of blocks (32 * 64 = 64 * 16 * 2 = 2048)


def _tdiv(a, d):
    """C# integer division: the quotient truncated towards zero (numpy's // floors)"""
    return np.sign(a) * (np.abs(a) // d)


def dct_numpy(n, blocks):
    """MobiEncoder.DCT64 (n = 8) / DCT16 (n = 4) for an array of blocks, int64 throughout.  blocks: (count, n * n), row-major residuals."""
    W, D = ((W8, D8) if n == 8 else (W4, D4))
    W, D = W.astype(np.int64), D.astype(np.int64)
    x = np.asarray(blocks, np.int64).reshape(-1, n, n) * 64
    t = _tdiv(np.einsum("uj,bij->biu", W, x), D)          # rows: t[b][i][u] = output u of row i
    o = _tdiv(np.einsum("uj,bji->biu", W, t), D)          # columns: output u of column i is stored at [i][u] -- transposed, as the reference does
    return o.reshape(-1, n * n)


def special_blocks(n):
    """The blocks every run draws from: the extremes, the alternations, every single-sample block"""
    nn = n * n
    r, c = np.divmod(np.arange(nn), n)
    out = [np.full(nn, 255), np.full(nn, -255), np.where(r % 2, 255, -255), np.where(c % 2, 255, -255), np.where((r + c) % 2, 255, -255),
           np.where((r + c) % 2, -255, 255), np.zeros(nn, np.int64)]
    for k in range(nn):
        e = np.zeros(nn, np.int64)
        e[k] = 255 if k % 2 else -255
        out.append(e)
    return np.array(out, np.int32)


def make_blocks(n, count, seed):
    """`count` blocks: random residuals in [-255, 255]; from block 1 on, every third block is its predecessor with ONE sample changed (a
    lane that reads its neighbour's input or LDS rows gives the neighbour's answer); the special blocks are dealt over the rest, starting
    at a place that depends on `count` so that the short runs see different ones and the long run sees all of them."""
    nn = n * n
    rng = np.random.default_rng(seed)
    x = rng.integers(-255, 256, (count, nn)).astype(np.int32)
    sp = special_blocks(n)
    for i in range(count):
        if i % 3 == 1:
            x[i] = x[i - 1]
            k = int(rng.integers(0, nn))
            x[i, k] = -x[i, k] if x[i, k] else 77
        elif i % 3 == 2:
            x[i] = sp[(i // 3 + 5 * count) % len(sp)]
    return x


def _oracle_dct(n, x):
    L = oracle_lib()
    f = L.mobi_oracle_dct8 if n == 8 else L.mobi_oracle_dct4
    f.argtypes = [C.c_void_p, C.c_void_p]
    f.restype = None
    x = np.ascontiguousarray(x, np.int32)
    out = np.empty_like(x)
    for i in range(len(x)):
        f(x[i].ctypes.data, out[i].ctypes.data)
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU


@pytest.mark.parametrize("n", [8, 4])
def test_numpy_statement_equals_the_reference_vectors_and_the_oracle(n):
    V = np.load(NPZ)
    assert np.array_equal(dct_numpy(n, V[f"dct{n}_in"]), V[f"dct{n}_out"])
    x = np.concatenate([special_blocks(n), make_blocks(n, 3001, 11 + n)])
    want = _oracle_dct(n, x)
    got = dct_numpy(n, x)
    assert got.dtype == np.int64 and np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    # the statement is not a symmetric one: a version that forgot the transposed store would differ
    assert not np.array_equal(got.reshape(-1, n, n), got.reshape(-1, n, n).transpose(0, 2, 1))


def test_the_runs_contain_what_they_claim():
    for n in (8, 4):
        sp = special_blocks(n)
        big = make_blocks(n, COUNTS[-1], 100 + n)
        assert all((big == s).all(1).any() for s in sp)  # the long run holds every special block
        k = len(big[1::3])
        assert ((big[1::3] != big[0::3][:k]).sum(1) == 1).all()  # neighbours that differ in exactly one sample
        assert COUNTS[-1] % 32 and COUNTS[-1] % 64 and big.min() == -255 and big.max() == 255


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 4])
def test_gpu_every_block_of_every_count(n):
    from mobiclipdecoder_amd.decoder import default_device, load_library
    lib = load_library()
    nn = n * n
    for count in COUNTS:
        x = make_blocks(n, count, 100 + n if count == COUNTS[-1] else 1000 * n + count)
        host = np.full(2 * PAD + count * nn, SENTINEL_IN, np.int32)
        host[PAD:PAD + count * nn] = x.ravel()
        before = host.copy()
        extra = 70  # blocks of fill behind the run: more than one workgroup of either kernel
        out = np.full((count + extra, nn), SENTINEL_OUT, np.int32)
        rc = lib.mobi_forward_dct(default_device(), n, host[PAD:].ctypes.data, out.ctypes.data, count)
        assert rc == 0, (n, count, rc)
        assert np.array_equal(host, before), ("the input was written", n, count)
        assert (out[count:] == SENTINEL_OUT).all(), ("written behind the last block", n, count, np.argwhere(out[count:] != SENTINEL_OUT)[:5].tolist())
        want = dct_numpy(n, x)
        bad = np.flatnonzero((out[:count] != want).any(1))
        assert bad.size == 0, (n, count, "blocks", bad[:10].tolist(), "block in workgroup", (bad[:10] % (32 if n == 8 else 64)).tolist(),
                               out[bad[0]].tolist(), want[bad[0]].tolist())
