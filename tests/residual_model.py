"""The residual stage written down twice in numpy (TEST INFRASTRUCTURE, no GPU): the inverse transforms of MD.cs:3435-3798 in int64, and
the same with every intermediate wrapped to int16 in the operation order of bfly8_pk / bfly4_pk (csrc/mobi_kernels.hip) -- what the packed
rounds of mobi_recon_inter8 compute.  tests/test_residual_edges.py checks the kernels' MOBI_PK_LIMIT with it and looks for its directed
streams with it; tools/fuzz_inter_gpu.py --scripted draws its levels from the same tables."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mobiclipdecoder_amd", "csrc")


def _table(name):
    text = open(os.path.join(CSRC, "mobi_tables.h")).read()
    m = re.search(r"\b%s\[\d+\]\s*=\s*\{([^}]*)\}" % name, text)
    return np.array([int(v) for v in m.group(1).replace("\n", " ").split(",") if v.strip()], np.int64)


ZZ8, ZZ4, DQ8, DQ4, QDIV6, QMOD6 = (_table("mobi_" + n) for n in ("zz8", "zz4", "dq8", "dq4", "qdiv6", "qmod6"))


def pk_limit():
    """MOBI_PK_LIMIT as the kernel source has it"""
    m = re.search(r"#define\s+MOBI_PK_LIMIT\s+(\d+)", open(os.path.join(CSRC, "mobi_kernels.hip")).read())
    return int(m.group(1))


def scales(q, n):
    """dequant scale by SCAN position of the n x n transform at quantizer q (SetupQuantizationTables, MD.cs:3897-3912)"""
    sh, m = int(QDIV6[q]) + 8, int(QMOD6[q])
    if n == 4:
        return (DQ4[16 * m:16 * m + 16] << sh) >> 8
    return (DQ8[64 * m:64 * m + 64] << (sh - 2)) >> 8


def zz(n):
    return ZZ8 if n == 8 else ZZ4


def _w16(x):
    return ((x + 32768) & 0xFFFF) - 32768


def _same(x):
    return x


def _bfly8(i, w):
    a0, a1 = w(i[0] + i[4]), w(i[0] - i[4])
    a2, a3 = w(i[2] + (i[6] >> 1)), w((i[2] >> 1) - i[6])
    e0, e1, e2, e3 = w(a0 + a2), w(a1 + a3), w(a1 - a3), w(a0 - a2)
    b0 = w(w(w(i[1] + i[7]) - i[3]) - (i[3] >> 1))
    b1 = w(w(w(i[7] - i[1]) + i[5]) + (i[5] >> 1))
    b2 = w(w(i[5] - w(i[7] + (i[7] >> 1))) - i[3])
    b3 = w(w(w(i[3] + i[5]) + i[1]) + (i[1] >> 1))
    o0, o3 = w(b2 + (b3 >> 2)), w(b3 - (b2 >> 2))
    o1, o2 = w(b0 + (b1 >> 2)), w((b0 >> 2) - b1)
    return [w(e0 + o3), w(e1 + o2), w(e2 + o1), w(e3 + o0), w(e3 - o0), w(e2 - o1), w(e1 - o2), w(e0 - o3)]


def _bfly4(i, w):
    a, b = w(i[0] + i[2]), w(i[0] - i[2])
    c, d = w((i[1] >> 1) - i[3]), w(i[1] + (i[3] >> 1))
    return [w(a + d), w(b + c), w(b - c), w(a - d)]


def idct(coef, n, wrap16=False):
    """coef: (B, n * n) dequantised coefficients in natural order -> (B, n, n) residuals (after the >> 6).  Pass 1 takes coefficient group k
    (+32 on the first coefficient of group 0) and hands its output m over TRANSPOSED, to [m][k]; pass 2 takes row i.  wrap16: the
    coefficients are stored as int16 and every sum, difference and shift result wraps to int16, as v_pk_add_i16 and its kin do."""
    w = _w16 if wrap16 else _same
    bf = _bfly8 if n == 8 else _bfly4
    c = w(np.asarray(coef, np.int64).reshape(-1, n, n))
    rows = [[c[:, k, m] for m in range(n)] for k in range(n)]
    rows[0][0] = w(rows[0][0] + 32)
    p1 = [bf(rows[k], w) for k in range(n)]           # p1[k][m] -> t[m][k]
    p2 = [bf([p1[k][i] for k in range(n)], w) for i in range(n)]
    return np.stack([np.stack([p2[i][j] >> 6 for j in range(n)], -1) for i in range(n)], -2)
