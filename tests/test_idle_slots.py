"""Idle frame slots (mobi_batch_set_idle, mobi_batch_clip_idle; mobi_idle.hip): clips whose stream has ended sit out the rest of a step or
group -- not parsed, not handed to the host parser, no state changed, no pixel written -- while every live frame of every clip stays what
the oracle gives for its stream.  640x480 Moflex3DS and 256x192 ModsDS, the generator's streams cut to unequal lengths (one clip never
starts, some end inside a group, one ends on a group boundary, one is of the hybrid mode's host share), on every decode path and in every
parse mode; against the empty-packet way of sitting out (the present behaviour: a damaged stream, handed to the host parser); with the
ring-index rule of mobiclip_hip.h, refills, damage in other clips, the refusals and the launch counter."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401 -- before the product library is loaded: torch tensors need torch's HIP runtime to be the library's too

from mobiclipdecoder_amd import MOBI_IDLE, MobiclipBatch, MobiclipError, default_params, generate_clip
from mobiclipdecoder_amd.streamgen import BASE_SEED
from tests.oracle_binding import OracleDecoder

pytestmark = pytest.mark.gpu

GEOMS = [(640, 480, 2), (256, 192, 1)]  # Moflex3DS; ModsDS (Width == Stride: the raster-order intra launch in groups)
N, T = 10, 14
LENGTHS = [14, 3, 9, 0, 11, 14, 12, 5, 14, 10]  # live frames per clip; parse mode 2: the host share is clips 8 and 9
SHARE = {0: 0, 1: 0, 2: N // 5, 3: 0}           # mobi_batch_host_clips without any hand-over, by parse mode (0: not compared, all clips)
EMPTY = np.zeros(0, np.uint8)
IDLE_OFFSET = 1234                               # handed in for idle slots: must come back unchanged


@functools.lru_cache(maxsize=None)
def _streams(geom, salt=0, n_frames=T):
    W, H, version = geom
    out = []
    for c in range(N):
        p = default_params("AB"[c % 2], BASE_SEED + 52000 + 131 * c + salt, width=W, height=H, version=version, n_frames=n_frames, iframe_interval=5 + c % 3,
                           pm_intra=60 + 20 * (c % 4), qdelta_prob=300)
        d, fo = generate_clip(p)
        out.append([d[fo[f]:fo[f + 1]] for f in range(n_frames)])
    return out


@functools.lru_cache(maxsize=None)
def _oracle(geom, salt=0, n_frames=T):
    """[c][t] -> (rc, offset, Y, UV, quantizer)"""
    W, H, version = geom
    exp = []
    for pk in _streams(geom, salt, n_frames):
        o = OracleDecoder(W, H, version)
        rows = []
        for d in pk:
            o.Data, o.Offset = d, 0
            o.DecodeFrame()
            assert o.last_error == 0
            rows.append((0, o.Offset, o.y(0).ravel(), o.uv(0).ravel(), o.Quantizer))
        o.close()
        exp.append(rows)
    return exp


def _units(path, K):
    if path in ("decode", "submit"):
        return [1] * T
    if path == "pipe":
        return [2, 9, 3]  # the group of nine is finished in two parts; clips 2 and 9 go idle in its second part, clip 4 on the boundary behind it
    return [K] * (T // K) + ([T % K] if T % K else [])


def _drive(geom, mode, path, K=1, masked=True, lengths=LENGTHS, streams=None, check=None):
    """one batch through the whole schedule.  masked: ended clips' slots are marked idle (data None); else they are fed empty packets.
    -> res[(c, t)] = (rc, offset, Y, UV), quant[(c, t)] (where the call reported frame t last), log = [(frames handed over, host_clips)],
    the batch's idle_launches, hand-overs that had an idle slot"""
    W, H, version = geom
    pk = streams or _streams(geom)
    b = MobiclipBatch(N, W, H, version, device_parse=mode)
    res, quant, log = {}, {}, []
    with_idle = 0

    def hand(t0, Kc):
        nonlocal with_idle
        frames = [[pk[c][t0 + k] if t0 + k < lengths[c] else (None if masked else EMPTY) for c in range(N)] for k in range(Kc)]
        offs = [[0 if t0 + k < lengths[c] else IDLE_OFFSET for c in range(N)] for k in range(Kc)]
        mask = np.array([[t0 + k >= lengths[c] for c in range(N)] for k in range(Kc)])
        if masked and mask.any():
            b.set_idle(mask if path not in ("decode", "submit") else mask[0])
            with_idle += 1
        return frames, offs

    def report(t, rcs, offs, ring_idx, last):
        for c in range(N):
            y, uv = b.planes(c, ring_idx)
            res[(c, t)] = (rcs[c], offs[c], y.ravel().copy(), uv.ravel().copy())
            if last:
                quant[(c, t)] = b.quantizer(c)

    units, t, handed = _units(path, K), 0, 0
    if path == "decode":
        for _ in units:
            frames, offs = hand(t, 1)
            rcs, o = b.decode(frames[0], offs[0])
            handed += 1
            log.append((handed, b.host_clips()))
            report(t, rcs, o, 0, True)
            t += 1
    elif path == "submit":
        for s in range(T + 1):  # two steps in flight
            if s < T:
                frames, offs = hand(s, 1)
                b.submit(frames[0], offs[0])
                handed += 1
                log.append((handed, b.host_clips()))
            if s >= 1:
                rcs, o = b.wait()
                report(s - 1, rcs, o, 1 if s < T else 0, True)
    elif path == "gop":
        for Kc in units:
            frames, offs = hand(t, Kc)
            rcs, o = b.decode_gop(frames, offs)
            handed += Kc
            log.append((handed, b.host_clips()))
            for k in range(Kc):
                report(t + k, rcs[k], o[k], Kc - 1 - k, k == Kc - 1)
            if check:
                check(b, t + Kc)
            t += Kc
    else:  # two groups begun
        pending = []

        def finish():
            t0, Kc = pending.pop(0)
            done = 0
            while done < Kc:
                rcs, o = b.gop_finish()
                P = len(rcs)
                for j in range(P):
                    report(t0 + done + j, rcs[j], o[j], P - 1 - j, j == P - 1)
                done += P
        for Kc in units:
            frames, offs = hand(t, Kc)
            b.gop_begin(frames, offs)
            handed += Kc
            log.append((handed, b.host_clips()))
            pending.append((t, Kc))
            t += Kc
            if len(pending) == 2:
                finish()
        while pending:
            finish()
    launches = b.idle_launches()
    idle_now = b.clip_idle().tolist()
    frames_now = b.clip_frames().tolist()
    b.close()
    return res, quant, log, launches, with_idle, idle_now, frames_now


def _check_exact(geom, res, quant, lengths=LENGTHS, exp=None):
    exp = exp or _oracle(geom)
    for (c, t), (rc, off, y, uv) in res.items():
        if t < lengths[c]:
            e = exp[c][t]
            assert (rc, off) == (e[0], e[1]), (c, t, rc, off)
            assert np.array_equal(y, e[2]) and np.array_equal(uv, e[3]), f"clip {c} frame {t} differs from the oracle"
        else:
            assert (rc, off) == (MOBI_IDLE, IDLE_OFFSET), (c, t, rc, off)
    for (c, t), q in quant.items():
        if lengths[c]:  # Quantizer stays that of the clip's last live frame
            assert q == exp[c][min(t, lengths[c] - 1)][4], (c, t, q)


PATHS = [("decode", 1), ("submit", 1), ("gop", 1), ("gop", 3), ("gop", 6), ("pipe", 0)]
# (mobi_batch_submit and mobi_batch_gop_begin have no host-parsed form: parse mode 0 goes through decode and decode_gop)
MODE_PATHS = [(m, p, K) for m in (0, 1, 2, 3) for p, K in PATHS if m or p in ("decode", "gop")]


def _host_clips_expected(mode, handed):
    """the parse mode's own share, less its clips whose stream has ended (an ended clip is not counted: mobiclip_hip.h)"""
    return sum(1 for c in range(N - SHARE[mode], N) if LENGTHS[c] >= handed)


# ---- 1. every live frame is the oracle's, on every path, in every parse mode ---------------------------------------------------------
@pytest.mark.parametrize("mode,path,K", MODE_PATHS)
@pytest.mark.parametrize("geom", GEOMS)
def test_live_frames_equal_the_oracle_and_idle_slots_report_idle(geom, mode, path, K):
    res, quant, log, launches, with_idle, idle_now, frames_now = _drive(geom, mode, path, K)
    assert len(res) == N * T
    _check_exact(geom, res, quant)
    assert idle_now == [T - L for L in LENGTHS] and frames_now == LENGTHS
    if mode:  # 3. no hand-over: an ended clip is nobody's to parse, nobody else went to the host parser
        for handed, hc in log:
            assert hc == _host_clips_expected(mode, handed), (handed, hc)
    assert launches == (with_idle if mode else 0), "one launch of mobi_idle_rows per device-parsed hand-over that has idle slots"


# ---- 2. + 3. the same pictures as the empty-packet way, which goes through the host parser ---------------------------------------------
@pytest.mark.parametrize("path,K", [("decode", 1), ("gop", 3), ("pipe", 0)])
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("geom", GEOMS)
def test_same_pictures_as_empty_packets_without_the_hand_over(geom, mode, path, K):
    a = _drive(geom, mode, path, K, masked=True)
    e = _drive(geom, mode, path, K, masked=False)
    for (c, t), (rc, off, y, uv) in a[0].items():
        if t < LENGTHS[c]:
            erc, eoff, ey, euv = e[0][(c, t)]
            assert (rc, off) == (erc, eoff) and np.array_equal(y, ey) and np.array_equal(uv, euv), (c, t)
        else:
            assert e[0][(c, t)][0] == -1  # MOBI_E_INDEX: an empty packet is a damaged stream
    for (c, t), q in a[1].items():
        if t < LENGTHS[c]:
            assert q == e[1][(c, t)], (c, t)
    share = SHARE[mode]
    for handed, hc in a[2]:
        assert hc == _host_clips_expected(mode, handed), (handed, hc)
    assert max(hc for _, hc in e[2]) > share, "the empty-packet batch hands its ended clips to the host parser: the yardstick of this test"
    assert e[3] == 0  # and never launches the idle kernel


# ---- 4. where the pictures are -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("geom", GEOMS)
def test_ring_index_rule_with_getters_and_device_export(geom, mode):
    W, H, version = geom
    exp = _oracle(geom)

    def check(b, handed):
        idle, frames = b.clip_idle(), b.clip_frames()
        S = b.Stride
        part = b.export_tensor("i420", ring_idx=5, n_frames=6).cpu().numpy() if handed >= 6 else None  # picture j = ring index 5 - j
        torch.cuda.synchronize()
        for c in range(N):
            live = min(LENGTHS[c], handed)
            assert idle[c] == handed - live and frames[c] == live, (c, handed, idle[c], frames[c])
            for r in range(min(6, handed)):
                y, uv = b.planes(c, r)  # (delivered whether the rule holds or not: batch-wide checks)
                if not idle[c] <= r < min(6, idle[c] + frames[c]):
                    continue
                e = exp[c][live - 1 - (r - idle[c])]
                assert np.array_equal(y.ravel(), e[2]) and np.array_equal(uv.ravel(), e[3]), (c, handed, r)
                if part is not None:
                    ey, euv = e[2].reshape(H, S), e[3].reshape(H // 2, S)
                    i420 = np.concatenate([ey[:, :W].ravel(), euv[:, :W // 2].ravel(), euv[:, S // 2:S // 2 + W // 2].ravel()])
                    assert np.array_equal(part[5 - r, c], i420), (c, handed, r)

    _drive(geom, mode, "gop", 6, check=check)


# ---- 5. refill: idle, reset with the group still in flight, a new stream --------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("geom", GEOMS)
def test_refill_after_idle_with_the_previous_group_in_flight(geom, mode):
    W, H, version = geom
    pk, exp = _streams(geom), _oracle(geom)
    pk2, exp2 = _streams(geom, 7, 6), _oracle(geom, 7, 6)
    refill = [c for c in range(N) if LENGTHS[c] < 6]  # clips 1, 3, 7: ended inside (or before) the first group
    b = MobiclipBatch(N, W, H, version, device_parse=mode)
    b.set_idle([[k >= LENGTHS[c] for c in range(N)] for k in range(6)])
    b.gop_begin([[pk[c][k] if k < LENGTHS[c] else None for c in range(N)] for k in range(6)])
    assert b.clip_idle().tolist() == [max(0, 6 - L) for L in LENGTHS]
    b.reset_clips(refill)  # the first group is still in flight
    b.gop_begin([[pk2[c][k] if c in refill else pk[c][6 + k] for c in range(N)] for k in range(6)])
    assert b.clip_idle().tolist() == [0] * N
    for g in range(2):
        rcs, offs = b.gop_finish()
        for k in range(6):
            for c in range(N):
                if g == 0 and k >= LENGTHS[c]:
                    assert rcs[k][c] == MOBI_IDLE
                    continue
                e = exp[c][6 * g + k] if g == 0 or c not in refill else exp2[c][k]
                y, uv = b.planes(c, 5 - k)
                assert (rcs[k][c], offs[k][c]) == (e[0], e[1]), (g, k, c)
                assert np.array_equal(y.ravel(), e[2]) and np.array_equal(uv.ravel(), e[3]), (g, k, c)
    assert b.clip_idle().tolist() == [0] * N and b.clip_frames().tolist() == [6 if c in refill else 12 for c in range(N)]
    assert b.host_clips() == SHARE[mode]
    b.close()


# ---- 6. with damage in other clips ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["pipe", "submit"])
@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("geom", GEOMS)
def test_damaged_clips_are_repaired_as_without_idle_slots(geom, mode, path):
    rng = np.random.default_rng(0x1D1E)
    damaged = [0, 5, 8]  # live throughout
    pk = [list(s) for s in _streams(geom)]
    for c in damaged:
        for t in (4, 10):
            d = pk[c][t].copy()
            for _ in range(6):
                d[int(rng.integers(2, d.size))] ^= 1 << int(rng.integers(0, 8))
            pk[c][t] = d
    a = _drive(geom, mode, path, streams=pk, masked=True)
    full = _drive(geom, mode, path, streams=pk, lengths=[T] * N)  # no idle slot anywhere: every clip live to the end
    for c in damaged:
        for t in range(T):
            (rc, off, y, uv), (frc, foff, fy, fuv) = a[0][(c, t)], full[0][(c, t)]
            assert (rc, off) == (frc, foff), (c, t)
            if path == "pipe" or rc == 0:  # (mobi_batch_wait: the slot of a frame whose repaired parse is rejected is unspecified, mobiclip_hip.h)
                assert np.array_equal(y, fy) and np.array_equal(uv, fuv), (c, t)
    assert [hc for _, hc in a[2]] == [hc for _, hc in full[2]]  # the same clips went to the host parser at the same hand-overs
    for c in range(N):  # and the clips with idle slots did not notice the damage next to them
        if c not in damaged:
            for t in range(LENGTHS[c]):
                assert a[0][(c, t)][0] == 0 and np.array_equal(a[0][(c, t)][2], full[0][(c, t)][2])
            for t in range(LENGTHS[c], T):
                assert a[0][(c, t)][0] == MOBI_IDLE


# ---- 7. refusals, each leaving the batch usable ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 3])
@pytest.mark.parametrize("geom", GEOMS)
def test_refusals_leave_the_batch_usable(geom, mode):
    W, H, version = geom
    pk, exp = _streams(geom), _oracle(geom)
    b = MobiclipBatch(N, W, H, version, device_parse=mode)
    group = lambda t0, K, idle=(): [[None if (k, c) in idle else pk[c][t0 + k] for c in range(N)] for k in range(K)]
    mask = lambda K, idle: np.array([[(k, c) in idle for c in range(N)] for k in range(K)])

    def exact(rcs, offs, t0, K, idle=()):
        for k in range(K):
            for c in range(N):
                if (k, c) in idle:
                    assert rcs[k][c] == MOBI_IDLE
                    continue
                e = exp[c][t0 + k]
                y, uv = b.planes(c, K - 1 - k)
                assert (rcs[k][c], offs[k][c]) == (e[0], e[1]) and np.array_equal(y.ravel(), e[2]) and np.array_equal(uv.ravel(), e[3]), (t0, k, c)

    # a mask of the wrong n_frames: refused, the mask stays and serves the group it was made for
    idle = {(1, 2), (2, 2)}
    b.set_idle(mask(3, idle))
    with pytest.raises(MobiclipError):
        b.decode_gop(group(0, 2, idle))
    exact(*b.decode_gop(group(0, 3, idle)), 0, 3, idle)
    assert b.clip_idle()[2] == 2 and b.clip_frames()[2] == 1
    # a live frame for the ended clip without a reset: refused with a mask that leaves it live, and without any mask
    with pytest.raises(MobiclipError):
        b.decode_gop(group(3, 2))
    b.set_idle(mask(2, {(1, 4)}))
    with pytest.raises(MobiclipError):
        b.decode_gop(group(3, 2, {(1, 4)}))
    b.set_idle(None)
    # idle slots that are not a suffix
    gap = {(0, 2), (1, 2), (0, 6)}
    b.set_idle(mask(2, gap))
    with pytest.raises(MobiclipError):
        b.decode_gop(group(3, 2, gap))
    # a correct hand-over right after succeeds and is exact; nothing of the refused ones was booked
    ok = {(0, 2), (1, 2)}
    b.set_idle(mask(2, ok))
    exact(*b.decode_gop(group(3, 2, ok)), 3, 2, ok)
    assert b.clip_idle().tolist() == [4 if c == 2 else 0 for c in range(N)]
    assert b.clip_frames().tolist() == [1 if c == 2 else 5 for c in range(N)]
    b.close()


# ---- 8. nothing added when unused --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,K", [("decode", 1), ("submit", 1), ("gop", 3), ("pipe", 0)])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_no_mask_no_launch(mode, path, K):
    geom = GEOMS[1]
    res, quant, log, launches, with_idle, idle_now, frames_now = _drive(geom, mode, path, K, lengths=[T] * N)
    assert launches == 0 and with_idle == 0 and idle_now == [0] * N and frames_now == [T] * N
    _check_exact(geom, res, quant, lengths=[T] * N)
