"""The receive planner's rule on the CPU (srtp_rx_plan_host, the host twin
of re_amd/csrc/hip/plan_rx.hip: the same functions of plan_rx_rule.h in the
same block decomposition) against the oracle receiver.

Truth: about 600 packets of 16-byte payload are protected in order with
oracle_srtp_encrypt; the reshaped arrival order (swaps, displacement,
duplicates, loss, forward jumps, a packet from before a rollover after it)
is fed to oracle_srtp_decrypt one call at a time.  The rule must either
report the batch unsettled (fail != 0) or give the oracle's errno for every
packet and its final (roc, s_l, lix, bitmap): a wrong settled answer is
never allowed.  Small block / lookback values put a block boundary and a
look-back boundary next to every shape.
"""
import ctypes
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import oracle_lib as O

SUITE = 1
KEY = bytes((11 * i + 3) & 0xff for i in range(30))
SSRC = 0x5150
N = 600
BLOCKS = (4, 8, 64)
LOOKBACKS = (2, 4, 128)
S0S = (100, 32700, 65000)


def packet(seq, k):
    hdr = bytes([0x80, 96, (seq >> 8) & 0xff, seq & 0xff]) + \
        (1000 + k).to_bytes(4, "big") + SSRC.to_bytes(4, "big")
    return hdr + bytes((k + j) & 0xff for j in range(16))


def protect(be, seqs):
    """the packets of sequence numbers seqs, protected in that order"""
    ctx, err = be.alloc(SUITE, KEY, 0)
    assert err == 0
    out = []
    for k, seq in enumerate(seqs):
        p = packet(seq & 0xffff, k)
        e, _, en, _, buf = be.call(ctx, "srtp_encrypt", 256, 0, len(p), p, 0)
        assert e == 0
        out.append(buf[:en])
    be.free(ctx)
    return out


def seq_of(pkt):
    return pkt[2] << 8 | pkt[3]


class Receiver:
    """the oracle receiver, one srtp_decrypt call per arrival"""

    def __init__(self, be):
        self.be = be
        self.ctx, err = be.alloc(SUITE, KEY, 0)
        assert err == 0

    def feed(self, pkts):
        return [self.be.call(self.ctx, "srtp_decrypt", 256, 0, len(p), p,
                             0)[0] for p in pkts]

    def state(self):
        return self.be.export(self.ctx, SSRC)

    def close(self):
        self.be.free(self.ctx)


def stream_state(st=None):
    s = P.StreamState()
    s.ssrc = SSRC
    if st is not None:
        s.roc, s.s_l, s.replay_rtp_lix, s.replay_rtp_bitmap = st
        s.s_l_set = 1
    return s


@pytest.fixture(scope="module")
def be():
    P.load()
    return O.OracleBackend()


@pytest.fixture(scope="module")
def sent(be):
    """per s0: the in-order protected stream (shared, never modified)"""
    return {s0: protect(be, [s0 + k for k in range(N)]) for s0 in S0S}


def verdicts(be, arrivals, first=None):
    """oracle truth of a batch: (state before, errnos, state after); first:
    a batch received before it (continuing state)"""
    rx = Receiver(be)
    st0 = None
    if first is not None:
        rx.feed(first)
        st0 = rx.state()
    errs = rx.feed(arrivals)
    fin = rx.state()
    rx.close()
    return st0, errs, fin


def sweep(truth, arrivals, blocks=BLOCKS, lookbacks=LOOKBACKS):
    """the rule over every (block, lookback): {(block, lookback): settled};
    a settled plan must equal the oracle"""
    st0, errs, fin = truth
    seq = np.array([seq_of(p) for p in arrivals], dtype=np.uint16)
    out = {}
    for b in blocks:
        for lb in lookbacks:
            fail, ix, err, st1 = P.rx_plan_host(stream_state(st0), seq, b, lb)
            out[(b, lb)] = not fail
            if fail:
                assert (st1.roc, st1.s_l, st1.s_l_set) == \
                    ((st0[0], st0[1], 1) if st0 else (0, 0, 0))
                continue
            assert err.tolist() == errs, (b, lb, [
                (i, int(err[i]), errs[i]) for i in range(len(errs))
                if err[i] != errs[i]][:5])
            got = (st1.roc, st1.s_l, st1.replay_rtp_lix,
                   st1.replay_rtp_bitmap)
            assert got == fin, (b, lb, got, fin)
            assert st1.s_l_set == 1
            assert ((ix & 0xffff) == seq).all()
    return out


# ---- shapes: arrival orders as lists of send positions ------------------

def swaps_at_block_boundaries():
    a = list(range(N))
    for k in (4, 8, 64, 128, 256, 512):
        a[k - 1], a[k] = a[k], a[k - 1]
    a[N - 2], a[N - 1] = a[N - 1], a[N - 2]
    return a


def swap_first_two():
    return [1, 0] + list(range(2, N))


def displaced():
    """every 37th packet arrives 1..8 places late"""
    a = list(range(N))
    for j, k in enumerate(range(20, N - 10, 37)):
        x = a.pop(k)
        a.insert(k + 1 + j % 8, x)
    return a


DUP_AT = (450, 257, 63)


def dup_back(d):
    """duplicates whose original is d arrivals back (several places, one
    of them with the original in the block before)"""
    a = list(range(N))
    for k in DUP_AT:                    # highest first: no pair shifts another
        a.insert(k + d, a[k])
    return a


def dup_below_max(dist):
    """a copy of the packet `dist` below the maximum, right after it"""
    return list(range(200)) + [199 - dist] + list(range(200, N))


def repeated():
    return list(range(100)) + [99] * 300 + list(range(100, 300))


def late_by(k, d):
    a = list(range(N))
    x = a.pop(k)
    a.insert(k + d, x)
    return a


SHAPES = {
    "in_order": lambda: list(range(N)),
    "block_swaps": swaps_at_block_boundaries,
    "swap_first": swap_first_two,
    "displaced": displaced,
    "dup_1": lambda: dup_back(1),
    "dup_2": lambda: dup_back(2),
    "dup_3": lambda: dup_back(3),
    "dup_4": lambda: dup_back(4),
    "dup_5": lambda: dup_back(5),
    "dup_128": lambda: dup_back(128),
    "dup_129": lambda: dup_back(129),
    "dup_max63": lambda: dup_below_max(63),
    "dup_max64": lambda: dup_below_max(64),
    "dup_max65": lambda: dup_below_max(65),
    "repeated_300": repeated,
    # s0 = 65000 rolls over at position 536: a packet from before it after
    "pre_wrap_late": lambda: late_by(530, 12),
    "late_70": lambda: late_by(300, 70),
}


@pytest.mark.parametrize("s0", S0S)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shape_fresh_stream(be, sent, shape, s0):
    arr = [sent[s0][k] for k in SHAPES[shape]()]
    ok = sweep(verdicts(be, arr), arr)
    if shape == "pre_wrap_late" and s0 == 65000:
        assert not any(ok.values())             # ETIMEDOUT in the reference
    elif shape in ("in_order", "block_swaps", "swap_first", "dup_1",
                   "repeated_300"):
        # nothing here needs more than one arrival of look-back
        assert all(ok.values()), (shape, ok)
    elif shape in ("displaced", "dup_max63", "dup_max64", "dup_max65"):
        assert all(v for (b, lb), v in ok.items() if lb == 128), (shape, ok)
    if shape.startswith("dup_") and shape[4:].isdigit():
        d = int(shape[4:])
        # s0 = 65000 rolls over at position 536: a copy of a packet from
        # before it, arriving after it, is ETIMEDOUT in the reference
        wrapped = s0 == 65000 and any(k < 536 <= k + d for k in DUP_AT)
        for (b, lb), v in ok.items():
            if lb >= d and not wrapped:
                assert v, (shape, b, lb)
            if wrapped:
                assert not v


@pytest.mark.parametrize("s0", S0S)
@pytest.mark.parametrize("jump", (30000, 33000, 40000))
def test_forward_jump(be, jump, s0):
    seqs = [s0 + k + (jump if k >= 300 else 0) for k in range(N)]
    arr = protect(be, seqs)
    ok = sweep(verdicts(be, arr), arr)
    if jump == 30000:
        assert all(ok.values())
    else:
        # past half the sequence space the receiver's guess is a late
        # packet: ETIMEDOUT, or EAUTH at the index it guesses
        assert not any(ok.values())


@pytest.mark.parametrize("s0", S0S)
def test_continuing_state(be, sent, s0):
    """a first batch that leaves a non-zero bitmap, then replays of its
    packets among new ones"""
    first = sent[s0][:300]
    new = sent[s0][300:]
    # inside the window the first batch left
    arr = new[:50] + [first[299], first[290]] + new[50:200] + \
        [first[260], first[299]] + new[200:]
    truth = verdicts(be, arr, first=first)
    assert truth[0][3] != 0 and truth[0][2] != 0
    assert truth[1].count(errno.EALREADY) == 4
    assert all(sweep(truth, arr).values())
    # a gap in the first batch filled late, and replays from far below
    holes = [k for k in range(300) if k not in (280, 285)]
    first = [sent[s0][k] for k in holes]
    arr = new[:10] + [sent[s0][285]] + new[10:40] + [sent[s0][280]] + \
        new[40:100] + [sent[s0][285], sent[s0][5]] + new[100:]
    truth = verdicts(be, arr, first=first)
    assert truth[1][10] == 0 and truth[1][41] == 0
    # (short look-backs may leave it unsettled: never a wrong answer)
    ok = sweep(truth, arr)
    assert not ok[(64, 2)] or ok[(64, 128)]


def network_shaped(rng, n):
    """arrival order of n sent packets: 1 % loss, 2 % adjacent swaps, 1 %
    displaced by up to 8, 0.5 % duplicates of one of the last 32 arrivals"""
    a = [k for k in range(n) if rng.random() >= 0.01]
    i = 0
    while i + 1 < len(a):
        if rng.random() < 0.02:
            a[i], a[i + 1] = a[i + 1], a[i]
            i += 1
        i += 1
    for k in np.flatnonzero(rng.random(len(a)) < 0.01)[::-1]:
        x = a.pop(int(k))
        a.insert(min(len(a), int(k) + int(rng.integers(1, 9))), x)
    out = []
    for x in a:
        out.append(x)
        if rng.random() < 0.005:
            out.append(out[-int(rng.integers(1, min(32, len(out)) + 1))])
    return out


@pytest.mark.parametrize("seed", range(6))
def test_network_shaped_settles(be, sent, seed):
    """the cap: real-network reshaping always settles at lookback 128"""
    rng = np.random.default_rng(9000 + seed)
    order = network_shaped(rng, N)
    assert len(order) != N or order != list(range(N))
    arr = [sent[100][k] for k in order]
    truth = verdicts(be, arr)
    ok = sweep(truth, arr)
    assert all(v for (b, lb), v in ok.items() if lb == 128), ok
    # continuing: the second half behind the first
    h = len(arr) // 2
    truth = verdicts(be, arr[h:], first=arr[:h])
    assert all(v for (b, lb), v in sweep(truth, arr[h:]).items()
               if lb == 128)
    # s0 = 65000: unsettled only when a packet from before the rollover
    # arrives after one from behind it
    arr = [sent[65000][k] for k in order]
    wrap = 65536 - 65000
    seen_post, late_pre = False, False
    for k in order:
        if k >= wrap:
            seen_post = True
        elif seen_post:
            late_pre = True
    ok = sweep(verdicts(be, arr), arr)
    for (b, lb), v in ok.items():
        if lb == 128:
            assert v or late_pre, (b, lb)


def test_bad_arguments():
    st = stream_state()
    seq = np.zeros(4, dtype=np.uint16)
    ix = np.zeros(4, dtype=np.uint64)
    err = np.zeros(4, dtype=np.int32)
    st1, fail = P.StreamState(), ctypes.c_uint32()
    f = P.lib().srtp_rx_plan_host
    args = lambda n, b: (ctypes.byref(st), seq.ctypes.data, n, b, 128,
                         ix.ctypes.data, err.ctypes.data, ctypes.byref(st1),
                         ctypes.byref(fail))
    assert f(*args(4, 0)) == errno.EINVAL
    assert f(*args(0, 4)) == errno.EINVAL
    assert f(*args(4, 4)) == 0 and fail.value == 0
    assert err.tolist() == [0, errno.EALREADY, errno.EALREADY,
                            errno.EALREADY]
