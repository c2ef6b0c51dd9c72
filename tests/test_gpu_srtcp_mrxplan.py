"""The many-session SRTCP receive planner (plan_buckets_rtcp_rx.hip,
batch_dev.c dev_mrrxplanned): srtcp_decrypt_batch_dev with a device session
array over sessions whose streams arrive reordered, duplicated or replayed,
HMAC suites.

Every batch goes through PlanDrive (tests/test_gpu_srtcp_mplan.py): per packet
errno, pos, end and bytes and per (session, SSRC) the exported
(replay_rtcp_lix, replay_rtcp_bitmap, rtcp_index), against the oracle called
one packet at a time and against the same call on contexts of their own under
nomrplan=1 (the host engine).  Counter deltas are asserted per call:
"mrrxplans" (accepted receive plans), "mrplans", "rejects", "folds", "rxdups"
(the oracle's EALREADY count), "rxlate".

The planner runs behind a plan of dev_mplanned_rtcp rejected for a replayed or
decreasing index only, so an accepted batch shows mrrxplans +1, mrplans +0,
rejects +1, folds +0.  40 sessions, at most 600 packets per batch, bpexp 250:
16 sessions per bucket, 3 buckets.

Not here: a copy beyond the look-back (RX_LOOKBACK 128 arrivals of one stream;
no knob makes it smaller, tests/c/rtcp_seg_rx_check.c reaches that branch with
small look-backs).  A 9th SSRC and a session past SGPU_BP_SEGMAX are rejected
by the in-order plan with more than SPF_REPLAY, so the receive planner is not
asked: the counters asserted are the same.  The SEGMAX case needs the 1100
packets tests/test_gpu_srtcp_mplan.py test_rejected_segmax sends.
"""
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import mrtcp_rx_traffic as T
from tests.test_gpu_srtcp import rtcp_packet
from tests.test_gpu_srtcp_mplan import ACCEPT, BPEXP, NSESS, PlanDrive
from tests.test_gpu_srtcp_multi import U, flipped, ssrc_of, wire_of
from tests.test_gpu_srtcp_replay import CASES, has_hmac

pytestmark = pytest.mark.gpu

EALREADY, ENOSR = errno.EALREADY, errno.ENOSR
XCNT = ("mrrxplans", "rxdups", "rxlate")
HMAC_CASES = [(s, f) for s, f in CASES if has_hmac(s)]
GCM = [s for s, _ in CASES if not has_hmac(s)][0]
ids = ["s%d%s" % (s, "u" if f else "") for s, f in HMAC_CASES]
assert T.ssrc_of(3, 2) == ssrc_of(3, 2) and T.NSESS == NSESS


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


class RxDrive(PlanDrive):
    """PlanDrive that also records the receive planner's counters (the
    comparison run under nomrplan=1 does not move them)"""

    def step(self, side, op, pkts, rooms=None, what=None, expect=None):
        x0 = {c: P.counter(c) for c in XCNT}
        rows = super().step(side, op, pkts, rooms, what, expect)
        self.x = {c: P.counter(c) - x0[c] for c in XCNT}
        return rows


def drive(torch, scn, suite, flags, *args, nsess=NSESS, bpexp=BPEXP,
          limit=600, **kw):
    d = RxDrive(torch, suite, flags, nsess, limit=limit)
    try:
        with P.tune(bpexp=bpexp):
            return scn(d, *args, **kw)
    finally:
        d.close()


def send(d, rng, who, what, size=None):
    """the senders' batch [(session, stream)], every stream in order: the
    wire packets in that order"""
    pk = [(s, rtcp_packet(rng, ssrc_of(s, k),
                          int(4 * rng.integers(0, 30)) if size is None
                          else size)) for s, k in who]
    rows = d.step("tx", "srtcp_encrypt", pk, what=(what, "send"),
                  expect=ACCEPT)
    assert not any(r[0] for r in rows)
    return wire_of(pk, rows)


def index_of(d, w):
    """the SRTCP index a wire packet carries"""
    t = P.tag_len(d.suite)
    return int.from_bytes(w[len(w) - t - 4:len(w) - t], "big") & 0x7fffffff


def recv(d, wire, what, kind="taken"):
    rows = d.step("rx", "srtcp_decrypt", wire, what=(what, "recv"))
    dc, x = d.deltas[-1][3], d.x
    ndup = sum(1 for r in rows if r[0] == EALREADY)
    got = (x["mrrxplans"], dc["mrplans"], dc["rejects"], dc["folds"])
    if kind == "taken":
        assert {r[0] for r in rows} <= {0, EALREADY}, what
        assert got == (1, 0, 1, 0), (what, got, x)
        assert x["rxdups"] == ndup, (what, x, ndup)
    elif kind == "forged":
        assert got[0] == 1 and got[3] == 1, (what, got)
    elif kind == "off":
        assert got[0] == 0, (what, got)
    elif kind == "left":
        assert got[0] == 0 and got[2] == 1, (what, got)
    elif kind in ("gcm", "clean"):
        assert got[:3] == (0, 1, 0), (what, got)
    return rows


def at(who, s, k):
    """the places of stream (s, k)'s packets in a batch"""
    return [i for i, w in enumerate(who) if w == (s, k)]


def shuffled(rng, who):
    return [who[i] for i in rng.permutation(len(who)).tolist()]


def everyone(rng, per=3, nk=2):
    return shuffled(rng, [(s, k) for s in range(NSESS) for k in range(nk)] * per)


def swap(a, i, j):
    a[i], a[j] = a[j], a[i]


def last_first(w, a):
    """the last of a stream's packets (places a) moved in front of its
    first: the stream's places afterwards, in arrival order"""
    w.insert(a[0], w.pop(a[-1]))
    return [a[0]] + [i + 1 for i in a[:-1]]


# ---- accepted: the named disturbances ------------------------------------------

def scn_cases(d, seed):
    rng = np.random.default_rng(seed)
    # adjacent and distant swaps inside a stream
    who = everyone(rng)
    w = send(d, rng, who, "swaps")
    a, b = at(who, 2, 0), at(who, 20, 1)
    swap(w, a[0], a[1])
    swap(w, b[0], b[2])
    rows = recv(d, w, "swaps")
    assert not any(r[0] for r in rows) and d.x["rxlate"] == 3, d.x
    # a duplicate directly behind and far behind its original
    who = everyone(rng)
    w = send(d, rng, who, "dups")
    prev = list(w)
    a, b = at(who, 3, 0), at(who, 35, 1)
    w.append(w[b[0]])
    w.insert(a[0] + 1, w[a[0]])
    rows = recv(d, w, "dups")
    assert [i for i, r in enumerate(rows) if r[0]] == [a[0] + 1, len(w) - 1]
    # the batch before again, whole
    rows = recv(d, prev, "replay whole")
    assert all(r[0] == EALREADY for r in rows)
    # ... and in part, among new packets
    who = everyone(rng)
    w = send(d, rng, who, "replay part")
    for i in rng.choice(len(prev), 30, replace=False).tolist():
        w.insert(int(rng.integers(0, len(w) + 1)), prev[i])
    rows = recv(d, w, "replay part")
    assert sum(1 for r in rows if r[0]) == 30
    # a packet exactly 63 and 64 below the top: 66 packets of one stream (a
    # segment across waves), the last one first
    who = shuffled(rng, [(1, 0)] * 65 + [(s, 0) for s in range(NSESS)])
    w = send(d, rng, who, "63 / 64")
    a = last_first(w, at(who, 1, 0))
    assert len(a) == 66
    top = index_of(d, w[a[0]][1])
    rows = recv(d, w, "63 / 64")
    below = {top - index_of(d, w[i][1]): rows[i][0] for i in a[:4]}
    assert below == {0: 0, 65: EALREADY, 64: EALREADY, 63: 0}, below
    # a first packet at both edges of the stored window, and on a set bit
    for k, first, bm in ((0x20, 1000 - 64, 1), (0x21, 1000 - 63, 1),
                         (0x22, 1000 - 63, 1 | 1 << 63)):
        d.set_rtcp("tx", 38, ssrc_of(38, k), first - 1, 0, 0)
        d.set_rtcp("rx", 38, ssrc_of(38, k), 0, 1000, bm)
    who = shuffled(rng, [(38, k) for k in (0x20, 0x21, 0x22)] * 2 +
                   [(s, 0) for s in range(NSESS)] * 2)
    w = send(d, rng, who, "edges")
    rows = recv(d, w, "edges")
    got = {k: [rows[i][0] for i in at(who, 38, k)] for k in (0x20, 0x21, 0x22)}
    assert got == {0x20: [EALREADY, 0], 0x21: [0, 0], 0x22: [EALREADY, 0]}, got
    # the 31-bit wrap, a swap in front of it
    x = ssrc_of(5, 0x30)
    d.set_rtcp("tx", 5, x, 0x7ffffff0, 0, 0)
    d.set_rtcp("rx", 5, x, 0, 0x7ffffff0, 1)
    who = shuffled(rng, [(5, 0x30)] * 20 + [(s, 1) for s in range(NSESS)] * 2)
    w = send(d, rng, who, "wrap")
    a = at(who, 5, 0x30)
    swap(w, a[3], a[4])
    rows = recv(d, w, "wrap")
    assert [rows[i][0] for i in a] == [0] * 15 + [EALREADY] * 5
    # two SSRCs of a session disturbed independently, a new SSRC mid-batch
    # (its packets in reverse)
    who = shuffled(rng, [(7, 0), (7, 1)] * 6 + [(s, 0) for s in range(NSESS)])
    mid = len(who) // 2
    who[mid:mid] = [(7, 0x40)] * 3
    w = send(d, rng, who, "two streams")
    a, b, c = at(who, 7, 0), at(who, 7, 1), at(who, 7, 0x40)
    swap(w, a[1], a[4])
    swap(w, c[0], c[2])
    w.insert(b[3] + 1, w[b[2]])
    rows = recv(d, w, "two streams")
    assert [i for i, r in enumerate(rows) if r[0]] == [b[3] + 1]
    # sessions in three buckets, one session of the middle one disturbed
    who = everyone(rng, 2, 1)
    w = send(d, rng, who, "one bucket")
    a = at(who, 20, 0)
    swap(w, a[0], a[1])
    rows = recv(d, w, "one bucket")
    assert not any(r[0] for r in rows) and d.x["rxlate"] == 1
    d.require("rx", {0, EALREADY})
    return d.finish()


@pytest.mark.parametrize("suite,flags", HMAC_CASES, ids=ids)
def test_accepted_cases(torch_cuda, suite, flags):
    drive(torch_cuda, scn_cases, suite, flags, 500 + suite)


def scn_random(d, seed):
    rng = np.random.default_rng(seed)
    start, batches = T.random_batches(seed)
    for (s, k), ix in sorted(start.items()):
        if ix != 1:
            d.set_rtcp("tx", s, ssrc_of(s, k), ix - 1, 0, 0)
    wires = []
    for b, (sent, arrive, ndist) in enumerate(batches):
        w = send(d, rng, [(s, k) for s, k, _ in sent], ("random", b))
        assert [index_of(d, p) for _, p in w] == [ix for _, _, ix in sent]
        wires.append(w)
        assert ndist > 0
        rows = recv(d, [wires[bb][i] for bb, i in arrive], ("random", b))
        assert d.x["mrrxplans"] == 1
    d.require("rx", {0, EALREADY})
    return d.finish()


@pytest.mark.parametrize("suite,flags", HMAC_CASES, ids=ids)
def test_random_traffic_is_accepted(torch_cuda, suite, flags):
    drive(torch_cuda, scn_random, suite, flags, 801)


# ---- forged, switched off, rejected, GCM -----------------------------------------

def disturbed(d, rng, what):
    """a batch with a swap and a duplicate, and the places of stream (1, 0),
    whose 70 packets arrive with the last one first"""
    who = shuffled(rng, [(1, 0)] * 70 + [(s, k) for s in range(d.nsess)
                                         for k in range(2)] * 2)
    w = send(d, rng, who, what)
    w.append(w[at(who, 6, 1)[0]])
    return w, last_first(w, at(who, 1, 0))


def scn_forged(d, seed):
    """a flipped tag bit on the packet above everything, then on one 64 or
    more below the top (EAUTH, not EALREADY): the plan is accepted, the
    crypto launch counts the miss, everything is undone and the host engine
    folds"""
    rng = np.random.default_rng(seed)
    for b, q in enumerate((0, 1)):
        w, a = disturbed(d, rng, ("forged", b))
        s, p = w[a[q]]
        w[a[q]] = (s, flipped(p, len(p) - 1, 0x40))
        rows = recv(d, w, ("forged", b), "forged")
        assert rows[a[q]][0] == P.EAUTH
        assert {r[0] for r in rows} <= {0, EALREADY, P.EAUTH}
        assert sum(1 for r in rows if r[0] == P.EAUTH) == 1
    return d.finish()


@pytest.mark.parametrize("suite,flags", [(1, 0), (1, U)], ids=["s1", "s1u"])
def test_forged_among_disturbed(torch_cuda, suite, flags):
    drive(torch_cuda, scn_forged, suite, flags, 520 + flags)


def scn_off(d, seed):
    rng = np.random.default_rng(seed)
    w, _ = disturbed(d, rng, "off")
    with P.tune(nomrrxplan=1):
        rows = recv(d, w, "off", "off")
    assert EALREADY in {r[0] for r in rows}
    w, _ = disturbed(d, rng, "on again")
    recv(d, w, "on again")
    return d.finish()


def test_nomrrxplan(torch_cuda):
    drive(torch_cuda, scn_off, 1, 0, 530)


def scn_ninth(d, seed):
    """a receiver session with 8 streams meets a 9th SSRC (ENOSR) beside a
    swap"""
    rng = np.random.default_rng(seed)
    for q in range(6):
        d.set_rtcp("rx", 3, ssrc_of(3, 0x50 + q), 0, 0, 0)
    who = shuffled(rng, [(s, k) for s in range(d.nsess) for k in range(2)])
    recv(d, send(d, rng, who, "eight"), "eight", "clean")
    who = shuffled(rng, [(s, k) for s in range(d.nsess) for k in range(2)] * 2)
    who.insert(len(who) // 2, (3, 2))
    w = send(d, rng, who, "ninth")
    a = at(who, 9, 0)
    swap(w, a[0], a[1])
    rows = recv(d, w, "ninth", "left")
    assert [r[0] for r in rows].count(ENOSR) == 1
    return d.finish()


def test_rejected_ninth_ssrc(torch_cuda):
    drive(torch_cuda, scn_ninth, 1, 0, 540)


def test_rejected_segmax(torch_cuda):
    """a session past SGPU_BP_SEGMAX (1024) in its bucket, one swap: 1100
    packets of 8 bytes, 1040 of them session 0's (module docstring)"""
    def scn(d):
        rng = np.random.default_rng(541)
        who = shuffled(rng, [(0, 0)] * 1040 + [(s, 0) for s in range(1, 6)] * 12)
        pk = [(s, rtcp_packet(rng, ssrc_of(s, k), 0)) for s, k in who]
        rows = d.step("tx", "srtcp_encrypt", pk, what="segmax")
        w = wire_of(pk, rows)
        a = at(who, 2, 0)
        swap(w, a[0], a[1])
        rows = recv(d, w, "segmax", "left")
        assert not any(r[0] for r in rows)
    drive(torch_cuda, scn, 1, 0, nsess=6, bpexp=400, limit=1100)


def scn_gcm(d, seed):
    """GCM keeps no SRTCP replay window: the in-order planner takes any
    order, as before"""
    rng = np.random.default_rng(seed)
    w, _ = disturbed(d, rng, "gcm")
    recv(d, w, "gcm", "gcm")
    return d.finish()


def test_gcm_keeps_the_old_planner(torch_cuda):
    drive(torch_cuda, scn_gcm, GCM, 0, 550)
