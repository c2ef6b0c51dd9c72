"""The one-session SRTCP planner (plan_streams_rtcp.hip, batch_dev.c
dev_splanned_rtcp): srtcp_*_batch_dev without a session array ("dev1") on one
session whose SRTCP carries several SSRCs, or whose packets arrive reordered,
duplicated or replayed.

Every batch goes through PairDrive (tests/test_gpu_srtcp_multi.py): per packet
errno, pos, end and bytes and per SSRC the exported SRTCP state (rtcp_index,
replay_rtcp_lix, replay_rtcp_bitmap) and RTP state, against the oracle called
one packet at a time.  Counter deltas are asserted per call: "srplans" (batches
the planner completed), "srundos" (accepted plans undone for a forged packet),
"rplans", "rejects", "folds", "rxdups" (the oracle's EALREADY count), "rxlate"
(accepted packets below their window's top, counted here from the indices on
the wire).

A session with at most one stream first gets the one-stream planner, whose
rejection (rejects +1) for a second SSRC or a replayed index brings this one
in; a session with several streams gets it directly (rejects +0).  Batches are
at most 600 packets: three workgroups of 256.

Not here: a copy beyond the look-back (RX_LOOKBACK 128 arrivals of one stream;
no knob makes it smaller, tests/c/rtcp_str_check.c reaches that branch with
small look-backs).
"""
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import srtcp_str_traffic as T
from tests.test_gpu_srtcp import rtcp_packet
from tests.test_gpu_srtcp_multi import (A, B, COUNTERS, FULL, SUB, U, PairDrive,
                                        flipped, scn_srtcp_first, scn_wrap,
                                        sub_ids, trailer, wire_of)
from tests.test_gpu_srtcp_replay import has_hmac

pytestmark = pytest.mark.gpu

EALREADY, ENOSR, EBADMSG, ENOMEM = (errno.EALREADY, errno.ENOSR,
                                    errno.EBADMSG, errno.ENOMEM)
XCNT = COUNTERS + ("srplans", "srundos", "rxdups", "rxlate")
HMAC_CASES = [(s, f) for s, f in SUB if has_hmac(s)]
hmac_ids = ["s%d%s" % (s, "u" if f else "") for s, f in HMAC_CASES]
GCM = [s for s, _ in SUB if not has_hmac(s)][0]
RTCP = ("srtcp_encrypt", "srtcp_decrypt")
assert T.ssrc_of(3) == 0x51000003


def X(k):
    return T.ssrc_of(k)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


class Drive(PairDrive):
    """PairDrive on one session through the device arrays without a session
    array, recording every call's counter deltas"""

    def __init__(self, torch, suite, flags):
        super().__init__(torch, suite, flags, 1, "dev1")
        self.hist = []

    def step(self, side, op, pkts, rooms=None, what=None, expect=None):
        x0 = {c: P.counter(c) for c in XCNT}
        # the streams the side's context holds before the call
        self.ns = len(self.seen[side])
        rows = super().step(side, op, pkts, rooms, what, expect)
        self.x = {c: P.counter(c) - x0[c] for c in XCNT}
        self.hist.append((side, op, what, self.ns, dict(self.x)))
        return rows

    def lix(self, side, ssrc):
        st = self.twin[side].state(0, ssrc)
        return 0 if st is None else st[0][1]


def drive(torch, scn, suite, flags, *args, **kw):
    d = Drive(torch, suite, flags)
    try:
        return scn(d, *args, **kw)
    finally:
        d.close()


def taken(d, what, rejects=None):
    """the call before was completed by the planner"""
    x = d.x
    want = (d.ns <= 1) if rejects is None else rejects
    got = (x["srplans"], x["srundos"], x["rplans"], x["rejects"], x["folds"])
    assert got == (1, 0, 0, int(want), 0), (what, d.ns, x)


def left(d, what):
    """... was not"""
    assert d.x["srplans"] == 0 and d.x["srundos"] == 0, (what, d.x)


def send(d, rng, who, what, size=None, plan=True):
    """the sender's batch [stream], every stream in order: the wire packets in
    that order"""
    pk = [(0, rtcp_packet(rng, X(k), int(4 * rng.integers(0, 30))
                          if size is None else size)) for k in who]
    rows = d.step("tx", "srtcp_encrypt", pk, what=(what, "send"))
    assert not any(r[0] for r in rows)
    if plan:
        taken(d, (what, "send"))
    return wire_of(pk, rows)


def index_of(d, w):
    """the SRTCP index a wire packet carries"""
    t = P.tag_len(d.suite)
    return int.from_bytes(w[len(w) - t - 4:len(w) - t], "big") & 0x7fffffff


def ssrc_at(w):
    return int.from_bytes(w[4:8], "big")


def recv(d, wire, what, kind="taken"):
    top = {}
    for _, p in wire:
        x = ssrc_at(p)
        if x not in top:
            top[x] = d.lix("rx", x)
    rows = d.step("rx", "srtcp_decrypt", wire, what=(what, "recv"))
    x = d.x
    if kind == "taken":
        assert {r[0] for r in rows} <= {0, EALREADY}, what
        taken(d, (what, "recv"))
        if has_hmac(d.suite):
            late = 0
            for (_, p), r in zip(wire, rows):
                s, ix = ssrc_at(p), index_of(d, p)
                late += r[0] == 0 and ix < top[s]
                top[s] = max(top[s], ix)
            ndup = sum(1 for r in rows if r[0] == EALREADY)
            assert (x["rxdups"], x["rxlate"]) == (ndup, late), (what, x, ndup,
                                                                late)
        else:
            assert not any(r[0] for r in rows)
    elif kind == "forged":
        got = (x["srplans"], x["srundos"], x["rplans"])
        assert got == (0, 1, 0), (what, x)
    elif kind == "left":
        left(d, (what, "recv"))
    return rows


def at(who, k):
    """the places of stream k's packets in a batch"""
    return [i for i, w in enumerate(who) if w == k]


def shuffled(rng, who):
    return [who[i] for i in rng.permutation(len(who)).tolist()]


def swap(a, i, j):
    a[i], a[j] = a[j], a[i]


def last_first(w, a):
    """the last of a stream's packets (places a) moved in front of its first:
    the stream's places afterwards, in arrival order"""
    w.insert(a[0], w.pop(a[-1]))
    return [a[0]] + [i + 1 for i in a[:-1]]


# ---- 1. round trip over 2..8 interleaved SSRCs ----------------------------------

def scn_round_trip(d, seed, nss, n=560):
    rng = np.random.default_rng(seed)
    for b in range(2):
        who = shuffled(rng, list(range(nss)) +
                       rng.integers(0, nss, n - nss).tolist())
        w = send(d, rng, who, ("round trip", b), plan=False)
        taken(d, ("round trip", b, "send"), rejects=b == 0)
        rows = recv(d, w, ("round trip", b))
        assert d.x["rejects"] == (b == 0) and not any(r[0] for r in rows)
    d.require("tx", {0})
    d.require("rx", {0})
    return d.finish()


@pytest.mark.parametrize("case", list(enumerate(SUB)), ids=sub_ids)
def test_round_trip(torch_cuda, case):
    i, (suite, flags) = case
    drive(torch_cuda, scn_round_trip, suite, flags, 300 + i, 2 + (3 * i) % 7)


@pytest.mark.parametrize("nss", [2, 8])
def test_round_trip_two_and_eight(torch_cuda, nss):
    suite, flags = HMAC_CASES[0]
    drive(torch_cuda, scn_round_trip, suite, flags, 320 + nss, nss)


# ---- 2. the table grows 1 -> 3 -> 8, then a 9th SSRC ------------------------------

def scn_growing(d, seed):
    rng = np.random.default_rng(seed)
    # one stream in order: the one-stream planner's
    w = send(d, rng, [0] * 40, "one", plan=False)
    assert (d.x["rplans"], d.x["srplans"]) == (1, 0), d.x
    recv(d, w, "one", "left")
    assert d.x["rplans"] == 1
    # 1 -> 3 and 3 -> 8: the new SSRCs first appear mid-batch
    for have, upto in ((1, 3), (3, 8)):
        who = shuffled(rng, list(range(have)) * 60)
        for k in range(have, upto):
            for _ in range(20):
                who.insert(int(rng.integers(len(who) // 2, len(who) + 1)), k)
        w = send(d, rng, who, ("grow", upto))
        assert d.ns == have
        b = at(who, 0)
        swap(w, b[2], b[3])
        rows = recv(d, w, ("grow", upto))
        assert d.ns == have and not any(r[0] for r in rows)
    # a 9th: ENOSR for that packet, from the host engine
    who = shuffled(rng, list(range(8)) * 20)
    who.insert(len(who) // 2, 8)
    pk = [(0, rtcp_packet(rng, X(k), 24)) for k in who]
    rows = d.step("tx", "srtcp_encrypt", pk, what="ninth")
    left(d, "ninth")
    assert [i for i, r in enumerate(rows) if r[0]] == [len(who) // 2]
    assert rows[len(who) // 2][0] == ENOSR
    rows = d.step("rx", "srtcp_decrypt", wire_of(pk, rows), what="ninth")
    left(d, "ninth")
    assert [r[0] for r in rows].count(ENOSR) == 1
    return d.finish()


@pytest.mark.parametrize("case", [HMAC_CASES[0], (GCM, 0)], ids=["hmac", "gcm"])
def test_growing_table(torch_cuda, case):
    drive(torch_cuda, scn_growing, case[0], case[1], 330)


# ---- 3. a batch on an SSRC the session does not know -------------------------------

def scn_unknown(d, seed):
    rng = np.random.default_rng(seed)
    d.set_rtcp("tx", 0, A, 500, 0, 0)
    d.set_rtcp("rx", 0, A, 0, 500, FULL)
    pk = [(0, rtcp_packet(rng, B, 4 * int(rng.integers(0, 65))))
          for _ in range(30)]
    rows = d.step("tx", "srtcp_encrypt", pk, what="unknown")
    taken(d, "unknown", rejects=True)
    assert d.twin["tx"].state(0, A)[0][0] == 500
    assert d.twin["tx"].state(0, B)[0][0] == 30
    d.step("rx", "srtcp_decrypt", wire_of(pk, rows), what="unknown")
    taken(d, "unknown", rejects=True)
    assert d.twin["rx"].state(0, A)[0][1:] == (500, FULL)
    if has_hmac(d.suite):
        assert d.twin["rx"].state(0, B)[0][1:] == (30, (1 << 30) - 1)
    return d.finish()


@pytest.mark.parametrize("sep", [0, 1])
@pytest.mark.parametrize("case", SUB, ids=sub_ids)
def test_batch_on_unknown_ssrc(torch_cuda, case, sep):
    with P.tune(noplanfuse=sep):
        drive(torch_cuda, scn_unknown, case[0], case[1], 340)


# ---- 4. the 31-bit wrap of one of three streams -------------------------------------

@pytest.mark.parametrize("case", SUB, ids=sub_ids)
def test_index_wrap_per_stream(torch_cuda, case):
    d = Drive(torch_cuda, case[0], case[1])
    try:
        scn_wrap(d, 350)
        calls = [h for h in d.hist if h[1] in RTCP and h[2] == "wrap"]
        assert len(calls) == 2
        for side, op, what, ns, x in calls:
            assert (x["srplans"], x["rplans"], x["rejects"]) == (1, 0, 1), \
                (side, x)
        if has_hmac(d.suite):
            # B's five packets behind the wrap are old to the reference
            assert calls[1][4]["rxdups"] == 5
    finally:
        d.close()


# ---- 5. HMAC suites, disturbed unprotect ---------------------------------------------

def everyone(rng, nk=3, per=40):
    return shuffled(rng, list(range(nk)) * per)


def scn_cases(d, seed):
    rng = np.random.default_rng(seed)
    # adjacent and distant swaps inside a stream
    who = everyone(rng)
    w = send(d, rng, who, "swaps")
    a, b = at(who, 0), at(who, 2)
    swap(w, a[0], a[1])
    swap(w, b[3], b[9])
    rows = recv(d, w, "swaps")
    assert not any(r[0] for r in rows) and d.x["rxlate"] == 1 + 6, d.x
    # a duplicate directly behind and far behind its original
    who = everyone(rng)
    w = send(d, rng, who, "dups")
    prev = list(w)
    a, b = at(who, 0), at(who, 1)
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
    # a packet exactly 63, 64 and 65 below the top: 66 packets of one stream
    # (a run across waves), the last one first
    who = shuffled(rng, [1] * 66 + [0, 2] * 10)
    w = send(d, rng, who, "63 / 64")
    a = last_first(w, at(who, 1))
    assert len(a) == 66
    top = index_of(d, w[a[0]][1])
    rows = recv(d, w, "63 / 64")
    below = {top - index_of(d, w[i][1]): rows[i][0] for i in a[:4]}
    assert below == {0: 0, 65: EALREADY, 64: EALREADY, 63: 0}, below
    # a first packet at both edges of a stored window, and on a set bit
    for k, first, bm in ((0x20, 1000 - 64, 1), (0x21, 1000 - 63, 1),
                         (0x22, 1000 - 63, 1 | 1 << 63)):
        d.set_rtcp("tx", 0, X(k), first - 1, 0, 0)
        d.set_rtcp("rx", 0, X(k), 0, 1000, bm)
    who = shuffled(rng, [0x20, 0x21, 0x22] * 2 + [0, 1, 2] * 10)
    w = send(d, rng, who, "edges")
    rows = recv(d, w, "edges")
    got = {k: [rows[i][0] for i in at(who, k)] for k in (0x20, 0x21, 0x22)}
    assert got == {0x20: [EALREADY, 0], 0x21: [0, 0], 0x22: [EALREADY, 0]}, got
    d.require("rx", {0, EALREADY})
    return d.finish()


@pytest.mark.parametrize("suite,flags", HMAC_CASES, ids=hmac_ids)
def test_disturbed_cases(torch_cuda, suite, flags):
    drive(torch_cuda, scn_cases, suite, flags, 500 + suite)


def scn_two_streams(d, seed):
    """two streams disturbed independently, a new SSRC mid-batch whose packets
    arrive reversed; then a stream of more than RX_LOOKBACK + 64 arrivals over
    three workgroups with a duplicate inside the look-back"""
    rng = np.random.default_rng(seed)
    w = send(d, rng, shuffled(rng, [0, 1] * 20), "open")
    recv(d, w, "open")
    who = shuffled(rng, [0, 1] * 30)
    mid = len(who) // 2
    who[mid:mid] = [0x40] * 3
    w = send(d, rng, who, "two streams")
    a, b, c = at(who, 0), at(who, 1), at(who, 0x40)
    swap(w, a[1], a[4])
    swap(w, c[0], c[2])
    w.insert(b[3] + 1, w[b[2]])
    rows = recv(d, w, "two streams")
    assert [i for i, r in enumerate(rows) if r[0]] == [b[3] + 1]
    # 260 arrivals of stream 0 among 590: its run crosses two workgroup
    # borders, the duplicate's original lies 100 arrivals of the stream back
    who = shuffled(rng, [0] * 260 + [1] * 200 + [0x40] * 129)
    w = send(d, rng, who, "long")
    a = at(who, 0)
    assert a[-1] - a[0] > 512
    w.insert(a[200] + 1, w[a[100]])
    swap(w, a[30], a[38])
    assert len(w) == 590
    rows = recv(d, w, "long")
    assert [i for i, r in enumerate(rows) if r[0]] == [a[200] + 1]
    d.require("rx", {0, EALREADY})
    return d.finish()


@pytest.mark.parametrize("suite,flags", HMAC_CASES, ids=hmac_ids)
def test_two_streams_and_a_long_one(torch_cuda, suite, flags):
    drive(torch_cuda, scn_two_streams, suite, flags, 520 + suite)


# ---- 6. one stream, disturbed ----------------------------------------------------------

def scn_one_stream(d, seed):
    """one stream of 580 packets, in order for the sender (the one-stream
    planner's), with swaps, a duplicate and a lost packet for the receiver"""
    rng = np.random.default_rng(seed)
    for b in range(2):
        w = send(d, rng, [0] * 580, ("one stream", b), size=16, plan=False)
        assert (d.x["rplans"], d.x["srplans"]) == (1, 0), d.x
        swap(w, 10, 11)
        swap(w, 250, 258)
        w.insert(400, w[380])
        del w[520]
        rows = recv(d, w, ("one stream", b))
        assert d.ns == b and d.x["rejects"] == 1
        assert [i for i, r in enumerate(rows) if r[0]] == [400]
    return d.finish()


@pytest.mark.parametrize("suite,flags", HMAC_CASES[:2], ids=hmac_ids[:2])
def test_one_stream_disturbed(torch_cuda, suite, flags):
    drive(torch_cuda, scn_one_stream, suite, flags, 540)


# ---- 7. GCM ----------------------------------------------------------------------------

def scn_gcm(d, seed):
    """GCM keeps no SRTCP replay window: shuffled and duplicated packets of
    several SSRCs are all accepted"""
    rng = np.random.default_rng(seed)
    who = everyone(rng, 4, 60)
    w = send(d, rng, who, "gcm")
    w = shuffled(rng, w + w[:40])
    rows = recv(d, w, "gcm")
    assert not any(r[0] for r in rows) and d.x["rxdups"] == 0
    return d.finish()


def test_gcm_any_order(torch_cuda):
    drive(torch_cuda, scn_gcm, GCM, 0, 550)


# ---- 8. a forged tag among disturbed packets --------------------------------------------

def disturbed(d, rng, what):
    """a batch of three streams with a swap and a duplicate, and the places of
    stream 1, whose 70 packets arrive with the last one first"""
    who = shuffled(rng, [1] * 70 + [0, 2] * 40)
    w = send(d, rng, who, what)
    w.append(w[at(who, 2)[0]])
    a = at(who, 0)
    swap(w, a[5], a[7])
    return w, last_first(w, at(who, 1))


def scn_forged(d, seed, off):
    """a flipped tag bit on the packet above everything, then on one 64 or
    more below the top (EAUTH, not EALREADY); off: the same calls under
    nosrplan=1.  Returns each call's (folds, rejects)."""
    rng = np.random.default_rng(seed)
    out = []
    for b, q in enumerate((0, 1)):
        w, a = disturbed(d, rng, ("forged", b))
        s, p = w[a[q]]
        w[a[q]] = (s, flipped(p, len(p) - 1, 0x40))
        with P.tune(nosrplan=1 if off else None):
            rows = recv(d, w, ("forged", b), "left" if off else "forged")
        assert rows[a[q]][0] == P.EAUTH
        assert {r[0] for r in rows} <= {0, EALREADY, P.EAUTH}
        assert sum(1 for r in rows if r[0] == P.EAUTH) == 1
        out.append((d.x["folds"], d.x["rejects"]))
    d.finish()
    return out


@pytest.mark.parametrize("suite,flags", [HMAC_CASES[0], (HMAC_CASES[0][0], U)],
                         ids=["e", "u"])
def test_forged_among_disturbed(torch_cuda, suite, flags):
    on = drive(torch_cuda, scn_forged, suite, flags, 560 + flags, False)
    off = drive(torch_cuda, scn_forged, suite, flags, 560 + flags, True)
    assert on == off, (on, off)


# ---- 9. declined for a check ------------------------------------------------------------

def scn_declined(d, seed):
    rng = np.random.default_rng(seed)
    w = send(d, rng, everyone(rng, 2, 20), "open")
    recv(d, w, "open")
    # a cap one byte short of the trailer: ENOMEM for that packet
    pk = [(0, rtcp_packet(rng, X(k), 24)) for k in everyone(rng, 2, 20)]
    rooms = [60] * len(pk)
    rooms[7] = trailer(d.suite) - 1
    rows = d.step("tx", "srtcp_encrypt", pk, rooms, what="cap")
    left(d, "cap")
    assert [i for i, r in enumerate(rows) if r[0]] == [7]
    assert rows[7][0] == ENOMEM
    w = [x for i, x in enumerate(wire_of(pk, rows)) if i != 7]
    # a 6-byte packet: EBADMSG beside good packets
    w.insert(11, (0, w[3][1][:6]))
    rows = d.step("rx", "srtcp_decrypt", w, what="short")
    left(d, "short")
    assert [i for i, r in enumerate(rows) if r[0]] == [11]
    assert rows[11][0] == EBADMSG
    return d.finish()


@pytest.mark.parametrize("case", [HMAC_CASES[0], (GCM, 0)], ids=["hmac", "gcm"])
def test_declined_for_a_check(torch_cuda, case):
    drive(torch_cuda, scn_declined, case[0], case[1], 570)


# ---- 10. nosrplan ----------------------------------------------------------------------

def scn_off(d, seed):
    rng = np.random.default_rng(seed)
    with P.tune(nosrplan=1):
        w = send(d, rng, everyone(rng), "off", plan=False)
        left(d, "off")
        w.append(w[5])
        rows = recv(d, w, "off", "left")
    assert [r[0] for r in rows].count(EALREADY) == 1
    w = send(d, rng, everyone(rng), "on again")
    w.append(w[5])
    recv(d, w, "on again")
    return d.finish()


def test_nosrplan(torch_cuda):
    suite, flags = HMAC_CASES[0]
    drive(torch_cuda, scn_off, suite, flags, 580)


# ---- 11. RTP after SRTCP ------------------------------------------------------------------

def scn_rtp_after(d, seed):
    """the planner opens the stream RTP will use (0x7000) and another, mid-batch
    and in that order; then SRTCP on a third SSRC and RTP from just below
    65536: the RTP stream exists with s_l unset (scn_srtcp_first)"""
    rng = np.random.default_rng(seed)
    ss = [0x7000] * 10 + [0x9100] * 10
    pk = [(0, rtcp_packet(rng, x, 16)) for x in ss]
    swap(pk, 3, 12)
    rows = d.step("tx", "srtcp_encrypt", pk, what="opens")
    taken(d, "opens", rejects=True)
    d.step("rx", "srtcp_decrypt", wire_of(pk, rows), what="opens")
    taken(d, "opens", rejects=True)
    return scn_srtcp_first(d, seed, True)


@pytest.mark.parametrize("suite", [HMAC_CASES[0][0], GCM])
def test_rtp_after_srtcp(torch_cuda, suite):
    d = Drive(torch_cuda, suite, 0)
    try:
        scn_rtp_after(d, 590 + suite)
        first = [h for h in d.hist if h[2] == "first, srtcp"]
        assert len(first) == 2
        for side, op, what, ns, x in first:
            assert ns == 2 and (x["srplans"], x["rejects"]) == (1, 0), (side, x)
    finally:
        d.close()


# ---- 12. random traffic ---------------------------------------------------------------------

def scn_random(d, seed):
    rng = np.random.default_rng(seed)
    start, batches = T.random_batches(seed)
    for k, ix in sorted(start.items()):
        d.set_rtcp("tx", 0, X(k), (ix - 1) & 0x7fffffff, 0, 0)
    # (the receiver learns its streams from the traffic)
    wires = []
    for b, (sent, arrive, ndist) in enumerate(batches):
        w = send(d, rng, [k for k, _ in sent], ("random", b), plan=False)
        assert d.x["srplans"] == 1
        assert [index_of(d, p) for _, p in w] == [ix for _, ix in sent]
        wires.append(w)
        assert ndist > 0
        recv(d, [wires[bb][i] for bb, i in arrive], ("random", b))
        assert d.x["srplans"] == 1
    d.require("rx", {0, EALREADY})
    return d.finish()


@pytest.mark.parametrize("seed", T.SEEDS)
@pytest.mark.parametrize("suite,flags", HMAC_CASES[:2], ids=hmac_ids[:2])
def test_random_traffic_is_taken(torch_cuda, suite, flags, seed):
    drive(torch_cuda, scn_random, suite, flags, seed)
