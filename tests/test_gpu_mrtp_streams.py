"""The many-session RTP device planner for sessions of several SSRCs
(plan_buckets_rtp_streams.hip, batch_dev.c dev_msplanned): srtp_*_batch_dev
with a device session array and more than one session, up to 8 SSRCs per
session, every stream in order.

Every batch goes through PairDrive (tests/test_gpu_srtcp_multi.py): per packet
errno, pos, end and bytes, and per (session, SSRC) the exported RTP and SRTCP
state, against the oracle called one packet at a time.  MsDrive adds the
counter deltas around the product's call (msplans: accepted plans of this
planner; mplans / mrxplans: the one-stream bucket planners'; rejects; folds)
and runs the same batch on a second set of product contexts under
srtp_gpu_tune nomsplan=1 (the host engine behind dev_staged), compared against
the same oracle rows and states, with msplans +0 there.

A call reaches the planner two ways.  Sessions whose tables already hold
several streams: the bucket planner's gather leaves the batch, no plan is
tried (ACCEPT: msplans +1, rejects +0).  Fresh or one-stream sessions that
gain an SSRC in the batch: the bucket plan is rejected for the second SSRC and
counts it (FIRST: msplans +1, rejects +1).  Rejected: msplans +0, rejects +1,
the results still the oracle's.  Forged: msplans +0, folds >= 1, rejects +0.

Shape: 40 sessions at bpexp 250 are three buckets of 16, the last part-full.
One case cannot keep to 600 packets per batch: a session past SGPU_BP_SEGMAX
(1024) packets in its bucket needs 1025 of them; test_rejected_segmax sends
1100 packets of 12 bytes and says so, as tests/test_gpu_srtcp_mplan.py does.
"""
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests.test_gpu_fastpath import rtp_packet
from tests.test_gpu_srtcp import rtcp_packet
from tests.test_gpu_srtcp_multi import (PairDrive, Prod, ROOM, Twin, flipped,
                                        rtp_batch, scn_mux, ssrc_in, wire_of)

pytestmark = pytest.mark.gpu

ENOSR, ENOMEM, EALREADY, ETIMEDOUT = (errno.ENOSR, errno.ENOMEM,
                                      errno.EALREADY, errno.ETIMEDOUT)
CNT = ("msplans", "mplans", "mrxplans", "rejects", "folds", "misses")
ACCEPT = {"msplans": 1, "mplans": 0, "folds": 0, "rejects": 0}
FIRST = {"msplans": 1, "mplans": 0, "folds": 0, "rejects": 1}
REJECT = {"msplans": 0, "mplans": 0, "rejects": 1}
NOT_TAKEN = {"msplans": 0}
NSESS = 40
BPEXP = 250     # 40 sessions, <= 600 packets: 16 sessions per bucket, 3 buckets
SUITES = [1, 3, 5]      # AES-CM-128, AES-CM-256 (HMAC-SHA1-80), AES-256-GCM


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


def need(suite):
    """bytes srtp_encrypt appends"""
    return max(P.tag_len(suite), 4)


class CapTwin(Twin):
    """Twin with the fixed arena's rule for RTP (srtp.c cap_short): a protect
    whose tag does not fit fails with ENOMEM right after the stream lookup,
    pos past the header.  For a stream whose s_l is set the lookup changes
    nothing but may answer ENOSR; the scenarios here keep to those, with
    12-byte headers."""

    def run(self, op, pkts, rooms, fixed):
        rows = [None] * len(pkts)
        rest = []
        for i, ((s, p), room) in enumerate(zip(pkts, rooms)):
            if fixed and op == "srtp_encrypt" and len(p) >= 12 and \
                    room < need(self.suite):
                rest.append(i)
        for i, row in zip([i for i in range(len(pkts)) if i not in rest],
                          super().run(op, [q for i, q in enumerate(pkts)
                                           if i not in rest],
                                      [r for i, r in enumerate(rooms)
                                       if i not in rest], fixed)):
            rows[i] = row
        # (the short packets' streams exist: their lookups commute with the
        # other packets')
        for i in rest:
            s, p = pkts[i]
            c, x = self.ctx[s], ssrc_in(op, p)
            assert self.ob.rtcp_state(c, x) is not None
            rows[i] = (ENOMEM, 12, len(p), p)
        return rows


class MsDrive(PairDrive):
    """PairDrive on the "dev" entry that records the planners' counters and
    runs every batch again on contexts of its own under nomsplan=1"""

    def __init__(self, torch, suite, flags, nsess, entry="dev", limit=600):
        super().__init__(torch, suite, flags, nsess, entry)
        for k in ("tx", "rx"):
            self.twin[k].close()
            self.twin[k] = CapTwin(suite, self.flags[k])
        self.ref = {k: Prod(torch, suite, self.flags[k], entry)
                    for k in ("tx", "rx")}
        self.deltas = []
        self.limit = limit
        self.knobs = {}         # srtp_gpu_tune knobs around the product's call

    def close(self):
        super().close()
        for p in self.ref.values():
            p.close()

    def step(self, side, op, pkts, rooms=None, what=None, expect=None):
        c0 = {c: P.counter(c) for c in CNT}
        with P.tune(**self.knobs):
            if len(pkts) <= 600:
                rows = super().step(side, op, pkts, rooms, what, None)
            else:
                rows = self.big_step(side, op, pkts, what)
        dc = {c: P.counter(c) - c0[c] for c in CNT}
        self.deltas.append((what, side, op, dc))
        with P.tune(nomsplan=1):
            c1 = P.counter("msplans")
            ref = self.ref[side].run(op, pkts, self.log[-1][3])
            assert P.counter("msplans") == c1
        for i, (g, w) in enumerate(zip(ref, rows)):
            assert g[:3] == w[:3], (what, "nomsplan", i, g[:3], w[:3])
            assert g[3] == w[3], (what, "nomsplan", i, "bytes")
        for s, x in sorted(self.seen[side]):
            g, w = self.ref[side].state(s, x), self.twin[side].state(s, x)
            assert g == w, (what, "nomsplan state", s, hex(x), g, w)
        if expect is not None:
            assert {c: dc[c] for c in expect} == expect, (what, side, op, dc)
        return rows

    def big_step(self, side, op, pkts, what):
        """PairDrive.step for a batch past its 600 packets (module
        docstring): the same comparisons"""
        assert len(pkts) <= self.limit
        rooms = [ROOM] * len(pkts)
        rows = self.twin[side].run(op, pkts, rooms, self.fixed)
        self.seen[side].update((s, ssrc_in(op, p)) for s, p in pkts)
        self.log.append((side, op, list(pkts), rooms, rows))
        P.lib().srtp_gpu_tune(b"freshmulti", 0)
        got = self.prod[side].run(op, pkts, rooms)
        for i, (g, w) in enumerate(zip(got, rows)):
            assert g[:3] == w[:3], (what, i, g[:3], w[:3])
            assert g[3] == w[3], (what, i, "bytes")
        self.same_states(side, what)
        return rows


def drive(torch, scn, suite, nsess, *args, bpexp=BPEXP, **kw):
    d = MsDrive(torch, suite, 0, nsess)
    try:
        with P.tune(bpexp=bpexp):
            return scn(d, *args, **kw)
    finally:
        d.close()


def round_trip(d, pk, rooms=None, what=None, tx=ACCEPT, rx=ACCEPT):
    rows = d.step("tx", "srtp_encrypt", pk, rooms, what, expect=tx)
    wire = wire_of(pk, rows)
    d.step("rx", "srtp_decrypt", wire, what=what, expect=rx)
    return rows, wire


# ---- traffic ----------------------------------------------------------------

def ssrc_of(s, k):
    return 0x53000000 | (s << 8) | k


class Flow:
    """the senders: one seq counter per (session, stream), each starting a
    few packets below 65536 at its own distance, so the ROC rolls over inside
    a batch at a different place for every stream of a session"""

    def __init__(self, ssrc=ssrc_of, start=None):
        self.nxt = {}
        self.ssrc = ssrc
        self.start = start or (lambda s, k: 65536 - 1 - (s + 3 * k) % 7)

    def seq(self, s, k, step=1):
        v = self.nxt.setdefault((s, k), self.start(s, k))
        assert v >= 65400
        self.nxt[(s, k)] = v + step
        return v & 0xffff

    def batch(self, rng, who, plen=None, cc=0, x=False):
        """[(session, packet)] for [(session, stream)] in that order; bodies
        of every length mod 4 unless plen says otherwise"""
        return [(s, rtp_packet(rng, self.seq(s, k), self.ssrc(s, k), cc, x,
                               plen=int(rng.integers(0, 230))
                               if plen is None else plen)) for s, k in who]


def shuffled(rng, who):
    return [who[i] for i in rng.permutation(len(who)).tolist()]


def rtp_state(d, side, s, x):
    """(roc, s_l, lix, bitmap) of the oracle's stream"""
    return d.twin[side].state(s, x)[1]


# ---- accepted ---------------------------------------------------------------

def scn_accept(d, seed):
    """40 sessions in 3 buckets of 16 (bpexp 250), the last part-full.
    Session 0: 8 SSRCs new in batch 1 (it reaches exactly 8 inside the
    batch); session 1: 1 SSRC; session 2: 2; session 3: 3 SSRCs in batch 1
    and 5 more in batch 2 (exactly 8 again, 3 of them known); session 5's
    stream 0 carries the SSRC value of session 4's; session 6's stream 0 has
    over 80 packets per batch (a segment across waves, more than a window of
    bits); session 7: two streams in batch 1, in batch 2 only the second (a
    known stream without a packet, slot 0 idle); the others 1..3.  Every
    stream starts 1..7 packets below 65536.  Bodies of every length mod 4,
    cap exact on twelve packets.  Protect then unprotect, twice: streams
    made in batch 1 are known in batch 2.  Batch 1 meets fresh sessions: the
    bucket plan is tried and rejected for the second SSRCs (FIRST); batch 2
    meets tables with several streams (ACCEPT)."""
    rng = np.random.default_rng(seed)
    shared = ssrc_of(4, 0)
    fl = Flow(lambda s, k: shared if (s, k) == (5, 0) else ssrc_of(s, k))
    nss = {s: 1 + int(rng.integers(0, 3)) for s in range(NSESS)}
    nss[0], nss[1], nss[2], nss[3], nss[6], nss[7] = 8, 1, 2, 3, 2, 2
    for b in range(2):
        if b == 1:
            nss[3] = 8
        who = [(s, k) for s in range(NSESS) for k in range(nss[s])
               if not (b == 1 and (s, k) == (7, 0))] * 4
        who += [(6, 0)] * 78 + [(0, int(rng.integers(0, 8)))
                                for _ in range(40)]
        who += [(s, int(rng.integers(1 if s == 7 and b else 0, nss[s])))
                for s in rng.integers(0, NSESS, 560 - len(who)).tolist()]
        who = shuffled(rng, who)
        pk = fl.batch(rng, who)
        assert {len(p) % 4 for _, p in pk} == {0, 1, 2, 3} and len(pk) <= 600
        assert sum(1 for s, k in who if (s, k) == (6, 0)) > 64
        rooms = [ROOM] * len(pk)
        for i in rng.choice(len(pk), 12, replace=False).tolist():
            rooms[i] = need(d.suite)
        exp = FIRST if b == 0 else ACCEPT
        rows, _ = round_trip(d, pk, rooms, ("accept", b), tx=exp, rx=exp)
        assert not any(r[0] for r in rows)
    for side in ("tx", "rx"):
        assert [len([x for s, x in d.seen[side] if s == k])
                for k in (0, 1, 2, 3)] == [8, 1, 2, 8]
        # every stream of the first sessions rolled over, each at its place
        assert all(rtp_state(d, side, s, ssrc_of(s, k))[0] == 1
                   for s in (0, 2, 6) for k in range(nss[s]))
        assert all(d.twin[side].state(s, shared) is not None for s in (4, 5))
    assert len({fl.nxt[(0, k)] for k in range(8)}) > 1
    return d.log


@pytest.mark.parametrize("suite", SUITES)
def test_accepted(torch_cuda, suite):
    log = drive(torch_cuda, scn_accept, suite, NSESS, 500 + suite)
    assert len(log) == 4


def scn_two_batches(d, seed, nss=2, per=6, cc=0, x=False, plen=None):
    """every session with nss streams, `per` packets each per batch, protect
    and unprotect, twice: FIRST, then ACCEPT"""
    rng = np.random.default_rng(seed)
    fl = Flow()
    for b in range(2):
        who = shuffled(rng, [(s, k) for s in range(d.nsess)
                             for k in range(nss)] * per)
        exp = FIRST if b == 0 else ACCEPT
        rows, _ = round_trip(d, fl.batch(rng, who, plen, cc, x),
                             what=("two", b), tx=exp, rx=exp)
        assert not any(r[0] for r in rows)
    return fl


@pytest.mark.parametrize("knob", ["nolean", "nomk", "perclass"])
@pytest.mark.parametrize("suite", [1, 5])
def test_accepted_under_kernel_knobs(torch_cuda, suite, knob):
    """the crypto launches' knobs, one at a time: the planner's batches take
    the general kernels whatever they say"""
    d = MsDrive(torch_cuda, suite, 0, 12)
    d.knobs = {knob: 1}
    try:
        scn_two_batches(d, 520 + suite)
    finally:
        d.close()


def hdr_packet(rng, seq, ssrc, cc, xl, plen):
    """RTP with cc CSRCs and, for xl >= 0, an extension of xl words"""
    b = bytearray([0x80 | (0x10 if xl >= 0 else 0) | cc, 96,
                   (seq >> 8) & 0xff, seq & 0xff])
    b += int(rng.integers(0, 1 << 32)).to_bytes(4, "big")
    b += ssrc.to_bytes(4, "big")
    b += rng.integers(0, 256, 4 * cc, dtype=np.uint8).tobytes()
    if xl >= 0:
        b += b"\xbe\xde" + xl.to_bytes(2, "big")
        b += rng.integers(0, 256, 4 * xl, dtype=np.uint8).tobytes()
    return bytes(b + rng.integers(0, 256, plen, dtype=np.uint8).tobytes())


@pytest.mark.parametrize("suite", [1, 5])
def test_accepted_header_lengths_of_one_class(torch_cuda, suite):
    """headers of 12, 28 (4 CSRCs), 28 (an extension of 3 words), 44 (2
    CSRCs and an extension of 5) and 60 bytes: one class ((len >> 2) & 3),
    one plan"""
    shapes = [(0, -1), (4, -1), (0, 3), (2, 5), (8, 3)]
    d = MsDrive(torch_cuda, suite, 0, 12)
    rng = np.random.default_rng(530 + suite)
    fl = Flow()
    try:
        for b in range(2):
            who = shuffled(rng, [(s, k) for s in range(12)
                                 for k in range(2)] * 5)
            pk = []
            for i, (s, k) in enumerate(who):
                cc, xl = shapes[i % len(shapes)]
                pk.append((s, hdr_packet(rng, fl.seq(s, k), ssrc_of(s, k), cc,
                                         xl, int(rng.integers(0, 200)))))
            exp = FIRST if b == 0 else ACCEPT
            rows, _ = round_trip(d, pk, what=("hdr", b), tx=exp, rx=exp)
            assert not any(r[0] for r in rows)
    finally:
        d.close()


def scn_srtcp_first(d, seed, both):
    """fresh contexts get an SRTCP batch and then RTP in order from just
    below 65536: the RTP stream exists with s_l unset (both: SRTCP ran on
    the RTP SSRC and on another one, so the tables hold two streams and
    slot 0 stays idle) or is new behind SRTCP's stream (the bucket plan sees
    a second SSRC: FIRST); the first RTP seq becomes s_l (stream.c:87-109)"""
    rng = np.random.default_rng(seed)
    n = d.nsess
    fl = Flow(lambda s, k: 0x7000 + s, lambda s, k: 65530 + s % 4)
    pk = [(s, rtcp_packet(rng, 0x9000 + s if k == 0 else 0x7000 + s,
                          4 * int(rng.integers(0, 65))))
          for s in range(n) for k in range(2 if both else 1) for _ in range(4)]
    rows = d.step("tx", "srtcp_encrypt", pk, what="first, srtcp")
    rows = d.step("rx", "srtcp_decrypt", wire_of(pk, rows),
                  what="first, srtcp")
    assert not any(r[0] for r in rows)
    for b in range(2):
        who = shuffled(rng, [(s, 0) for s in range(n)] * 10)
        exp = ACCEPT if both or b else FIRST
        rows, _ = round_trip(d, fl.batch(rng, who), what=("first, rtp", b),
                             tx=exp, rx=exp)
        assert not any(r[0] for r in rows)
    for side in ("tx", "rx"):
        for s in range(n):
            assert rtp_state(d, side, s, 0x7000 + s)[:2] == \
                (1, (fl.nxt[(s, 0)] - 1) & 0xffff), (side, s)
    return d.log


@pytest.mark.parametrize("both", [True, False], ids=["known", "new"])
@pytest.mark.parametrize("suite", [1, 5])
def test_stream_srtcp_created_first(torch_cuda, suite, both):
    drive(torch_cuda, scn_srtcp_first, suite, 24, 540 + suite, both)


# ---- rejected ---------------------------------------------------------------

def scn_reject(d, seed, case):
    """12 sessions of two SSRCs (session 3: eight), a clean round trip from
    just below 65536 that rolls every stream over, then one batch with one
    trouble in stream 1 of session 5, whose stream 0 is clean"""
    rng = np.random.default_rng(seed)
    n = d.nsess
    fl = Flow(start=lambda s, k: 65535 - (s + k) % 3)
    streams = [(s, k) for s in range(n) for k in range(8 if s == 3 else 2)]
    round_trip(d, fl.batch(rng, shuffled(rng, streams * 5)), what=(case, 0),
               tx=FIRST, rx=FIRST)
    wire0 = d.log[-1][2]
    who = shuffled(rng, streams * 5)
    mine = [i for i, w in enumerate(who) if w == (5, 1)]
    at = mine[2]
    if case == "jump":
        fl.nxt[(5, 1)] += 40000         # (seq 40000-odd: no rollover near)
    pk = fl.batch(rng, who, cc=0)
    rooms = [ROOM] * len(pk)
    tx, codes = ACCEPT, {"tx": {0}, "rx": {0}}
    if case == "ninth":
        pk[at] = (3, rtp_packet(rng, 7, ssrc_of(3, 0x33), plen=20))
        tx, codes["tx"] = REJECT, {0, ENOSR}
    elif case == "cap_short":
        rooms[at] = need(d.suite) - 1
        tx, codes["tx"] = REJECT, {0, ENOMEM}
    elif case == "classes":
        s, p = pk[at]
        pk[at] = (s, hdr_packet(rng, int.from_bytes(p[2:4], "big"),
                                ssrc_of(5, 1), 1, -1, 40))
        tx = REJECT
    rows = d.step("tx", "srtp_encrypt", pk, rooms, (case, 1), expect=tx)
    assert {r[0] for r in rows} == codes["tx"]
    wire = wire_of(pk, rows)
    rx = REJECT if case == "classes" else ACCEPT
    if case in ("ninth", "cap_short"):
        # the refused packet does not arrive
        wire = [w for i, w in enumerate(wire) if i != at]
    elif case == "swap":
        i, j = mine[1], mine[2]
        wire[i], wire[j] = wire[j], wire[i]
        rx = REJECT     # both are new to the window: the oracle takes them
    elif case == "dup":
        wire.insert(at + 7, wire[at])
        rx, codes["rx"] = REJECT, {0, EALREADY}
    elif case == "replay":
        old = [w for w in wire0 if w[0] == 5 and
               ssrc_in("srtp_decrypt", w[1]) == ssrc_of(5, 1)][-1]
        wire.insert(at, old)
        rx, codes["rx"] = REJECT, {0, EALREADY}
    elif case == "jump":
        rx, codes["rx"] = REJECT, {0, ETIMEDOUT}
    rows = d.step("rx", "srtp_decrypt", wire, what=(case, 1), expect=rx)
    assert {r[0] for r in rows} == codes["rx"]
    # stream 0 of the session went on undisturbed
    assert rtp_state(d, "rx", 5, ssrc_of(5, 0))[:2] == \
        (1, (fl.nxt[(5, 0)] - 1) & 0xffff)
    return d.log


REJECTS = ("swap", "dup", "replay", "jump", "ninth", "cap_short", "classes")


@pytest.mark.parametrize("case", REJECTS)
def test_rejected(torch_cuda, case):
    """AES_CM_128_HMAC_SHA1_80, 12 sessions"""
    drive(torch_cuda, scn_reject, 1, 12, 550 + REJECTS.index(case), case,
          bpexp=0)


def test_rejected_segmax(torch_cuda):
    """a session with more than SGPU_BP_SEGMAX (1024) packets in its bucket
    at a small bpexp: 1100 packets of 12 bytes, 1040 of them session 0's two
    streams' (the module docstring: no batch of 600 can get there); and one
    of 500 is planned"""
    d = MsDrive(torch_cuda, 1, 0, 6, limit=1100)
    rng = np.random.default_rng(561)
    fl = Flow()
    try:
        with P.tune(bpexp=400):
            who = shuffled(rng, [(s, k) for s in range(6) for k in range(2)])
            round_trip(d, fl.batch(rng, who, plen=0), what="segmax, first",
                       tx=FIRST, rx=FIRST)
            who = shuffled(rng, [(0, 0), (0, 1)] * 520 +
                           [(s, 0) for s in range(1, 6)] * 12)
            pk = fl.batch(rng, who, plen=0)
            rows = d.step("tx", "srtp_encrypt", pk, what="segmax",
                          expect=REJECT)
            assert not any(r[0] for r in rows)
            d.step("rx", "srtp_decrypt", wire_of(pk, rows), what="segmax",
                   expect=REJECT)
            who = shuffled(rng, [(0, 0), (0, 1)] * 250 +
                           [(s, 0) for s in range(1, 6)] * 12)
            round_trip(d, fl.batch(rng, who, plen=0), what="below segmax")
    finally:
        d.close()


# ---- forged -----------------------------------------------------------------

def scn_forged(d, seed):
    """12 sessions of two SSRCs behind a clean round trip: a bit flipped in
    one tag, then in one body with, in the same batch, a forged packet of an
    SSRC nothing else carries (stream_get_seq precedes the tag check: the
    SSRC takes a slot).  The plan holds, the crypto launch counts the
    misses, everything is undone and the host engine folds: EAUTH on those
    packets alone"""
    rng = np.random.default_rng(seed)
    fl = Flow()
    streams = [(s, k) for s in range(d.nsess) for k in range(2)] * 3
    round_trip(d, fl.batch(rng, shuffled(rng, streams)), what=("forged", 0),
               tx=FIRST, rx=FIRST)
    for b in (1, 2):
        who = shuffled(rng, streams)
        if b == 2:
            who.insert(60, (7, 0x77))
        pk = fl.batch(rng, who, plen=64)
        rows = d.step("tx", "srtp_encrypt", pk, what=("forged", b),
                      expect=ACCEPT)
        wire = wire_of(pk, rows)
        bad = [40] if b == 1 else [40, 60]
        for i in bad:
            s, w = wire[i]
            wire[i] = (s, flipped(w, 12 + 30 if (b, i) == (2, 40)
                                  else len(w) - 1, 0x40))
        rows = d.step("rx", "srtp_decrypt", wire, what=("forged", b))
        dc = d.deltas[-1][3]
        assert dc["msplans"] == 0 and dc["rejects"] == 0 and \
            dc["folds"] >= 1 and dc["misses"] >= len(bad), dc
        assert [i for i, r in enumerate(rows) if r[0]] == bad
        assert all(rows[i][0] == P.EAUTH for i in bad)
    assert d.twin["rx"].state(7, ssrc_of(7, 0x77)) is not None
    return d.log


@pytest.mark.parametrize("suite", [1, 5])
def test_forged(torch_cuda, suite):
    drive(torch_cuda, scn_forged, suite, 12, 570 + suite, bpexp=0)


# ---- not taken ----------------------------------------------------------------

@pytest.mark.parametrize("knob", ["nomsplan", "noplan"])
def test_not_taken_switched_off(torch_cuda, knob):
    """12 sessions whose tables hold two streams: with the planner (or every
    device planner) switched off the host engine answers, msplans +0; without
    the knob the same traffic is planned"""
    d = MsDrive(torch_cuda, 1, 0, 12)
    rng = np.random.default_rng(580)
    try:
        fl = scn_two_batches(d, 581)
        who = shuffled(rng, [(s, k) for s in range(12) for k in range(2)] * 4)
        d.knobs = {knob: 1}
        rows, _ = round_trip(d, fl.batch(rng, who), what=knob, tx=NOT_TAKEN,
                             rx=NOT_TAKEN)
        assert not any(r[0] for r in rows)
        d.knobs = {}
        round_trip(d, fl.batch(rng, who), what="on again")
    finally:
        d.close()


@pytest.mark.parametrize("entry", ["dev", "dev1"])
def test_not_taken_one_session(torch_cuda, entry):
    """one session of three SSRCs, with a session array (nsess == 1 is not
    this planner's) and without one: msplans +0"""
    d = MsDrive(torch_cuda, 1, 0, 1, entry=entry)
    rng = np.random.default_rng(585)
    fl = Flow()
    try:
        for b in range(2):
            who = shuffled(rng, [(0, k) for k in range(3)] * 20)
            rows, _ = round_trip(d, fl.batch(rng, who), what=(entry, b),
                                 tx=NOT_TAKEN, rx=NOT_TAKEN)
            assert not any(r[0] for r in rows)
    finally:
        d.close()


# ---- beside the other planners ---------------------------------------------------

def test_one_stream_paths_unchanged(torch_cuda):
    """24 sessions of one SSRC each, in order: the bucket planner as before
    (mplans +1, msplans +0); then the same sessions' arrivals reordered
    inside a session: the bucket receive planner (mrxplans +1, msplans +0)"""
    one = {"mplans": 1, "msplans": 0, "rejects": 0}
    d = MsDrive(torch_cuda, 1, 0, 24)
    rng = np.random.default_rng(590)
    nxt = [65400 + 7 * s for s in range(24)]
    try:
        for b in range(2):
            pk = rtp_batch(rng, nxt, 400, lambda s: 0x7000 + s)
            rows = d.step("tx", "srtp_encrypt", pk, what=("one", b),
                          expect=one)
            wire = wire_of(pk, rows)
            rx = one
            if b == 1:
                i, j = [i for i, (s, _) in enumerate(wire) if s == 9][3:5]
                wire[i], wire[j] = wire[j], wire[i]
                rx = {"mrxplans": 1, "msplans": 0, "mplans": 0}
            rows = d.step("rx", "srtp_decrypt", wire, what=("one", b),
                          expect=rx)
            assert not any(r[0] for r in rows)
    finally:
        d.close()


@pytest.mark.parametrize("suite", [1, 5])
def test_rtp_and_srtcp_in_turn(torch_cuda, suite):
    """scn_mux on 24 sessions: the first RTP batch is the bucket planner's
    (scn_mux asserts mplans 1); the SRTCP batches give a third of the
    sessions a second SSRC, so the RTP batches behind them are this
    planner's (msplans 1, no plan rejected before it) -- but the last
    receive batch, whose forged packet the host engine folds; the states
    agree after every batch (PairDrive)"""
    d = MsDrive(torch_cuda, suite, 0, 24)
    try:
        scn_mux(d, 595 + suite)
        rtp = [(what[1], side, dc) for what, side, op, dc in d.deltas
               if op.startswith("srtp_") and what and what[0] == "mux"]
        assert [(b, side) for b, side, _ in rtp] == \
            [(b, side) for b in (0, 2, 4) for side in ("tx", "rx")]
        for b, side, dc in rtp:
            if b == 0:
                assert dc["mplans"] == 1 and dc["msplans"] == 0, (b, side, dc)
            elif (b, side) == (4, "rx"):
                assert dc["msplans"] == 0 and dc["folds"] >= 1 and \
                    dc["rejects"] == 0, (b, side, dc)
            else:
                assert {c: dc[c] for c in ACCEPT} == ACCEPT, (b, side, dc)
    finally:
        d.close()
