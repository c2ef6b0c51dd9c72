"""The receive planner for reordered many-session batches whose sessions carry
several SSRCs (plan_buckets_rtp_streams_rx.hip, batch_dev.c dev_msrxplanned):
srtp_decrypt_batch_dev with a device session array, up to 8 SSRCs per
session, some stream arriving with a swap, a loss, a duplicate or a replay of
the batch before.

Every batch goes through MsDrive (tests/test_gpu_mrtp_streams.py) on PairDrive
(tests/test_gpu_srtcp_multi.py): per packet errno, pos, end and bytes, and per
(session, SSRC) the exported state, against the oracle called one packet at a
time, and against the same call on contexts of their own under nomsplan=1 (the
host engine).  Counter deltas are asserted per call: "msrxplans" (accepted
plans of this planner), "rxlate" / "rxdups" (its late and EALREADY packets),
and MsDrive's msplans / mplans / mrxplans / rejects / folds / misses.

The planner runs behind a plan of dev_msplanned rejected for the order or a
replayed index only, so an accepted batch shows TAKEN: msrxplans +1, rejects
+1 (the rejected in-order plan), every other planner +0, folds 0.

Shapes: 40 sessions at bpexp 250 are three buckets of 16, the last part-full;
12 sessions at bpexp 0 for single troubles; one session with a 150-packet
stream, whose segment crosses the waves of the scan.  No batch passes 600
packets.
"""
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import msrx_traffic as T
from tests.test_gpu_fastpath import rtp_packet
from tests.test_gpu_mrtp_streams import (ACCEPT, BPEXP, FIRST, Flow, MsDrive,
                                         hdr_packet, round_trip, rtp_state,
                                         shuffled, ssrc_of)
from tests.test_gpu_srtcp import rtcp_packet
from tests.test_gpu_srtcp_multi import (ROOM, Twin, flipped, rtp_batch, ssrc_in,
                                        wire_of)

pytestmark = pytest.mark.gpu

ENOSR, EALREADY, ETIMEDOUT = errno.ENOSR, errno.EALREADY, errno.ETIMEDOUT
XCNT = ("msrxplans", "rxlate", "rxdups")
TAKEN = {"msplans": 0, "mplans": 0, "mrxplans": 0, "rejects": 1, "folds": 0}
LEFT = {"msplans": 0, "mplans": 0, "mrxplans": 0, "rejects": 1}
NSESS = 40


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


class Drive(MsDrive):
    """MsDrive that also records this planner's counters around the
    product's call alone (d.x)"""

    def __init__(self, torch, suite, nsess, entry="dev"):
        super().__init__(torch, suite, 0, nsess, entry)
        self.x = {}
        for p in self.prod.values():
            p.run = self.counted(p.run)

    def counted(self, run):
        def wrapped(op, pkts, rooms):
            c0 = {c: P.counter(c) for c in XCNT}
            out = run(op, pkts, rooms)
            self.x = {c: P.counter(c) - c0[c] for c in XCNT}
            return out
        return wrapped

    def rx(self, wire, what, expect, msrx, codes={0}, late=None, dups=None):
        rows = self.step("rx", "srtp_decrypt", wire, what=what, expect=expect)
        assert self.x["msrxplans"] == msrx, (what, self.x, self.deltas[-1])
        assert {r[0] for r in rows} == set(codes), what
        if late is not None:
            assert self.x["rxlate"] == late, (what, self.x)
        if dups is not None:
            assert self.x["rxdups"] == dups, (what, self.x)
            assert sum(1 for r in rows if r[0] == EALREADY) == dups
        return rows

    def in_order(self, rng, fl, who, what):
        """a later batch in order on the same contexts: the in-order planner
        takes it again, so the applied state is right"""
        round_trip(self, fl.batch(rng, who), what=what, tx=ACCEPT, rx=ACCEPT)
        assert self.x["msrxplans"] == 0


class Air:
    """what the network does to one batch: who[i] = (session, stream) of
    wire[i]; a stream's arrivals are counted from 0"""

    def __init__(self, who, wire):
        self.who, self.wire = who, wire
        self.slot = list(range(len(wire)))
        self.after = {}

    def at(self, key, a):
        return [i for i, w in enumerate(self.who) if w == key][a]

    def swap(self, key, a, d=1):
        i, j = self.at(key, a), self.at(key, a + d)
        self.slot[i], self.slot[j] = self.slot[j], self.slot[i]

    def lose(self, key, a):
        self.slot[self.at(key, a)] = None

    def inject(self, key, a, pkt):
        """pkt arrives right behind the stream's arrival a"""
        self.after.setdefault(self.at(key, a), []).append(pkt)

    def dup(self, key, a, later):
        self.inject(key, a + later, self.wire[self.at(key, a)])

    def out(self):
        res = []
        for place, i in enumerate(self.slot):
            if i is not None:
                res.append(self.wire[i])
            res += self.after.get(place, [])
        assert len(res) <= 600
        return res


def last_of(wire, s, ssrc):
    """the stream's last packet on a batch's wire"""
    return [w for w in wire if w[0] == s and
            ssrc_in("srtp_decrypt", w[1]) == ssrc][-1]


def calm(s, k):
    """streams 40-46 packets below 65536: no rollover near these batches"""
    return 65536 - 40 - (s + 3 * k) % 7


def sent(d, rng, fl, who, what, tx=ACCEPT, **kw):
    """one batch protected in order: (who, its wire)"""
    pk = fl.batch(rng, who, **kw)
    rows = d.step("tx", "srtp_encrypt", pk, what=what, expect=tx)
    assert not any(r[0] for r in rows)
    return Air(who, wire_of(pk, rows))


# ---- accepted ---------------------------------------------------------------

def scn_mixed(d, seed):
    """40 sessions in 3 buckets of 16 (bpexp 250), the last part-full, 2-3
    SSRCs each and session 3 with eight.  Behind a clean round trip, one batch
    with: an adjacent swap, a swap 5 apart, a loss next to a swap, a duplicate
    inside the batch, a replay of the batch before's last packet (from
    bitmap0) in the last bucket, two streams of one session disturbed, all
    eight streams of session 3 disturbed.  Then a batch in order."""
    rng = np.random.default_rng(seed)
    fl = Flow(start=calm)
    streams = [(s, k) for s in range(NSESS)
               for k in range(8 if s == 3 else 2 + (s % 5 == 0))]
    round_trip(d, fl.batch(rng, shuffled(rng, streams * 5)),
               what=("mixed", 0), tx=FIRST, rx=FIRST)
    wire0 = d.log[-1][2]
    air = sent(d, rng, fl, shuffled(rng, streams * 6), ("mixed", 1))
    air.swap((5, 1), 1)
    air.swap((20, 0), 0, 5)
    air.lose((33, 1), 1)
    air.swap((33, 1), 3)
    air.dup((7, 0), 1, 2)
    air.inject((39, 1), 2, last_of(wire0, 39, ssrc_of(39, 1)))
    air.swap((12, 0), 2)
    air.swap((12, 1), 0)
    for k in range(8):
        air.swap((3, k), k % 5)
    d.rx(air.out(), ("mixed", 1), TAKEN, 1, {0, EALREADY},
         late=1 + 5 + 1 + 2 + 8, dups=2)
    d.in_order(rng, fl, shuffled(rng, streams * 3), ("mixed", 2))


@pytest.mark.parametrize("suite", [1, 3, 5])
def test_accepted(torch_cuda, suite):
    """AES-CM-128, AES-CM-256 (HMAC-SHA1-80: an EALREADY packet is not
    decrypted) and AES-256-GCM (it decrypts to authenticate)"""
    d = Drive(torch_cuda, suite, NSESS)
    try:
        with P.tune(bpexp=BPEXP):
            scn_mixed(d, 700 + suite)
    finally:
        d.close()


SINGLES = ("swap1", "swap5", "loss", "dup", "replay", "two_streams",
           "eight_streams", "new_stream")


def scn_single(d, seed, case):
    """12 sessions of two SSRCs (session 3: eight) behind a clean round trip,
    then one batch with one trouble, then a batch in order"""
    rng = np.random.default_rng(seed)
    fl = Flow(start=calm)
    streams = [(s, k) for s in range(d.nsess)
               for k in range(8 if s == 3 else 2)]
    round_trip(d, fl.batch(rng, shuffled(rng, streams * 5)), what=(case, 0),
               tx=FIRST, rx=FIRST)
    wire0 = d.log[-1][2]
    who = streams * 6
    if case == "new_stream":
        who = who + [(6, 2)] * 4
    air = sent(d, rng, fl, shuffled(rng, who), (case, 1))
    late, dups = 1, 0
    if case == "swap1":
        air.swap((5, 1), 2)
    elif case == "swap5":
        air.swap((5, 1), 0, 5)
        late = 5
    elif case == "loss":
        air.lose((5, 1), 2)
        air.swap((5, 1), 3)
    elif case == "dup":
        air.dup((5, 1), 2, 2)
        late, dups = 0, 1
    elif case == "replay":
        air.inject((5, 1), 2, last_of(wire0, 5, ssrc_of(5, 1)))
        late, dups = 0, 1
    elif case == "two_streams":
        air.swap((5, 0), 1)
        air.swap((5, 1), 3)
        late = 2
    elif case == "eight_streams":
        for k in range(8):
            air.swap((3, k), k % 4)
        late = 8
    elif case == "new_stream":
        # its first arrival sets s_l, the one sent before it comes late
        air.swap((6, 2), 0)
    d.rx(air.out(), (case, 1), TAKEN, 1, {0, EALREADY} if dups else {0},
         late=late, dups=dups)
    d.in_order(rng, fl, shuffled(rng, streams * 3), (case, 2))
    if case == "new_stream":
        assert rtp_state(d, "rx", 6, ssrc_of(6, 2))[1] == \
            (fl.nxt[(6, 2)] - 1) & 0xffff


@pytest.mark.parametrize("case", SINGLES)
def test_accepted_single_trouble(torch_cuda, case):
    """AES_CM_128_HMAC_SHA1_80, 12 sessions, bpexp 0"""
    d = Drive(torch_cuda, 1, 12)
    try:
        with P.tune(bpexp=0):
            scn_single(d, 720 + SINGLES.index(case), case)
    finally:
        d.close()


@pytest.mark.parametrize("case", ["dup", "replay"])
def test_accepted_gcm_already(torch_cuda, case):
    """AES-256-GCM: the EALREADY packet is decrypted to authenticate it, and
    its bytes are the oracle's"""
    d = Drive(torch_cuda, 5, 12)
    try:
        with P.tune(bpexp=0):
            scn_single(d, 735, case)
    finally:
        d.close()


def test_accepted_stream_srtcp_created(torch_cuda):
    """fresh contexts get SRTCP on two SSRCs, one of them the RTP stream's:
    it exists with s_l not set.  The first RTP batch arrives with session 2's
    first two packets swapped (s_l is the first arrival's seq) and a swap
    further on in session 7"""
    d = Drive(torch_cuda, 1, 12)
    rng = np.random.default_rng(740)
    fl = Flow(lambda s, k: 0x7000 + s, lambda s, k: 65400 + s % 4)
    try:
        with P.tune(bpexp=0):
            pk = [(s, rtcp_packet(rng, 0x9000 + s if k == 0 else 0x7000 + s,
                                  4 * int(rng.integers(0, 65))))
                  for s in range(12) for k in range(2) for _ in range(3)]
            rows = d.step("tx", "srtcp_encrypt", pk, what="srtcp")
            rows = d.step("rx", "srtcp_decrypt", wire_of(pk, rows),
                          what="srtcp")
            assert not any(r[0] for r in rows)
            streams = [(s, 0) for s in range(12)]
            air = sent(d, rng, fl, shuffled(rng, streams * 10), "rtp")
            air.swap((2, 0), 0)
            air.swap((7, 0), 3)
            d.rx(air.out(), "rtp", TAKEN, 1, late=2, dups=0)
            d.in_order(rng, fl, shuffled(rng, streams * 5), "rtp, in order")
    finally:
        d.close()


def test_accepted_rollover_inside_the_batch(torch_cuda):
    """every stream rolls over at its 8th packet of the batch; swaps 5 before
    and 4 behind the rollover, a duplicate 5 behind it"""
    d = Drive(torch_cuda, 1, 12)
    rng = np.random.default_rng(745)
    fl = Flow(start=lambda s, k: 65536 - 12)
    streams = [(s, k) for s in range(12) for k in range(2)]
    try:
        with P.tune(bpexp=0):
            round_trip(d, fl.batch(rng, shuffled(rng, streams * 5)),
                       what=("roll", 0), tx=FIRST, rx=FIRST)
            air = sent(d, rng, fl, shuffled(rng, streams * 14), ("roll", 1))
            air.swap((5, 1), 1)         # seqs 65530, 65531
            air.swap((5, 1), 11)        # seqs 4, 5
            air.dup((8, 0), 11, 1)      # seq 4
            d.rx(air.out(), ("roll", 1), TAKEN, 1, {0, EALREADY}, late=2,
                 dups=1)
            assert all(rtp_state(d, "rx", s, ssrc_of(s, k))[:2] == (1, 6)
                       for s, k in streams)
            d.in_order(rng, fl, shuffled(rng, streams * 3), ("roll", 2))
    finally:
        d.close()


def test_accepted_long_stream(torch_cuda):
    """session 4's stream 0 has 150 packets in the batch: its segment crosses
    the waves of the scan, and more arrivals than a window holds lie between
    its troubles"""
    d = Drive(torch_cuda, 1, 12)
    rng = np.random.default_rng(750)
    fl = Flow(start=lambda s, k: 66536 if (s, k) == (4, 0) else calm(s, k))
    streams = [(s, k) for s in range(12) for k in range(2)]
    try:
        with P.tune(bpexp=0):
            round_trip(d, fl.batch(rng, shuffled(rng, streams * 5), plen=40),
                       what=("long", 0), tx=FIRST, rx=FIRST)
            air = sent(d, rng, fl, shuffled(rng, streams * 4 + [(4, 0)] * 146),
                       ("long", 1), plen=40)
            air.swap((4, 0), 60)
            air.swap((4, 0), 100, 5)
            air.dup((4, 0), 120, 3)
            air.lose((4, 0), 130)
            air.swap((4, 0), 140)
            d.rx(air.out(), ("long", 1), TAKEN, 1, {0, EALREADY}, late=7,
                 dups=1)
            d.in_order(rng, fl, shuffled(rng, streams * 3), ("long", 2))
    finally:
        d.close()


# ---- still rejected ----------------------------------------------------------

REJECTS = ("jump", "before_rollover", "ninth", "classes")


def scn_reject(d, seed, case):
    """12 sessions of two SSRCs (session 3: eight) behind a clean round trip
    that rolls every stream over; one batch with a swap in session 2 and, in
    session 5, what no device planner settles: the host engine answers"""
    rng = np.random.default_rng(seed)
    fl = Flow(start=(lambda s, k: 65536 - 8) if case == "before_rollover"
              else (lambda s, k: 65535 - (s + k) % 3))
    streams = [(s, k) for s in range(d.nsess)
               for k in range(8 if s == 3 else 2)]
    round_trip(d, fl.batch(rng, shuffled(rng, streams * 5)), what=(case, 0),
               tx=FIRST, rx=FIRST)
    who = shuffled(rng, streams * 6)
    codes, tx = {0}, ACCEPT
    if case == "jump":
        fl.nxt[(5, 1)] += 40000
    pk = fl.batch(rng, who)
    if case == "classes":
        at = [i for i, w in enumerate(who) if w == (5, 1)][2]
        s, p = pk[at]
        pk[at] = (s, hdr_packet(rng, int.from_bytes(p[2:4], "big"),
                                ssrc_of(5, 1), 1, -1, 40))
        tx = LEFT
    rows = d.step("tx", "srtp_encrypt", pk, what=(case, 1), expect=tx)
    assert not any(r[0] for r in rows)
    air = Air(who, wire_of(pk, rows))
    if case == "before_rollover":
        # seqs 65533 65534 65535 0 1 2: 65535 arrives behind 0
        air.swap((5, 1), 2)
        codes = {0, ETIMEDOUT}
    else:
        air.swap((2, 0), 2)
    if case == "jump":
        codes = {0, ETIMEDOUT}
    elif case == "ninth":
        snd = Twin(d.suite, d.flags["tx"])
        row = snd.run("srtp_encrypt",
                      [(3, rtp_packet(rng, 7, ssrc_of(3, 0x33), plen=20))],
                      [ROOM], False)[0]
        snd.close()
        assert row[0] == 0
        air.inject((5, 1), 2, (3, row[3][:row[2]]))
        codes = {0, ENOSR}
    d.rx(air.out(), (case, 1), LEFT, 0, codes)


@pytest.mark.parametrize("case", REJECTS)
def test_still_rejected(torch_cuda, case):
    d = Drive(torch_cuda, 1, 12)
    try:
        with P.tune(bpexp=0):
            scn_reject(d, 760 + REJECTS.index(case), case)
    finally:
        d.close()


@pytest.mark.parametrize("suite", [1, 5])
def test_forged(torch_cuda, suite):
    """a swap in session 2 and a bit flipped in a tag of session 5: this
    planner's plan holds, the crypto launch counts the miss, everything is
    undone and the host engine folds: EAUTH on that packet alone"""
    d = Drive(torch_cuda, suite, 12)
    rng = np.random.default_rng(770 + suite)
    fl = Flow(start=calm)
    streams = [(s, k) for s in range(12) for k in range(2)]
    try:
        with P.tune(bpexp=0):
            round_trip(d, fl.batch(rng, shuffled(rng, streams * 5)),
                       what=("forged", 0), tx=FIRST, rx=FIRST)
            air = sent(d, rng, fl, shuffled(rng, streams * 6), ("forged", 1),
                       plen=64)
            bad = air.at((5, 1), 3)
            s, w = air.wire[bad]
            air.wire[bad] = (s, flipped(w, len(w) - 1, 0x40))
            air.swap((2, 0), 2)
            rows = d.step("rx", "srtp_decrypt", air.out(), what=("forged", 1),
                          expect=LEFT)
            dc = d.deltas[-1][3]
            assert d.x["msrxplans"] == 0 and dc["folds"] >= 1 and \
                dc["misses"] >= 1, (d.x, dc)
            assert [r[0] for r in rows].count(P.EAUTH) == 1
            assert {r[0] for r in rows} == {0, P.EAUTH}
    finally:
        d.close()


# ---- not taken ----------------------------------------------------------------

def test_not_taken_switched_off(torch_cuda):
    """nomsrxplan=1: the rejected in-order plan goes straight to the host
    engine; nomsplan=1: no plan of either; without a knob the same trouble is
    this planner's"""
    d = Drive(torch_cuda, 1, 12)
    rng = np.random.default_rng(780)
    fl = Flow(start=calm)
    streams = [(s, k) for s in range(12) for k in range(2)]
    try:
        with P.tune(bpexp=0):
            round_trip(d, fl.batch(rng, shuffled(rng, streams * 4)),
                       what=("off", 0), tx=FIRST, rx=FIRST)
            for b, (knobs, expect, msrx) in enumerate((
                    ({"nomsrxplan": 1}, LEFT, 0),
                    ({"nomsplan": 1}, {"msplans": 0, "folds": 0}, 0),
                    ({}, TAKEN, 1))):
                air = sent(d, rng, fl, shuffled(rng, streams * 4), ("off", b))
                air.swap((5, 1), 1)
                d.knobs = knobs
                d.rx(air.out(), ("off", b, tuple(knobs)), expect, msrx)
                d.knobs = {}
    finally:
        d.close()


@pytest.mark.parametrize("entry", ["dev", "dev1"])
def test_not_taken_one_session(torch_cuda, entry):
    """one session of three SSRCs, with a session array and without one,
    reordered: not this planner's"""
    d = Drive(torch_cuda, 1, 1, entry=entry)
    rng = np.random.default_rng(785)
    fl = Flow(start=calm)
    try:
        for b in range(2):
            who = shuffled(rng, [(0, k) for k in range(3)] * 20)
            pk = fl.batch(rng, who)
            rows = d.step("tx", "srtp_encrypt", pk, what=(entry, b))
            air = Air(who, wire_of(pk, rows))
            air.swap((0, 1), 4)
            d.rx(air.out(), (entry, b), {"msplans": 0}, 0)
    finally:
        d.close()


def test_one_stream_per_session_is_the_bucket_receive_planners(torch_cuda):
    """24 sessions of one SSRC each, a swap inside session 9: mrxplans +1 as
    before, this planner +0"""
    d = Drive(torch_cuda, 1, 24)
    rng = np.random.default_rng(790)
    nxt = [65400 + 7 * s for s in range(24)]
    try:
        for b in range(2):
            pk = rtp_batch(rng, nxt, 400, lambda s: 0x7000 + s)
            rows = d.step("tx", "srtp_encrypt", pk, what=("one", b),
                          expect={"mplans": 1, "msplans": 0, "rejects": 0})
            wire = wire_of(pk, rows)
            i, j = [i for i, (s, _) in enumerate(wire) if s == 9][3:5]
            wire[i], wire[j] = wire[j], wire[i]
            d.rx(wire, ("one", b),
                 {"mrxplans": 1, "msplans": 0, "mplans": 0, "rejects": 1}, 0)
    finally:
        d.close()


# ---- random traffic ------------------------------------------------------------

@pytest.mark.parametrize("suite", [1, 5])
def test_random_traffic_is_always_accepted(torch_cuda, suite):
    """tests/msrx_traffic.py: 40 sessions of 2-3 SSRCs, swaps up to 8 apart,
    loss and duplicates at a few percent per stream, nothing near a rollover
    (tests/test_rtp_seg_rx_rule.py: the sequential receiver answers 0 /
    EALREADY only).  Every batch must be accepted by this planner: a rejected
    one would still equal the oracle through the host engine"""
    d = Drive(torch_cuda, suite, T.NSESS)
    rng = np.random.default_rng(795)
    try:
        with P.tune(bpexp=BPEXP):
            for b, (snt, arrive, ndist) in enumerate(T.random_batches(701)):
                assert ndist > 0
                pk = [(s, rtp_packet(rng, seq, T.ssrc_of(s, k),
                                     plen=int(rng.integers(0, 120))))
                      for s, k, seq in snt]
                rows = d.step("tx", "srtp_encrypt", pk, what=("random", b),
                              expect=FIRST if b == 0 else ACCEPT)
                assert not any(r[0] for r in rows)
                wire = wire_of(pk, rows)
                rows = d.step("rx", "srtp_decrypt", [wire[i] for i in arrive],
                              what=("random", b), expect=TAKEN)
                assert d.x["msrxplans"] == 1, (b, d.x, d.deltas[-1])
                assert {r[0] for r in rows} <= {0, EALREADY}
                assert d.x["rxdups"] == \
                    sum(1 for r in rows if r[0] == EALREADY)
    finally:
        d.close()
