"""The many-session SRTCP device planner (plan_buckets_rtcp.hip,
batch_dev.c dev_mplanned_rtcp): srtcp_*_batch_dev with a device session array
and more than one session, up to 8 SSRCs per session.

Every batch goes through PairDrive (tests/test_gpu_srtcp_multi.py): per packet
errno, pos, end and bytes, and per (session, SSRC) the exported SRTCP and RTP
state, against the oracle called one packet at a time.  PlanDrive adds the
counter deltas around the product's call (mrplans: accepted many-session
SRTCP plans; rejects; folds; mplans; rplans) and runs the same batch on a
second set of product contexts under srtp_gpu_tune nomrplan=1 (the host
engine behind dev_staged), compared against the same oracle rows and states.

Accepted: mrplans +1, rejects +0.  Rejected: mrplans +0, rejects +1, the
results still the oracle's.  Forged: mrplans +1, folds +1.  Not taken:
neither moves.

One case cannot keep to 600 packets per batch: a session past SGPU_BP_SEGMAX
(1024) packets in its bucket needs 1025 of them (the smallest bucket region
holds 2048 entries, so a bucket over its capacity needs more still);
test_rejected_segmax sends 1100 packets of 8 bytes and says so.
"""
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests.test_gpu_srtcp import rtcp_packet
from tests.test_gpu_srtcp_multi import (PairDrive, Prod, ROOM, U, flipped,
                                        scn_mux, scn_round_trip, scn_wrap,
                                        ssrc_of, trailer, wire_of, rtp_batch)
from tests.test_gpu_srtcp_replay import has_hmac

pytestmark = pytest.mark.gpu

ENOSR, ENOMEM, EBADMSG, EALREADY = (errno.ENOSR, errno.ENOMEM, errno.EBADMSG,
                                    errno.EALREADY)
CNT = ("mrplans", "rejects", "folds", "mplans", "rplans")
ACCEPT = {"mrplans": 1, "rejects": 0, "folds": 0}
REJECT = {"mrplans": 0, "rejects": 1}
FORGED = {"mrplans": 1, "rejects": 0, "folds": 1}
NOT_TAKEN = {"mrplans": 0, "rejects": 0}
NSESS = 40
BPEXP = 250     # 40 sessions, <= 600 packets: 16 sessions per bucket, 3 buckets


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


class PlanDrive(PairDrive):
    """PairDrive on the "dev" entry that records the planner's counters and
    runs every batch again on contexts of its own under nomrplan=1"""

    def __init__(self, torch, suite, flags, nsess, entry="dev", limit=600):
        super().__init__(torch, suite, flags, nsess, entry)
        self.ref = {k: Prod(torch, suite, self.flags[k], entry)
                    for k in ("tx", "rx")}
        self.deltas = []
        self.limit = limit
        self.off = False        # the planner switched off for the product too

    def close(self):
        super().close()
        for p in self.ref.values():
            p.close()

    def step(self, side, op, pkts, rooms=None, what=None, expect=None):
        c0 = {c: P.counter(c) for c in CNT}
        with P.tune(nomrplan=1 if self.off else None):
            if len(pkts) <= 600:
                rows = super().step(side, op, pkts, rooms, what, None)
            else:
                rows = self.big_step(side, op, pkts, what)
        dc = {c: P.counter(c) - c0[c] for c in CNT}
        self.deltas.append((what, side, op, dc))
        with P.tune(nomrplan=1):
            c1 = P.counter("mrplans")
            ref = self.ref[side].run(op, pkts, self.log[-1][3])
            assert P.counter("mrplans") == c1
        for i, (g, w) in enumerate(zip(ref, rows)):
            assert g[:3] == w[:3], (what, "nomrplan", i, g[:3], w[:3])
            assert g[3] == w[3], (what, "nomrplan", i, "bytes")
        for s, x in sorted(self.seen[side]):
            g, w = self.ref[side].state(s, x), self.twin[side].state(s, x)
            assert g == w, (what, "nomrplan state", s, hex(x), g, w)
        if expect is not None:
            assert {c: dc[c] for c in expect} == expect, (what, side, op, dc)
        return rows

    def big_step(self, side, op, pkts, what):
        """PairDrive.step for a batch past its 600 packets (module
        docstring): the same comparisons"""
        assert len(pkts) <= self.limit
        rooms = [ROOM] * len(pkts)
        rows = self.twin[side].run(op, pkts, rooms, self.fixed)
        self.seen[side].update((s, int.from_bytes(p[4:8], "big"))
                               for s, p in pkts if len(p) >= 8)
        self.errs[side].update(r[0] for r in rows)
        self.log.append((side, op, list(pkts), rooms, rows))
        got = self.prod[side].run(op, pkts, rooms)
        for i, (g, w) in enumerate(zip(got, rows)):
            assert g[:3] == w[:3], (what, i, g[:3], w[:3])
            assert g[3] == w[3], (what, i, "bytes")
        self.same_states(side, what)
        return rows

    def set_rtcp(self, side, s, ssrc, rtcp_index, lix, bitmap):
        super().set_rtcp(side, s, ssrc, rtcp_index, lix, bitmap)
        st = P.StreamState()
        st.ssrc, st.rtcp_index = ssrc, rtcp_index
        st.replay_rtcp_lix, st.replay_rtcp_bitmap = lix, bitmap
        assert self.ref[side].ctx[s].import_(st) == 0


def drive(torch, scn, suite, flags, nsess, *args, bpexp=BPEXP, **kw):
    d = PlanDrive(torch, suite, flags, nsess)
    try:
        with P.tune(bpexp=bpexp):
            return scn(d, *args, **kw)
    finally:
        d.close()


def round_trip(d, pk, rooms=None, what=None, tx=ACCEPT, rx=ACCEPT):
    rows = d.step("tx", "srtcp_encrypt", pk, rooms, what, expect=tx)
    wire = wire_of(pk, rows)
    d.step("rx", "srtcp_decrypt", wire, what=what, expect=rx)
    return rows, wire


def clean_batch(rng, who, sizes=None):
    """[(session, packet)] for [(session, stream)] in that order"""
    return [(s, rtcp_packet(rng, ssrc_of(s, k), int(
        sizes[i] if sizes is not None else 4 * rng.integers(0, 40))))
            for i, (s, k) in enumerate(who)]


# ---- accepted ---------------------------------------------------------------

LOW = 0x5A            # the stream that starts below its window's top


def scn_accept(d, seed):
    """40 sessions in 3 buckets of 16 (bpexp 250): sessions 16..31 silent
    (an empty bucket), the last bucket part-full.  Session 0: 8 SSRCs new in
    batch 1 (it reaches exactly 8 inside the batch) and 80 packets (a
    segment across waves); session 1: 1 SSRC; session 2: 2; session 3: 5
    SSRCs in batch 1 and 3 more in batch 2 (exactly 8 again, 5 of them
    known); the others 1..4.  Bodies of every length mod 4, the 8-byte
    packet (protected: the shortest valid packet), cap exact on twelve
    packets.  Session 39's stream LOW: the sender at index 99, the receiver's
    window at 105 with the bits of 100 and 101 unset -- one packet per batch,
    each below lix on an unset bit (HMAC suites).  Protect then unprotect,
    twice: streams made in batch 1 are known in batch 2."""
    rng = np.random.default_rng(seed)
    live = [s for s in range(NSESS) if not 16 <= s < 32]
    nss = {s: 1 + int(rng.integers(0, 4)) for s in live}
    nss[0], nss[1], nss[2], nss[3] = 8, 1, 2, 5
    d.set_rtcp("tx", 39, ssrc_of(39, LOW), 99, 0, 0)
    d.set_rtcp("rx", 39, ssrc_of(39, LOW), 0, 105, 0b001111)
    for b in range(2):
        if b == 1:
            nss[3] = 8
        who = [(s, k) for s in live for k in range(nss[s])]
        who += [(0, int(rng.integers(0, 8))) for _ in range(72)]
        who += [(s, int(rng.integers(0, nss[s]))) for s in
                rng.choice(live, 540 - len(who)).tolist()]
        who = [who[i] for i in rng.permutation(len(who)).tolist()]
        who.insert(int(rng.integers(0, len(who))), (39, LOW))
        sizes = rng.integers(0, 230, len(who))
        sizes[:8] = [0, 1, 2, 3, 4, 5, 6, 7]
        pk = clean_batch(rng, who, sizes)
        assert {len(p) % 4 for _, p in pk} == {0, 1, 2, 3}
        assert min(len(p) for _, p in pk) == 8 and len(pk) <= 600
        assert sum(1 for s, _ in pk if s == 0) > 64
        rooms = [ROOM] * len(pk)
        for i in rng.choice(len(pk), 12, replace=False).tolist():
            rooms[i] = trailer(d.suite)
        rows, wire = round_trip(d, pk, rooms, ("accept", b))
        assert not any(r[0] for r in rows)
        assert min(len(w) for _, w in wire) == 8 + trailer(d.suite)
    assert [len([x for s, x in d.seen["rx"] if s == k]) for k in (0, 1, 2, 3)] \
        == [8, 1, 2, 8]
    if has_hmac(d.suite):
        lix, bm = d.twin["rx"].state(39, ssrc_of(39, LOW))[0][1:]
        assert (lix, bm) == (105, 0b111111)
    d.require("tx", {0})
    d.require("rx", {0})
    # (the probe of an unused SSRC: ENOSR for the full sessions 0 and 3)
    return d.finish()


@pytest.mark.parametrize("flags", [0, U], ids=["e", "u"])
@pytest.mark.parametrize("suite", [1, 3, 5])
def test_accepted(torch_cuda, suite, flags):
    log = drive(torch_cuda, scn_accept, suite, flags, NSESS,
                300 + 2 * suite + flags)
    assert len(log) == 6


def scn_wrap_many(d, seed):
    """the 31-bit index wrap of one stream among 12 sessions: the sender's
    plan is accepted (index (rtcp_index + r + 1) & 0x7fffffff); the
    receiver's indices fall back to 0 behind 0x7fffffff, which replay.c
    takes for old (HMAC suites: EALREADY, a rejected plan; GCM keeps no
    window)"""
    rng = np.random.default_rng(seed)
    hm = has_hmac(d.suite)
    x = ssrc_of(5, 1)
    d.set_rtcp("tx", 5, x, 0x7ffffff0, 0, 0)
    d.set_rtcp("rx", 5, x, 0, 0x7ffffff0, 1)
    who = [(5, 1)] * 20 + [(s, 0) for s in range(12)] * 3
    who = [who[i] for i in rng.permutation(len(who)).tolist()]
    pk = clean_batch(rng, who)
    rows, _ = round_trip(d, pk, what="wrap", rx=REJECT if hm else ACCEPT)
    assert not any(r[0] for r in rows)
    assert d.twin["tx"].state(5, x)[0][0] == 4
    d.require("rx", {0, EALREADY} if hm else {0})
    return d.finish()


@pytest.mark.parametrize("suite", [1, 5])
def test_index_wrap_in_one_of_many_sessions(torch_cuda, suite):
    drive(torch_cuda, scn_wrap_many, suite, 0, 12, 330 + suite, bpexp=0)


# ---- rejected ---------------------------------------------------------------

def scn_reject(d, seed, case):
    """a clean round trip (accepted), then one batch with one trouble"""
    rng = np.random.default_rng(seed)
    n = d.nsess
    who = [(s, k) for s in range(n) for k in range(8 if s == 3 else 2)] * 2
    who = [who[i] for i in rng.permutation(len(who)).tolist()]
    round_trip(d, clean_batch(rng, who), what=(case, 0))
    who = [who[i] for i in rng.permutation(len(who)).tolist()]
    pk = clean_batch(rng, who)
    rooms = [ROOM] * len(pk)
    at = len(pk) // 2
    tx, code = ACCEPT, None
    if case == "one_short":
        pk[at] = (pk[at][0], pk[at][1][:8])
    if case == "ninth":
        pk[at] = (3, rtcp_packet(rng, ssrc_of(3, 0x33), 20))
        tx, code = REJECT, ("tx", ENOSR)
    elif case == "cap_short":
        rooms[at] = trailer(d.suite) - 1
        tx, code = REJECT, ("tx", ENOMEM)
    elif case == "seven_tx":
        pk[at] = (pk[at][0], pk[at][1][:7])
        tx, code = REJECT, ("tx", EBADMSG)
    rows = d.step("tx", "srtcp_encrypt", pk, rooms, (case, 1), expect=tx)
    wire = wire_of(pk, rows)
    rx = ACCEPT
    if case in ("ninth", "cap_short", "seven_tx"):
        # the refused packet arrives as it was left
        wire = [w for i, w in enumerate(wire) if i != at]
    elif case == "replay":
        wire.insert(at + 7, wire[at])
        rx, code = REJECT, ("rx", EALREADY)
    elif case == "swapped":
        i, j = next((i, j) for i in range(len(wire))
                    for j in range(i + 1, len(wire))
                    if wire[j][0] == wire[i][0] and
                    wire[j][1][4:8] == wire[i][1][4:8])
        wire[i], wire[j] = wire[j], wire[i]
        rx = REJECT
    elif case == "one_short":
        # the shortest valid packet (8 bytes protected) less its last byte
        assert len(wire[at][1]) == 8 + trailer(d.suite)
        wire[at] = (wire[at][0], wire[at][1][:-1])
        rx, code = REJECT, ("rx", EBADMSG)
    elif case == "seven_rx":
        wire[at] = (wire[at][0], wire[at][1][:7])
        rx, code = REJECT, ("rx", EBADMSG)
    rows = d.step("rx", "srtcp_decrypt", wire, what=(case, 1), expect=rx)
    if case == "swapped" and has_hmac(d.suite):
        # both are new to the window: the oracle takes them, the plan's
        # speculation (indices increase) does not hold
        assert not any(r[0] for r in rows)
    if code:
        d.require(*[code[0], {0, code[1]}])
    return d.finish()


REJECTS = ("ninth", "replay", "swapped", "one_short", "cap_short",
           "seven_tx", "seven_rx")


@pytest.mark.parametrize("case", REJECTS)
def test_rejected(torch_cuda, case):
    """AES_CM_128_HMAC_SHA1_80, 12 sessions"""
    drive(torch_cuda, scn_reject, 1, 0, 12, 340 + REJECTS.index(case), case,
          bpexp=0)


def test_rejected_segmax(torch_cuda):
    """a session with more than SGPU_BP_SEGMAX (1024) packets in its bucket
    at a small bpexp: 1100 packets of 8 bytes, 1040 of them session 0's (the
    module docstring: no batch of 600 can get there)"""
    d = PlanDrive(torch_cuda, 1, 0, 6, limit=1100)
    rng = np.random.default_rng(361)
    try:
        with P.tune(bpexp=400):
            who = [(0, 0)] * 1040 + [(s, 0) for s in range(1, 6)] * 12
            who = [who[i] for i in rng.permutation(len(who)).tolist()]
            pk = clean_batch(rng, who, [0] * len(who))
            rows = d.step("tx", "srtcp_encrypt", pk, what="segmax",
                          expect=REJECT)
            assert not any(r[0] for r in rows)
            d.step("rx", "srtcp_decrypt", wire_of(pk, rows), what="segmax",
                   expect=REJECT)
            # and one packet fewer than the limit allows is planned
            who = [(0, 0)] * 500 + [(s, 0) for s in range(1, 6)] * 12
            who = [who[i] for i in rng.permutation(len(who)).tolist()]
            pk = clean_batch(rng, who, [0] * len(who))
            round_trip(d, pk, what="below segmax")
    finally:
        d.close()


# ---- forged -----------------------------------------------------------------

def scn_forged(d, seed):
    """one flipped tag bit in a batch over 12 sessions: the plan is accepted,
    the crypto launch counts the miss, everything is undone and the host
    engine folds: EAUTH on that packet alone.  Then the same with a forged
    packet of an SSRC nothing else carries (stream_get precedes the tag
    check: the SSRC takes a slot)"""
    rng = np.random.default_rng(seed)
    hm = has_hmac(d.suite)
    who = [(s, k) for s in range(d.nsess) for k in range(2)] * 3
    for b in range(2):
        who = [who[i] for i in rng.permutation(len(who)).tolist()]
        pk = clean_batch(rng, who)
        if b == 1:
            pk.insert(40, (7, rtcp_packet(rng, ssrc_of(7, 0x77), 36)))
        rows = d.step("tx", "srtcp_encrypt", pk, what=("forged", b),
                      expect=ACCEPT)
        wire = wire_of(pk, rows)
        s, w = wire[40]
        wire[40] = (s, flipped(w, len(w) - 1 if hm else len(w) - 5, 0x40))
        rows = d.step("rx", "srtcp_decrypt", wire, what=("forged", b),
                      expect=FORGED)
        assert [i for i, r in enumerate(rows) if r[0]] == [40]
        assert rows[40][0] == P.EAUTH
    assert d.twin["rx"].state(7, ssrc_of(7, 0x77)) is not None
    return d.finish()


@pytest.mark.parametrize("suite", [1, 5])
def test_forged(torch_cuda, suite):
    drive(torch_cuda, scn_forged, suite, 0, 12, 370 + suite, bpexp=0)


# ---- not taken ----------------------------------------------------------------

def scn_plain(d, seed, expect, off=False):
    rng = np.random.default_rng(seed)
    d.off = off
    who = [(s, k) for s in range(d.nsess) for k in range(2)] * 3
    who = [who[i] for i in rng.permutation(len(who)).tolist()]
    round_trip(d, clean_batch(rng, who), what="plain", tx=expect, rx=expect)
    return d.finish()


def test_not_taken_differing_flags(torch_cuda):
    flags = {k: [U if s == 4 else 0 for s in range(12)] for k in ("tx", "rx")}
    drive(torch_cuda, scn_plain, 1, flags, 12, 380, NOT_TAKEN, bpexp=0)


def test_not_taken_one_context_twice(torch_cuda):
    """sessv names one context twice (sessions 1 and 2), the oracle's twins
    likewise"""
    d = PlanDrive(torch_cuda, 1, 0, 12)
    keep = []
    try:
        for side in ("tx", "rx"):
            for grp in (d.prod[side], d.ref[side], d.twin[side]):
                keep.append((grp, grp.ctx[2]))
                grp.ctx[2] = grp.ctx[1]
        rng = np.random.default_rng(381)
        who = [(s, k) for s in range(12) for k in range(2)] * 3
        who = [who[i] for i in rng.permutation(len(who)).tolist()]
        # sessions 1 and 2 are one context now: one SSRC numbering
        pk = [(s, rtcp_packet(rng, ssrc_of(1 if s == 2 else s, k), 24))
              for s, k in who]
        round_trip(d, pk, what="alias", tx=NOT_TAKEN, rx=NOT_TAKEN)
    finally:
        for grp, c in keep:
            grp.ctx[2] = c
        d.close()


def test_not_taken_nomrplan(torch_cuda):
    drive(torch_cuda, scn_plain, 1, 0, 12, 382, NOT_TAKEN, True, bpexp=0)
    drive(torch_cuda, scn_plain, 1, 0, 12, 382, ACCEPT, bpexp=0)


# ---- beside the other planners ---------------------------------------------------

@pytest.mark.parametrize("suite", [1, 5])
def test_rtcp_mux(torch_cuda, suite):
    """scn_mux on 24 sessions: every SRTCP batch is planned (mrplans 1,
    rejects 0), the first RTP batch by the many-session RTP planner (scn_mux
    asserts mplans 1 there; behind the SRTCP batches a third of the sessions
    has a second SSRC, which that planner does not take -- as before)"""
    d = PlanDrive(torch_cuda, suite, 0, 24)
    try:
        scn_mux(d, 390 + suite)
        rtcp = [dc for what, _, op, dc in d.deltas
                if op.startswith("srtcp") and what and what[0] == "mux"]
        assert len(rtcp) == 4
        assert all(dc["mrplans"] == 1 and dc["rejects"] == 0 for dc in rtcp), \
            d.deltas
        rtp = [dc for _, _, op, dc in d.deltas if op.startswith("srtp_")]
        assert all(dc["mrplans"] == 0 for dc in rtp)
    finally:
        d.close()


@pytest.mark.parametrize("suite", [1, 5])
def test_rtp_planner_behind_srtcp(torch_cuda, suite):
    """24 sessions, RTP and SRTCP on one SSRC each: SRTCP batches mrplans 1,
    and the RTP batches behind them still mplans 1, rejects 0 (the host's
    tables, which the SRTCP plan advanced, go up again as they do behind the
    host engine)"""
    d = PlanDrive(torch_cuda, suite, 0, 24)
    try:
        rng = np.random.default_rng(395 + suite)
        nxt = [65400 + 7 * s for s in range(24)]
        ssrc = lambda s: 0x7000 + s
        rtp = {"mplans": 1, "rejects": 0, "mrplans": 0}
        for b in range(4):
            if b % 2 == 0:
                pk = rtp_batch(rng, nxt, 400, ssrc)
                rows = d.step("tx", "srtp_encrypt", pk, what=("rtp", b),
                              expect=rtp)
                rows = d.step("rx", "srtp_decrypt", wire_of(pk, rows),
                              what=("rtp", b), expect=rtp)
            else:
                pk = [(s, rtcp_packet(rng, ssrc(s), int(rng.integers(0, 200))))
                      for s in rng.integers(0, 24, 200).tolist()]
                rows, _ = round_trip(d, pk, what=("rtcp", b))
            assert not any(r[0] for r in rows)
        d.finish()
    finally:
        d.close()


def test_one_session_path_unchanged(torch_cuda):
    """one session without a session array: the one-stream SRTCP planner as
    before (rplans +1), the many-session planner not asked"""
    one = {"rplans": 1, "mrplans": 0, "rejects": 0}
    d = PlanDrive(torch_cuda, 1, 0, 1, entry="dev1")
    try:
        rng = np.random.default_rng(399)
        pk = [(0, rtcp_packet(rng, 0xABCD, 4 * int(rng.integers(0, 50))))
              for _ in range(60)]
        round_trip(d, pk, what="one session", tx=one, rx=one)
    finally:
        d.close()


def test_one_session_with_session_array(torch_cuda):
    """scn_wrap (one context, three SSRCs, the index wrap) through the entry
    with a session array: nsess == 1 is not the planner's (mrplans +0), the
    results the oracle's as before"""
    d = PlanDrive(torch_cuda, 1, 0, 1)
    try:
        scn_wrap(d, 398)
        assert d.deltas and all(dc["mrplans"] == 0 for *_, dc in d.deltas)
    finally:
        d.close()


@pytest.mark.parametrize("suite", [1, 5])
def test_round_trip_scenario(torch_cuda, suite):
    """scn_round_trip (40 sessions, 1..8 SSRCs, packets either side of
    SGPU_CACHED_MAX, caps one byte short: rejected and accepted batches
    mixed) with the nomrplan comparison"""
    d = PlanDrive(torch_cuda, suite, 0, 40)
    try:
        scn_round_trip(d, 400 + suite)
        assert sum(dc["mrplans"] + dc["rejects"] for _, _, op, dc in d.deltas
                   if op.startswith("srtcp")) == len(d.deltas)
    finally:
        d.close()
