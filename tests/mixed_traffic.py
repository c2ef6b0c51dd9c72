"""Many-session batches whose sessions use different suites, built with the
oracle alone: no GPU, no product.

A bridge with AES-CM-128, AES-256-CM and GCM endpoints in one room hands the
library one session array over several suites.  No device planner takes such
a batch (their gathers decline on the second suite they meet, and run_fast
does, batch_host.c), so it is completed by the general engine, which sorts
the packets into kernel classes by (mode, rounds, header shift) and launches
the CTR-10, CTR-14 and GCM kernels over one arena with per-packet keys and
tag lengths (round_launch, srtp.c).  The scenarios here are that traffic and
its truth; tests/test_mixed_traffic_cpu.py checks that they are what they
claim, tests/test_gpu_mixed_suites.py runs the product beside them.

Sessions (SUITES_OF): "cycle", 12 sessions, suites 0..5 in turn (two per
suite; the second of each suite carries two SSRCs in the RTP traffic), and
"odd_1" / "odd_mid" / "odd_last", 300 sessions of suite 1 except one of suite
5 at index 1, 150 or 299.  The odd-numbered sessions of each suite carry
SRTP_UNENCRYPTED_SRTCP (rtcp_flags), so an SRTCP batch is mixed in its E bit
too.  session_key() gives every session a key of its own.

A scenario is a list of steps in issue order, each one batch [(session,
bytes)] through the sender's ("tx") or the receiver's ("rx") contexts, with
the oracle's rows [(errno, pos, end, bytes[:max(end, len)])], one oracle call
per packet in batch order, and the oracle's state of every (session, SSRC)
the side has seen after the step: RTP (roc, s_l, s_l_set, lix, bitmap) and
SRTCP (rtcp_index, lix, bitmap).  A receiver's batch is what the oracle's
sender made, so the truth never depends on the code under test.

The oracle keeps s_l_set to itself; the twin states it: stream_get_seq
(stream.c:87-109) sets it at the stream lookup of every RTP operation, before
any check that can fail, so it is 1 for a stream an RTP packet has named and
0 for one only SRTCP has.  No packet here is too short to parse and no
session holds more than two SSRCs (no ENOSR), so the lookup always happens.

The fixed-arena rule is that of tests/test_gpu_srtcp_multi.py: an SRTCP
protect whose trailer does not fit in the room behind the packet fails with
ENOMEM right after the stream lookup, pos past the header, nothing else
changed.  Such a packet is not sent: the receiver's batch leaves it out.

RTP: sequence numbers start 3 to 8 below 65536, so every stream with more
than 8 packets rolls its ROC over inside the first batch; the CSRC count runs
through 0..3 and one packet per session has an extension (the four header
shift classes); payload lengths run through 0..70 across the batch, one
packet per suite has 1200 bytes; the streams are interleaved packet by
packet.  The first receive batch has, per suite, on one stream (STAR), a
forged packet (the payload's first byte for the even suites, the tag's last
for the odd ones), a duplicate and an adjacent swap, at fixed arrivals past
the rollover; the second protect / unprotect pair is in order.

SRTCP: the same sessions, one SSRC each, packets of 8..200 bytes in steps of
7 (every length mod 4); per suite one protect with a byte too little room and
one with exactly enough; the first receive batch has, per suite, a forged
packet and a replayed one.
"""
import errno

import numpy as np

import re_amd.srtp as P
from tests import oracle_lib as O
from tests.test_gpu_fastpath import keys_for, rtp_packet
from tests.test_gpu_srtcp import rtcp_packet

U = P.SRTP_UNENCRYPTED_SRTCP
EAUTH = P.EAUTH
ENOMEM, EALREADY = errno.ENOMEM, errno.EALREADY
ROOM = 60                       # to_arena's cap - end
RTCP_OPS = ("srtcp_encrypt", "srtcp_decrypt")
NCYCLE, NODD = 12, 300
ODD_AT = {"odd_1": 1, "odd_mid": NODD // 2, "odd_last": NODD - 1}
SHAPES = ("cycle",) + tuple(ODD_AT)
MAXPKTS = 600
# arrivals of a STAR stream that the first receive batch disturbs
RTP_FORGE, RTP_DUP, RTP_SWAP, RTP_BIG = 10, 11, 13, 2
RTCP_SHORT, RTCP_EXACT, RTCP_FORGE, RTCP_DUP = 1, 2, 3, 4


def SUITES_OF(shape):
    """the suite of every session of a shape"""
    if shape == "cycle":
        return [k % 6 for k in range(NCYCLE)]
    out = [1] * NODD
    out[ODD_AT[shape]] = 5
    return out


def rtcp_flags(suites):
    """the odd-numbered sessions of each suite: SRTP_UNENCRYPTED_SRTCP"""
    seen, out = {}, []
    for u in suites:
        out.append(U if seen.get(u, 0) % 2 else 0)
        seen[u] = seen.get(u, 0) + 1
    return out


def session_key(suite, s):
    """keys_for(suite, .)[s]; that family has 256 members (7 * s mod 256), so
    from session 256 on the key of s - 256 rotated by a byte, which is no
    member: no two sessions of a shape share a key"""
    k = keys_for(suite, s % 256 + 1)[s % 256]
    r = s // 256
    return k[r:] + k[:r]


def ssrc_of(s, k=0):
    return 0x7000 + s + (k << 16)


def trailer(suite):
    """bytes srtcp_encrypt appends: E || index and the tag"""
    return 4 + P.tag_len(suite)


def hdr_len(p):
    """RTP header length: fixed part, CSRCs, extension"""
    n = 12 + 4 * (p[0] & 15)
    if p[0] & 0x10:
        n += 4 + 4 * int.from_bytes(p[n + 2:n + 4], "big")
    return n


def ssrc_in(op, p):
    at = 4 if op in RTCP_OPS else 8
    return int.from_bytes(p[at:at + 4], "big")


# ---- the oracle twin -------------------------------------------------------------

class Twin:
    """oracle contexts, one per session with its own suite, flags and key,
    called one packet at a time in batch order (tests/test_gpu_srtcp_multi.py
    Twin with a suite per session)"""

    def __init__(self, suites, flags):
        self.ob = O.OracleBackend()
        self.suites = list(suites)
        self.ctx = []
        self.rtp_seen = set()
        for s, (u, f) in enumerate(zip(suites, flags)):
            c, err = self.ob.alloc(u, session_key(u, s), f)
            assert err == 0
            self.ctx.append(c)

    def close(self):
        for c in self.ctx:
            self.ob.free(c)
        self.ctx = []

    def run(self, op, pkts, rooms=None, fixed=True):
        rows = []
        for i, (s, p) in enumerate(pkts):
            room = ROOM if rooms is None else rooms[i]
            c = self.ctx[s]
            if op in RTCP_OPS:
                if fixed and op == "srtcp_encrypt" and len(p) >= 8 and \
                        room < trailer(self.suites[s]):
                    # the arena cannot grow (module docstring)
                    x = ssrc_in(op, p)
                    e = self.ob.rtcp_set(c, x, *(self.ob.rtcp_state(c, x) or
                                                 (0, 0, 0)))
                    rows.append((e or ENOMEM, 8, len(p), p))
                    continue
            else:
                # the tag fits, the header parses: the lookup happens
                assert len(p) >= hdr_len(p) >= 12 and room >= 16
                self.rtp_seen.add((s, ssrc_in(op, p)))
            e, po, en, _, buf = self.ob.call(c, op, len(p) + room, 0, len(p),
                                             p, len(p))
            assert e != errno.ENOSR
            rows.append((e, po, en, buf[:max(en, len(p))]))
        return rows

    def state(self, s, ssrc):
        """((roc, s_l, s_l_set, lix, bitmap), (rtcp_index, lix, bitmap)), or
        None if the session has no such stream"""
        r = self.ob.rtcp_state(self.ctx[s], ssrc)
        if r is None:
            return None
        roc, s_l, lix, bitmap = self.ob.export(self.ctx[s], ssrc)
        return ((roc, s_l, int((s, ssrc) in self.rtp_seen), lix, bitmap), r)


class Step:
    """one batch of a scenario and the oracle's truth about it"""

    def __init__(self, what, side, op, pkts, rooms=None, sub=None):
        self.what, self.side, self.op = what, side, op
        self.pkts = list(pkts)
        self.rooms = [ROOM] * len(pkts) if rooms is None else list(rooms)
        self.sub = sub          # (lo, hi): the sessions of the call; None: all
        self.key = None         # (session, k) per packet
        self.forged = []        # indices of the forged packets
        self.rows = None
        self.states = None      # {(session, ssrc): Twin.state} after the step

    def errnos(self):
        return [r[0] for r in self.rows]


class Scenario:
    def __init__(self, name, suites, flags=None):
        self.name, self.suites = name, list(suites)
        self.flags = rtcp_flags(suites) if flags is None else list(flags)
        self.steps = []
        self.star = {}          # suite -> the stream (session, k) disturbed
        self.twin = {k: Twin(self.suites, self.flags) for k in ("tx", "rx")}
        self.seen = {"tx": set(), "rx": set()}

    def step(self, st):
        """the oracle's rows and states of one more step"""
        assert 0 < len(st.pkts) <= MAXPKTS
        tw = self.twin[st.side]
        st.rows = tw.run(st.op, st.pkts, st.rooms)
        for s, p in st.pkts:
            self.seen[st.side].add((s, ssrc_in(st.op, p)))
        st.states = {(s, x): tw.state(s, x)
                     for s, x in sorted(self.seen[st.side])}
        self.steps.append(st)
        return st

    def finish(self):
        for t in self.twin.values():
            t.close()
        return self


def wire_of(st):
    """what a sender's batch puts on the wire, with the stream of each: a
    refused packet is not sent"""
    w = [((s, r[3][:r[2]]), k) for (s, _), r, k in
         zip(st.pkts, st.rows, st.key) if r[0] == 0]
    return [x for x, _ in w], [k for _, k in w]


def flipped(p, at, bit=0x10):
    q = bytearray(p)
    q[at] ^= bit
    return bytes(q)


class Air:
    """what the network does to a batch; a stream's arrivals count from 0"""

    def __init__(self, wire, keys):
        self.item = [[w, k, False] for w, k in zip(wire, keys)]

    def at(self, key, a):
        return [i for i, it in enumerate(self.item) if it[1] == key][a]

    def forge(self, key, a, where):
        """flip a bit in the payload's first byte ("payload": behind the RTP
        header), in an SRTCP packet's body ("body": byte 8) or in the last
        byte of the packet ("tag": the tag's last)"""
        it = self.item[self.at(key, a)]
        s, p = it[0]
        i = {"payload": hdr_len(p), "body": 8, "tag": len(p) - 1}[where]
        assert i < len(p)
        it[0], it[2] = (s, flipped(p, i)), True

    def swap(self, key, a):
        """the stream's arrivals a and a + 1 change places"""
        i, j = self.at(key, a), self.at(key, a + 1)
        self.item[i], self.item[j] = self.item[j], self.item[i]

    def dup(self, key, a, later=2):
        """arrival a once more, behind the stream's arrival a + later"""
        it = self.item[self.at(key, a)]
        self.item.insert(self.at(key, a + later) + 1, [it[0], key, False])

    def out(self):
        return ([it[0] for it in self.item], [it[1] for it in self.item],
                [i for i, it in enumerate(self.item) if it[2]])


def _streams(shape, suites):
    """(streams in interleaving order, packets of each in batch 1, in batch
    2, the STAR stream of every suite)"""
    n = len(suites)
    if shape == "cycle":
        keys = [(s, 0) for s in range(n)] + [(s, 1) for s in range(6, n)]
        star = {suites[s]: (s, 0) for s in range(6)}
        return keys, {k: 30 for k in keys}, {k: 12 for k in keys}, star
    odd = ODD_AT[shape]
    busy = sorted({odd, (odd - 1) % n, (odd + 1) % n, 0, n - 1})
    keys = [(s, 0) for s in range(n)]
    star = {5: (odd, 0), 1: ([s for s in busy if s != odd][0], 0)}
    return (keys, {k: 16 if k[0] in busy else 1 for k in keys},
            {k: 6 if k[0] in busy else 1 for k in keys}, star)


def interleaved(keys, count):
    """[(stream, its arrival number)] packet by packet, not in blocks"""
    return [(k, j) for j in range(max(count.values())) for k in keys
            if j < count[k]]


_built = {}


def rtp_scenario(shape):
    """protect, unprotect with the disturbances, protect, unprotect"""
    if ("rtp", shape) in _built:
        return _built[("rtp", shape)]
    suites = SUITES_OF(shape)
    sc = Scenario(shape, suites)
    rng = np.random.default_rng(7100 + SHAPES.index(shape))
    keys, n1, n2, sc.star = _streams(shape, suites)
    stars = set(sc.star.values())
    nxt = {k: 65536 - (3 + (k[0] + 2 * k[1]) % 6) for k in keys}
    for b, count in enumerate((n1, n2)):
        pk, who = [], []
        for i, (k, j) in enumerate(interleaved(keys, count)):
            s = k[0]
            plen = i % 71
            if b == 0 and k in stars and j == RTP_BIG:
                plen = 1200
            if b == 0 and k in stars and j == RTP_FORGE:
                plen = max(plen, 1)     # a payload byte to forge
            pk.append((s, rtp_packet(
                rng, nxt[k] & 0xffff, ssrc_of(*k), cc=(j + s + k[1]) % 4,
                x=k[1] == 0 and j == min(1, count[k] - 1), plen=plen)))
            who.append(k)
            nxt[k] += 1
        st = Step(("protect", b), "tx", "srtp_encrypt", pk)
        st.key = who
        sc.step(st)
        assert not any(st.errnos())
        air = Air(*wire_of(st))
        if b == 0:
            for u, k in sorted(sc.star.items()):
                air.forge(k, RTP_FORGE, "tag" if u % 2 else "payload")
                air.swap(k, RTP_SWAP)
                air.dup(k, RTP_DUP)     # (last: it adds an arrival)
        w, wk, forged = air.out()
        st = Step(("unprotect", b), "rx", "srtp_decrypt", w)
        st.key, st.forged = wk, forged
        sc.step(st)
    _built[("rtp", shape)] = sc.finish()
    return sc


def rtcp_scenario(shape):
    """the same for SRTCP, one SSRC per session, mixed in suite and E bit"""
    if ("rtcp", shape) in _built:
        return _built[("rtcp", shape)]
    suites = SUITES_OF(shape)
    sc = Scenario(shape, suites)
    rng = np.random.default_rng(7200 + SHAPES.index(shape))
    keys, n1, n2, sc.star = _streams(shape, suites)
    keys = [k for k in keys if k[1] == 0]
    stars = {k: u for u, k in sc.star.items()}
    n1 = {k: 20 if n1[k] > 1 else 1 for k in keys}
    at = 0
    for b, count in enumerate((n1, {k: n2[k] for k in keys})):
        pk, who, rooms = [], [], []
        for k, j in interleaved(keys, count):
            pk.append((k[0], rtcp_packet(rng, ssrc_of(*k), 7 * at % 193)))
            at += 1
            who.append(k)
            room = ROOM
            if b == 0 and k in stars and j in (RTCP_SHORT, RTCP_EXACT):
                room = trailer(stars[k]) - (j == RTCP_SHORT)
            rooms.append(room)
        st = Step(("protect", b), "tx", "srtcp_encrypt", pk, rooms)
        st.key = who
        sc.step(st)
        air = Air(*wire_of(st))
        if b == 0:
            # (the refused packet is not on the wire: arrivals from
            # RTCP_EXACT on are one lower)
            for u, k in sorted(sc.star.items()):
                air.forge(k, RTCP_FORGE - 1, "tag" if u % 2 else "body")
                air.dup(k, RTCP_DUP - 1)
        w, wk, forged = air.out()
        st = Step(("unprotect", b), "rx", "srtcp_decrypt", w)
        st.key, st.forged = wk, forged
        sc.step(st)
    _built[("rtcp", shape)] = sc.finish()
    return sc


# ---- resident states handed to the host and back -----------------------------------

HAND_PAIRS = ((1, 5), (3, 4))
HAND_N = 4                      # sessions per suite
HAND_COUNT = {"A": 6, "B": 8, "C": 6}
HAND_FORGE = ((1, 5, "payload"), (6, 6, "tag"))     # session, arrival in B


def handover_scenario(pair, side):
    """four sessions of each suite of the pair, one SSRC each, every stream in
    order from 65525..65527: stage A, one batch per suite (65532 at the most),
    stage B, one batch over all eight sessions in which every stream crosses
    65535 -> 0, stage C, one batch per suite again.  Stages A and C have one
    header class (no CSRC: a device plan takes one class per batch), stage B
    all four.  side "tx": the stages as
    protect; "rx": as unprotect of what the oracle's sender made, with two
    forged packets in stage B (neither is sequence number 0)"""
    if ("hand", pair, side) in _built:
        return _built[("hand", pair, side)]
    suites = [pair[0]] * HAND_N + [pair[1]] * HAND_N
    sc = Scenario("hand%d%d" % pair, suites)
    rng = np.random.default_rng(7300 + 10 * pair[0] + (side == "rx"))
    nxt = {s: 65527 - s % 3 for s in range(2 * HAND_N)}
    for stage in "ABC":
        subs = [(0, 2 * HAND_N)] if stage == "B" else \
            [(0, HAND_N), (HAND_N, 2 * HAND_N)]
        for lo, hi in subs:
            keys = [(s, 0) for s in range(lo, hi)]
            pk, who = [], []
            for i, (k, j) in enumerate(interleaved(
                    keys, {k: HAND_COUNT[stage] for k in keys})):
                pk.append((k[0], rtp_packet(rng, nxt[k[0]] & 0xffff,
                                            ssrc_of(*k),
                                            cc=(i + j) % 4 if stage == "B"
                                            else 0, plen=20 + (7 * i) % 50)))
                who.append(k)
                nxt[k[0]] += 1
            st = Step((stage, lo), "tx", "srtp_encrypt", pk, sub=(lo, hi))
            st.key = who
            if side == "tx":
                sc.step(st)
                assert not any(st.errnos())
                continue
            st.rows = sc.twin["tx"].run(st.op, st.pkts)
            air = Air(*wire_of(st))
            if stage == "B":
                for s, a, where in HAND_FORGE:
                    air.forge((s, 0), a, where)
            w, wk, forged = air.out()
            st = Step((stage, lo), "rx", "srtp_decrypt", w, sub=(lo, hi))
            st.key, st.forged = wk, forged
            sc.step(st)
    _built[("hand", pair, side)] = sc.finish()
    return sc


# ---- one suite, a session that holds two SSRCs (the MPG_MULTI decline) ---------------

MULTI_N = 8


def multi_scenario(suite=1):
    """eight sessions of one suite: a first protect batch in which session 1
    uses two SSRCs, then a second one over the same streams, in order.  The
    many-session planner's gather declines the second at session 1 (several
    streams) and the multi-SSRC planner takes it"""
    if ("multi", suite) in _built:
        return _built[("multi", suite)]
    sc = Scenario("multi%d" % suite, [suite] * MULTI_N, [0] * MULTI_N)
    rng = np.random.default_rng(7400 + suite)
    keys = [(s, 0) for s in range(MULTI_N)] + [(1, 1)]
    nxt = {k: 65530 + k[0] % 4 for k in keys}
    for b in range(3):
        pk, who = [], []
        for i, (k, j) in enumerate(interleaved(keys, {k: 8 for k in keys})):
            pk.append((k[0], rtp_packet(rng, nxt[k] & 0xffff, ssrc_of(*k),
                                        plen=10 + (5 * i) % 60)))
            who.append(k)
            nxt[k] += 1
        st = Step(("protect", b), "tx", "srtp_encrypt", pk)
        st.key = who
        sc.step(st)
        assert not any(st.errnos())
    _built[("multi", suite)] = sc.finish()
    return sc
