"""Scenarios for chained asynchronous device batches (srtp_*_batch_dev_async,
include/re_srtp_batch.h), built with the oracle alone: no GPU, no product.

A scenario is a list of calls in issue order.  Every call names an operation,
a session set and its packets [(session, bytes)], and carries the oracle's
rows [(errno, pos, end, bytes left)], one oracle call per packet.  Protected
input of an unprotect call is what the oracle's srtp_encrypt produced, so the
truth never depends on the code under test.  After the last call the oracle's
exported state of every (session, SSRC) of every set is kept.

The chain is four calls on disjoint contexts:

  c1  protect of batch A on set "tx1", in order, accepted
  c2  the disturbed call of the route under test, on set "x2"
  c3  unprotect of c1's arena on "rx1" (Call.share: it reads the arena, pos
      and end that c1 wrote, and is queued behind c2)
  c4  protect on "tx3"

Calls in front of them (Call.role "pre") give "x2" the state the route needs,
a stream held before or several SSRCs; they are issued and completed one at a
time.  tests/test_async_traffic_cpu.py checks that every scenario is what it
claims; tests/test_gpu_async_chain.py runs them.

Payloads are 16-64 bytes.  Sequence numbers start at 65400 or later: c1 and
c4 roll the ROC over, and so does c2.  A disturbed packet keeps 12 sequence
numbers away from a rollover, and a forged one is never sequence number 0 (a
forged packet that rolls the ROC over leaves roc + 1 behind in the reference,
which the many-session fold hands to the host).
"""
import errno

import numpy as np

from tests import oracle_lib as O

EAUTH = 217             # the reference's, outside errno.h
SUITES = (1, 5)         # AES-CM-128 / HMAC-SHA1-80, AES-256-GCM
TAG = {1: 10, 5: 16}
KEYLEN = {1: 16 + 14, 5: 32 + 12}
NSESS = 130             # two buckets of the bucket planner
WG = 1024               # packets of one plan workgroup; SGPU_BP_SEGMAX too
ROOM = 60               # bytes behind a packet in the arena

#: scenario -> the counter its c2 must move in the synchronous run
ROUTES = {
    "rx": "rxplans", "ssrc": "splans", "ssrc_rx": "srxplans",
    "s_rx": "srxplans", "forged1": "misses", "forged_s": "misses",
    "reject_host": "rejects", "shortcap": "rejects", "m_rx": "mrxplans",
    "m_seg": "mplans", "m_forged": "misses", "m_ssrc": "msplans",
    "m_ssrc_rx": "msrxplans", "m_multi": "msplans",
}


def keys_for(family, suite, nsess):
    return [bytes((7 * s + i + 31 * family) & 0xff
                  for i in range(KEYLEN[suite])) for s in range(nsess)]


def rtp_packet(rng, seq, ssrc, cc=0):
    b = bytearray([0x80 | cc, 96, (seq >> 8) & 0xff, seq & 0xff])
    b += int(rng.integers(0, 1 << 32)).to_bytes(4, "big")
    b += ssrc.to_bytes(4, "big")
    b += rng.integers(0, 256, 4 * cc, dtype=np.uint8).tobytes()
    b += rng.integers(0, 256, int(rng.integers(16, 65)),
                      dtype=np.uint8).tobytes()
    return bytes(b)


def ssrc_of(s, k=0):
    return 0x7000 + s + (k << 16)


class Call:
    """one call of a scenario; as_tuple() is (op, set id, packets)"""

    def __init__(self, role, op, set_id, pkts, share=None, short_cap=()):
        self.role, self.op, self.set, self.pkts = role, op, set_id, pkts
        self.share = share              # index of the call whose arena it is
        self.short_cap = tuple(short_cap)
        self.rows = None                # the oracle's, one per packet
        self.key = None                 # (session, SSRC) per packet, or None

    def as_tuple(self):
        return (self.op, self.set, self.pkts)

    def errnos(self):
        return [r[0] for r in self.rows]


class Scenario:
    def __init__(self, name, suite):
        self.name, self.suite = name, suite
        self.sets = {}          # set id -> (key family, number of sessions)
        self.calls = []
        self.states = {}        # set id -> {(session, ssrc): oracle export}
        self.claims = {}        # what c2 is said to hold (the CPU test)
        self.reach = ROUTES[name]

    def keys(self, set_id):
        fam, n = self.sets[set_id]
        return keys_for(fam, self.suite, n)

    def call(self, role):
        return [c for c in self.calls if c.role == role][0]

    def index(self, role):
        return [i for i, c in enumerate(self.calls) if c.role == role][0]


class Oracle:
    """oracle contexts per (set, session), made on first use"""

    def __init__(self, sc):
        self.sc, self.be, self.ctx = sc, O.OracleBackend(), {}

    def get(self, set_id, s, fam=None):
        if (set_id, s) not in self.ctx:
            fam = self.sc.sets[set_id][0] if fam is None else fam
            c, err = self.be.alloc(self.sc.suite,
                                   keys_for(fam, self.sc.suite, s + 1)[s], 0)
            assert err == 0
            self.ctx[(set_id, s)] = c
        return self.ctx[(set_id, s)]

    def one(self, set_id, s, op, p, fam=None):
        e, po, en, _, buf = self.be.call(
            self.get(set_id, s, fam), op, len(p) + ROOM, 0, len(p),
            p, len(p) + 16 if op == "srtp_encrypt" else len(p))
        return (e, po, en, buf)

    def run(self, call):
        """the oracle's rows.  Its buffers grow as the reference's mbufs do;
        a device arena cannot, and the fixed arena's rule is CapTwin's of
        tests/test_gpu_mrtp_streams.py: a protect whose tag does not fit
        fails with ENOMEM right after the stream lookup, pos past the header,
        nothing else changed (the stream exists: the packet is not its
        first), so such a packet never reaches the oracle"""
        call.rows = []
        for i, (s, p) in enumerate(call.pkts):
            if i in call.short_cap:
                assert call.op == "srtp_encrypt" and i and p[0] == 0x80
                call.rows.append((errno.ENOMEM, 12, len(p), p))
            else:
                call.rows.append(self.one(call.set, s, call.op, p))

    def protect(self, sender, fam, plain):
        """plain [(session, bytes)] through the oracle's sender contexts
        `sender` (no set of the chain: the far end of "x2")"""
        out = []
        for s, p in plain:
            e, _, en, buf = self.one(sender, s, "srtp_encrypt", p, fam=fam)
            assert e == 0
            out.append((s, buf[:en]))
        return out

    def close(self):
        for c in self.ctx.values():
            self.be.free(c)


class Air:
    """what the network does to a batch: who[i] is the stream of wire[i]; a
    stream's arrivals are counted from 0"""

    def __init__(self, who, wire):
        self.who, self.wire = list(who), list(wire)
        self.slot = list(range(len(wire)))
        self.after = {}
        self.forged = []        # indices into wire

    def at(self, key, a):
        return [i for i, w in enumerate(self.who) if w == key][a]

    def swap(self, key, a, d=1):
        i, j = self.at(key, a), self.at(key, a + d)
        self.slot[i], self.slot[j] = self.slot[j], self.slot[i]

    def lose(self, key, a):
        self.slot[self.at(key, a)] = None

    def inject(self, key, a, pkt):
        self.after.setdefault(self.at(key, a), []).append((key, pkt))

    def dup(self, key, a, later):
        self.inject(key, a + later, self.wire[self.at(key, a)])

    def forge(self, key, a, where):
        """flip a bit of the payload's first byte or of the tag's last"""
        i = self.at(key, a)
        s, p = self.wire[i]
        q = bytearray(p)
        q[12 if where == "payload" else len(q) - 1] ^= 0x10
        assert q[2:4] != b"\x00\x00"
        self.wire[i] = (s, bytes(q))
        self.forged.append(i)

    def out(self):
        """(packets, stream of each, indices of the forged ones)"""
        pk, who, forged = [], [], []
        for place, i in enumerate(self.slot):
            if i is not None:
                if i in self.forged:
                    forged.append(len(pk))
                pk.append(self.wire[i])
                who.append(self.who[i])
            for key, p in self.after.get(place, []):
                pk.append(p)
                who.append(key)
        return pk, who, forged


class Flow:
    """senders: next extended sequence number per stream key (session, k)"""

    def __init__(self, rng, start):
        self.rng, self.start, self.nxt = rng, start, {}

    def packet(self, key, jump=0, cc=0):
        s, k = key
        x = self.nxt.get(key, self.start(s, k)) + jump
        assert x >= 65400
        self.nxt[key] = x + 1
        return (s, rtp_packet(self.rng, x & 0xffff, ssrc_of(s, k), cc))

    def batch(self, who):
        return [self.packet(key) for key in who]


def shuffled(rng, who):
    """the streams of `who` interleaved at random, each keeping its count"""
    return [who[i] for i in rng.permutation(len(who)).tolist()]


# ---- c2 of every route -------------------------------------------------------

def _recv(sc, orc, fl, pre_who, who, disturb=None, nsess=1):
    """"x2" receives: the calls in front (pre_who: a list of batches, in
    order) and c2, whose wire `disturb(air, wire_of_pre)` reshapes"""
    sc.sets["x2"] = (2, nsess)
    wires = []
    for pw in pre_who:
        wire = orc.protect("far2", 2, fl.batch(pw))
        wires.append(wire)
        c = Call("pre", "srtp_decrypt", "x2", wire)
        c.key = list(pw)
        sc.calls.append(c)
    air = Air(who, orc.protect("far2", 2, fl.batch(who)))
    if disturb:
        disturb(air, wires)
    pk, keys, forged = air.out()
    c2 = Call("c2", "srtp_decrypt", "x2", pk)
    c2.key = keys
    sc.claims["forged"] = forged
    return c2


def _one(k=0):
    return lambda n: [(0, k)] * n


def c2_rx(sc, orc, rng):
    fl = Flow(rng, lambda s, k: 65400)

    def disturb(air, wires):
        key = (0, 0)
        air.inject(key, 10, wires[0][-1])       # replay of the batch before
        air.swap(key, 300)
        air.lose(key, 500)
        air.dup(key, 700, 2)
        air.swap(key, 1050)
        air.dup(key, 1070, 3)
    sc.claims.update(dup=True, swap=True, span=True)
    return _recv(sc, orc, fl, [_one()(40)], _one()(1100), disturb)


def _two_streams(rng, rx):
    """SSRC 0 held from the call before; SSRC 1 appears at arrival 80"""
    fl = Flow(rng, lambda s, k: 65400 + 50 * k)
    who = [(0, 0)] * 80 + shuffled(rng, [(0, 0)] * 60 + [(0, 1)] * 60)

    def disturb(air, wires):
        air.swap((0, 1), 5)
        air.dup((0, 1), 20, 2)
    return fl, who, disturb if rx else None


def c2_ssrc(sc, orc, rng):
    fl, who, dis = _two_streams(rng, False)
    return _recv(sc, orc, fl, [_one()(30)], who, dis)


def c2_ssrc_rx(sc, orc, rng):
    fl, who, dis = _two_streams(rng, True)
    sc.claims.update(dup=True, swap=True)
    return _recv(sc, orc, fl, [_one()(30)], who, dis)


def _four(rng, n):
    return shuffled(rng, [(0, k) for k in range(4)] * (n // 4))


def c2_s_rx(sc, orc, rng):
    fl = Flow(rng, lambda s, k: 65480 + k)

    def disturb(air, wires):
        air.swap((0, 1), 5)
        air.lose((0, 1), 60)
        air.dup((0, 3), 8, 1)
        air.swap((0, 3), 62, 2)
    sc.claims.update(dup=True, swap=True)
    return _recv(sc, orc, fl, [_four(rng, 40)], _four(rng, 300), disturb)


def c2_forged1(sc, orc, rng):
    fl = Flow(rng, lambda s, k: 65440)

    def disturb(air, wires):
        air.forge((0, 0), 200, "payload")
        air.forge((0, 0), 1080, "tag")
    sc.claims.update(span=True)
    return _recv(sc, orc, fl, [], _one()(1100), disturb)


def c2_forged_s(sc, orc, rng):
    fl = Flow(rng, lambda s, k: 65480 + k)

    def disturb(air, wires):
        air.forge((0, 0), 7, "payload")
        air.forge((0, 2), 66, "tag")
    return _recv(sc, orc, fl, [_four(rng, 40)], _four(rng, 300), disturb)


def c2_reject_host(sc, orc, rng):
    """the CSRC count changes at packet 50, packet 100 jumps 40000 ahead (a
    sender of its own protects it: ETIMEDOUT comes before the tag check, and
    the stream's sender goes on undisturbed), packet 150 is cut to 7 bytes"""
    sc.sets["x2"] = (2, 1)
    fl = Flow(rng, lambda s, k: 65450)
    plain = [fl.packet((0, 0), cc=1 if i == 50 else 0) for i in range(200)]
    wire = orc.protect("far2", 2, plain)
    seq = int.from_bytes(plain[100][1][2:4], "big")
    far = rtp_packet(rng, (seq + 40000) & 0xffff, ssrc_of(0))
    wire[100] = orc.protect("far2b", 2, [(0, far)])[0]
    wire[150] = (0, wire[150][1][:7])
    c2 = Call("c2", "srtp_decrypt", "x2", wire)
    sc.claims.update(timedout=[100], short=[150], forged=[])
    return c2


def c2_shortcap(sc, orc, rng):
    sc.sets["x2"] = (2, 1)
    fl = Flow(rng, lambda s, k: 65450)
    c2 = Call("c2", "srtp_encrypt", "x2", fl.batch(_one()(200)),
              short_cap=(120,))
    sc.claims.update(enomem=[120], forged=[])
    return c2


def _many(rng, per):
    """the sessions' packets, each session in order, interleaved at random"""
    return shuffled(rng, [(s, 0) for s in range(NSESS) for _ in range(per)])


def c2_m_rx(sc, orc, rng):
    # reshaped sessions stay clear of the rollover, the others cross it
    fl = Flow(rng, lambda s, k: 65400 + s % 50 if s % 3 == 0 else 65532)

    def disturb(air, wires):
        for s in range(0, NSESS, 3):
            what = (s // 3) % 3
            if what == 0:
                air.swap((s, 0), 1)
            elif what == 1:
                air.lose((s, 0), 2)
                air.swap((s, 0), 3)
            else:
                air.dup((s, 0), 2, 1)
    sc.claims.update(dup=True, swap=True)
    return _recv(sc, orc, fl, [], _many(rng, 6), disturb, NSESS)


def c2_m_seg(sc, orc, rng):
    fl = Flow(rng, lambda s, k: 65400 if s == 7 else 65535)
    who = shuffled(rng, [(s, 0) for s in range(NSESS)
                         for _ in range(1100 if s == 7 else 2)])
    sc.claims.update(hot=7)
    return _recv(sc, orc, fl, [], who, None, NSESS)


def c2_m_forged(sc, orc, rng):
    fl = Flow(rng, lambda s, k: 65400 + s % 50 if s % 3 == 0 else 65532)

    def disturb(air, wires):
        air.forge((9, 0), 2, "payload")
        air.forge((120, 0), 4, "tag")
    return _recv(sc, orc, fl, [], _many(rng, 6), disturb, NSESS)


GAIN = tuple(range(5, NSESS, 13))       # the 10 sessions that gain an SSRC


def _m_ssrc(sc, orc, rng, rx):
    fl = Flow(rng, lambda s, k: 65430 if k else 65530)
    who = shuffled(rng, [(s, k % 2 if s in GAIN else 0)
                         for s in range(NSESS) for k in range(6)])

    def disturb(air, wires):
        for s in GAIN[:4]:
            air.swap((s, 1), 1)
        air.dup((GAIN[4], 0), 0, 1)
    assert len(GAIN) == 10
    return _recv(sc, orc, fl, [_many(rng, 2)], who, disturb if rx else None,
                 NSESS)


def c2_m_ssrc(sc, orc, rng):
    return _m_ssrc(sc, orc, rng, False)


def c2_m_ssrc_rx(sc, orc, rng):
    sc.claims.update(dup=True, swap=True)
    return _m_ssrc(sc, orc, rng, True)


def c2_m_multi(sc, orc, rng):
    fl = Flow(rng, lambda s, k: 65532 + k)
    two = lambda per: shuffled(rng, [(s, k % 2) for s in range(NSESS)
                                     for k in range(per)])
    return _recv(sc, orc, fl, [two(4)], two(6), None, NSESS)


# ---- scenarios -----------------------------------------------------------------

def _chain(sc, orc, rng, c2, n1=70, n4=50, s1=65500):
    """c1 .. c4 around c2; c1 / c3 on contexts of the same keys"""
    sc.sets.update(tx1=(1, 1), rx1=(1, 1), tx3=(3, 1))
    f1 = Flow(rng, lambda s, k: s1)
    f3 = Flow(rng, lambda s, k: 65510)
    c1 = Call("c1", "srtp_encrypt", "tx1", f1.batch(_one()(n1)))
    orc.run(c1)
    sc.calls.append(c1)
    i1 = len(sc.calls) - 1
    sc.calls.append(c2)
    c3 = Call("c3", "srtp_decrypt", "rx1",
              [(s, r[3][:r[2]]) for (s, _), r in zip(c1.pkts, c1.rows)],
              share=i1)
    sc.calls.append(c3)
    sc.calls.append(Call("c4", "srtp_encrypt", "tx3", f3.batch(_one()(n4))))
    c1.key = c3.key = [(0, 0)] * n1
    sc.calls[-1].key = [(0, 0)] * n4
    if c2.key is None:
        c2.key = [(0, 0)] * len(c2.pkts)


def _finish(sc, orc):
    for c in sc.calls:
        if c.rows is None:
            orc.run(c)
    for set_id in sc.sets:
        keys = set()
        for c in sc.calls:
            if c.set == set_id:
                keys.update(c.key)
        sc.states[set_id] = {
            (s, ssrc_of(s, k)): orc.be.export(orc.get(set_id, s),
                                              ssrc_of(s, k))
            for s, k in sorted(keys)}
    orc.close()


_built = {}


def scenario(name, suite):
    """the scenario and its oracle truth, built once per (name, suite)"""
    if (name, suite) not in _built:
        sc = Scenario(name, suite)
        orc = Oracle(sc)
        rng = np.random.default_rng(9000 + 10 * list(ROUTES).index(name) +
                                    suite)
        c2 = globals()["c2_" + name](sc, orc, rng)
        _chain(sc, orc, rng, c2)
        _finish(sc, orc)
        _built[(name, suite)] = sc
    return _built[(name, suite)]


def six(name, suite):
    """six calls on six disjoint context sets, the rejected c2 of `name`
    second (the calls in front of it first, as in scenario()): a fifth and a
    sixth pending call each complete the oldest"""
    if ("six", name, suite) not in _built:
        sc = Scenario(name, suite)
        orc = Oracle(sc)
        rng = np.random.default_rng(9500 + suite)
        c2 = globals()["c2_" + name](sc, orc, rng)
        _chain(sc, orc, rng, c2)
        for j, fam in ((5, 5), (6, 6)):
            sc.sets["tx%d" % j] = (fam, 1)
            fl = Flow(rng, lambda s, k: 65490 + fam)
            c = Call("c%d" % j, "srtp_encrypt", "tx%d" % j,
                     fl.batch(_one()(40)))
            c.key = [(0, 0)] * 40
            sc.calls.append(c)
        _finish(sc, orc)
        _built[("six", name, suite)] = sc
    return _built[("six", name, suite)]


def ring(suite=1, ncalls=140, nctx=8, n=32, every=7):
    """140 calls of 32 packets on 8 rotating disjoint contexts (set "r0" ..
    "r7", each a receiver of its own stream), every 7th one reordered: a
    scenario whose calls all have role "ring"; claims["reordered"]: which"""
    if ("ring", suite) not in _built:
        sc = Scenario("rx", suite)
        orc = Oracle(sc)
        rng = np.random.default_rng(9900 + suite)
        fl = Flow(rng, lambda s, k: 65400)
        bad = []
        for j in range(ncalls):
            cid = "r%d" % (j % nctx)
            sc.sets[cid] = (10 + j % nctx, 1)
            # a flow per context: the stream key's k names the context
            plain = [fl.packet((0, j % nctx)) for _ in range(n)]
            wire = [(0, orc.one("far" + cid, 0, "srtp_encrypt", p,
                                fam=10 + j % nctx)) for _, p in plain]
            wire = [(0, r[3][:r[2]]) for _, r in wire]
            # (a context's stream rolls over at place 8 of its fifth call:
            # places 20 and 21 are clear of it in every call)
            if j % every == every - 1:
                a = 20
                wire[a], wire[a + 1] = wire[a + 1], wire[a]
                bad.append(j)
            c = Call("ring", "srtp_decrypt", cid, wire)
            c.key = [(0, j % nctx)] * n
            sc.calls.append(c)
        sc.claims["reordered"] = bad
        _finish(sc, orc)
        _built[("ring", suite)] = sc
    return _built[("ring", suite)]
