"""The receive planner for reordered one-session batches that carry several
SSRCs (re_amd/csrc/hip/plan_streams_rx.hip, batch_dev.c dev_srxplanned):
srtp_decrypt_batch_dev on one session with up to 8 SSRCs, some stream arriving
with a swap, a loss, a duplicate or a replay of the batch before.

Every call is compared with the oracle called one packet at a time (errno,
pos, end, bytes, every SSRC's exported state) and with the same call on
contexts of its own under srtp_gpu_tune nosrxplan=1 (the host engine behind
the rejected per-stream plan), and asserts its counter deltas: "srxplans"
(accepted plans of this planner), "splans" (the in-order per-stream planner,
which does not move for them), "rxlate" / "rxdups" (its late and EALREADY
packets), "rejects" (the rejected in-order plan: 1) and "folds".

The kernels' workgroup is W = 256 packets wide (SRX_BLOCK), one packet per
thread, over the batch in arrival order (count, place) and again over the
stream-major order (scan, settle).  The seam shapes are cut to it: stream 0
of the second batch has exactly 3 W arrivals, so the boundary to stream 1 lies
on a workgroup edge and the stream is longer than two workgroups; stream 1 has
300, so the next boundary lies inside a workgroup; the last stream has one
packet and is new in the second batch; the batches span 5 and 7 workgroups.
No batch passes 4096 packets of 200 bytes.
"""
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import oracle_lib as O
from tests import srx_traffic as T
from tests.test_gpu_fastpath import keys_for, rtp_packet, run, run_dev, to_arena
from tests.test_gpu_rxplan import run_async

pytestmark = pytest.mark.gpu

W = 256                 # SRX_BLOCK
LOOKBACK = 128          # RX_LOOKBACK
ENOSR, EALREADY, ETIMEDOUT = errno.ENOSR, errno.EALREADY, errno.ETIMEDOUT
COUNTERS = ("srxplans", "splans", "rxlate", "rxdups", "rejects", "folds")
IN_ORDER = {"srxplans": 0, "splans": 1, "rxlate": 0, "rxdups": 0,
            "rejects": 0, "folds": 0}
TAKEN = {"srxplans": 1, "splans": 0, "rejects": 1, "folds": 0}
LEFT = {"srxplans": 0, "splans": 0, "rxlate": 0, "rxdups": 0, "rejects": 1,
        "folds": 0}


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


def ssrc_of(k):
    return 0x6b000000 | k


def ssrc_in(pkt):
    return int.from_bytes(pkt[8:12], "big")


class Link:
    """one sender and three receivers of one session: the planner's, the
    same calls under nosrxplan=1, the oracle's"""

    def __init__(self, torch, suite, start=65000):
        key = keys_for(suite, 1)[0]
        self.torch, self.suite = torch, suite
        self.tx = P.Srtp(suite, key)
        self.rxa, self.rxb = P.Srtp(suite, key), P.Srtp(suite, key)
        self.be = O.OracleBackend()
        self.ctx, err = self.be.alloc(suite, key, 0)
        assert err == 0
        self.start = start
        self.nxt = {}           # stream -> next extended seq
        self.ext = {}           # wire bytes -> its extended seq
        self.top = {}           # SSRC -> highest extended seq accepted
        self.ssrcs = set()

    def close(self):
        for s in (self.tx, self.rxa, self.rxb):
            s.close()
        self.be.free(self.ctx)

    def send(self, rng, who):
        """who[i]: the stream of the i-th packet sent; protected in order.
        Returns the wire packets."""
        pk, ext = [], []
        for k in who:
            x = self.nxt.get(k, self.start(k) if callable(self.start)
                             else self.start)
            self.nxt[k] = x + 1
            ext.append(x)
            pk.append((0, rtp_packet(rng, x & 0xffff, ssrc_of(k), plen=40)))
        arena, pos, end, cap, _ = to_arena(pk)
        enc = run(self.torch, "srtp_encrypt", [self.tx], arena, pos, end, cap,
                  None, False)
        assert not enc[3].any()
        wire = [enc[0][pos[i]:enc[2][i]].tobytes() for i in range(len(pk))]
        for w, x in zip(wire, ext):
            self.ext[w] = x
        return wire

    def call(self, entry, rx, pkts):
        arena, pos, end, cap, _ = to_arena([(0, p) for p in pkts])
        fn = run_dev if entry == "dev" else run_async
        c0 = {c: P.counter(c) for c in COUNTERS}
        # (a fresh session's first batch goes to the per-stream planner)
        with P.tune(freshmulti=1):
            r = fn(self.torch, "srtp_decrypt", [rx], arena, pos, end, cap,
                   None)
        return r, pos, {c: P.counter(c) - c0[c] for c in COUNTERS}

    def state(self, rx, ssrc):
        e, st = rx.export(ssrc)
        if e:
            return (0, 0, 0, 0)
        return (st.roc, st.s_l, st.replay_rtp_lix, st.replay_rtp_bitmap)

    def rx(self, pkts, expect, what, entry="dev", forged=()):
        """unprotect one batch everywhere; returns the errnos"""
        assert 0 < len(pkts) <= 4096 and max(len(p) for p in pkts) <= 200
        da, pos, delta = self.call(entry, self.rxa, pkts)
        print(what, delta)
        with P.tune(nosrxplan=1):
            db, _, dref = self.call(entry, self.rxb, pkts)
        assert dref["srxplans"] == 0, (what, dref)
        for x, y, name in zip(da, db, ("arena", "pos", "end", "err")):
            assert (x == y).all(), (what, name, np.flatnonzero(x != y)[:8])
        late = dups = 0
        for i, p in enumerate(pkts):
            e, po, en, _, buf = self.be.call(self.ctx, "srtp_decrypt",
                                             len(p) + 64, 0, len(p), p, len(p))
            got = (int(da[3][i]), int(da[1][i] - pos[i]),
                   int(da[2][i] - pos[i]))
            assert got == (e, po, en), (what, i, got, (e, po, en))
            assert da[0][pos[i]:pos[i] + len(buf)].tobytes() == buf, (what, i)
            s = ssrc_in(p)
            self.ssrcs.add(s)
            if e == 0:
                x = self.ext[p]
                late += x < self.top.get(s, -1)
                self.top[s] = max(self.top.get(s, -1), x)
            dups += e == EALREADY
            if i in forged:
                assert e == P.EAUTH, (what, i, e)
            else:
                assert e != P.EAUTH, (what, i)
        for s in sorted(self.ssrcs):
            want = self.be.export(self.ctx, s)
            assert self.state(self.rxa, s) == want, (what, hex(s))
            assert self.state(self.rxb, s) == want, (what, hex(s))
        want = dict(expect)
        if want["srxplans"]:
            want.update(rxlate=late, rxdups=dups)
        assert delta == want, (what, delta, want)
        # every counter that existed before moves as without the planner
        if not want["srxplans"]:
            assert delta == dref, (what, delta, dref)
        else:
            assert delta["rejects"] == dref["rejects"], (what, delta, dref)
        return da[3]


class Air:
    """what the network does to one batch's wire; a stream's arrivals are
    counted from 0, every call in terms of the arrivals as they are now"""

    def __init__(self, wire):
        self.arr = list(wire)

    def at(self, k, a):
        return [i for i, p in enumerate(self.arr)
                if ssrc_in(p) == ssrc_of(k)][a]

    def count(self, k):
        return sum(1 for p in self.arr if ssrc_in(p) == ssrc_of(k))

    def swap(self, k, a, d=1):
        i, j = self.at(k, a), self.at(k, a + d)
        self.arr[i], self.arr[j] = self.arr[j], self.arr[i]

    def lose(self, k, a):
        del self.arr[self.at(k, a)]

    def put(self, k, a, pkt):
        """pkt becomes the stream's arrival a"""
        self.arr.insert(self.at(k, a), pkt)

    def stale_dup(self, k, a, behind):
        """a copy of arrival a (the top of its stream's window when it
        arrives) `behind` arrivals of its stream after it; the arrivals
        between are copies of the ten before it, so the top stays where it is
        and the copy lies inside the window, not 64 below it"""
        for j in range(behind - 1):
            self.put(k, a + 1 + j, self.arr[self.at(k, a - 10 + j % 10)])
        self.put(k, a + behind, self.arr[self.at(k, a)])

    def dup(self, k, a, behind):
        """a copy of arrival a, `behind` arrivals of its stream after it"""
        self.put(k, a + behind, self.arr[self.at(k, a)])


def mixed(rng, counts):
    """the streams of a batch interleaved, each stream's first packet in slot
    order at the front (new SSRCs take their slots by first appearance)"""
    rest = [k for k, c in enumerate(counts) for _ in range(c - 1)]
    rest = [rest[i] for i in rng.permutation(len(rest)).tolist()]
    return [k for k, c in enumerate(counts) if c] + rest


def of_stream(wire, k):
    return [p for p in wire if ssrc_in(p) == ssrc_of(k)]


# ---- seams --------------------------------------------------------------------

SEAMS = {3: [3 * W, 300, 1], 8: [3 * W, 300, 40, 41, 131, 255, 7, 1]}


@pytest.mark.parametrize("suite", [1, 5])
@pytest.mark.parametrize("nst", [3, 8])
def test_seams(torch_cuda, suite, nst):
    """A fresh session (no stream yet) takes a disturbed first batch of
    nst - 1 streams, then a second batch that opens the last stream with one
    packet.  Streams start at 65000, so stream 0 rolls over at its 136th
    packet of the second batch.  Second batch, stream 0 (slot 0: its arrival
    a lies at place a of the stream-major order): swaps 5 before and 4 behind
    the rollover, a duplicate 9 behind its original next to it, a swap of
    arrivals W - 1 and W (two workgroups), a duplicate exactly RX_LOOKBACK
    arrivals behind its original with the window's top still at the original
    (found by the look-back alone); stream 1 (no rollover): a replay of the
    batch before's last packet as its first arrival (the look-back has nothing
    of its own segment before it), a loss, a replay of the batch before some
    400 below the top; every other stream a swap where it has the packets."""
    L = Link(torch_cuda, suite)
    rng = np.random.default_rng(800 + 10 * suite + nst)
    want = SEAMS[nst]
    try:
        first = [400, 200] + [20] * (nst - 3)
        w1 = L.send(rng, mixed(rng, first))
        air = Air(w1)
        air.swap(0, 0)          # a new stream's first two arrivals
        air.swap(1, 50, 8)
        air.dup(0, 100, 3)
        air.lose(1, 120)
        assert len(air.arr) >= 2 * W
        L.rx(air.arr, TAKEN, ("seams", nst, 1))
        # the second batch: as many packets sent as make the arrivals `want`
        sent = list(want)
        sent[0] -= 1 + LOOKBACK
        sent[1] -= 1
        w2 = L.send(rng, mixed(rng, sent))
        air = Air(w2)
        air.swap(0, 128, 5)
        air.swap(0, 138, 4)
        air.dup(0, 137, 9)
        air.swap(0, W - 1)
        air.stale_dup(0, 300, LOOKBACK)
        air.lose(1, 50)
        air.put(1, 250, of_stream(w1, 1)[50])
        air.put(1, 0, of_stream(w1, 1)[-1])
        for k in range(2, nst - 1):
            if want[k] > 6:
                air.swap(k, 2, 3)
        assert [air.count(k) for k in range(nst)] == want
        assert -(-len(air.arr) // W) >= 5         # workgroups
        errs = L.rx(air.arr, TAKEN, ("seams", nst, 2))
        assert int((errs == EALREADY).sum()) == 3 + LOOKBACK
        assert L.state(L.rxa, ssrc_of(0))[0] == 1       # rolled over
        # then a batch in order: the in-order planner takes it again
        w3 = L.send(rng, mixed(rng, [60] * nst))
        L.rx(w3, IN_ORDER, ("seams", nst, 3))
    finally:
        L.close()


# ---- random traffic -------------------------------------------------------------

@pytest.mark.parametrize("suite,seed", list(zip([1, 5], T.SEEDS)))
def test_random_traffic(torch_cuda, suite, seed):
    """tests/srx_traffic.py: 3-8 streams over a rollover, swaps, loss and
    duplicates at a few percent.  tests/test_streams_rx_rule.py shows on the
    CPU that every batch is disturbed and one the rule settles: every call
    must be the planner's."""
    L = Link(torch_cuda, suite, start=lambda k: 0)
    rng = np.random.default_rng(seed)
    try:
        for b, (sent, arrive, ndist) in enumerate(T.random_batches(seed)):
            for k, seq in sent:
                L.nxt.setdefault(k, seq)        # the generator's starts
            wire = L.send(rng, [k for k, _ in sent])
            assert all(L.ext[w] & 0xffff == seq for w, (_, seq) in
                       zip(wire, sent))
            errs = L.rx([wire[i] for i in arrive], TAKEN, ("random", seed, b))
            assert {int(e) for e in errs} <= {0, EALREADY}
    finally:
        L.close()


# ---- left to the host -------------------------------------------------------------

def known(L, rng, counts, what):
    """a first batch in order on a fresh session"""
    wire = L.send(rng, mixed(rng, counts))
    L.rx(wire, IN_ORDER, (what, 0))
    return wire


def test_dup_past_the_lookback(torch_cuda):
    """a duplicate RX_LOOKBACK + 1 arrivals of its stream behind its original,
    the window's top still at the original: the look-back does not reach it,
    the rule cannot tell, the host engine settles it"""
    L = Link(torch_cuda, 1, start=1000)
    rng = np.random.default_rng(830)
    try:
        known(L, rng, [40, 40, 40], "dup129")
        air = Air(L.send(rng, mixed(rng, [400, 150, 50])))
        air.swap(1, 10)
        air.stale_dup(0, 100, LOOKBACK + 1)
        errs = L.rx(air.arr, LEFT, ("dup129", 1))
        assert int((errs == EALREADY).sum()) == LOOKBACK + 1
    finally:
        L.close()


def test_ninth_ssrc(torch_cuda):
    """eight known streams, a swap, and a packet of a ninth SSRC: ENOSR"""
    L = Link(torch_cuda, 1, start=1000)
    rng = np.random.default_rng(831)
    try:
        known(L, rng, [30] * 8, "ninth")
        air = Air(L.send(rng, mixed(rng, [70] * 8)))
        air.swap(3, 10)
        p = bytearray(air.arr[200])
        p[8:12] = ssrc_of(8).to_bytes(4, "big")
        L.ext[bytes(p)] = 0
        air.arr.insert(300, bytes(p))
        errs = L.rx(air.arr, LEFT, ("ninth", 1))
        assert {int(e) for e in errs} == {0, ENOSR}
        assert int((errs == ENOSR).sum()) == 1
    finally:
        L.close()


def test_etimedout(torch_cuda):
    """the packet before a rollover arrives behind the one after it: the
    reference's ETIMEDOUT"""
    L = Link(torch_cuda, 1, start=65500)
    rng = np.random.default_rng(832)
    try:
        known(L, rng, [20, 20, 20], "etimedout")
        air = Air(L.send(rng, mixed(rng, [300, 200, 100])))
        air.swap(0, 15)         # seqs 65535 and 0
        air.swap(1, 100)
        errs = L.rx(air.arr, LEFT, ("etimedout", 1))
        assert {int(e) for e in errs} == {0, ETIMEDOUT}
    finally:
        L.close()


@pytest.mark.parametrize("suite", [1, 5])
def test_forged_among_disturbed(torch_cuda, suite):
    """one forged packet among swaps and a duplicate: the planner's crypto
    launches meet the miss, the batch is undone and the host engine folds
    it, once; the EAUTH is on that packet alone"""
    L = Link(torch_cuda, suite, start=1000)
    rng = np.random.default_rng(833)
    try:
        known(L, rng, [40, 40, 40], "forged")
        air = Air(L.send(rng, mixed(rng, [300, 200, 100])))
        air.swap(0, 100, 3)
        air.swap(2, 20)
        air.dup(1, 50, 4)
        i = air.at(1, 120)
        p = bytearray(air.arr[i])
        p[30] ^= 0x10
        L.ext[bytes(p)] = L.ext[air.arr[i]]
        air.arr[i] = bytes(p)
        errs = L.rx(air.arr, dict(LEFT, folds=1), ("forged", 1), forged={i})
        assert int((errs == P.EAUTH).sum()) == 1
    finally:
        L.close()


def test_nosrxplan_and_in_order_keep_their_paths(torch_cuda):
    """the knob exists and is off by default; the library knows the counter"""
    assert P.lib().srtp_gpu_tune(b"nosrxplan", 1) == 0
    assert P.lib().srtp_gpu_tune(b"nosrxplan", 0) == 0
    L = Link(torch_cuda, 1, start=1000)
    rng = np.random.default_rng(834)
    try:
        known(L, rng, [40, 40], "paths")
        L.rx(L.send(rng, mixed(rng, [300, 300])), IN_ORDER, ("paths", 1))
    finally:
        L.close()


# ---- asynchronous -------------------------------------------------------------------

def test_async(torch_cuda):
    """srtp_decrypt_batch_dev_async + srtp_batch_wait on a session of four
    SSRCs: a first batch in order, then a disturbed one -- the per-stream
    ticket is rejected and completed by the planner"""
    L = Link(torch_cuda, 1, start=65400)
    rng = np.random.default_rng(835)
    try:
        w0 = L.send(rng, mixed(rng, [50, 50, 50, 50]))
        L.rx(w0, IN_ORDER, ("async", 0), entry="async")
        air = Air(L.send(rng, mixed(rng, [W + 40, 200, 100, 3])))
        air.swap(0, 90, 2)
        air.swap(0, W - 1)
        air.dup(1, 20, 6)
        air.lose(2, 10)
        air.put(3, 1, of_stream(w0, 3)[-2])
        errs = L.rx(air.arr, TAKEN, ("async", 1), entry="async")
        assert int((errs == EALREADY).sum()) == 2
    finally:
        L.close()
