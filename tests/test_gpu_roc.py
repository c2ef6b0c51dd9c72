"""The RTP rollover counter at 2^16, 2^31 and 2^32 on every device path.

Every device planner carries the ROC through prefix sums, packs it into the
64-bit descriptor and feeds it to the AES-CM / GCM IVs and the HMAC trailer;
here the streams start just below ROC 2^16, 2^31 and 2^32 (srtp_stream_import
on the product, oracle_stream_set on its oracle twin) and roll over inside
the batch.  The reference is peculiar from 2^31 on (srtp_get_index keeps the
ROC in an int, src/srtp/misc.c:22-41: the index the replay window stores is
sign-extended; behind 2^32 the ROC is 0 again and every later packet is
EALREADY), tests/test_roc_cpu.py pins the oracle to it there.

Every case is protect, unprotect, then a second batch of each on the carried
state -- the second unprotect replays packets of the first beside new ones.
Compared with the oracle called one packet at a time: errno, pos and end
relative to the packet, every byte the oracle leaves (unprotect: the tag
region included) and the exported state of every stream after every batch.

Which path ran is asserted from the srtp_gpu_counter deltas.  At 2^16 nothing
in the reference is special: every batch takes its device path (the planner's
counter +1; `rejects` +0 for an ordered batch, and +1 for a disturbed one --
the receive planners run only behind the in-order planner's rejection, which
is that one count).  At 2^31 and 2^32 the table DECLINES names the batches
a planner hands to the host engine (DESIGN.md 5 says why); they are compared
all the same, which tests the host engine's own index (srtp.c get_index).

Shapes: one-stream batches are just over two workgroups of the planner under
test (the widths are read from the planners' sources), the rollover once
inside the first wave and once on the first packet of the second workgroup;
many-session batches deal 16 packets to each session, the sessions at the
boundaries adjacent in session order among sessions at ROC 0, so that the
segmented scans carry indices near 2^47 and small ones side by side; the
first of them starts where the second workgroup's positions start.
"""
import ctypes
import errno
import os
import re

import numpy as np
import pytest

import re_amd.srtp as P
from tests import oracle_lib as O
from tests import roc_util as R
from tests.test_gpu_fastpath import keys_for, rtp_packet, run, run_dev, \
    states, to_arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "re_amd", "csrc")
SOURCES = ("srtpgpu.h", "hip/k_ctr_fast.h", "hip/k_ctr_fused.h",
           "hip/plan_rx.hip", "hip/plan_streams_tab.h",
           "hip/plan_streams_rx.hip", "hip/plan_buckets.hip")


_sources = []


def constant(name):
    """a planner's own #define, names and products resolved"""
    if not _sources:
        for f in SOURCES:
            with open(os.path.join(CSRC, f)) as fh:
                _sources.append(fh.read())
    for t in _sources:
        m = re.search(r"^#define\s+%s\s+([^/\n]+)" % name, t, re.M)
        if m:
            expr = re.sub(r"[A-Za-z_]\w*",
                          lambda x: str(constant(x.group(0))),
                          re.sub(r"\b(\d+)[uU]\b", r"\1", m.group(1)))
            return int(eval(expr, {"__builtins__": {}}))
    raise KeyError(name)


FZ_BLOCK = constant("FZ_BLOCK")         # the fused launch: packets / workgroup
LP_WG = constant("LP_WG")               # the lean planner's
RX_BLOCK = constant("RX_BLOCK")
SP_BLOCK = constant("SP_BLOCK")
SRX_BLOCK = constant("SRX_BLOCK")
BPB = constant("BPB")                   # the bucket planners' workgroup

BOUNDS = ("2p16", "2p31", "2p32")
PER = 16                # packets per session in the many-session batches
GCM = (4, 5)
PLANNERS = ("fused", "lplans", "dplans", "splans", "srxplans", "mplans",
            "mrxplans", "msplans", "msrxplans", "rxplans")
COUNTERS = PLANNERS + ("rejects", "folds", "devfolds")

# The batches a planner declines before it modifies anything: (highest
# boundary in the batch, step, arrival order of the first unprotect).  Not
# listed: planned on the device.  Protect never declines (srtp.c:213: the
# sender's index is 65536 * roc + seq in 64 bits, the uint32_t ROC wraps to
# 0 behind 2^32 - 1 as the reference's does).  The in-order unprotect
# planners compute the reference's sign-extended index themselves
# (plan_rule.h plan_index) and cross 2^31 on the device; behind 2^32 the
# index falls from near 2^64 to 0, which no in-order plan accepts.  The
# receive rule (plan_rx_rule.h) settles nothing at ROC 2^31 or above.
DECLINES = {
    ("2p31", "unprotect1", "disturbed"),
    ("2p31", "unprotect2", "ordered"),
    ("2p31", "unprotect2", "disturbed"),
    ("2p32", "unprotect1", "ordered"),
    ("2p32", "unprotect1", "disturbed"),
    ("2p32", "unprotect2", "ordered"),
    ("2p32", "unprotect2", "disturbed"),
}


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


def bounds_in(b):
    """the boundaries of a many-stream batch whose highest is b"""
    return BOUNDS[:BOUNDS.index(b) + 1]


class Stream:
    """a stream whose last packet was s_l at roc"""

    def __init__(self, sess, ssrc, roc, s_l):
        self.sess, self.ssrc, self.roc, self.s_l = sess, ssrc, roc, s_l
        self.sent = 0           # packets made so far: k = 0, 1, ...
        self.empty = False      # the receiver's window: nothing seen yet

    def seq(self, k):
        return (self.s_l + 1 + k) & 0xffff

    def tx_state(self):
        return (self.roc, self.s_l, 1, 0, 0)

    def rx_state(self):
        if self.empty:
            return (self.roc, self.s_l, 1, 0, 0)
        return (self.roc, self.s_l, 1, R.ref_lix(self.roc, self.s_l), 1)


def rolls_at(b, pos, sess, ssrc):
    """a stream one packet-run below boundary b (None: ROC 0, no rollover
    in reach) whose packet k = pos has sequence number 0"""
    if b is None:
        return Stream(sess, ssrc, 0, 999 + 7 * (ssrc & 0xff))
    return Stream(sess, ssrc, R.BOUNDS[b], (65535 - pos) & 0xffff)


def imported(ctx, ssrc, st):
    s = P.StreamState()
    s.ssrc = ssrc
    s.roc, s.s_l, s.s_l_set, s.replay_rtp_lix, s.replay_rtp_bitmap = st
    assert ctx.import_(s) == 0


class World:
    """product sessions and their oracle twins with the same streams"""

    def __init__(self, torch, suite, nsess, streams, seed):
        self.torch, self.suite, self.nsess = torch, suite, nsess
        self.streams = streams
        self.rng = np.random.default_rng(seed)
        self.be = O.OracleBackend()
        keys = keys_for(suite, nsess)
        self.ctx = {side: [P.Srtp(suite, k) for k in keys]
                    for side in ("tx", "rx")}
        self.twin = {side: [self.be.alloc(suite, k, 0)[0] for k in keys]
                     for side in ("tx", "rx")}
        for st in streams:
            for side, state in (("tx", st.tx_state()), ("rx", st.rx_state())):
                imported(self.ctx[side][st.sess], st.ssrc, state)
                assert self.be.l.oracle_stream_set(
                    self.twin[side][st.sess], st.ssrc, *state) == 0
        self.prot = {}          # (stream index, k): the protected packet
        self.same_states("import")

    def close(self):
        for side in ("tx", "rx"):
            for c in self.ctx[side]:
                c.close()
            for c in self.twin[side]:
                self.be.free(c)

    def same_states(self, what):
        for side in ("tx", "rx"):
            for st in self.streams:
                (got,) = states([self.ctx[side][st.sess]], [st.ssrc])
                assert len(got) == 5, (what, side, hex(st.ssrc), got)
                want = self.be.export(self.twin[side][st.sess], st.ssrc)
                assert (got[0], got[1], got[4], got[3]) == want, \
                    (what, side, st.sess, hex(st.ssrc),
                     [hex(x) for x in got], [hex(x) for x in want])

    def call(self, side, op, pkts, entry, knobs, want, what):
        """pkts [(session, bytes)] through the oracle one at a time and
        through the product's entry; everything compared, then the path"""
        prot = op == "srtp_encrypt"
        rows = []
        for s, p in pkts:
            e, po, en, _, buf = self.be.call(
                self.twin[side][s], op, len(p) + 64, 0, len(p), p,
                len(p) + 16 if prot else len(p))
            rows.append((e, po, en, buf))
        arena, pos, end, cap, sess = to_arena(pkts)
        P.lib().srtp_gpu_tune(b"freshmulti", 0)
        c0 = {c: P.counter(c) for c in COUNTERS}
        with P.tune(**knobs):
            if entry == "dev":
                out = run_dev(self.torch, op, self.ctx[side], arena, pos, end,
                              cap, sess if self.nsess > 1 else None)
            else:
                out = run(self.torch, op, self.ctx[side], arena, pos, end,
                          cap, sess if self.nsess > 1 else None,
                          entry == "general")
        d = {c: P.counter(c) - c0[c] for c in COUNTERS}
        got_arena, p, e, err = out
        for i, (we, wpo, wen, buf) in enumerate(rows):
            got = (int(err[i]), int(p[i]) - int(pos[i]),
                   int(e[i]) - int(pos[i]))
            assert got == (we, wpo, wen), (what, i, got, (we, wpo, wen), d)
            n = wen if prot else len(buf)
            assert got_arena[pos[i]:pos[i] + n].tobytes() == buf[:n], \
                (what, i, d)
        self.same_states(what)
        assert {c: d[c] for c in want} == want, (what, d)
        return rows

    def send(self, who, entry, knobs, want, what):
        """the streams of who (indices, in send order) send their next
        packets"""
        pkts, ids = [], []
        for j in who:
            st = self.streams[j]
            k = st.sent
            st.sent += 1
            pkts.append((st.sess, rtp_packet(
                self.rng, st.seq(k), st.ssrc,
                plen=int(self.rng.integers(16, 65)))))
            ids.append((j, k))
        rows = self.call("tx", "srtp_encrypt", pkts, entry, knobs, want, what)
        assert not any(r[0] for r in rows)
        for i, r in zip(ids, rows):
            self.prot[i] = r[3][:r[2]]

    def recv(self, arrivals, entry, knobs, want, what):
        """arrivals [(stream index, k)] in arrival order"""
        pkts = [(self.streams[j].sess, self.prot[(j, k)])
                for j, k in arrivals]
        rows = self.call("rx", "srtp_decrypt", pkts, entry, knobs, want, what)
        errs = {r[0] for r in rows}
        assert errs <= {0, errno.EALREADY}, (what, errs)
        return rows


def path(counter, rejects):
    """counter deltas of a batch its device planner took (None: declined
    to the host engine, no planner counted it)"""
    want = {c: 0 for c in PLANNERS}
    if counter is not None:
        want[counter] = 1
        want["rejects"] = rejects
    return want


def disturbed(n, roll):
    """arrival order of one stream's n packets whose rollover is packet
    `roll` (beyond n: none in reach): adjacent swaps, a gap and a duplicate
    two arrivals late on both sides of it, none across it (a packet from
    before the rollover behind it is ETIMEDOUT in the reference)"""
    a = list(range(n))
    for i in (roll - 4, roll + 3, roll + 20, n - 3, 5):
        if 0 <= i and i + 1 < n and roll not in (i, i + 1):
            a[i], a[i + 1] = a[i + 1], a[i]
    a = [k for k in a if k not in (roll - 12, roll + 12)]
    ndup = 0
    for k in (roll + 8, roll - 8, 2):
        if k not in a or ndup == 2:
            continue
        at = a.index(k) + 2
        if at > len(a) or (k < roll and roll in a and at > a.index(roll)):
            continue
        a.insert(at, k)
        ndup += 1
    assert a != sorted(set(a))
    return a


def dealt(per_stream):
    """[(stream, k)] round-robin over the streams, each in its own order"""
    out, i = [], 0
    while any(i < len(a) for a in per_stream):
        out += [(j, a[i]) for j, a in enumerate(per_stream) if i < len(a)]
        i += 1
    return out


def second_batch(arrived, fresh, rolls):
    """per stream: its new packets with two packets it received in the
    first batch between them, both from behind its rollover (packet `roll`)
    if it had one (one from before it would be ETIMEDOUT)"""
    out = []
    for a, new, roll in zip(arrived, fresh, rolls):
        b = list(new)
        a = [k for k in a if k >= roll] or a
        if a:
            b.insert(1, a[-1])
            b.insert(min(4, len(b)), a[max(0, len(a) - 6)])
        out.append(b)
    return out


def round_trips(w, b, kind, first, ord_c, rx_c, knobs, more=8, rx_knobs=None):
    """protect, unprotect, and again on the carried state.  first: per
    stream its packets' arrival order in batch 1 (the sender sends them all,
    in order); ord_c / rx_c: the in-order and the receive planner's counter;
    rx_knobs: the knobs of the second unprotect where they differ"""
    def want(step, counter, dist):
        if (b, step, kind) in DECLINES and b != "2p16":
            return path(None, 0)
        return path(counter, 1 if dist else 0)

    nsent = [max(a) + 1 if a else 0 for a in first]
    w.send([j for j, k in dealt([list(range(n)) for n in nsent])], "dev",
           knobs, want("protect1", ord_c, False), (b, kind, "protect1"))
    w.recv(dealt(first), "dev", knobs,
           want("unprotect1", rx_c if kind == "disturbed" else ord_c,
                kind == "disturbed"), (b, kind, "unprotect1"))
    fresh = [list(range(n, n + more)) if n else [] for n in nsent]
    w.send([j for j, k in dealt(fresh)], "dev", knobs,
           want("protect2", ord_c, False), (b, kind, "protect2"))
    rolls = [(65535 - st.s_l) & 0xffff for st in w.streams]
    w.recv(dealt(second_batch(first, fresh, rolls)), "dev",
           knobs if rx_knobs is None else rx_knobs,
           want("unprotect2", rx_c, True), (b, kind, "unprotect2"))


# ---- one stream -------------------------------------------------------------

def one_stream(torch, suite, b, block, where, kind, knobs, ord_c, seed):
    n = 2 * block + 70
    roll = 37 if where == "wave" else block
    st = rolls_at(b, roll, 0, 0x726f6331)
    w = World(torch, suite, 1, [st], seed)
    try:
        first = disturbed(n, roll) if kind == "disturbed" else list(range(n))
        round_trips(w, b, kind, [first], ord_c, "rxplans", knobs)
        assert w.be.export(w.twin["tx"][0], st.ssrc)[0] == \
            (R.BOUNDS[b] + 1) & 0xffffffff
    finally:
        w.close()


@pytest.mark.parametrize("where", ["wave", "block"])
@pytest.mark.parametrize("b", BOUNDS)
@pytest.mark.parametrize("suite", range(6))
def test_one_stream_in_order(suite, b, where, torch_cuda):
    """the fused launch (AES-CM) and the one-launch GCM planner"""
    gcm = suite in GCM
    one_stream(torch_cuda, suite, b, LP_WG if gcm else FZ_BLOCK, where,
               "ordered", {}, "lplans" if gcm else "fused", 100 + suite)


@pytest.mark.parametrize("where", ["wave", "block"])
@pytest.mark.parametrize("b", BOUNDS)
@pytest.mark.parametrize("suite", [1, 3])
def test_one_stream_lean_planner(suite, b, where, torch_cuda):
    one_stream(torch_cuda, suite, b, LP_WG, where, "ordered", {"lplan": 1},
               "lplans", 200 + suite)


@pytest.mark.parametrize("where", ["wave", "block"])
@pytest.mark.parametrize("b", BOUNDS)
@pytest.mark.parametrize("suite", [1, 3, 5])
def test_one_stream_disturbed(suite, b, where, torch_cuda):
    """plan_rx.hip behind the in-order planner's rejection"""
    one_stream(torch_cuda, suite, b, RX_BLOCK, where, "disturbed", {},
               "lplans" if suite in GCM else "fused", 300 + suite)


@pytest.mark.parametrize("suite", [1, 5])
def test_stream_taken_over_above_2p31(suite, torch_cuda):
    """a stream handed over at ROC 0x80000005 before the receiver saw a
    packet of it (s_l set, lix 0, bitmap 0): no window to warn a planner.
    In order it is planned on the device, in the reference's sign-extended
    index; the disturbed batch behind it is declined"""
    st = Stream(0, 0x726f6332, 0x80000005, 1000)
    st.empty = True
    ord_c = "lplans" if suite in GCM else "fused"
    w = World(torch_cuda, suite, 1, [st], 350 + suite)
    try:
        w.send([0] * 300, "dev", {}, path(ord_c, 0), "protect1")
        w.recv([(0, k) for k in range(300)], "dev", {}, path(ord_c, 0),
               "unprotect1")
        assert w.be.export(w.twin["rx"][0], st.ssrc)[2] == \
            0xffff800000050000 + 1300
        w.send([0] * 40, "dev", {}, path(ord_c, 0), "protect2")
        w.recv([(0, 300 + k) for k in disturbed(40, 1 << 20)] + [(0, 299)],
               "dev", {}, path(None, 0), "unprotect2")
    finally:
        w.close()


# ---- one session, several SSRCs ---------------------------------------------

@pytest.mark.parametrize("kind", ["ordered", "disturbed"])
@pytest.mark.parametrize("nss", [2, 8])
@pytest.mark.parametrize("b", BOUNDS)
@pytest.mark.parametrize("suite", [1, 5])
def test_one_session_streams(suite, b, nss, kind, torch_cuda):
    """plan_streams.hip (splans) and plan_streams_rx.hip (srxplans): the
    streams dealt round-robin, stream j's packet k at batch position
    k * nss + j.  Stream 0 is at boundary b and rolls over on the first
    packet of the second workgroup, stream 1 at ROC 0; of eight, streams 2..
    are at the boundaries up to b and roll over inside the first wave, each
    at its own place, and the last two at ROC 0 and ROC 5"""
    block = SRX_BLOCK if kind == "disturbed" else SP_BLOCK
    per = (2 * block + 70) // nss
    bs = bounds_in(b)
    streams = [rolls_at(b, block // nss, 0, 0x53000000),
               rolls_at(None, 0, 0, 0x53000001)]
    for j in range(2, nss):
        streams.append(rolls_at(bs[j % len(bs)] if j < 6 else None, j, 0,
                                0x53000000 + j))
    if nss == 8:
        streams[7].roc = 5
    w = World(torch_cuda, suite, 1, streams, 400 + suite)
    try:
        first = []
        for j, st in enumerate(streams):
            roll = (65535 - st.s_l) & 0xffff
            first.append(disturbed(per, roll)
                         if kind == "disturbed" and j % 3 != 1
                         else list(range(per)))
        round_trips(w, b, kind, first, "splans", "srxplans", {})
    finally:
        w.close()


# ---- many sessions ----------------------------------------------------------

def many_sessions(torch, suite, b, nsess, nss, kind, knobs, ord_c, rx_c, seed,
                  rx_knobs=None):
    """nsess sessions of nss SSRCs and PER packets per stream.  The sessions
    from k0 on are at the boundaries up to b, three per boundary, adjacent,
    each rolling over at its own packet (k0: the session whose packets
    start at position BPB of a batch grouped by session, where the batch
    is that long; else the middle); the others at ROC 0, every third of
    them rolling over to ROC 1 as well"""
    k0 = min(BPB // (PER * nss) if nsess * nss * PER > BPB else nsess // 2,
             nsess - 10)
    at = {}
    for i, bb in enumerate(bounds_in(b)):
        for q in range(3):
            at[k0 + 3 * i + q] = (bb, 2 + 5 * q + i)
    assert max(at) < nsess
    streams = []
    for s in range(nsess):
        for k in range(nss):
            ssrc = 0x4d000000 | s << 8 | k
            if s in at and k == 0:
                streams.append(rolls_at(at[s][0], at[s][1], s, ssrc))
            elif s in at:
                streams.append(rolls_at(None, 0, s, ssrc))
            elif s % 3 == 0:
                streams.append(Stream(s, ssrc, 0, 65535 - (1 + s % 11)))
            else:
                streams.append(rolls_at(None, 0, s, ssrc))
    w = World(torch, suite, nsess, streams, seed)
    try:
        first = []
        for j, st in enumerate(streams):
            roll = (65535 - st.s_l) & 0xffff
            dist = kind == "disturbed" and (st.sess in at or st.sess % 4 == 1)
            first.append(disturbed(PER, roll) if dist else list(range(PER)))
        round_trips(w, b, kind, first, ord_c, rx_c, knobs, more=6,
                    rx_knobs=rx_knobs)
    finally:
        w.close()


@pytest.mark.parametrize("b", BOUNDS)
@pytest.mark.parametrize("suite", [1, 5])
def test_many_sessions_counting_planner(suite, b, torch_cuda):
    """plan_multi.hip: 40 sessions, in order (nobucket=1).  It has no
    receive planner of its own (mrx_eligible, batch_dev.c): the second
    unprotect, with its replays, runs without the knob"""
    many_sessions(torch_cuda, suite, b, 40, 1, "ordered", {"nobucket": 1},
                  "mplans", "mrxplans", 500 + suite, rx_knobs={})


@pytest.mark.parametrize("kind", ["ordered", "disturbed"])
@pytest.mark.parametrize("b", BOUNDS)
@pytest.mark.parametrize("suite", [1, 3, 5])
def test_many_sessions_bucket_planner(suite, b, kind, torch_cuda):
    """plan_buckets.hip (mplans) and plan_buckets_rx.hip (mrxplans): 130
    sessions in two buckets"""
    many_sessions(torch_cuda, suite, b, 130, 1, kind, {}, "mplans",
                  "mrxplans", 600 + suite)


@pytest.mark.parametrize("kind", ["ordered", "disturbed"])
@pytest.mark.parametrize("b", BOUNDS)
@pytest.mark.parametrize("suite", [1, 5])
def test_many_sessions_two_ssrcs(suite, b, kind, torch_cuda):
    """plan_buckets_rtp_streams.hip (msplans) and its receive planner
    (msrxplans): 40 sessions of two SSRCs in three buckets"""
    many_sessions(torch_cuda, suite, b, 40, 2, kind, {"bpexp": 250},
                  "msplans", "msrxplans", 700 + suite)


# ---- the other entry points -------------------------------------------------

def small_world(torch, suite, b, seed):
    """one stream that rolls over at its tenth packet, 40 arrivals"""
    st = rolls_at(b, 9, 0, 0x6f746831)
    return World(torch, suite, 1, [st], seed), disturbed(40, 9)


@pytest.mark.parametrize("entry", ["general", "noplan"])
@pytest.mark.parametrize("b", BOUNDS)
@pytest.mark.parametrize("suite", [1, 5])
def test_host_planned_batches(suite, b, entry, torch_cuda):
    """srtp_*_batch with host arrays under general=1 (the general engine)
    and noplan=1 (the host-planned fast path): the host's own index"""
    w, first = small_world(torch_cuda, suite, b, 800 + suite)
    ent = "general" if entry == "general" else "host"
    knobs = {entry: 1}
    host = path(None, 0)
    try:
        w.send([0] * 40, ent, knobs, host, (b, entry, "protect1"))
        w.recv([(0, k) for k in first], ent, knobs, host,
               (b, entry, "unprotect1"))
        w.send([0] * 8, ent, knobs, host, (b, entry, "protect2"))
        (second,) = second_batch([first], [list(range(40, 48))], [9])
        w.recv([(0, k) for k in second], ent, knobs, host,
               (b, entry, "unprotect2"))
    finally:
        w.close()


def mbuf_result(e, mb):
    m = mb.contents
    return (e, m.pos, m.end, m.size, ctypes.string_at(m.buf, m.size))


@pytest.mark.parametrize("entry", ["percall", "mbufs"])
@pytest.mark.parametrize("b", BOUNDS)
@pytest.mark.parametrize("suite", [1, 5])
def test_mbuf_entries(suite, b, entry, torch_cuda):
    """one mbuf per srtp_encrypt / srtp_decrypt (the per-call small kernel)
    and the mbuf batch srtp_*_mbufs, packet for packet against the oracle"""
    be = O.OracleBackend()
    key = keys_for(suite, 1)[0]
    st = rolls_at(b, 9, 0, 0x6d627566)
    rng = np.random.default_rng(900 + suite)
    ctx = {"tx": P.Srtp(suite, key), "rx": P.Srtp(suite, key)}
    twin = {}
    for side, state in (("tx", st.tx_state()), ("rx", st.rx_state())):
        imported(ctx[side], st.ssrc, state)
        twin[side] = R.oracle_at(be, suite, key, st.ssrc, state)
    first = disturbed(40, 9)
    (second,) = second_batch([first], [list(range(40, 48))], [9])
    prot = {}
    small0 = P.counter("small_launches")

    def step(side, op, datas, what):
        want = [be.call(twin[side], op, len(d) + 32, 0, len(d), d,
                        len(d) + 32) for d in datas]
        mbs = [P.new_mbuf(d, len(d) + 32, 0) for d in datas]
        if entry == "percall":
            with P.tune(nosmall=0):
                errs = [ctx[side]._op(op, mb) for mb in mbs]
        else:
            rc, errs = P.batch_run(ctx[side], op, mbs)
            assert rc == 0
        for i, (mb, e, w) in enumerate(zip(mbs, errs, want)):
            got = mbuf_result(e, mb)
            assert got[:4] == w[:4], (what, i, got[:4], w[:4])
            assert got[4] == w[4], (what, i)
            P.free_mbuf(mb)
        (got,) = states([ctx[side]], [st.ssrc])
        exp = be.export(twin[side], st.ssrc)
        assert (got[0], got[1], got[4], got[3]) == exp, \
            (what, [hex(x) for x in got], [hex(x) for x in exp])
        return want

    try:
        for lo, hi, arrivals in ((0, 40, first), (40, 48, second)):
            plain = [rtp_packet(rng, st.seq(k), st.ssrc,
                                plen=int(rng.integers(16, 65)))
                     for k in range(lo, hi)]
            rows = step("tx", "srtp_encrypt", plain, (b, entry, "protect", lo))
            assert not any(r[0] for r in rows)
            for k, r in zip(range(lo, hi), rows):
                prot[k] = r[4][:r[2]]
            rows = step("rx", "srtp_decrypt", [prot[k] for k in arrivals],
                        (b, entry, "unprotect", lo))
            assert {r[0] for r in rows} <= {0, errno.EALREADY}
        if entry == "percall":
            assert P.counter("small_launches") > small0
    finally:
        for side in ("tx", "rx"):
            ctx[side].close()
            be.free(twin[side])
