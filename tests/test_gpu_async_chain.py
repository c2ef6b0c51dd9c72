"""Chained asynchronous device batches over every planner route, against the
oracle (srtp_*_batch_dev_async + srtp_batch_wait, batch_async.c
tk_finish_one, whose fallback ladder must reach what run_dev's reaches).

The scenarios are those of tests/async_traffic.py (checked by
tests/test_async_traffic_cpu.py): c1 protect, c2 the route's disturbed call,
c3 unprotect of c1's arena queued behind c2, c4 protect, on disjoint
contexts, all issued before any is waited for.  Every call's errno, pos, end
and bytes and every context's exported state must be the oracle's, through
the asynchronous entries and through the synchronous ones; the planners'
counters must move alike under both, and "gated" by the number of calls
queued behind a c2 whose gate word was set.

c3 shares c1's arena, pos and end (it reads what c1 wrote), so after an
asynchronous chain c1's bytes are gone: there c1 shows in its errnos and
through c3 -- c3's tags verify on a context of its own, and the bytes the
oracle leaves behind c3 include c1's tag.  The synchronous chain looks at
every call's output right after the call.

Expected "gated", from batch_dev.c: plan_out_back (fused and one-launch
plans), sgpu_plan_finish (the separate planner, the per-stream planner, the
many-session planner) and the bucket planner's finish set the gate word when
the plan failed, or when a tag did not verify and no device fold sits behind
the kernels.  So a rejected c2 gates c3, whose own plan then fails with
SPF_PRED and gates c4: 2.  A forged packet gates alike on the fused, the
one-launch and the per-stream routes (the fold runs when c2 is waited for),
and not behind the separate planner and the many-session planner, whose fold
is queued with the kernels: 0.  A many-session c2 whose gather meets a
session of several streams (m_multi) is never queued: it completes c1, runs
synchronously, and c3 starts a new chain: 0.
"""
import numpy as np
import pytest

import re_amd.srtp as P
from tests import async_traffic as T
from tests.test_gpu_async import Dev
from tests.test_gpu_fastpath import to_arena

pytestmark = pytest.mark.gpu

ROUTE_COUNTERS = ("rejects", "rxplans", "srxplans", "mrxplans", "splans",
                  "msplans", "msrxplans")
COUNTERS = ROUTE_COUNTERS + ("mplans", "misses", "gated")


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    yield torch
    P.lib().srtp_gpu_tune(b"freshmulti", 0)


class ChainDev(Dev):
    """a call's device arrays; base: the call whose arena, pos, end and cap
    it shares (an err array of its own); pos0: where the packets start"""

    def __init__(self, torch, call, many, base=None):
        if base is None:
            arena, pos, end, cap, sess = to_arena(call.pkts,
                                                  short_cap=call.short_cap)
            super().__init__(torch, arena, pos, end, cap,
                             sess if many else None)
            self.pos0 = pos.astype(np.int64)
            return
        self.arena, self.nbytes, self.n = base.arena, base.nbytes, base.n
        self.pos, self.end, self.cap = base.pos, base.end, base.cap
        self.sess, self.pos0 = base.sess, base.pos0
        self.err = torch.full((self.n,), -1, dtype=torch.int32,
                              device="cuda")


def counters():
    return {c: P.counter(c) for c in COUNTERS}


def moved(c0):
    return {c: P.counter(c) - c0[c] for c in COUNTERS}


class Run:
    """one scenario through one entry on fresh contexts"""

    def __init__(self, torch, sc, mode, streams=None):
        self.torch, self.sc, self.mode = torch, sc, mode
        # every mode from the same first-batch hint (a rejected plan for a
        # second SSRC of a fresh session sets it, re_srtp_batch.h)
        P.lib().srtp_gpu_tune(b"freshmulti", 0)
        self.ctx = {sid: [P.Srtp(sc.suite, k) for k in sc.keys(sid)]
                    for sid in sc.sets}
        self.devs = []
        for c in sc.calls:
            self.devs.append(ChainDev(
                torch, c, sc.sets[c.set][1] > 1,
                self.devs[c.share] if c.share is not None else None))
        self.streams = streams or [None] * len(sc.calls)
        self.outs = [None] * len(sc.calls)
        self.percall = [None] * len(sc.calls)
        self.pend = []
        torch.cuda.synchronize()
        self.c0 = counters()
        self.gated0 = None

    def issue(self, i):
        c, d = self.sc.calls[i], self.devs[i]
        if c.role != "pre" and self.gated0 is None:
            self.gated0 = P.counter("gated")
        if self.mode == "sync":
            b = counters()
            rc = P.device_batch_dev(c.op, self.ctx[c.set], *d.args(),
                                    self.streams[i])
            assert rc == 0, (i, rc, P.lib().srtp_gpu_error())
            self.torch.cuda.synchronize()
            self.percall[i] = moved(b)
            self.outs[i] = d.out()
            return
        rc, t, keep = P.device_batch_dev_async(c.op, self.ctx[c.set],
                                               *d.args(), self.streams[i])
        assert rc == 0
        if c.role == "pre":
            assert P.batch_wait(t) == 0, P.lib().srtp_gpu_error()
        else:
            self.pend.append((i, t, keep))

    def wait(self, order="issue"):
        pend = self.pend[::-1] if order == "reverse" else self.pend
        for k, (i, t, _) in enumerate(pend):
            assert P.batch_wait(t) == 0, (i, P.lib().srtp_gpu_error())
            if order == "reverse" and k == 0:
                # waiting for the last completed every call before it
                self.torch.cuda.synchronize()
                self.collect()
        self.pend = []

    def collect(self):
        self.torch.cuda.synchronize()
        for i, d in enumerate(self.devs):
            if self.outs[i] is None:
                self.outs[i] = d.out()

    def finish(self):
        self.collect()
        self.delta = moved(self.c0)
        self.gated = P.counter("gated") - self.gated0

    def check(self):
        """every call and every context against the oracle"""
        sc = self.sc
        shared = {c.share for c in sc.calls if c.share is not None}
        for i, c in enumerate(sc.calls):
            arena, pos, end, err = self.outs[i]
            what = (sc.name, sc.suite, self.mode, c.role)
            want = np.array(c.errnos(), dtype=np.int32)
            assert (err == want).all(), \
                (what, [(int(j), int(err[j]), int(want[j]))
                        for j in np.flatnonzero(err != want)[:8]])
            if self.mode != "sync" and i in shared:
                continue        # overwritten by the call that shares it
            p0 = self.devs[i].pos0
            for j, (e, po, en, buf) in enumerate(c.rows):
                got = (int(pos[j]) - int(p0[j]), int(end[j]) - int(p0[j]))
                assert got == (po, en), (what, j, got, (e, po, en))
                a = int(p0[j])
                assert arena[a:a + len(buf)].tobytes() == buf, (what, j, e)
        for sid, want in sc.states.items():
            for (s, ssrc), w in want.items():
                e, st = self.ctx[sid][s].export(ssrc)
                assert e == 0, (sc.name, self.mode, sid, s, hex(ssrc))
                got = (st.roc, st.s_l, st.replay_rtp_lix,
                       st.replay_rtp_bitmap)
                assert got == w, (sc.name, self.mode, sid, s, hex(ssrc))

    def close(self):
        for v in self.ctx.values():
            for c in v:
                c.close()


def run_sync(torch, sc, streams=None):
    r = Run(torch, sc, "sync", streams)
    try:
        for i in range(len(sc.calls)):
            r.issue(i)
        r.finish()
        r.check()
    finally:
        r.close()
    return r


def run_async(torch, sc, order="issue", streams=None):
    """every call of the chain issued before any is waited for"""
    r = Run(torch, sc, "async", streams)
    try:
        for i in range(len(sc.calls)):
            r.issue(i)
        if order == "export":
            # any other entry point of the thread completes the pending calls
            c1 = sc.call("c1")
            e, _ = r.ctx[c1.set][0].export(T.ssrc_of(0))
            assert e == 0
            r.collect()
        r.wait(order)
        r.finish()
        r.check()
    finally:
        r.close()
    return r


def gated_expected(name, knobs=()):
    if name in ("m_forged", "m_multi"):
        return 0
    if name == "forged1" and "noplanfuse" in knobs:
        return 0
    return 2


def both(torch, sc, knobs=None):
    """the synchronous and the asynchronous chain against the oracle, and
    the routes they took against each other"""
    knobs = knobs or {}
    with P.tune(**knobs):
        rs = run_sync(torch, sc)
        ra = run_async(torch, sc)
    print("ROUTE %-11s suite %d %-22s reach %-9s sync %s | async %s | gated "
          "%d" % (sc.name, sc.suite, "+".join(sorted(knobs)) or "default",
                  sc.reach,
                  {k: v for k, v in rs.delta.items() if v and k != "gated"},
                  {k: v for k, v in ra.delta.items() if v and k != "gated"},
                  ra.gated))
    # the scenario reaches its route: c2's own call moves the counter
    c2 = rs.percall[sc.index("c2")]
    assert c2[sc.reach] >= 1, (sc.name, sc.reach, c2)
    assert rs.gated == 0
    for c in ROUTE_COUNTERS:
        assert ra.delta[c] == rs.delta[c], (sc.name, c, rs.delta, ra.delta)
    assert ra.gated == gated_expected(sc.name, knobs), (sc.name, ra.gated)
    return rs, ra


# ---- a, b: every route, chained, against the oracle; route parity ---------------

@pytest.mark.parametrize("suite", T.SUITES)
@pytest.mark.parametrize("name", list(T.ROUTES))
def test_chain(torch_cuda, name, suite):
    both(torch_cuda, T.scenario(name, suite))


# ---- c: where the single-stream plan writes the gate word ---------------------

KNOBS = {"default": {}, "nopost": {"nopost": 1}, "lplan": {"lplan": 1},
         "lplan_nopost": {"lplan": 1, "nopost": 1},
         "noplanfuse": {"noplanfuse": 1}}


@pytest.mark.parametrize("suite,mode",
                         [(1, m) for m in KNOBS] +
                         [(5, "lplan"), (5, "lplan_nopost")])
@pytest.mark.parametrize("name", ["rx", "forged1", "reject_host"])
def test_gate_write_variants(torch_cuda, name, suite, mode):
    """the post launch, the copy with sgpu_plan_finish in front (nopost),
    both again behind the one-launch planner (lplan), and the separate
    planner's dp_issue (noplanfuse), whose device fold does not gate"""
    both(torch_cuda, T.scenario(name, suite), KNOBS[mode])


# ---- d: wait order and draining ------------------------------------------------

@pytest.mark.parametrize("name", ["rx", "m_rx"])
def test_wait_in_reverse_order(torch_cuda, name):
    """waiting for the last ticket completes every call (Run.wait looks at
    all the outputs right after the first wait)"""
    r = run_async(torch_cuda, T.scenario(name, 1), order="reverse")
    assert r.gated == 2


@pytest.mark.parametrize("name", ["rx", "m_rx"])
def test_export_drains(torch_cuda, name):
    """no ticket waited for: export() on one context completes them all, the
    results are there before any wait, the tickets still give theirs"""
    r = run_async(torch_cuda, T.scenario(name, 1), order="export")
    assert r.gated == 2


@pytest.mark.parametrize("name", ["rx", "m_rx"])
def test_fifth_and_sixth_call_complete_the_oldest(torch_cuda, name):
    """six calls on six disjoint context sets and no wait, the rejected one
    second: the fifth completes c1 and is queued behind the gated c4, the
    sixth completes c2 on the host and is queued behind the gated fifth"""
    sc = T.six(name, 1)
    r = run_async(torch_cuda, sc)
    assert r.delta[sc.reach] == 1
    assert r.gated == 4


# ---- e: streams ------------------------------------------------------------------

def test_chain_on_a_stream_of_its_own(torch_cuda):
    torch = torch_cuda
    sc = T.scenario("rx", 1)
    st = torch.cuda.Stream()
    h = [st.cuda_stream] * len(sc.calls)
    rs = run_sync(torch, sc, h)
    ra = run_async(torch, sc, streams=h)
    for c in ROUTE_COUNTERS:
        assert ra.delta[c] == rs.delta[c], (c, rs.delta, ra.delta)
    assert ra.delta["rxplans"] == 1 and ra.gated == 2


def test_stream_change_drains(torch_cuda):
    """c1 and c2 on one stream, c3 and c4 on another: the gate words are
    ordered by the stream, so the change completes c1 and c2 first, and c3
    and c4 start a chain of their own that nothing gates"""
    torch = torch_cuda
    sc = T.scenario("rx", 1)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    h = [sa.cuda_stream if c.role in ("pre", "c1", "c2") else sb.cuda_stream
         for c in sc.calls]
    ra = run_async(torch, sc, streams=h)
    assert ra.delta["rxplans"] == 1
    assert ra.gated == 0


# ---- f: the gate ring -----------------------------------------------------------

def test_gate_ring_reuse(torch_cuda):
    """140 queued calls of one thread on its 64 gate words (call number q, from
    1, uses word q % 64), in groups of 4 issued then waited for, every 7th
    call rejected: a rejected call leaves 1 in its word, and so does every
    call gated behind it.  By the issue pattern that is 50 calls on 33 of the
    words, 23 of which are used again by a later call: that one must start
    from the word of the call in front of it, not from what its own word
    held, and must overwrite it"""
    torch = torch_cuda
    sc = T.ring()
    r = Run(torch, sc, "async")
    bad = set(sc.claims["reordered"])
    want = 0
    ones = {}
    try:
        r.gated0 = P.counter("gated")
        for g in range(0, len(sc.calls), 4):
            hit = False
            for i in range(g, g + 4):
                r.issue(i)
                want += hit
                if hit or i in bad:
                    ones.setdefault((i + 1) % 64, i)
                hit = hit or i in bad
            r.wait()
        r.finish()
        r.check()
    finally:
        r.close()
    assert r.delta["rxplans"] == len(bad) == 20
    assert r.delta["rejects"] == len(bad)
    assert r.gated == want == 30
    assert len(ones) == 33
    assert sum(i + 64 < len(sc.calls) for i in ones.values()) == 23
