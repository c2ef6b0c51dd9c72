"""Many-session batches whose sessions use different suites, the product
beside the oracle twin (the scenarios of tests/mixed_traffic.py, checked by
tests/test_mixed_traffic_cpu.py).

After every batch: per packet errno, pos and end relative to the packet and
every byte the oracle leaves; per (session, SSRC) the exported RTP state
(roc, s_l, s_l_set, lix, bitmap) and SRTCP state (rtcp_index, lix, bitmap).
Bit for bit, no tolerance.

Entries: "dev" srtp_*_batch_dev / srtcp_*_batch_dev with a device session
array, "host" srtp_*_batch / srtcp_*_batch with host arrays, "async"
srtp_*_batch_dev_async + srtp_batch_wait (RTP only: there is no asynchronous
SRTCP entry).

What the code does with a mixed batch, asserted through the counters around
every mixed call: the many-session gathers (mplan_gather_part,
msplan_count_part, mrplan_count_part, batch_host.c) decline at the first
session whose suite (SRTCP: or SRTP_UNENCRYPTED_SRTCP) is not session 0's,
before any plan is launched, so the issue returns -1 without counting: no
planner counter moves, and "rejects" (plans the device rejected) does not
move either.  The call goes sess_host() -> after_host() -> dev_staged() ->
run_batch(), where run_fast declines on the suites too, and the general
engine (run_batch_general) completes it.
"""
import threading

import numpy as np
import pytest

import re_amd.srtp as P
from tests import mixed_traffic as M
from tests.test_gpu_async import Dev
from tests.test_gpu_fastpath import to_arena

pytestmark = pytest.mark.gpu

PLANNERS = ("mplans", "msplans", "mrxplans", "msrxplans", "mrplans",
            "mrrxplans", "lplans", "fused", "dplans", "splans", "srplans",
            "rplans")
COUNTERS = PLANNERS + ("rejects",)
WAIT = 60       # seconds a thread waits for the other before it gives up


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    yield torch
    P.lib().srtp_gpu_tune(b"freshmulti", 0)


def counters():
    return {c: P.counter(c) for c in COUNTERS}


def moved(c0):
    return {c: P.counter(c) - v for c, v in c0.items() if P.counter(c) != v}


def arrays(st):
    """a step's arena and arrays; sessions numbered within st.sub"""
    lo = st.sub[0] if st.sub else 0
    arena, pos, end, cap, sess = to_arena([(s - lo, p) for s, p in st.pkts])
    cap = (end + np.array(st.rooms, dtype=np.uint32)).astype(np.uint32)
    return arena, pos, end, cap, sess


def rows_of(st, pos0, arena, pos, end, err):
    out = []
    for i, (_, q) in enumerate(st.pkts):
        b, n = int(pos0[i]), int(end[i]) - int(pos0[i])
        out.append((int(err[i]), int(pos[i]) - b, n,
                    arena[b:b + max(n, len(q))].tobytes()))
    return out


class Prod:
    """product contexts of a scenario's sessions through one entry"""

    def __init__(self, torch, sc, entry):
        self.torch, self.sc, self.entry = torch, sc, entry
        # (every run from the same first-batch hint, tests/test_gpu_fused.py)
        P.lib().srtp_gpu_tune(b"freshmulti", 0)
        self.ctx = [P.Srtp(u, M.session_key(u, s), f) for s, (u, f) in
                    enumerate(zip(sc.suites, sc.flags))]
        assert not any(c.err for c in self.ctx)

    def close(self):
        for c in self.ctx:
            c.close()

    def sessions(self, st):
        return self.ctx[st.sub[0]:st.sub[1]] if st.sub else self.ctx

    def run(self, st, entry=None):
        """the step through the entry: rows like the oracle's"""
        entry = entry or self.entry
        torch = self.torch
        ctx = self.sessions(st)
        arena, pos, end, cap, sess = arrays(st)
        if entry == "host":
            dev = torch.from_numpy(arena.copy()).cuda()
            p, e = pos.copy(), end.copy()
            torch.cuda.synchronize()
            rc, err = P.device_batch(st.op, ctx, dev.data_ptr(),
                                     arena.nbytes, p, e, cap, sess)
            assert rc == 0, (rc, P.lib().srtp_gpu_error())
            return rows_of(st, pos, dev.cpu().numpy(), p, e, err)
        d = Dev(torch, arena, pos, end, cap, sess)
        torch.cuda.synchronize()
        if entry == "dev":
            rc = P.device_batch_dev(st.op, ctx, *d.args())
        else:
            rc, t, keep = P.device_batch_dev_async(st.op, ctx, *d.args())
            assert rc == 0
            rc = P.batch_wait(t)
        assert rc == 0, (rc, P.lib().srtp_gpu_error())
        torch.cuda.synchronize()
        return rows_of(st, pos, *d.out())

    def state(self, s, ssrc):
        e, st = self.ctx[s].export(ssrc)
        if e:
            return None
        return ((st.roc, st.s_l, st.s_l_set, st.replay_rtp_lix,
                 st.replay_rtp_bitmap),
                (st.rtcp_index, st.replay_rtcp_lix, st.replay_rtcp_bitmap))


def same_rows(what, st, got, suites):
    ge, we = [g[0] for g in got], st.errnos()
    assert ge == we, (what, [(i, suites[st.pkts[i][0]], g, w) for i, (g, w)
                             in enumerate(zip(ge, we)) if g != w][:8])
    for i, (g, w) in enumerate(zip(got, st.rows)):
        u = suites[st.pkts[i][0]]
        assert g[:3] == w[:3], (what, i, "suite", u, g[:3], w[:3])
        assert g[3] == w[3], (what, i, "suite", u, "bytes", g[:3])


def same_states(what, st, prod, suites):
    for (s, x), w in st.states.items():
        g = prod.state(s, x)
        assert g == w, (what, "state", s, "suite", suites[s], hex(x), g, w)


def mixed(sc, st):
    lo, hi = st.sub or (0, len(sc.suites))
    return len(set(sc.suites[lo:hi])) > 1 or \
        (st.op in M.RTCP_OPS and len(set(sc.flags[lo:hi])) > 1)


def replay(torch, sc, entry, what):
    """the scenario's steps through tx and rx product contexts; around every
    mixed call no planner counter and no reject (module docstring)"""
    prod = {k: Prod(torch, sc, entry) for k in ("tx", "rx")}
    try:
        for st in sc.steps:
            w = (what, sc.name, entry, st.what, st.op)
            c0 = counters()
            got = prod[st.side].run(st)
            dc = moved(c0)
            print("MIXED %-9s %-6s %-26s %s" % (sc.name, entry, st.what, dc))
            same_rows(w, st, got, sc.suites)
            same_states(w, st, prod[st.side], sc.suites)
            if mixed(sc, st):
                assert not dc, (w, dc)
    finally:
        for p in prod.values():
            p.close()


# ---- 1, 2: round trips -----------------------------------------------------------

@pytest.mark.parametrize("shape", M.SHAPES)
@pytest.mark.parametrize("entry", ["dev", "host", "async"])
def test_mixed_round_trip(torch_cuda, entry, shape):
    """protect, unprotect with a forged packet, a duplicate and a swap per
    suite, and a second pair in order on the same contexts, every batch over
    sessions of several suites: rows and states are the oracle's, and no
    planner counter and no reject moves (the gathers decline before any plan
    is tried; the general engine completes the call).  The odd_* shapes once
    more with the gather split over the host pool (par_min 4: parts of four
    sessions, the odd session not in the first)"""
    sc = M.rtp_scenario(shape)
    replay(torch_cuda, sc, entry, "round trip")
    if shape != "cycle":
        P.lib().srtp_gpu_tune(b"par_min", 4)
        try:
            replay(torch_cuda, sc, entry, "round trip, par_min 4")
        finally:
            P.lib().srtp_gpu_tune(b"par_min", 0)


@pytest.mark.parametrize("entry", ["dev", "host"])
def test_mixed_srtcp_round_trip(torch_cuda, entry):
    """the same for SRTCP, the sessions mixed in suite and in
    SRTP_UNENCRYPTED_SRTCP, with a protect refused for a byte of room per
    suite (ENOMEM, the trailer length is the session's own)"""
    for shape in ("cycle", "odd_mid"):
        replay(torch_cuda, M.rtcp_scenario(shape), entry, "srtcp")


# ---- 3: resident states handed to the host and back ------------------------------------

@pytest.mark.parametrize("pair", M.HAND_PAIRS, ids=["s1s5", "s3s4"])
def test_resident_handover(torch_cuda, pair):
    """the stages as protect ("tx") and as unprotect ("rx")"""
    for side in ("tx", "rx"):
        handover(torch_cuda, pair, side)


def handover(torch_cuda, pair, side):
    """stage A, one batch per suite, planned on the device (mplans + 1 each):
    the states are resident (DRES_DEV).  Stage B, one mixed batch over all
    eight sessions: sess_host() reads them back, every stream crosses 65535
    -> 0 on the host engine.  Stage C, one batch per suite again, mplans + 1
    each: the states go up again, and a stale device copy would show as the
    old ROC in the ciphertext (tx) or as EAUTH rows (rx).  rx: two forged
    packets in stage B.

    srtp_stream_export reads a resident state back itself (sess_host), so
    the stages run twice: once with the states compared only after stage C
    -- stage B then meets the states where stage A left them, on the device
    -- and once with the states compared after every stage"""
    torch = torch_cuda
    sc = M.handover_scenario(pair, side)
    for every in (False, True):
        prod = Prod(torch, sc, "dev")
        try:
            for st in sc.steps:
                w = ("handover", pair, side, st.what, every)
                c0 = counters()
                got = prod.run(st)
                dc = moved(c0)
                print("HANDOVER %s %s %s %s" % (pair, side, st.what, dc))
                same_rows(w, st, got, sc.suites)
                if st.what[0] == "B":
                    assert not dc, (w, dc)
                else:
                    assert dc == {"mplans": 1}, (w, dc)
                if every or st is sc.steps[-1]:
                    same_states(w, st, prod, sc.suites)
        finally:
            prod.close()


# ---- 4: the general engine by the knob --------------------------------------------------

def test_mixed_general_engine_agrees(torch_cuda):
    """the cycle receive batch (fresh receivers, the disturbances inside)
    under srtp_gpu_tune general = 1 and without it, through both synchronous
    entries: the same rows and states, and the oracle's.

    general = 1 does bypass run_fast for many-session batches: run_batch
    (batch_host.c) tries run_fast only under "... && !g_env.general" and
    otherwise falls through to run_batch_general; run_dev and batch_async
    (batch_async.c) try the many-session device planners only under
    "!g_env.noplan && !g_env.general".  Without the knob the same batch
    reaches run_batch_general because run_fast returns -1 on the second
    suite, so the two runs differ in everything a declined attempt may leave
    behind"""
    torch = torch_cuda
    sc = M.rtp_scenario("cycle")
    st = sc.steps[1]
    assert st.side == "rx" and st.forged
    res = {}
    for entry in ("dev", "host"):
        for general in (0, 1):
            prod = Prod(torch, sc, entry)
            try:
                with P.tune(general=general):
                    c0 = counters()
                    got = prod.run(st)
                    assert not moved(c0)
                w = ("general", general, entry)
                same_rows(w, st, got, sc.suites)
                same_states(w, st, prod, sc.suites)
                res[(entry, general)] = (
                    got, [prod.state(s, x) for s, x in sorted(st.states)])
            finally:
                prod.close()
    first = res[("dev", 0)]
    assert all(v == first for v in res.values())


# ---- 5: a declined asynchronous call leaves no pending mark ---------------------------

def one_session_calls(torch, prod, st, s, tag, got):
    """the main thread on session s: srtp_encrypt_batch_dev without a session
    array and the per-packet srtp_encrypt, on the session's next two packets
    (st: the step that holds them, with the oracle's rows), and export"""
    mine = [(i, p) for i, (t, p) in enumerate(st.pkts) if t == s][:2]
    (i0, p0), (i1, p1) = mine
    arena, pos, end, cap, _ = to_arena([(0, p0)])
    d = Dev(torch, arena, pos, end, cap, None)
    torch.cuda.synchronize()
    got[tag + "_dev"] = P.device_batch_dev("srtp_encrypt", [prod.ctx[s]],
                                           *d.args())
    torch.cuda.synchronize()
    a, p, e, err = d.out()
    got[tag + "_dev_row"] = (int(err[0]), a[int(pos[0]):int(e[0])].tobytes())
    mb = P.new_mbuf(p1, len(p1) + 64)
    got[tag + "_one"] = prod.ctx[s].encrypt(mb)
    got[tag + "_one_row"] = P.mbuf_bytes(mb)
    P.free_mbuf(mb)
    got[tag + "_export"] = prod.ctx[s].export(M.ssrc_in("srtp_encrypt", p0))[0]
    return (st.rows[i0][3][:st.rows[i0][2]], st.rows[i1][3][:st.rows[i1][2]])


def free_and_right(got, tag, want):
    assert (got[tag + "_dev"], got[tag + "_one"], got[tag + "_export"]) == \
        (0, 0, 0), (tag, {k: v for k, v in got.items() if "row" not in k})
    assert got[tag + "_dev_row"] == (0, want[0]), tag
    assert got[tag + "_one_row"] == want[1], tag


def issue_async(torch, prod, st, got, tag):
    """st through the asynchronous entry on the calling thread: (ticket,
    what keeps the arrays alive)"""
    arena, pos, end, cap, sess = arrays(st)
    d = Dev(torch, arena, pos, end, cap, sess)
    torch.cuda.synchronize()
    rc, t, keep = P.device_batch_dev_async(st.op, prod.sessions(st),
                                           *d.args())
    got[tag + "_issue"] = rc
    return t, (d, keep, pos)


def wait_async(torch, st, got, tag, t, held):
    d, _, pos = held
    got[tag + "_wait"] = P.batch_wait(t)
    torch.cuda.synchronize()
    got[tag + "_rows"] = rows_of(st, pos, *d.out())


@pytest.mark.parametrize("case", ["cycle", "odd_mid", "multi",
                                  "behind_pending"])
def test_declined_async_call_leaves_no_pending_mark(torch_cuda, case):
    """finding: the gather of an asynchronous many-session call marks every
    session it visits as pending (pend_m = the call's sequence number) before
    it meets the one that makes it decline; batch_async then completes the
    call synchronously and must account that sequence number as completed,
    or sess_busy() reports those sessions busy to every other thread until
    the issuing thread completes some later queued call -- never, if it makes
    none or has exited"""
    if case == "behind_pending":
        declined_behind_a_pending_one(torch_cuda)
    else:
        declined_and_thread_exits(torch_cuda, case)


def declined_and_thread_exits(torch_cuda, case):
    """a worker thread issues one asynchronous protect whose many-session
    gather declines after it has visited some sessions -- at the first
    session of another suite (cycle: session 1; odd_mid: session 150, behind
    150 sessions it visited), or at a session that holds two SSRCs (multi:
    one suite, session 1; the multi-SSRC planner then takes the batch,
    msplans + 1) -- waits for its ticket and exits.  batch_async completes
    such a call synchronously; the sessions the gather had visited must not
    stay marked as pending behind a sequence number the thread never
    completes.  The main thread then calls srtp_encrypt_batch_dev (one
    session, no session array), srtp_encrypt and srtp_stream_export on
    session 0, on the session in front of the declining one and on the
    declining one: 0 and the oracle's bytes, not EBUSY"""
    torch = torch_cuda
    if case == "multi":
        sc = M.multi_scenario(1)
        pre, st, nxt = sc.steps
        at = 1
    else:
        sc = M.rtp_scenario(case)
        pre, st, nxt = None, sc.steps[0], sc.steps[2]
        at = 1 if case == "cycle" else M.ODD_AT[case]
    prod = Prod(torch, sc, "async")
    got = {}
    try:
        if pre:
            same_rows((case, "pre"), pre, prod.run(pre, "dev"), sc.suites)

        def worker():
            c0 = counters()
            t, held = issue_async(torch, prod, st, got, "w")
            wait_async(torch, st, got, "w", t, held)
            got["w_moved"] = moved(c0)

        th = threading.Thread(target=worker)
        th.start()
        th.join(WAIT)
        assert not th.is_alive()
        assert (got["w_issue"], got["w_wait"]) == (0, 0)
        same_rows((case, "async"), st, got["w_rows"], sc.suites)
        assert got["w_moved"] == ({"msplans": 1} if case == "multi" else {})
        for s in sorted({0, at - 1, at}):
            tag = "s%d" % s
            want = one_session_calls(torch, prod, nxt, s, tag, got)
            free_and_right(got, tag, want)
    finally:
        prod.close()


def declined_behind_a_pending_one(torch_cuda):
    """the worker does not exit: it has a one-session call pending on another
    context when it issues the mixed call.  While that earlier call is
    pending its session is busy for the main thread (EBUSY, nothing changed);
    the declined mixed call completes it on the way (tk_drain) and runs
    synchronously, after which no session of either call is busy, before the
    tickets are waited for and after"""
    torch = torch_cuda
    sc = M.rtp_scenario("cycle")
    one = M.multi_scenario(1)       # session 0 of it: one stream, in order
    st, nxt = sc.steps[0], sc.steps[2]
    prod, first = Prod(torch, sc, "async"), Prod(torch, one, "async")
    pk = [[(0, p) for s, p in b.pkts if s == 0] for b in one.steps]
    rows = [[r for (s, _), r in zip(b.pkts, b.rows) if s == 0]
            for b in one.steps]
    got, ev = {}, {k: threading.Event() for k in
                   ("issued1", "checked1", "issued2", "checked2", "waited")}

    def dev_of(pkts):
        arena, pos, end, cap, _ = to_arena(pkts)
        return Dev(torch, arena, pos, end, cap, None), pos

    def worker():
        try:
            d1, pos1 = dev_of(pk[0])
            torch.cuda.synchronize()
            rc, t1, keep = P.device_batch_dev_async(
                "srtp_encrypt", [first.ctx[0]], *d1.args())
            got["w1_issue"] = rc
            ev["issued1"].set()
            assert ev["checked1"].wait(WAIT)
            t2, held = issue_async(torch, prod, st, got, "w2")
            ev["issued2"].set()
            assert ev["checked2"].wait(WAIT)
            got["w1_wait"] = P.batch_wait(t1)
            wait_async(torch, st, got, "w2", t2, held)
            torch.cuda.synchronize()
            a, p, e, err = d1.out()
            got["w1_rows"] = [(int(err[i]), a[int(pos1[i]):int(e[i])]
                               .tobytes()) for i in range(len(pk[0]))]
        finally:
            for e in ev.values():       # (a failure here: nobody waits)
                e.set()

    def main_on_first(tag, batch):
        d, pos = dev_of(pk[batch][:1])
        torch.cuda.synchronize()
        got[tag] = P.device_batch_dev("srtp_encrypt", [first.ctx[0]],
                                      *d.args())
        torch.cuda.synchronize()
        a, p, e, err = d.out()
        got[tag + "_row"] = (int(err[0]), a[int(pos[0]):int(e[0])].tobytes())

    th = threading.Thread(target=worker)
    try:
        th.start()
        assert ev["issued1"].wait(WAIT) and got["w1_issue"] == 0
        # the earlier call is pending: its session is busy, nothing changes
        main_on_first("busy", 1)
        ev["checked1"].set()
        assert ev["issued2"].wait(WAIT)
        assert got["busy"] == P.EBUSY and got["busy_row"][0] == -1
        # the mixed call ran synchronously and completed the earlier one
        assert got["w2_issue"] == 0
        want = one_session_calls(torch, prod, nxt, 0, "mid0", got)
        free_and_right(got, "mid0", want)
        main_on_first("mid", 1)
        ev["checked2"].set()
        assert ev["waited"].wait(WAIT)
        th.join(WAIT)
        assert not th.is_alive()
        assert (got["w1_wait"], got["w2_wait"]) == (0, 0)
        same_rows("behind", st, got["w2_rows"], sc.suites)
        assert got["w1_rows"] == [(0, r[3][:r[2]]) for r in rows[0]]
        r = rows[1][0]
        assert (got["mid"], got["mid_row"]) == (0, (0, r[3][:r[2]]))
        want = one_session_calls(torch, prod, nxt, 1, "end1", got)
        free_and_right(got, "end1", want)
        main_on_first("end", 2)
        # (the session's second packet of batch 1 was never sent: batch 2's
        # first packet follows with a gap, which a sender does not mind)
        r = rows[2][0]
        assert (got["end"], got["end_row"]) == (0, (0, r[3][:r[2]]))
    finally:
        for e in ev.values():
            e.set()
        th.join(WAIT)
        prod.close()
        first.close()
