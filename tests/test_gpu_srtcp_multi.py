"""SRTCP batches beyond one session and one SSRC, and RTP and SRTCP on the
same contexts (rtcp-mux), against the oracle called one packet at a time in
batch order (srtcp_encrypt srtcp.c:31-140, srtcp_decrypt srtcp.c:143-287,
stream_get stream.c:29-84, srtp_replay_check replay.c:32-62).

srtcp_*_batch_dev plans a batch on the device only for one session without a
session array and at most one stream (batch_async.c run_dev).  Everything
here goes the other ways: dev_staged and run_batch_general with plan_rtcp_enc
/ plan_rtcp_dec per packet (srtp.c), the speculate / undo / re-run rounds,
the general kernels with per-packet keys, the single-stream planner rejecting
an SSRC it does not know (SPF_SSRC), and the RTP planners meeting streams
that SRTCP created (s_l_set == 0) or that live in the resident copies.

A scenario (scn_*) is a traffic generator written against a drive: it calls
drive.step(side, op, packets) and gets the oracle's rows back, from which it
builds the next batch (the receiver's batch is what the oracle's sender
made).  OracleDrive runs the oracle twins alone (tests/test_srtcp_multi_cpu.py
checks the generators there); PairDrive hands every batch to product contexts
too and compares, after every batch, per packet (errno, pos, end, bytes up to
max(end, input length)) and per (session, SSRC) the exported SRTCP state
(rtcp_index, window) and RTP state (roc, s_l, window).  A case ends with one
packet of an unused SSRC to every session: 0 while the table has room, ENOSR
when it is full.  Every scenario asserts on the oracle's rows that the errno
classes it is meant to produce occur.

Short capacity: a device arena cannot grow the way mbuf_write_mem does, so
a protect whose trailer would not fit in cap fails with ENOMEM right after
the stream lookup (srtp.c cap_short, the batch extension's documented
deviation; the mbuf entry grows like the reference).  The twin states that
rule where the arena is fixed: the lookup (which may take a slot, or give
ENOSR), then ENOMEM with pos past the header and nothing else changed.
"""
import collections
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import oracle_lib as O
from tests.test_gpu_fastpath import keys_for, rtp_packet, to_arena
from tests.test_gpu_fastpath import run_dev as run_dev_arrays
from tests.test_gpu_srtcp import rtcp_packet
from tests.test_gpu_srtcp_replay import _suites, has_hmac

pytestmark = pytest.mark.gpu

U = P.SRTP_UNENCRYPTED_SRTCP
ENOSR, ENOMEM, EBADMSG, EALREADY = (errno.ENOSR, errno.ENOMEM, errno.EBADMSG,
                                    errno.EALREADY)
ROOM = 60                       # to_arena's cap - end
UNUSED = 0x7E57AB1E
RTCP_OPS = ("srtcp_encrypt", "srtcp_decrypt")


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


def trailer(suite):
    """bytes srtcp_encrypt appends: E || index and the tag"""
    return 4 + P.tag_len(suite)


def ssrc_of(s, k):
    return 0x51000000 | (s << 8) | k


def ssrc_in(op, p):
    at = 4 if op in RTCP_OPS else 8
    return int.from_bytes(p[at:at + 4], "big") if len(p) >= at + 4 else None


# ---- the oracle twins ------------------------------------------------------

class Twin:
    """oracle contexts of nsess sessions, called one packet at a time"""

    def __init__(self, suite, flags):
        self.ob = O.OracleBackend()
        self.suite = suite
        self.keys = keys_for(suite, len(flags))
        self.ctx = [self.ob.alloc(suite, k, f)[0]
                    for k, f in zip(self.keys, flags)]

    def close(self):
        for c in self.ctx:
            self.ob.free(c)

    def run(self, op, pkts, rooms, fixed):
        rows = []
        for (s, p), room in zip(pkts, rooms):
            c = self.ctx[s]
            if fixed and op == "srtcp_encrypt" and len(p) >= 8 and \
                    room < trailer(self.suite):
                # the arena cannot grow (module docstring)
                x = ssrc_in(op, p)
                e = self.ob.rtcp_set(c, x, *(self.ob.rtcp_state(c, x) or
                                             (0, 0, 0)))
                rows.append((e or ENOMEM, 8, len(p), p))
                continue
            e, po, en, _, buf = self.ob.call(c, op, len(p) + room, 0, len(p),
                                             p, len(p))
            rows.append((e, po, en, buf[:max(en, len(p))]))
        return rows

    def state(self, s, ssrc):
        r = self.ob.rtcp_state(self.ctx[s], ssrc)
        return None if r is None else (r, self.ob.export(self.ctx[s], ssrc))


class OracleDrive:
    """the twins alone.  flags: one value, or {"tx": [...], "rx": [...]}
    per session; fixed: the packets lie in an arena that cannot grow"""

    def __init__(self, suite, flags, nsess, fixed=True):
        if not isinstance(flags, dict):
            flags = {"tx": [flags] * nsess, "rx": [flags] * nsess}
        self.suite, self.flags, self.nsess = suite, flags, nsess
        self.fixed = fixed
        self.twin = {k: Twin(suite, flags[k]) for k in ("tx", "rx")}
        self.seen = {"tx": set(), "rx": set()}
        self.errs = {"tx": collections.Counter(),
                     "rx": collections.Counter()}
        self.log = []

    def close(self):
        for t in self.twin.values():
            t.close()

    def step(self, side, op, pkts, rooms=None, what=None, expect=None):
        """one batch [(session, bytes)] through side's contexts; rooms: cap
        - end per packet; expect: counter deltas of the device entry.
        Returns the oracle's rows [(errno, pos, end, bytes)]."""
        assert 0 < len(pkts) <= 600
        rooms = [ROOM] * len(pkts) if rooms is None else list(rooms)
        rows = self.twin[side].run(op, pkts, rooms, self.fixed)
        for s, p in pkts:
            x = ssrc_in(op, p)
            if x is not None:
                self.seen[side].add((s, x))
        if op in RTCP_OPS:
            self.errs[side].update(r[0] for r in rows)
        self.log.append((side, op, list(pkts), rooms, rows))
        return rows

    def set_rtcp(self, side, s, ssrc, rtcp_index, lix, bitmap):
        t = self.twin[side]
        assert t.ob.rtcp_set(t.ctx[s], ssrc, rtcp_index, lix, bitmap) == 0
        self.seen[side].add((s, ssrc))

    def require(self, side, codes):
        """the coverage guard: the oracle gave each of codes on side"""
        got = {e for e, n in self.errs[side].items() if n}
        assert set(codes) <= got, (side, sorted(codes), sorted(got))

    def finish(self):
        """one packet of an unused SSRC to every session, both sides"""
        rng = np.random.default_rng(99)
        plain = [(s, rtcp_packet(rng, UNUSED, 24)) for s in range(self.nsess)]
        rows = self.step("tx", "srtcp_encrypt", plain, what="probe")
        assert {r[0] for r in rows} <= {0, ENOSR}
        snd = Twin(self.suite, self.flags["tx"])
        wire = [(s, r[3][:r[2]]) for (s, _), r in
                zip(plain, snd.run("srtcp_encrypt", plain,
                                   [ROOM] * len(plain), False))]
        snd.close()
        rows = self.step("rx", "srtcp_decrypt", wire, what="probe")
        assert {r[0] for r in rows} <= {0, ENOSR}, [r[0] for r in rows]
        return self.log


# ---- the product beside them -----------------------------------------------

COUNTERS = ("rplans", "rejects", "mplans", "fused", "lplans", "dplans",
            "folds")


class Prod:
    """product contexts through one entry point: "dev" srtcp_*_batch_dev /
    srtp_*_batch_dev with a device session array, "dev1" the same without
    one (one session), "host" srtcp_*_batch (host arrays), "mbufs" """

    def __init__(self, torch, suite, flags, entry):
        self.torch, self.entry = torch, entry
        self.ctx = [P.Srtp(suite, k, f)
                    for k, f in zip(keys_for(suite, len(flags)), flags)]
        assert entry == "dev" or entry == "host" or len(self.ctx) == 1

    def close(self):
        for c in self.ctx:
            c.close()

    def run(self, op, pkts, rooms):
        if self.entry == "mbufs":
            return self.mbufs(op, pkts, rooms)
        arena, pos, end, cap, sess = to_arena(pkts)
        cap = (end + np.array(rooms, dtype=np.uint32)).astype(np.uint32)
        if self.entry == "host":
            dev = self.torch.from_numpy(arena).cuda()
            p, e = pos.copy(), end.copy()
            self.torch.cuda.synchronize()
            rc, err = P.device_batch(op, self.ctx, dev.data_ptr(),
                                     arena.nbytes, p, e, cap,
                                     sess if len(self.ctx) > 1 else None)
            assert rc == 0, (rc, P.lib().srtp_gpu_error())
            a = dev.cpu().numpy()
        else:
            a, p, e, err = run_dev_arrays(
                self.torch, op, self.ctx, arena, pos, end, cap,
                sess if self.entry == "dev" else None)
        out = []
        for i, (_, q) in enumerate(pkts):
            b, n = int(pos[i]), int(e[i]) - int(pos[i])
            out.append((int(err[i]), int(p[i]) - b, n,
                        a[b:b + max(n, len(q))].tobytes()))
        return out

    def mbufs(self, op, pkts, rooms):
        mbs = [P.new_mbuf(p, len(p) + r) for (_, p), r in zip(pkts, rooms)]
        rc, errs = P.batch_run(self.ctx[0], op, mbs)
        assert rc == 0, (rc, P.lib().srtp_gpu_error())
        out = [(int(errs[i]), int(m.contents.pos), int(m.contents.end),
                P.mbuf_bytes(m, max(int(m.contents.end), len(pkts[i][1]))))
               for i, m in enumerate(mbs)]
        for m in mbs:
            P.free_mbuf(m)
        return out

    def state(self, s, ssrc):
        e, st = self.ctx[s].export(ssrc)
        if e:
            return None
        return ((st.rtcp_index, st.replay_rtcp_lix, st.replay_rtcp_bitmap),
                (st.roc, st.s_l, st.replay_rtp_lix, st.replay_rtp_bitmap))


class PairDrive(OracleDrive):
    """product contexts and oracle twins fed the same batches"""

    def __init__(self, torch, suite, flags, nsess, entry):
        super().__init__(suite, flags, nsess, fixed=entry != "mbufs")
        self.entry = entry
        self.prod = {k: Prod(torch, suite, self.flags[k], entry)
                     for k in ("tx", "rx")}

    def close(self):
        super().close()
        for p in self.prod.values():
            p.close()

    def step(self, side, op, pkts, rooms=None, what=None, expect=None):
        rows = super().step(side, op, pkts, rooms, what, expect)
        what = (what, side, op, self.entry)
        # (every call from the same first-batch hint, tests/test_gpu_fused.py)
        P.lib().srtp_gpu_tune(b"freshmulti", 0)
        c0 = {c: P.counter(c) for c in COUNTERS}
        got = self.prod[side].run(op, pkts, self.log[-1][3])
        dc = {c: P.counter(c) - c0[c] for c in COUNTERS}
        ge, we = [g[0] for g in got], [r[0] for r in rows]
        assert ge == we, (what, [(i, g, w) for i, (g, w)
                                 in enumerate(zip(ge, we)) if g != w][:8])
        for i, (g, w) in enumerate(zip(got, rows)):
            assert g[:3] == w[:3], (what, i, g[:3], w[:3])
            assert g[3] == w[3], (what, i, "bytes", g[:3])
        self.same_states(side, what)
        if expect and self.entry in ("dev", "dev1"):
            assert {c: dc[c] for c in expect} == expect, (what, dc)
        return rows

    def same_states(self, side, what):
        for s, x in sorted(self.seen[side]):
            g, w = self.prod[side].state(s, x), self.twin[side].state(s, x)
            assert g == w, (what, "state", s, hex(x), g, w)

    def set_rtcp(self, side, s, ssrc, rtcp_index, lix, bitmap):
        super().set_rtcp(side, s, ssrc, rtcp_index, lix, bitmap)
        st = P.StreamState()
        st.ssrc, st.rtcp_index = ssrc, rtcp_index
        st.replay_rtcp_lix, st.replay_rtcp_bitmap = lix, bitmap
        assert self.prod[side].ctx[s].import_(st) == 0
        self.same_states(side, "import")


def wire_of(pkts, rows):
    """what a sender's batch puts on the wire: every packet as it was left,
    a refused one (still plain) included"""
    return [(s, r[3][:r[2]]) for (s, _), r in zip(pkts, rows)]


# ---- 1. round trip, state carried over ------------------------------------

def scn_round_trip(d, seed, n=600, big=True):
    """every session with 1..8 SSRCs (session 0: 8, session 1: 1), packets
    interleaved at random, bodies of 4 * k bytes (k in 0..80), two packets
    of 4028 and 4100 bytes in the first batch (either side of
    SGPU_CACHED_MAX), twelve packets per batch with room for the trailer
    exactly or one byte less; protect then unprotect, twice"""
    rng = np.random.default_rng(seed)
    nss = [8, 1][:d.nsess] + (1 + rng.permutation(max(d.nsess - 2, 0)) %
                              8).tolist()
    need = trailer(d.suite)
    for b in range(2):
        # every stream once, the rest drawn
        who = [(s, k) for s in range(d.nsess) for k in range(nss[s])][:n]
        who += [(s, int(rng.integers(0, nss[s])))
                for s in rng.integers(0, d.nsess, n - len(who)).tolist()]
        pk = [(s, rtcp_packet(rng, ssrc_of(s, k), 4 * int(rng.integers(
            0, 81)))) for s, k in (who[i] for i in rng.permutation(n))]
        if big and b == 0:
            for at, size in ((n // 3, 4028), (n // 2, 4100)):
                s = pk[at][0]
                pk[at] = (s, rtcp_packet(rng, ssrc_of(s, 0), size - 8))
        rooms = [ROOM] * n
        for k, i in enumerate(rng.choice(n, 12, replace=False).tolist()):
            rooms[i] = need - k % 2
        rows = d.step("tx", "srtcp_encrypt", pk, rooms, ("round trip", b))
        d.step("rx", "srtcp_decrypt", wire_of(pk, rows),
               what=("round trip", b))
    d.require("tx", {0, ENOMEM} if d.fixed else {0})
    # a refused packet arrives plain: no tag, or one that cannot match
    d.require("rx", {0, P.EAUTH} if d.fixed and has_hmac(d.suite) else {0})
    return d.finish()


# ---- 2. unprotect with trouble inside one batch ---------------------------

KINDS = ("tag", "body", "index", "ebit", "forged_first", "forged_last",
         "dup", "repeat", "short8", "short_trailer")
NTROUBLE = 16


def trouble_flags(flags):
    """sessions 2 and 3: a sender whose E bit disagrees with the receiver"""
    return {"tx": [flags ^ U if s in (2, 3) else flags
                   for s in range(NTROUBLE)], "rx": [flags] * NTROUBLE}


def flipped(p, at, bit=0x10):
    q = bytearray(p)
    q[at] ^= bit
    return bytes(q)


def scn_trouble(d, seed):
    """batch 1: 16 sessions, every stream's first packets, clean (session
    0's first stream long enough to leave its third packet, held back, 64
    indices behind); session 1 has 8 streams, session 5 has 7.  Batch 2: 25
    packets per session, of which one each, at places drawn per session,
    has a bit flipped in the tag, the body, the index or the E bit, comes
    behind or ahead of a forged copy, comes twice, comes behind a packet of
    batch 1, or is cut below 8 bytes or below header + index + tag; then
    the held-back packet, GCM packets with fewer than 16 bytes before the
    index word, forged packets of new SSRCs (they take a slot: session 5 is
    full after its one) and a 9th SSRC for sessions 1 and 5 with more of
    those sessions' own traffic behind it"""
    hm, suite = has_hmac(d.suite), d.suite
    T = P.tag_len(suite) if hm else 0           # bytes behind E || index
    rng = np.random.default_rng(seed)
    nss = [int(rng.integers(1, 7)) for _ in range(NTROUBLE)]
    nss[0], nss[1], nss[5] = 2, 8, 7
    # batch 1
    pk = [(s, rtcp_packet(rng, ssrc_of(s, k), 4 * int(rng.integers(1, 30))))
          for s in range(NTROUBLE) for k in range(nss[s]) for _ in range(3)]
    pk = [pk[i] for i in rng.permutation(len(pk)).tolist()]
    pk += [(0, rtcp_packet(rng, ssrc_of(0, 0), 4 * int(rng.integers(1, 30))))
           for _ in range(80)]
    rows = d.step("tx", "srtcp_encrypt", pk, what=("trouble", 1))
    assert not any(r[0] for r in rows)
    wire1 = wire_of(pk, rows)
    held = [i for i, (s, p) in enumerate(wire1)
            if ssrc_in("srtcp_decrypt", p) == ssrc_of(0, 0)][2]
    old = wire1[held]
    arr1 = wire1[:held] + wire1[held + 1:]
    rows = d.step("rx", "srtcp_decrypt", arr1, what=("trouble", 1))
    assert not any(r[0] for r in rows)
    # batch 2
    pk, kind = [], []
    for s in range(NTROUBLE):
        rs = np.random.default_rng(1000 * seed + s)
        at = rs.choice(25, len(KINDS), replace=False).tolist()
        for j in range(25):
            pk.append((s, rtcp_packet(rs, ssrc_of(s, int(rs.integers(
                0, nss[s]))), 4 * int(rs.integers(1, 81)))))
            kind.append(KINDS[at.index(j)] if j in at else None)
    order = rng.permutation(len(pk)).tolist()
    pk, kind = [pk[i] for i in order], [kind[i] for i in order]
    rows = d.step("tx", "srtcp_encrypt", pk, what=("trouble", 2))
    assert not any(r[0] for r in rows)
    wire2 = wire_of(pk, rows)
    arr, later, pairs = [], [], []
    for i, ((s, w), k) in enumerate(zip(wire2, kind)):
        tag_at = len(w) - 1 if hm else len(w) - 5
        forged = (s, flipped(w, tag_at, 0x40))
        if k == "tag":
            arr.append(forged)
        elif k == "body":
            arr.append((s, flipped(w, 8 + (len(w) - 8 - trailer(suite)) // 2)))
        elif k == "index":
            arr.append((s, flipped(w, len(w) - T - 1, 0x02)))
        elif k == "ebit":
            arr.append((s, flipped(w, len(w) - T - 4, 0x80)))
        elif k == "forged_first":
            arr += [forged, (s, w)]
            pairs.append((forged, (s, w)))
        elif k == "forged_last":
            arr += [(s, w), forged]
        elif k == "dup":
            arr.append((s, w))
            later.append((len(arr) + int(rng.integers(1, 40)), (s, w)))
        elif k == "repeat":
            mine = [q for q in arr1 if q[0] == s]
            arr += [mine[int(rng.integers(0, len(mine)))], (s, w)]
        elif k == "short8":
            arr.append((s, w[:(1, 4, 7)[i % 3]]))
        elif k == "short_trailer":
            arr.append((s, w[:(8, 9, 8 + trailer(suite) - 1)[i % 3]]))
        else:
            arr.append((s, w))
    for at, q in sorted(later, reverse=True):
        arr.insert(min(at, len(arr)), q)
    arr.append(old)
    if not hm:
        w = wire2[0][1]
        arr += [(wire2[0][0], w[:8 + k] + w[-4:]) for k in (0, 15)]
    # forged packets of new SSRCs, a 9th SSRC, the sessions' own traffic on
    tail = [(s, rtcp_packet(rng, ssrc_of(s, 0x40), 40) +
             rng.integers(0, 256, trailer(suite), dtype=np.uint8).tobytes())
            for s in (5, 6)]
    ninth = [(s, rtcp_packet(rng, ssrc_of(s, 0x50), 32)) for s in (1, 5)]
    more = [(s, rtcp_packet(rng, ssrc_of(s, k), 4 * int(rng.integers(1, 20))))
            for s in (1, 5) for k in (0, nss[s] - 1)]
    # the sender of session 5 has a slot left for the new SSRC, the
    # receiver has not: its forged packet took it
    rows = d.step("tx", "srtcp_encrypt", ninth + more, what=("trouble", 3))
    assert [r[0] for r in rows] == [ENOSR, 0] + [0] * len(more)
    arr += tail + wire_of(ninth + more, rows)
    rows = d.step("rx", "srtcp_decrypt", arr, what=("trouble", 2))
    # the genuine packet behind its forged copy is accepted
    assert len(pairs) == NTROUBLE
    for forged, genuine in pairs:
        i, j = arr.index(forged), arr.index(genuine)
        assert i < j and (rows[i][0], rows[j][0]) == (P.EAUTH, 0), (i, j)
    assert [r[0] for r in rows[-len(more):]] == [0] * len(more)
    assert [r[0] for r in rows[-len(more) - 2:-len(more)]] == [ENOSR, ENOSR]
    assert [r[1] for r in rows[-len(more) - 2:-len(more)]] == [8, 8]
    d.require("tx", {0, ENOSR})
    d.require("rx", {0, P.EAUTH, ENOSR, EBADMSG} |
              ({EALREADY} if hm else set()))
    return d.finish()


# ---- 3. the stream the planner does not know -------------------------------

A, B, C = 0x0A0A0001, 0x0B0B0002, 0x0C0C0003
FULL = (1 << 64) - 1


def pkts_of(rng, ssrcs, n):
    return [(0, rtcp_packet(rng, ssrcs[i % len(ssrcs)],
                            4 * int(rng.integers(0, 65)))) for i in range(n)]


def scn_unknown_stream(d, seed, which):
    """one session: (a) a sender whose only stream is A at index 500
    protects a batch of B alone, (b) the receiver of that batch has A's
    window seeded, (c) a context with streams [A, B] gets A alone, (d) a
    fresh context gets A and B in turn"""
    rng = np.random.default_rng(seed)
    if which == "ab":
        d.set_rtcp("tx", 0, A, 500, 0, 0)
        d.set_rtcp("rx", 0, A, 0, 500, FULL)
        pk = pkts_of(rng, [B], 30)
        rows = d.step("tx", "srtcp_encrypt", pk, what="a",
                      expect={"rplans": 0, "rejects": 1})
        assert d.twin["tx"].state(0, A)[0][0] == 500
        assert d.twin["tx"].state(0, B)[0][0] == 30
        d.step("rx", "srtcp_decrypt", wire_of(pk, rows), what="b",
               expect={"rplans": 0})
        assert d.twin["rx"].state(0, A)[0][1:] == (500, FULL)
        if has_hmac(d.suite):
            assert d.twin["rx"].state(0, B)[0][1:] == (30, (1 << 30) - 1)
    elif which == "c":
        for x in (A, B):
            d.set_rtcp("tx", 0, x, 7, 0, 0)
            d.set_rtcp("rx", 0, x, 0, 7, 0x7f)
        pk = pkts_of(rng, [A], 30)
        rows = d.step("tx", "srtcp_encrypt", pk, what="c",
                      expect={"rplans": 0})
        d.step("rx", "srtcp_decrypt", wire_of(pk, rows), what="c",
               expect={"rplans": 0})
    else:
        pk = pkts_of(rng, [A, B], 40)
        rows = d.step("tx", "srtcp_encrypt", pk, what="d")
        d.step("rx", "srtcp_decrypt", wire_of(pk, rows), what="d")
    d.require("tx", {0})
    d.require("rx", {0})
    return d.finish()


# ---- 4. per-stream 31-bit index wrap ---------------------------------------

def scn_wrap(d, seed):
    """a sender with three SSRCs, B taken up at rtcp_index 0x7ffffff0 (and
    the receiver's window of B at that index): 40 packets, 20 of them B's,
    so B wraps and A and C do not"""
    rng = np.random.default_rng(seed)
    d.set_rtcp("tx", 0, B, 0x7ffffff0, 0, 0)
    d.set_rtcp("rx", 0, B, 0, 0x7ffffff0, 1)
    who = [A] * 10 + [B] * 20 + [C] * 10
    who = [who[i] for i in rng.permutation(40).tolist()]
    pk = [(0, rtcp_packet(rng, x, 4 * int(rng.integers(0, 65)))) for x in who]
    rows = d.step("tx", "srtcp_encrypt", pk, what="wrap")
    assert not any(r[0] for r in rows)
    t = d.twin["tx"]
    assert [t.state(0, x)[0][0] for x in (A, B, C)] == [10, 4, 10]
    rows = d.step("rx", "srtcp_decrypt", wire_of(pk, rows), what="wrap")
    d.require("rx", {0, EALREADY} if has_hmac(d.suite) else {0})
    return d.finish()


# ---- 5. RTP and SRTCP on the same contexts ---------------------------------

NMUX = 24


def rtp_batch(rng, nxt, n, ssrc):
    out = []
    for _ in range(n):
        s = int(rng.integers(0, len(nxt)))
        out.append((s, rtp_packet(rng, nxt[s] & 0xffff, ssrc(s),
                                  plen=int(rng.integers(0, 300)))))
        nxt[s] += 1
    return out


def scn_mux(d, seed):
    """24 sessions: RTP (in order, the many-session planner), SRTCP over
    the same sessions -- two thirds on the RTP SSRC, one third on a new one
    -- RTP, SRTCP, RTP with one forged packet; both directions"""
    rng = np.random.default_rng(seed)
    nxt = [65400 + 7 * s for s in range(NMUX)]
    rtp_ssrc = lambda s: 0x7000 + s
    rtcp_ssrc = lambda s: 0x9000 + s if s % 3 == 2 else 0x7000 + s
    for b in range(5):
        if b % 2 == 0:
            pk = rtp_batch(rng, nxt, 500, rtp_ssrc)
            exp = {"mplans": 1} if b == 0 else None
            rows = d.step("tx", "srtp_encrypt", pk, what=("mux", b),
                          expect=exp)
            assert not any(r[0] for r in rows)
            w = wire_of(pk, rows)
            if b == 4:
                w[77] = (w[77][0], flipped(w[77][1], len(w[77][1]) - 1, 1))
            rows = d.step("rx", "srtp_decrypt", w, what=("mux", b),
                          expect=exp)
            assert [i for i, r in enumerate(rows) if r[0]] == \
                ([77] if b == 4 else [])
        else:
            pk = [(s, rtcp_packet(rng, rtcp_ssrc(s),
                                  4 * int(rng.integers(0, 81))))
                  for s in rng.integers(0, NMUX, 200).tolist()]
            rows = d.step("tx", "srtcp_encrypt", pk, what=("mux", b))
            rows = d.step("rx", "srtcp_decrypt", wire_of(pk, rows),
                          what=("mux", b))
            assert not any(r[0] for r in rows)
    for side in ("tx", "rx"):
        assert len(d.seen[side]) == NMUX + NMUX // 3
    d.require("tx", {0})
    d.require("rx", {0})
    return d.finish()


# ---- 6. SRTCP first ---------------------------------------------------------

def scn_srtcp_first(d, seed, other, counter=None):
    """fresh contexts get an SRTCP batch and then RTP in order from just
    below 65536 (the ROC rolls over inside): the stream exists with s_l
    unset, and the first RTP seq becomes s_l (stream.c:87-109; from s_l = 0
    the first index would be guessed a ROC too low).  other: SRTCP on
    another SSRC than RTP's; counter: the counter the RTP batch's accepted
    plan moves"""
    rng = np.random.default_rng(seed)
    n = d.nsess
    nxt = [65400] if n == 1 else [65530 + s % 4 for s in range(n)]
    rtp_ssrc = lambda s: 0x7000 + s
    pk = [(s, rtcp_packet(rng, 0x9000 + s if other else rtp_ssrc(s),
                          4 * int(rng.integers(0, 65))))
          for s in rng.permutation(np.arange(20 * n) % n).tolist()]
    rows = d.step("tx", "srtcp_encrypt", pk, what="first, srtcp")
    rows = d.step("rx", "srtcp_decrypt", wire_of(pk, rows),
                  what="first, srtcp")
    assert not any(r[0] for r in rows)
    exp = {counter: 1, "rejects": 0} if counter else None
    pk = rtp_batch(rng, nxt, 300 if n == 1 else 600, rtp_ssrc)
    rows = d.step("tx", "srtp_encrypt", pk, what="first, rtp", expect=exp)
    rows = d.step("rx", "srtp_decrypt", wire_of(pk, rows), what="first, rtp",
                  expect=exp)
    assert not any(r[0] for r in rows)
    for side in ("tx", "rx"):
        for s in range(n):
            assert d.twin[side].state(s, rtp_ssrc(s))[1][:2] == \
                (1, (nxt[s] - 1) & 0xffff), (side, s)
    d.require("tx", {0})
    d.require("rx", {0})
    return d.finish()


# ---- the GPU cases ----------------------------------------------------------

SUB = _suites()
sub_ids = ["s%d%s" % (s, "u" if f else "") for s, f in SUB]
MUX_SUITES = [1, 5]             # one AES-CM suite, one GCM suite


def drive(torch, scn, suite, flags, nsess, entry, *args, **kw):
    d = PairDrive(torch, suite, flags, nsess, entry)
    try:
        return scn(d, *args, **kw)
    finally:
        d.close()


@pytest.mark.parametrize("flags", [0, U], ids=["e", "u"])
@pytest.mark.parametrize("suite", list(range(6)))
def test_round_trip_many_sessions(torch_cuda, suite, flags):
    """case 1 through srtcp_*_batch_dev with a device session array"""
    drive(torch_cuda, scn_round_trip, suite, flags, 40, "dev",
          110 + 2 * suite + flags)


@pytest.mark.parametrize("case", SUB, ids=sub_ids)
def test_round_trip_host_arrays(torch_cuda, case):
    suite, flags = case
    drive(torch_cuda, scn_round_trip, suite, flags, 40, "host",
          130 + 2 * suite + flags)


@pytest.mark.parametrize("entry", ["mbufs", "dev1"])
@pytest.mark.parametrize("case", SUB, ids=sub_ids)
def test_round_trip_one_session_eight_ssrcs(torch_cuda, case, entry):
    """one context, 8 SSRCs: srtcp_*_mbufs (the mbufs grow like the
    reference's), and the device entry without a session array"""
    suite, flags = case
    drive(torch_cuda, scn_round_trip, suite, flags, 1, entry,
          150 + 2 * suite + flags, n=300)


@pytest.mark.parametrize("entry", ["dev", "host"])
@pytest.mark.parametrize("case", SUB, ids=sub_ids)
def test_unprotect_trouble(torch_cuda, case, entry):
    """case 2"""
    suite, flags = case
    drive(torch_cuda, scn_trouble, suite, trouble_flags(flags), NTROUBLE,
          entry, 170 + 2 * suite + flags)


@pytest.mark.parametrize("sep", [0, 1])
@pytest.mark.parametrize("which", ["ab", "c", "d"])
@pytest.mark.parametrize("case", SUB, ids=sub_ids)
def test_stream_the_planner_does_not_know(torch_cuda, case, which, sep):
    """case 3, with the one-launch plan and the separate planner launches"""
    suite, flags = case
    with P.tune(noplanfuse=sep):
        drive(torch_cuda, scn_unknown_stream, suite, flags, 1, "dev1",
              190 + 2 * suite + flags, which)


@pytest.mark.parametrize("entry", ["dev1", "dev", "host", "mbufs"])
@pytest.mark.parametrize("case", SUB, ids=sub_ids)
def test_index_wrap_per_stream(torch_cuda, case, entry):
    """case 4"""
    suite, flags = case
    drive(torch_cuda, scn_wrap, suite, flags, 1, entry,
          210 + 2 * suite + flags)


@pytest.mark.parametrize("suite", MUX_SUITES)
def test_rtp_and_srtcp_share_contexts(torch_cuda, suite):
    """case 5"""
    drive(torch_cuda, scn_mux, suite, 0, NMUX, "dev", 230 + suite)


@pytest.mark.parametrize("shape", ["same", "other", "many"])
@pytest.mark.parametrize("suite", MUX_SUITES)
def test_srtcp_first_then_rtp(torch_cuda, suite, shape):
    """case 6: one session and the RTP SSRC (the single-stream device
    planner takes the RTP batch), one session and another SSRC (results
    only), 24 sessions (the many-session planner)"""
    one = "lplans" if not has_hmac(suite) else "fused"
    if shape == "many":
        drive(torch_cuda, scn_srtcp_first, suite, 0, NMUX, "dev",
              250 + suite, False, "mplans")
    else:
        drive(torch_cuda, scn_srtcp_first, suite, 0, 1, "dev1", 260 + suite,
              shape == "other", None if shape == "other" else one)
