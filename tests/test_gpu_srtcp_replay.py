"""The SRTCP receiver's replay window across batches (srtcp_decrypt_batch_dev
and dev_planned_rtcp: the one-launch plan k_rp_plan, and with srtp_gpu_tune
noplanfuse k_parse + k_plan_rtcp; plan_rule.h plan_rtcp_packet; the window
rebuilt from the plan's tail, batch_host.c plan_replay) against the oracle
called one packet at a time (srtcp_decrypt srtcp.c:143-287, srtp_replay_check
replay.c:32-62).

One oracle sender makes the wire packets of indices 1..N of one SSRC.  A
case hands one arrival sequence, cut into consecutive batches, to a product
receiver and an oracle receiver; after every batch each packet's (err, pos,
end, bytes) and the exported window (replay_rtcp_lix, replay_rtcp_bitmap)
must be the oracle's.  Every case ends with a probe: each of the last 70
indices again, one packet per call, so the window is also compared by what
it accepts.

Arrivals: a late packet followed by one already seen; a repeat and a step
back across a planner workgroup seam (PLAN_BLOCK 256); a first packet at
the window's edges; batches around the plan's tail (SGPU_PLAN_TAIL 65);
the 31-bit index wrap; a forged packet above everything beside a late one;
the host-array and mbuf entry points; senders and receivers that differ in
SRTP_UNENCRYPTED_SRTCP (the E bit against the receiver's cipher).  Suites: one AES-CM suite per tag
length and key size, one GCM suite (the reference keeps no SRTCP replay
window without an HMAC, srtcp.c:180: a repeated GCM packet is whatever the
oracle makes of it), SRTP_UNENCRYPTED_SRTCP.
"""
import errno
import functools

import numpy as np
import pytest

import re_amd.srtp as P
from tests import oracle_lib as O
from tests.test_gpu_fastpath import keys_for, to_arena
from tests.test_gpu_srtcp import oracle_run, rtcp_packet, run_dev

pytestmark = pytest.mark.gpu

SSRC = 0xC0FFEE01
PROBE = 70


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    P.load()
    return torch


def _suites():
    """(suite, flags): one AES-CM suite (14-byte salt) per key size and tag
    length, the first GCM suite, SRTP_UNENCRYPTED_SRTCP on an AES-CM one"""
    cm = [s for s in P.SUITES if P.salt_len(s) == 14]
    gcm = [s for s in P.SUITES if P.salt_len(s) != 14]
    one = {}
    for s in cm:
        one.setdefault((P.key_len(s), P.tag_len(s)), s)
    assert {k for k, _ in one} == {P.key_len(s) for s in cm}
    assert {t for _, t in one} == {P.tag_len(s) for s in cm}
    unenc = max(cm, key=P.tag_len)
    return [(s, 0) for s in sorted(one.values())] + [(gcm[0], 0)] + \
        [(unenc, P.SRTP_UNENCRYPTED_SRTCP)]


CASES = _suites()
case_ids = ["s%d%s" % (s, "u" if f else "") for s, f in CASES]


def has_hmac(suite):
    return P.salt_len(suite) == 14


class Wire:
    """the oracle sender's packets: wire[ix] carries SRTCP index ix"""

    def __init__(self, suite, flags):
        self.ob = O.OracleBackend()
        self.tx = self.ob.alloc(suite, keys_for(suite, 1)[0], flags)[0]
        self.rng = np.random.default_rng(4100 + 10 * suite + flags)
        self.pk = [None]

    def upto(self, n):
        while len(self.pk) <= n:
            p = rtcp_packet(self.rng, SSRC, int(self.rng.integers(0, 65)))
            (e, _, en, buf), = oracle_run(self.ob, self.tx, "srtcp_encrypt",
                                          [p])
            assert e == 0
            self.pk.append(buf[:en])
        assert self.ob.rtcp_state(self.tx, SSRC)[0] == len(self.pk) - 1

    def __getitem__(self, ix):
        self.upto(ix)
        return self.pk[ix]


@functools.lru_cache(maxsize=None)
def wire_of(suite, flags):
    return Wire(suite, flags)


def run_host(torch, ctx, pkts):
    """srtcp_decrypt_batch: the arena on the device, the arrays on the host"""
    arena, pos, end, cap, _ = to_arena([(0, p) for p in pkts])
    dev = torch.from_numpy(arena).cuda()
    p, e = pos.copy(), end.copy()
    torch.cuda.synchronize()
    rc, err = P.device_batch("srtcp_decrypt", [ctx], dev.data_ptr(),
                             arena.nbytes, p, e, cap)
    assert rc == 0, (rc, P.lib().srtp_gpu_error())
    a = dev.cpu().numpy()
    return [(int(err[i]), int(p[i] - pos[i]), int(e[i] - pos[i]),
             a[pos[i]:pos[i] + max(int(e[i] - pos[i]), len(q))].tobytes())
            for i, q in enumerate(pkts)]


def run_mbufs(ctx, pkts):
    """srtcp_decrypt_mbufs"""
    mbs = [P.new_mbuf(p, len(p) + 64) for p in pkts]
    rc, errs = P.batch_run(ctx, "srtcp_decrypt", mbs)
    assert rc == 0, (rc, P.lib().srtp_gpu_error())
    out = [(int(errs[i]), int(m.contents.pos), int(m.contents.end),
            P.mbuf_bytes(m, max(int(m.contents.end), len(pkts[i]))))
           for i, m in enumerate(mbs)]
    for m in mbs:
        P.free_mbuf(m)
    return out


class Pair:
    """a product receiver and an oracle receiver fed the same batches"""

    def __init__(self, torch, suite, flags, entry="dev", tx_flags=None):
        """tx_flags: the sender's flags where they differ from flags"""
        key = keys_for(suite, 1)[0]
        self.torch, self.entry, self.suite = torch, entry, suite
        self.ob = O.OracleBackend()
        self.orx = self.ob.alloc(suite, key, flags)[0]
        self.rx = P.Srtp(suite, key, flags)
        self.wire = wire_of(suite, flags if tx_flags is None else tx_flags)
        self.top = 0

    def close(self):
        self.ob.free(self.orx)
        self.rx.close()

    def seed(self, lix, bitmap):
        st = P.StreamState()
        st.ssrc = SSRC
        st.replay_rtcp_lix, st.replay_rtcp_bitmap = lix, bitmap
        assert self.rx.import_(st) == 0
        assert self.ob.rtcp_set(self.orx, SSRC, 0, lix, bitmap) == 0

    def windows(self):
        e, st = self.rx.export(SSRC)
        o = self.ob.rtcp_state(self.orx, SSRC)
        return (None if e else (st.replay_rtcp_lix, st.replay_rtcp_bitmap),
                None if o is None else o[1:])

    def packets(self, pkts, what, expect=None):
        """one batch of wire packets; expect (device entry only): "plan" --
        the device plan took it (rplans +1, rejects +0), "reject" -- the
        plan was rejected (rejects +1).  Returns the oracle's errnos."""
        assert 0 < len(pkts) <= 600
        c0 = P.counter("rplans"), P.counter("rejects")
        if self.entry == "dev":
            got = run_dev(self.torch, "srtcp_decrypt", self.rx, pkts)
        elif self.entry == "host":
            got = run_host(self.torch, self.rx, pkts)
        else:
            got = run_mbufs(self.rx, pkts)
        dc = P.counter("rplans") - c0[0], P.counter("rejects") - c0[1]
        want = oracle_run(self.ob, self.orx, "srtcp_decrypt", pkts)
        ge, we = [g[0] for g in got], [w[0] for w in want]
        assert ge == we, (what, [(i, g, w) for i, (g, w)
                                 in enumerate(zip(ge, we)) if g != w][:8])
        assert got == want, what
        w = self.windows()
        assert w[0] == w[1], (what, "window", w)
        if self.entry == "dev" and expect == "plan":
            assert dc == (1, 0), (what, "expected the device plan", dc)
        if self.entry == "dev" and expect == "reject":
            assert dc == (0, 1), (what, "expected a rejected plan", dc)
        return we

    def batch(self, idxs, what, expect=None):
        self.top = max([self.top] + list(idxs))
        return self.packets([self.wire[i] for i in idxs], what, expect)

    def probe(self, what):
        """each of the last 70 indices again, one packet per call"""
        for ix in range(max(1, self.top - PROBE + 1), self.top + 1):
            self.packets([self.wire[ix]], (what, "probe", ix))


def repeats(history, idxs):
    """positions of idxs that repeat an index of history or of idxs"""
    seen, out = set(history), []
    for k, ix in enumerate(idxs):
        if ix in seen:
            out.append(k)
        seen.add(ix)
    return out


# (noplanfuse, entry point): both planners through the device entry, the
# host-array and mbuf entries once
VIA = [(0, "dev"), (1, "dev"), (0, "host"), (0, "mbufs")]
via_ids = ["%s%s" % (e, "-sep" if s else "") for s, e in VIA]

FIRST = [i for i in range(1, 101) if i not in (90, 93)]
LATE_THEN_SEEN = [
    [90, 95] + list(range(101, 111)),
    [90, 93] + list(range(101, 111)),
    [90, 93, 95],
    [90, 101, 95],
    [93, 90],
]


@pytest.mark.parametrize("via", VIA, ids=via_ids)
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_srtcp_late_then_seen(torch_cuda, case, via):
    """batch 1: indices 1..100 without 90 and 93.  Batch 2 opens with the
    late 90 (a clear bit of the window) and goes on inside the window: the
    reference says EALREADY exactly where an index repeats (with an HMAC;
    never without one)"""
    suite, flags = case
    sep, entry = via
    hm = has_hmac(suite)
    with P.tune(noplanfuse=sep):
        for b2 in LATE_THEN_SEEN:
            pr = Pair(torch_cuda, suite, flags, entry)
            e1 = pr.batch(FIRST, (b2, 1), "plan")
            assert not any(e1)
            rep = repeats(FIRST, b2)
            # (no replay window without an HMAC: nothing to reject)
            e2 = pr.batch(b2, (b2, 2),
                          "reject" if hm and rep else
                          "plan" if not hm else None)
            assert e2 == [errno.EALREADY if hm and k in rep else 0
                          for k in range(len(b2))], b2
            pr.probe(b2)
            pr.close()


SEAM = [255, 256, 257, 512]


@pytest.mark.parametrize("sep", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_srtcp_planner_workgroup_seam(torch_cuda, case, sep):
    """batch 2 is 600 packets rising from 101 with, at one position either
    side of a planner workgroup's first packet, a copy of the packet before
    it, or that packet and its predecessor swapped (a step back by one
    index not seen yet)"""
    suite, flags = case
    hm = has_hmac(suite)
    run = list(range(101, 700))
    with P.tune(noplanfuse=sep):
        for p in SEAM:
            for kind in ("copy", "back"):
                pr = Pair(torch_cuda, suite, flags)
                pr.batch(list(range(1, 101)), (p, kind, 1), "plan")
                if kind == "copy":
                    b2 = run[:p] + [run[p - 1]] + run[p:]
                    exp = "reject" if hm else "plan"
                else:
                    b2 = run[:p - 1] + [run[p], run[p - 1]] + run[p + 1:] + \
                        [700]
                    assert b2[p] == b2[p - 1] - 1
                    exp = None if hm else "plan"
                assert len(b2) == 600
                e2 = pr.batch(b2, (p, kind, 2), exp)
                assert e2 == [errno.EALREADY if hm and kind == "copy" and
                              k == p else 0 for k in range(600)]
                pr.probe((p, kind))
                pr.close()


@pytest.mark.parametrize("via", VIA, ids=via_ids)
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_srtcp_window_edges(torch_cuda, case, via):
    """batch 1: 1..100 without one index.  Batch 2 opens with that index,
    1, 62 and 63 behind lix (inside the window, bit clear: accepted), 64
    and 65 behind it (below the window), or with lix itself, and goes on in
    order"""
    suite, flags = case
    sep, entry = via
    hm = has_hmac(suite)
    with P.tune(noplanfuse=sep):
        for d in (1, 62, 63, 64, 65, 0):
            pr = Pair(torch_cuda, suite, flags, entry)
            pr.batch([i for i in range(1, 101) if d == 0 or i != 100 - d],
                     (d, 1), "plan")
            b2 = [100 - d] + list(range(101, 131))
            bad = hm and (d == 0 or d >= 64)
            e2 = pr.batch(b2, (d, 2), "reject" if bad else "plan")
            assert e2 == [errno.EALREADY if bad else 0] + [0] * 30, d
            pr.probe(d)
            pr.close()


def tail_batch(rng, m, kind):
    """the late 90, then m - 1 rising indices from 101"""
    if kind == "run":
        gaps = [1] * (m - 2)
    elif kind == "gaps":
        gaps = [int(g) for g in rng.integers(1, 71, m - 2)]
    else:                               # one gap above 64 in the last 65
        gaps = [1] * (m - 2)
        gaps[-30] = 80
    out = [90, 101]
    for g in gaps:
        out.append(out[-1] + g)
    return out


@pytest.mark.parametrize("sep", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_srtcp_window_from_plan_tail(torch_cuda, case, sep):
    """the window after an accepted plan comes from the plan's last 65
    indices (plan_replay): a late first packet and then 63, 64, 65 and 129
    rising ones, consecutive, 1..70 apart, and with one gap above 64 among
    the last 65"""
    suite, flags = case
    rng = np.random.default_rng(65 + suite)
    with P.tune(noplanfuse=sep):
        for m in (64, 65, 66, 130):
            for kind in ("run", "gaps", "biggap"):
                pr = Pair(torch_cuda, suite, flags)
                pr.batch([i for i in range(1, 101) if i != 90],
                         (m, kind, 1), "plan")
                b2 = tail_batch(rng, m, kind)
                assert len(b2) == m
                e2 = pr.batch(b2, (m, kind, 2), "plan")
                assert not any(e2)
                pr.probe((m, kind))
                pr.close()


@pytest.mark.parametrize("sep", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_srtcp_index_wrap(torch_cuda, case, sep):
    """senders at rtcp_index 0x7ffffffd protect six packets through the wrap
    to 0 (srtcp.c:54); receivers at lix 0x7ffffffc unprotect them: what the
    oracle gives for the indices behind the wrap"""
    torch = torch_cuda
    suite, flags = case
    key = keys_for(suite, 1)[0]
    rng = np.random.default_rng(7 + suite)
    ob = O.OracleBackend()
    otx = ob.alloc(suite, key, flags)[0]
    tx = P.Srtp(suite, key, flags)
    st = P.StreamState()
    st.ssrc, st.rtcp_index = SSRC, 0x7ffffffd
    assert tx.import_(st) == 0
    assert ob.rtcp_set(otx, SSRC, 0x7ffffffd, 0, 0) == 0
    pkts = [rtcp_packet(rng, SSRC, int(rng.integers(0, 65)))
            for _ in range(6)]
    with P.tune(noplanfuse=sep):
        got = run_dev(torch, "srtcp_encrypt", tx, pkts)
        want = oracle_run(ob, otx, "srtcp_encrypt", pkts)
        assert got == want
        assert not any(w[0] for w in want)
        e, st = tx.export(SSRC)
        assert e == 0 and st.rtcp_index == ob.rtcp_state(otx, SSRC)[0] == 3
        wire = [w[3][:w[2]] for w in want]
        T = P.tag_len(suite) if has_hmac(suite) else 0
        words = [int.from_bytes(w[len(w) - T - 4:len(w) - T], "big")
                 & 0x7fffffff for w in wire]
        assert words == [0x7ffffffe, 0x7fffffff, 0, 1, 2, 3]
        pr = Pair(torch, suite, flags)
        pr.seed(0x7ffffffc, 1)
        pr.packets(wire, "wrap")
        for k, w in enumerate(wire):
            pr.packets([w], ("wrap", "probe", k))
        # ... and cut behind the wrap: the second batch starts at index 0
        pr2 = Pair(torch, suite, flags)
        pr2.seed(0x7ffffffc, 1)
        pr2.packets(wire[:2], "wrap, first half", "plan")
        pr2.packets(wire[2:], "wrap, second half")
        pr.close()
        pr2.close()
    ob.free(otx)
    tx.close()


@pytest.mark.parametrize("sep", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_srtcp_forged_and_late(torch_cuda, case, sep):
    """batch 2 holds the late 90 and a forged packet of index 120, above
    every other: EAUTH, lix stays at the highest genuine index; batch 3
    brings the genuine 120"""
    suite, flags = case
    hm = has_hmac(suite)
    with P.tune(noplanfuse=sep):
        pr = Pair(torch_cuda, suite, flags)
        pr.batch([i for i in range(1, 101) if i != 90], 1, "plan")
        good = bytearray(pr.wire[120])
        # the tag's last byte (GCM: the E || index word follows the tag)
        good[-1 if hm else -5] ^= 0x40
        b2 = [pr.wire[i] for i in [90] + list(range(101, 111))] + \
            [bytes(good)]
        e2 = pr.packets(b2, 2)
        assert e2 == [0] * 11 + [P.EAUTH]
        if hm:
            assert pr.windows()[0][0] == 110
        e3 = pr.batch([120, 121], 3, "plan")
        assert e3 == [0, 0]
        if hm:
            assert pr.windows()[0][0] == 121
        pr.probe("forged")
        pr.close()


@pytest.mark.parametrize("sep", [0, 1])
@pytest.mark.parametrize("suite", [s for s, f in CASES if has_hmac(s) and
                                   not f])
def test_srtcp_e_bit_and_receiver_cipher(torch_cuda, suite, sep):
    """a receiver deciphers only a packet with the E bit set and only if it
    has a cipher itself (srtcp.c:214, "rtcp->aes && ep"): E = 1 packets at
    an SRTP_UNENCRYPTED_SRTCP receiver stay as they are, E = 0 packets at
    an encrypting one too -- in a planned batch, and in one a forged packet
    has the device undo"""
    U = P.SRTP_UNENCRYPTED_SRTCP
    with P.tune(noplanfuse=sep):
        for txf, rxf in ((0, U), (U, 0)):
            pr = Pair(torch_cuda, suite, rxf, tx_flags=txf)
            e1 = pr.batch(list(range(1, 41)), (txf, rxf, 1), "plan")
            assert not any(e1)
            bad = bytearray(pr.wire[60])
            bad[-1] ^= 0x40
            e2 = pr.packets([pr.wire[i] for i in range(41, 51)] +
                            [bytes(bad)], (txf, rxf, 2))
            assert e2 == [0] * 10 + [P.EAUTH]
            pr.top = 50
            pr.probe((txf, rxf))
            pr.close()
