"""Length geometry of the unchanged re_srtp.h path -- one mbuf per srtp_* call,
or one srtp_*_mbufs batch -- up to and past the small kernel's 2048-byte
bound, bit-exact against the oracle (tests/oracle_lib.py, pinned to the
reference at these lengths by tests/test_long_geom_cpu.py) called one packet
at a time.

This path runs three kernels of its own, all with length-dependent
structure: k_ctr_small / gcm_small (small.hip: one packet per workgroup,
staged in 2048 bytes of LDS; the SHA-1 schedule of up to 33 blocks, the
guards past word 511, the GHASH split over n = 2..131 blocks, region_ks with
the partial last word at every length mod 16 and GCM's counter offset), the
coop kernels' one-workgroup-per-packet cipher pass and the general kernels'
MAC-only walk (nosmall / nocoop), whose head, steady and tail chunks run for
every packet past the bound.

Traffic (tests/long_geom.py): RTP packets of every length 12..2120 in the
four header classes and with CC = 15 plus an extension, the ROC rolling
inside, then 4000..9000 bytes; SRTCP packets of every length 8..2120 with and
without SRTP_UNENCRYPTED_SRTCP; mb->pos cycling through 0, 1, 2, 3, 5, 6, 7;
forged copies and a repeat at every 97th length and where the protected
packet is 2047, 2048 and 2049 bytes long.

Which kernel ran is asserted by the counter "small_launches" (srtp.c
round_small, percall.c pc_run_fused: +1 per launch of the small kernel):
without that a fallback to the copy path would pass the byte comparison.
small_fits() sends a round to the small kernel only if every packet's
protected length from mb->pos is at most SGPU_SMALL_MAX (2048) and the round
has at most SGPU_COOP_MAX (2048) jobs.

Compared with the oracle: errno, pos, end, size and every byte of the mbuf
(unprotect: the tag region and a forged packet's bytes included), and the
exported stream state after every sweep.
"""
import functools
import threading
import time

import pytest

import re_amd.srtp as P
from tests import long_geom as LG
from tests import srtcp_geom as G
from tests import test_gpu_percall as PC
from tests.test_gpu_hdrgeom import mbuf_result, product_states, same_mbuf

pytestmark = pytest.mark.gpu

PATHS = ("small", "coop", "general")
kinds = pytest.mark.parametrize("kind", range(3), ids=LG.KIND_IDS)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


def small():
    return P.counter("small_launches")


def state_of(ctx, kind):
    """the exported stream state in the oracle's shape"""
    if kind == "srtp":
        return product_states([ctx], [LG.SSRC])[0]
    return G.product_states([ctx], [(0, LG.SSRC)])[0]


# ---- a. one call per packet ----------------------------------------------------

@kinds
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("suite", range(6))
def test_per_call_sweep(suite, path, kind, torch_cuda):
    """every length, one srtp_* call each, through the three per-call paths
    of test_per_call_golden.  One call holds one packet, and a packet whose
    job ran is not planned again with another job (srtp.c verdict_for: a
    forged copy and a repeat have the job of their first plan), so a call is
    one round: on "small" exactly one launch of the small kernel where the
    protected length is at most 2048 and none above; none at all under
    nosmall."""
    kind, flags = LG.KINDS[kind]
    R = LG.sweep(suite, kind, flags)
    tx, rx = P.Srtp(suite, R["key"], flags), P.Srtp(suite, R["key"], flags)
    seen = set()
    t0 = time.perf_counter()
    with P.tune(nosmall=0 if path == "small" else 1,
                nocoop=1 if path == "general" else 0):
        for ctx, calls in ((tx, R["enc"]), (rx, R["dec"])):
            for c in calls:
                mb = P.new_mbuf(c.data, c.size, c.off)
                s0 = small()
                e = ctx._op(c.op, mb)
                d = small() - s0
                got = mbuf_result(e, mb)
                P.free_mbuf(mb)
                what = (c.op, c.L, c.off, c.note)
                same_mbuf(got, c.want, what)
                fits = path == "small" and c.plen <= LG.SMALL_MAX
                assert d == (1 if fits else 0), (what, c.plen, d)
                seen.add((c.op, c.plen, c.note))
    print("per-call sweep %s %s s%d: %.2f s" % (
        path, LG.KIND_IDS[LG.KINDS.index((kind, flags))], suite,
        time.perf_counter() - t0))
    # either side of the switch, forged and repeated too
    for op in LG.op_names(kind):
        assert {(op, p, "true") for p in LG.EDGE} <= seen
    assert {(LG.op_names(kind)[1], p, n) for p in LG.EDGE
            for n in ("body", "tag", "again")} <= seen
    assert state_of(tx, kind) == R["tx_state"]
    assert state_of(rx, kind) == R["rx_state"]
    tx.close()
    rx.close()


# ---- b. the same calls as mbuf batches ---------------------------------------

def run_batches(ctx, calls, what):
    """calls as srtp_*_mbufs batches of at most SGPU_COOP_MAX mbufs, compared
    with the oracle's rows; returns the launches of the small kernel per
    batch"""
    moved = []
    for b in range(0, len(calls), 2048):
        part = calls[b:b + 2048]
        mbs = [P.new_mbuf(c.data, c.size, c.off) for c in part]
        s0 = small()
        rc, errs = P.batch_run(ctx, part[0].op, mbs)
        moved.append(small() - s0)
        assert rc == 0, what
        for mb, e, c in zip(mbs, errs, part):
            same_mbuf(mbuf_result(e, mb), c.want, (what, c.op, c.L, c.note))
            P.free_mbuf(mb)
    return moved


@kinds
@pytest.mark.parametrize("suite", range(6))
def test_mbuf_batches(suite, kind, torch_cuda):
    """"fit": every length whose protected packet is at most 2048 bytes long
    in one srtp_*_mbufs batch (the receiver's list, longer than SGPU_COOP_MAX
    with its forged copies and repeats, in two): the small kernel takes
    every batch, in as many rounds as the forged copies ask for (a verdict
    that changes a later packet's plan makes another round).  "edge":
    protected lengths 2040..2060 in one batch: one packet past the bound
    sends the whole round to the copy path, and the disturbed packet of 2049
    bytes is part of every later round.  "jumbo": 4000..9000 bytes in one
    batch."""
    kind, flags = LG.KINDS[kind]
    for name, ref in (("fit", LG.fitting), ("edge", LG.straddling),
                      ("jumbo", LG.jumbo)):
        R = ref(suite, kind, flags)
        tx, rx = (P.Srtp(suite, R["key"], flags) for _ in range(2))
        for ctx, calls, st in ((tx, R["enc"], R["tx_state"]),
                               (rx, R["dec"], R["rx_state"])):
            what = (name, calls[0].op)
            moved = run_batches(ctx, calls, what)
            if name == "fit":
                assert max(c.plen for c in calls) == LG.SMALL_MAX
                assert len(moved) == (1 if ctx is tx else 2), what
                assert all(d >= 1 for d in moved), (what, moved)
            else:
                if name == "edge":
                    assert min(c.plen for c in calls) < LG.SMALL_MAX < \
                        max(c.plen for c in calls)
                assert moved == [0], (what, moved)
            assert state_of(ctx, kind) == st, what
        tx.close()
        rx.close()


# ---- c. the job-count bound ----------------------------------------------------

@pytest.mark.parametrize("suite", range(6))
def test_job_count_edge(suite, torch_cuda):
    """2047, 2048 and 2049 packets of 60..90 bytes in one srtp_encrypt_mbufs
    and one srtp_decrypt_mbufs batch, packet 1000 forged on the way back: a
    round of more than SGPU_COOP_MAX jobs leaves the small kernel (and
    sgpu_run_class drops the coop split).  The forged packet changes no
    later packet's job (in order, no rollover), so the batch is one round."""
    for n in LG.NJOBS:
        R = LG.many_short(suite, n)
        tx, rx = P.Srtp(suite, R["key"]), P.Srtp(suite, R["key"])
        for ctx, calls, st in ((tx, R["enc"], R["tx_state"]),
                               (rx, R["dec"], R["rx_state"])):
            mbs = [P.new_mbuf(c.data, c.size, c.off) for c in calls]
            s0 = small()
            rc, errs = P.batch_run(ctx, calls[0].op, mbs)
            d = small() - s0
            assert rc == 0 and len(mbs) == n
            for i, (mb, e, c) in enumerate(zip(mbs, errs, calls)):
                same_mbuf(mbuf_result(e, mb), c.want, (n, c.op, i))
                P.free_mbuf(mb)
            assert d == (1 if n <= 2048 else 0), (n, calls[0].op, d)
            assert state_of(ctx, "srtp") == st, (n, calls[0].op)
        tx.close()
        rx.close()


# ---- d. threads: shared launches with long packets ---------------------------

LONG_THREADS = (0, 5, 10, 15)   # one of every suite of the set


def long_plens(rng, t, k):
    """payloads of 20..300 and 1990..2036 bytes (12-byte headers: protected
    lengths up to and just past 2048); on four threads every 7th of
    2037..2200 bytes"""
    if t in LONG_THREADS and k % 7 == 3:
        return int(rng.integers(2037, 2201))
    if int(rng.integers(0, 2)):
        return int(rng.integers(1990, 2037))
    return int(rng.integers(20, 301))


@pytest.mark.parametrize("suites,fuse", [
    ([1, 0, 3, 2], 1), ([1, 0, 3, 2], 0), (PC.SUITES, 1), (PC.SUITES, 0)],
    ids=["ctr-fuse", "ctr-nofuse", "gcm-fuse", "gcm-nofuse"])
def test_threads_with_long_packets(torch_cuda, monkeypatch, suites, fuse):
    """16 threads as in test_threads_share_launches_exactly (one runner: its
    queue gathers every thread's next call, so lists mix operations), with
    packets either side of the bound: pc_run_fused runs a mixed list as one
    launch only if every operation's small_fits holds, else it returns with
    nothing changed and each operation runs its usual way.  Every call
    equals the oracle's; some lists were fused and some batches were not."""
    monkeypatch.setattr(PC, "script",
                        functools.partial(PC.script, plens=long_plens))
    T = 16
    lens = [len(a) for t in range(T) for op, a in PC.script(t)
            if op == "srtp_encrypt"]
    assert min(lens) < 400 and max(lens) > 2100
    keys = [bytes((13 * t + i) & 0xff for i in range(46)) for t in range(T)]
    want, got, ths = {}, {}, []
    for t in range(T):
        s = suites[t % 4]
        k = keys[t][:P.key_len(s) + P.salt_len(s)]
        PC.run_thread(t, s, k, PC.oracle_backend, want)
        ths.append(threading.Thread(target=PC.run_thread,
                                    args=(t, s, k, PC.dev_backend, got)))
    b0, p0 = P.counter("pcbatches"), P.counter("pcpackets")
    f0 = P.counter("pcfused")
    with P.tune(nofuse=0 if fuse else 1, pcrunners=1):
        for th in ths:
            th.start()
        for th in ths:
            th.join(120)
    assert len(got) == T
    for t in range(T):
        assert len(got[t]) == len(want[t])
        for i, (g, w) in enumerate(zip(got[t], want[t])):
            assert g[:3] == w[:3], (t, i)
            assert g[3][:len(w[3])] == w[3][:len(g[3])], (t, i)
    batches = P.counter("pcbatches") - b0
    fused = P.counter("pcfused") - f0
    assert P.counter("pcpackets") - p0 == sum(len(v) for v in got.values())
    if fuse:
        assert fused > 0
    else:
        assert fused == 0
    assert batches - fused > 0
