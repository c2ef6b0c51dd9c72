"""SRTCP length geometry: packets of every byte length 8..207 on every device
route, the per-call paths and the mbuf batch, bit-exact against the oracle
(tests/oracle_lib.py, pinned to the reference at these lengths by
tests/test_srtcp_geom_cpu.py) called one packet at a time.

The reference takes any SRTCP packet of at least 8 bytes (srtcp.c:31-140,
143-287); a length that is no multiple of 4 puts the end of the cipher region,
the E || index word and the tag inside a word: the byte-exact region end of
k_ctr_fast.h ctr_fast_pkt<RTCP>, the msg_word splice and the tag stores at an
unaligned address, the trailer across a 64-byte chunk on an HMAC unprotect
(plain length % 64 in 61..63), the AAD splice of gcm.hip at A = L with
SRTP_UNENCRYPTED_SRTCP, SJ_TRAILER / SJ_STORE_TRAIL at an odd offset in the
general kernels.  Short packets: L = 8 has an empty cipher region, 51..63 a
SHA-1 block that is all padding, below 24 no whole GCM block.

Batches (tests/srtcp_geom.py): the lengths LENS = 8..207 as a "run" (the
lanes of a quad differ by one byte) and "spread" (packet i has length
LENS[53 i % 200]: neighbouring lanes differ in chunk count).  Unprotect takes
the oracle's protected packets, once clean and once with about 1 % forged in
the body or the tag's last byte.  Which route ran is asserted by the counters
of srtp_gpu_counter, as batch_dev.c moves them: a fallback to the host engine
would pass any byte comparison.

  dev_planned_rtcp    rplans +1, rejects +0; a forged batch: rplans +1,
                      folds +1 (rplanned_done), rejects +0
  dev_mplanned_rtcp   mrplans +1, rejects +0; forged: folds +1 as well
  dev_splanned_rtcp   srplans +1 (a new session's first batch comes behind the
                      one-stream plan's rejection: rejects +1); forged:
                      srundos +1, srplans +0
  dev_mrrxplanned     mrrxplans +1 behind mrplans +0, rejects +1

"nolean" only switches the crypto kernel of the one-stream route (batch_dev.c
dev_lplanned_rtcp / dev_planned_rtcp: C.uniform 1 instead of 4) and is a
variant there alone.  "nobucket" is not read on any SRTCP route
(dev_mplanned_rtcp always takes sgpu_bplan_geometry's buckets), so the
many-session route has no such variant.

Compared with the oracle: errno, pos and end relative to the packet, every
byte the oracle leaves (protect: [0, end); unprotect: the whole received
length, trailer and tag included) and per SSRC the exported rtcp_index and
SRTCP replay window.
"""
import numpy as np
import pytest

import re_amd.srtp as P
from tests import oracle_lib as O
from tests import srtcp_geom as G
from tests.golden_util import replay_scenario
from tests.product_backend import ProductBackend
from tests.test_gpu_fastpath import keys_for, run_dev, to_arena
from tests.test_gpu_hdrgeom import (counted, mbuf_result, same_as_oracle,
                                    same_mbuf)
from tests.test_srtcp_geom_cpu import load_geom_golden

pytestmark = pytest.mark.gpu

CNT = ("rplans", "mrplans", "mrrxplans", "srplans", "srundos", "rejects",
       "folds", "rxdups")
flag_ids = ["e", "u"]


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


def only(d, **want):
    """the counters named moved as given, every other planner's not at all"""
    plans = ("rplans", "mrplans", "mrrxplans", "srplans", "srundos")
    exp = {c: 0 for c in plans}
    exp.update(want)
    return {c: d[c] for c in exp} == exp


def run_checked(torch, knobs, op, ctx, pkts, many, rows, what):
    """one device batch of [(session, packet)] on the contexts ctx, compared
    with the oracle's rows; returns the counters it moved"""
    arena, pos, end, cap, sess = to_arena(pkts)
    out, d = counted(torch, run_dev, knobs, op, ctx, arena, pos, end, cap,
                     sess if many else None, names=CNT)
    same_as_oracle(out, pos, rows, op == "srtcp_encrypt", what)
    return d


def route(torch, R, suite, flags, many, knobs, accept, forged, what):
    """protect, unprotect of the clean batch and of the forged one (a
    receiver of its own) under the knobs; accept / forged: the counters an
    accepted plan and one with forged packets move"""
    new = lambda: [P.Srtp(suite, k, flags) for k in R["keys"]]
    tx, rx, frx = new(), new(), new()
    for op, ctx, pkts, rows, st, exp in (
            ("srtcp_encrypt", tx, R["plain"], R["enc"], R["tx_state"], accept),
            ("srtcp_decrypt", rx, R["clean"], R["dec"], R["rx_state"], accept),
            ("srtcp_decrypt", frx, R["forged"], R["fdec"], R["frx_state"],
             forged)):
        w = (what, op, exp is forged)
        d = run_checked(torch, knobs, op, ctx, pkts, many, rows, w)
        if exp is not None:
            assert only(d, **exp), (w, d)
        assert G.product_states(ctx, R["streams"]) == st, w
    for c in tx + rx + frx:
        c.close()


# ---- one stream: dev_planned_rtcp ------------------------------------------

ONE = [("default", {}), ("nolean", {"nolean": 1}),
       ("planner", {"noplanfuse": 1})]


@pytest.mark.parametrize("order", G.ORDERS)
@pytest.mark.parametrize("flags", G.FLAGS, ids=flag_ids)
@pytest.mark.parametrize("suite", range(6))
def test_one_stream(suite, flags, order, torch_cuda):
    """k_rp_plan in front of the lean SRTCP form of k_ctr_fast.h (GCM:
    k_gcmu), the general compact kernel (nolean), and k_parse + k_plan_rtcp
    (noplanfuse)"""
    R = G.reference(suite, flags, order, "one")
    for path, knobs in ONE:
        route(torch_cuda, R, suite, flags, False, knobs,
              {"rplans": 1, "rejects": 0, "folds": 0},
              {"rplans": 1, "rejects": 0, "folds": 1}, path)


# ---- many sessions: dev_mplanned_rtcp and the host engine --------------------

@pytest.mark.parametrize("order", G.ORDERS)
@pytest.mark.parametrize("flags", G.FLAGS, ids=flag_ids)
@pytest.mark.parametrize("suite", range(6))
def test_many_sessions(suite, flags, order, torch_cuda):
    """130 sessions in two buckets, 520 packets dealt round-robin: the bucket
    planner of plan_buckets_rtcp.hip in front of the compact kernels with
    per-packet keys; then the same batches under nomrplan=1, the host engine
    and the general kernels with SJ_TRAILER (results only).  No nobucket or
    nolean variant: dev_mplanned_rtcp reads neither (module docstring)."""
    R = G.reference(suite, flags, order, "many")
    with P.tune(bpexp=G.BPEXP):
        route(torch_cuda, R, suite, flags, True, {},
              {"mrplans": 1, "rejects": 0, "folds": 0},
              {"mrplans": 1, "rejects": 0, "folds": 1}, "bucket")
    off = {"mrplans": 0}
    route(torch_cuda, R, suite, flags, True, {"nomrplan": 1}, off, off,
          "host")


# ---- one session, three SSRCs: dev_splanned_rtcp -----------------------------

@pytest.mark.parametrize("flags", G.FLAGS, ids=flag_ids)
@pytest.mark.parametrize("suite", range(6))
def test_three_ssrcs(suite, flags, torch_cuda):
    """600 packets of three interleaved SSRCs, "spread" lengths: the
    per-stream planner of plan_streams_rtcp.hip and the general
    descriptor-driven kernels (class 2) behind the one-stream plan's
    rejection for the second SSRC; a forged packet has the plan undone and
    the host engine take the batch"""
    R = G.reference(suite, flags, "spread", "three")
    route(torch_cuda, R, suite, flags, False, {},
          {"srplans": 1, "rejects": 1, "folds": 0},
          {"srundos": 1, "rejects": 1}, "streams")


# ---- disturbed receive -----------------------------------------------------------

@pytest.mark.parametrize("nsess", [1, 12], ids=["one", "many"])
@pytest.mark.parametrize("suite", [1, 3])
def test_disturbed_receive(suite, nsess, torch_cuda):
    """two SSRCs per session, every other packet of a plain length % 64 in
    61..63 (the E || index word across the chunk boundary between the last
    cipher chunk and the MAC tail); per stream two arrivals swapped and the
    first delivered again five arrivals later: EALREADY for exactly the
    copies, which stay authenticated and not deciphered.  One session:
    dev_splanned_rtcp; twelve: dev_mrrxplanned behind the in-order plan's
    rejection."""
    keys, streams, arr, rows, st, dup = G.disturbed(suite, nsess)
    assert {len(arr[i][1]) - G.growth(suite) for i in dup} <= set(G.STRADDLE)
    rx = [P.Srtp(suite, k) for k in keys]
    d = run_checked(torch_cuda, {}, "srtcp_decrypt", rx, arr, nsess > 1, rows,
                    ("disturbed", nsess))
    if nsess == 1:
        assert only(d, srplans=1, rejects=1, folds=0, rxdups=len(dup)), d
    else:
        assert only(d, mrrxplans=1, rejects=1, folds=0, rxdups=len(dup)), d
    assert G.product_states(rx, streams) == st
    for c in rx:
        c.close()


# ---- per-call and mbuf-batch API --------------------------------------------------

@pytest.mark.parametrize("path", ["small", "coop", "general"])
@pytest.mark.parametrize("flags", G.FLAGS, ids=flag_ids)
@pytest.mark.parametrize("suite", range(6))
def test_per_call(suite, flags, path, torch_cuda):
    """srtcp_encrypt / srtcp_decrypt one call at a time, lengths either side
    of every word, SHA-1 block and 64-byte chunk, any mb->pos, the receiver's
    buffer with no room to spare: through the three per-call paths of
    test_per_call_golden"""
    key, enc, dec = G.percall_reference(suite, flags)
    tx, rx = P.Srtp(suite, key, flags), P.Srtp(suite, key, flags)
    with P.tune(nosmall=0 if path == "small" else 1,
                nocoop=1 if path == "general" else 0):
        for ctx, calls in ((tx, enc), (rx, dec)):
            for i, (op, data, size, off, want) in enumerate(calls):
                mb = P.new_mbuf(data, size, off)
                got = mbuf_result(ctx._op(op, mb), mb)
                P.free_mbuf(mb)
                same_mbuf(got, want, (op, i, off, len(data) - off))
    tx.close()
    rx.close()


@pytest.mark.parametrize("flags", G.FLAGS, ids=flag_ids)
@pytest.mark.parametrize("suite", range(6))
def test_mbuf_batch(suite, flags, torch_cuda):
    """the same calls as one srtcp_encrypt_mbufs and one srtcp_decrypt_mbufs
    batch"""
    key, enc, dec = G.percall_reference(suite, flags)
    tx, rx = P.Srtp(suite, key, flags), P.Srtp(suite, key, flags)
    for ctx, calls in ((tx, enc), (rx, dec)):
        mbs = [P.new_mbuf(data, size, off) for _, data, size, off, _ in calls]
        rc, errs = P.batch_run(ctx, calls[0][0], mbs)
        assert rc == 0
        for i, (mb, e, c) in enumerate(zip(mbs, errs, calls)):
            same_mbuf(mbuf_result(e, mb), c[4], (c[0], i, c[3]))
            P.free_mbuf(mb)
    tx.close()
    rx.close()


@pytest.mark.parametrize("path", ["small", "coop", "general"])
def test_per_call_geom_golden(path, torch_cuda):
    """the reference's own recorded calls (srtcp_geom_golden.json.gz: every
    length 8..143, the receiver's repeat included) one call at a time"""
    be = ProductBackend()
    with P.tune(nosmall=0 if path == "small" else 1,
                nocoop=1 if path == "general" else 0):
        bad = [m for m in (replay_scenario(be, s)
                           for s in load_geom_golden()["scenarios"]) if m]
    assert not bad, bad[:5]


# ---- the size bound ------------------------------------------------------------------

@pytest.mark.parametrize("suite", [1, 5])
def test_size_bound_odd_lengths(suite, torch_cuda):
    """plain lengths 4027..4037 and the same minus the suite's growth: odd
    lengths either side of the counter-cached kernels' bound (SGPU_CACHED_MAX,
    4032) before and after protection.  A packet at or past the bound has the
    plan rejected (SPF_SIZE) and the host engine send it to the plain
    kernels; the packets below it alone are planned (rplans +1)."""
    lens = G.bound_lengths(suite)
    rng = np.random.default_rng(4030 + suite)
    key = keys_for(suite, 1)[0]
    plain = [(0, G.packet(rng, G.SSRC, L)) for L in lens]
    be = O.OracleBackend()
    for part in ("all", "below"):
        otx, orx = be.alloc(suite, key, 0)[0], be.alloc(suite, key, 0)[0]
        tx, rx = P.Srtp(suite, key), P.Srtp(suite, key)
        pk = plain
        for op, octx, ctx in (("srtcp_encrypt", otx, tx),
                              ("srtcp_decrypt", orx, rx)):
            if part == "below":
                pk = [q for q in pk if len(q[1]) < 4032]
            assert len(pk) >= 5 and {len(q[1]) % 4 for q in pk} == {0, 1, 2, 3}
            rows = G.oracle_rows(be, [octx], op, pk)
            assert not any(r[0] for r in rows)
            d = run_checked(torch_cuda, {}, op, [ctx], pk, False, rows,
                            (part, op))
            if part == "below":
                assert only(d, rplans=1, rejects=0, folds=0), (op, d)
            else:
                assert max(len(q[1]) for q in pk) >= 4032
                assert only(d, rejects=1), (op, d)
            assert G.product_states([ctx], [(0, G.SSRC)]) == \
                G.rtcp_states(be, [octx], [(0, G.SSRC)]), (part, op)
            pk = [(0, r[3][:r[2]]) for r in rows]
        for c in (otx, orx):
            be.free(c)
        tx.close()
        rx.close()
