"""The RTP rollover counter at 2^16, 2^31 and 2^32 on the CPU.

The reference is peculiar at large ROCs and a drop-in has to be peculiar in
the same way: srtp_get_index (src/srtp/misc.c:22-41) holds the ROC in an int
and returns seq + v * (uint64_t)65536, so from ROC 2^31 on the index the
replay window stores (replay.c:49) is sign-extended, 0xffff8000_0000_0000
and above.  Crossing 2^31 looks like a jump of more than 64 (the bitmap
restarts at 1, a late packet from before it is EALREADY); behind 2^32 the
uint32_t ROC is 0 again while the window's top stays near 2^64, and every
later packet is EALREADY behind a good tag.

  * the oracle (oracle/srtp_oracle.c) against the reference's own answers,
    tests/golden/srtp_roc_golden.json.gz (oracle/gen_roc_golden.c);
  * the receive rule's host twin srtp_rx_plan_host (plan_rx_rule.h in the
    decomposition of plan_rx.hip) over the fixture's arrivals and over the
    longer arrivals of tests/test_rxplan_cpu.py started at each boundary:
    fail != 0 with the state untouched, or exactly the sequential
    receiver's errnos and (roc, s_l, lix, bitmap) -- a wrong settled answer
    is never allowed.
"""
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import oracle_lib as O
from tests import roc_util as R
from tests import test_rxplan_cpu as X

BLOCKS = (4, 8, 64)
LOOKBACKS = (2, 4, 128)
SUITE = 1
KEY = bytes((13 * i + 5) & 0xff for i in range(30))
SSRC = X.SSRC
N = 600


@pytest.fixture(scope="module")
def be():
    P.load()
    return O.OracleBackend()


# ---- the oracle against the reference -------------------------------------

def test_fixture_covers_the_boundaries():
    names = {c["name"] for c in R.load()}
    for b in R.BOUNDS:
        for s in range(6):
            assert "tx_in_order_%s_s%d" % (b, s) in names
        for s in (1, 5):
            for shape in ("in_order", "swap_across", "late_before",
                          "dup_both_sides", "gap", "nine"):
                assert "rx_%s_%s_s%d" % (shape, b, s) in names
    assert {"rx_takeover_roc80000005_s1", "rx_takeover_roc80000005_s5"} \
        <= names
    for c in R.load():
        assert c["state0"]["roc"] in list(R.BOUNDS.values()) + [0x80000005]
        for b in c["batches"]:
            assert len(b["ops"]) <= 36
            for op in b["ops"]:
                hl = 12
                tag = (4, 10, 4, 10, 16, 16)[c["suite"]]
                n = len(op["in"]) // 2 - hl - (tag if c["kind"] == "rx" else 0)
                assert 16 <= n <= 32


@pytest.mark.parametrize("name", [c["name"] for c in R.load()])
def test_oracle_equals_reference(be, name):
    """every errno, pos, end, byte and state of the fixture, the oracle
    called one packet at a time from the case's state"""
    c = R.case(name)
    op = "srtp_encrypt" if c["kind"] == "tx" else "srtp_decrypt"
    ctx = R.oracle_at(be, c["suite"], bytes.fromhex(c["key"]), c["ssrc"],
                      R.state_tuple(c["state0"]))
    try:
        for bi, b in enumerate(c["batches"]):
            for i, o in enumerate(b["ops"]):
                inb, out = bytes.fromhex(o["in"]), bytes.fromhex(o["out"])
                e, pos, end, _, buf = be.call(ctx, op, len(inb) + 64, 0,
                                              len(inb), inb, len(out))
                assert (e, pos, end) == (o["err"], o["pos"], o["end"]), \
                    (name, bi, i)
                assert buf[:len(out)] == out, (name, bi, i)
            st = b["state"]
            assert be.export(ctx, c["ssrc"]) == \
                (st["roc"], st["s_l"], st["lix"], st["bitmap"]), (name, bi)
    finally:
        be.free(ctx)


# ---- the receive rule's host twin -----------------------------------------

def stream_state(st, ssrc=SSRC):
    s = P.StreamState()
    s.ssrc = ssrc
    s.roc, s.s_l, s.s_l_set, s.replay_rtp_lix, s.replay_rtp_bitmap = st
    return s


def sweep(st0, seq, errs, fin):
    """the rule over every (block, lookback) from st0 = (roc, s_l, s_l_set,
    lix, bitmap): {(block, lookback): settled}.  Not settled: the state is
    untouched; settled: the errnos and the final (roc, s_l, lix, bitmap)
    are the sequential receiver's"""
    seq = np.asarray(seq, dtype=np.uint16)
    out = {}
    for b in BLOCKS:
        for lb in LOOKBACKS:
            fail, ix, err, st1 = P.rx_plan_host(stream_state(st0), seq, b, lb)
            out[(b, lb)] = not fail
            got = (st1.roc, st1.s_l, st1.s_l_set, st1.replay_rtp_lix,
                   st1.replay_rtp_bitmap)
            if fail:
                assert got == tuple(st0), (b, lb)
                continue
            assert err.tolist() == list(errs), (b, lb, err.tolist(), errs)
            assert (got[0], got[1], got[3], got[4]) == tuple(fin), \
                (b, lb, [hex(x) for x in got], [hex(x) for x in fin])
            assert got[2] == 1
            assert ((ix & 0xffff) == seq).all()
    return out


def fixture_batches(c):
    """[(state before, sequence numbers, errnos, state after)] of the
    case's batches"""
    st, out = c["state0"], []
    for b in c["batches"]:
        seq = [int(o["in"][4:8], 16) for o in b["ops"]]
        out.append((R.state_tuple(st), seq, [o["err"] for o in b["ops"]],
                    (b["state"]["roc"], b["state"]["s_l"], b["state"]["lix"],
                     b["state"]["bitmap"])))
        st = b["state"]
    return out


RX_CASES = [c["name"] for c in R.load() if c["kind"] == "rx"
            and c["suite"] == 1]


@pytest.mark.parametrize("name", RX_CASES)
def test_rule_on_fixture_arrivals(name):
    """the reference's own verdicts and states: both batches of every
    receiver case (the second starts from the state the first left)"""
    c = R.case(name)
    for st0, seq, errs, fin in fixture_batches(c):
        ok = sweep(st0, seq, errs, fin)
        if c["state0"]["roc"] == R.BOUNDS["2p16"] and \
                errno.ETIMEDOUT not in errs:
            # nothing in the reference is special at 2^16
            assert all(v for (b, lb), v in ok.items() if lb == 128), \
                (name, ok)


def test_nine_arrivals_across_2p31():
    """roc 0x7fffffff, s_l 65530, lix 0x7fffffff_fffa, bitmap 1; arrivals
    65531, 65532, 65534, 65533, 65535, 0, 2, 1, 3: all accepted, and the
    reference's window ends at lix 0xffff_8000_0000_0003, bitmap 0xf (the
    index is sign-extended behind 2^31, the bitmap restarted at the
    crossing).  A rule that settles this in the zero-extended domain leaves
    lix 0x0000_8000_0000_0003, bitmap 0x3ff -- and accepts a later replay of
    seq 1, which the reference answers with EALREADY"""
    c = R.case("rx_nine_2p31_s1")
    (st0, seq, errs, fin), (st1, seq1, errs1, fin1) = fixture_batches(c)
    assert st0 == (0x7fffffff, 65530, 1, 0x7ffffffffffa, 1)
    assert seq == [65531, 65532, 65534, 65533, 65535, 0, 2, 1, 3]
    assert errs == [0] * 9
    assert fin == (0x80000000, 3, 0xffff800000000003, 0xf)
    sweep(st0, seq, errs, fin)
    # the second batch replays seq 1 (EALREADY in the reference)
    assert seq1[0] == 1 and errs1[0] == errno.EALREADY
    sweep(st1, seq1, errs1, fin1)


# ---- longer arrivals, as tests/test_rxplan_cpu.py builds them -------------

S0S = (65000, 65500)    # the boundary at send position 536 and at 36
SHAPES = ("in_order", "block_swaps", "displaced", "dup_2", "dup_128",
          "dup_max64", "repeated_300", "late_70")


def oracle_state(roc, s0):
    """a stream whose last packet was s0 - 1 at roc, nothing else seen"""
    return (roc, (s0 - 1) & 0xffff, 1, R.ref_lix(roc, (s0 - 1) & 0xffff), 1)


@pytest.fixture(scope="module")
def sent(be):
    """per (boundary, s0): the in-order protected stream from just below
    the boundary (shared, never modified)"""
    out = {}
    for bname, roc in R.BOUNDS.items():
        for s0 in S0S:
            ctx = R.oracle_at(be, SUITE, KEY, SSRC, oracle_state(roc, s0))
            pk = []
            for k in range(N):
                p = X.packet((s0 + k) & 0xffff, k)
                e, _, en, _, buf = be.call(ctx, "srtp_encrypt", 256, 0,
                                           len(p), p, 0)
                assert e == 0
                pk.append(buf[:en])
            be.free(ctx)
            out[(bname, s0)] = pk
    return out


def receive(be, st0, pkts):
    ctx = R.oracle_at(be, SUITE, KEY, SSRC, st0)
    errs = [be.call(ctx, "srtp_decrypt", 256, 0, len(p), p, 0)[0]
            for p in pkts]
    fin = be.export(ctx, SSRC)
    be.free(ctx)
    return errs, fin


def check_arrivals(be, bname, st0, arr, must_settle):
    errs, fin = receive(be, st0, arr)
    assert P.EAUTH not in errs
    ok = sweep(st0, [X.seq_of(p) for p in arr], errs, fin)
    crossed = fin[0] != st0[0]
    if bname == "2p16":
        if must_settle:
            assert all(v for (b, lb), v in ok.items() if lb == 128), ok
    elif crossed:
        # the sign-extended domain is left to the sequential receiver
        assert not any(ok.values()), ok
    return ok, errs, fin


@pytest.mark.parametrize("s0", S0S)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("bname", sorted(R.BOUNDS))
def test_shapes_across_the_boundary(be, sent, bname, shape, s0):
    arr = [sent[(bname, s0)][k] for k in X.SHAPES[shape]()]
    st0 = oracle_state(R.BOUNDS[bname], s0)
    # a copy of a packet from before the rollover arriving behind it is
    # ETIMEDOUT in the reference: never settled
    wrap = 65536 - s0
    d = int(shape[4:]) if shape[4:].isdigit() else 0
    timeout = any(k < wrap <= k + d for k in X.DUP_AT)
    settles = shape != "late_70" and not timeout
    ok, errs, fin = check_arrivals(be, bname, st0, arr, settles)
    assert (errno.ETIMEDOUT in errs) == timeout
    # stopping one packet short of the rollover settles at every boundary
    short = [p for p in arr[:wrap] if X.seq_of(p) >= s0]
    errs, fin = receive(be, st0, short)
    assert fin[0] == R.BOUNDS[bname]
    ok = sweep(st0, [X.seq_of(p) for p in short], errs, fin)
    if bname != "2p32" and shape != "late_70":
        # (at 2^32 - 1 the window before the batch is sign-extended already)
        assert all(v for (b, lb), v in ok.items() if lb == 128), ok


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("bname", sorted(R.BOUNDS))
def test_network_shaped_across_the_boundary(be, sent, bname, seed):
    rng = np.random.default_rng(9100 + seed)
    order = X.network_shaped(rng, N)
    for s0 in S0S:
        wrap = 65536 - s0
        seen_post, late_pre = False, False
        for k in order:
            if k >= wrap:
                seen_post = True
            elif seen_post:
                late_pre = True
        arr = [sent[(bname, s0)][k] for k in order]
        st0 = oracle_state(R.BOUNDS[bname], s0)
        check_arrivals(be, bname, st0, arr, not late_pre)
        # continuing: the second half behind the first
        h = len(arr) // 2
        errs, mid = receive(be, st0, arr[:h])
        st1 = (mid[0], mid[1], 1, mid[2], mid[3])
        errs, fin = receive(be, st1, arr[h:])
        sweep(st1, [X.seq_of(p) for p in arr[h:]], errs, fin)


@pytest.mark.parametrize("roc", [0x80000000, 0x80000005, 0xfffffffe,
                                 0xffffffff])
def test_imported_state_with_empty_window(roc):
    """a stream taken over at a ROC of 2^31 or more before any packet was
    received (lix 0, bitmap 0): the `lix >> 62` guard on the window sees
    nothing; the rule itself must decline"""
    for s_l, seq in ((1000, [1001, 1002, 1004, 1003]),
                     (65534, [65535, 0, 1])):
        st0 = (roc, s_l, 1, 0, 0)
        for b in BLOCKS:
            fail, _, _, st1 = P.rx_plan_host(stream_state(st0),
                                             np.array(seq, dtype=np.uint16),
                                             b, 128)
            assert fail
            assert (st1.roc, st1.s_l, st1.s_l_set, st1.replay_rtp_lix,
                    st1.replay_rtp_bitmap) == st0


# ---- the cross-rank fold ---------------------------------------------------

def arena_of(pkts):
    pos, end, buf = [], [], bytearray()
    for p in pkts:
        pos.append(len(buf))
        buf += p
        end.append(len(buf))
        buf += bytes(-len(buf) % 16)
    return (np.frombuffer(bytes(buf), dtype=np.uint8),
            np.array(pos, dtype=np.uint32), np.array(end, dtype=np.uint32))


def fold_equals(st0, pkts, errs, fin, ssrc=SSRC):
    """srtp_rx_index + srtp_rx_fold over one rank's records from the true
    state: exact, or stopped with the state before the first void packet"""
    from re_amd import shard as S
    arena, pos, end = arena_of(pkts)
    rec = S.rx_records(stream_state(st0, ssrc), arena, pos, end,
                       np.array(errs, dtype=np.int32))
    st = stream_state(st0, ssrc)
    err, nd = S.rx_fold(st, SUITE, rec)
    got = (st.roc, st.s_l, st.replay_rtp_lix, st.replay_rtp_bitmap)
    assert err.tolist() == list(errs[:nd])
    if nd < len(pkts):
        # refused from packet nd on: nothing behind it was applied (never
        # at packet 0 here -- the records are the true receiver's own)
        assert nd == 0 and got == (st0[0], st0[1], st0[3], st0[4]), nd
        return False
    assert got == tuple(fin), ([hex(x) for x in got], [hex(x) for x in fin])
    return True


@pytest.mark.parametrize("name", RX_CASES)
def test_fold_on_fixture_arrivals(name):
    """the fold's own walk (rxfold.c, get_index of srtp.c) over the
    reference's verdicts: the records of the true receiver fold to the
    reference's state at every boundary"""
    c = R.case(name)
    st = R.state_tuple(c["state0"])
    for b in c["batches"]:
        pkts = [bytes.fromhex(o["in"]) for o in b["ops"]]
        errs = [o["err"] for o in b["ops"]]
        fin = (b["state"]["roc"], b["state"]["s_l"], b["state"]["lix"],
               b["state"]["bitmap"])
        assert fold_equals(st, pkts, errs, fin, c["ssrc"])
        st = R.state_tuple(b["state"])


# srtp_rx_index walks in parallel parts while roc + n + 2 < 0x7fffffff
# (rxfold.c rx_walk_packed), srtp_rx_fold while roc + n + 4 < 0x7fffffff and
# n >= 65536: one ROC just under and one just over each guard
FOLD_N = 65536
FOLD_ROCS = (0x7fffffff - FOLD_N - 5, 0x7fffffff - FOLD_N - 4,
             0x7fffffff - FOLD_N - 3, 0x7fffffff - FOLD_N - 2)


@pytest.mark.parametrize("roc", FOLD_ROCS)
def test_fold_guard(be, roc):
    """65536 arrivals (one rollover inside, swaps and duplicates) from a
    ROC beside the guards of the parallel walks: exact against the oracle
    receiver, or refused with the state unchanged"""
    s0 = 40000
    st0 = oracle_state(roc, s0)
    ctx = R.oracle_at(be, SUITE, KEY, SSRC, st0)
    order = list(range(FOLD_N - 60))
    for k in range(500, len(order) - 1, 1009):
        order[k], order[k + 1] = order[k + 1], order[k]
    for k in range(60):
        at = 700 + 1091 * k
        order.insert(at + 3, order[at])
    assert len(order) == FOLD_N
    sent = []
    for k in range(FOLD_N - 60):
        p = X.packet((s0 + k) & 0xffff, k)
        e, _, en, _, buf = be.call(ctx, "srtp_encrypt", 64, 0, len(p), p, 0)
        assert e == 0
        sent.append(buf[:en])
    be.free(ctx)
    arr = [sent[k] for k in order]
    errs, fin = receive(be, st0, arr)
    assert errs.count(errno.EALREADY) == 60 and errs.count(0) == FOLD_N - 60
    assert fin[0] == roc + 1
    fold_equals(st0, arr, errs, fin)
