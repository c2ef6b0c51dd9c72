"""GPU tests of the many-session device receive planner (re_amd/csrc/hip/
plan_buckets_rx.hip, batch_dev.c dev_mrxplanned): a many-session unprotect
batch, one stream per session, whose sessions see reordered, duplicated or
lost packets is planned exactly on the device behind the bucket planner's
rejection, the session states staying resident.

Every case protects each session's packets in order, reshapes the arrivals
per session, interleaves the sessions at random and unprotects through
srtp_decrypt_batch_dev (or its asynchronous form).  Arena, pos, end, err
and every session's exported state must equal those of the same call with
the planner off (srtp_gpu_tune norxplan: the host engine) and those of the
oracle receiver called one packet at a time per session; the counters say
which path produced them ("mrxplans": this planner).
"""
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import oracle_lib as O
from tests.test_gpu_buckets import states
from tests.test_gpu_fastpath import keys_for, rtp_packet, run_dev, to_arena

pytestmark = pytest.mark.gpu

NSESS = 600
COUNTERS = ("mrxplans", "mplans", "rejects", "folds", "devfolds", "rxplans",
            "rxlate", "rxdups")


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


def run_async(torch, opname, sessions, arena, pos, end, cap, sess):
    """srtp_*_batch_dev_async + srtp_batch_wait, every array in HBM"""
    dev = torch.from_numpy(arena.copy()).cuda()
    t = lambda a: torch.from_numpy(a.astype(np.int64)).cuda().to(torch.int32)
    p, e, c, s = t(pos), t(end), t(cap), t(sess)
    er = torch.full((len(pos),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc, tk, keep = P.device_batch_dev_async(
        opname, sessions, dev.data_ptr(), arena.nbytes, p.data_ptr(),
        e.data_ptr(), c.data_ptr(), er.data_ptr(), len(pos), s.data_ptr())
    assert rc == 0
    assert P.batch_wait(tk) == 0, P.lib().srtp_gpu_error()
    torch.cuda.synchronize()
    u32 = lambda x: x.cpu().numpy().view(np.uint32)
    return dev.cpu().numpy(), u32(p), u32(e), er.cpu().numpy()


_sent = {}


def sent(torch, suite, s0, per, jump=0):
    """pk[s][k]: session s's packet of sequence number s0[s] + k (64-byte
    payload, SSRC 0x7000 + s), k < per[s], protected in order on the device;
    jump: added to session 0's sequence numbers from half way on.  Computed
    once per (suite, s0, per, jump) and shared"""
    key = (suite, tuple(s0), tuple(per), jump)
    if key not in _sent:
        rng = np.random.default_rng(suite + 17 * len(per))
        seq = lambda s, k: s0[s] + k + \
            (jump if s == 0 and k >= per[0] // 2 else 0)
        plain = [(s, rtp_packet(rng, seq(s, k) & 0xffff, 0x7000 + s,
                                plen=64))
                 for k in range(max(per)) for s in range(len(per))
                 if k < per[s]]
        arena, pos, end, cap, sess = to_arena(plain)
        tx = [P.Srtp(suite, k) for k in keys_for(suite, len(per))]
        enc = run_dev(torch, "srtp_encrypt", tx, arena, pos, end, cap, sess)
        assert not enc[3].any()
        for c in tx:
            c.close()
        pk = [[] for _ in per]
        for i, (s, _) in enumerate(plain):
            pk[s].append(enc[0][pos[i]:enc[2][i]].tobytes())
        _sent[key] = pk
    return _sent[key]


def interleave(rng, pk, orders):
    """[(session, packet)]: session s's arrivals pk[s][k] for k in
    orders[s], the sessions interleaved at random"""
    owner = np.repeat(np.arange(len(orders)), [len(o) for o in orders])
    at = [0] * len(orders)
    out = []
    for s in rng.permutation(owner).tolist():
        out.append((s, pk[s][orders[s][at[s]]]))
        at[s] += 1
    return out


def oracle(suite, nsess, batches):
    """the oracle receiver, one context per session, over the batches in
    turn, one call per packet: per batch [(errno, pos, end, bytes)], and
    every session's final (roc, s_l, lix, bitmap) (None: no packet)"""
    be = O.OracleBackend()
    ctx = []
    for k in keys_for(suite, nsess):
        c, err = be.alloc(suite, k, 0)
        assert err == 0
        ctx.append(c)
    out, seen = [], set()
    for pkts in batches:
        rows = []
        for s, p in pkts:
            e, po, en, _, buf = be.call(ctx[s], "srtp_decrypt", len(p) + 64,
                                        0, len(p), p, len(p))
            rows.append((e, po, en, buf))
            seen.add(s)
        out.append(rows)
    fin = [be.export(ctx[s], 0x7000 + s) if s in seen else None
           for s in range(nsess)]
    for c in ctx:
        be.free(c)
    return out, fin


def check(torch, suite, entry, nsess, batches, truth=None):
    """unprotect the batches in turn through `entry`; each must equal the
    same call under norxplan and the oracle.  Returns every batch's counter
    deltas and the last batch's errnos."""
    keys = keys_for(suite, nsess)
    rxa = [P.Srtp(suite, k) for k in keys]
    rxb = [P.Srtp(suite, k) for k in keys]
    call = run_dev if entry == "dev" else run_async
    rows, fin = truth or oracle(suite, nsess, batches)
    deltas = []
    for bi, pkts in enumerate(batches):
        arena, pos, end, cap, sess = to_arena(pkts)
        c0 = {c: P.counter(c) for c in COUNTERS}
        da = call(torch, "srtp_decrypt", rxa, arena, pos, end, cap, sess)
        deltas.append({c: P.counter(c) - c0[c] for c in COUNTERS})
        with P.tune(norxplan=1):
            r0 = P.counter("mrxplans")
            db = call(torch, "srtp_decrypt", rxb, arena, pos, end, cap, sess)
            assert P.counter("mrxplans") == r0
        for x, y, what in zip(da, db, ("arena", "pos", "end", "err")):
            assert (x == y).all(), (bi, what, np.flatnonzero(x != y)[:8])
        ea = np.array([r[0] for r in rows[bi]], dtype=np.int32)
        assert (da[3] == ea).all(), (bi, np.flatnonzero(da[3] != ea)[:8])
        for i, ((s, p), (e, po, en, buf)) in enumerate(zip(pkts, rows[bi])):
            got = (int(da[1][i] - pos[i]), int(da[2][i] - pos[i]))
            assert got == (po, en), (bi, i, s, got, (e, po, en))
            assert da[0][pos[i]:pos[i] + len(buf)].tobytes() == buf, (bi, i)
    sa = states(rxa)
    assert sa == states(rxb)
    for s, f in enumerate(fin):
        if f is not None:
            roc, s_l, _, bitmap, lix = sa[s]
            assert (roc, s_l, lix, bitmap) == f, (s, sa[s], f)
    for c in rxa + rxb:
        c.close()
    return deltas, da[3]


def reshaped(rng, n, loss=0.03, swap=0.05, move=0.03, dup=0.02):
    """arrival order of n sent packets (network_shaped of
    tests/test_gpu_rxplan.py with higher rates, the sessions being short):
    loss, adjacent swaps, displacement by up to 8, duplicates of one of the
    last 32 arrivals"""
    a = [k for k in range(n) if rng.random() >= loss] or [0]
    i = 0
    while i + 1 < len(a):
        if rng.random() < swap:
            a[i], a[i + 1] = a[i + 1], a[i]
            i += 1
        i += 1
    for k in np.flatnonzero(rng.random(len(a)) < move)[::-1]:
        x = a.pop(int(k))
        a.insert(min(len(a), int(k) + int(rng.integers(1, 9))), x)
    out = []
    for x in a:
        out.append(x)
        if rng.random() < dup:
            out.append(out[-int(rng.integers(1, min(32, len(out)) + 1))])
    return out


def start_seqs(seed, nsess=NSESS):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(1000, 60000, nsess)]


_net = {}


def net_case(torch, suite):
    """600 sessions x 20 packets, every session reshaped; the batch and its
    oracle truth (shared by the entries)"""
    if suite not in _net:
        per = [20] * NSESS
        pk = sent(torch, suite, start_seqs(1), per)
        rng = np.random.default_rng(4242 + suite)
        arr = interleave(rng, pk, [reshaped(rng, 20) for _ in per])
        _net[suite] = (arr, oracle(suite, NSESS, [arr]))
    return _net[suite]


@pytest.mark.parametrize("entry", ["dev", "async"])
@pytest.mark.parametrize("suite", [1, 3, 5])
def test_network_shaped(suite, entry, torch_cuda):
    arr, truth = net_case(torch_cuda, suite)
    (d,), errs = check(torch_cuda, suite, entry, NSESS, [arr], truth)
    assert d["mrxplans"] == 1 and d["rejects"] == 1 and d["folds"] == 0, d
    assert d["mplans"] == 0 and d["rxplans"] == 0, d
    assert {int(e) for e in errs} == {0, errno.EALREADY}
    assert d["rxdups"] == int((errs == errno.EALREADY).sum())
    assert d["rxlate"] > 0


def swapped(n, i):
    a = list(range(n))
    a[i], a[i + 1] = a[i + 1], a[i]
    return a


# (the reshaped session, its arrivals of 10 sent packets, the silent
# sessions, EALREADY verdicts expected)
EDGES = {
    "swap_first": (300, swapped(10, 0), (), 0),
    "swap_last": (300, swapped(10, 8), (), 0),
    # five of its own arrivals back: ~3000 arrivals of the batch between
    "dup_5_back": (300, [0, 1, 2, 3, 4, 5, 6, 7, 3, 8, 9], (), 1),
    # 600 sessions: the last bucket is part-full whatever its width
    "last_session": (NSESS - 1, swapped(10, 4), (), 0),
    # the buckets of sessions 128..255 are empty (width 64 or 128)
    "after_empty_bucket": (256, swapped(10, 4), range(128, 256), 0),
    "before_empty_bucket": (127, [0, 1, 2, 2, 3, 4, 5, 6, 7, 8, 9],
                            range(128, 256), 1),
}


@pytest.mark.parametrize("shape", sorted(EDGES))
@pytest.mark.parametrize("suite", [1, 5])
def test_segment_edges(suite, shape, torch_cuda):
    """one reshaped session among in-order ones"""
    x, order, silent, dups = EDGES[shape]
    per = [10] * NSESS
    pk = sent(torch_cuda, suite, start_seqs(2), per)
    orders = [[] if s in silent else list(range(10)) for s in range(NSESS)]
    orders[x] = order
    rng = np.random.default_rng(len(shape) + suite)
    (d,), errs = check(torch_cuda, suite, "dev", NSESS,
                       [interleave(rng, pk, orders)])
    assert d["mrxplans"] == 1 and d["rejects"] == 1 and d["folds"] == 0, d
    assert int((errs == errno.EALREADY).sum()) == dups == d["rxdups"]


@pytest.mark.parametrize("suite", [1, 5])
def test_single_packet_duplicate_of_previous_batch(suite, torch_cuda):
    """batch 2 holds one packet of session 300: its last one of batch 1"""
    per = [10] * NSESS
    pk = sent(torch_cuda, suite, start_seqs(2), per)
    rng = np.random.default_rng(77 + suite)
    b1 = interleave(rng, pk, [list(range(5)) for _ in per])
    o2 = [list(range(5, 10)) for _ in per]
    o2[300] = [4]
    d, errs = check(torch_cuda, suite, "dev", NSESS,
                    [b1, interleave(rng, pk, o2)])
    assert d[0]["mplans"] == 1 and d[0]["mrxplans"] == 0, d
    assert d[1]["mrxplans"] == 1 and d[1]["rejects"] == 1, d
    assert int((errs == errno.EALREADY).sum()) == 1 == d[1]["rxdups"]


@pytest.mark.parametrize("suite", [1, 5])
def test_continuing_state(suite, torch_cuda):
    """batch 1 in order (ten sessions with 70 packets, session 599 silent);
    batch 2 replays the packets 1, 30 and 63 below each of those ten
    sessions' tops among new ones, and brings session 599's first packet
    twice"""
    per = [80 if s < 10 else 20 for s in range(NSESS)]
    pk = sent(torch_cuda, suite, start_seqs(3), per)
    rng = np.random.default_rng(99 + suite)
    o1 = [list(range(70 if s < 10 else 10)) for s in range(NSESS)]
    o1[NSESS - 1] = []
    o2 = [list(range(70, 80)) if s < 10 else list(range(10, 20))
          for s in range(NSESS)]
    for s in range(10):
        o2[s].insert(7, 69 - 1)
        o2[s].insert(3, 69 - 30)
        o2[s].insert(0, 69 - 63)
    o2[NSESS - 1] = [0, 0] + list(range(1, 10))
    b2 = interleave(rng, pk, o2)
    d, errs = check(torch_cuda, suite, "dev", NSESS,
                    [interleave(rng, pk, o1), b2])
    assert d[0]["mplans"] == 1 and d[0]["mrxplans"] == 0 and \
        d[0]["rejects"] == 0, d
    assert d[1]["mrxplans"] == 1 and d[1]["rejects"] == 1 and \
        d[1]["folds"] == 0, d
    # the duplicates are exactly the replays: the second copy of each
    want, seen = [], set()
    for i, (s, p) in enumerate(b2):
        if (s < 10 and p in (pk[s][68], pk[s][39], pk[s][6])) or \
                (s, p) in seen:
            want.append(i)
        seen.add((s, p))
    assert len(want) == 31
    assert np.flatnonzero(errs == errno.EALREADY).tolist() == want
    assert d[1]["rxdups"] == 31


@pytest.mark.parametrize("suite", [1, 5])
def test_rollover_inside_reshaped_sessions(suite, torch_cuda):
    """twenty sessions start at 65500 and roll over at their 37th packet,
    with swaps on either side of the rollover (none across it)"""
    s0 = [65500 if s < 20 else 2000 + s for s in range(NSESS)]
    per = [60 if s < 20 else 10 for s in range(NSESS)]
    pk = sent(torch_cuda, suite, s0, per)
    orders = [list(range(n)) for n in per]
    for s in range(20):
        a = orders[s]
        for i in (10 + s, 40 + s % 15):
            a[i], a[i + 1] = a[i + 1], a[i]
    rng = np.random.default_rng(5 + suite)
    (d,), errs = check(torch_cuda, suite, "dev", NSESS,
                       [interleave(rng, pk, orders)])
    assert not errs.any()
    assert d["mrxplans"] == 1 and d["rejects"] == 1 and d["folds"] == 0, d
    assert d["rxlate"] == 40


def late(n, k, d):
    a = list(range(n))
    a.insert(k + d, a.pop(k))
    return a


@pytest.mark.parametrize("case", ["dup_200", "pre_wrap_late", "jump_40000"])
def test_falls_back_still_exact(case, torch_cuda):
    """what the rule leaves unsettled in one session runs on the host engine
    as before"""
    suite = 1
    s0 = start_seqs(4)
    per = [10] * NSESS
    if case == "dup_200":
        # session 0: a copy of its top packet 200 of its own arrivals after
        # it, the arrivals between (copies of the ten packets below it) not
        # moving the top
        per[0] = 100
        pk = sent(torch_cuda, suite, s0, per)
        o0 = list(range(51)) + [40 + j % 10 for j in range(199)] + [50] + \
            list(range(51, 100))
    elif case == "pre_wrap_late":
        # session 0 rolls over at its 37th packet; the one sent 31st arrives
        # after the 46th
        s0[0], per[0] = 65500, 60
        pk = sent(torch_cuda, suite, s0, per)
        o0 = late(60, 30, 15)
    else:
        # session 0 jumps forward by 40000 half way
        s0[0], per[0] = 100, 40
        pk = sent(torch_cuda, suite, s0, per, jump=40000)
        o0 = list(range(40))
    orders = [list(range(n)) for n in per]
    orders[0] = o0
    rng = np.random.default_rng(13)
    (d,), errs = check(torch_cuda, suite, "dev", NSESS,
                       [interleave(rng, pk, orders)])
    assert d["mrxplans"] == 0 and d["rejects"] == 1, d
    codes = {int(e) for e in errs}
    assert codes == {"dup_200": {0, errno.EALREADY},
                     "pre_wrap_late": {0, errno.ETIMEDOUT},
                     "jump_40000": {0, errno.ETIMEDOUT}}[case]


@pytest.mark.parametrize("suite", [1, 5])
def test_forged_and_reordered(suite, torch_cuda):
    """three forged packets in the network shape: the planner's crypto
    launch counts the misses, the batch is undone and folds on the host"""
    arr, _ = net_case(torch_cuda, suite)
    arr = list(arr)
    for i in (700, 5600, 11100):
        q = bytearray(arr[i][1])
        q[20] ^= 0x10
        arr[i] = (arr[i][0], bytes(q))
    (d,), errs = check(torch_cuda, suite, "dev", NSESS, [arr])
    assert d["folds"] >= 1 and d["mrxplans"] == 0, d
    # (check() compared every errno with the oracle's)
    assert [int(errs[i]) for i in (700, 5600, 11100)] == [P.EAUTH] * 3


@pytest.mark.parametrize("suite", [1, 5])
def test_in_order_batch_keeps_its_path(suite, torch_cuda):
    per = [10] * NSESS
    pk = sent(torch_cuda, suite, start_seqs(2), per)
    rng = np.random.default_rng(3)
    (d,), errs = check(torch_cuda, suite, "dev", NSESS,
                       [interleave(rng, pk, [list(range(10)) for _ in per])])
    assert not errs.any()
    assert d["mplans"] == 1 and d["rejects"] == 0 and d["mrxplans"] == 0, d
