"""GPU tests of the device receive planner (re_amd/csrc/hip/plan_rx.hip,
batch_dev.c dev_rxplanned): a one-stream unprotect batch that arrives
reordered, duplicated or with gaps is planned exactly on the device behind
the in-order planners' rejection.

Every case protects N packets in order, reshapes the arrival order and
unprotects.  Arena, pos, end, err and the exported stream state must equal
those of the same call with the planner off (srtp_gpu_tune norxplan: the
host engine) and those of the oracle receiver called one packet at a time;
the counters say which path produced them ("rxplans": this planner).
"""
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import oracle_lib as O
from tests.test_gpu_fastpath import (keys_for, rtp_packet, run, run_dev,
                                     states, to_arena)

pytestmark = pytest.mark.gpu

N = 5000
SSRC = 0x7a7a
COUNTERS = ("rxplans", "rejects", "folds", "fused", "lplans", "rxlate",
            "rxdups")


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def run_async(torch, opname, sessions, arena, pos, end, cap, sess):
    """srtp_*_batch_dev_async + srtp_batch_wait, arrays in HBM"""
    dev = torch.from_numpy(arena.copy()).cuda()
    t = lambda a: torch.from_numpy(a.astype(np.int64)).cuda().to(torch.int32)
    p, e, c = t(pos), t(end), t(cap)
    er = torch.full((len(pos),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc, tk, keep = P.device_batch_dev_async(
        opname, sessions, dev.data_ptr(), arena.nbytes, p.data_ptr(),
        e.data_ptr(), c.data_ptr(), er.data_ptr(), len(pos))
    assert rc == 0
    assert P.batch_wait(tk) == 0, P.lib().srtp_gpu_error()
    torch.cuda.synchronize()
    u32 = lambda x: x.cpu().numpy().view(np.uint32)
    return dev.cpu().numpy(), u32(p), u32(e), er.cpu().numpy()


def unprotect(torch, entry, rx, pkts):
    arena, pos, end, cap, _ = to_arena([(0, p) for p in pkts])
    if entry == "dev":
        r = run_dev(torch, "srtp_decrypt", [rx], arena, pos, end, cap, None)
    elif entry == "host":
        r = run(torch, "srtp_decrypt", [rx], arena, pos, end, cap, None,
                False)
    else:
        r = run_async(torch, "srtp_decrypt", [rx], arena, pos, end, cap,
                      None)
    return r, pos


_sent = {}


def sent(torch, suite, seqs):
    """the packets of sequence numbers seqs (64-byte payload), protected in
    order on the device; computed once per (suite, seqs) and shared"""
    k = (suite, seqs[0], len(seqs), seqs[-1])
    if k not in _sent:
        rng = np.random.default_rng(suite + seqs[0])
        pk = [(0, rtp_packet(rng, s & 0xffff, SSRC, plen=64)) for s in seqs]
        arena, pos, end, cap, _ = to_arena(pk)
        tx = P.Srtp(suite, keys_for(suite, 1)[0])
        enc = run(torch, "srtp_encrypt", [tx], arena, pos, end, cap, None,
                  False)
        assert not enc[3].any()
        tx.close()
        _sent[k] = [enc[0][pos[i]:enc[2][i]].tobytes()
                    for i in range(len(pk))]
    return _sent[k]


def oracle(suite, batches):
    """the oracle receiver over the batches in turn, one call per packet:
    per batch [(errno, pos, end, bytes)], and its final state"""
    be = O.OracleBackend()
    ctx, err = be.alloc(suite, keys_for(suite, 1)[0], 0)
    assert err == 0
    out = []
    for pkts in batches:
        rows = []
        for p in pkts:
            e, po, en, _, buf = be.call(ctx, "srtp_decrypt", len(p) + 64, 0,
                                        len(p), p, len(p))
            rows.append((e, po, en, buf))
        out.append(rows)
    fin = be.export(ctx, SSRC)
    be.free(ctx)
    return out, fin


def check(torch, suite, entry, batches, truth=None):
    """unprotect the batches in turn through `entry`; each must equal the
    same call under norxplan and the oracle.  Returns the last batch's
    counter deltas and errnos."""
    key = keys_for(suite, 1)[0]
    rxa, rxb = P.Srtp(suite, key), P.Srtp(suite, key)
    rows, fin = truth or oracle(suite, batches)
    for bi, pkts in enumerate(batches):
        c0 = {c: P.counter(c) for c in COUNTERS}
        da, pos = unprotect(torch, entry, rxa, pkts)
        delta = {c: P.counter(c) - c0[c] for c in COUNTERS}
        with P.tune(norxplan=1):
            r0 = P.counter("rxplans")
            db, _ = unprotect(torch, entry, rxb, pkts)
            assert P.counter("rxplans") == r0
        for x, y, what in zip(da, db, ("arena", "pos", "end", "err")):
            assert (x == y).all(), (bi, what, np.flatnonzero(x != y)[:8])
        assert states([rxa], [SSRC]) == states([rxb], [SSRC])
        for i, (p, (e, po, en, buf)) in enumerate(zip(pkts, rows[bi])):
            got = (int(da[3][i]), int(da[1][i] - pos[i]),
                   int(da[2][i] - pos[i]))
            assert got == (e, po, en), (bi, i, got, (e, po, en))
            assert da[0][pos[i]:pos[i] + len(buf)].tobytes() == buf, (bi, i)
    e, st = rxa.export(SSRC)
    assert e == 0
    assert (st.roc, st.s_l, st.replay_rtp_lix, st.replay_rtp_bitmap) == fin
    rxa.close()
    rxb.close()
    return delta, da[3]


def network_shaped(rng, n):
    """arrival order of n sent packets: 1 % loss, 2 % adjacent swaps, 1 %
    displaced by up to 8, 0.5 % duplicates of one of the last 32 arrivals"""
    a = [k for k in range(n) if rng.random() >= 0.01]
    i = 0
    while i + 1 < len(a):
        if rng.random() < 0.02:
            a[i], a[i + 1] = a[i + 1], a[i]
            i += 1
        i += 1
    for k in np.flatnonzero(rng.random(len(a)) < 0.01)[::-1]:
        x = a.pop(int(k))
        a.insert(min(len(a), int(k) + int(rng.integers(1, 9))), x)
    out = []
    for x in a:
        out.append(x)
        if rng.random() < 0.005:
            out.append(out[-int(rng.integers(1, min(32, len(out)) + 1))])
    return out


_net = {}


def net_case(torch, suite):
    """the network-shaped batch of a suite and its oracle truth (shared by
    the three entries)"""
    if suite not in _net:
        pk = sent(torch, suite, list(range(100, 100 + N)))
        order = network_shaped(np.random.default_rng(4242), N)
        arr = [pk[k] for k in order]
        _net[suite] = (arr, oracle(suite, [arr]))
    return _net[suite]


@pytest.mark.parametrize("entry", ["dev", "host", "async"])
@pytest.mark.parametrize("suite", [1, 0, 2, 4, 5])
def test_network_shaped(suite, entry, torch_cuda):
    arr, truth = net_case(torch_cuda, suite)
    d, errs = check(torch_cuda, suite, entry, [arr], truth)
    assert d["rxplans"] == 1 and d["rejects"] == 1 and d["folds"] == 0, d
    assert {int(e) for e in errs} == {0, errno.EALREADY}
    assert d["rxdups"] == int((errs == errno.EALREADY).sum())
    assert d["rxlate"] > 0


def swapped(n, i):
    a = list(range(n))
    a[i], a[i + 1] = a[i + 1], a[i]
    return a


BOUNDARY = {
    "swap_1023_1024": lambda: swapped(N, 1023),
    "swap_last": lambda: swapped(N, N - 2),
    "swap_first": lambda: swapped(N, 0),
    # the original is the last packet of the 256-packet block before, and
    # one five arrivals back across the 1024 boundary
    "dup_prev_block": lambda: list(range(256)) + [255] +
    list(range(256, 1024)) + [1020] + list(range(1024, N)),
}


@pytest.mark.parametrize("shape", sorted(BOUNDARY))
@pytest.mark.parametrize("suite", [1, 5])
def test_boundaries(suite, shape, torch_cuda):
    pk = sent(torch_cuda, suite, list(range(100, 100 + N)))
    arr = [pk[k] for k in BOUNDARY[shape]()]
    d, errs = check(torch_cuda, suite, "dev", [arr])
    assert d["rxplans"] == 1 and d["folds"] == 0, d
    want = 2 if shape == "dup_prev_block" else 0
    assert int((errs == errno.EALREADY).sum()) == want == d["rxdups"]


@pytest.mark.parametrize("suite", [1, 5])
def test_continuing_state(suite, torch_cuda):
    """batch 1 in order; batch 2 replays five of its last 64 packets among
    new ones"""
    pk = sent(torch_cuda, suite, list(range(100, 100 + N)))
    h = N // 2
    b2 = list(range(h, N))
    for at, k in ((2000, h - 1), (1500, h - 64), (700, h - 30), (3, h - 2),
                  (0, h - 7)):
        b2.insert(at, k)
    d, errs = check(torch_cuda, suite, "dev",
                    [pk[:h], [pk[k] for k in b2]])
    assert d["rxplans"] == 1 and d["rejects"] == 1 and d["folds"] == 0, d
    assert int((errs == errno.EALREADY).sum()) == 5 == d["rxdups"]


def late(n, k, d):
    a = list(range(n))
    a.insert(k + d, a.pop(k))
    return a


@pytest.mark.parametrize("case", ["pre_wrap_late", "jump_40000", "dup_200"])
def test_falls_back_still_exact(case, torch_cuda):
    """what the rule leaves unsettled runs on the host engine as before"""
    suite = 1
    if case == "pre_wrap_late":
        # s0 = 65000 rolls over at position 536
        pk = sent(torch_cuda, suite, list(range(65000, 65000 + N)))
        arr = [pk[k] for k in late(N, 530, 15)]
    elif case == "jump_40000":
        seqs = [100 + k + (40000 if k >= N // 2 else 0) for k in range(N)]
        arr = sent(torch_cuda, suite, seqs)
    else:
        # a copy of the top packet 200 arrivals after it, the arrivals
        # between (copies of the ten packets below it) not moving the top
        pk = sent(torch_cuda, suite, list(range(100, 100 + N)))
        order = list(range(1001)) + [990 + j % 10 for j in range(199)] + \
            [1000] + list(range(1001, N))
        arr = [pk[k] for k in order]
    d, errs = check(torch_cuda, suite, "dev", [arr])
    assert d["rxplans"] == 0 and d["rejects"] == 1, d
    codes = {int(e) for e in errs}
    assert codes == {"pre_wrap_late": {0, errno.ETIMEDOUT},
                     "jump_40000": {0, errno.ETIMEDOUT},
                     "dup_200": {0, errno.EALREADY}}[case]


@pytest.mark.parametrize("entry", ["dev", "host"])
@pytest.mark.parametrize("suite", [1, 5])
def test_forged_and_reordered(suite, entry, torch_cuda):
    """three forged packets in the network shape: the planner's crypto
    launch counts the misses, the batch is undone and folds on the host"""
    arr, _ = net_case(torch_cuda, suite)
    arr = list(arr)
    for i in (700, 2600, 4100):
        q = bytearray(arr[i])
        q[20] ^= 0x10
        arr[i] = bytes(q)
    f0 = P.counter("folds")
    d, errs = check(torch_cuda, suite, entry, [arr])
    assert d["folds"] >= 1 and P.counter("folds") > f0
    assert d["rxplans"] == 0
    assert int((errs == P.EAUTH).sum()) >= 3


@pytest.mark.parametrize("suite", [1, 5])
def test_in_order_batch_keeps_its_path(suite, torch_cuda):
    pk = sent(torch_cuda, suite, list(range(100, 100 + N)))
    d, errs = check(torch_cuda, suite, "dev", [pk])
    assert not errs.any()
    assert d["rxplans"] == 0 and d["rejects"] == 0
    assert d["fused"] + d["lplans"] == 1
