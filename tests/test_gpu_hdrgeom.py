"""Header geometry: every header class and headers past one 64-byte chunk
through the device planners, the per-call paths and the mbuf batch, bit-exact
against the oracle (tests/oracle_lib.py, pinned to the reference by the
golden scenarios srtp_header_shapes_s*) called one packet at a time.

Every crypto kernel specialises on the RTP header length hl (rtp_hdr_decode,
src/rtp/rtp.c:88-137: 12 + 4*CC, plus 4 + 4*length with X set): the class
(hl >> 2) & 3 picks the SHIFT template argument, and hl splits the walk over
64-byte chunks into head, steady and tail chunks (k_ctr_fast.h kf0 / cw4,
k_ctr_fused.h, k_ctr.h, small.hip, the AAD walk of gcm.hip).  The header
lengths here are 12..92, 124..140 and 252..268 in steps of 4: about eight per
class, with headers of one to five chunks, CSRCs alone up to 72
bytes and CC = 15 plus an extension above (28 and 76 also as CC = 0 plus an
extension, on odd payload lengths).

Batches: one per class, its header lengths times every payload length
0..140, sequence numbers from 65000 (the ROC rolls over inside), in two
orders -- "payload": the four packets of a quad hold four header lengths
(lanes of one quad with different head chunk counts); "header": a quad holds
one header length and four consecutive payload lengths.  Unprotect takes the
oracle's protected packets, about 1 % of them forged in the payload or the
tag.  Which planner and kernel ran is asserted by the counters of
srtp_gpu_counter: without that a fallback to the host engine would pass the
byte comparison.  No planner rejects a long header: every path accepts every
batch here.

Compared with the oracle: errno, pos and end relative to the packet, every
byte the oracle leaves (unprotect: the tag region included, srtp.c:342-344),
and the exported stream states (roc, s_l, replay window).
"""
import ctypes
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import oracle_lib as O
from tests.test_gpu_fastpath import keys_for, run_dev, states, to_arena

pytestmark = pytest.mark.gpu

HLS = list(range(12, 93, 4)) + list(range(124, 141, 4)) + \
    list(range(252, 269, 4))
SHAPES = [(hl, False) for hl in HLS] + [(28, True), (76, True)]
ORDERS = ("payload", "header")
GCM = (4, 5)
SSRC = 0x68647267
NSESS = 130             # two buckets of the bucket planner
S0 = 65000
S0_MANY = 65532         # every session rolls over at its fifth packet


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


def header_shape(hl, alt=False):
    """(CC, extension words or None) of a header of hl bytes; alt: CC = 0
    and the extension alone"""
    if alt:
        return 0, (hl - 16) // 4
    if hl <= 72:
        return (hl - 12) // 4, None
    return 15, (hl - 76) // 4


def rtp_packet(rng, seq, ssrc, hl, plen, alt=False):
    cc, xw = header_shape(hl, alt)
    b = bytearray([0x80 | (0x10 if xw is not None else 0) | cc,
                   int(rng.integers(0, 256)), (seq >> 8) & 0xff, seq & 0xff])
    b += int(rng.integers(0, 1 << 32)).to_bytes(4, "big")
    b += ssrc.to_bytes(4, "big")
    b += rng.integers(0, 256, 4 * cc, dtype=np.uint8).tobytes()
    if xw is not None:
        b += b"\xbe\xde" + xw.to_bytes(2, "big")
        b += rng.integers(0, 256, 4 * xw, dtype=np.uint8).tobytes()
    assert len(b) == hl
    b += rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
    return bytes(b)


def class_of(hl):
    return (hl >> 2) & 3


def layout(cls, order):
    """[(hl, plen)] of class cls's batch"""
    H = [h for h in HLS if class_of(h) == cls]
    if order == "payload":
        # rotated per row, so that the sessions of the round-robin deal see
        # every header length too
        return [(H[(j + plen) % len(H)], plen) for plen in range(141)
                for j in range(len(H))]
    return [(hl, plen) for hl in H for plen in range(141)]


def forge(prot, lay, cand):
    """about 1 % of the packets of cand forged, in the payload and in the
    tag in turn (a packet without payload: in the tag); returns the batch
    and the forged indices"""
    idx = cand[5::89]
    out = list(prot)
    for k, i in enumerate(idx):
        hl, plen = lay[i]
        q = bytearray(out[i])
        at = hl + plen // 2 if (k % 2 == 0 and plen) else len(q) - 1 - k % 4
        q[at] ^= 0x10
        out[i] = bytes(q)
    assert sum(lay[i][0] >= 64 for i in idx) >= 2
    assert len(idx) >= len(prot) // 120
    return out, idx


def oracle_rows(be, ctx, op, pkts):
    """[(errno, pos, end, bytes)] of the packets through ctx[s] in turn"""
    rows = []
    for s, p in pkts:
        if op == "srtp_encrypt":
            e, po, en, _, buf = be.call(ctx[s], op, len(p) + 64, 0, len(p), p,
                                        len(p) + 16)
        else:
            e, po, en, _, buf = be.call(ctx[s], op, len(p) + 64, 0, len(p), p,
                                        len(p))
        rows.append((e, po, en, buf))
    return rows


_ref = {}


def reference(suite, cls, order, many):
    """the class's batch and the oracle's results, computed once and shared:
    plain and received packets [(session, bytes)], the oracle's rows for
    both, the forged indices and every session's (roc, s_l, lix, bitmap)
    after protect and after unprotect"""
    key = (suite, cls, order, many)
    if key in _ref:
        return _ref[key]
    lay = layout(cls, order)
    rng = np.random.default_rng(7000 + 100 * suite + 10 * cls +
                                ORDERS.index(order) + (5 if many else 0))
    nsess = NSESS if many else 1
    nxt = [S0_MANY if many else S0] * nsess
    plain = []
    for i, (hl, plen) in enumerate(lay):
        s = i % nsess           # dealt round-robin, each session in order
        plain.append((s, rtp_packet(rng, nxt[s] & 0xffff,
                                    0x7000 + s if many else SSRC, hl, plen,
                                    alt=hl in (28, 76) and plen % 2 == 1)))
        nxt[s] += 1
    be = O.OracleBackend()
    keys = keys_for(suite, nsess)
    ssrc = [0x7000 + s if many else SSRC for s in range(nsess)]
    tx = [be.alloc(suite, k, 0)[0] for k in keys]
    rx = [be.alloc(suite, k, 0)[0] for k in keys]
    enc = oracle_rows(be, tx, "srtp_encrypt", plain)
    assert all(r[0] == 0 for r in enc)
    prot = [r[3][:r[2]] for r in enc]
    # a forged packet that rolls the ROC over leaves roc + 1 behind
    # (srtp.c:318-321 runs before the tag check); the many-session fold
    # hands such a batch to the host (tests/test_gpu_buckets.py), so the
    # many-session batches keep their forged packets off seq 0
    cand = [i for i, (_, p) in enumerate(plain)
            if not many or p[2:4] != b"\x00\x00"]
    recv, forged = forge(prot, lay, cand)
    recv = [(s, q) for (s, _), q in zip(plain, recv)]
    dec = oracle_rows(be, rx, "srtp_decrypt", recv)
    # every unforged packet returns 0, every forged one EAUTH
    assert [i for i, r in enumerate(dec) if r[0]] == sorted(forged)
    assert all(dec[i][0] == P.EAUTH for i in forged)
    res = {"lay": lay, "plain": plain, "recv": recv, "enc": enc, "dec": dec,
           "forged": forged, "ssrc": ssrc, "keys": keys,
           "tx_state": [be.export(c, x) for c, x in zip(tx, ssrc)],
           "rx_state": [be.export(c, x) for c, x in zip(rx, ssrc)]}
    for c in tx + rx:
        be.free(c)
    _ref[key] = res
    return res


def same_as_oracle(out, pos, rows, prot, what):
    """errno, pos / end relative to the packet and the oracle's bytes, of
    every packet"""
    arena, p, e, err = out
    assert len(rows) == len(pos)
    for i, (we, wpo, wen, buf) in enumerate(rows):
        got = (int(err[i]), int(p[i]) - int(pos[i]), int(e[i]) - int(pos[i]))
        assert got == (we, wpo, wen), (what, i, got, (we, wpo, wen))
        n = wen if prot else len(buf)
        assert arena[pos[i]:pos[i] + n].tobytes() == buf[:n], (what, i)


def product_states(sessions, ssrcs):
    """(roc, s_l, lix, bitmap) per session, as OracleBackend.export"""
    out = []
    for s, x in zip(sessions, ssrcs):
        (st,) = states([s], [x])
        assert len(st) == 5, (x, st)
        out.append((st[0], st[1], st[4], st[3]))
    return out


COUNTERS = ("fused", "lplans", "dplans", "mplans", "rejects", "devfolds",
            "folds", "rxplans", "mrxplans")


def counted(torch, call, knobs, *args, names=COUNTERS):
    """call(*args) under the knobs: (its result, the counters it moved)"""
    # every call from the same first-batch hint (tests/test_gpu_fused.py)
    P.lib().srtp_gpu_tune(b"freshmulti", 0)
    c0 = {c: P.counter(c) for c in names}
    with P.tune(**knobs):
        out = call(torch, *args)
    return out, {c: P.counter(c) - c0[c] for c in names}


def one_stream_paths(suite):
    """(path, tune knobs, the counter its accepted plan moves)"""
    return [("default", {}, "lplans" if suite in GCM else "fused"),
            ("lean", {"lplan": 1}, "lplans"),
            ("planner", {"noplanfuse": 1}, "dplans")]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("cls", range(4))
@pytest.mark.parametrize("suite", range(6))
def test_one_stream(suite, cls, order, torch_cuda):
    """k_ctr_fused (AES-CM default), k_ctr_fast_any / k_ctr_fast_refix
    (lplan) and the separate planner's launch; k_gcmu for the GCM suites"""
    R = reference(suite, cls, order, False)
    key = R["keys"][0]
    ea = to_arena(R["plain"])
    da = to_arena(R["recv"])
    for path, knobs, cname in one_stream_paths(suite):
        tx, rx = P.Srtp(suite, key), P.Srtp(suite, key)
        for op, ctx, a, rows, st in (
                ("srtp_encrypt", tx, ea, R["enc"], R["tx_state"]),
                ("srtp_decrypt", rx, da, R["dec"], R["rx_state"])):
            arena, pos, end, cap, _ = a
            out, d = counted(torch_cuda, run_dev, knobs, op, [ctx], arena,
                             pos, end, cap, None)
            # the forged batch too: misses folded behind an accepted plan
            assert d[cname] == 1 and d["rejects"] == 0, (path, op, d)
            same_as_oracle(out, pos, rows, op == "srtp_encrypt", (path, op))
            assert product_states([ctx], [SSRC]) == st, (path, op)
        tx.close()
        rx.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("cls", range(4))
@pytest.mark.parametrize("suite", range(6))
def test_many_sessions(suite, cls, order, torch_cuda):
    """k_ctr_fast_mk<10 / 14, protect / unprotect> in the class's SHIFT
    body, k_ctr_refix_list, the many-session GCM launch and the device
    verdict fold, behind the bucket planner and the counting planner"""
    R = reference(suite, cls, order, True)
    ea = to_arena(R["plain"])
    da = to_arena(R["recv"])
    for path, knobs in (("bucket", {}), ("count", {"nobucket": 1})):
        tx = [P.Srtp(suite, k) for k in R["keys"]]
        rx = [P.Srtp(suite, k) for k in R["keys"]]
        for op, ctx, a, rows, st, folds in (
                ("srtp_encrypt", tx, ea, R["enc"], R["tx_state"], 0),
                ("srtp_decrypt", rx, da, R["dec"], R["rx_state"], 1)):
            arena, pos, end, cap, sess = a
            out, d = counted(torch_cuda, run_dev, knobs, op, ctx, arena, pos,
                             end, cap, sess)
            assert {c: d[c] for c in ("mplans", "rejects", "devfolds",
                                      "folds")} == \
                {"mplans": 1, "rejects": 0, "devfolds": folds, "folds": 0}, \
                (path, op, d)
            same_as_oracle(out, pos, rows, op == "srtp_encrypt", (path, op))
            assert product_states(ctx, R["ssrc"]) == st, (path, op)
        for c in tx + rx:
            c.close()


@pytest.mark.parametrize("many", [False, True], ids=["one", "many"])
@pytest.mark.parametrize("suite", [1, 3, 5])
def test_receive_planners(suite, many, torch_cuda):
    """class 1 reordered, with a duplicate, at hl = 68: two arrivals of one
    stream swapped and the first of them delivered again five arrivals
    later (EALREADY) -- the device receive planners (plan_rx.hip,
    plan_buckets_rx.hip) behind the in-order planners' rejection"""
    R = reference(suite, 1, "payload", many)
    nsess = NSESS if many else 1
    arr = [(s, r[3][:r[2]]) for (s, _), r in zip(R["plain"], R["enc"])]
    lay = R["lay"]
    # past every rollover (one stream: arrival 536; many: a session's
    # fifth packet, arrivals 520..649)
    i = next(k for k in range(650, len(arr)) if lay[k][0] == 68)
    j = i + nsess               # the stream's next packet
    arr[i], arr[j] = arr[j], arr[i]
    dup = j + (60 if many else 5)
    assert dup < len(arr)
    arr.insert(dup, arr[j])
    be = O.OracleBackend()
    octx = [be.alloc(suite, k, 0)[0] for k in R["keys"]]
    rows = oracle_rows(be, octx, "srtp_decrypt", arr)
    want = [be.export(c, x) for c, x in zip(octx, R["ssrc"])]
    for c in octx:
        be.free(c)
    assert [k for k, r in enumerate(rows) if r[0]] == [dup]
    assert rows[dup][0] == errno.EALREADY
    rx = [P.Srtp(suite, k) for k in R["keys"]]
    arena, pos, end, cap, sess = to_arena(arr)
    out, d = counted(torch_cuda, run_dev, {}, "srtp_decrypt", rx, arena, pos,
                     end, cap, sess if many else None)
    assert d["mrxplans" if many else "rxplans"] == 1 and d["folds"] == 0, d
    same_as_oracle(out, pos, rows, False, "rx")
    assert product_states(rx, R["ssrc"]) == want
    for c in rx:
        c.close()


# ---- per-call and mbuf-batch API: unaligned mb->pos ------------------------

PLENS = (0, 1, 15, 16, 17, 63, 64, 65, 130)
POS = (0, 1, 2, 3, 5, 6, 7)
_pc = {}


def percall_reference(suite):
    """every header shape times PLENS, mb->pos cycling through POS, through
    the oracle: [(op, data, size, pos, (errno, pos, end, size, bytes))] for
    the sender and for the receiver (the protected packets at another
    offset, in a buffer with no room to spare)"""
    if suite in _pc:
        return _pc[suite]
    rng = np.random.default_rng(8100 + suite)
    key = keys_for(suite, 1)[0]
    be = O.OracleBackend()
    tx, rx = be.alloc(suite, key, 0)[0], be.alloc(suite, key, 0)[0]
    enc, dec = [], []
    cases = [(hl, alt, plen) for hl, alt in SHAPES for plen in PLENS]
    for i, (hl, alt, plen) in enumerate(cases):
        off = POS[i % len(POS)]
        data = bytes(off) + rtp_packet(rng, (65400 + i) & 0xffff, SSRC, hl,
                                       plen, alt)
        size = len(data) + 32
        r = be.call(tx, "srtp_encrypt", size, off, len(data), data, size)
        assert r[0] == 0
        enc.append(("srtp_encrypt", data, size, off, r))
        off2 = POS[(i + 3) % len(POS)]
        data2 = bytes(off2) + r[4][off:r[2]]
        r2 = be.call(rx, "srtp_decrypt", len(data2), off2, len(data2), data2,
                     len(data2))
        assert r2[0] == 0
        dec.append(("srtp_decrypt", data2, len(data2), off2, r2))
    be.free(tx)
    be.free(rx)
    _pc[suite] = (key, enc, dec)
    return _pc[suite]


def mbuf_result(e, mb):
    m = mb.contents
    return (e, m.pos, m.end, m.size, ctypes.string_at(m.buf, m.size))


def same_mbuf(got, want, what):
    assert got[:4] == want[:4], (what, got[:4], want[:4])
    assert got[4] == want[4], what


@pytest.mark.parametrize("path", ["small", "coop", "general"])
@pytest.mark.parametrize("suite", range(6))
def test_per_call_unaligned_pos(suite, path, torch_cuda):
    """srtp_encrypt / srtp_decrypt with any mb->pos (the staging copies of
    srtp.c), through the three per-call paths of test_per_call_golden"""
    key, enc, dec = percall_reference(suite)
    tx, rx = P.Srtp(suite, key), P.Srtp(suite, key)
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


@pytest.mark.parametrize("suite", range(6))
def test_mbuf_batch_unaligned_pos(suite, torch_cuda):
    """the same calls as one srtp_encrypt_mbufs and one srtp_decrypt_mbufs
    batch"""
    key, enc, dec = percall_reference(suite)
    tx, rx = P.Srtp(suite, key), P.Srtp(suite, key)
    for ctx, calls in ((tx, enc), (rx, dec)):
        mbs = [P.new_mbuf(data, size, off) for _, data, size, off, _ in calls]
        rc, errs = P.batch_run(ctx, calls[0][0], mbs)
        assert rc == 0
        for i, (mb, e, c) in enumerate(zip(mbs, errs, calls)):
            same_mbuf(mbuf_result(e, mb), c[4], (c[0], i, c[3]))
            P.free_mbuf(mb)
    tx.close()
    rx.close()


# ---- a misaligned window in a device batch ---------------------------------

def call_dev(torch, op, sessions, arena, pos, end, cap, sess):
    """srtp_*_batch_dev as run_dev, returning rc instead of asserting it"""
    dev = torch.from_numpy(arena.copy()).cuda()
    i32 = lambda a: torch.from_numpy(
        np.asarray(a, dtype=np.uint32).view(np.int32)).cuda()
    p, e, c = i32(pos), i32(end), i32(cap)
    s = i32(sess) if sess is not None else None
    er = torch.full((len(pos),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = P.device_batch_dev(op, sessions, dev.data_ptr(), arena.nbytes,
                            p.data_ptr(), e.data_ptr(), c.data_ptr(),
                            er.data_ptr(), len(pos),
                            s.data_ptr() if s is not None else None)
    torch.cuda.synchronize()
    return rc, dev.cpu().numpy()


@pytest.mark.parametrize("case", ["one_cm", "one_gcm", "many"])
def test_misaligned_window_rejected(case, torch_cuda):
    """one packet of a valid batch at pos % 4 == 2, wholly inside the arena
    and its capacity: the planners' window rule (plan_rule.h
    plan_window_flags, SPF_BAD) rejects the plan, the call returns EINVAL
    with nothing modified; the next valid batch on the same contexts is
    planned on the device again (the fused plan's ticket and look-back state
    restarts from zero behind SPF_BAD) and equals the oracle"""
    suite = 5 if case == "one_gcm" else 1
    many = case == "many"
    R = reference(suite, 1, "payload", many)
    arena, pos, end, cap, sess = to_arena(R["plain"])
    tx = [P.Srtp(suite, k) for k in R["keys"]]
    k = 777
    bad_arena, bad_pos, bad_end = arena.copy(), pos.copy(), end.copy()
    a, b = int(pos[k]), int(end[k])
    # to_arena leaves 80 bytes behind every packet and cap = end + 60
    bad_arena[a + 2:b + 2] = arena[a:b]
    bad_arena[a:a + 2] = 0
    bad_pos[k] += 2
    bad_end[k] += 2
    assert bad_pos[k] % 4 == 2 and bad_end[k] <= cap[k] <= arena.nbytes
    assert (bad_end <= arena.nbytes).all() and (cap <= arena.nbytes).all()
    (rc, after), d = counted(torch_cuda, call_dev, {}, "srtp_encrypt", tx,
                             bad_arena, bad_pos, bad_end, cap,
                             sess if many else None)
    assert rc == errno.EINVAL, rc
    assert (after == bad_arena).all()
    assert d["fused"] == d["lplans"] == d["mplans"] == d["dplans"] == 0, d
    # no stream was created
    assert all(len(st) == 1 for s, x in zip(tx, R["ssrc"])
               for st in states([s], [x]))
    out, d = counted(torch_cuda, run_dev, {}, "srtp_encrypt", tx, arena, pos,
                     end, cap, sess if many else None)
    assert d["mplans" if many else "lplans" if suite in GCM else "fused"] \
        == 1 and d["rejects"] == 0, d
    same_as_oracle(out, pos, R["enc"], True, case)
    assert product_states(tx, R["ssrc"]) == R["tx_state"]
    for c in tx:
        c.close()
