"""SRTCP packets of every byte length: the batches, the oracle's answers and
the comparisons tests/test_gpu_srtcp_geom.py shares between its routes.

The oracle (tests/oracle_lib.py) is pinned to the reference at these lengths
by tests/test_srtcp_geom_cpu.py; it is called one packet at a time, once per
(suite, flags, order, layout), and the result is cached and never modified.
Nothing here needs a GPU.
"""
import errno

import numpy as np

import re_amd.srtp as P
from tests import oracle_lib as O
from tests.test_gpu_fastpath import keys_for
from tests.test_gpu_srtcp import rtcp_packet

U = P.SRTP_UNENCRYPTED_SRTCP
FLAGS = (0, U)
LENS = range(8, 208)
ORDERS = ("run", "spread")
NSESS = 130             # two buckets of 128 under bpexp 1000
BPEXP = 1000
NMANY = 520
SSRC = 0x67656f31
SSRC3 = (0x67656f41, 0x67656f42, 0x67656f43)
# plaintext lengths whose E || index word straddles a 64-byte chunk on an
# HMAC unprotect (the cipher ends at L, the MAC at L + 4)
STRADDLE = [L for L in LENS if L % 64 in (61, 62, 63)]


def has_hmac(suite):
    return P.salt_len(suite) == 14


def growth(suite):
    """bytes srtcp_encrypt appends: E || index and the tag"""
    return 4 + (P.tag_len(suite) if has_hmac(suite) else 16)


def length_of(order, i):
    """packet i's length: "run" -- the lanes of a quad differ by one byte;
    "spread" -- neighbouring lanes differ in chunk count"""
    return LENS[i % 200] if order == "run" else LENS[(53 * i) % 200]


def packet(rng, ssrc, L):
    """an RTCP packet of L bytes; the header's length field is L // 4 - 1
    (the reference does not read it)"""
    p = rtcp_packet(rng, ssrc, L - 8)
    assert len(p) == L and int.from_bytes(p[2:4], "big") == L // 4 - 1
    return p


def layout(kind, order):
    """[(session, ssrc, length)] of a batch: "one" -- one stream, 200
    packets; "many" -- 130 sessions with one SSRC each, 520 packets dealt
    round-robin; "three" -- one session, three SSRCs interleaved, 600
    packets (200 % 3 == 2: every SSRC meets every length)"""
    if kind == "one":
        return [(0, SSRC, length_of(order, i)) for i in range(200)]
    if kind == "many":
        return [(i % NSESS, 0x6d000000 + i % NSESS, length_of(order, i))
                for i in range(NMANY)]
    assert kind == "three"
    return [(0, SSRC3[i % 3], length_of(order, i)) for i in range(600)]


def forge_at(suite, w, body):
    """the byte of the wire packet w to flip: the middle of the body (the
    tag, for a packet without body), or the tag's last byte (GCM: the
    E || index word follows the tag)"""
    L = len(w) - growth(suite)
    last = len(w) - 1 if has_hmac(suite) else len(w) - 5
    if body and L > 8:
        return 8 + (L - 8) // 2
    return last


def forge(suite, wire):
    """about 1 % of the packets forged (at least 2, at most 2 %), in the
    body and in the tag's last byte in turn: the batch and the indices"""
    idx = list(range(37, len(wire), 89))
    assert len(idx) >= 2 and len(wire) <= 100 * len(idx) <= 2 * len(wire)
    out = list(wire)
    for k, i in enumerate(idx):
        s, w = out[i]
        q = bytearray(w)
        q[forge_at(suite, w, k % 2 == 0)] ^= 0x10
        out[i] = (s, bytes(q))
    return out, idx


def oracle_rows(be, ctx, op, pkts):
    """[(errno, pos, end, bytes)] of [(session, packet)] through ctx[session]
    in turn: protect with room to grow, unprotect with none; bytes are the
    whole buffer the oracle leaves"""
    rows = []
    for s, p in pkts:
        size = len(p) + (32 if op == "srtcp_encrypt" else 0)
        e, po, en, _, buf = be.call(ctx[s], op, size, 0, len(p), p, size)
        rows.append((e, po, en, buf))
    return rows


def rtcp_states(be, ctx, streams):
    """(rtcp_index, replay lix, replay bitmap) of every (session, ssrc)"""
    return [be.rtcp_state(ctx[s], x) for s, x in streams]


def product_states(sessions, streams):
    """the same of product contexts (None: no such stream)"""
    out = []
    for s, x in streams:
        e, st = sessions[s].export(x)
        out.append(None if e else (st.rtcp_index, st.replay_rtcp_lix,
                                   st.replay_rtcp_bitmap))
    return out


def receive(be, suite, flags, keys, recv, streams):
    """recv through fresh oracle receivers: (rows, states)"""
    rx = [be.alloc(suite, k, flags)[0] for k in keys]
    rows = oracle_rows(be, rx, "srtcp_decrypt", recv)
    st = rtcp_states(be, rx, streams)
    for c in rx:
        be.free(c)
    return rows, st


_ref = {}


def reference(suite, flags, order, kind):
    """the batch and the oracle's results, computed once and shared: plain
    [(session, bytes)], the clean and the forged received batch, the
    oracle's rows for the three, the forged indices, the streams
    [(session, ssrc)] and their states after each"""
    key = (suite, flags, order, kind)
    if key in _ref:
        return _ref[key]
    lay = layout(kind, order)
    rng = np.random.default_rng(9000 + 100 * suite + 10 * flags +
                                ORDERS.index(order) +
                                5 * ("one", "many", "three").index(kind))
    plain = [(s, packet(rng, x, L)) for s, x, L in lay]
    streams = sorted({(s, x) for s, x, _ in lay})
    nsess = 1 + max(s for s, _, _ in lay)
    keys = keys_for(suite, nsess)
    be = O.OracleBackend()
    tx = [be.alloc(suite, k, flags)[0] for k in keys]
    enc = oracle_rows(be, tx, "srtcp_encrypt", plain)
    assert all(r[:2] == (0, 0) for r in enc)
    assert all(r[2] == len(p) + growth(suite) for r, (_, p) in zip(enc, plain))
    tx_state = rtcp_states(be, tx, streams)
    for c in tx:
        be.free(c)
    clean = [(s, r[3][:r[2]]) for (s, _), r in zip(plain, enc)]
    forged, idx = forge(suite, clean)
    dec, rx_state = receive(be, suite, flags, keys, clean, streams)
    fdec, frx_state = receive(be, suite, flags, keys, forged, streams)
    # on the oracle alone: the clean batch returns 0 everywhere and gives
    # the plain packets back, the forged one fails exactly where forged
    assert not any(r[0] for r in dec)
    assert all(r[3][:r[2]] == p for r, (_, p) in zip(dec, plain))
    assert [i for i, r in enumerate(fdec) if r[0]] == idx
    assert all(fdec[i][0] == P.EAUTH for i in idx)
    res = {"lay": lay, "plain": plain, "clean": clean, "forged": forged,
           "enc": enc, "dec": dec, "fdec": fdec, "idx": idx, "keys": keys,
           "streams": streams, "tx_state": tx_state, "rx_state": rx_state,
           "frx_state": frx_state}
    _ref[key] = res
    return res


# ---- disturbed receive ------------------------------------------------------

NDIST = 24              # packets per stream


def disturbed(suite, nsess):
    """nsess sessions x 2 SSRCs, 24 packets per stream, every other one of a
    STRADDLE length; per stream the arrivals 4 and 5 swapped and the packet
    of arrival 5 (the sender's 4th, a STRADDLE length) delivered again five
    arrivals later; the streams interleaved round-robin.  Through the oracle:
    (keys, streams, arrivals [(session, wire)], rows, states, the copies'
    places)"""
    key = ("disturbed", suite, nsess)
    if key in _ref:
        return _ref[key]
    rng = np.random.default_rng(9900 + 10 * suite + nsess)
    keys = keys_for(suite, nsess)
    streams = [(s, 0x64000000 + 16 * s + k) for s in range(nsess)
               for k in range(2)]
    be = O.OracleBackend()
    tx = [be.alloc(suite, k, 0)[0] for k in keys]
    per, copies = [], []
    for q, (s, x) in enumerate(streams):
        lens = [STRADDLE[(j // 2 + q) % len(STRADDLE)] if j % 2 == 0
                else length_of("spread", j + 7 * q) for j in range(NDIST)]
        pk = [(s, packet(rng, x, L)) for L in lens]
        rows = oracle_rows(be, tx, "srtcp_encrypt", pk)
        assert not any(r[0] for r in rows)
        w = [(s, r[3][:r[2]]) for r in rows]
        assert len(w[4][1]) - growth(suite) in STRADDLE
        w[4], w[5] = w[5], w[4]
        w.insert(10, w[5])
        per.append(w)
        copies.append(10)
    for c in tx:
        be.free(c)
    arr, dup = [], []
    for j in range(NDIST + 1):
        for q, w in enumerate(per):
            if j == copies[q]:
                dup.append(len(arr))
            arr.append(w[j])
    rows, st = receive(be, suite, 0, keys, arr, streams)
    assert [i for i, r in enumerate(rows) if r[0]] == dup
    assert all(rows[i][0] == errno.EALREADY for i in dup)
    # "authenticated and not deciphered": a copy stays as it arrived
    assert all(rows[i][3] == arr[i][1] for i in dup)
    _ref[key] = (keys, streams, arr, rows, st, dup)
    return _ref[key]


# ---- per-call and mbuf batch ------------------------------------------------

PC_LENS = (8, 9, 10, 11, 12, 13, 55, 59, 60, 61, 63, 64, 65, 67, 71, 125, 127,
           128, 129, 131)
POS = (0, 1, 2, 3, 5, 6, 7)


def percall_reference(suite, flags):
    """every length of PC_LENS, mb->pos cycling through POS, through the
    oracle: [(op, data, size, pos, (errno, pos, end, size, bytes))] for the
    sender and for the receiver (the protected packets at another offset,
    in a buffer with no room to spare)"""
    key = ("percall", suite, flags)
    if key in _ref:
        return _ref[key]
    rng = np.random.default_rng(9500 + 10 * suite + flags)
    k = keys_for(suite, 1)[0]
    be = O.OracleBackend()
    tx, rx = be.alloc(suite, k, flags)[0], be.alloc(suite, k, flags)[0]
    enc, dec = [], []
    for i, L in enumerate(PC_LENS):
        off = POS[i % len(POS)]
        pkt = packet(rng, SSRC, L)
        data = bytes(off) + pkt
        size = len(data) + 32
        r = be.call(tx, "srtcp_encrypt", size, off, len(data), data, size)
        assert r[:3] == (0, off, len(data) + growth(suite)), (L, r[:3])
        enc.append(("srtcp_encrypt", data, size, off, r))
        off2 = POS[(i + 3) % len(POS)]
        data2 = bytes(off2) + r[4][off:r[2]]
        r2 = be.call(rx, "srtcp_decrypt", len(data2), off2, len(data2), data2,
                     len(data2))
        assert r2[:3] == (0, off2, off2 + L), (L, r2[:3])
        assert r2[4][off2:r2[2]] == pkt, L
        dec.append(("srtcp_decrypt", data2, len(data2), off2, r2))
    be.free(tx)
    be.free(rx)
    _ref[key] = (k, enc, dec)
    return _ref[key]


# ---- the size bound -----------------------------------------------------------

def bound_lengths(suite):
    """plain lengths either side of SGPU_CACHED_MAX (4032), and the same
    minus the suite's growth: their protected packets are either side"""
    g = growth(suite)
    return list(range(4027 - g, 4038 - g)) + list(range(4027, 4038))
