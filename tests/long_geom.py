"""Packets up to and past the small kernel's 2048-byte bound through the
per-call API and the mbuf batches: the traffic, the oracle's answers and the
fixture's packet function, shared by tests/test_long_geom_cpu.py and
tests/test_gpu_long_geom.py.

The oracle (tests/oracle_lib.py) is pinned to the reference at these lengths
by tests/test_long_geom_cpu.py; it is called one packet at a time, once per
(suite, kind, flags, traffic), and the result is cached and never modified.
Nothing here needs a GPU.

Traffic: one sender and one receiver per (suite, kind, flags).  RTP packets
of every plain length 12..2120, header length 12 + 4 (L % 4) (the four shift
classes; 12 where that does not fit) and 76 + 4 (L % 4) (CC = 15 plus an
extension) where L % 11 == 0, sequence numbers from 65000 (the ROC rolls
inside), then the jumbo lengths; SRTCP packets of every length 8..2120.
mb->pos cycles through POS; the receiver takes the protected packet at
another offset in a buffer with no room to spare.  At every 97th length, and
at the lengths whose protected packet is 2047, 2048 and 2049 bytes long, the
receiver first gets a copy forged in the body, then one forged in the tag's
last byte, then the true packet, then the true packet again.
"""
import collections
import errno

import numpy as np

import re_amd.srtp as P
from tests import oracle_lib as O
from tests import srtcp_geom as G
from tests.test_gpu_fastpath import keys_for
from tests.test_gpu_hdrgeom import header_shape, rtp_packet

U = P.SRTP_UNENCRYPTED_SRTCP
KINDS = (("srtp", 0), ("srtcp", 0), ("srtcp", U))
KIND_IDS = ("srtp", "srtcp", "srtcp_u")
SMALL_MAX = 2048        # SGPU_SMALL_MAX: protected bytes from mb->pos
RTP_LENS = range(12, 2121)
RTCP_LENS = range(8, 2121)
JUMBO = (4000, 4031, 4032, 4033, 4100, 6000, 9000)
POS = (0, 1, 2, 3, 5, 6, 7)
S0 = 65000
SSRC = 0x6c6f6e67
EDGE = (2047, 2048, 2049)       # protected lengths disturbed on receive

# one call: the operation, the mbuf's bytes [0, end), its size and pos, the
# oracle's (errno, pos, end, size, bytes), the plain length, the protected
# length and what the receiver was handed ("true", "body", "tag", "again")
Call = collections.namedtuple("Call", "op data size off want L plen note")


def growth(suite, kind):
    """bytes protection appends"""
    if kind == "srtcp":
        return G.growth(suite)
    return P.tag_len(suite)


def hdr_len(L):
    """the RTP header length of the packet of L bytes"""
    x = L % 4
    if L % 11 == 0 and L >= 76 + 4 * x:
        return 76 + 4 * x
    return 12 + 4 * x if 12 + 4 * x <= L else 12


def rtcp_packet(rng, ssrc, L):
    """an RTCP packet of L bytes; the header's length field is L // 4 - 1
    (the reference does not read it)"""
    return bytes([0x80, 200]) + (L // 4 - 1).to_bytes(2, "big") + \
        ssrc.to_bytes(4, "big") + \
        rng.integers(0, 256, L - 8, dtype=np.uint8).tobytes()


def lengths(kind, jumbo=True):
    if kind == "srtp":
        return list(RTP_LENS) + (list(JUMBO) if jumbo else [])
    return list(RTCP_LENS)


def op_names(kind):
    return kind + "_encrypt", kind + "_decrypt"


def forge_at(suite, kind, wire, L, body):
    """the byte of the protected packet to flip: the middle of the body (of
    the payload for RTP), or the tag's last byte"""
    if kind == "srtcp":
        return G.forge_at(suite, wire, body)
    hl = hdr_len(L)
    if body and L > hl:
        return hl + (L - hl) // 2
    return len(wire) - 1


def traffic(suite, kind, flags, lens, seed, disturbed):
    """lens through a sender and a receiver of the oracle: the key, the
    sender's and the receiver's [Call] and both exported states.  disturbed:
    the plain lengths the receiver gets forged copies and a repeat of."""
    rng = np.random.default_rng(seed)
    key = keys_for(suite, 1)[0]
    enc_op, dec_op = op_names(kind)
    g = growth(suite, kind)
    be = O.OracleBackend()
    tx, rx = be.alloc(suite, key, flags)[0], be.alloc(suite, key, flags)[0]
    enc, dec = [], []
    window = kind == "srtp" or G.has_hmac(suite)
    for i, L in enumerate(lens):
        off = POS[i % len(POS)]
        if kind == "srtp":
            hl = hdr_len(L)
            assert header_shape(hl)[0] == (15 if hl >= 76 else (hl - 12) // 4)
            pkt = rtp_packet(rng, (S0 + i) & 0xffff, SSRC, hl, L - hl)
        else:
            pkt = rtcp_packet(rng, SSRC, L)
        assert len(pkt) == L
        data = bytes(off) + pkt
        size = len(data) + 32
        r = be.call(tx, enc_op, size, off, len(data), data, size)
        assert r[:3] == (0, off, len(data) + g), (L, r[:3])
        enc.append(Call(enc_op, data, size, off, r, L, L + g, "true"))
        wire = r[4][off:r[2]]
        off2 = POS[(i + 3) % len(POS)]
        notes = ("body", "tag", "true", "again") if L in disturbed \
            else ("true",)
        for note in notes:
            w = bytearray(wire)
            if note in ("body", "tag"):
                w[forge_at(suite, kind, wire, L, note == "body")] ^= 0x10
            data2 = bytes(off2) + bytes(w)
            r2 = be.call(rx, dec_op, len(data2), off2, len(data2), data2,
                         len(data2))
            # on the oracle alone: a forged copy fails, the true packet
            # comes back as it was sent, its repeat is a replay where the
            # suite keeps a window
            if note in ("body", "tag"):
                assert r2[0] == P.EAUTH, (L, note, r2[0])
            elif note == "true" or not window:
                assert r2[:3] == (0, off2, off2 + L), (L, note, r2[:3])
                assert r2[4][off2:r2[2]] == pkt, (L, note)
            else:
                assert r2[0] == errno.EALREADY, (L, note, r2[0])
            dec.append(Call(dec_op, data2, len(data2), off2, r2, L, L + g,
                            note))
    if kind == "srtp":
        st = (be.export(tx, SSRC), be.export(rx, SSRC))
    else:
        st = (be.rtcp_state(tx, SSRC), be.rtcp_state(rx, SSRC))
    be.free(tx)
    be.free(rx)
    return {"key": key, "enc": enc, "dec": dec, "tx_state": st[0],
            "rx_state": st[1]}


def disturbed_lengths(suite, kind, lens):
    """every 97th length of lens and those whose protected packet is 2047,
    2048 or 2049 bytes long"""
    g = growth(suite, kind)
    d = {L for i, L in enumerate(lens) if i % 97 == 50}
    d |= {p - g for p in EDGE if p - g in lens}
    return d


_ref = {}


def _cached(key, lens, seed):
    if key not in _ref:
        suite, kind, flags = key[1:4]
        _ref[key] = traffic(suite, kind, flags, lens, seed,
                            disturbed_lengths(suite, kind, lens))
    return _ref[key]


def _seed(base, suite, kind, flags):
    return base + 10 * suite + KINDS.index((kind, flags))


def sweep(suite, kind, flags):
    """every length (RTP: the jumbo lengths behind them), computed once"""
    lens = lengths(kind)
    assert all(p - growth(suite, kind) in lens for p in EDGE)
    return _cached(("sweep", suite, kind, flags), lens,
                   _seed(11000, suite, kind, flags))


def fitting(suite, kind, flags):
    """every length whose protected packet is at most 2048 bytes long"""
    g = growth(suite, kind)
    lens = [L for L in lengths(kind, False) if L + g <= SMALL_MAX]
    return _cached(("fit", suite, kind, flags), lens,
                   _seed(12000, suite, kind, flags))


def straddling(suite, kind, flags):
    """protected lengths 2040..2060: either side of the bound in one batch"""
    g = growth(suite, kind)
    lens = [p - g for p in range(2040, 2061)]
    return _cached(("edge", suite, kind, flags), lens,
                   _seed(13000, suite, kind, flags))


def jumbo(suite, kind, flags):
    """the jumbo lengths alone"""
    return _cached(("jumbo", suite, kind, flags), list(JUMBO),
                   _seed(14000, suite, kind, flags))


# ---- many short packets: the job-count bound ---------------------------------

NJOBS = (2047, 2048, 2049)      # either side of SGPU_COOP_MAX
FORGED = 1000


def many_short(suite, n):
    """n RTP packets of 60..90 bytes, packet FORGED forged in the tag on the
    way back; through the oracle one packet at a time"""
    key = ("short", suite, n)
    if key in _ref:
        return _ref[key]
    rng = np.random.default_rng(15000 + 10 * suite + n % 10)
    k = keys_for(suite, 1)[0]
    g = growth(suite, "srtp")
    be = O.OracleBackend()
    tx, rx = be.alloc(suite, k, 0)[0], be.alloc(suite, k, 0)[0]
    enc, dec = [], []
    for i in range(n):
        L = 60 + i % 31
        hl = 12 + 4 * (i % 4)
        off = POS[i % len(POS)]
        pkt = rtp_packet(rng, 1000 + i, SSRC, hl, L - hl)
        data = bytes(off) + pkt
        size = len(data) + 32
        r = be.call(tx, "srtp_encrypt", size, off, len(data), data, size)
        assert r[:3] == (0, off, len(data) + g), (i, r[:3])
        enc.append(Call("srtp_encrypt", data, size, off, r, L, L + g, "true"))
        w = bytearray(r[4][off:r[2]])
        if i == FORGED:
            w[-1] ^= 0x10
        data2 = bytes(off) + bytes(w)
        r2 = be.call(rx, "srtp_decrypt", len(data2), off, len(data2), data2,
                     len(data2))
        assert r2[0] == (P.EAUTH if i == FORGED else 0), (i, r2[0])
        dec.append(Call("srtp_decrypt", data2, len(data2), off, r2, L, L + g,
                        "tag" if i == FORGED else "true"))
    st = (be.export(tx, SSRC), be.export(rx, SSRC))
    be.free(tx)
    be.free(rx)
    _ref[key] = {"key": k, "enc": enc, "dec": dec, "tx_state": st[0],
                 "rx_state": st[1]}
    return _ref[key]


# ---- the fixture's packets (oracle/gen_long_geom_golden.c) ------------------

GOLDEN_SSRC = 0x6c67656f
GOLDEN_SEQ0 = 63450


def golden_packet(kind, L):
    """the packet of L bytes of tests/golden/long_geom_golden.json.gz, as the
    generator's comment states it"""
    p = bytearray((29 * L + 7 * i + 3 * (i >> 4) + 1) & 0xff
                  for i in range(L))
    if kind == "srtcp":
        p[0], p[1] = 0x81, 200 + L % 5
        p[2:4] = (L // 4 - 1).to_bytes(2, "big")
        p[4:8] = GOLDEN_SSRC.to_bytes(4, "big")
        return bytes(p)
    ext = L % 11 == 0
    cc = 15 if ext else L % 4
    p[0] = 0x80 | (0x10 if ext else 0) | cc
    p[2:4] = ((GOLDEN_SEQ0 + L) & 0xffff).to_bytes(2, "big")
    p[8:12] = GOLDEN_SSRC.to_bytes(4, "big")
    if ext:
        p[12 + 4 * cc:16 + 4 * cc] = b"\xbe\xde\x00" + bytes([L % 4])
    assert 12 + 4 * cc + (4 + 4 * (L % 4) if ext else 0) == hdr_len(L)
    return bytes(p)
