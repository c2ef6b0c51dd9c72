"""Receiver-statistics test helpers (test infrastructure): the goldens of
tests/golden/rtp_source_golden.json.gz (scripts/gen_rtp_source_golden.c, the
reference's own source.c / member.c / hash.c / rtp_hdr_decode) replayed
through rtp_rx_stats / rtp_rx_sr / rtp_rx_report on host or device memory,
and random traffic for the device-against-host-twin tests.
"""
import errno
import gzip
import json
import os

import numpy as np

import re_amd.srtp as P

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rtp_source_golden.json.gz")

STAT = {"ok": 0, "badseq": P.RTP_RX_BADSEQ, "nomember": P.RTP_RX_NOMEMBER,
        "badmsg": errno.EBADMSG}
SRC_DT, SESS_DT = P.rtp_rx_dtypes()
MSG_DT, RB_DT = P.rtcp_enc_dtypes()[:2]
# the fields of a golden check's member rows, in order
M_FIELDS = ("ssrc", "flags", "max_seq", "cycles", "base_seq", "bad_seq",
            "received", "expected_prior", "received_prior", "transit",
            "jitter", "last_rtp_ts", "rx_bytes", "sr_recv", "sr_ntp_hi",
            "sr_ntp_lo", "sr_rtp_ts", "sr_psent", "sr_osent")
RB_FIELDS = ("ssrc", "fraction", "lost", "last_seq", "jitter", "lsr", "dlsr")

_cache = None


def load_cases():
    global _cache
    if _cache is None:
        with gzip.open(GOLDEN, "rt") as f:
            _cache = json.load(f)["cases"]
    return _cache


class HostMem:
    """arrays in host memory, for the host twins"""
    host = True

    def up(self, a):
        return np.ascontiguousarray(a).copy()

    def ptr(self, h):
        return None if h is None else h.ctypes.data

    def down(self, h):
        return h


class DevMem:
    """arrays in device memory (torch tensors of bytes)"""
    host = False

    def up(self, a):
        import torch
        a = np.ascontiguousarray(a)
        return (torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda(),
                a.dtype, a.shape)

    def ptr(self, h):
        return None if h is None else h[0].data_ptr()

    def down(self, h):
        return h[0].cpu().numpy().view(h[1]).reshape(h[2])


def hash_order(sess_row):
    """a session's members in hash_apply order: by ssrc & 7, then slot"""
    mc = int(sess_row["memberc"])
    return sorted(range(mc),
                  key=lambda k: (int(sess_row["m"][k]["ssrc"]) & 7, k))


def member_rows(sess_row):
    out = []
    for k in hash_order(sess_row):
        m = sess_row["m"][k]
        out.append([int(m[f]) for f in M_FIELDS])
    return out


def interleave(lists):
    """round-robin over the lists: (list index, item), each list in order"""
    out, j = [], 0
    while True:
        row = [(i, l[j]) for i, l in enumerate(lists) if j < len(l)]
        if not row:
            return out
        out.extend(row)
        j += 1


def pack(pkts, gap=3):
    """packets (bytes) into one arena with gaps; arena, pos, end"""
    pos, end, chunks, at = [], [], [], 5
    chunks.append(b"\xee" * at)
    for b in pkts:
        pos.append(at)
        end.append(at + len(b))
        chunks.append(b + b"\xee" * gap)
        at += len(b) + gap
    arena = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
    return arena, np.array(pos, np.uint32), np.array(end, np.uint32)


def call_stats(be, pkts, sess, arrival, sessv_h, nsess, res=None):
    """one rtp_rx_stats call over packets (bytes); stat as int32 array"""
    n = len(pkts)
    arena, pos, end = pack(pkts)
    stat_h = be.up(np.full(n, 0x5a5a5a5a, np.int32))
    hs = [be.up(arena), be.up(pos), be.up(end),
          None if res is None else be.up(np.asarray(res, np.int32)),
          None if sess is None else be.up(np.asarray(sess, np.uint32)),
          None if arrival is None else be.up(np.asarray(arrival, np.uint32))]
    rc = P.rtp_rx_stats(be.ptr(hs[0]), arena.nbytes, be.ptr(hs[1]),
                        be.ptr(hs[2]), be.ptr(hs[3]), be.ptr(hs[4]),
                        be.ptr(hs[5]), n, be.ptr(sessv_h), nsess,
                        be.ptr(stat_h), host=be.host)
    assert rc == 0, rc
    return be.down(stat_h)


def call_sr(be, sess, ev, recv_ms, sessv_h, nsess):
    """ev: rows of (ssrc, ntp_sec, ntp_frac, rtp_ts, psent, osent)"""
    n = len(ev)
    if not n:
        return
    cols = [be.up(np.array([e[k] for e in ev], np.uint32)) for k in range(6)]
    sh = None if sess is None else be.up(np.asarray(sess, np.uint32))
    rc = P.rtp_rx_sr(be.ptr(sessv_h), nsess, be.ptr(sh),
                     *[be.ptr(c) for c in cols], recv_ms, n, host=be.host)
    assert rc == 0, rc


def call_report(be, sessv_h, nsess, now_ms, local_ssrc=None):
    """rbv (nsess x 8), nrb, rr_msgv (None without local_ssrc)"""
    rb_h = be.up(np.frombuffer(b"\x5a" * (nsess * 8 * RB_DT.itemsize),
                               RB_DT))
    nrb_h = be.up(np.full(nsess, 0x5a5a5a5a, np.uint32))
    ls_h = msg_h = None
    if local_ssrc is not None:
        ls_h = be.up(np.asarray(local_ssrc, np.uint32))
        msg_h = be.up(np.frombuffer(b"\x5a" * (nsess * MSG_DT.itemsize),
                                    MSG_DT))
    rc = P.rtp_rx_report(be.ptr(sessv_h), nsess, now_ms, be.ptr(rb_h),
                         be.ptr(nrb_h), be.ptr(ls_h), be.ptr(msg_h),
                         host=be.host)
    assert rc == 0, rc
    return (be.down(rb_h).reshape(nsess, 8), be.down(nrb_h),
            None if msg_h is None else be.down(msg_h))


def check_rr_msgs(msgv, nrb, local_ssrc):
    """the RR descriptors rtp_rx_report writes for rtcp_encode_batch_dev"""
    nsess = len(nrb)
    assert (msgv["pt"] == 201).all()
    assert (msgv["count"] == nrb).all() and (msgv["num"] == nrb).all()
    assert (msgv["first"] == 8 * np.arange(nsess)).all()
    assert (msgv["w"][:, 0] == np.asarray(local_ssrc, np.uint32)).all()
    assert not msgv["w"][:, 1:].any() and not msgv["flags"].any()
    assert not msgv["off"].any() and not msgv["len"].any()


def replay_golden(be, cases):
    """All cases as one batch, one session per case, the packets of every
    stage interleaved across the sessions; states, stat, report blocks,
    counts and RR descriptors equal the golden at every stage."""
    nsess = len(cases)
    use_arrival = bool(cases[0]["arrival"])
    assert all(bool(c["arrival"]) == use_arrival for c in cases)
    nstage = len(cases[0]["stages"])
    assert all(len(c["stages"]) == nstage for c in cases)
    sessv_h = be.up(np.zeros(nsess, SESS_DT))
    local_ssrc = [0x10000 + i for i in range(nsess)]
    for k in range(nstage):
        ops = {c["stages"][k]["op"] for c in cases}
        assert len(ops) == 1
        op = ops.pop()
        st = [c["stages"][k] for c in cases]
        if op == "rtp":
            items = interleave([s["pk"] for s in st])
            if not items:
                continue
            stat = call_stats(be, [bytes.fromhex(p[0]) for _, p in items],
                              [i for i, _ in items],
                              [p[1] for _, p in items] if use_arrival
                              else None, sessv_h, nsess)
            want = [STAT[p[2]] for _, p in items]
            bad = [(cases[items[j][0]]["name"], items[j][1], int(stat[j]))
                   for j in range(len(items)) if stat[j] != want[j]]
            assert not bad, (k, bad[:5])
        elif op == "sr":
            items = interleave([s["ev"] for s in st])
            recv = {s["recv_ms"] for s in st}
            assert len(recv) == 1
            call_sr(be, [i for i, _ in items], [e for _, e in items],
                    recv.pop(), sessv_h, nsess)
        elif op == "check":
            sv = be.down(sessv_h)
            for i, s in enumerate(st):
                assert int(sv[i]["memberc"]) == s["memberc"], \
                    (k, cases[i]["name"])
                assert member_rows(sv[i]) == s["m"], \
                    (k, cases[i]["name"], member_rows(sv[i]), s["m"])
        elif op == "report":
            now = {s["now_ms"] for s in st}
            assert len(now) == 1
            rbv, nrb, msgv = call_report(be, sessv_h, nsess, now.pop(),
                                         local_ssrc)
            for i, s in enumerate(st):
                got = [[int(rbv[i][j][f]) for f in RB_FIELDS]
                       for j in range(int(nrb[i]))]
                want = [[v & 0xffffffff for v in r] for r in s["rb"]]
                assert got == want, (k, cases[i]["name"], got, want)
                assert not rbv[i][int(nrb[i]):].view(np.uint8).any()
            check_rr_msgs(msgv, nrb, local_ssrc)
        else:
            raise AssertionError(op)


# ---- random traffic ------------------------------------------------------

def rtp_packet(seq, ts, ssrc, payload=8, b0=0x80, cut=None):
    b = bytes([b0, 96, (seq >> 8) & 0xff, seq & 0xff]) + \
        int(ts & 0xffffffff).to_bytes(4, "big") + \
        int(ssrc & 0xffffffff).to_bytes(4, "big")
    cc = b0 & 15
    b += b"\x11" * (4 * cc)
    if b0 & 0x10:
        b += b"\xbe\xde\x00\x01" + b"\x22" * 4
    b += b"\xa5" * payload
    return b if cut is None else b[:cut]


def random_traffic(rng, nsess, n):
    """n packets over nsess sessions interleaved at random, 1-10 SSRCs per
    session, with planted wraps, gaps, duplicates, jumps, resyncs, equal
    timestamps, bad headers and res != 0.  Returns pkts (bytes), sess,
    arrival, res."""
    nss = rng.integers(1, 11, nsess)
    seq = [rng.integers(0, 65536, k) for k in nss]
    # a quarter of the sources start near the wrap
    for s in range(nsess):
        near = rng.random(nss[s]) < 0.25
        seq[s] = np.where(near, 65536 - rng.integers(1, 6, nss[s]), seq[s])
    ts = [rng.integers(0, 1 << 32, k) for k in nss]
    ts[0][0] = 0                    # a first timestamp of 0: jitter skipped
    arr0 = [rng.integers(0, 1 << 32, k) for k in nss]
    jump = [[None] * k for k in nss]
    sess = rng.integers(0, nsess, n)
    sess[0] = 0
    which = rng.random(n)
    pkts, arrival, res = [], [], []
    first0 = True
    for i in range(n):
        s = int(sess[i])
        k = 0 if (s == 0 and first0) else int(rng.integers(0, nss[s]))
        if s == 0 and first0:
            first0 = False
        ssrc = 0x1000 * (s + 1) + 9 * k       # several share ssrc & 7
        w = which[i]
        sq = int(seq[s][k])
        adv = 1
        if jump[s][k] is not None:            # the packet after a jump
            sq = (jump[s][k] + 1) & 0xffff if w < 0.6 else \
                int(rng.integers(0, 65536))
            if w < 0.6:
                seq[s][k] = (sq + 1) & 0xffff
            jump[s][k] = None
            adv = 0
        elif w < 0.05:                        # gap near the dropout bound
            sq = (sq + int(rng.integers(2990, 3003))) & 0xffff
            seq[s][k] = sq
        elif w < 0.10:                        # duplicate / misordered
            sq = (sq - int(rng.integers(1, 104))) & 0xffff
            adv = 0
        elif w < 0.14:                        # big jump
            sq = (sq + int(rng.integers(5000, 60000))) & 0xffff
            jump[s][k] = sq
            adv = 0
        if adv:
            seq[s][k] = (int(seq[s][k]) + 1) & 0xffff
        if not (0.14 <= w < 0.24):            # else: the same timestamp
            ts[s][k] = (int(ts[s][k]) + int(rng.integers(1, 4000))) \
                & 0xffffffff if not (s == 0 and k == 0 and i == 0) else 0
        a = (int(ts[s][k]) + int(arr0[s][k]) +
             int(rng.integers(0, 400))) & 0xffffffff
        if 0.24 <= w < 0.25:
            a = int(ts[s][k])                 # transit 0
        b0, cut = 0x80, None
        if 0.25 <= w < 0.28:
            b0 = int(rng.choice([0x81, 0x90, 0x93, 0xa0]))
        if 0.28 <= w < 0.31:                  # bad header
            b0 = int(rng.choice([0x00, 0x40, 0xc0, 0x83, 0x90]))
            cut = {0x83: 23, 0x90: 19}.get(b0, int(rng.integers(0, 12))
                                           if rng.random() < 0.5 else None)
        pkts.append(rtp_packet(sq, int(ts[s][k]), ssrc,
                               int(rng.integers(0, 40)), b0, cut))
        arrival.append(a)
        res.append(int(rng.choice([errno.EBADMSG, 217]))
                   if 0.31 <= w < 0.34 else 0)
    return pkts, sess.astype(np.uint32), np.array(arrival, np.uint32), \
        np.array(res, np.int32)
