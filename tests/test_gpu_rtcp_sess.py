"""RTCP session state on the GPU (include/re_rtcp_sess_batch.h,
re_amd/csrc/hip/rtcp_sess.hip) through the C-ABI library:

  * every case of tests/golden/rtcp_sess_golden.json.gz (the reference's own
    decoder, member hash, sources and NTP routines, driven as src/rtp/sess.c
    drives them) in one batch, one session per case: the golden's packet
    bytes through rtcp_decode_full_batch_dev -> rtcp_rx_handle_batch_dev
    (which also pins the decoder's SR / RR / BYE output to the reference),
    and rtcp_tx_report_batch_dev -> rtcp_encode_batch_dev against the
    reference's SR / RR bytes;
  * random traffic against the host twin: 4096 sessions, 16 384 compounds
    and 65 536 outgoing packets interleaved with received RTP, as one call
    each and as three consecutive calls on resident state, every state byte
    for byte (tests/test_rtcp_sess_cpu.py shows what that traffic reaches);
  * one session without a session array: 20 000 outgoing packets, with a
    re-synchronisation between two calls, and compounds;
  * the round trip on device arrays only, between a "local" and a "peer"
    array of sessions, through SRTCP both ways, up to the round-trip time;
  * a forged packet (res != 0) is skipped and changes nothing.
"""
import numpy as np
import pytest

import re_amd.srtp as P
from tests import rtp_stats_util as U
from tests import rtcp_sess_util as R

pytestmark = pytest.mark.gpu

EAUTH = 217


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    P.load()
    return torch


# ---- the goldens -------------------------------------------------------------

GOLD_MAXMSG, GOLD_MAXITEM = 8, 16


def _decode_on_device(be):
    def decode(pkts, golden):
        n = len(pkts)
        arena, pos, end = U.pack(pkts)
        hs = [be.up(arena), be.up(pos), be.up(end)]
        desc = be.up(np.zeros((n, GOLD_MAXMSG), R.DESC_DT))
        item = be.up(np.zeros((n, GOLD_MAXITEM), R.ITEM_DT))
        nmsg, nitem, stop = (be.up(np.zeros(n, np.uint32)) for _ in range(3))
        err = be.up(np.zeros(n, np.int32))
        rc = P.rtcp_decode_full_dev(be.ptr(hs[0]), arena.nbytes,
                                    be.ptr(hs[1]), be.ptr(hs[2]), n,
                                    be.ptr(desc), GOLD_MAXMSG, be.ptr(nmsg),
                                    be.ptr(item), GOLD_MAXITEM,
                                    be.ptr(nitem), be.ptr(err), be.ptr(stop))
        assert rc == 0, (rc, P.lib().srtp_gpu_error())
        # the decoder's output for the kinds the handler reads is the
        # reference's
        h_desc, h_item = be.down(desc), be.down(item)
        h_nmsg, h_nitem = be.down(nmsg), be.down(nitem)
        for i, g in enumerate(golden):
            assert int(h_nmsg[i]) == len(g["msgs"]) <= GOLD_MAXMSG, i
            assert int(h_nitem[i]) <= GOLD_MAXITEM, i
            for j, m in enumerate(g["msgs"]):
                d = h_desc[i, j]
                got = [int(d[f]) for f in ("off", "size", "pt", "count",
                                           "length")]
                assert got == m[:5], (i, j, got, m)
                if m[2] in (200, 201, 203):
                    assert [int(d["ssrc"]), int(d["aux"])] == m[5:7], (i, j)
            got = [[int(e["msg"]), int(e["kind"]), int(e["sub"])] +
                   [int(x) for x in e["v"]]
                   for e in h_item[i, :int(h_nitem[i])]
                   if int(e["kind"]) in (R.ITEM_SR, R.ITEM_RB,
                                         R.ITEM_BYE_SRC)]
            assert got == g["items"], (i, got, g["items"])
        return desc, GOLD_MAXMSG, nmsg, item, GOLD_MAXITEM, nitem
    return decode


def _encode_on_device(be):
    def encode(rb_h, msg_h, nsess):
        room = 512
        pos = np.arange(nsess, dtype=np.uint32) * room
        hs = [be.up(np.zeros(nsess * room, np.uint8)), be.up(pos),
              be.up(np.zeros(nsess, np.uint32)), be.up(pos + room),
              be.up(np.arange(nsess + 1, dtype=np.uint32)),
              be.up(np.full(nsess, -1, np.int32))]
        rc = P.rtcp_encode_dev(be.ptr(hs[0]), nsess * room, be.ptr(hs[1]),
                               be.ptr(hs[2]), be.ptr(hs[3]), nsess,
                               be.ptr(hs[4]), be.ptr(msg_h), nsess,
                               be.ptr(rb_h), nsess * 8, err_ptr=be.ptr(hs[5]))
        assert rc == 0, (rc, P.lib().srtp_gpu_error())
        assert not be.down(hs[5]).any()
        arena, end = be.down(hs[0]), be.down(hs[2])
        return [arena[pos[i]:end[i]].tobytes() for i in range(nsess)]
    return encode


def test_golden_one_batch_decoded_and_encoded_on_device(torch_cuda):
    be = U.DevMem()
    R.replay_golden(be, R.load_cases(), _decode_on_device(be),
                    _encode_on_device(be))


# ---- random traffic against the host twin ------------------------------------

@pytest.fixture(scope="module")
def traffic():
    return R.session_traffic()


@pytest.mark.parametrize("calls", [1, 3])
def test_random_traffic_against_host_twin(torch_cuda, traffic, calls):
    parts, q_sess, q_ssrc = traffic
    if calls == 1:
        parts = [R.join_parts(parts)]
    host = R.run_session_traffic(U.HostMem(), parts, q_sess, q_ssrc)
    dev = R.run_session_traffic(U.DevMem(), parts, q_sess, q_ssrc)
    assert len(host) == len(dev)
    for k, (h, d) in enumerate(zip(host, dev)):
        assert h.dtype == d.dtype and h.tobytes() == d.tobytes(), k
    R.check_invariant(dev[-2], dev[-1])
    assert dev[-1]["rtt"].any() and dev[-1]["jit"].any()


# ---- one session, no session array -------------------------------------------

def test_one_session_without_session_array(torch_cuda):
    rng = np.random.default_rng(7)
    n = 20000
    pkts, _, jfs, res = R.random_tx(rng, 1, n)
    rows, _, rres = R.random_compounds(rng, 1, 300, R.T_NOW_US)
    arr = R.decoded_arrays(rows, R.T_MAXMSG, R.T_MAXITEM)
    out = []
    for be in (U.HostMem(), U.DevMem()):
        sessv = be.up(np.zeros(2, R.SESS_DT))
        extv = be.up(R.fresh_ext(2, 90000, 90000))
        o = [R.call_tx(be, pkts[:12000], None, jfs[:12000], extv, 2,
                       res[:12000])]
        first = R.tx_row(be.down(extv)[0])
        o += list(R.call_tx_report(be, sessv, extv, 2, 5000,
                                   R.T_NOW_US + 1000000, [1, 2]))
        # the report cleared ts_synced: the next call's first accepted
        # packet is the new reference
        o.append(R.call_tx(be, pkts[12000:], None, jfs[12000:], extv, 2,
                           res[12000:]))
        second = R.tx_row(be.down(extv)[0])
        assert first[4] == 1 and second[4] == 1 and second[2] != first[2]
        k = int(np.flatnonzero(o[-1] == 0)[0])
        assert second[2] == int(jfs[12000 + k])
        o.append(R.call_handle(be, be.up(arr[0]), R.T_MAXMSG, be.up(arr[1]),
                               be.up(arr[2]), R.T_MAXITEM, be.up(arr[3]),
                               rres, None, len(rows), sessv, extv, 2, 1000,
                               R.T_NOW_US))
        o += [be.down(sessv), be.down(extv)]
        out.append(o)
    host, dev = out
    for k, (h, d) in enumerate(zip(host, dev)):
        assert h.tobytes() == d.tobytes(), k
    ok = (host[0] == 0).sum() + (host[4] == 0).sum()
    assert int(dev[-1][0]["psent"]) == ok > 15000
    assert int(dev[-2][0]["memberc"]) > 0
    assert not dev[-2][1].tobytes().strip(b"\0")
    assert not dev[-1][1]["psent"]


# ---- the round trip ----------------------------------------------------------

class _Side:
    """one array of sessions on the device, with its SRTCP contexts"""

    def __init__(self, torch, nsess, tx_ctx, rx_ctx, ssrc0):
        self.be = U.DevMem()
        self.nsess = nsess
        self.sessv = self.be.up(np.zeros(nsess, R.SESS_DT))
        self.extv = self.be.up(R.fresh_ext(nsess, 8000, 8000))
        self.tx_ctx, self.rx_ctx = tx_ctx, rx_ctx
        self.ssrc = ssrc0 + np.arange(nsess, dtype=np.uint32)
        self.room = 256

    def report_protected(self, now_ms, now_us):
        """rtcp_tx_report -> rtcp_encode -> srtcp_encrypt, all on device
        arrays; the arena and its pos / end handles"""
        be, n, room = self.be, self.nsess, self.room
        r = R.call_tx_report(be, self.sessv, self.extv, n, now_ms, now_us,
                             self.ssrc, keep=True)
        pos = np.arange(n, dtype=np.uint32) * room
        arena = be.up(np.zeros(n * room, np.uint8))
        h_pos, h_end = be.up(pos), be.up(np.zeros(n, np.uint32))
        h_cap = be.up(pos + room)
        err = be.up(np.full(n, -1, np.int32))
        mfirst = be.up(np.arange(n + 1, dtype=np.uint32))
        rc = P.rtcp_encode_dev(be.ptr(arena), n * room, be.ptr(h_pos),
                               be.ptr(h_end), be.ptr(h_cap), n,
                               be.ptr(mfirst), be.ptr(r[4]), n, be.ptr(r[3]),
                               n * 8, err_ptr=be.ptr(err))
        assert rc == 0 and not be.down(err).any()
        sess = be.up(np.arange(n, dtype=np.uint32))
        rc = P.device_batch_dev("srtcp_encrypt", self.tx_ctx, be.ptr(arena),
                                n * room, be.ptr(h_pos), be.ptr(h_end),
                                be.ptr(h_cap), be.ptr(err), n, be.ptr(sess))
        assert rc == 0 and not be.down(err).any(), P.lib().srtp_gpu_error()
        return arena, h_pos, h_end, h_cap, sess, r[:3]

    def receive(self, wire, recv_ms, now_us):
        """srtcp_decrypt -> rtcp_decode_full -> rtcp_rx_handle on what the
        other side protected; res, stat, and the plaintext packets"""
        be, n, room = self.be, self.nsess, self.room
        arena, h_pos, h_end, h_cap, sess = wire
        res = be.up(np.full(n, -1, np.int32))
        rc = P.device_batch_dev("srtcp_decrypt", self.rx_ctx, be.ptr(arena),
                                n * room, be.ptr(h_pos), be.ptr(h_end),
                                be.ptr(h_cap), be.ptr(res), n, be.ptr(sess))
        assert rc == 0, P.lib().srtp_gpu_error()
        desc = be.up(np.zeros((n, 2), R.DESC_DT))
        item = be.up(np.zeros((n, 10), R.ITEM_DT))
        nmsg, nitem, stop = (be.up(np.zeros(n, np.uint32)) for _ in range(3))
        derr = be.up(np.zeros(n, np.int32))
        rc = P.rtcp_decode_full_dev(be.ptr(arena), n * room, be.ptr(h_pos),
                                    be.ptr(h_end), n, be.ptr(desc), 2,
                                    be.ptr(nmsg), be.ptr(item), 10,
                                    be.ptr(nitem), be.ptr(derr), be.ptr(stop))
        assert rc == 0, P.lib().srtp_gpu_error()
        stat = be.up(np.full(n, 0x5a5a5a5a, np.int32))
        rc = P.rtcp_rx_handle(be.ptr(desc), 2, be.ptr(nmsg), be.ptr(item),
                              10, be.ptr(nitem), be.ptr(res), be.ptr(sess),
                              n, be.ptr(self.sessv), be.ptr(self.extv), n,
                              recv_ms, now_us, be.ptr(stat))
        assert rc == 0, P.lib().srtp_gpu_error()
        a, p, e = be.down(arena), be.down(h_pos), be.down(h_end)
        r = be.down(res)
        plain = [a[p[i]:e[i]].tobytes() if not r[i] else None
                 for i in range(n)]
        return r, be.down(stat), plain, (be.down(desc), be.down(nmsg),
                                         be.down(item), be.down(nitem))


def test_round_trip_on_device_arrays(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(31)
    nsess = 64
    ctx = []
    for _ in range(4):          # local tx / peer rx, peer tx / local rx
        if len(ctx) % 2 == 0:
            keys = bytes(rng.integers(0, 256, nsess * 30, dtype=np.uint8))
        e, c = P.alloc_many(nsess, 1, keys)
        assert e == 0
        ctx.append(c)
    local = _Side(torch, nsess, ctx[0], ctx[3], 0x10000)
    peer = _Side(torch, nsess, ctx[2], ctx[1], 0x20000)
    T0 = R.T_NOW_US + 100000000      # clear of the compact-NTP wrap

    # the peer has seen the local side's RTP, so its member has a source
    rx = [U.rtp_packet(100 + j, 160 * j, int(local.ssrc[s]))
          for j in range(3) for s in range(nsess)]
    rx_sess = list(range(nsess)) * 3
    U.call_stats(peer.be, rx, rx_sess, [5000 + 161 * (i // nsess)
                                        for i in range(len(rx))],
                 peer.sessv, nsess)
    # local: rtp_tx_stats -> report (an SR) -> encode -> protect
    txp = [R.tx_packet(rng, 1000 + 160 * j) for j in range(4)
           for s in range(nsess)]
    st = R.call_tx(local.be, txp, list(range(nsess)) * 4,
                   [T0 - 100000 + 20000 * (i // nsess)
                    for i in range(len(txp))], local.extv, nsess)
    assert not st.any()
    wire = local.report_protected(4000, T0)
    assert (wire[5][2]["pt"] == 200).all()
    # one packet is forged on the way: skipped, nothing changes for it
    forged = 5
    e_end = local.be.down(wire[2])
    wire[0][0][int(e_end[forged]) - 1] ^= 1
    before = peer.be.down(peer.sessv)[forged].tobytes()
    res, stat, plain, _ = peer.receive(wire[:5], 1000, T0 + 30000)
    assert res[forged] == EAUTH and stat[forged] == P.RTP_RX_SKIPPED
    assert not np.delete(res, forged).any() and \
        not np.delete(stat, forged).any()
    pv = peer.be.down(peer.sessv)
    assert pv[forged].tobytes() == before
    ok = [s for s in range(nsess) if s != forged]
    assert all(int(pv[s]["m"][0]["sr_recv"]) == 1000 for s in ok)
    assert int(pv[forged]["m"][0]["sr_recv"]) == 0

    # the peer's own report 2.5 s later carries the matching lsr / dlsr
    back = peer.report_protected(3500, T0 + 2530000)
    rbv, nrb, msgv = back[5]
    assert (nrb == 1).all() and (msgv["pt"] == 201).all()
    lsr = R.ntp_compact_of(T0)
    assert all(int(rbv[s][0]["lsr"]) == lsr and
               int(rbv[s][0]["dlsr"]) == 65536 * 2500 // 1000 for s in ok)
    assert int(rbv[forged][0]["lsr"]) == 0
    # back through SRTCP, the local side gets its round-trip time: 2.56 s
    # on the wall clock less the peer's 2.5 s
    res, stat, plain, dec = local.receive(back[:5], 9000, T0 + 2560000)
    assert not res.any() and not stat.any()
    lx, lv = local.be.down(local.extv), local.be.down(local.sessv)
    assert (lv["memberc"] == 1).all()
    assert (lv["m"]["ssrc"][:, 0] == peer.ssrc).all()
    # ... equal to the host twin's, from the same decoded packets
    hb = U.HostMem()
    h_sessv = np.zeros(nsess, R.SESS_DT)
    h_extv = R.fresh_ext(nsess, 8000, 8000)
    h_stat = R.call_handle(hb, dec[0], 2, dec[1], dec[2], 10, dec[3], None,
                           list(range(nsess)), nsess, h_sessv, h_extv, nsess,
                           9000, T0 + 2560000)
    assert not h_stat.any()
    for f in ("cum_lost", "jit", "rtt"):
        assert (lx[f] == h_extv[f]).all(), f
    assert h_sessv.tobytes() == lv.tobytes()
    rtt = lx["rtt"][:, 0]
    assert all(abs(int(rtt[s]) - 60000) < 50 for s in ok), rtt
    assert int(rtt[forged]) == 0
    rows, err = R.call_stats(local.be, local.sessv, local.extv, nsess,
                             list(range(nsess)), peer.ssrc)
    assert not err.any() and (rows[:, 0] == 4).all() and \
        (rows[:, 6] == rtt).all()
