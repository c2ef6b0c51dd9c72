"""The host twins rtcp_rx_handle_host / rtp_tx_stats_host /
rtcp_tx_report_host / rtcp_stats_host (include/re_rtcp_sess_batch.h) against
the reference's own decoder, member hash, sources and NTP routines driven as
src/rtp/sess.c drives them: every case of
tests/golden/rtcp_sess_golden.json.gz, bit-exact at every checkpoint --
members in hash order with cum_lost / jit / rtt, the transmit statistics, the
report blocks and their number, the SR / RR descriptors, the rtcp_stats rows
and errnos and the per-packet stat.  Needs no GPU.  (The encoded SR / RR
bytes are compared in tests/test_gpu_rtcp_sess.py: the encoder is on the
device.)
"""
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import rtp_stats_util as U
from tests import rtcp_sess_util as R


def test_golden_has_every_case_kind():
    cases = R.load_cases()
    names = {c["name"] for c in cases}
    assert len(names) == len(cases) >= 12
    kinds = set().union(*[c["kinds"] for c in cases])
    assert kinds == set(R.KINDS), set(R.KINDS) ^ kinds
    ops = [s["op"] for s in cases[0]["stages"]]
    assert ops == ["rtp", "tx", "rtcp", "check", "report", "check", "rtcp",
                   "rtp", "tx", "check", "report", "stats"]
    pts = {m[2] for c in cases for s in c["stages"] if s["op"] == "rtcp"
           for p in s["pk"] for m in p["msgs"]}
    assert {200, 201, 202, 203, 204, 206} <= pts
    assert {s["pt"] for c in cases for s in c["stages"]
            if s["op"] == "report"} == {200, 201}
    assert {p["stat"] for c in cases for s in c["stages"]
            if s["op"] == "rtcp" for p in s["pk"]} == {"ok", "nomember"}
    assert {q[1] for c in cases for q in c["stages"][-1]["q"]} == \
        {0, errno.ENOENT}
    assert any(c["srate_tx"] == 0 for c in cases)
    assert any(c["srate_rx"] == 0 for c in cases)


@pytest.mark.parametrize("case", R.load_cases(), ids=lambda c: c["name"])
def test_host_twin_golden_case(case):
    R.replay_golden(U.HostMem(), [case])


def test_host_twin_golden_one_batch():
    R.replay_golden(U.HostMem(), R.load_cases())


def _one_sr(ssrc, nblocks=0):
    msgs = [[0, 28 + 24 * nblocks, 200, nblocks, 6 + 6 * nblocks, ssrc, 5]]
    items = [[0, R.ITEM_SR, 0, 1, 2, 5, 4, 5, 0, 0]] + \
        [[0, R.ITEM_RB, 0, 9, 0, 0xfffffe, 1, 8, 0, 0]] * nblocks
    return msgs, items


def test_host_twin_stat_values():
    """skipped, bad session, truncated by messages and by items: nothing of
    such a packet is applied; a 9th SSRC: the packet's other messages are"""
    be = U.HostMem()
    rows = [_one_sr(0x10 + i) for i in range(8)]          # fill session 0
    rows += [_one_sr(0x99),                               # [8] skipped
             _one_sr(0x98),                               # [9] sess >= nsess
             (_one_sr(0x97)[0] * 3, _one_sr(0x97)[1]),    # [10] 3 messages
             _one_sr(0x96, 4),                            # [11] 5 items
             ([[0, 8, 201, 0, 1, 0x95, 0]] +              # [12] 9th, then BYE
              [[8, 8, 203, 1, 1, 0x10, 0]],
              [[1, R.ITEM_BYE_SRC, 0, 0x10, 0, 0, 0, 0, 0, 0]])]
    sess = [0] * 8 + [1, 2, 1, 1, 0]
    res = [0] * 8 + [217, 0, 0, 0, 0]
    desc, nmsg, item, nitem = R.decoded_arrays(rows, 2, 4)
    sessv_h = be.up(np.zeros(2, R.SESS_DT))
    extv_h = be.up(R.fresh_ext(2, 8000, 8000))
    stat = R.call_handle(be, desc, 2, nmsg, item, 4, nitem, res, sess,
                         len(rows), sessv_h, extv_h, 2, 1000, 1 << 50)
    assert stat.tolist() == [0] * 8 + [
        P.RTP_RX_SKIPPED, errno.EINVAL, P.RTCP_RX_TRUNCATED,
        P.RTCP_RX_TRUNCATED, P.RTP_RX_NOMEMBER]
    assert int(sessv_h[0]["memberc"]) == 7                # the BYE counted
    assert sessv_h[0]["m"]["ssrc"].tolist() == \
        [0x11 + i for i in range(7)] + [0]
    assert not sessv_h[1].tobytes().strip(b"\0")
    assert not extv_h[1]["cum_lost"].any()
    R.check_invariant(sessv_h, extv_h)


def test_host_twin_tx_bad_windows_and_skips():
    be = U.HostMem()
    good = bytes([0x82, 96, 0, 1]) + (77).to_bytes(4, "big") + b"\0" * 4 + \
        b"\x11" * 8 + b"\xa5" * 10                        # 2 CSRCs, payload 10
    pkts = [good, good, good, good, good, good, good[:19], good[:20],
            bytes([0x42]) + good[1:], good[:11]]
    arena, pos, end = U.pack(pkts)
    n = len(pos)
    pos[1], end[1] = end[1], pos[1]                       # end < pos
    end[2] = arena.nbytes + 1                             # past the arena
    pos[3] = end[3] = arena.nbytes + 40                   # empty, outside
    sess = np.array([0, 0, 0, 0, 2, 0, 0, 0, 0, 0], np.uint32)
    res = np.array([0, 0, 0, 0, 0, 217, 0, 0, 0, 0], np.int32)
    jfs = np.arange(100, 100 + n, dtype=np.uint64)
    extv = R.fresh_ext(2, 8000, 8000)
    stat = np.full(n, 99, np.int32)
    rc = P.rtp_tx_stats(arena.ctypes.data, arena.nbytes, pos.ctypes.data,
                        end.ctypes.data, res.ctypes.data, sess.ctypes.data,
                        jfs.ctypes.data, n, extv.ctypes.data, 2,
                        stat.ctypes.data, host=True)
    assert rc == 0
    assert stat.tolist() == [0, errno.EINVAL, errno.EINVAL, errno.EINVAL,
                             errno.EINVAL, P.RTP_RX_SKIPPED, errno.EBADMSG,
                             0, errno.EBADMSG, errno.EBADMSG]
    assert R.tx_row(extv[0]) == [2, 10, 100, 77, 1]       # [7]: header only
    assert not extv[1]["psent"] and not extv[1]["ts_synced"]
    assert be.host


def test_host_twin_arguments():
    sessv = np.zeros(1, R.SESS_DT)
    extv = R.fresh_ext(1, 8000, 8000)
    desc, nmsg, item, nitem = R.decoded_arrays([_one_sr(1)], 1, 1)
    a = np.zeros(16, np.uint8)
    z = np.zeros(1, np.uint32)
    j = np.zeros(1, np.uint64)
    out = np.zeros(7, np.uint32)
    err = np.zeros(1, np.int32)

    def handle(d=desc, mm=1, nm=nmsg, it=item, mi=1, ni=nitem, n=1, sv=sessv,
               xv=extv, ns=1):
        p = [None if x is None else x.ctypes.data
             for x in (d, nm, it, ni, sv, xv)]
        return P.rtcp_rx_handle(p[0], mm, p[1], p[2], mi, p[3], None, None,
                                n, p[4], p[5], ns, 0, 0, None, host=True)

    assert handle() == 0                                  # stat may be NULL
    assert handle(n=0, d=None, sv=None, ns=0) == 0
    for bad in (dict(d=None), dict(nm=None), dict(it=None), dict(ni=None),
                dict(sv=None), dict(xv=None), dict(ns=0), dict(mm=0),
                dict(mi=0), dict(mm=65537)):
        assert handle(**bad) == errno.EINVAL, bad

    def tx(ar=a, po=z, en=z, jf=j, n=1, xv=extv, ns=1):
        p = [None if x is None else x.ctypes.data for x in (ar, po, en, jf, xv)]
        return P.rtp_tx_stats(p[0], 16, p[1], p[2], None, None, p[3], n,
                              p[4], ns, None, host=True)

    assert tx() == 0 and tx(n=0, ar=None, ns=0) == 0
    for bad in (dict(ar=None), dict(po=None), dict(en=None), dict(jf=None),
                dict(xv=None), dict(ns=0)):
        assert tx(**bad) == errno.EINVAL, bad

    rb = np.zeros(8, R.RB_DT)
    msg = np.zeros(1, R.MSG_DT)
    ok = (sessv.ctypes.data, extv.ctypes.data, 1, 0, 0, rb.ctypes.data,
          z.ctypes.data, z.ctypes.data, msg.ctypes.data)
    assert P.rtcp_tx_report(*ok, host=True) == 0
    assert P.rtcp_tx_report(None, None, 0, 0, 0, None, None, None, None,
                            host=True) == 0
    for k in (0, 1, 5, 6, 7, 8):
        bad = list(ok)
        bad[k] = None
        assert P.rtcp_tx_report(*bad, host=True) == errno.EINVAL, k

    ok = (sessv.ctypes.data, extv.ctypes.data, 1, None, z.ctypes.data, 1,
          out.ctypes.data, err.ctypes.data)
    assert P.rtcp_stats(*ok, host=True) == 0
    assert int(err[0]) == errno.ENOENT and not out.any()
    assert P.rtcp_stats(None, None, 0, None, None, 0, None, None,
                        host=True) == 0
    for k in (0, 1, 4, 6, 7):
        bad = list(ok)
        bad[k] = None
        assert P.rtcp_stats(*bad, host=True) == errno.EINVAL, k
    bad = list(ok)
    bad[2] = 0
    assert P.rtcp_stats(*bad, host=True) == errno.EINVAL
    # a query for a session that does not exist
    s2 = np.array([1], np.uint32)
    assert P.rtcp_stats(sessv.ctypes.data, extv.ctypes.data, 1,
                        s2.ctypes.data, z.ctypes.data, 1, out.ctypes.data,
                        err.ctypes.data, host=True) == 0
    assert int(err[0]) == errno.EINVAL


def test_device_entries_without_gpu_or_with_bad_arguments():
    """the device entries check their arguments before they look for a
    device"""
    assert P.rtcp_rx_handle(None, 1, None, None, 1, None, None, None, 0,
                            None, None, 0, 0, 0, None) == 0
    assert P.rtcp_rx_handle(None, 1, None, None, 1, None, None, None, 1,
                            None, None, 1, 0, 0, None) == errno.EINVAL
    assert P.rtp_tx_stats(None, 0, None, None, None, None, None, 1, None, 1,
                          None) == errno.EINVAL
    assert P.rtcp_tx_report(None, None, 1, 0, 0, None, None, None,
                            None) == errno.EINVAL
    assert P.rtcp_stats(None, None, 1, None, None, 1, None,
                        None) == errno.EINVAL


def test_random_traffic_reaches_everything():
    """The random traffic of tests/test_gpu_rtcp_sess.py, through the host
    twin: it reaches every stat value, every removal position, full tables,
    re-adds, maxmsg / maxitem overflow, both report kinds and every
    rtcp_stats errno -- so the device-against-host-twin comparison there is
    not vacuous.  The compounds are also applied one call per packet, which
    shows where each BYE removed its member and gives the batch's states."""
    parts, q_sess, q_ssrc = R.session_traffic()
    out = R.run_session_traffic(U.HostMem(), parts, q_sess, q_ssrc)
    hstat = np.concatenate([out[2], out[5], out[8]])
    assert set(hstat.tolist()) == {0, P.RTP_RX_SKIPPED, errno.EINVAL,
                                   P.RTP_RX_NOMEMBER, P.RTCP_RX_TRUNCATED}
    tstat = np.concatenate([out[1], out[4], out[7]])
    assert set(tstat.tolist()) == {0, P.RTP_RX_SKIPPED, errno.EINVAL,
                                   errno.EBADMSG}
    nmsg = np.concatenate([p["rtcp"][1] for p in parts])
    nitem = np.concatenate([p["rtcp"][3] for p in parts])
    assert (nmsg > R.T_MAXMSG).any()
    assert ((nitem > R.T_MAXITEM) & (nmsg <= R.T_MAXMSG)).any()
    rbv, nrb, msgv, rows, err = out[9:14]
    assert set(msgv["pt"].tolist()) == {200, 201}
    assert set(nrb.tolist()) == set(range(9))
    assert set(err.tolist()) == {0, errno.ENOENT, errno.EINVAL}
    assert rows[err == 0][:, 6].any() and rows[err == 0][:, 3].any()

    nsess = R.T_NSESS
    sessv, extv = np.zeros(nsess, R.SESS_DT), out[-1].copy()
    for f in ("cum_lost", "jit", "rtt", "psent", "osent", "jfs_rt_ref",
              "ts_ref", "ts_synced"):
        extv[f] = 0
    be = U.HostMem()
    gone = [set() for _ in range(nsess)]
    removed, readd, full = set(), 0, 0
    for p in parts:
        U.call_stats(be, *p["rtp"], sessv, nsess)
        R.call_tx(be, *p["tx"][:3], extv, nsess, p["tx"][3])
        desc, nmsg, item, nitem, sess, res = p["rtcp"]
        st1 = np.zeros(1, np.int32)
        for i in range(len(sess)):
            s = int(sess[i]) if sess[i] < nsess else 0
            mc = int(sessv[s]["memberc"])
            before = sessv[s]["m"]["ssrc"][:mc].tolist()
            rc = P.rtcp_rx_handle(desc[i:].ctypes.data, R.T_MAXMSG,
                                  nmsg[i:].ctypes.data, item[i:].ctypes.data,
                                  R.T_MAXITEM, nitem[i:].ctypes.data,
                                  res[i:].ctypes.data, sess[i:].ctypes.data,
                                  1, sessv.ctypes.data, extv.ctypes.data,
                                  nsess, p["recv_ms"], p["now_us"],
                                  st1.ctypes.data, host=True)
            assert rc == 0
            mc = int(sessv[s]["memberc"])
            after = sessv[s]["m"]["ssrc"][:mc].tolist()
            full += mc == 8
            if len(before) >= 3:
                for k, x in enumerate(before):
                    if x not in after:
                        removed.add("first" if k == 0 else "last"
                                    if k + 1 == len(before) else "middle")
            gone[s].update(x for x in before if x not in after)
            readd += any(x in gone[s] and x not in before for x in after)
    assert removed == {"first", "middle", "last"}
    assert readd > 100 and full > 100
    # packet by packet the twin leaves what the three batches left (the
    # report afterwards changed only the priors and ts_synced)
    assert (sessv["memberc"] == out[-2]["memberc"]).all()
    assert (sessv["m"]["ssrc"] == out[-2]["m"]["ssrc"]).all()
    for f in ("cum_lost", "jit", "rtt", "psent", "osent", "jfs_rt_ref"):
        assert (extv[f] == out[-1][f]).all(), f
    R.check_invariant(out[-2], out[-1])
