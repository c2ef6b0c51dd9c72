"""RTP receiver statistics on the GPU (include/re_rtp_stats_batch.h,
re_amd/csrc/hip/rtp_stats.hip) through the C-ABI library:

  * every case of tests/golden/rtp_source_golden.json.gz (the reference's
    own source.c / member.c / hash.c / rtp_hdr_decode) in one batch, one
    session per case, interleaved across the sessions: states, stat, report
    blocks, counts and RR descriptors bit-exact at every checkpoint;
  * 65 536 random packets over 4096 sessions against the host twin, as one
    call and as three consecutive calls on resident state;
  * one stream without a session array, 20 000 packets across two wraps,
    with and without arrival times;
  * the chain srtp_decrypt_batch_dev -> statistics (from its res) -> report
    (with RR descriptors) -> rtcp_encode_batch_dev ->
    rtcp_decode_full_batch_dev, all on device arrays;
  * windows outside the arena and session indices past nsess: EINVAL, the
    state untouched.
"""
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import rtp_stats_util as U

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


@pytest.mark.parametrize("g", [1, 0], ids=["arrival", "no_arrival"])
def test_golden_cases_one_batch(torch_cuda, g):
    cases = [c for c in U.load_cases() if bool(c["arrival"]) == bool(g)]
    assert cases
    U.replay_golden(U.DevMem(), cases)


# ---- random traffic against the host twin --------------------------------

NSESS, NPKT = 4096, 65536


@pytest.fixture(scope="module")
def traffic():
    """the traffic, and what the host twin makes of it in three consecutive
    calls (which a single call must equal too)"""
    rng = np.random.default_rng(20251)
    pkts, sess, arrival, res = U.random_traffic(rng, NSESS, NPKT)
    # a few session indices past nsess
    bad = rng.choice(NPKT, 40, replace=False)
    sess[bad] = NSESS + rng.integers(0, 3, 40).astype(np.uint32)
    be = U.HostMem()
    sessv = be.up(np.zeros(NSESS, U.SESS_DT))
    cuts = [0, NPKT // 3, NPKT // 3 + 20001, NPKT]
    stat, snaps = [], []
    for a, b in zip(cuts, cuts[1:]):
        stat.append(U.call_stats(be, pkts[a:b], sess[a:b], arrival[a:b],
                                 sessv, NSESS, res[a:b]))
        snaps.append(sessv.copy())
    return dict(pkts=pkts, sess=sess, arrival=arrival, res=res, cuts=cuts,
                stat=np.concatenate(stat), snaps=snaps)


def test_random_traffic_covers_every_path(traffic):
    """nothing below is compared vacuously"""
    stat, snaps = traffic["stat"], traffic["snaps"]
    for v in (0, P.RTP_RX_BADSEQ, P.RTP_RX_NOMEMBER, P.RTP_RX_SKIPPED,
              errno.EBADMSG, errno.EINVAL):
        assert (stat == v).any(), v
    final = snaps[-1]
    assert (final["m"]["cycles"] > 0).any()
    assert (final["memberc"] == 8).any() and (final["memberc"] == 1).any()
    # a resync: a source's base_seq moved between two calls
    moved = False
    for a, b in zip(snaps, snaps[1:]):
        had = (a["m"]["flags"] & P.RTP_RX_HAS_SOURCE) != 0
        moved |= bool((had & (a["m"]["base_seq"] != b["m"]["base_seq"])).any())
    assert moved
    # a packet whose jitter step was skipped: its source's timestamp again
    last, skipped = {}, 0
    for i in np.flatnonzero((stat == 0) | (stat == P.RTP_RX_BADSEQ)):
        p = traffic["pkts"][i]
        key, ts = (int(traffic["sess"][i]), p[8:12]), p[4:8]
        skipped += last.get(key, b"\0\0\0\0") == ts
        last[key] = ts
    assert skipped > 0


def _device_run(traffic, cuts):
    be = U.DevMem()
    sessv = be.up(np.zeros(NSESS, U.SESS_DT))
    stat = []
    for a, b in zip(cuts, cuts[1:]):
        stat.append(U.call_stats(be, traffic["pkts"][a:b],
                                 traffic["sess"][a:b],
                                 traffic["arrival"][a:b], sessv, NSESS,
                                 traffic["res"][a:b]))
    return np.concatenate(stat), be.down(sessv)


@pytest.mark.parametrize("calls", [1, 3])
def test_random_traffic_vs_host_twin(torch_cuda, traffic, calls):
    cuts = traffic["cuts"] if calls == 3 else [0, NPKT]
    stat, sessv = _device_run(traffic, cuts)
    bad = np.flatnonzero(stat != traffic["stat"])
    assert not len(bad), (bad[:8], stat[bad[:8]], traffic["stat"][bad[:8]])
    want = traffic["snaps"][-1]
    diff = [i for i in range(NSESS)
            if sessv[i].tobytes() != want[i].tobytes()]
    assert not diff, (len(diff), diff[:4], sessv[diff[0]], want[diff[0]])
    # and the reports of that state, on both sides
    hb, db = U.HostMem(), U.DevMem()
    ls = np.arange(NSESS, dtype=np.uint32) * 3 + 1
    h_sess, d_sess = hb.up(want), db.up(sessv)
    for now in (900000, 905000):
        h = U.call_report(hb, h_sess, NSESS, now, ls)
        d = U.call_report(db, d_sess, NSESS, now, ls)
        assert (h[1] == d[1]).all()
        assert h[0].tobytes() == d[0].tobytes()
        assert h[2].tobytes() == d[2].tobytes()
    assert db.down(d_sess).tobytes() == h_sess.tobytes()


# ---- one stream -----------------------------------------------------------

@pytest.mark.parametrize("with_arrival", [True, False])
def test_one_stream_two_wraps(torch_cuda, with_arrival):
    """sess == NULL: every packet to sessv[0], no grouping"""
    rng = np.random.default_rng(7)
    n = 20000
    step = rng.integers(1, 10, n)                   # ~5 per packet: 2 wraps
    seq = (64000 + np.cumsum(step)) & 0xffff
    ts = (0xfff00000 + np.cumsum(rng.integers(0, 500, n))) & 0xffffffff
    arr = (ts + 77777 + rng.integers(0, 300, n)) & 0xffffffff
    pkts = [U.rtp_packet(int(seq[i]), int(ts[i]), 0xabcdef01,
                         int(step[i])) for i in range(n)]
    arrival = arr.astype(np.uint32) if with_arrival else None
    out = []
    for be in (U.HostMem(), U.DevMem()):
        sessv = be.up(np.zeros(2, U.SESS_DT))
        stat = U.call_stats(be, pkts, None, arrival, sessv, 2)
        out.append((stat, be.down(sessv).copy()))
    (hs, hv), (ds, dv) = out
    assert (hs == 0).all() and (ds == hs).all()
    assert int(hv[0]["m"][0]["cycles"]) == 2 * 65536
    assert int(hv[0]["m"][0]["received"]) == n
    assert (int(hv[0]["m"][0]["jitter"]) > 0) == with_arrival
    assert dv.tobytes() == hv.tobytes()
    assert not dv[1].tobytes().strip(b"\0")


# ---- the chain -------------------------------------------------------------

def test_chain_unprotect_stats_report_encode_decode(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(99)
    nsess, per = 256, 6
    keys = bytes(rng.integers(0, 256, nsess * 30, dtype=np.uint8))
    e, tx = P.alloc_many(nsess, 1, keys)
    assert e == 0
    e, rx = P.alloc_many(nsess, 1, keys)
    assert e == 0
    # per session two SSRCs, increasing sequence numbers with a few losses
    n = nsess * per
    sess = rng.permutation(np.repeat(np.arange(nsess, dtype=np.uint32), per))
    seqs = np.zeros((nsess, 2), np.int64) + 100
    tss = np.zeros((nsess, 2), np.int64)
    pkts, arrival = [], []
    for i in range(n):
        s, k = int(sess[i]), int(rng.integers(0, 2))
        seqs[s, k] += int(rng.integers(1, 4))
        tss[s, k] += 160
        pkts.append(U.rtp_packet(int(seqs[s, k]), int(tss[s, k]),
                                 0x5000 + 2 * s + k, 24))
        arrival.append(int(tss[s, k]) + int(rng.integers(0, 90)) + 5000)
    slot = 64
    arena = np.zeros(n * slot, np.uint8)
    pos = np.arange(n, dtype=np.uint32) * slot
    end = pos + np.array([len(p) for p in pkts], np.uint32)
    for i, p in enumerate(pkts):
        arena[pos[i]:end[i]] = np.frombuffer(p, np.uint8)
    cap = pos + slot
    dev = lambda a: torch.from_numpy(
        np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_arena, d_pos, d_end, d_cap, d_sess = (dev(x) for x in
                                            (arena, pos, end, cap, sess))
    d_res = dev(np.full(n, -1, np.int32))
    rc = P.device_batch_dev("srtp_encrypt", tx, d_arena.data_ptr(),
                            arena.nbytes, d_pos.data_ptr(), d_end.data_ptr(),
                            d_cap.data_ptr(), d_res.data_ptr(), n,
                            d_sess.data_ptr())
    assert rc == 0, (rc, P.lib().srtp_gpu_error())
    assert not d_res.cpu().numpy().view(np.int32).any()
    # forge a few tags
    forged = rng.choice(n, 9, replace=False)
    e_end = d_end.cpu().numpy().view(np.uint32)
    d_arena[torch.from_numpy((e_end[forged] - 1).astype(np.int64)).cuda()] ^= 1
    rc = P.device_batch_dev("srtp_decrypt", rx, d_arena.data_ptr(),
                            arena.nbytes, d_pos.data_ptr(), d_end.data_ptr(),
                            d_cap.data_ptr(), d_res.data_ptr(), n,
                            d_sess.data_ptr())
    assert rc == 0, (rc, P.lib().srtp_gpu_error())
    # statistics from the unprotect's own res, all on the device
    d_arr = dev(np.array(arrival, np.uint32))
    d_sessv = dev(np.zeros(nsess, U.SESS_DT))
    d_stat = dev(np.full(n, 0x5a5a5a5a, np.int32))
    rc = P.rtp_rx_stats(d_arena.data_ptr(), arena.nbytes, d_pos.data_ptr(),
                        d_end.data_ptr(), d_res.data_ptr(),
                        d_sess.data_ptr(), d_arr.data_ptr(), n,
                        d_sessv.data_ptr(), nsess, d_stat.data_ptr())
    assert rc == 0, (rc, P.lib().srtp_gpu_error())
    d_rb = dev(np.zeros(nsess * 8, U.RB_DT))
    d_nrb = dev(np.zeros(nsess, np.uint32))
    d_msg = dev(np.zeros(nsess, U.MSG_DT))
    local = np.arange(nsess, dtype=np.uint32) + 0x77000000
    d_local = dev(local)
    rc = P.rtp_rx_report(d_sessv.data_ptr(), nsess, 123456, d_rb.data_ptr(),
                         d_nrb.data_ptr(), d_local.data_ptr(),
                         d_msg.data_ptr())
    assert rc == 0, (rc, P.lib().srtp_gpu_error())
    # one RR compound per session from those device arrays
    room = 256
    r_pos = np.arange(nsess, dtype=np.uint32) * room
    d_rarena = dev(np.zeros(nsess * room, np.uint8))
    d_rpos, d_rcap = dev(r_pos), dev(r_pos + room)
    d_rend = dev(np.zeros(nsess, np.uint32))
    d_mfirst = dev(np.arange(nsess + 1, dtype=np.uint32))
    d_err = dev(np.full(nsess, -1, np.int32))
    rc = P.rtcp_encode_dev(d_rarena.data_ptr(), nsess * room,
                           d_rpos.data_ptr(), d_rend.data_ptr(),
                           d_rcap.data_ptr(), nsess, d_mfirst.data_ptr(),
                           d_msg.data_ptr(), nsess, d_rb.data_ptr(),
                           nsess * 8, err_ptr=d_err.data_ptr())
    assert rc == 0, (rc, P.lib().srtp_gpu_error())
    maxitem = 8
    d_desc = dev(np.zeros(nsess * 5, np.uint32))
    d_item = dev(np.zeros(nsess * maxitem * 8, np.uint32))
    d_nmsg, d_nitem, d_derr, d_stop = (dev(np.zeros(nsess, np.uint32))
                                       for _ in range(4))
    rc = P.rtcp_decode_full_dev(d_rarena.data_ptr(), nsess * room,
                                d_rpos.data_ptr(), d_rend.data_ptr(), nsess,
                                d_desc.data_ptr(), 1, d_nmsg.data_ptr(),
                                d_item.data_ptr(), maxitem,
                                d_nitem.data_ptr(), d_derr.data_ptr(),
                                d_stop.data_ptr())
    assert rc == 0, (rc, P.lib().srtp_gpu_error())
    torch.cuda.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)

    # the host twin on the plaintext, with the same res
    res = d_res.cpu().numpy().view(np.int32)
    assert (res[forged] == EAUTH).all() and (res != 0).sum() == len(forged)
    stat = d_stat.cpu().numpy().view(np.int32)
    assert (stat[forged] == P.RTP_RX_SKIPPED).all()
    assert not np.delete(stat, forged).any()
    hb = U.HostMem()
    h_sessv = hb.up(np.zeros(nsess, U.SESS_DT))
    h_stat = U.call_stats(hb, pkts, sess, arrival, h_sessv, nsess, res)
    assert (h_stat == stat).all()
    h_rb, h_nrb, h_msg = U.call_report(hb, h_sessv, nsess, 123456, local)
    assert d_sessv.cpu().numpy().tobytes() == h_sessv.tobytes()
    assert (u32(d_nrb) == h_nrb).all() and h_nrb.min() >= 1 and \
        h_nrb.max() == 2
    assert (h_rb["lost"] != 0).any() and (h_rb["jitter"] != 0).any()
    assert not d_err.cpu().numpy().view(np.int32).any()
    assert (u32(d_rend) - r_pos == 8 + 24 * h_nrb).all()
    assert (u32(d_nmsg) == 1).all() and (u32(d_nitem) == h_nrb).all()
    desc = u32(d_desc).reshape(nsess, 5)
    assert (desc[:, 3] == local).all()              # the RR's sender
    item = u32(d_item).reshape(nsess, maxitem, 8)
    for i in range(nsess):
        for j in range(int(h_nrb[i])):
            w = [int(x) for x in item[i, j]]
            assert (w[0] >> 16) & 0xff == 2, (i, j, w)      # RTCP_ITEM_RB
            r = h_rb[i][j]
            want = [int(r["ssrc"]), int(r["fraction"]) & 0xff,
                    int(r["lost"]) & 0xffffff, int(r["last_seq"]),
                    int(r["jitter"]), int(r["lsr"]), int(r["dlsr"])]
            assert w[1:8] == want, (i, j, w, want)


# ---- bad windows ------------------------------------------------------------

def test_bad_windows_leave_state_untouched(torch_cuda):
    be = U.DevMem()
    nsess = 3
    sessv = be.up(np.zeros(nsess, U.SESS_DT))
    first = [U.rtp_packet(10 + i, 100 * i, 0x900 + (i % 4)) for i in range(24)]
    st = U.call_stats(be, first, [i % nsess for i in range(24)],
                      list(range(24)), sessv, nsess)
    assert not st.any()
    before = be.down(sessv).tobytes()
    assert before.strip(b"\0")

    good = U.rtp_packet(99, 5, 0x900)
    arena, pos, end = U.pack([good] * 8)
    n = len(pos)
    pos[0], end[0] = end[0], pos[0]                 # end < pos
    end[1] = arena.nbytes + 1                       # one past the arena
    pos[2], end[2] = arena.nbytes, arena.nbytes + 12    # wholly outside
    pos[3], end[3] = 0xfffffff0, 0xfffffffc
    pos[4], end[4] = 0, 0xffffffff
    sess = np.array([0, 1, 2, 0, 1, nsess, nsess + 1, 0xffffffff], np.uint32)
    hs = [be.up(x) for x in (arena, pos, end, sess,
                             np.arange(n, dtype=np.uint32))]
    stat = be.up(np.full(n, 0x5a5a5a5a, np.int32))
    rc = P.rtp_rx_stats(be.ptr(hs[0]), arena.nbytes, be.ptr(hs[1]),
                        be.ptr(hs[2]), None, be.ptr(hs[3]), be.ptr(hs[4]), n,
                        be.ptr(sessv), nsess, be.ptr(stat))
    assert rc == 0
    assert be.down(stat).tolist() == [errno.EINVAL] * n
    assert be.down(sessv).tobytes() == before
