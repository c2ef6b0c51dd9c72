"""The host twins rtp_rx_stats_host / rtp_rx_sr_host / rtp_rx_report_host
(include/re_rtp_stats_batch.h) against the reference's own sequence tracker,
jitter estimator, member hash and header decode: every case of
tests/golden/rtp_source_golden.json.gz, bit-exact -- per-packet stat, every
member's state in hash_apply order at every checkpoint, and the report
blocks of two successive reports.  Needs no GPU.
"""
import errno

import numpy as np
import pytest

import re_amd.srtp as P
from tests import rtp_stats_util as U


def _groups():
    cases = U.load_cases()
    return [[c for c in cases if c["arrival"]],
            [c for c in cases if not c["arrival"]]]


def test_golden_has_every_case_kind():
    cases = U.load_cases()
    names = {c["name"] for c in cases}
    assert len(names) == len(cases) >= 20
    stats = {p[2] for c in cases for s in c["stages"] if s["op"] == "rtp"
             for p in s["pk"]}
    assert stats == {"ok", "badseq", "nomember", "badmsg"}
    assert any(not c["arrival"] for c in cases)


@pytest.mark.parametrize("case", U.load_cases(), ids=lambda c: c["name"])
def test_host_twin_golden_case(case):
    U.replay_golden(U.HostMem(), [case])


@pytest.mark.parametrize("g", [0, 1], ids=["arrival", "no_arrival"])
def test_host_twin_golden_one_batch(g):
    U.replay_golden(U.HostMem(), _groups()[g])


def test_host_twin_bad_windows_and_skips():
    be = U.HostMem()
    good = U.rtp_packet(7, 1000, 0x55)
    arena, pos, end = U.pack([good] * 6)
    n = len(pos)
    pos[1], end[1] = end[1], pos[1]             # end < pos
    end[2] = arena.nbytes + 1                   # past the arena
    pos[3] = end[3] = arena.nbytes + 40         # empty, outside
    sess = np.array([0, 0, 0, 0, 2, 0], np.uint32)      # [4]: sess >= nsess
    res = np.array([0, 0, 0, 0, 0, 217], np.int32)      # [5]: skipped
    sessv = np.zeros(2, U.SESS_DT)
    stat = np.full(n, 99, np.int32)
    rc = P.rtp_rx_stats(arena.ctypes.data, arena.nbytes, pos.ctypes.data,
                        end.ctypes.data, res.ctypes.data, sess.ctypes.data,
                        None, n, sessv.ctypes.data, 2, stat.ctypes.data,
                        host=True)
    assert rc == 0
    assert stat.tolist() == [0, errno.EINVAL, errno.EINVAL, errno.EINVAL,
                             errno.EINVAL, P.RTP_RX_SKIPPED]
    assert int(sessv[0]["memberc"]) == 1 and \
        int(sessv[0]["m"][0]["received"]) == 1
    assert not sessv[1].tobytes().strip(b"\0")
    assert be.host


def test_host_twin_arguments():
    sessv = np.zeros(1, U.SESS_DT)
    a = np.zeros(16, np.uint8)
    z = np.zeros(1, np.uint32)
    assert P.rtp_rx_stats(a.ctypes.data, 16, z.ctypes.data, z.ctypes.data,
                          None, None, None, 0, None, 0, None, host=True) == 0
    assert P.rtp_rx_stats(None, 16, z.ctypes.data, z.ctypes.data, None, None,
                          None, 1, sessv.ctypes.data, 1, None,
                          host=True) == errno.EINVAL
    assert P.rtp_rx_stats(a.ctypes.data, 16, z.ctypes.data, z.ctypes.data,
                          None, None, None, 1, sessv.ctypes.data, 0, None,
                          host=True) == errno.EINVAL
    # stat may be NULL
    assert P.rtp_rx_stats(a.ctypes.data, 16, z.ctypes.data, z.ctypes.data,
                          None, None, None, 1, sessv.ctypes.data, 1, None,
                          host=True) == 0
    assert P.rtp_rx_report(sessv.ctypes.data, 1, 0, None, None,
                           host=True) == errno.EINVAL
