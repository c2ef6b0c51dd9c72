"""The traffic generators of tests/test_gpu_srtcp_multi.py through the oracle
alone: every scenario runs to its end (its coverage guard -- the errno
classes it is meant to produce, asserted on the oracle's rows -- and the
table-fill probe hold), and two runs from one seed give identical batches
and rows.  So the inputs do what the GPU cases rely on, shown without a GPU.
"""
import errno

import pytest

import re_amd.srtp as P
from tests import test_gpu_srtcp_multi as M

U = P.SRTP_UNENCRYPTED_SRTCP


def twice(scn, suite, flags, nsess, *args, fixed=True, **kw):
    logs = []
    for _ in range(2):
        d = M.OracleDrive(suite, flags, nsess, fixed)
        try:
            logs.append(scn(d, *args, **kw))
            errs = d.errs
        finally:
            d.close()
    assert logs[0] == logs[1]
    return logs[0], errs


@pytest.mark.parametrize("flags", [0, U], ids=["e", "u"])
@pytest.mark.parametrize("suite", list(range(6)))
def test_round_trip(suite, flags):
    log, errs = twice(M.scn_round_trip, suite, flags, 40, 110 + 2 * suite +
                      flags)
    # six packets per batch lack one byte, six fit exactly
    assert errs["tx"][errno.ENOMEM] == 12
    sizes = [len(p) for _, p in log[0][2]]
    assert 4028 in sizes and 4100 in sizes and len(sizes) == 600
    # every stream count 1..8 occurs among the sessions
    per = {}
    for s, p in log[0][2] + log[2][2]:
        per.setdefault(s, set()).add(p[4:8])
    assert {len(v) for v in per.values()} == set(range(1, 9))
    # where the mbufs grow, the same rooms refuse nothing
    log, errs = twice(M.scn_round_trip, suite, flags, 1, 150 + 2 * suite +
                      flags, fixed=False, n=300)
    assert set(errs["tx"]) == {0, errno.ENOSR} and set(errs["rx"]) == \
        {0, errno.ENOSR}
    assert len({p[4:8] for _, p in log[0][2]}) == 8


@pytest.mark.parametrize("case", M.SUB, ids=M.sub_ids)
def test_trouble(case):
    suite, flags = case
    log, errs = twice(M.scn_trouble, suite, M.trouble_flags(flags),
                      M.NTROUBLE, 170 + 2 * suite + flags)
    rx = errs["rx"]
    assert rx[P.EAUTH] >= 4 * M.NTROUBLE and rx[errno.EBADMSG] >= \
        2 * M.NTROUBLE and rx[errno.ENOSR] >= 2
    if M.has_hmac(suite):
        # a duplicate and a repeat per session, and the packet 64 behind
        assert rx[errno.EALREADY] >= 2 * M.NTROUBLE + 1
    assert max(len(step[2]) for step in log) <= 600


@pytest.mark.parametrize("which", ["ab", "c", "d"])
@pytest.mark.parametrize("case", M.SUB, ids=M.sub_ids)
def test_unknown_stream(case, which):
    suite, flags = case
    twice(M.scn_unknown_stream, suite, flags, 1, 190 + 2 * suite + flags,
          which)


@pytest.mark.parametrize("case", M.SUB, ids=M.sub_ids)
def test_wrap(case):
    suite, flags = case
    log, errs = twice(M.scn_wrap, suite, flags, 1, 210 + 2 * suite + flags)
    if M.has_hmac(suite):
        # B's five packets behind the wrap lie below its window
        assert errs["rx"][errno.EALREADY] == 5


@pytest.mark.parametrize("suite", M.MUX_SUITES)
def test_mux(suite):
    twice(M.scn_mux, suite, 0, M.NMUX, 230 + suite)


@pytest.mark.parametrize("shape", ["same", "other", "many"])
@pytest.mark.parametrize("suite", M.MUX_SUITES)
def test_srtcp_first(suite, shape):
    if shape == "many":
        twice(M.scn_srtcp_first, suite, 0, M.NMUX, 250 + suite, False)
    else:
        twice(M.scn_srtcp_first, suite, 0, 1, 260 + suite, shape == "other")
