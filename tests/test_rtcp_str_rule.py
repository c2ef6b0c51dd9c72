"""The one-session SRTCP planner's rule on the CPU: tests/c/rtcp_str_check.c
includes re_amd/csrc/hip/plan_rtcp_str.h (over plan_rtcp_seg.h,
plan_rtcp_seg_rx.h and plan_rx_rule.h) as C and runs random one-session worlds
of 1-9 SSRCs -- tables carried from batch to batch, known streams, streams RTP
created, room for new ones or none; per batch protect, then unprotect with and
without a replay window; swaps up to 8 apart, duplicates, replays of the batch
before, streams starting at 0x7ffffff0, first arrivals at lix - 63, lix - 64
and on a set bit -- through the decomposition of plan_streams_rtcp.hip with
small workgroup, wave and scan-thread widths and look-backs of 2-13 as well as
128, and through a sequential stream_get + srtcp.c:54 / srtcp.c:208 +
replay.c:32-62 sender and receiver, under AddressSanitizer + UBSan (a
stand-alone program run as a child process, as tests/test_streams_rx_rule.py
does).  The same program's sequential receiver then takes the random traffic
of tests/srtcp_str_traffic.py, which tests/test_gpu_srtcp_splan.py sends
through the library.
"""
import os
import re
import subprocess

import pytest

from tests import srtcp_str_traffic as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rtcp_str") / "rtcp_str_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=all", "-o", path,
                           os.path.join(ROOT, "tests", "c",
                                        "rtcp_str_check.c")])
    return path


def run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    return r.stdout


def test_rtcp_str_rule_against_sequential_sender_and_receiver(exe):
    out = run([exe])
    m = re.search(r"(\d+) accepted \((\d+) must\), (\d+) rejected "
                  r"\(\d+ unsettled\), (\d+) wrong", out)
    assert m, out[-4000:]
    accepted, must, rejected, wrong = (int(x) for x in m.groups())
    assert wrong == 0
    # exactly the batches of at most 8 streams that the sequential per-stream
    # rx_replay settles
    assert accepted == must
    # it accepted and it rejected: neither property held vacuously
    assert accepted != 0 and rejected != 0


@pytest.mark.parametrize("seed", T.SEEDS)
def test_random_traffic_is_settled_by_the_sequential_receiver(exe, tmp_path,
                                                               seed):
    """the generator of tests/test_gpu_srtcp_splan.py's random batches: the
    sequential receiver answers only 0 / EALREADY with some EALREADY, every
    batch is disturbed, and every batch is one the rule settles at the
    kernels' own widths -- so the GPU test leaves out no batch"""
    _, batches = T.random_batches(seed)
    path = str(tmp_path / "traffic.txt")
    T.write_traffic(path, batches)
    rows = re.findall(r"batch (\d+): (\d+) packets ok (\d+) already (\d+) "
                      r"other (\d+) disturbed (\d+) streams (\d+) plan (\w+) "
                      r"must (\d)", run([exe, path]))
    assert len(rows) == len(batches) == 2
    already = 0
    nst = []
    for row, (sent, arrive, ndist) in zip(rows, batches):
        _, n, ok, dup, other, ooo, streams = (int(x) for x in row[:7])
        assert n == len(arrive) <= 1400 and ndist > 0 and ooo > 0
        assert other == 0 and ok + dup == n, row
        assert row[7] == "accepted" and row[8] == "1", row
        already += dup
        nst.append(streams)
    assert already > 0
    # the second batch opens a stream behind known ones
    assert 2 <= nst[0] == nst[1] - 1 <= 7
