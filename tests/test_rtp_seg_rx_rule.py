"""The reordered multi-SSRC receive planner's rule
(re_amd/csrc/hip/plan_rtp_seg_rx.h) on the CPU: tests/c/rtp_seg_rx_check.c
includes the header as C, runs random interleaved batches of 2-40 sessions
with 1-9 SSRCs each (swaps, gaps, duplicates, replays of the batch before,
jumps) through the composition in the decomposition of k_bsr_plan
(plan_buckets_rtp_streams_rx.hip) and through a sequential stream_get_seq +
srtp_decrypt index / replay receiver, under AddressSanitizer + UBSan (a
stand-alone program run as a child process, as tests/test_rtp_seg_rule.py
does).  The same program's sequential receiver then takes the random traffic
of tests/msrx_traffic.py, which tests/test_gpu_msrxplan.py sends through the
library.
"""
import os
import re
import subprocess

import pytest

from tests import msrx_traffic as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rtp_seg_rx") / "rtp_seg_rx_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=all", "-o", path,
                           os.path.join(ROOT, "tests", "c",
                                        "rtp_seg_rx_check.c")])
    return path


def run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    return r.stdout


def test_rtp_seg_rx_rule_against_sequential_receiver(exe):
    out = run([exe])
    m = re.search(r"(\d+) accepted \((\d+) must\), (\d+) rejected, (\d+) wrong",
                  out)
    assert m, out[-4000:]
    accepted, must, rejected, wrong = (int(x) for x in m.groups())
    assert wrong == 0
    # exactly the batches the sequential per-stream rx_settle settles
    assert accepted == must
    # it accepted and it rejected: neither property held vacuously
    assert accepted != 0 and rejected != 0


@pytest.mark.parametrize("seed", [701, 702])
def test_random_traffic_is_settled_by_the_sequential_receiver(exe, tmp_path,
                                                               seed):
    """the generator of tests/test_gpu_msrxplan.py's random batches: the
    sequential receiver answers only 0 / EALREADY, every batch is disturbed,
    and every batch is one the rule settles"""
    batches = T.random_batches(seed)
    path = str(tmp_path / "traffic.txt")
    T.write_traffic(path, batches)
    rows = re.findall(r"batch (\d+): (\d+) packets ok (\d+) already (\d+) "
                      r"timedout (\d+) other (\d+) plan (\w+) must (\d)",
                      run([exe, path]))
    assert len(rows) == len(batches)
    already = 0
    for row, (sent, arrive, ndist) in zip(rows, batches):
        _, n, ok, dup, timedout, other = (int(x) for x in row[:6])
        assert n == len(arrive) <= 600 and ndist > 0
        assert timedout == 0 and other == 0 and ok + dup == n, row
        assert row[6] == "accepted" and row[7] == "1", row
        already += dup
    assert already > 0
