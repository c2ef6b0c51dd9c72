"""The many-session SRTCP receive planner's rule
(re_amd/csrc/hip/plan_rtcp_seg_rx.h) on the CPU: tests/c/rtcp_seg_rx_check.c
includes the header as C, runs random interleaved batches of 2-40 sessions
with 1-9 SSRCs each (swaps, gaps, duplicates, replays of the batch before,
indices more than 64 below the top, streams next to the 31-bit wrap) through
the composition in the decomposition of k_bprx_plan
(plan_buckets_rtcp_rx.hip), with small widths and look-backs, and through a
sequential stream_get + srtp_replay_check receiver, under AddressSanitizer +
UBSan (a stand-alone program run as a child process, as
tests/test_rtp_seg_rx_rule.py does).  The same program's sequential receiver
then takes the random traffic of tests/mrtcp_rx_traffic.py, which
tests/test_gpu_srtcp_mrxplan.py sends through the library.
"""
import os
import re
import subprocess

import pytest

from tests import mrtcp_rx_traffic as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rtcp_seg_rx") / "rtcp_seg_rx_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=all", "-o", path,
                           os.path.join(ROOT, "tests", "c",
                                        "rtcp_seg_rx_check.c")])
    return path


def run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    return r.stdout


def test_rtcp_seg_rx_rule_against_sequential_receiver(exe):
    out = run([exe])
    m = re.search(r"(\d+) batches: (\d+) accepted \((\d+) must\), (\d+) "
                  r"rejected \((\d+) unsettled\), (\d+) wrong", out)
    assert m, out[-4000:]
    total, accepted, must, rejected, unsettled, wrong = \
        (int(x) for x in m.groups())
    assert total >= 5000
    assert wrong == 0
    # exactly the batches the sequential per-stream rx_replay settles
    assert accepted == must
    # it accepted and it rejected, for a copy beyond the look-back too:
    # neither property held vacuously
    assert accepted != 0 and rejected != 0 and unsettled != 0


@pytest.mark.parametrize("seed", [801, 802])
def test_random_traffic_is_settled_by_the_sequential_receiver(exe, tmp_path,
                                                               seed):
    """the generator of tests/test_gpu_srtcp_mrxplan.py's random batches: the
    sequential receiver answers only 0 / EALREADY, every batch is disturbed,
    and every batch is one the rule settles"""
    _, batches = T.random_batches(seed)
    path = str(tmp_path / "traffic.txt")
    T.write_traffic(path, batches)
    rows = re.findall(r"batch (\d+): (\d+) packets ok (\d+) already (\d+) "
                      r"other (\d+) plan (\w+) must (\d)", run([exe, path]))
    assert len(rows) == len(batches)
    already = 0
    for row, (sent, arrive, ndist) in zip(rows, batches):
        _, n, ok, dup, other = (int(x) for x in row[:5])
        assert n == len(arrive) <= 600 and ndist > 0
        assert arrive != [(int(row[0]), i) for i in range(len(sent))]
        assert other == 0 and ok + dup == n, row
        assert row[5] == "accepted" and row[6] == "1", row
        already += dup
    assert already > 0
