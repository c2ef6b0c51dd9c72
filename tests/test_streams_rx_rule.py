"""The reordered one-session multi-SSRC receive planner's rule on the CPU:
tests/c/streams_rx_check.c includes re_amd/csrc/hip/plan_rx_rule.h and
plan_rtp_seg_rx.h as C, runs random interleaved one-session batches of 1-9
SSRCs (swaps up to 8 apart, gaps, duplicates, replays of the batch before,
jumps, streams starting just below a ROC wrap, tables carried from batch to
batch) through the decomposition of plan_streams_rx.hip -- small workgroup,
wave and per-thread widths, look-backs of 2-13 as well as 128 -- and through a
sequential stream_get_seq + srtp_decrypt index / replay receiver, under
AddressSanitizer + UBSan (a stand-alone program run as a child process, as
tests/test_rtp_seg_rx_rule.py does).  The same program's sequential receiver
then takes the random traffic of tests/srx_traffic.py, which
tests/test_gpu_srxplan.py sends through the library.
"""
import os
import re
import subprocess

import pytest

from tests import srx_traffic as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("streams_rx") / "streams_rx_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=all", "-o", path,
                           os.path.join(ROOT, "tests", "c",
                                        "streams_rx_check.c")])
    return path


def run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    return r.stdout


def test_streams_rx_rule_against_sequential_receiver(exe):
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


@pytest.mark.parametrize("seed", T.SEEDS)
def test_random_traffic_is_settled_by_the_sequential_receiver(exe, tmp_path,
                                                               seed):
    """the generator of tests/test_gpu_srxplan.py's random batches: the
    sequential receiver answers only 0 / EALREADY, every batch is disturbed,
    and every batch is one the rule settles -- so the GPU test leaves out no
    batch"""
    batches = T.random_batches(seed)
    path = str(tmp_path / "traffic.txt")
    T.write_traffic(path, batches)
    rows = re.findall(r"batch (\d+): (\d+) packets ok (\d+) already (\d+) "
                      r"timedout (\d+) other (\d+) disturbed (\d+) streams "
                      r"(\d+) plan (\w+) must (\d)", run([exe, path]))
    assert len(rows) == len(batches) == 2
    already = 0
    nst = []
    for row, (sent, arrive, ndist) in zip(rows, batches):
        _, n, ok, dup, timedout, other, ooo, streams = \
            (int(x) for x in row[:8])
        assert n == len(arrive) <= 1400 and ndist > 0 and ooo > 0
        assert timedout == 0 and other == 0 and ok + dup == n, row
        assert row[8] == "accepted" and row[9] == "1", row
        already += dup
        nst.append(streams)
    assert already > 0
    # the second batch opens a stream behind known ones
    assert 2 <= nst[0] == nst[1] - 1 <= 7
