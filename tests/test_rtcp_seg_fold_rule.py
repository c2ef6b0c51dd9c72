"""The rule that settles forged packets of many-session SRTCP unprotect batches
(re_amd/csrc/hip/plan_rtcp_seg_fold.h) on the CPU: tests/c/rtcp_seg_fold_check.c
includes the header as C, runs random interleaved batches of 2-40 sessions
with 1-9 SSRCs each (the disturbances of tests/c/rtcp_seg_rx_check.c and about
5 % forged arrivals: far above the top, copies ahead of and behind the genuine
packet, on an unset bit of the stored window, whole streams, SSRCs opened by a
forged packet alone) through the decomposition of k_bprf_settle
(plan_buckets_rtcp_fold.hip), with small widths and look-backs, and through a
sequential stream_get + tag + srtp_replay_check receiver, under
AddressSanitizer + UBSan (a stand-alone program run as a child process, as
tests/test_rtcp_seg_rx_rule.py does).  The same program's sequential receiver
then takes the random traffic of tests/mrtcp_fold_traffic.py, which
tests/test_gpu_srtcp_mfold.py sends through the library.
"""
import os
import re
import subprocess

import pytest

from tests import mrtcp_fold_traffic as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rtcp_seg_fold") / "rtcp_seg_fold_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=all", "-o", path,
                           os.path.join(ROOT, "tests", "c",
                                        "rtcp_seg_fold_check.c")])
    return path


def run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    return r.stdout


def test_rtcp_seg_fold_rule_against_sequential_receiver(exe):
    out = run([exe])
    m = re.search(r"(\d+) batches: (\d+) settled \((\d+) must\), (\d+) "
                  r"declined \((\d+) unsettled\), (\d+) forged packets, "
                  r"(\d+) deciphered behind them, (\d+) wrong", out)
    assert m, out[-4000:]
    total, settled, must, declined, unsettled, forged, flips, wrong = \
        (int(x) for x in m.groups())
    assert total >= 5000
    assert wrong == 0
    # exactly the batches the sequential per-stream masked rx_replay settles
    assert settled == must
    # it settled and it declined, for a copy beyond the look-back too, with
    # forged packets and verdicts they moved: no property held vacuously
    assert settled != 0 and declined != 0 and unsettled != 0
    assert forged != 0 and flips != 0


@pytest.mark.parametrize("seed", [801, 802])
def test_forged_random_traffic_is_settled_by_the_sequential_receiver(
        exe, tmp_path, seed):
    """the generator of tests/test_gpu_srtcp_mfold.py's random batches: the
    sequential receiver answers only 0 / EALREADY / EAUTH, every bucket of
    every batch holds a forged packet, and every batch is one the masked rule
    settles at the kernel's widths (no copy beyond the look-back)"""
    _, batches = F.forged_batches(seed)
    path = str(tmp_path / "traffic.txt")
    F.write_traffic(path, batches)
    rows = re.findall(r"batch (\d+): (\d+) packets ok (\d+) already (\d+) "
                      r"forged (\d+) other (\d+) settle (\w+) must (\d)",
                      run([exe, path]))
    assert len(rows) == len(batches)
    for row, (sent, arrive, ndist, forged) in zip(rows, batches):
        _, n, ok, dup, bad, other = (int(x) for x in row[:6])
        assert n == len(arrive) <= 600 and ndist > 0
        assert other == 0 and ok + dup + bad == n, row
        assert bad == len(forged) and 3 <= bad <= n // 25, row
        buckets = {batches[bb][0][i][0] // F.BUCKET
                   for j, (bb, i) in enumerate(arrive) if j in forged}
        assert buckets == {0, 1, 2}
        assert row[6] == "settled" and row[7] == "1", row
