"""The receiver-statistics rule (re_amd/csrc/hip/rtp_rx_rule.h) on the CPU:
tests/c/rtp_rx_check.c includes the header as C and runs random traffic with
arbitrary 32-bit timestamps and arrival times through it in the decomposition
of rtp_stats.hip (records, stable grouping, eight slot owners per session)
and through a plain sequential walk, SR events and report blocks included,
under AddressSanitizer + UBSan (a stand-alone program run as a child
process, as tests/test_rtcp_seg_rule.py does).
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rtp_rx_rule_against_sequential_walk(tmp_path):
    exe = str(tmp_path / "rtp_rx_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "c",
                                        "rtp_rx_check.c")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    assert " 0 wrong" in r.stdout
    # every outcome occurred: nothing held vacuously
    for what in ("ok", "badseq", "nomember", "skipped", "badmsg", "einval"):
        m = re.search(r"(\d+) %s[,;]" % what, r.stdout)
        assert m and int(m.group(1)) > 0, (what, r.stdout)
    for what in ("resyncs", "cycled", "report blocks"):
        m = re.search(r"(\d+) %s[,;]" % what, r.stdout)
        assert m and int(m.group(1)) > 0, (what, r.stdout)
