"""The RTCP session rule (re_amd/csrc/hip/rtcp_sess_rule.h) on the CPU:
tests/c/rtcp_sess_check.c includes the header as C and runs random decoded
compounds, outgoing packets, reports and statistics queries through it in
the decomposition of rtcp_sess.hip (stable grouping, eight slot owners,
removal as a shuffle, the transmit reduction combined in random association
orders) and through a plain sequential walk, over many rounds on the same
states, under AddressSanitizer + UBSan (a stand-alone program run as a child
process, as tests/test_rtp_rx_rule.py does).
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rtcp_sess_rule_against_sequential_walk(tmp_path):
    exe = str(tmp_path / "rtcp_sess_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "c",
                                        "rtcp_sess_check.c")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    assert " 0 wrong" in r.stdout
    # every outcome occurred: nothing held vacuously
    for what in ("added by rr", "ninth refused", "removed first",
                 "removed middle", "removed last", "readded", "rtt clamped",
                 "rtt positive", "jit wrapped", "truncated", "skipped",
                 "einval", "sr stored", "bye unknown", "accepted",
                 "rejected", "tx resyncs", "sr reports", "rr reports",
                 "stats rows"):
        m = re.search(r"(\d+) %s[,;]" % what, r.stdout)
        assert m and int(m.group(1)) > 0, (what, r.stdout)
