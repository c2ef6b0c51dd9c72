"""The many-session multi-SSRC RTP planner's rule
(re_amd/csrc/hip/plan_rtp_seg.h) on the CPU: tests/c/rtp_seg_check.c includes
the header as C, runs random interleaved batches of 2-40 sessions with 1-9
SSRCs each through the composition in the decomposition of k_bps_plan
(plan_buckets_rtp_streams.hip) and through a sequential stream_get_seq +
index + replay sender / receiver, under AddressSanitizer + UBSan (a
stand-alone program run as a child process, as tests/test_rtcp_seg_rule.py
does).
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rtp_seg_rule_against_sequential_streams(tmp_path):
    exe = str(tmp_path / "rtp_seg_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "c",
                                        "rtp_seg_check.c")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    m = re.search(r"(\d+) accepted \((\d+) must\), (\d+) rejected, (\d+) wrong",
                  r.stdout)
    assert m, r.stdout[-4000:]
    accepted, _, rejected, wrong = (int(x) for x in m.groups())
    assert wrong == 0
    # it accepted and it rejected: neither property held vacuously
    assert accepted != 0 and rejected != 0
