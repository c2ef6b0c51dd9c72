"""The many-session SRTCP planner's rule (re_amd/csrc/hip/plan_rtcp_seg.h) on
the CPU: tests/c/rtcp_seg_check.c includes the header as C, runs random
interleaved batches through the composition in the decomposition of
k_bpr_plan (plan_buckets_rtcp.hip) and through a sequential stream_get +
SRTCP index / replay restatement, under AddressSanitizer + UBSan (a
stand-alone program run as a child process, as tests/test_plan_rule.py does).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rtcp_seg_rule_against_sequential_streams(tmp_path):
    exe = str(tmp_path / "rtcp_seg_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "c",
                                        "rtcp_seg_check.c")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    assert " 0 wrong" in r.stdout
    # it accepted and it rejected: neither property held vacuously
    assert " 0 accepted" not in r.stdout and " 0 rejected" not in r.stdout
