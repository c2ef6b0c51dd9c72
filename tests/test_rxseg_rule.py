"""The receive rule for many streams in one scan (re_amd/csrc/hip/
plan_rx_rule.h: struct rx_seg, rx_seg_combine) on the CPU: tests/c/
rx_seg_check.c includes the header as C and runs interleaved many-session
batches in the decomposition of k_bp_rx_plan (plan_buckets_rx.hip), against
every session alone through the one-stream composition and against a
sequential receiver, under AddressSanitizer + UBSan (a stand-alone program
with the sanitizers' runtimes linked in, nothing preloaded; built as
tests/test_plan_rule.py builds plan_rule_check.c).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmented_rule_against_one_stream_and_sequential_receiver(tmp_path):
    exe = str(tmp_path / "rx_seg_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra",
                           "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "c",
                                        "rx_seg_check.c")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    assert " 0 wrong" in r.stdout, r.stdout[-2000:]
