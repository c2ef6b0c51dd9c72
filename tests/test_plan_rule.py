"""The device planners' shared per-packet rules (re_amd/csrc/hip/plan_rule.h)
on the CPU: tests/c/plan_rule_check.c includes the header as C and runs one
stream's batches through the rules and through a sequential receiver, under
AddressSanitizer + UBSan (built and run as tests/test_san_cpu.py does
pool_stress.c: a stand-alone program, nothing preloaded).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_rule_against_sequential_receiver(tmp_path):
    exe = str(tmp_path / "plan_rule_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra",
                           "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "c",
                                        "plan_rule_check.c")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60,
                       env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    assert "0 wrong" in r.stdout
