"""The one statement of how the bucket planners' workspace pool is cut up
(re_amd/csrc/host/bp_layout.h), swept on the CPU under AddressSanitizer +
UBSan by tests/c/bp_layout_check.c: every route's regions over a grid of
batch shapes -- head offsets, alignment, sizes, no overlap, and a total no
larger than what the route reserved before the layout was stated once.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "re_amd", "csrc", "host")


def test_bp_layout_under_sanitizer(tmp_path):
    exe = str(tmp_path / "bp_layout_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=all", "-I" + HOST, "-o", exe,
                           os.path.join(ROOT, "tests", "c",
                                        "bp_layout_check.c")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    assert "2016 layouts, 0 wrong" in r.stdout, r.stdout
