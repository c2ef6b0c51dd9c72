"""bench.py on the GPU: what a plain run does and what it dumps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from re_amd import workload as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dump(tmp_path):
    """a plain run (no --full) times exactly --steps steps, prints the
    headline fields and none of the --full legs, and --dump-outputs holds
    what the last step returned: every packet window the plaintext again
    (protect + unprotect in place), ends where the input's were, no errors,
    and past each end the 10-byte tag with the ROC over its first four
    bytes"""
    n, steps = 8192, 3
    d = str(tmp_path / "dump")
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                        "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"),
                        "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--packets", str(n), "--dump-outputs", d],
                       capture_output=True, text=True, env=env, timeout=120,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines()
             if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    ln = lines[0]
    assert ln["steps"] == steps and ln["errors"] == 0
    assert ln["unit"] == "GiB/s" and ln["higher_is_better"] is True
    assert ln["dtype"] == "u8" and ln["ms_per_step"] > 0
    # value is the RTP bytes of one step over ms_per_step (which is
    # rounded to a microsecond: 2 % covers steps down to 25 us)
    assert ln["value"] == pytest.approx(
        n * 1200 / (ln["ms_per_step"] * 1e-3) / 2**30, rel=0.02)
    assert "cpu_baseline" not in ln and ln["verified_roundtrip"] is None

    arena, pos, end, cap = W.make_arena(n, 1200, s0=65000 & 0xffff)
    slot = int(cap[0] - pos[0])
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["packet_index"], np.arange(n))
    assert np.array_equal(got["pos"], pos.astype(np.float64))
    assert np.array_equal(got["end"], end.astype(np.float64))
    assert not got["err_protect"].any() and not got["err_unprotect"].any()
    idx = got["slot_index"].astype(np.int64)
    slots = got["arena_slots"]
    assert slots.shape == (len(idx), slot)
    want = arena.reshape(n, slot)[idx]
    assert np.array_equal(slots[:, :1200], want[:, :1200].astype(np.float32))
    tag = slots[:, 1200:1210]
    # unprotect wrote the packet's ROC, big-endian, over the tag's first
    # four bytes (the stream starts at seq 65000 and wraps after 536)
    roc = (65000 + idx) >> 16
    assert roc.min() == 0 and roc.max() == 1
    assert np.array_equal(tag[:, :4], np.stack(
        [(roc >> s) & 0xff for s in (24, 16, 8, 0)], axis=1))
    assert (tag[:, 4:].max(axis=1) > 0).all()
