"""bench.py's output dump and option set, without a GPU."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_files(tmp_path):
    """dump_outputs: float32 / float64 .npy files, the arena as a seeded
    sample of whole slots (the same slots on every call), the per-packet
    arrays whole, device-style int32 views of uint32 windows read back as
    unsigned, host arrays and tensors alike; under 64 MB at the largest
    slot and the full packet count"""
    import torch
    import bench
    n, slot = 6000, 1216
    arena = (torch.arange(n * slot, dtype=torch.int64) % 251).to(torch.uint8)
    pos_h = np.arange(n, dtype=np.uint32) * slot + np.uint32(3 << 30)
    end_h = pos_h + np.uint32(1200)
    err = np.zeros(n, dtype=np.int32)
    err[17] = 74
    as_dev = lambda a: torch.from_numpy(a.view(np.int32))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, "", arena, slot, (as_dev(pos_h), as_dev(end_h),
                                            torch.from_numpy(err),
                                            torch.from_numpy(err)))
    bench.dump_outputs(b, "", arena, slot, (pos_h, end_h, err, err))
    names = sorted(os.listdir(a))
    assert names == sorted(x + ".npy" for x in (
        "arena_slots", "slot_index", "packet_index", "pos", "end",
        "err_protect", "err_unprotect"))
    got = {f[:-4]: np.load(os.path.join(a, f)) for f in names}
    for f in names:
        assert np.array_equal(got[f[:-4]], np.load(os.path.join(b, f))), f
        assert got[f[:-4]].dtype in (np.float32, np.float64), f
    idx = got["slot_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SLOTS and (np.diff(idx) > 0).all()
    assert got["arena_slots"].shape == (bench.DUMP_SLOTS, slot)
    assert np.array_equal(got["arena_slots"],
                          arena.numpy().reshape(n, slot)[idx])
    assert np.array_equal(got["packet_index"], np.arange(n))
    assert np.array_equal(got["pos"], pos_h.astype(np.float64))
    assert np.array_equal(got["end"], end_h.astype(np.float64))
    assert got["err_protect"][17] == 74 and got["err_protect"].sum() == 74
    worst = bench.DUMP_SLOTS * 1416 * 4 + bench.DUMP_SLOTS * 8 + \
        bench.DUMP_PACKETS * (8 + 8 + 8 + 4 + 4)
    assert worst <= 64 * 2**20


def test_bench_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"),
                          "--help"], capture_output=True, text=True,
                         check=True).stdout
    for opt in ("--full", "--dump-outputs DIR", "--steps", "--warmup",
                "--gpus"):
        assert opt in out, opt
