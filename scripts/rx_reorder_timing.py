"""Unprotect of a reordered, lossy, duplicated receive batch (DESIGN §5,
the device receive planner plan_rx.hip): config-2 shape (1M x 1200 B, one
stream) protected in order on the device, then reshaped on the receive side
-- 0.1 % adjacent swaps and 0.1 % loss by permuting / dropping windows,
0.01 % duplicates as byte copies into spare arena slots (no two windows
alias).  Times srtp_decrypt_batch_dev with a synchronise, alternating
within one run: this shape, the in-order shape, and this shape under
srtp_gpu_tune norxplan (the host engine behind the rejected plan: what the
library did before the planner).  Every timed call gets a fresh copy of the
protected arena, fresh windows and a fresh receiver.  Prints one JSON line.

  python scripts/rx_reorder_timing.py [--calls 12] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import re_amd.srtp as P  # noqa: E402
from re_amd import workload as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--packets", type=int, default=1 << 20)
args = ap.parse_args()
assert args.calls >= 10

P.load()
n, suite = args.packets, 1
rng = np.random.default_rng(20260)
arena, pos, end, cap = W.make_arena(n, 1200, s0=65000)
slot = W.slot_size(1200)
assert arena.size == n * slot
key = W.make_keys(1, 30)[0].tobytes()

# duplicates: 0.01 % of the packets, each copied into a spare slot
ndup = max(1, n // 10000)
dup_of = np.sort(rng.choice(n, ndup, replace=False))
dev = torch.zeros((n + ndup) * slot, dtype=torch.uint8, device="cuda")
dev[:n * slot] = torch.from_numpy(arena.reshape(-1)).cuda()
del arena
t32 = lambda a: torch.from_numpy(
    np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()
p_d, e_d, c_d = t32(pos), t32(end), t32(cap)
err = torch.zeros(n, dtype=torch.int32, device="cuda")
tx = P.Srtp(suite, key)
assert P.device_batch_dev("srtp_encrypt", [tx], dev.data_ptr(), n * slot,
                          p_d.data_ptr(), e_d.data_ptr(), c_d.data_ptr(),
                          err.data_ptr(), n) == 0
torch.cuda.synchronize()
assert not err.any().item()
tx.close()
end_tx = e_d.cpu().numpy().view(np.uint32)
v = dev.view(n + ndup, slot)
v[n:] = v[torch.from_numpy(dup_of).cuda()]
pristine = dev.clone()
torch.cuda.synchronize()

# windows of the sent packets and of the copies
pos_all = np.r_[pos, (n + np.arange(ndup, dtype=np.uint64)) * slot
                ].astype(np.uint32)
end_all = np.r_[end_tx, pos_all[n:] + (end_tx[dup_of] - pos[dup_of])
                ].astype(np.uint32)
cap_all = np.r_[cap, pos_all[n:] + (cap[dup_of] - pos[dup_of])
                ].astype(np.uint32)

# arrival order: loss, adjacent swaps, each copy 1..32 arrivals behind its
# original
keep = rng.random(n) >= 0.001
order = np.flatnonzero(keep)
sw = np.flatnonzero(rng.random(len(order) - 1) < 0.001)
sw = sw[np.r_[True, np.diff(sw) > 1]]
order[sw], order[sw + 1] = order[sw + 1].copy(), order[sw].copy()
where = {int(k): i for i, k in enumerate(order)}
ins = sorted((where[int(k)] + int(rng.integers(1, 33)), n + j)
             for j, k in enumerate(dup_of) if int(k) in where)
order = np.insert(order, [min(a, len(order)) for a, _ in ins],
                  [b for _, b in ins])
shapes = {
    "reordered": order,
    "in_order": np.arange(n),
}
win = {k: (t32(pos_all[o]), t32(end_all[o]), t32(cap_all[o]), len(o))
       for k, o in shapes.items()}
COUNTERS = ("rxplans", "rxlate", "rxdups", "rejects", "folds", "fused")


def one(shape, norxplan):
    """one timed call on a fresh arena copy, windows and receiver"""
    p0, e0, c0, m = win[shape]
    dev.copy_(pristine)
    p, e = p0.clone(), e0.clone()
    er = torch.full((m,), -1, dtype=torch.int32, device="cuda")
    rx = P.Srtp(suite, key)
    P.lib().srtp_gpu_tune(b"norxplan", 1 if norxplan else 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = P.device_batch_dev("srtp_decrypt", [rx], dev.data_ptr(),
                            dev.numel(), p.data_ptr(), e.data_ptr(),
                            c0.data_ptr(), er.data_ptr(), m)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    P.lib().srtp_gpu_tune(b"norxplan", 0)
    assert rc == 0, (rc, P.lib().srtp_gpu_error())
    rx.close()
    return dt, er


runs = (("reordered", False), ("in_order", False), ("reordered", True))
ms = {r: [] for r in runs}
errs = {}
deltas = {}
for rep in range(args.warmup + args.calls):
    for r in runs:
        before = {c: P.counter(c) for c in COUNTERS}
        dt, er = one(*r)
        if rep >= args.warmup:
            ms[r].append(dt)
        if rep == args.warmup:
            deltas[r] = {c: P.counter(c) - before[c] for c in COUNTERS}
            errs[r] = er.cpu().numpy()
# both paths gave the same per-packet results
assert (errs[runs[0]] == errs[runs[2]]).all()
assert deltas[runs[0]]["rxplans"] == 1, deltas
stat = lambda x: {"median": round(float(np.median(x)), 3),
                  "min": round(min(x), 3), "max": round(max(x), 3)}
a, b, c = (stat(ms[r]) for r in runs)
nbytes = int((end_all[order] - pos_all[order]).sum())
print(json.dumps({
    "shape": "config 2 (1M x 1200 B, AES-CM-128 HMAC-SHA1-80), 0.1% swaps, "
             "0.1% loss, 0.01% duplicates",
    "packets": int(len(order)), "calls": args.calls,
    "swaps": int(len(sw)), "lost": int(n - keep.sum()),
    "duplicates": int(len(ins)),
    "ealready": int((errs[runs[0]] == 114).sum()),
    "reordered_ms": a, "in_order_ms": b, "reordered_norxplan_ms": c,
    "reordered_GiBps": round(nbytes / 2**30 / (a["median"] * 1e-3), 1),
    "speedup_vs_norxplan": round(c["median"] / a["median"], 2),
    "ratio_to_in_order": round(a["median"] / b["median"], 2),
    "counters_reordered": deltas[runs[0]],
    "counters_in_order": deltas[runs[1]],
    "counters_reordered_norxplan": deltas[runs[2]],
}))
