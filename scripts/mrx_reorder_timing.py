"""Unprotect of a many-session receive batch whose sessions see reordered,
lost and duplicated packets (the bucket receive planner
plan_buckets_rx.hip): config-4 shape (1M packets of 200 / 1400 B over 64K
sessions, every array in HBM) protected in order on the device, then
reshaped on the receive side per session -- 0.1 % of the packets swapped
with their session's next arrival and 0.1 % lost by permuting / dropping
windows, 0.01 % duplicated as byte copies into spare arena slots (no two
windows alias).  Times srtp_decrypt_batch_dev with a synchronise,
alternating within one run: this shape, the in-order shape, and this shape
under srtp_gpu_tune norxplan (the host engine behind the rejected plan:
what the library did before the planner).  Every timed call gets a fresh
copy of the protected arena, fresh windows and fresh receivers.  A library
without the planner (no "mrxplans" counter) runs the same calls; its
reshaped batch takes the host path either way.  Prints one JSON line.

  python scripts/mrx_reorder_timing.py [--calls 12] [--warmup 2]
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
ap.add_argument("--sessions", type=int, default=1 << 16)
args = ap.parse_args()
assert args.calls >= 10

P.load()
n, nsess, suite = args.packets, args.sessions, 1
rng = np.random.default_rng(20268)
lengths = W.mixed_lengths(n)
sess = W.random_sessions(n, nsess)
arena, pos, end, cap = W.make_arena(n, lengths, s0=65000, sess=sess)
slot = arena.size // n
assert arena.size == n * slot
keys = W.make_keys(nsess, P.key_len(suite) + P.salt_len(suite)).tobytes()

# duplicates: 0.01 % of the packets, each copied into a spare slot
ndup = max(1, n // 10000)
dup_of = np.sort(rng.choice(n, ndup, replace=False))
dev = torch.zeros((n + ndup) * slot, dtype=torch.uint8, device="cuda")
dev[:n * slot] = torch.from_numpy(arena.reshape(-1)).cuda()
del arena
t32 = lambda a: torch.from_numpy(
    np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()
p_d, e_d, c_d, s_d = t32(pos), t32(end), t32(cap), t32(sess)
err = torch.zeros(n, dtype=torch.int32, device="cuda")


def sessions():
    e, sv = P.alloc_many(nsess, suite, keys)
    assert not e, (e, P.lib().srtp_gpu_error())
    return sv


tx = sessions()
assert P.device_batch_dev("srtp_encrypt", tx, dev.data_ptr(), n * slot,
                          p_d.data_ptr(), e_d.data_ptr(), c_d.data_ptr(),
                          err.data_ptr(), n, s_d.data_ptr()) == 0
torch.cuda.synchronize()
assert not err.any().item()
for s in tx:
    s.close()
end_tx = e_d.cpu().numpy().view(np.uint32)
v = dev.view(n + ndup, slot)
v[n:] = v[torch.from_numpy(dup_of).cuda()]
pristine = dev.clone()
torch.cuda.synchronize()

# windows (and sessions) of the sent packets and of the copies
pos_all = np.r_[pos, (n + np.arange(ndup, dtype=np.uint64)) * slot
                ].astype(np.uint32)
end_all = np.r_[end_tx, pos_all[n:] + (end_tx[dup_of] - pos[dup_of])
                ].astype(np.uint32)
cap_all = np.r_[cap, pos_all[n:] + (cap[dup_of] - pos[dup_of])
                ].astype(np.uint32)
sess_all = np.r_[sess, sess[dup_of]].astype(np.uint32)

# arrival order: loss; a swapped packet trades places with its session's
# next arrival; each copy 1..32 arrivals of the batch behind its original
keep = rng.random(n) >= 0.001
order = np.flatnonzero(keep)
by_sess = np.argsort(sess[order], kind="stable")
has_next = np.r_[sess[order][by_sess][1:] == sess[order][by_sess][:-1], False]
sw = np.flatnonzero((rng.random(len(order)) < 0.001) & has_next)
sw = sw[np.r_[True, np.diff(sw) > 1]]           # no chains
a, b = by_sess[sw], by_sess[sw + 1]
order[a], order[b] = order[b].copy(), order[a].copy()
where = {int(k): i for i, k in enumerate(order)}
ins = sorted((where[int(k)] + int(rng.integers(1, 33)), n + j)
             for j, k in enumerate(dup_of) if int(k) in where)
order = np.insert(order, [min(x, len(order)) for x, _ in ins],
                  [y for _, y in ins])
shapes = {
    "reordered": order,
    "in_order": np.arange(n),
}
win = {k: (t32(pos_all[o]), t32(end_all[o]), t32(cap_all[o]),
           t32(sess_all[o]), len(o)) for k, o in shapes.items()}
COUNTERS = ("mrxplans", "mplans", "rxlate", "rxdups", "rejects", "folds")


def one(shape, norxplan):
    """one timed call on a fresh arena copy, windows and receivers"""
    p0, e0, c0, s0, m = win[shape]
    dev.copy_(pristine)
    p, e = p0.clone(), e0.clone()
    er = torch.full((m,), -1, dtype=torch.int32, device="cuda")
    rx = sessions()
    P.lib().srtp_gpu_tune(b"norxplan", 1 if norxplan else 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = P.device_batch_dev("srtp_decrypt", rx, dev.data_ptr(),
                            dev.numel(), p.data_ptr(), e.data_ptr(),
                            c0.data_ptr(), er.data_ptr(), m, s0.data_ptr())
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    P.lib().srtp_gpu_tune(b"norxplan", 0)
    assert rc == 0, (rc, P.lib().srtp_gpu_error())
    for s in rx:
        s.close()
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
assert set(np.unique(errs[runs[0]]).tolist()) <= {0, 114}
assert not errs[runs[1]].any()
stat = lambda x: {"median": round(float(np.median(x)), 3),
                  "min": round(min(x), 3), "max": round(max(x), 3)}
a, b, c = (stat(ms[r]) for r in runs)
nbytes = int((end_all[order].astype(np.int64) - pos_all[order]).sum())
print(json.dumps({
    "shape": "config 4 (%d x 200/1400 B over %d sessions, AES-CM-128 "
             "HMAC-SHA1-80), per session 0.1%% swaps, 0.1%% loss, 0.01%% "
             "duplicates" % (n, nsess),
    "packets": int(len(order)), "sessions": nsess, "calls": args.calls,
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
