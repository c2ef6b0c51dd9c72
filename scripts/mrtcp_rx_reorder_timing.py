"""SRTCP unprotect of a many-session batch whose streams arrive slightly
disturbed, on device windows (the many-session SRTCP receive
planner plan_buckets_rtcp_rx.hip): the shape of scripts/mrtcp_timing.py --
AES_CM_128_HMAC_SHA1_80, 262 144 packets of 28..228 bytes over 65 536
sessions, two thirds of the sessions on one SSRC and one third on two, every
array in HBM -- with per stream 0.1 % adjacent swaps and 0.01 % duplicates (a
duplicate arrives behind the stream's next packet; no loss: a missing SRTCP
index disturbs nothing).  One sender protects each call's packets in order
(not timed); the timed region is srtcp_decrypt_batch_dev plus a synchronise,
alternating within one run between

  planner      the disturbed arrivals, the library as it is
  nomrrxplan   the same arrivals under srtp_gpu_tune nomrrxplan=1 (the host
               engine behind dev_staged: what the library did before)
  inorder      the same packets undisturbed (the in-order planner, mrplans)

each on receivers of its own, which live through the run; every call's packets
continue their streams' indices.  Results are checked after every call: 0
everywhere and EALREADY on the duplicates, the ends (a duplicate keeps its
E || index word), the payloads the sender's.  A library without the planner
(no "nomrrxplan" knob, no "mrrxplans" counter) runs the same calls; its first
two variants both take the host path.  Prints one JSON line.

  python scripts/mrtcp_rx_reorder_timing.py [--calls 12] [--warmup 2]
"""
import argparse
import ctypes
import errno
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
ap.add_argument("--packets", type=int, default=1 << 18)
ap.add_argument("--sessions", type=int, default=1 << 16)
args = ap.parse_args()

P.load()
n, nsess, suite = args.packets, args.sessions, 1
SLOT, TAG, GROW = 256, 10, 14
rng = np.random.default_rng(20291)
length = rng.integers(28, 229, n).astype(np.uint32)
sess = rng.integers(0, nsess, n).astype(np.uint32)
# two thirds of the sessions on one SSRC, one third on two
second = (sess % 3 == 2) & (rng.random(n) < 0.5)
stream = (2 * sess.astype(np.int64) + second)
ssrc = (0x40000000 + stream).astype(np.uint32)
# the stream's next packet in array order (-1: none)
order = np.argsort(stream, kind="stable")
nxt = np.full(n, -1, dtype=np.int64)
same = stream[order][1:] == stream[order][:-1]
nxt[order[:-1][same]] = order[1:][same]

# the network: each packet takes part in at most one disturbance
u = rng.random(n)
free = np.ones(n, dtype=bool)
key = np.arange(n, dtype=np.float64)
swaps = []
for i in np.flatnonzero((u < 0.001) & (nxt >= 0)).tolist():
    j = int(nxt[i])
    if free[i] and free[j]:
        free[i] = free[j] = False
        key[i], key[j] = key[j], key[i]
        swaps.append(i)
dups = [i for i in np.flatnonzero((u >= 0.001) & (u < 0.0011)).tolist()
        if free[i] and (nxt[i] < 0 or free[nxt[i]])]
ndup = len(dups)
src = np.r_[np.arange(n), np.array(dups, dtype=np.int64)]
keys_all = np.r_[key, [(key[nxt[i]] if nxt[i] >= 0 else key[i]) + 0.5
                       for i in dups]]
arrive = np.argsort(keys_all, kind="stable")    # slots in arrival order
m = len(arrive)
a_src = src[arrive]                             # the packet each arrival carries
a_dup = arrive >= n

pos_all = (np.arange(n + ndup, dtype=np.uint64) * SLOT).astype(np.uint32)
pos, end, cap = pos_all[:n], pos_all[:n] + length, pos_all[:n] + SLOT
keys = W.make_keys(nsess, P.key_len(suite) + P.salt_len(suite)).tobytes()

t32 = lambda a: torch.from_numpy(
    np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()
arena = rng.integers(0, 256, (n, SLOT), dtype=np.uint8)
arena[:, 0], arena[:, 1] = 0x81, 200
words = (length // 4).astype(np.uint32)
arena[:, 2], arena[:, 3] = words >> 8, words & 0xff
arena[:, 4:8] = ssrc.astype(">u4").view(np.uint8).reshape(n, 4)
plain = torch.from_numpy(arena).cuda()
del arena
wire = torch.empty((n + ndup, SLOT), dtype=torch.uint8, device="cuda")
dups_d = torch.from_numpy(np.array(dups, dtype=np.int64)).cuda()
a_src_d = torch.from_numpy(a_src).cuda()
a_ok_d = torch.from_numpy(~a_dup).cuda()
COUNTERS = ("mrrxplans", "mrplans", "rxlate", "rxdups", "rejects", "folds",
            "misses")
# per variant: pos, end (protected), cap, sess, expected errno, expected end
a_end = pos_all[arrive] + length[a_src] + GROW
ARR = {
    "disturbed": (t32(pos_all[arrive]), t32(a_end),
                  t32(pos_all[arrive] + SLOT), t32(sess[a_src]),
                  torch.from_numpy(np.where(a_dup, errno.EALREADY, 0)
                                   .astype(np.int32)).cuda(),
                  t32(a_end - np.where(a_dup, TAG, GROW).astype(np.uint32))),
    "inorder": (t32(pos), t32(end + GROW), t32(cap), t32(sess),
                torch.zeros(n, dtype=torch.int32, device="cuda"), t32(end)),
}


def sessions():
    e, sv = P.alloc_many(nsess, suite, keys)
    assert not e, (e, P.lib().srtp_gpu_error())
    return sv


def batch(dev, p, e, c, s, er, k):
    b = P.SrtpBatchDev()
    b.arena, b.arena_size = dev.data_ptr(), dev.numel()
    b.pos, b.end, b.cap = p.data_ptr(), e.data_ptr(), c.data_ptr()
    b.err, b.sess, b.n, b.stream = er.data_ptr(), s.data_ptr(), k, None
    return b


tx = sessions()
tx_arr = P.session_array(tx)
p0, e0, c0, s0 = t32(pos), t32(end), t32(cap), t32(sess)


def protect():
    """the call's packets, every stream going on where the call before left
    it, protected in order into wire; the duplicates' copies behind them"""
    wire[:n].copy_(plain)
    p, e = p0.clone(), e0.clone()
    er = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    b = batch(wire, p, e, c0, s0, er, n)
    rc = P.lib().srtcp_encrypt_batch_dev(tx_arr, len(tx_arr), ctypes.byref(b))
    torch.cuda.synchronize()
    assert rc == 0 and not er.any().item(), (rc, P.lib().srtp_gpu_error())
    assert (e - e0 == GROW).all().item()
    if ndup:
        wire[n:] = wire[dups_d]


class Variant:
    def __init__(self, arrays, knob):
        self.arr, self.knob = ARR[arrays], knob
        self.rx = sessions()
        self.sv = P.session_array(self.rx)
        self.dev = torch.empty_like(wire)
        self.ms, self.delta = [], {}

    def rep(self, timed, first):
        p1, e1, c1, s1, want, wend = self.arr
        k = p1.numel()
        self.dev.copy_(wire)
        p, e = p1.clone(), e1.clone()
        er = torch.full((k,), -1, dtype=torch.int32, device="cuda")
        b = batch(self.dev, p, e, c1, s1, er, k)
        # (a library without the knob answers EINVAL: the host path anyway)
        if self.knob:
            P.lib().srtp_gpu_tune(b"nomrrxplan", 1)
        before = {c: P.counter(c) for c in COUNTERS}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = P.lib().srtcp_decrypt_batch_dev(self.sv, len(self.sv),
                                             ctypes.byref(b))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        after = {c: P.counter(c) for c in COUNTERS}
        P.lib().srtp_gpu_tune(b"nomrrxplan", 0)
        assert rc == 0, (rc, P.lib().srtp_gpu_error())
        assert (er == want).all().item(), "errno"
        assert (e == wend).all().item(), "end"
        if k == n:
            got = self.dev[:n, :28]
            assert (got == plain[:, :28]).all().item(), "payload"
        else:
            got = self.dev.view(-1, SLOT)[(p1.long() // SLOT)[a_ok_d], :28]
            assert (got == plain[a_src_d[a_ok_d], :28]).all().item(), \
                "payload"
        if timed:
            self.ms.append(dt)
        if first:
            self.delta = {c: after[c] - before[c] for c in COUNTERS}


variants = {"planner": Variant("disturbed", False),
            "nomrrxplan": Variant("disturbed", True),
            "inorder": Variant("inorder", False)}
for r in range(args.warmup + args.calls):
    protect()
    for v in variants.values():
        v.rep(r >= args.warmup, r == args.warmup)
stat = lambda x: {"median": round(float(np.median(x)), 3),
                  "min": round(min(x), 3), "max": round(max(x), 3)}
out = {
    "shape": "%d SRTCP packets of 28..228 B over %d sessions (2/3 on one "
             "SSRC, 1/3 on two), per stream 0.1%% adjacent swaps and 0.01%% "
             "duplicates, AES-CM-128 HMAC-SHA1-80, every array in HBM"
             % (n, nsess),
    "packets": n, "sessions": nsess, "calls": args.calls,
    "streams": int(len(np.unique(stream))), "arrivals": int(m),
    "swaps": len(swaps), "duplicates": ndup,
    "library": os.environ.get("RE_SRTP_LIB") or "in-tree",
}
for name, v in variants.items():
    out["unprotect_%s_ms" % name] = stat(v.ms)
    out["counters_%s" % name] = v.delta
a, b, c = (out["unprotect_%s_ms" % k]
           for k in ("planner", "nomrrxplan", "inorder"))
out["speedup_vs_nomrrxplan"] = round(b["median"] / a["median"], 2)
out["slowest_planner_below_fastest_nomrrxplan"] = a["max"] < b["min"]
out["planner_over_inorder_ms"] = round(a["median"] - c["median"], 3)
print(json.dumps(out))
