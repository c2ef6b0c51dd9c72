"""SRTP unprotect of a one-session batch that carries several SSRCs whose
streams arrive slightly disturbed, on device windows (the reordered
one-session multi-SSRC receive planner plan_streams_rx.hip): bench.py's config
2 -- AES_CM_128_HMAC_SHA1_80, 1 048 576 packets of 1200 bytes, one session,
every array in HBM -- with packet i on SSRC i mod K; per stream 0.1 % adjacent
swaps, 0.1 % loss and 0.01 % duplicates (a duplicate arrives behind the
stream's next packet).  One sender protects each call's packets in order (not
timed); the timed region is srtp_decrypt_batch_dev plus a synchronise,
alternating within one run between

  planner      the disturbed arrivals, the library as it is
  nosrxplan    the same arrivals under srtp_gpu_tune nosrxplan=1 (the host
               engine behind dev_staged: what the library did before)
  inorder      the same packets undisturbed (the in-order planner, splans)

each on a receiver of its own, which lives through the run; every call's
packets continue their streams' sequence numbers.  A stream rolls over every
65536 packets, many times per call; no disturbed packet lies within 12
sequence numbers of a rollover, since a packet late across one is the
reference's ETIMEDOUT and no planner's.  Results are checked after every call:
0 everywhere, EALREADY on the duplicates, the payloads the sender's.  A
library without the planner (no "nosrxplan" knob, no "srxplans" counter) runs
the same calls; its first two variants both take the host path.  Prints one
JSON line.

  python scripts/srx_reorder_timing.py --ssrcs 2 [--calls 12] [--warmup 2]
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
ap.add_argument("--packets", type=int, default=1 << 20)
ap.add_argument("--ssrcs", type=int, default=2)
args = ap.parse_args()

P.load()
n, K, suite = args.packets, args.ssrcs, 1
assert 1 <= K <= 8 and n % (K * 65536) == 0, "a whole number of rollovers"
SLOT, LEN, TAG, S0, KEEP_OFF = 1280, 1200, 10, 1000, 12
rng = np.random.default_rng(20290 + K)
idx = np.arange(n, dtype=np.int64)
stream, rank, per = idx % K, idx // K, n // K
ssrc = (0x41000000 + stream).astype(np.uint32)
nxt = np.where(idx + K < n, idx + K, -1)        # the stream's next packet
seq0 = (S0 + rank) % 65536                      # the same in every call
calm = (seq0 >= KEEP_OFF) & (seq0 < 65536 - KEEP_OFF)

# the network: each packet takes part in at most one disturbance
u = rng.random(n)
free = calm.copy()
key = np.arange(n, dtype=np.float64)
swaps = []
for i in np.flatnonzero((u < 0.001) & (nxt >= 0)).tolist():
    j = int(nxt[i])
    if free[i] and free[j]:
        free[i] = free[j] = False
        key[i], key[j] = key[j], key[i]
        swaps.append(i)
lost = np.flatnonzero((u >= 0.001) & (u < 0.002) & free)
free[lost] = False
dups = [i for i in np.flatnonzero((u >= 0.002) & (u < 0.0021)).tolist()
        if free[i] and (nxt[i] < 0 or free[nxt[i]])]
ndup = len(dups)
src = np.r_[np.arange(n), np.array(dups, dtype=np.int64)]
keys_all = np.r_[key, [(key[nxt[i]] if nxt[i] >= 0 else key[i]) + 0.5
                       for i in dups]]
keep = np.ones(n + ndup, dtype=bool)
keep[lost] = False
arrive = np.argsort(keys_all, kind="stable")
arrive = arrive[keep[arrive]]           # slots in arrival order
m = len(arrive)
a_src = src[arrive]                     # the packet each arrival carries
a_dup = arrive >= n

pos_all = (np.arange(n + ndup, dtype=np.uint64) * SLOT).astype(np.uint32)
pos, end, cap = pos_all[:n], pos_all[:n] + LEN, pos_all[:n] + SLOT
key_bytes = W.make_keys(1, P.key_len(suite) + P.salt_len(suite)).tobytes()

t32 = lambda a: torch.from_numpy(
    np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()
plain = torch.randint(0, 256, (n, SLOT), dtype=torch.uint8, device="cuda")
plain[:, 0], plain[:, 1] = 0x80, 96
plain[:, 8:12] = torch.from_numpy(
    ssrc.astype(">u4").view(np.uint8).reshape(n, 4)).cuda()
wire = torch.empty((n + ndup, SLOT), dtype=torch.uint8, device="cuda")
rank_d = torch.from_numpy(rank).cuda()
dups_d = torch.from_numpy(np.array(dups, dtype=np.int64)).cuda()
a_src_d = torch.from_numpy(a_src).cuda()
a_ok_d = torch.from_numpy(~a_dup).cuda()
COUNTERS = ("srxplans", "splans", "rxlate", "rxdups", "rejects", "folds",
            "misses")
# per variant: pos, end (protected), cap, expected errno
ARR = {
    "disturbed": (t32(pos_all[arrive]), t32(pos_all[arrive] + LEN + TAG),
                  t32(pos_all[arrive] + SLOT),
                  torch.from_numpy(np.where(a_dup, errno.EALREADY, 0)
                                   .astype(np.int32)).cuda()),
    "inorder": (t32(pos), t32(end + TAG), t32(cap),
                torch.zeros(n, dtype=torch.int32, device="cuda")),
}


def session():
    s = P.Srtp(suite, key_bytes)
    assert s.err == 0, (s.err, P.lib().srtp_gpu_error())
    return s


def batch(dev, p, e, c, er, k):
    b = P.SrtpBatchDev()
    b.arena, b.arena_size = dev.data_ptr(), dev.numel()
    b.pos, b.end, b.cap = p.data_ptr(), e.data_ptr(), c.data_ptr()
    b.err, b.sess, b.n, b.stream = er.data_ptr(), None, k, None
    return b


tx = session()
tx_arr = P.session_array([tx])
p0, e0, c0 = t32(pos), t32(end), t32(cap)


def protect(r):
    """call r's packets, every stream going on where call r - 1 left it,
    protected in order into wire; the duplicates' copies behind them"""
    seq = (S0 + r * per + rank_d) & 0xffff
    plain[:, 2] = (seq >> 8).to(torch.uint8)
    plain[:, 3] = (seq & 0xff).to(torch.uint8)
    wire[:n].copy_(plain)
    p, e = p0.clone(), e0.clone()
    er = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    b = batch(wire, p, e, c0, er, n)
    rc = P.lib().srtp_encrypt_batch_dev(tx_arr, 1, ctypes.byref(b))
    torch.cuda.synchronize()
    assert rc == 0 and not er.any().item(), (rc, P.lib().srtp_gpu_error())
    if ndup:
        wire[n:] = wire[dups_d]


class Variant:
    def __init__(self, arrays, knob):
        self.arr, self.knob = ARR[arrays], knob
        self.rx = session()
        self.sv = P.session_array([self.rx])
        self.dev = torch.empty_like(wire)
        self.ms, self.delta = [], {}

    def rep(self, timed, first):
        p1, e1, c1, want = self.arr
        k = p1.numel()
        self.dev.copy_(wire)
        p, e = p1.clone(), e1.clone()
        er = torch.full((k,), -1, dtype=torch.int32, device="cuda")
        b = batch(self.dev, p, e, c1, er, k)
        # (a library without the knob answers EINVAL: the host path anyway)
        if self.knob:
            P.lib().srtp_gpu_tune(b"nosrxplan", 1)
        before = {c: P.counter(c) for c in COUNTERS}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = P.lib().srtp_decrypt_batch_dev(self.sv, 1, ctypes.byref(b))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        after = {c: P.counter(c) for c in COUNTERS}
        P.lib().srtp_gpu_tune(b"nosrxplan", 0)
        assert rc == 0, (rc, P.lib().srtp_gpu_error())
        assert (er == want).all().item(), "errno"
        assert (e == e1 - TAG).all().item(), "end"
        if k == n:
            got = self.dev[:n, 12:200]
            assert (got == plain[:, 12:200]).all().item(), "payload"
        else:
            got = self.dev.view(-1, SLOT)[(p1.long() // SLOT)[a_ok_d], 12:200]
            assert (got == plain[a_src_d[a_ok_d], 12:200]).all().item(), \
                "payload"
        if timed:
            self.ms.append(dt)
        if first:
            self.delta = {c: after[c] - before[c] for c in COUNTERS}


variants = {"planner": Variant("disturbed", False),
            "nosrxplan": Variant("disturbed", True),
            "inorder": Variant("inorder", False)}
for r in range(args.warmup + args.calls):
    protect(r)
    for v in variants.values():
        v.rep(r >= args.warmup, r == args.warmup)
stat = lambda x: {"median": round(float(np.median(x)), 3),
                  "min": round(min(x), 3), "max": round(max(x), 3)}
out = {
    "shape": "%d RTP packets of %d B on one session, packet i on SSRC i mod "
             "%d, per stream 0.1%% adjacent swaps, 0.1%% loss, 0.01%% "
             "duplicates, AES-CM-128 HMAC-SHA1-80, every array in HBM"
             % (n, LEN, K),
    "packets": n, "ssrcs": K, "calls": args.calls, "arrivals": int(m),
    "swaps": len(swaps), "lost": int(len(lost)), "duplicates": ndup,
    "library": os.environ.get("RE_SRTP_LIB") or "in-tree",
}
for name, v in variants.items():
    out["unprotect_%s_ms" % name] = stat(v.ms)
    out["counters_%s" % name] = v.delta
a, b, c = (out["unprotect_%s_ms" % k]
           for k in ("planner", "nosrxplan", "inorder"))
out["speedup_vs_nosrxplan"] = round(b["median"] / a["median"], 2)
out["slowest_planner_below_fastest_nosrxplan"] = a["max"] < b["min"]
out["planner_over_inorder_ms"] = round(a["median"] - c["median"], 3)
print(json.dumps(out))
