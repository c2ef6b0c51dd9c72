"""SRTP unprotect of a many-session batch whose sessions carry two SSRCs each
and whose streams arrive slightly disturbed, on device windows (DESIGN §5,
the reordered multi-SSRC receive planner plan_buckets_rtp_streams_rx.hip):
AES_CM_128_HMAC_SHA1_80, 1 048 576 packets over 65 536 sessions, every session
with an "audio" SSRC of 200-byte packets and a "video" SSRC of 1400-byte
packets, interleaved at random; per stream 0.1 % adjacent swaps, 0.1 % loss and
0.01 % duplicates (a duplicate arrives behind the stream's next packet); every
array in HBM.  One sender protects each call's packets in order (not timed);
the timed region is srtp_decrypt_batch_dev plus a synchronise, alternating
within one run between

  planner      the disturbed arrivals, the library as it is
  nomsrxplan   the same arrivals under srtp_gpu_tune nomsrxplan=1 (the host
               engine behind dev_staged: what the library did before)
  inorder      the same packets undisturbed (the in-order planner, msplans)

each on receivers of its own, which live through the run; every call's packets
continue their streams' sequence numbers (from 1000 on: no rollover falls into
the run, since a packet late across one is the reference's ETIMEDOUT and no
planner's).  Results are checked: 0 everywhere, EALREADY on the duplicates,
the payloads the sender's.  A library without the planner (no "nomsrxplan"
knob, no "msrxplans" counter) runs the same calls; its first two variants both
take the host path.  Prints one JSON line.

  python scripts/msrx_reorder_timing.py [--calls 12] [--warmup 2]
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
ap.add_argument("--sessions", type=int, default=1 << 16)
args = ap.parse_args()

P.load()
n, nsess, suite = args.packets, args.sessions, 1
SLOT, TAG, S0 = 1472, 10, 1000
rng = np.random.default_rng(20280)
sess = rng.integers(0, nsess, n).astype(np.uint32)
video = rng.random(n) < 0.5
length = np.where(video, 1400, 200).astype(np.uint32)
stream = (2 * sess + video).astype(np.int64)
ssrc = (0x40000000 + stream).astype(np.uint32)
# a packet's rank in its stream (array order), its stream's packets, and the
# stream's next packet (-1: none)
order = np.argsort(stream, kind="stable")
first = np.r_[0, np.flatnonzero(np.diff(stream[order])) + 1]
count = np.diff(np.r_[first, n])
rank = np.empty(n, dtype=np.int64)
rank[order] = np.arange(n) - np.repeat(first, count)
per = np.empty(n, dtype=np.int64)
per[order] = np.repeat(count, count)
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
pos, end, cap = pos_all[:n], pos_all[:n] + length, pos_all[:n] + SLOT
keys = W.make_keys(nsess, P.key_len(suite) + P.salt_len(suite)).tobytes()

t32 = lambda a: torch.from_numpy(
    np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()
plain = torch.randint(0, 256, (n, SLOT), dtype=torch.uint8, device="cuda")
plain[:, 0], plain[:, 1] = 0x80, 96
plain[:, 8:12] = torch.from_numpy(
    ssrc.astype(">u4").view(np.uint8).reshape(n, 4)).cuda()
wire = torch.empty((n + ndup, SLOT), dtype=torch.uint8, device="cuda")
rank_d, per_d = torch.from_numpy(rank).cuda(), torch.from_numpy(per).cuda()
dups_d = torch.from_numpy(np.array(dups, dtype=np.int64)).cuda()
a_src_d = torch.from_numpy(a_src).cuda()
a_ok_d = torch.from_numpy(~a_dup).cuda()
COUNTERS = ("msrxplans", "msplans", "mplans", "mrxplans", "rxlate", "rxdups",
            "rejects", "folds", "misses")
# per variant: pos, end (protected), cap, sess, expected errno
ARR = {
    "disturbed": (t32(pos_all[arrive]),
                  t32(pos_all[arrive] + length[a_src] + TAG),
                  t32(pos_all[arrive] + SLOT), t32(sess[a_src]),
                  torch.from_numpy(np.where(a_dup, errno.EALREADY, 0)
                                   .astype(np.int32)).cuda()),
    "inorder": (t32(pos), t32(end + TAG), t32(cap), t32(sess),
                torch.zeros(n, dtype=torch.int32, device="cuda")),
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


def protect(r):
    """call r's packets, every stream going on where call r - 1 left it,
    protected in order into wire; the duplicates' copies behind them"""
    seq = (S0 + r * per_d + rank_d) & 0xffff
    plain[:, 2] = (seq >> 8).to(torch.uint8)
    plain[:, 3] = (seq & 0xff).to(torch.uint8)
    wire[:n].copy_(plain)
    p, e = p0.clone(), e0.clone()
    er = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    b = batch(wire, p, e, c0, s0, er, n)
    rc = P.lib().srtp_encrypt_batch_dev(tx_arr, len(tx_arr), ctypes.byref(b))
    torch.cuda.synchronize()
    assert rc == 0 and not er.any().item(), (rc, P.lib().srtp_gpu_error())
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
        p1, e1, c1, s1, want = self.arr
        k = p1.numel()
        self.dev.copy_(wire)
        p, e = p1.clone(), e1.clone()
        er = torch.full((k,), -1, dtype=torch.int32, device="cuda")
        b = batch(self.dev, p, e, c1, s1, er, k)
        # (a library without the knob answers EINVAL: the host path anyway)
        if self.knob:
            P.lib().srtp_gpu_tune(b"nomsrxplan", 1)
        before = {c: P.counter(c) for c in COUNTERS}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = P.lib().srtp_decrypt_batch_dev(self.sv, len(self.sv),
                                            ctypes.byref(b))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        after = {c: P.counter(c) for c in COUNTERS}
        P.lib().srtp_gpu_tune(b"nomsrxplan", 0)
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
            "nomsrxplan": Variant("disturbed", True),
            "inorder": Variant("inorder", False)}
for r in range(args.warmup + args.calls):
    protect(r)
    for v in variants.values():
        v.rep(r >= args.warmup, r == args.warmup)
stat = lambda x: {"median": round(float(np.median(x)), 3),
                  "min": round(min(x), 3), "max": round(max(x), 3)}
out = {
    "shape": "%d RTP packets over %d sessions, two SSRCs per session (200 B "
             "on one, 1400 B on the other), per stream 0.1%% adjacent swaps, "
             "0.1%% loss, 0.01%% duplicates, AES-CM-128 HMAC-SHA1-80, every "
             "array in HBM" % (n, nsess),
    "packets": n, "sessions": nsess, "calls": args.calls,
    "streams": int(len(count)), "arrivals": int(m), "swaps": len(swaps),
    "lost": int(len(lost)), "duplicates": ndup,
    "library": os.environ.get("RE_SRTP_LIB") or "in-tree",
}
for name, v in variants.items():
    out["unprotect_%s_ms" % name] = stat(v.ms)
    out["counters_%s" % name] = v.delta
a, b, c = (out["unprotect_%s_ms" % k]
           for k in ("planner", "nomsrxplan", "inorder"))
out["speedup_vs_nomsrxplan"] = round(b["median"] / a["median"], 2)
out["slowest_planner_below_fastest_nomsrxplan"] = a["max"] < b["min"]
out["planner_over_inorder_ms"] = round(a["median"] - c["median"], 3)
print(json.dumps(out))
