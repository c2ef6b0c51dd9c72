"""SRTCP unprotect of a many-session batch some of whose packets are forged, on
device windows (the settlement pass plan_buckets_rtcp_fold.hip
behind the many-session SRTCP planners; srtp_gpu_tune mrfold): the shape of
scripts/mrtcp_timing.py -- AES_CM_128_HMAC_SHA1_80, 262 144 packets of 28..228
bytes over 65 536 sessions, two thirds of the sessions on one SSRC and one
third on two, every array in HBM.  One sender protects each call's packets in
order (not timed); a forged packet is its wire packet with a tag bit flipped.
The timed region is srtcp_decrypt_batch_dev plus a synchronise, alternating
within one run between

  clean          the packets in order, none forged (the in-order planner)
  one            in order, one forged packet per call
  some           in order, 0.1 % forged
  disturbed      the arrivals of scripts/mrtcp_rx_reorder_timing.py (per stream
                 0.1 % adjacent swaps, 0.01 % duplicates), 0.1 % forged (never
                 a duplicate or its original, so no other verdict moves)

the three forged shapes each under srtp_gpu_tune mrfold=1 (settled on the
device) and mrfold=0 (undone, folded by the host engine), every variant on
receivers of its own, which live through the run; every call's packets
continue their streams' indices.  After every call: errno (EAUTH on the forged
packets, EALREADY on the duplicates, 0 elsewhere), the ends, the payloads of
the accepted packets, and the counters ("mrfolds" +1, "folds" +0 and "misses"
the forged count under mrfold=1; "folds" +1 and "mrfolds" +0 under mrfold=0).
A library without the knob runs the same calls; all its forged variants take
the host engine.  Prints one JSON line.

  python scripts/mrtcp_forged_timing.py [--calls 8] [--warmup 2]
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
ap.add_argument("--calls", type=int, default=8)
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

# the forged packets, the same in every call
frng = np.random.default_rng(20315)
f_one = np.zeros(n, dtype=bool)
f_one[n // 2] = True
f_some = frng.random(n) < 0.001
copied = np.zeros(n, dtype=bool)
copied[dups] = True
f_dist = (frng.random(m) < 0.001) & ~a_dup & ~copied[a_src]

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
COUNTERS = ("mrfolds", "folds", "misses", "mrplans", "mrrxplans", "rejects",
            "rxdups")
HAS_KNOB = P.lib().srtp_gpu_tune(b"mrfold", 0) == 0


def arrays(p, e_prot, c, s, carried, dup, forged):
    """a variant's windows and what to expect of them: pos, end (protected),
    cap, sess, errno, end after, the last tag byte of the forged packets, the
    accepted arrivals and the packets they carry"""
    want = np.where(forged, P.EAUTH, np.where(dup, errno.EALREADY, 0))
    wend = e_prot - np.where(forged | dup, TAG, GROW).astype(np.uint32)
    ok = ~(forged | dup)
    return (t32(p), t32(e_prot), t32(c), t32(s),
            torch.from_numpy(want.astype(np.int32)).cuda(), t32(wend),
            torch.from_numpy((e_prot[forged] - 1).astype(np.int64)).cuda(),
            torch.from_numpy((p[ok] // SLOT).astype(np.int64)).cuda(),
            torch.from_numpy(carried[ok].astype(np.int64)).cuda(),
            int(forged.sum()))


no = np.zeros(n, dtype=bool)
ident = np.arange(n)
ARR = {
    "clean": arrays(pos, end + GROW, cap, sess, ident, no, no),
    "one": arrays(pos, end + GROW, cap, sess, ident, no, f_one),
    "some": arrays(pos, end + GROW, cap, sess, ident, no, f_some),
    "disturbed": arrays(pos_all[arrive], pos_all[arrive] + length[a_src] + GROW,
                        pos_all[arrive] + SLOT, sess[a_src], a_src, a_dup,
                        f_dist),
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
    def __init__(self, shape, mrfold):
        self.shape, self.mrfold = shape, mrfold
        self.arr = ARR[shape]
        self.rx = sessions()
        self.sv = P.session_array(self.rx)
        self.dev = torch.empty_like(wire)
        self.ms, self.delta = [], {}

    def rep(self, timed, first):
        p1, e1, c1, s1, want, wend, fbyte, okslot, okpkt, nforged = self.arr
        k = p1.numel()
        self.dev.copy_(wire)
        if nforged:
            self.dev.view(-1)[fbyte] ^= 0x40
        p, e = p1.clone(), e1.clone()
        er = torch.full((k,), -1, dtype=torch.int32, device="cuda")
        b = batch(self.dev, p, e, c1, s1, er, k)
        # (a library without the knob answers EINVAL: the host engine anyway)
        P.lib().srtp_gpu_tune(b"mrfold", self.mrfold)
        before = {c: P.counter(c) for c in COUNTERS}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = P.lib().srtcp_decrypt_batch_dev(self.sv, len(self.sv),
                                             ctypes.byref(b))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        after = {c: P.counter(c) for c in COUNTERS}
        P.lib().srtp_gpu_tune(b"mrfold", 0)
        d = {c: after[c] - before[c] for c in COUNTERS}
        assert rc == 0, (rc, P.lib().srtp_gpu_error())
        assert (er == want).all().item(), (self.shape, "errno")
        assert (e == wend).all().item(), (self.shape, "end")
        assert (p == p1).all().item(), (self.shape, "pos")
        got = self.dev.view(-1, SLOT)[okslot, :28]
        assert (got == plain[okpkt, :28]).all().item(), (self.shape, "payload")
        settled = 1 if nforged and self.mrfold and HAS_KNOB else 0
        assert d["mrfolds"] == settled, (self.shape, self.mrfold, d)
        assert not settled or d["misses"] == nforged, (self.shape, d)
        assert d["folds"] == (1 if nforged and not settled else 0), \
            (self.shape, self.mrfold, d)
        if timed:
            self.ms.append(dt)
        if first:
            self.delta = d


variants = {"clean": Variant("clean", 0)}
for shape in ("one", "some", "disturbed"):
    for knob in (1, 0):
        variants["%s_mrfold%d" % (shape, knob)] = Variant(shape, knob)
for r in range(args.warmup + args.calls):
    protect()
    for v in variants.values():
        v.rep(r >= args.warmup, r == args.warmup)
stat = lambda x: {"median": round(float(np.median(x)), 3),
                  "min": round(min(x), 3), "max": round(max(x), 3)}
out = {
    "shape": "%d SRTCP packets of 28..228 B over %d sessions (2/3 on one "
             "SSRC, 1/3 on two), AES-CM-128 HMAC-SHA1-80, every array in HBM; "
             "disturbed: per stream 0.1%% adjacent swaps and 0.01%% duplicates"
             % (n, nsess),
    "packets": n, "sessions": nsess, "calls": args.calls,
    "arrivals_disturbed": int(m), "swaps": len(swaps), "duplicates": ndup,
    "forged": {k: ARR[k][9] for k in ("one", "some", "disturbed")},
    "knob": bool(HAS_KNOB),
    "library": os.environ.get("RE_SRTP_LIB") or "in-tree",
}
for name, v in variants.items():
    out["unprotect_%s_ms" % name] = stat(v.ms)
    out["counters_%s" % name] = v.delta
clean = out["unprotect_clean_ms"]["median"]
for shape in ("one", "some", "disturbed"):
    a = out["unprotect_%s_mrfold1_ms" % shape]
    b = out["unprotect_%s_mrfold0_ms" % shape]
    out["%s_slowest_mrfold1_below_fastest_mrfold0" % shape] = \
        a["max"] < b["min"]
    out["%s_speedup" % shape] = round(b["median"] / a["median"], 2)
    out["%s_mrfold1_over_clean_ms" % shape] = round(a["median"] - clean, 3)
print(json.dumps(out))
