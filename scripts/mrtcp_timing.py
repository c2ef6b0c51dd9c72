"""SRTCP protect and unprotect of a many-session batch on device windows
(the many-session SRTCP planner plan_buckets_rtcp.hip):
AES_CM_128_HMAC_SHA1_80, 262 144 packets of 28..228 bytes over 65 536
sessions, two thirds of the sessions on one SSRC and one third on two, every
array in HBM.  Times srtcp_encrypt_batch_dev and srtcp_decrypt_batch_dev with
a synchronise, alternating within one run: the planner, and srtp_gpu_tune
nomrplan=1 (the host engine behind dev_staged: what the library did before
the planner).  Each variant has its own senders and receivers, which live
through the run (the first call makes the streams, the later ones find
them); every timed call gets a fresh copy of the plain packets and fresh
windows, and unprotects what its own protect call made.  A library without
the planner (no "nomrplan" knob, no "mrplans" counter) runs the same calls;
both its variants take the host path.  Prints one JSON line.

  python scripts/mrtcp_timing.py [--calls 12] [--warmup 2]
"""
import argparse
import ctypes
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
SLOT = 256
rng = np.random.default_rng(20269)
length = rng.integers(28, 229, n).astype(np.uint32)
sess = rng.integers(0, nsess, n).astype(np.uint32)
# two thirds of the sessions on one SSRC, one third on two
second = (sess % 3 == 2) & (rng.random(n) < 0.5)
ssrc = (0x40000000 + 2 * sess + second).astype(np.uint32)
arena = rng.integers(0, 256, (n, SLOT), dtype=np.uint8)
arena[:, 0], arena[:, 1] = 0x81, 200
words = (length // 4).astype(np.uint32)
arena[:, 2], arena[:, 3] = words >> 8, words & 0xff
arena[:, 4:8] = ssrc.astype(">u4").view(np.uint8).reshape(n, 4)
pos = (np.arange(n, dtype=np.uint64) * SLOT).astype(np.uint32)
end = pos + length
cap = pos + SLOT
keys = W.make_keys(nsess, P.key_len(suite) + P.salt_len(suite)).tobytes()

t32 = lambda a: torch.from_numpy(
    np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()
plain = torch.from_numpy(arena.reshape(-1)).cuda()
del arena
p0, e0, c_d, s_d = t32(pos), t32(end), t32(cap), t32(sess)
COUNTERS = ("mrplans", "rejects", "folds", "misses")


def sessions():
    e, sv = P.alloc_many(nsess, suite, keys)
    assert not e, (e, P.lib().srtp_gpu_error())
    return sv


class Variant:
    def __init__(self, nomrplan):
        self.nomrplan = nomrplan
        self.tx, self.rx = sessions(), sessions()
        # the session arrays once: marshalling 64K pointers is not the call
        self.sv = {id(x): P.session_array(x) for x in (self.tx, self.rx)}
        self.dev = torch.empty_like(plain)
        self.ms = {"protect": [], "unprotect": []}
        self.delta = {}

    def call(self, op, sv, p, e, er):
        # (a library without the knob answers EINVAL: both variants the same)
        P.lib().srtp_gpu_tune(b"nomrplan", 1 if self.nomrplan else 0)
        b = P.SrtpBatchDev()
        b.arena, b.arena_size = self.dev.data_ptr(), self.dev.numel()
        b.pos, b.end, b.cap = p.data_ptr(), e.data_ptr(), c_d.data_ptr()
        b.err, b.sess, b.n, b.stream = er.data_ptr(), s_d.data_ptr(), n, None
        fn, arr = getattr(P.lib(), op + "_batch_dev"), self.sv[id(sv)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = fn(arr, len(arr), ctypes.byref(b))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        P.lib().srtp_gpu_tune(b"nomrplan", 0)
        assert rc == 0, (rc, P.lib().srtp_gpu_error())
        assert not er.any().item(), op
        return dt

    def rep(self, timed, first):
        self.dev.copy_(plain)
        p, e = p0.clone(), e0.clone()
        er = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        before = {c: P.counter(c) for c in COUNTERS}
        a = self.call("srtcp_encrypt", self.tx, p, e, er)
        mid = {c: P.counter(c) for c in COUNTERS}
        assert (e - e0 == 14).all().item()
        er.fill_(-1)
        b = self.call("srtcp_decrypt", self.rx, p, e, er)
        after = {c: P.counter(c) for c in COUNTERS}
        assert (e == e0).all().item()
        v = self.dev.view(n, SLOT)[:, :28]
        assert (v == plain.view(n, SLOT)[:, :28]).all().item()
        if timed:
            self.ms["protect"].append(a)
            self.ms["unprotect"].append(b)
        if first:
            self.delta = {
                "protect": {c: mid[c] - before[c] for c in COUNTERS},
                "unprotect": {c: after[c] - mid[c] for c in COUNTERS}}


variants = {"planner": Variant(False), "nomrplan": Variant(True)}
for r in range(args.warmup + args.calls):
    for v in variants.values():
        v.rep(r >= args.warmup, r == args.warmup)
stat = lambda x: {"median": round(float(np.median(x)), 3),
                  "min": round(min(x), 3), "max": round(max(x), 3)}
out = {
    "shape": "%d SRTCP packets of 28..228 B over %d sessions (2/3 on one "
             "SSRC, 1/3 on two), AES-CM-128 HMAC-SHA1-80, every array in HBM"
             % (n, nsess),
    "packets": n, "sessions": nsess, "calls": args.calls,
    "streams": int(len(np.unique(ssrc))),
    "bytes": int(length.sum()),
    "library": os.environ.get("RE_SRTP_LIB") or "in-tree",
}
for name, v in variants.items():
    for d in ("protect", "unprotect"):
        out["%s_%s_ms" % (d, name)] = stat(v.ms[d])
        out["counters_%s_%s" % (d, name)] = v.delta[d]
for d in ("protect", "unprotect"):
    a, b = out["%s_planner_ms" % d], out["%s_nomrplan_ms" % d]
    out["%s_speedup_vs_nomrplan" % d] = round(b["median"] / a["median"], 2)
    out["%s_slowest_planner_below_fastest_nomrplan" % d] = a["max"] < b["min"]
print(json.dumps(out))
