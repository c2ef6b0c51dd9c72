"""SRTP protect and unprotect of a many-session batch whose sessions carry two
SSRCs each, on device windows (the many-session multi-SSRC RTP
planner plan_buckets_rtp_streams.hip): the config-4 shape,
AES_CM_128_HMAC_SHA1_80, 1 048 576 packets over 65 536 sessions, every
session with an "audio" SSRC of 200-byte packets and a "video" SSRC of
1400-byte packets, interleaved at random and in order per stream, every array
in HBM.  Times srtp_encrypt_batch_dev and srtp_decrypt_batch_dev with a
synchronise, alternating within one run: the planner, and srtp_gpu_tune
nomsplan=1 (the host engine behind dev_staged: what the library did before
the planner).  Each variant has its own senders and receivers, which live
through the run (the first call makes the streams, the later ones find them);
every call's packets continue their streams' sequence numbers from 65400 on
(the ROC rolls over inside batches), every timed call gets a fresh copy of
them and fresh windows, and unprotects what its own protect call made.  A
library without the planner (no "nomsplan" knob, no "msplans" counter) runs
the same calls; both its variants take the host path.  Prints one JSON line.

  python scripts/mrtp_streams_timing.py [--calls 12] [--warmup 2]
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
ap.add_argument("--packets", type=int, default=1 << 20)
ap.add_argument("--sessions", type=int, default=1 << 16)
args = ap.parse_args()

P.load()
n, nsess, suite = args.packets, args.sessions, 1
SLOT, TAG, S0 = 1472, 10, 65400
rng = np.random.default_rng(20270)
sess = rng.integers(0, nsess, n).astype(np.uint32)
video = rng.random(n) < 0.5
length = np.where(video, 1400, 200).astype(np.uint32)
stream = (2 * sess + video).astype(np.int64)
ssrc = (0x40000000 + stream).astype(np.uint32)
# a packet's rank in its stream (array order) and its stream's packets
order = np.argsort(stream, kind="stable")
first = np.r_[0, np.flatnonzero(np.diff(stream[order])) + 1]
count = np.diff(np.r_[first, n])
rank = np.empty(n, dtype=np.int64)
rank[order] = np.arange(n) - np.repeat(first, count)
per = np.empty(n, dtype=np.int64)
per[order] = np.repeat(count, count)
pos = (np.arange(n, dtype=np.uint64) * SLOT).astype(np.uint32)
end = pos + length
cap = pos + SLOT
keys = W.make_keys(nsess, P.key_len(suite) + P.salt_len(suite)).tobytes()

t32 = lambda a: torch.from_numpy(
    np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()
plain = torch.randint(0, 256, (n, SLOT), dtype=torch.uint8, device="cuda")
plain[:, 0], plain[:, 1] = 0x80, 96
plain[:, 8:12] = torch.from_numpy(
    ssrc.astype(">u4").view(np.uint8).reshape(n, 4)).cuda()
rank_d, per_d = torch.from_numpy(rank).cuda(), torch.from_numpy(per).cuda()
p0, e0, c_d, s_d = t32(pos), t32(end), t32(cap), t32(sess)
COUNTERS = ("msplans", "mplans", "rejects", "folds", "misses")


def set_seq(r):
    """call r's sequence numbers: every stream goes on where call r - 1
    left it"""
    seq = (S0 + r * per_d + rank_d) & 0xffff
    plain[:, 2] = (seq >> 8).to(torch.uint8)
    plain[:, 3] = (seq & 0xff).to(torch.uint8)


def sessions():
    e, sv = P.alloc_many(nsess, suite, keys)
    assert not e, (e, P.lib().srtp_gpu_error())
    return sv


class Variant:
    def __init__(self, nomsplan):
        self.nomsplan = nomsplan
        self.tx, self.rx = sessions(), sessions()
        # the session arrays once: marshalling 64K pointers is not the call
        self.sv = {id(x): P.session_array(x) for x in (self.tx, self.rx)}
        self.dev = torch.empty_like(plain)
        self.ms = {"protect": [], "unprotect": []}
        self.delta = {}

    def call(self, op, sv, p, e, er):
        # (a library without the knob answers EINVAL: both variants the same)
        P.lib().srtp_gpu_tune(b"nomsplan", 1 if self.nomsplan else 0)
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
        P.lib().srtp_gpu_tune(b"nomsplan", 0)
        assert rc == 0, (rc, P.lib().srtp_gpu_error())
        assert not er.any().item(), op
        return dt

    def rep(self, timed, first):
        self.dev.copy_(plain)
        p, e = p0.clone(), e0.clone()
        er = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        before = {c: P.counter(c) for c in COUNTERS}
        a = self.call("srtp_encrypt", self.tx, p, e, er)
        mid = {c: P.counter(c) for c in COUNTERS}
        assert (e - e0 == TAG).all().item()
        er.fill_(-1)
        b = self.call("srtp_decrypt", self.rx, p, e, er)
        after = {c: P.counter(c) for c in COUNTERS}
        assert (e == e0).all().item() and (p == p0).all().item()
        assert (self.dev.view(n, SLOT)[:, :200] ==
                plain[:, :200]).all().item()
        if timed:
            self.ms["protect"].append(a)
            self.ms["unprotect"].append(b)
        if first:
            self.delta = {
                "protect": {c: mid[c] - before[c] for c in COUNTERS},
                "unprotect": {c: after[c] - mid[c] for c in COUNTERS}}


variants = {"planner": Variant(False), "nomsplan": Variant(True)}
for r in range(args.warmup + args.calls):
    set_seq(r)
    for v in variants.values():
        v.rep(r >= args.warmup, r == args.warmup)
stat = lambda x: {"median": round(float(np.median(x)), 3),
                  "min": round(min(x), 3), "max": round(max(x), 3)}
out = {
    "shape": "%d RTP packets over %d sessions, two SSRCs per session (200 B "
             "on one, 1400 B on the other), in order per stream, "
             "AES-CM-128 HMAC-SHA1-80, every array in HBM" % (n, nsess),
    "packets": n, "sessions": nsess, "calls": args.calls,
    "streams": int(len(count)),
    "bytes": int(length.sum()),
    "library": os.environ.get("RE_SRTP_LIB") or "in-tree",
}
for name, v in variants.items():
    for d in ("protect", "unprotect"):
        out["%s_%s_ms" % (d, name)] = stat(v.ms[d])
        out["counters_%s_%s" % (d, name)] = v.delta[d]
for d in ("protect", "unprotect"):
    a, b = out["%s_planner_ms" % d], out["%s_nomsplan_ms" % d]
    out["%s_speedup_vs_nomsplan" % d] = round(b["median"] / a["median"], 2)
    out["%s_slowest_planner_below_fastest_nomsplan" % d] = a["max"] < b["min"]
print(json.dumps(out))
