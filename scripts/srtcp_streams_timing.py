"""SRTCP protect and unprotect of ONE session whose SRTCP carries several
SSRCs, or whose packets arrive slightly disturbed, on device windows (DESIGN
§5, the one-session SRTCP planner plan_streams_rtcp.hip): 1M packets of 1200
bytes, AES_CM_128_HMAC_SHA1_80, the SSRCs interleaved round robin.  Shapes:

  k2 / k8      2 and 8 SSRCs: protect; unprotect in order; unprotect with per
               stream 0.1 % swaps (with the stream's next packet), 0.1 % loss
               and 0.01 % duplicates (behind the stream's next packet)
  k1           1 SSRC, the same disturbance (unprotect only)

each timed as srtcp_*_batch_dev plus a synchronise, alternating within one run
between

  planner      the library as it is
  nosrplan     the same call under srtp_gpu_tune nosrplan=1 (the host engine
               behind dev_staged: what the library did before)

and, as the floor, the one-stream in-order unprotect of as many packets (the
one-launch plan, "rplans").  Contexts are fresh for every call (a sender or a
receiver that has seen nothing), so every call does the same work; the wire
packets of a shape are made once by a sender outside the timed region.
Results are checked after every call: errno (0, EALREADY on the duplicates)
and the ends.  The counters of every timed call are asserted, so the measured
path is the named one.  A library without the planner (no "nosrplan" knob, no
"srplans" counter; RE_SRTP_LIB names it) runs the same calls: both its
variants take the host engine.  --out FILE --label NAME stores the result
under NAME in FILE (JSON); with "this" and "parent" both there, the criterion
per shape -- the planner's median below the parent's fastest call -- is
evaluated into FILE too.  Prints one JSON line.

  python scripts/srtcp_streams_timing.py [--calls 20] [--warmup 5]
"""
import argparse
import errno
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import re_amd.srtp as P  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--packets", type=int, default=1 << 20)
ap.add_argument("--out")
ap.add_argument("--label", default="this")
args = ap.parse_args()

P.load()
n, suite = args.packets, 1
LEN, SLOT, TAG, GROW = 1200, 1280, 10, 14
KEY = bytes(range(1, 31))
HAS = P.lib().srtp_gpu_tune(b"nosrplan", 0) == 0
COUNTERS = ("srplans", "srundos", "rplans", "rxlate", "rxdups", "rejects",
            "folds", "misses")
t32 = lambda a: torch.from_numpy(
    np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def call(op, ctx, dev, p, e, c, k):
    """one timed call on fresh arrays: (ms, err, end, counter deltas)"""
    pp, ee = p.clone(), e.clone()
    er = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    before = {x: P.counter(x) for x in COUNTERS}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = P.device_batch_dev(op, [ctx], dev.data_ptr(), dev.numel(),
                            pp.data_ptr(), ee.data_ptr(), c.data_ptr(),
                            er.data_ptr(), k)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    assert rc == 0, (rc, P.lib().srtp_gpu_error())
    return dt, er, ee, {x: P.counter(x) - before[x] for x in COUNTERS}


def shape(K, rng):
    """the plain packets of K interleaved SSRCs, their wire form, and the
    disturbed arrivals: (plain, wire, arrays per arrangement)"""
    arena = rng.integers(0, 256, (n, SLOT), dtype=np.uint8)
    arena[:, 0], arena[:, 1] = 0x81, 200
    arena[:, 2], arena[:, 3] = (LEN // 4 - 1) >> 8, (LEN // 4 - 1) & 0xff
    ssrc = (0x40000000 + np.arange(n) % K).astype(np.uint32)
    arena[:, 4:8] = ssrc.astype(">u4").view(np.uint8).reshape(n, 4)
    plain = torch.from_numpy(arena).cuda()
    del arena
    pos = (np.arange(n, dtype=np.uint64) * SLOT).astype(np.uint32)
    # the network: each packet takes part in at most one disturbance
    nxt = np.where(np.arange(n) + K < n, np.arange(n) + K, -1)
    u = rng.random(n)
    free = np.ones(n, dtype=bool)
    key = np.arange(n, dtype=np.float64)
    nswap = 0
    for i in np.flatnonzero((u < 0.001) & (nxt >= 0)).tolist():
        j = int(nxt[i])
        if free[i] and free[j]:
            free[i] = free[j] = False
            key[i], key[j] = key[j], key[i]
            nswap += 1
    lost = np.flatnonzero((u >= 0.001) & (u < 0.002) & free)
    free[lost] = False
    dups = [i for i in np.flatnonzero((u >= 0.002) & (u < 0.0021)).tolist()
            if free[i] and (nxt[i] < 0 or free[nxt[i]])]
    keep = np.ones(n, dtype=bool)
    keep[lost] = False
    src = np.r_[np.flatnonzero(keep), np.array(dups, dtype=np.int64)]
    keys_all = np.r_[key[keep], [(key[nxt[i]] if nxt[i] >= 0 else key[i]) + 0.5
                                 for i in dups]]
    order = np.argsort(keys_all, kind="stable")
    a_src = src[order]
    a_dup = order >= int(keep.sum())
    m = len(a_src)
    pa = pos[:m]
    arr = {
        "inorder": (None, t32(pos), t32(pos + LEN + GROW), t32(pos + SLOT),
                    torch.zeros(n, dtype=torch.int32, device="cuda"),
                    t32(pos + LEN)),
        "disturbed": (torch.from_numpy(a_src).cuda(), t32(pa),
                      t32(pa + LEN + GROW), t32(pa + SLOT),
                      torch.from_numpy(np.where(a_dup, errno.EALREADY, 0)
                                       .astype(np.int32)).cuda(),
                      t32(pa + LEN + GROW -
                          np.where(a_dup, TAG, GROW).astype(np.uint32))),
    }
    info = {"ssrcs": K, "arrivals": int(m), "swaps": nswap,
            "lost": int(len(lost)), "duplicates": len(dups)}
    return plain, t32(pos), t32(pos + LEN), t32(pos + SLOT), arr, info


stat = lambda x: {"median": round(float(np.median(x)), 3),
                  "min": round(min(x), 3), "max": round(max(x), 3)}
out = {"packets": n, "bytes": LEN, "calls": args.calls, "warmup": args.warmup,
       "library": os.environ.get("RE_SRTP_LIB") or "in-tree",
       "has_planner": bool(HAS), "shapes": {}}
rng = np.random.default_rng(20314)
for K in (2, 8, 1):
    plain, p0, e0, c0, arr, info = shape(K, rng)
    wire = plain.clone()
    tx = P.Srtp(suite, KEY)
    dt, er, ee, _ = call("srtcp_encrypt", tx, wire, p0, e0, c0, n)
    assert not er.any().item() and (ee - e0 == GROW).all().item()
    tx.close()
    dev = torch.empty_like(wire)
    runs = []                           # (name, op, arrangement, knob)
    if K > 1:
        runs += [("protect", "srtcp_encrypt", None, 0),
                 ("protect_nosrplan", "srtcp_encrypt", None, 1),
                 ("inorder", "srtcp_decrypt", "inorder", 0),
                 ("inorder_nosrplan", "srtcp_decrypt", "inorder", 1)]
    else:
        runs += [("floor_inorder", "srtcp_decrypt", "inorder", 0)]
    runs += [("disturbed", "srtcp_decrypt", "disturbed", 0),
             ("disturbed_nosrplan", "srtcp_decrypt", "disturbed", 1)]
    ms = {r[0]: [] for r in runs}
    cnt = {}
    for rep in range(args.warmup + args.calls):
        for name, op, a, knob in runs:
            ctx = P.Srtp(suite, KEY)    # fresh for every call
            if op == "srtcp_encrypt":
                dev.copy_(plain)
                p, e, c, k, want, wend = p0, e0, c0, n, None, e0 + GROW
            else:
                gather, p, e, c, want, wend = arr[a]
                k = p.numel()
                if gather is None:
                    dev.copy_(wire)
                else:
                    torch.index_select(wire, 0, gather, out=dev[:k])
            # (a library without the knob answers EINVAL: the host path anyway)
            if knob:
                P.lib().srtp_gpu_tune(b"nosrplan", 1)
            dt, er, ee, d = call(op, ctx, dev, p, e, c, k)
            P.lib().srtp_gpu_tune(b"nosrplan", 0)
            ctx.close()
            assert (er == (0 if want is None else want)).all().item(), \
                (name, "errno")
            assert (ee == wend).all().item(), (name, "end")
            # the measured path is the named one
            planned = HAS and not knob and name != "floor_inorder"
            assert d["srplans"] == int(planned), (name, d)
            if name == "floor_inorder":
                assert d["rplans"] == 1, (name, d)
            if a == "disturbed" and planned:
                assert d["rxdups"] == info["duplicates"], (name, d)
            if rep >= args.warmup:
                ms[name].append(dt)
            if rep == args.warmup:
                cnt[name] = d
    info["ms"] = {k: stat(v) for k, v in ms.items()}
    info["counters"] = cnt
    out["shapes"]["k%d" % K] = info
    del plain, wire, dev, arr
    torch.cuda.empty_cache()
print(json.dumps(out))
if args.out:
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc[args.label] = out
    if "this" in doc and "parent" in doc:
        # per shape: the planner's median below the parent's fastest call
        crit = {}
        for sh, a in doc["this"]["shapes"].items():
            b = doc["parent"]["shapes"][sh]["ms"]
            for name in ("protect", "inorder", "disturbed"):
                if name in a["ms"]:
                    crit["%s_%s" % (sh, name)] = {
                        "planner_median_ms": a["ms"][name]["median"],
                        "parent_min_ms": b[name]["min"],
                        "met": a["ms"][name]["median"] < b[name]["min"]}
        doc["criterion"] = crit
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
