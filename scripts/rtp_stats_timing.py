"""Receiver statistics on device windows (DESIGN "Receiver statistics";
include/re_rtp_stats_batch.h): rtp_rx_stats_batch_dev and
rtp_rx_report_batch_dev timed at two shapes, every array in HBM,

  config4   1 048 576 RTP packets of 212 bytes interleaved at random over
            65 536 sessions, one or two SSRCs per session
  config2   one stream: 1 048 576 packets of one SSRC, no session array

against rtp_rx_stats_host / rtp_rx_report_host on one core over the same
arrays in host memory.  Every stream's sequence numbers run on with a loss
every 50 packets, timestamps step by 160 and arrival times carry up to 400
units of jitter.  Each timed call starts from fresh (zeroed) sessions, so
every call does the same work; the timed region is the call plus a
synchronise.  After the first call per shape the device's stat array and
session states are compared with the host twin's, and the report blocks of
both sides with each other.  Prints one JSON line (and writes it to --out).

  python scripts/rtp_stats_timing.py [--calls 10] [--warmup 3] [--out FILE]
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

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--host-calls", type=int, default=3)
ap.add_argument("--packets", type=int, default=1 << 20)
ap.add_argument("--sessions", type=int, default=1 << 16)
ap.add_argument("--out", default=None)
args = ap.parse_args()

P.load()
assert torch.cuda.is_available(), "needs a GPU: there is no fallback"
SRC_DT, SESS_DT = P.rtp_rx_dtypes()
MSG_DT, RB_DT = P.rtcp_enc_dtypes()[:2]
SLOT, LEN = 256, 212
n = args.packets


def make(nsess, one_stream):
    """arena, pos, end, sess (None for one stream), arrival"""
    rng = np.random.default_rng(20316 + nsess)
    if one_stream:
        sess, stream = None, np.zeros(n, np.int64)
    else:
        sess = rng.integers(0, nsess, n).astype(np.uint32)
        second = (sess % 3 == 2) & (rng.random(n) < 0.5)
        stream = 2 * sess.astype(np.int64) + second
    # the packet's ordinal in its stream, in array order
    order = np.argsort(stream, kind="stable")
    st = stream[order]
    first = np.r_[True, st[1:] != st[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(n), 0))
    ordinal = np.empty(n, np.int64)
    ordinal[order] = np.arange(n) - start
    s0 = (stream * 7919 + 65000) & 0xffff
    seq = (s0 + ordinal + ordinal // 50) & 0xffff
    ts = (stream * 1000003 + 160 * ordinal) & 0xffffffff
    arrival = (ts + 90000 + rng.integers(0, 400, n)) & 0xffffffff
    ssrc = (0x40000000 + stream).astype(np.uint32)
    arena = np.zeros((n, SLOT), np.uint8)
    arena[:, 0], arena[:, 1] = 0x80, 96
    arena[:, 2], arena[:, 3] = seq >> 8, seq & 0xff
    arena[:, 4:8] = ts.astype(">u4").view(np.uint8).reshape(n, 4)
    arena[:, 8:12] = ssrc.astype(">u4").view(np.uint8).reshape(n, 4)
    pos = (np.arange(n, dtype=np.uint64) * SLOT).astype(np.uint32)
    return (arena.reshape(-1), pos, pos + np.uint32(LEN), sess,
            arrival.astype(np.uint32))


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


def ptr(x):
    if x is None:
        return None
    return x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data


def stats(host, arena, pos, end, sess, arrival, sessv, nsess, stat):
    rc = P.rtp_rx_stats(ptr(arena), n * SLOT, ptr(pos), ptr(end), None,
                        ptr(sess), ptr(arrival), n, ptr(sessv), nsess,
                        ptr(stat), host=host)
    assert rc == 0, (rc, P.lib().srtp_gpu_error())


def report(host, sessv, nsess, rb, nrb, local, msg):
    rc = P.rtp_rx_report(ptr(sessv), nsess, 123456, ptr(rb), ptr(nrb),
                         ptr(local), ptr(msg), host=host)
    assert rc == 0, (rc, P.lib().srtp_gpu_error())


def med(x):
    return {"median": round(float(np.median(x)), 3), "min": round(min(x), 3),
            "max": round(max(x), 3)}


def run(name, nsess, one_stream):
    h = make(nsess, one_stream)
    d = [None if x is None else dev(x) for x in h]
    local = np.arange(nsess, dtype=np.uint32)
    # host twin, one core
    h_sessv = np.zeros(nsess, SESS_DT)
    h_stat = np.zeros(n, np.int32)
    h_rb, h_nrb = np.zeros(nsess * 8, RB_DT), np.zeros(nsess, np.uint32)
    h_msg = np.zeros(nsess, MSG_DT)
    hs, hr = [], []
    for _ in range(args.host_calls):
        h_sessv[:] = 0
        t0 = time.perf_counter()
        stats(True, *h, h_sessv, nsess, h_stat)
        hs.append((time.perf_counter() - t0) * 1e3)
        state = h_sessv.copy()
        t0 = time.perf_counter()
        report(True, h_sessv, nsess, h_rb, h_nrb, local, h_msg)
        hr.append((time.perf_counter() - t0) * 1e3)
    assert not h_stat.any()
    # the device
    d_sessv = dev(np.zeros(nsess, SESS_DT))
    d_stat = dev(np.zeros(n, np.int32))
    d_rb, d_nrb = dev(h_rb), dev(h_nrb)
    d_msg, d_local = dev(h_msg), dev(local)
    ds, dr = [], []
    for r in range(args.warmup + args.calls):
        d_sessv.zero_()
        d_stat.fill_(0x5a)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats(False, *d, d_sessv, nsess, d_stat)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if r == 0:
            assert (d_stat.cpu().numpy().view(np.int32) == h_stat).all()
            assert d_sessv.cpu().numpy().tobytes() == state.tobytes()
            torch.cuda.synchronize()
        t2 = time.perf_counter()
        report(False, d_sessv, nsess, d_rb, d_nrb, d_local, d_msg)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if r == 0:
            assert d_rb.cpu().numpy().tobytes() == h_rb.tobytes()
            assert d_msg.cpu().numpy().tobytes() == h_msg.tobytes()
            assert d_sessv.cpu().numpy().tobytes() == h_sessv.tobytes()
        if r >= args.warmup:
            ds.append((t1 - t0) * 1e3)
            dr.append((t3 - t2) * 1e3)
    out = {"sessions": nsess, "packets": n,
           "report_blocks": int(h_nrb.sum()),
           "stats_dev_ms": med(ds), "report_dev_ms": med(dr),
           "stats_host_1core_ms": med(hs), "report_host_1core_ms": med(hr)}
    out["stats_speedup"] = round(out["stats_host_1core_ms"]["median"] /
                                 out["stats_dev_ms"]["median"], 2)
    out["report_speedup"] = round(out["report_host_1core_ms"]["median"] /
                                  out["report_dev_ms"]["median"], 2)
    out["stats_dev_Mpkt_s"] = round(n / out["stats_dev_ms"]["median"] / 1e3,
                                    1)
    return name, out


res = {"shape": "%d RTP packets of %d B in %d-B slots, every array in HBM; "
                "host: rtp_rx_stats_host / rtp_rx_report_host on one core; "
                "each call from zeroed sessions; call + synchronise"
                % (n, LEN, SLOT),
       "calls": args.calls, "warmup": args.warmup,
       "host_calls": args.host_calls,
       "device": torch.cuda.get_device_name(0)}
for name, nsess, one in (("config4", args.sessions, False),
                         ("config2_one_stream", 1, True)):
    k, v = run(name, nsess, one)
    res[k] = v
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
