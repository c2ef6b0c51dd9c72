"""RTCP session state on device arrays (DESIGN "RTCP session state";
include/re_rtcp_sess_batch.h): the four entries timed per call, every array
in HBM,

  handle       262 144 decoded compounds (an SR with one report block and an
               SDES; one in twenty also a BYE) interleaved at random over
               65 536 sessions, four SSRCs per session
  tx           1 048 576 outgoing RTP packets of 172 bytes over 65 536
               sessions
  tx_one       the same packets in one session, no session array
  report       the SR / RR descriptors and report blocks of 65 536 sessions
  stats        65 536 rtcp_stats queries

against the host twins on one core over the same arrays in host memory.
Each timed call starts from the same states (handle, tx: fresh sessions;
report, stats: the states handle and tx left), so every call does the same
work; the timed region is the call plus a synchronise.  After the first
call per shape the device's outputs and states are compared with the host
twin's.  Prints one JSON line (and writes it to --out).

  python scripts/rtcp_sess_timing.py [--calls 10] [--warmup 3] [--out FILE]
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
ap.add_argument("--compounds", type=int, default=1 << 18)
ap.add_argument("--packets", type=int, default=1 << 20)
ap.add_argument("--sessions", type=int, default=1 << 16)
ap.add_argument("--out", default=None)
args = ap.parse_args()

P.load()
assert torch.cuda.is_available(), "needs a GPU: there is no fallback"
SESS_DT = P.rtp_rx_dtypes()[1]
EXT_DT = P.rtcp_sess_ext_dtype()
MSG_DT, RB_DT = P.rtcp_enc_dtypes()[:2]
DESC_DT, ITEM_DT = P.rtcp_dec_dtypes()
MAXMSG, MAXITEM = 3, 6
SLOT, LEN = 192, 172
NOW_US = 1694531965654321
nsess, nc, n = args.sessions, args.compounds, args.packets
rng = np.random.default_rng(20317)


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


def ptr(x):
    if x is None:
        return None
    return x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data


def med(x):
    return {"median": round(float(np.median(x)), 3), "min": round(min(x), 3),
            "max": round(max(x), 3)}


def compounds():
    """desc, nmsg, item, nitem, sess as rtcp_decode_full_batch_dev leaves
    them"""
    sess = rng.integers(0, nsess, nc).astype(np.uint32)
    ssrc = (0x2000 * (sess + 1) + 3 + 8 * rng.integers(0, 4, nc)).astype(
        np.uint32)
    bye = rng.random(nc) < 0.05
    desc = np.zeros((nc, MAXMSG), DESC_DT)
    item = np.zeros((nc, MAXITEM), ITEM_DT)
    desc["pt"][:, 0], desc["count"][:, 0] = 200, 1
    desc["pt"][:, 1], desc["count"][:, 1] = 202, 1
    desc["ssrc"][:, 0] = desc["ssrc"][:, 1] = ssrc
    item["kind"][:, 0] = 1                          # SR
    item["v"][:, 0, :5] = rng.integers(0, 1 << 32, (nc, 5))
    item["kind"][:, 1] = 2                          # RB
    item["v"][:, 1] = rng.integers(0, 1 << 24, (nc, 7))
    item["v"][:, 1, 5] = 0xfffd0000 + rng.integers(0, 1 << 16, nc)
    item["msg"][:, 2:4] = 1                         # SDES chunk, CNAME
    item["kind"][:, 2], item["kind"][:, 3] = 3, 4
    item["v"][:, 2, 0] = ssrc
    desc["pt"][bye, 2], desc["count"][bye, 2] = 203, 1
    desc["ssrc"][bye, 2] = ssrc[bye]
    item["msg"][bye, 4], item["kind"][bye, 4] = 2, 5
    item["v"][bye, 4, 0] = ssrc[bye]
    nmsg = np.where(bye, 3, 2).astype(np.uint32)
    nitem = np.where(bye, 5, 4).astype(np.uint32)
    return desc, nmsg, item, nitem, sess


def packets():
    """arena, pos, end, jfs_rt, sess"""
    sess = rng.integers(0, nsess, n).astype(np.uint32)
    arena = np.zeros((n, SLOT), np.uint8)
    arena[:, 0], arena[:, 1] = 0x80, 96
    arena[:, 4:8] = rng.integers(0, 256, (n, 4))
    pos = (np.arange(n, dtype=np.uint64) * SLOT).astype(np.uint32)
    jfs = (NOW_US - rng.integers(0, 1 << 30, n)).astype(np.uint64)
    return arena.reshape(-1), pos, pos + np.uint32(LEN), jfs, sess


def timed(name, call, reset, check, count):
    """call(host) timed on the host twin and on the device, each call after
    reset(host); check() after the device's first call"""
    hs, ds = [], []
    for _ in range(args.host_calls):
        reset(True)
        t0 = time.perf_counter()
        call(True)
        hs.append((time.perf_counter() - t0) * 1e3)
    for r in range(args.warmup + args.calls):
        reset(False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if r == 0:
            check()
        if r >= args.warmup:
            ds.append((t1 - t0) * 1e3)
    out = {"items": count, "dev_ms": med(ds), "host_1core_ms": med(hs)}
    out["speedup"] = round(out["host_1core_ms"]["median"] /
                           out["dev_ms"]["median"], 2)
    out["dev_M_per_s"] = round(count / out["dev_ms"]["median"] / 1e3, 1)
    res[name] = out


def same(d, h):
    assert d.cpu().numpy().tobytes() == h.tobytes()


ext0 = np.zeros(nsess, EXT_DT)
ext0["srate_tx"] = ext0["srate_rx"] = 8000
h_sessv, h_extv = np.zeros(nsess, SESS_DT), ext0.copy()
d_sessv, d_extv, d_ext0 = dev(h_sessv), dev(ext0), dev(ext0)
res = {"shape": "%d compounds / %d packets of %d B in %d-B slots over %d "
                "sessions, every array in HBM; host: the _host twins on one "
                "core; call + synchronise" % (nc, n, LEN, SLOT, nsess),
       "calls": args.calls, "warmup": args.warmup,
       "host_calls": args.host_calls,
       "device": torch.cuda.get_device_name(0)}


def reset(host):
    if host:
        h_sessv[:] = 0
        h_extv[:] = ext0
    else:
        d_sessv.zero_()
        d_extv.copy_(d_ext0)


# ---- handle ------------------------------------------------------------
hc = compounds()
dc = [dev(x) for x in hc]
h_stat, d_stat = np.zeros(nc, np.int32), dev(np.zeros(nc, np.int32))


def handle(host):
    a, st = (hc, h_stat) if host else (dc, d_stat)
    rc = P.rtcp_rx_handle(ptr(a[0]), MAXMSG, ptr(a[1]), ptr(a[2]), MAXITEM,
                          ptr(a[3]), None, ptr(a[4]), nc,
                          ptr(h_sessv if host else d_sessv),
                          ptr(h_extv if host else d_extv), nsess, 1000,
                          NOW_US, ptr(st), host=host)
    assert rc == 0, (rc, P.lib().srtp_gpu_error())


def check_states():
    same(d_stat, h_stat)
    same(d_sessv, h_sessv)
    same(d_extv, h_extv)


timed("handle", handle, reset, check_states, nc)
res["handle"]["members"] = int(h_sessv["memberc"].sum())

# ---- tx ----------------------------------------------------------------
hp = packets()
dp = [dev(x) for x in hp]
h_stat, d_stat = np.zeros(n, np.int32), dev(np.zeros(n, np.int32))
after_handle = h_sessv.copy()


def tx(one):
    def call(host):
        a, st = (hp, h_stat) if host else (dp, d_stat)
        rc = P.rtp_tx_stats(ptr(a[0]), n * SLOT, ptr(a[1]), ptr(a[2]), None,
                            None if one else ptr(a[4]), ptr(a[3]), n,
                            ptr(h_extv if host else d_extv), nsess, ptr(st),
                            host=host)
        assert rc == 0, (rc, P.lib().srtp_gpu_error())
    return call


def reset_ext(host):
    if host:
        h_extv[:] = ext0
    else:
        d_extv.copy_(d_ext0)


def check_ext():
    same(d_stat, h_stat)
    same(d_extv, h_extv)
    assert int(h_extv["psent"].sum()) == n


timed("tx_one", tx(True), reset_ext, check_ext, n)
timed("tx", tx(False), reset_ext, check_ext, n)

# ---- report and stats, on the states handle and tx left -------------------
h_sessv[:] = after_handle
d_sessv.copy_(dev(after_handle))
state = (h_sessv.copy(), h_extv.copy())
d_state = (dev(state[0]), dev(state[1]))
local = np.arange(nsess, dtype=np.uint32)
h_rb, h_nrb = np.zeros(nsess * 8, RB_DT), np.zeros(nsess, np.uint32)
h_msg = np.zeros(nsess, MSG_DT)
d_rb, d_nrb, d_msg, d_local = dev(h_rb), dev(h_nrb), dev(h_msg), dev(local)


def reset_state(host):
    if host:
        h_sessv[:], h_extv[:] = state
    else:
        d_sessv.copy_(d_state[0])
        d_extv.copy_(d_state[1])


def report(host):
    a = (h_sessv, h_extv, h_rb, h_nrb, local, h_msg) if host else \
        (d_sessv, d_extv, d_rb, d_nrb, d_local, d_msg)
    rc = P.rtcp_tx_report(ptr(a[0]), ptr(a[1]), nsess, 6000,
                          NOW_US + 5000000, ptr(a[2]), ptr(a[3]), ptr(a[4]),
                          ptr(a[5]), host=host)
    assert rc == 0, (rc, P.lib().srtp_gpu_error())


def check_report():
    same(d_rb, h_rb)
    same(d_nrb, h_nrb)
    same(d_msg, h_msg)
    same(d_extv, h_extv)
    same(d_sessv, h_sessv)


timed("report", report, reset_state, check_report, nsess)
res["report"]["sender_reports"] = int((h_msg["pt"] == 200).sum())

q_sess = rng.integers(0, nsess, nsess).astype(np.uint32)
q_ssrc = (0x2000 * (q_sess + 1) + 3 + 8 * rng.integers(0, 5, nsess)).astype(
    np.uint32)
h_out, h_err = np.zeros((nsess, 7), np.uint32), np.zeros(nsess, np.int32)
d_qs, d_qq, d_out, d_err = dev(q_sess), dev(q_ssrc), dev(h_out), dev(h_err)


def stats(host):
    a = (h_sessv, h_extv, q_sess, q_ssrc, h_out, h_err) if host else \
        (d_sessv, d_extv, d_qs, d_qq, d_out, d_err)
    rc = P.rtcp_stats(ptr(a[0]), ptr(a[1]), nsess, ptr(a[2]), ptr(a[3]),
                      nsess, ptr(a[4]), ptr(a[5]), host=host)
    assert rc == 0, (rc, P.lib().srtp_gpu_error())


def check_stats():
    same(d_out, h_out)
    same(d_err, h_err)


timed("stats", stats, lambda host: None, check_stats, nsess)
res["stats"]["found"] = int((h_err == 0).sum())

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
