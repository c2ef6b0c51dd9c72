"""Large RTP rollover counters: the fixture and the helpers the CPU and GPU
tests share (test infrastructure).

tests/golden/srtp_roc_golden.json.gz is written by oracle/gen_roc_golden.c
from the reference itself: streams put just below ROC 2^16, 2^31 and 2^32
and driven across (srtp_get_index holds the ROC in an int, misc.c:22-41, so
from 2^31 on the replay window's index is sign-extended; behind 2^32 the ROC
is 0 again while the window's top stays near 2^64).
"""
import gzip
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "srtp_roc_golden.json.gz")

# B - 1 for the three boundaries B of the ROC
BOUNDS = {"2p16": 0xffff, "2p31": 0x7fffffff, "2p32": 0xffffffff}

_cache = None


def load():
    global _cache
    if _cache is None:
        with gzip.open(GOLDEN, "rt") as f:
            _cache = json.load(f)["cases"]
    return _cache


def case(name):
    return next(c for c in load() if c["name"] == name)


def ref_lix(roc, seq):
    """the index the reference's window holds for (roc, seq): `int v`
    widened to 64 bits (misc.c:24, 40)"""
    v = roc - (1 << 32) if roc >> 31 else roc
    return (seq + v * 65536) & ((1 << 64) - 1)


def state_tuple(st):
    """(roc, s_l, s_l_set, lix, bitmap) of a fixture state"""
    return (st["roc"], st["s_l"], st["s_l_set"], st["lix"], st["bitmap"])


def oracle_at(be, suite, key, ssrc, st):
    """an oracle context whose stream ssrc is at st = (roc, s_l, s_l_set,
    lix, bitmap)"""
    ctx, err = be.alloc(suite, key, 0)
    assert err == 0
    assert be.l.oracle_stream_set(ctx, ssrc, *st) == 0
    return ctx
