"""Pin the C restatement oracle (oracle/srtp_oracle.c) to the reference for
SRTCP packets of every byte length.

tests/golden/srtcp_geom_golden.json.gz comes from the reference itself
(oracle/gen_srtcp_geom_golden.c, `make -C oracle srtcp_geom_golden`): per
suite and per flags in {0, SRTP_UNENCRYPTED_SRTCP} one sender protects a
packet of every length 8..143 in turn, one receiver unprotects each in a
buffer with no room to spare and, after the last, takes the packet of length
61 again.  tests/test_gpu_srtcp_geom.py compares the device paths with this
oracle at those lengths and above, so the oracle is pinned here first.  CPU
only.
"""
import errno
import gzip
import json
import os

import pytest

from tests import oracle_lib as O
from tests.golden_util import replay_scenario

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                    "srtcp_geom_golden.json.gz")
U = 2                   # SRTP_UNENCRYPTED_SRTCP
_cache = []


def load_geom_golden():
    if not _cache:
        with gzip.open(PATH, "rt") as f:
            _cache.append(json.load(f))
    return _cache[0]


def scenarios():
    return load_geom_golden()["scenarios"]


def test_file_shape():
    """twelve scenarios, every length of the range in order, and the file
    within its size bound"""
    g = load_geom_golden()
    lo, hi = g["lengths"]
    assert (lo, hi) == (8, 143)
    assert os.path.getsize(PATH) <= 256 * 1024
    assert sorted((s["ctxs"][0]["suite"], s["ctxs"][0]["flags"])
                  for s in g["scenarios"]) == \
        [(s, f) for s in range(6) for f in (0, U)]
    for s in g["scenarios"]:
        assert s["ctxs"][0] == s["ctxs"][1]
        enc = [op for op in s["ops"] if op["op"] == "srtcp_encrypt"]
        dec = [op for op in s["ops"] if op["op"] == "srtcp_decrypt"]
        assert [op["end"] for op in enc] == list(range(lo, hi + 1))
        assert len(dec) == len(enc) + 1
        # the receiver's buffers have no room to spare
        assert all(op["size"] == op["end"] for op in dec)


@pytest.mark.parametrize("k", range(12))
def test_oracle_replays_reference(k):
    """errno, pos, end, size and every byte of every call"""
    scn = scenarios()[k]
    assert replay_scenario(O.OracleBackend(), scn) is None


@pytest.mark.parametrize("k", range(12))
def test_round_trip_in_reference(k):
    """every first delivery returns 0 and gives the sender's input back;
    the repeat is EALREADY exactly where the suite has an HMAC"""
    scn = scenarios()[k]
    suite = scn["ctxs"][0]["suite"]
    enc = [op for op in scn["ops"] if op["op"] == "srtcp_encrypt"]
    dec = [op for op in scn["ops"] if op["op"] == "srtcp_decrypt"]
    for e, d in zip(enc, dec):
        L = e["end"]
        assert e["err"] == 0 and d["err"] == 0, L
        assert d["in"] == e["out"][:2 * e["end_o"]], L
        assert (d["pos_o"], d["end_o"]) == (0, L), L
        assert d["out"][:2 * L] == e["in"], L
    rep = dec[-1]
    assert rep["in"] == dec[load_geom_golden()["repeat"] - 8]["in"]
    assert rep["err"] == (errno.EALREADY if suite < 4 else 0)
