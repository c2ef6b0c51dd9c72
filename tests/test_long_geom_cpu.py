"""Pin the C restatement oracle (oracle/srtp_oracle.c) to the reference for
SRTP and SRTCP packets of about 2 KiB and above.

tests/golden/long_geom_golden.json.gz comes from the reference itself
(oracle/gen_long_geom_golden.c, `make -C oracle long_geom_golden`): per suite
and per {SRTP, SRTCP, SRTCP with SRTP_UNENCRYPTED_SRTCP} one sender protects
a packet of every 37th length from 208 to 1983, of every length 1984..2112
and of 4031, 4032, 4033 and 9000 bytes in turn; one receiver unprotects each
in a buffer with no room to spare.  The packets are a fixed function of
their length (tests/long_geom.py golden_packet), so the file holds per call
only errno, pos, end, size and the first 16 bytes of the SHA-256 of the
buffer.  tests/test_gpu_long_geom.py compares the per-call paths and the
mbuf batches with this oracle at these lengths, so the oracle is pinned here
first.  CPU only.
"""
import gzip
import hashlib
import json
import os

import pytest

from tests import long_geom as LG
from tests import oracle_lib as O

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                    "long_geom_golden.json.gz")
LENGTHS = list(range(208, 1984, 37)) + list(range(1984, 2113)) + \
    [4031, 4032, 4033, 9000]
_cache = []


def load_long_golden():
    if not _cache:
        with gzip.open(PATH, "rt") as f:
            _cache.append(json.load(f))
    return _cache[0]


def test_file_shape():
    """eighteen scenarios, every length of the list in order (the whole
    window 1984..2112), and the file within its size bound"""
    g = load_long_golden()
    assert os.path.getsize(PATH) <= 256 * 1024
    assert g["lengths"] == LENGTHS
    assert set(range(1984, 2113)) <= set(g["lengths"])
    assert g["columns"] == ["L", "dec", "size", "end", "err", "pos_o",
                            "end_o", "size_o", "sha256_16"]
    assert (g["seq0"], g["ssrc"]) == (LG.GOLDEN_SEQ0, LG.GOLDEN_SSRC)
    assert [(s["suite"], s["kind"], s["flags"]) for s in g["scenarios"]] == \
        [(s, k, f) for s in range(6) for k, f in LG.KINDS]
    for s in g["scenarios"]:
        enc, dec = s["calls"][0::2], s["calls"][1::2]
        assert [c[:2] for c in enc] == [[L, 0] for L in LENGTHS]
        assert [c[:2] for c in dec] == [[L, 1] for L in LENGTHS]
        assert all(c[2] == c[3] + g["room"] and c[3] == c[0] for c in enc)
        # the receiver's buffers have no room to spare: size == end, the
        # sender's end
        assert all(d[2] == d[3] == e[6] for e, d in zip(enc, dec))
        assert all(len(c[8]) == 32 for c in s["calls"])


@pytest.mark.parametrize("k", range(18))
def test_oracle_replays_reference(k):
    """errno, pos, end, size and the digest of the buffer of every call; every
    delivery returns 0 and gives the sender's input back"""
    scn = load_long_golden()["scenarios"][k]
    be = O.OracleBackend()
    key = bytes.fromhex(scn["key"])
    (tx, e1), (rx, e2) = (be.alloc(scn["suite"], key, scn["flags"])
                          for _ in range(2))
    assert (e1, e2) == (0, 0)
    ops = LG.op_names(scn["kind"])
    prot = None
    for L, dec, size, end, *want in scn["calls"]:
        pkt = LG.golden_packet(scn["kind"], L)
        inb = prot if dec else pkt
        assert len(inb) == end, (L, dec)
        r = be.call(rx if dec else tx, ops[dec], size, 0, end, inb, end)
        n = max(end, r[2])
        got = list(r[:4]) + [hashlib.sha256(r[4][:n]).hexdigest()[:32]]
        assert got == want, (scn["name"], L, dec, got[:4], want[:4])
        assert r[0] == 0, (L, dec)
        if dec:
            assert (r[1], r[2]) == (0, L) and r[4][:L] == pkt, L
        else:
            prot = r[4][:r[2]]
    be.free(tx)
    be.free(rx)
