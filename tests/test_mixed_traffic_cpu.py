"""The scenarios of tests/mixed_traffic.py are what they claim to be, by the
oracle alone, so that no comparison of tests/test_gpu_mixed_suites.py passes
on an empty case: every suite and every header class occurs in a batch, a
stream of every suite rolls its ROC over inside the first batch, the receive
rows hold per suite a success, an authentication failure and a replay, the
forged share stays within 5 %, and the odd session is where it was asked.

The replayed SRTCP packet: the AES-CM suites keep the window and give
EALREADY; the GCM suites keep none (srtcp.c:217-226 checks the replay only
behind the HMAC), so the oracle accepts the packet a second time, errno 0, and
that is what the guard requires for suites 4 and 5.
"""
import errno

import pytest

import re_amd.srtp as P
from tests import mixed_traffic as M


def by_suite(sc, st):
    out = {}
    for (s, _), r in zip(st.pkts, st.rows):
        out.setdefault(sc.suites[s], []).append(r[0])
    return out


def shift_classes(st):
    return {M.hdr_len(p) % 16 for _, p in st.pkts}


def test_sessions_are_as_asked():
    assert M.SUITES_OF("cycle") == [0, 1, 2, 3, 4, 5] * 2
    for shape, at in (("odd_1", 1), ("odd_mid", 150), ("odd_last", 299)):
        su = M.SUITES_OF(shape)
        assert len(su) == 300 and su[at] == 5
        assert [u for i, u in enumerate(su) if i != at] == [1] * 299
    for shape in M.SHAPES:
        su = M.SUITES_OF(shape)
        keys = [(u, M.session_key(u, s)) for s, u in enumerate(su)]
        assert len(set(keys)) == len(su)
        assert all(len(k) == P.key_len(u) + P.salt_len(u) for u, k in keys)
        # both values of SRTP_UNENCRYPTED_SRTCP in the batch
        fl = M.rtcp_flags(su)
        assert set(fl) == {0, M.U}
        for u in set(su):
            mine = [f for f, v in zip(fl, su) if v == u]
            assert mine == [M.U if k % 2 else 0 for k in range(len(mine))]


@pytest.mark.parametrize("shape", M.SHAPES)
def test_rtp_scenario_is_what_it_claims(shape):
    sc = M.rtp_scenario(shape)
    tx1, rx1, tx2, rx2 = sc.steps
    assert [(s.side, s.op) for s in sc.steps] == \
        [("tx", "srtp_encrypt"), ("rx", "srtp_decrypt")] * 2
    suites = set(sc.suites)
    for st in sc.steps:
        assert 0 < len(st.pkts) <= 600
        assert len(st.rows) == len(st.pkts) == len(st.key)
        assert {sc.suites[s] for s, _ in st.pkts} == suites
        assert shift_classes(st) == {0, 4, 8, 12}
        # interleaved: no stream sends twice in a row while others wait
        runs = sum(a == b for a, b in zip(st.key, st.key[1:]))
        assert runs <= len(suites), runs
    # every session once with an extension, CSRC counts 0..3, payloads 0..70
    # and one of 1200 bytes per suite
    for st in (tx1, tx2):
        ext = [s for s, p in st.pkts if p[0] & 0x10]
        assert sorted(ext) == list(range(len(sc.suites)))
        assert {p[0] & 15 for _, p in st.pkts} == {0, 1, 2, 3}
    lens = [len(p) - M.hdr_len(p) for _, p in tx1.pkts]
    assert set(range(71)) <= set(lens)
    big = {sc.suites[s] for (s, _), n in zip(tx1.pkts, lens) if n == 1200}
    assert big == suites
    if shape == "cycle":
        two = {s for s, k in tx1.key if k == 1}
        assert two == set(range(6, 12))
    # sequence numbers start 3..8 below 65536; the ROC of a stream of every
    # suite is 1 after the first batch, on both sides
    first = {}
    for (s, p), k in zip(tx1.pkts, tx1.key):
        first.setdefault(k, int.from_bytes(p[2:4], "big"))
    assert {65536 - v for v in first.values()} <= set(range(3, 9))
    for st in (tx1, rx1):
        rolled = {sc.suites[s] for (s, x), v in st.states.items()
                  if v[0][0] == 1}
        assert rolled == suites, (st.what, rolled)
        assert all(v[0][2] == 1 for v in st.states.values())
    # protect rows are clean; the receive rows hold, per suite, a success, an
    # authentication failure and a replay, and nothing else
    assert not any(tx1.errnos()) and not any(tx2.errnos())
    assert not any(rx2.errnos())
    for u, codes in by_suite(sc, rx1).items():
        assert sorted(set(codes)) == sorted({0, M.EAUTH, errno.EALREADY}), u
        assert codes.count(M.EAUTH) == 1 and codes.count(errno.EALREADY) == 1
    assert [i for i, e in enumerate(rx1.errnos()) if e == M.EAUTH] == \
        rx1.forged
    assert len(rx1.forged) == len(suites)
    assert len(rx1.forged) * 20 <= len(rx1.pkts)
    # the swap: an accepted packet below an earlier accepted one, per suite
    late = set()
    for u, k in sc.star.items():
        top = -1
        for (s, p), kk, r in zip(rx1.pkts, rx1.key, rx1.rows):
            if kk != k or r[0]:
                continue
            x = int.from_bytes(p[2:4], "big")
            x += 65536 if x < 32768 else 0
            if x < top:
                late.add(u)
            top = max(top, x)
    assert late == suites
    # the forged packets: payload for the even suites, tag for the odd ones
    sent, _ = M.wire_of(tx1)
    for i in rx1.forged:
        s, q = rx1.pkts[i]
        p, = [w for t, w in sent if t == s and w[:12] == q[:12] and
              len(w) == len(q)]
        diff = [j for j in range(len(p)) if p[j] != q[j]]
        u = sc.suites[s]
        if u % 2:
            assert diff == [len(p) - 1]
        else:
            assert diff == [M.hdr_len(p)] and diff[0] < len(p) - P.tag_len(u)
        assert q[2:4] != b"\x00\x00"


@pytest.mark.parametrize("shape", ["cycle", "odd_mid"])
def test_rtcp_scenario_is_what_it_claims(shape):
    sc = M.rtcp_scenario(shape)
    tx1, rx1, tx2, rx2 = sc.steps
    suites = set(sc.suites)
    lens = set()
    for st in sc.steps:
        assert 0 < len(st.pkts) <= 600
        assert {sc.suites[s] for s, _ in st.pkts} == suites
        # both E bits in the batch
        assert {sc.flags[s] for s, _ in st.pkts} == {0, M.U}
    for st in (tx1, tx2):
        lens |= {len(p) for _, p in st.pkts}
    assert min(lens) == 8 and max(lens) == 200
    assert {n % 4 for n in lens} == {0, 1, 2, 3}
    # one SSRC per session
    assert len({k for st in sc.steps for k in st.key}) == len(sc.suites)
    # per suite one protect refused for a byte of room, one that fits exactly
    for u, codes in by_suite(sc, tx1).items():
        assert sorted(set(codes)) == [0, errno.ENOMEM], u
        assert codes.count(errno.ENOMEM) == 1
    exact = [(s, p, r) for (s, p), room, r in
             zip(tx1.pkts, tx1.rooms, tx1.rows)
             if room == M.trailer(sc.suites[s])]
    assert {sc.suites[s] for s, _, _ in exact} == suites
    assert all(r[0] == 0 and r[2] == len(p) + M.trailer(sc.suites[s])
               for s, p, r in exact)
    assert not any(tx2.errnos()) and not any(rx2.errnos())
    # receive: per suite a success, an authentication failure, and for the
    # replayed packet what the oracle gives (module docstring)
    for u, codes in by_suite(sc, rx1).items():
        replay = errno.EALREADY if P.salt_len(u) == 14 else 0
        assert sorted(set(codes)) == sorted({0, M.EAUTH, replay}), (u, codes)
        assert codes.count(M.EAUTH) == 1
        if replay:
            assert codes.count(replay) == 1
    assert [i for i, e in enumerate(rx1.errnos()) if e == M.EAUTH] == \
        rx1.forged
    assert len(rx1.forged) * 20 <= len(rx1.pkts)
    # the replayed packet is in the batch twice, for every suite
    twice = {sc.suites[s] for s, p in rx1.pkts if rx1.pkts.count((s, p)) == 2}
    assert twice == suites
    # the sender's index and the receiver's window moved
    for (s, x), v in tx2.states.items():
        assert v[1][0] >= 2 and v[0] == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("side", ["tx", "rx"])
@pytest.mark.parametrize("pair", M.HAND_PAIRS)
def test_handover_scenario_is_what_it_claims(pair, side):
    sc = M.handover_scenario(pair, side)
    assert [st.what for st in sc.steps] == \
        [("A", 0), ("A", 4), ("B", 0), ("C", 0), ("C", 4)]
    a0, a4, b, c0, c4 = sc.steps
    for st in (a0, a4, c0, c4):
        lo, hi = st.sub
        assert {s for s, _ in st.pkts} == set(range(lo, hi))
        assert len({sc.suites[s] for s, _ in st.pkts}) == 1
        assert not any(st.errnos())
    assert {sc.suites[s] for s, _ in b.pkts} == set(pair) and b.sub == (0, 8)
    # no stream has rolled over before stage B, every one has after it
    assert all(v[0][0] == 0 for v in a4.states.values())
    assert len(b.states) == 8 and all(v[0][0] == 1 for v in b.states.values())
    for s in range(8):
        seqs = [int.from_bytes(p[2:4], "big") for t, p in b.pkts if t == s]
        assert 65535 in seqs and 0 in seqs
    bad = [i for i, e in enumerate(b.errnos()) if e]
    if side == "tx":
        assert not bad
    else:
        assert bad == b.forged and len(bad) == 2
        assert {sc.suites[b.pkts[i][0]] for i in bad} == set(pair)
        assert all(b.rows[i][0] == M.EAUTH for i in bad)
        assert all(b.pkts[i][1][2:4] != b"\x00\x00" for i in bad)
        assert len(bad) * 20 <= len(b.pkts)


def test_multi_scenario_is_what_it_claims():
    sc = M.multi_scenario(1)
    assert len(sc.steps) == 3 and set(sc.suites) == {1}
    for st in sc.steps:
        assert not any(st.errnos())
        assert {k for k in st.key if k[1]} == {(1, 1)}
        assert {s for s, _ in st.pkts} == set(range(M.MULTI_N))
    # session 1 holds two streams after the first batch
    assert sum(1 for s, _ in sc.steps[0].states if s == 1) == 2
    assert all(v[0][0] == 1 for v in sc.steps[0].states.values())


def test_scenarios_repeat():
    """built twice from their seeds: identical batches and rows"""
    a = M.rtp_scenario("cycle")
    M._built.pop(("rtp", "cycle"))
    b = M.rtp_scenario("cycle")
    assert a is not b
    for x, y in zip(a.steps, b.steps):
        assert x.pkts == y.pkts and x.rows == y.rows and x.states == y.states
