"""The scenarios of tests/async_traffic.py are what they claim to be, by the
oracle alone, so that no GPU test of tests/test_gpu_async_chain.py passes on a
batch that is something else: the named disturbance shows in the oracle's rows
of c2, every other row of every call is errno 0, and the sizes reach the
workgroup and segment bounds the routes are about.
"""
import errno

import pytest

from tests import async_traffic as T

CASES = [(n, s) for n in T.ROUTES for s in T.SUITES]


def rows_by_stream(call):
    by = {}
    for i, (key, r) in enumerate(zip(call.key, call.rows)):
        by.setdefault(key, []).append((i, r))
    return by


def ext_seq(call):
    """extended sequence numbers of a call's packets, per stream, in arrival
    order: the streams start in 65400.., so a sequence number below 32768 is
    past the rollover"""
    out = []
    for s, p in call.pkts:
        seq = int.from_bytes(p[2:4], "big")
        out.append(seq + (65536 if seq < 32768 else 0))
    return out


@pytest.mark.parametrize("name,suite", CASES)
def test_scenario_is_what_it_claims(name, suite):
    sc = T.scenario(name, suite)
    roles = [c.role for c in sc.calls]
    assert roles[-4:] == ["c1", "c2", "c3", "c4"]
    assert all(r == "pre" for r in roles[:-4])
    c1, c2, c3, c4 = sc.calls[-4:]
    # disjoint contexts; c3 reads c1's arena on the receiver of c1's keys
    assert len({c.set for c in (c1, c2, c3, c4)}) == 4
    assert sc.calls[c3.share] is c1 and sc.sets["rx1"] == sc.sets["tx1"]
    assert all(c.set == c2.set for c in sc.calls[:-4])
    for c in sc.calls:
        assert len(c.rows) == len(c.pkts) == len(c.key)
        if c is not c2:
            assert not any(c.errnos()), (c.role, c.errnos())
    # payloads of 16..64 bytes, sequence numbers from 65400 on, and a ROC
    # rollover inside c1, c2 and c4
    for c in (c1, c2, c4):
        tag = 0 if c.op == "srtp_encrypt" else T.TAG[suite]
        for s, p in c.pkts:
            if len(p) >= 12:
                assert 16 <= len(p) - 12 - 4 * (p[0] & 15) - tag <= 64
        x = [v for v, e in zip(ext_seq(c), c.errnos())
             if e != errno.ETIMEDOUT]
        assert min(x) >= 65400 and max(x) >= 65536 > min(x), c.role
    for set_id, st in sc.states.items():
        assert st and all(v != (0, 0, 0, 0) for v in st.values()), set_id
    assert max(v[0] for v in sc.states[c2.set].values()) == 1
    assert [v[:2] for v in sc.states["tx1"].values()] == \
        [v[:2] for v in sc.states["rx1"].values()]
    for set_id in ("tx1", "rx1", "tx3"):
        assert [v[0] for v in sc.states[set_id].values()] == [1]

    e2 = c2.errnos()
    cl = sc.claims
    bad = {i for i, e in enumerate(e2) if e}
    want = set()
    # EAUTH at exactly the forged indices
    assert {i for i in bad if e2[i] == T.EAUTH} == set(cl["forged"])
    want |= set(cl["forged"])
    if name in ("forged1", "forged_s", "m_forged"):
        assert len(cl["forged"]) == 2
    for what, code in (("timedout", errno.ETIMEDOUT),
                       ("short", errno.EBADMSG), ("enomem", errno.ENOMEM)):
        for i in cl.get(what, ()):
            assert e2[i] == code, (what, i, e2[i])
            want.add(i)
    dups = {i for i in bad if e2[i] == errno.EALREADY}
    if cl.get("dup"):
        assert dups
        want |= dups
    # every other row is errno 0
    assert bad == want, sorted(bad ^ want)
    if cl.get("swap"):
        # an accepted packet below an earlier accepted one of its stream
        x = ext_seq(c2)
        late = 0
        for key, rows in rows_by_stream(c2).items():
            top = -1
            for i, r in rows:
                if r[0] == 0:
                    late += x[i] < top
                    top = max(top, x[i])
        assert late >= 1
    else:
        # every stream arrives in order
        x = ext_seq(c2)
        for key, rows in rows_by_stream(c2).items():
            seqs = [x[i] for i, r in rows if r[0] not in (errno.ETIMEDOUT,
                                                          errno.EBADMSG)]
            assert seqs == sorted(seqs), key


def test_sizes_reach_the_bounds():
    for suite in T.SUITES:
        for name in ("rx", "forged1"):
            c2 = T.scenario(name, suite).call("c2")
            e2 = c2.errnos()
            bad = [i for i, e in enumerate(e2) if e]
            assert T.WG < len(c2.pkts) < 2 * T.WG
            # something in both workgroups
            assert min(bad) < T.WG <= max(bad), (name, bad)
        c2 = T.scenario("rx", suite).call("c2")
        x = ext_seq(c2)
        late = [i for i in range(1, len(x)) if x[i] < max(x[:i])
                and c2.rows[i][0] == 0]
        assert min(late) < T.WG <= max(late)
        sc = T.scenario("m_seg", suite)
        c2 = sc.call("c2")
        per = {}
        for s, _ in c2.pkts:
            per[s] = per.get(s, 0) + 1
        assert per[sc.claims["hot"]] > T.WG and len(per) == T.NSESS
        assert sorted(per.values())[-2] == 2
        for name in ("m_rx", "m_forged", "m_ssrc", "m_ssrc_rx", "m_multi"):
            c2 = T.scenario(name, suite).call("c2")
            assert len({s for s, _ in c2.pkts}) == T.NSESS
            assert 700 <= len(c2.pkts) <= 860
        for name in ("ssrc", "ssrc_rx", "reject_host", "shortcap"):
            assert len(T.scenario(name, suite).call("c2").pkts) in \
                range(200, 204)
        for name in ("s_rx", "forged_s"):
            assert len(T.scenario(name, suite).call("c2").pkts) in \
                range(298, 304)


def test_streams_are_what_the_routes_need():
    for suite in T.SUITES:
        # one stream held, a second one appearing mid-batch
        for name in ("ssrc", "ssrc_rx"):
            sc = T.scenario(name, suite)
            assert {k for c in sc.calls[:-4] for k in c.key} == {(0, 0)}
            keys = sc.call("c2").key
            assert set(keys) == {(0, 0), (0, 1)}
            assert 40 <= keys.index((0, 1)) <= 160
        # four SSRCs held before c2
        for name in ("s_rx", "forged_s"):
            sc = T.scenario(name, suite)
            assert len({k for c in sc.calls[:-4] for k in c.key}) == 4
        # one stream per session held, ten sessions gain a second one
        for name in ("m_ssrc", "m_ssrc_rx"):
            sc = T.scenario(name, suite)
            held = {k for c in sc.calls[:-4] for k in c.key}
            assert held == {(s, 0) for s in range(T.NSESS)}
            new = set(sc.call("c2").key) - held
            assert len(new) == 10 and all(k == 1 for _, k in new)
        # two streams per session held
        sc = T.scenario("m_multi", suite)
        held = {k for c in sc.calls[:-4] for k in c.key}
        assert held == {(s, k) for s in range(T.NSESS) for k in (0, 1)}
        assert set(sc.call("c2").key) == held
        # a third of the sessions reshaped
        sc = T.scenario("m_rx", suite)
        c2 = sc.call("c2")
        x = ext_seq(c2)
        touched = set()
        for key, rows in rows_by_stream(c2).items():
            seqs = [x[i] for i, _ in rows]
            if seqs != list(range(seqs[0], seqs[0] + 6)):
                touched.add(key)
        assert len(touched) == len(range(0, T.NSESS, 3))


def test_six_and_ring():
    sc = T.six("rx", 1)
    roles = [c.role for c in sc.calls if c.role != "pre"]
    assert roles == ["c1", "c2", "c3", "c4", "c5", "c6"]
    assert len({c.set for c in sc.calls if c.role != "pre"}) == 6
    for c in sc.calls:
        assert (c.role == "c2") == any(c.errnos())
    rg = T.ring()
    assert len(rg.calls) == 140 and len(rg.sets) == 8
    assert rg.claims["reordered"] == list(range(6, 140, 7))
    for j, c in enumerate(rg.calls):
        assert len(c.pkts) == 32 and not any(c.errnos())
        x = ext_seq(c)
        assert (x != sorted(x)) == (j in rg.claims["reordered"])
    # every gate word (call j + 1 uses word (j + 1) % 64) holds a rejected
    # call's 1 and is used again afterwards
    words = {(j + 1) % 64 for j in rg.claims["reordered"] if j + 1 + 64 <= 140}
    assert len(words) >= 10
