"""Random SRTCP receive traffic for the many-session receive planner
(plan_buckets_rtcp_rx.hip): 40 sessions of 2-3 SSRCs whose streams arrive with
swaps, loss, duplicates and replays of the batch before at a few percent.

tests/test_rtcp_seg_rx_rule.py runs it through the sequential receiver of
tests/c/rtcp_seg_rx_check.c (only 0 / EALREADY, every batch disturbed and one
the rule settles); tests/test_gpu_srtcp_mrxplan.py sends the same batches
through the library, where every one must be accepted by the planner.

A displacement is at most 8 arrivals of the packet's own stream and no stream
has more than 100 arrivals in a batch, fewer than the planner's look-back of
128: no verdict can hang on a copy older than that.  Four streams start just
below 0x7fffffff and wrap inside the batches: the indices behind the wrap are
old to the reference.
"""
import numpy as np

NSESS = 40
HOT = 64                # extra packets of session 0: a segment across waves
WRAP = {(5, 1): 0x7fffffff - 7, (17, 0): 0x7fffffff - 30,
        (33, 1): 0x7fffffff - 2, (39, 0): 0x7fffffff - 15}


def ssrc_of(s, k):
    return 0x51000000 | (s << 8) | k


def random_batches(seed, nsess=NSESS, nbatch=3, n=500, limit=600):
    """(start, batches).  start = {(session, k): the stream's first index}
    (1 unless it is in WRAP).  batches = [(sent, arrive, ndist)]: sent =
    [(session, k, index)] in the senders' order, every stream in order; arrive
    = [(batch, i)] in arrival order, naming sent[i] of that batch (a lost
    packet is missing, a duplicate twice, a replay names the batch before);
    ndist = the disturbances made."""
    rng = np.random.default_rng(seed)
    nss = [2 + int(rng.integers(0, 2)) for _ in range(nsess)]
    start = {(s, k): WRAP.get((s, k), 1)
             for s in range(nsess) for k in range(nss[s])}
    nxt = dict(start)
    out = []
    arrived = {}                        # stream -> [(batch, i)] of the batch before
    for b in range(nbatch):
        who = [(s, k) for s in range(nsess) for k in range(nss[s])] * 2
        who += [(0, int(rng.integers(0, nss[0]))) for _ in range(HOT)]
        who += [(s, int(rng.integers(0, nss[s])))
                for s in rng.integers(0, nsess, n - len(who)).tolist()]
        who = [who[i] for i in rng.permutation(len(who)).tolist()]
        sent = []
        for s, k in who:
            sent.append((s, k, nxt[(s, k)] & 0x7fffffff))
            nxt[(s, k)] += 1
        places = {}
        for i, (s, k, _) in enumerate(sent):
            places.setdefault((s, k), []).append(i)
        assert max(len(a) for a in places.values()) <= 100
        slot = [(b, i) for i in range(len(sent))]   # place -> arrival, or None
        extra = []                                  # (after place, arrival)
        ndist = 0
        for key in sorted(places):
            a = places[key]
            j = 0
            while j < len(a):
                r = rng.random()
                d = 1 if rng.random() < 0.6 else int(rng.integers(2, 9))
                span = a[j:j + d + 1]
                ok = len(span) == d + 1 and \
                    all(slot[q] == (b, q) for q in span)
                room = len(sent) + len(extra) < limit
                if r < 0.03 and ok:             # swap, d apart
                    slot[a[j]], slot[a[j + d]] = slot[a[j + d]], slot[a[j]]
                    ndist += 1
                    j += d + 1
                    continue
                if r < 0.04 and slot[a[j]] == (b, a[j]):
                    slot[a[j]] = None           # loss
                    ndist += 1
                elif r < 0.07 and ok and room:
                    extra.append((a[j + d], (b, a[j])))     # duplicate, d later
                    ndist += 1
                elif r < 0.09 and room and arrived.get(key):
                    old = arrived[key]          # replay of the batch before
                    extra.append((a[j], old[int(rng.integers(0, len(old)))]))
                    ndist += 1
                j += 1
        after = {}
        for place, arr in extra:
            after.setdefault(place, []).append(arr)
        arrive = []
        for place, arr in enumerate(slot):
            if arr is not None:
                arrive.append(arr)
            arrive += after.get(place, [])
        assert len(arrive) <= limit
        arrived = {}
        for bb, i in arrive:
            if bb == b:
                arrived.setdefault(sent[i][:2], []).append((bb, i))
        out.append((sent, arrive, ndist))
    return start, out


def write_traffic(path, batches):
    """the arrivals as tests/c/rtcp_seg_rx_check.c reads them"""
    with open(path, "w") as f:
        for sent, arrive, _ in batches:
            f.write("B\n")
            for bb, i in arrive:
                s, k, ix = batches[bb][0][i]
                f.write("%d %x %d\n" % (s, ssrc_of(s, k), ix))
