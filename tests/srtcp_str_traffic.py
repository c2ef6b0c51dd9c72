"""Random SRTCP receive traffic for the one-session planner
(plan_streams_rtcp.hip): one session of 2-7 SSRCs whose streams arrive
interleaved, with swaps, loss, duplicates and replays of the batch before at a
few percent; the second batch opens one more stream behind the known ones.

tests/test_rtcp_str_rule.py runs it through the sequential receiver of
tests/c/rtcp_str_check.c (only 0 / EALREADY, every batch disturbed and one the
rule settles at the kernels' own widths); tests/test_gpu_srtcp_splan.py sends
the same batches through the library, where every one must be taken by the
planner.

A displacement is at most 8 arrivals of the packet's own stream, far inside
the planner's look-back of 128 arrivals, so no verdict can hang on a copy older
than that although the busiest stream has more arrivals than the look-back.  A
batch has more than 512 arrivals: three workgroups.  One stream per seed
starts just below 0x7fffffff and wraps: the indices behind the wrap are old to
the reference.
"""
import numpy as np

SEEDS = (811, 812, 813)
LIMIT = 600


def ssrc_of(k):
    return 0x51000000 | k


def random_batches(seed, nbatch=2, n=540, limit=LIMIT):
    """(start, batches).  start = {k: the stream's first index}.  batches =
    [(sent, arrive, ndist)]: sent = [(k, index)] in the sender's order, every
    stream in order; arrive = [(batch, i)] in arrival order, naming sent[i] of
    that batch (a lost packet is missing, a duplicate twice, a replay names
    the batch before); ndist = the disturbances made."""
    rng = np.random.default_rng(seed)
    nss = 2 + int(rng.integers(0, 5))           # 2..6, one more in batch 1
    start = {k: 1 + int(rng.integers(0, 3000)) for k in range(nss + 1)}
    start[int(rng.integers(0, nss))] = 0x7fffffff - int(rng.integers(5, 40))
    nxt = dict(start)
    out = []
    arrived = {}                        # stream -> [(batch, i)] of the batch before
    for b in range(nbatch):
        ks = list(range(nss + (1 if b else 0)))
        # stream 0 is busy: more arrivals than the look-back
        who = ks * 2 + [0] * 200
        who += [ks[i] for i in rng.integers(0, len(ks), n - len(who)).tolist()]
        who = [who[i] for i in rng.permutation(len(who)).tolist()]
        if b:
            # the new stream first appears mid-batch
            new = [i for i, k in enumerate(who) if k == nss]
            who = [k for k in who if k != nss]
            for i in new:
                who.insert(int(rng.integers(len(who) // 2, len(who) + 1)), nss)
        sent = []
        for k in who:
            sent.append((k, nxt[k] & 0x7fffffff))
            nxt[k] += 1
        places = {}
        for i, (k, _) in enumerate(sent):
            places.setdefault(k, []).append(i)
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
        assert 512 < len(arrive) <= limit
        arrived = {}
        for bb, i in arrive:
            if bb == b:
                arrived.setdefault(sent[i][0], []).append((bb, i))
        out.append((sent, arrive, ndist))
    return start, out


def write_traffic(path, batches):
    """the arrivals as tests/c/rtcp_str_check.c reads them"""
    with open(path, "w") as f:
        for sent, arrive, _ in batches:
            f.write("B\n")
            for bb, i in arrive:
                k, ix = batches[bb][0][i]
                f.write("%x %d\n" % (ssrc_of(k), ix))
