"""Random receive traffic for the reordered multi-SSRC planner
(plan_buckets_rtp_streams_rx.hip): many sessions of 2-3 SSRCs whose streams
arrive with swaps, loss and duplicates at a few percent.

tests/test_rtp_seg_rx_rule.py runs it through the sequential receiver of
tests/c/rtp_seg_rx_check.c (only 0 / EALREADY, every batch one the rule
settles); tests/test_gpu_msrxplan.py sends the same batches through the
library, where every one must be accepted by the planner.

A displacement is at most 8 arrivals of the packet's own stream, and no
disturbed packet lies within 12 sequence numbers of a rollover: a late packet
from the far side of a rollover is the reference's ETIMEDOUT, which no device
planner settles.
"""
import numpy as np

NSESS = 40
KEEP_OFF = 12           # seqs next to a multiple of 65536 left undisturbed


def ssrc_of(s, k):
    return 0x55000000 | (s << 8) | k


def _calm(ext):
    return KEEP_OFF <= ext % 65536 < 65536 - KEEP_OFF


def random_batches(seed, nsess=NSESS, nbatch=3, n=540, limit=600):
    """[(sent, arrive, ndist)] per batch: sent = [(session, k, seq)] in the
    senders' order, every stream in order; arrive = indices into sent in
    arrival order (a lost packet is missing, a duplicate twice); ndist = the
    disturbances made.  Streams start 25-60 below 65536, each at its own
    place, so every one rolls over inside some batch."""
    rng = np.random.default_rng(seed)
    nss = [2 + int(rng.integers(0, 2)) for _ in range(nsess)]
    nxt = {(s, k): 65536 - 25 - int(rng.integers(0, 36))
           for s in range(nsess) for k in range(nss[s])}
    out = []
    for _ in range(nbatch):
        who = [(s, k) for s in range(nsess) for k in range(nss[s])] * 2
        who += [(s, int(rng.integers(0, nss[s])))
                for s in rng.integers(0, nsess, n - len(who)).tolist()]
        who = [who[i] for i in rng.permutation(len(who)).tolist()]
        sent, ext = [], []
        for s, k in who:
            sent.append((s, k, nxt[(s, k)] & 0xffff))
            ext.append(nxt[(s, k)])
            nxt[(s, k)] += 1
        # per stream: the places of its arrivals in the batch
        places = {}
        for i, (s, k, _) in enumerate(sent):
            places.setdefault((s, k), []).append(i)
        slot = list(range(len(sent)))   # place -> index into sent, or None
        extra = []                      # (after place, index into sent)
        ndist = 0
        for key in sorted(places):
            a = places[key]
            j = 0
            while j < len(a):
                r = rng.random()
                d = 1 if rng.random() < 0.6 else int(rng.integers(2, 9))
                span = a[j:j + d + 1]
                ok = len(span) == d + 1 and \
                    all(slot[q] == q and _calm(ext[q]) for q in span)
                if r < 0.03 and ok:             # swap, d apart
                    slot[a[j]], slot[a[j + d]] = a[j + d], a[j]
                    ndist += 1
                    j += d + 1
                    continue
                if r < 0.05 and _calm(ext[a[j]]) and slot[a[j]] == a[j]:
                    slot[a[j]] = None           # loss
                    ndist += 1
                elif r < 0.07 and ok and len(sent) + len(extra) < limit:
                    extra.append((a[j + d], a[j]))      # duplicate, d later
                    ndist += 1
                j += 1
        after = {}
        for place, i in extra:
            after.setdefault(place, []).append(i)
        arrive = []
        for place, i in enumerate(slot):
            if i is not None:
                arrive.append(i)
            arrive += after.get(place, [])
        out.append((sent, arrive, ndist))
    return out


def write_traffic(path, batches):
    """the arrivals as tests/c/rtp_seg_rx_check.c reads them"""
    with open(path, "w") as f:
        for sent, arrive, _ in batches:
            f.write("B\n")
            for i in arrive:
                s, k, seq = sent[i]
                f.write("%d %x %d\n" % (s, ssrc_of(s, k), seq))
