"""Random receive traffic for the reordered one-session multi-SSRC planner
(plan_streams_rx.hip): one session of 3-8 SSRCs whose streams arrive with
swaps, loss and duplicates at a few percent, two batches one after the other.

tests/test_streams_rx_rule.py runs it through the sequential receiver of
tests/c/streams_rx_check.c (only 0 / EALREADY, every batch disturbed, every
batch one the rule settles); tests/test_gpu_srxplan.py sends the same batches
through the library, where every one must be accepted by the planner.

A displacement is at most 8 arrivals of the packet's own stream, and no
disturbed packet lies within 12 sequence numbers of a rollover: a late packet
from the far side of a rollover is the reference's ETIMEDOUT, which no device
planner settles.  The last stream sends nothing in the first batch, so the
second one opens a stream behind known ones.
"""
import numpy as np

KEEP_OFF = 12           # seqs next to a multiple of 65536 left undisturbed
SEEDS = (811, 812)


def ssrc_of(k):
    return 0x56000000 | k


def _calm(ext):
    return KEEP_OFF <= ext % 65536 < 65536 - KEEP_OFF


def random_batches(seed, nbatch=2, n=1300, limit=1400):
    """[(sent, arrive, ndist)] per batch: sent = [(k, seq)] in the senders'
    order, every stream in order; arrive = indices into sent in arrival order
    (a lost packet is missing, a duplicate twice); ndist = the disturbances
    made.  Streams start 25-60 below 65536, each at its own place, so every
    one rolls over inside some batch."""
    rng = np.random.default_rng(seed)
    nss = 3 + int(rng.integers(0, 6))
    nxt = [65536 - 25 - int(rng.integers(0, 36)) for _ in range(nss)]
    out = []
    for b in range(nbatch):
        live = nss - 1 if b == 0 else nss
        who = list(range(live)) * 2
        who += rng.integers(0, live, n - len(who)).tolist()
        who = [who[i] for i in rng.permutation(len(who)).tolist()]
        sent, ext = [], []
        for k in who:
            sent.append((k, nxt[k] & 0xffff))
            ext.append(nxt[k])
            nxt[k] += 1
        # per stream: the places of its arrivals in the batch
        places = {}
        for i, (k, _) in enumerate(sent):
            places.setdefault(k, []).append(i)
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
    """the arrivals as tests/c/streams_rx_check.c reads them"""
    with open(path, "w") as f:
        for sent, arrive, _ in batches:
            f.write("B\n")
            for i in arrive:
                k, seq = sent[i]
                f.write("%x %d\n" % (ssrc_of(k), seq))
