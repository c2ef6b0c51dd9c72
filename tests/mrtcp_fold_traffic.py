"""The random SRTCP receive traffic of tests/mrtcp_rx_traffic.py with about
1 % of the arrivals forged, for the settlement pass of the many-session SRTCP
planners (plan_buckets_rtcp_fold.hip, srtp_gpu_tune mrfold).

tests/test_rtcp_seg_fold_rule.py runs it through the sequential receiver of
tests/c/rtcp_seg_fold_check.c (0 / EALREADY / EAUTH only, and every batch one
the masked rule settles: no copy beyond the look-back);
tests/test_gpu_srtcp_mfold.py sends the same batches through the library,
where every one must be settled on the device.

A forged arrival is the genuine wire packet with a tag bit flipped: it carries
the genuine packet's SSRC and index.  Every bucket of 16 sessions gets at
least one in every batch.
"""
import numpy as np

from tests import mrtcp_rx_traffic as T

BUCKET = 16             # sessions per bucket at bpexp 250, 40 sessions


def forged_batches(seed, share=0.01):
    """(start, batches) of T.random_batches(seed), each batch with a fourth
    part: forged = the set of places in `arrive` whose packet is forged"""
    start, batches = T.random_batches(seed)
    rng = np.random.default_rng(seed + 7919)
    out = []
    for sent, arrive, ndist in batches:
        forged = {i for i in range(len(arrive)) if rng.random() < share}
        sess = [batches[bb][0][i][0] for bb, i in arrive]
        for b in range((T.NSESS + BUCKET - 1) // BUCKET):
            mine = [i for i, s in enumerate(sess) if s // BUCKET == b]
            if not forged & set(mine):
                forged.add(mine[int(rng.integers(0, len(mine)))])
        out.append((sent, arrive, ndist, forged))
    return start, out


def write_traffic(path, batches):
    """the arrivals as tests/c/rtcp_seg_fold_check.c reads them"""
    with open(path, "w") as f:
        for _, arrive, _, forged in batches:
            f.write("B\n")
            for j, (bb, i) in enumerate(arrive):
                s, k, ix = batches[bb][0][i]
                f.write("%d %x %d %d\n" % (s, T.ssrc_of(s, k), ix,
                                           1 if j in forged else 0))
