/*
 * plan_rtcp_seg.h -- the SRTCP rule of plan_rule.h composed per session for
 * batches over many sessions with up to RSEG_MAX SSRCs each (stream_get,
 * stream.c:29-84; srtcp_encrypt / srtcp_decrypt, srtcp.c:31-287;
 * srtp_replay_check, replay.c:32-62).  Pure functions: they read the small
 * arrays they are handed and nothing else, no atomics.  Compiles as C
 * (tests/c/rtcp_seg_check.c runs them in the kernel's decomposition against
 * a sequential restatement) and as HIP device code (plan_buckets_rtcp.hip).
 *
 * A session's packets, ranked by their place in the batch, form its
 * segment.  Each packet looks back over the segment before it (rseg_look):
 * how many packets of its SSRC came before (its rank in its stream), where
 * the last of them is (its predecessor) and where the first is.  An SSRC
 * the session's table does not hold takes the slot behind the known ones
 * and behind the new SSRCs that appeared before it (rseg_slot); a slot past
 * the table is the reference's ENOSR (rseg_enosr) and rejects the plan.
 * With its stream's record, its rank and its predecessor's E || index word
 * the packet then is packet `rank` of a one-stream batch (rseg_packet ->
 * plan_rtcp_packet).  A stream's state after the batch: rseg_index_after
 * (sender), rseg_top / rseg_bit / rseg_window_after (receiver: the window
 * plan_win_step gives over the stream's packets in order, computed from
 * their maximum and one bit per packet, which needs no order).
 */
#ifndef PLAN_RTCP_SEG_H
#define PLAN_RTCP_SEG_H

#include "plan_rule.h"

#define RSEG_MAX 8u             /* SRTP_MAX_STREAMS (stream.c:16-17) */
#define RSEG_NONE 0xffu         /* no slot */

/* a stream of a session's table as the planner sees it: ix is rtcp_index
 * (protect) or the window's lix (unprotect, HMAC suites), blo / bhi the
 * window's bitmap; a new stream is its SSRC and zeros (stream.c:45-67) */
struct rseg_rec {
	uint32_t ssrc, ix, blo, bhi;
};

/* slot of ssrc among the nk streams the session had before the batch */
PLAN_FN uint32_t rseg_known(const struct rseg_rec *tab, uint32_t nk,
			    uint32_t ssrc)
{
	uint32_t q;
	for (q = 0; q < nk && q < RSEG_MAX; q++)
		if (tab[q].ssrc == ssrc)
			return q;
	return RSEG_NONE;
}

/* what the segment before sorted position k tells the packet there */
struct rseg_look {
	uint32_t rank;          /* packets of its SSRC before it */
	uint32_t prev;          /* position of the last of them (rank > 0) */
	uint32_t first;         /* position of the first (k itself if none) */
};

PLAN_FN struct rseg_look rseg_look_init(uint32_t k)
{
	struct rseg_look a;
	a.rank = 0;
	a.prev = k;
	a.first = k;
	return a;
}

/* position t < k (visited in increasing order) carries the same SSRC */
PLAN_FN struct rseg_look rseg_look_step(struct rseg_look a, uint32_t t,
					int same)
{
	if (same) {
		if (!a.rank)
			a.first = t;
		a.rank++;
		a.prev = t;
	}
	return a;
}

/* the packet at a position opens a new stream: its SSRC is not in the table
 * and no packet before it carries it */
PLAN_FN int rseg_opens(uint32_t known, struct rseg_look a)
{
	return known == RSEG_NONE && a.rank == 0;
}

/* the packet's slot: nnew = the streams opened in the segment before the
 * position where the packet's SSRC first appears (a.first) */
PLAN_FN uint32_t rseg_slot(uint32_t known, uint32_t nk, uint32_t nnew)
{
	return known != RSEG_NONE ? known : nk + nnew;
}

/* stream_get's ENOSR: the table is full */
PLAN_FN int rseg_enosr(uint32_t slot)
{
	return slot >= RSEG_MAX;
}

/*
 * The packet as packet `rank` of its stream's one-stream batch.  c: what
 * the whole batch shares (prot, tag, gcm, hmac, encrypted, need, maxlen);
 * st: its stream's record; word / pword: the E || index word of it and of
 * its predecessor in the stream (rank > 0); parsed, L, wflags as
 * plan_rtcp_packet.
 */
PLAN_FN struct plan_rtcp rseg_packet(struct sgpu_rplan_in c,
				     struct rseg_rec st, uint32_t rank,
				     int parsed, uint32_t L, uint32_t wflags,
				     uint32_t word, uint32_t pword)
{
	c.rtcp_index = st.ix;
	c.lix = st.ix;
	c.bitmap = (uint64_t)st.bhi << 32 | st.blo;
	return plan_rtcp_packet(c, rank, parsed, st.ssrc, st.ssrc, L, wflags,
				word, pword);
}

/* sender: rtcp_index after cnt packets (srtcp.c:54) */
PLAN_FN uint32_t rseg_index_after(uint32_t rtcp_index, uint32_t cnt)
{
	return (rtcp_index + cnt) & 0x7fffffffu;
}

/* receiver: the window's lix after the batch, top = the largest index of
 * the stream's packets */
PLAN_FN uint32_t rseg_top(uint32_t lix0, uint32_t top)
{
	return top > lix0 ? top : lix0;
}

/* ... the bit an accepted index leaves in the window that ends at lix1 */
PLAN_FN uint64_t rseg_bit(uint32_t lix1, uint32_t ix)
{
	return lix1 - ix < 64u ? 1ull << (lix1 - ix) : 0ull;
}

/* ... and the window: the old bits moved up, the packets' bits */
PLAN_FN struct plan_win rseg_window_after(struct rseg_rec st, uint32_t lix1,
					  uint64_t bits)
{
	struct plan_win w;
	const uint32_t d = lix1 - st.ix;
	const uint64_t b0 = (uint64_t)st.bhi << 32 | st.blo;
	w.lix = lix1;
	w.bitmap = (d < 64u ? b0 << d : 0ull) | bits;
	return w;
}

#endif
