/*
 * plan_rtp_seg.h -- the in-order RTP rule of plan_rule.h composed per
 * (session, SSRC) for batches over many sessions with up to RSEG_MAX SSRCs
 * each (stream_get_seq, stream.c:29-109; srtp_encrypt / srtp_decrypt,
 * srtp.c:183-432; srtp_get_index, misc.c:22-41; srtp_replay_check,
 * replay.c:32-62).  Pure functions over plan_rule.h and plan_rtcp_seg.h: no
 * memory access but the small table they are handed, no atomics.  Compiles
 * as C (tests/c/rtp_seg_check.c runs them in the kernel's decomposition
 * against a sequential sender / receiver) and as HIP device code
 * (plan_buckets_rtp_streams.hip).
 *
 * A session's packets, ranked by their place in the batch, form its
 * segment, and a packet finds its stream slot exactly as an SRTCP packet
 * does (rseg_known, rseg_look_*, rseg_opens, rseg_slot, rseg_enosr).  The
 * same look back over the segment carries what the one-stream rule needs
 * (tseg_look_step): the seq of the stream's packet before it, the s_l that
 * one saw, and the stream's rollovers so far (plan_wrap) -- each packet of a
 * stream speculates s_l = its predecessor's seq, the first one the stored
 * s_l, or its own seq where s_l is not set (a new stream, or one SRTCP
 * created).  tseg_packet then is the rule k_bp_plan applies per session:
 * plan_order (the predecessor must have left s_l as assumed; ETIMEDOUT),
 * plan_index under the stream's ROC, plan_new_first / plan_new_later against
 * the stream's stored window.  A stream's state after the batch is its last
 * packet's (tseg_after): roc, s_l (plan_s_l_after) and the window's top; the
 * window is the old bits moved up plus one bit per packet within 64 of the
 * top (tseg_bit, tseg_window_after), which needs no order.
 */
#ifndef PLAN_RTP_SEG_H
#define PLAN_RTP_SEG_H

#include "plan_rtcp_seg.h"

#define TSEG_SL_SET 0x10000u    /* tseg_rec.sl: s_l_set */

/* a stream of a session's table as the planner sees it (srtpgpu.h struct
 * sgpu_rtp_rec): sl = s_l | s_l_set << 16, llo / lhi the RTP window's 48-bit
 * lix, blo / bhi its bitmap; a new stream is its SSRC and zeros
 * (stream.c:45-67) */
struct tseg_rec {
	uint32_t ssrc, roc, sl, pad;
	uint32_t llo, lhi, blo, bhi;
};

PLAN_FN uint64_t tseg_lix(struct tseg_rec st)
{
	return (uint64_t)st.lhi << 32 | st.llo;
}

PLAN_FN uint64_t tseg_bitmap(struct tseg_rec st)
{
	return (uint64_t)st.bhi << 32 | st.blo;
}

/* slot of ssrc among the nk streams the session had before the batch
 * (rseg_known over the RTP records) */
PLAN_FN uint32_t tseg_known(const struct tseg_rec *tab, uint32_t nk,
			    uint32_t ssrc)
{
	uint32_t q;
	for (q = 0; q < nk && q < RSEG_MAX; q++)
		if (tab[q].ssrc == ssrc)
			return q;
	return RSEG_NONE;
}

/* the s_l the first packet (seq) of a stream's segment sees
 * (stream_get_seq, stream.c:87-109) */
PLAN_FN uint32_t tseg_sl0(uint32_t sl, uint32_t seq)
{
	return (sl & TSEG_SL_SET) ? (sl & 0xffffu) : seq;
}

/* what the segment before sorted position k tells the packet there */
struct tseg_look {
	struct rseg_look a;     /* rank in its stream, predecessor, first */
	uint32_t wraps;         /* rollovers of the stream's packets before it */
	uint32_t pseq;          /* the predecessor's seq (rank > 0) */
	uint32_t psb;           /* ... and the s_l it saw */
};

PLAN_FN struct tseg_look tseg_look_init(uint32_t k)
{
	struct tseg_look a;
	a.a = rseg_look_init(k);
	a.wraps = 0;
	a.pseq = 0;
	a.psb = 0;
	return a;
}

/* position t < k (visited in increasing order) with seq tseq; same: it
 * carries the packet's SSRC; sl: the stream's stored s_l word (0 for a
 * stream the table does not hold) */
PLAN_FN struct tseg_look tseg_look_step(struct tseg_look a, uint32_t t,
					int same, uint32_t tseq, uint32_t sl)
{
	if (same) {
		const uint32_t sb = a.a.rank ? a.pseq : tseg_sl0(sl, tseq);
		a.wraps += (uint32_t)plan_wrap(tseq, sb);
		a.psb = sb;
		a.pseq = tseq;
	}
	a.a = rseg_look_step(a.a, t, same);
	return a;
}

struct tseg_pkt {
	uint32_t flags;         /* SPF_ORDER | SPF_TIMEOUT | SPF_REPLAY */
	uint32_t fl;            /* desc flags (SD_*) */
	uint64_t ix;            /* the packet's 48-bit index */
	uint32_t roc, s_l;      /* its stream after it, were it the last */
};

/*
 * The packet (seq) as packet a.a.rank of its stream's one-stream batch; st:
 * the stream's record before the batch.
 */
PLAN_FN struct tseg_pkt tseg_packet(int prot, struct tseg_rec st,
				    struct tseg_look a, uint32_t seq)
{
	struct tseg_pkt r;
	const uint32_t sb = a.a.rank ? a.pseq : tseg_sl0(st.sl, seq);
	/* ETIMEDOUT is the packet's own; whether it leaves s_l as the next
	 * one assumes is checked by that one, so the stream's last packet is
	 * never asked (plan_order's `last`) */
	const struct plan_ord o = plan_order(seq, sb, 1, prot);
	const uint32_t roc = st.roc + a.wraps + o.wrap;
	const struct plan_idx x = plan_index(roc, (int)o.wrap, sb, seq, prot);
	r.flags = o.flags;
	if (a.a.rank)
		r.flags |= plan_order(a.pseq, a.psb, 0, prot).flags & SPF_ORDER;
	if (!prot) {
		const uint64_t lix = tseg_lix(st);
		const int ok = a.a.rank == 0 ?
			plan_new_first(x.ix, lix, tseg_bitmap(st)) :
			plan_new_later(x.ix, plan_prev_index(roc, (int)o.wrap,
							     a.psb, a.pseq), lix);
		if (!ok)
			r.flags |= SPF_REPLAY;
	}
	r.fl = x.fl;
	r.ix = x.ix;
	r.roc = roc;
	r.s_l = plan_s_l_after(seq, sb, (int)o.wrap);
	return r;
}

/* receiver: the window's top after the batch, last = the index of the
 * stream's last packet (the largest: every index is new and increasing) */
PLAN_FN uint64_t tseg_top(uint64_t lix0, uint64_t last)
{
	return last > lix0 ? last : lix0;
}

/* ... the bit an accepted index leaves in the window that ends at top */
PLAN_FN uint64_t tseg_bit(uint64_t top, uint64_t ix)
{
	return top - ix < 64u ? 1ull << (top - ix) : 0ull;
}

/* the stream's record after the batch: p its last packet's tseg_pkt; bits
 * the OR of its packets' tseg_bit (receiver; a sender's window stays) */
PLAN_FN struct tseg_rec tseg_after(int prot, struct tseg_rec st,
				   struct tseg_pkt p, uint64_t bits)
{
	st.roc = p.roc;
	st.sl = (p.s_l & 0xffffu) | TSEG_SL_SET;
	if (!prot) {
		const uint64_t lix0 = tseg_lix(st), top = tseg_top(lix0, p.ix);
		const uint64_t d = top - lix0;
		const uint64_t bm = (d < 64u ? tseg_bitmap(st) << d : 0ull) | bits;
		st.llo = (uint32_t)top;
		st.lhi = (uint32_t)(top >> 32);
		st.blo = (uint32_t)bm;
		st.bhi = (uint32_t)(bm >> 32);
	}
	return st;
}

#endif
