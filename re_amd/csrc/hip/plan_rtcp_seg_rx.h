/*
 * plan_rtcp_seg_rx.h -- the exact SRTCP receive rule per (session, SSRC) for
 * unprotect batches over many sessions with up to RSEG_MAX SSRCs each whose
 * packets arrive reordered, duplicated or replayed inside their streams
 * (stream_get, stream.c:29-84; srtcp_decrypt, srtcp.c:143-287;
 * srtp_replay_check, replay.c:32-62), HMAC suites (GCM keeps no SRTCP replay
 * window).  Pure functions over plan_rtcp_seg.h and plan_rx_rule.h: no memory
 * access beyond the arrays they are handed, no atomics, none of their rules
 * said again.  Compiles as C (tests/c/rtcp_seg_rx_check.c runs them in the
 * kernel's decomposition against a sequential receiver) and as HIP device
 * code (plan_buckets_rtcp_rx.hip).
 *
 * A packet finds its stream slot as in plan_rtcp_seg.h (rseg_known,
 * rseg_look_*, rseg_opens, rseg_slot, rseg_enosr).  The look back's rank is
 * its place among its stream's arrivals, so the streams of a session lie one
 * behind the other at rsrx_first and a stream's arrivals in batch order are
 * one segment of plan_rx_rule.h's (sum, max) scan.  The index travels in the
 * packet (E || index, srtcp.c:173-178), so nothing is speculated: the scan's
 * elements are the differences of consecutive indices, its sums u[] the
 * indices themselves and mx[] their exclusive prefix maxima.  The reference
 * checks the tag first and the window second (srtcp.c:187-209), a rejected
 * packet never lies above the window's top, and so the top before arrival i
 * is max(lix0, mx[i]) whatever the verdicts before it were: rx_replay with
 * tagged = 1 is the whole rule.  RX_UNSETTLED (a possible copy older than the
 * look-back) rejects the plan.  Every other check is plan_rtcp_packet's
 * (rsrx_flags); a touched stream's window after the batch is plan_rtcp_seg.h's
 * (rsrx_after).
 */
#ifndef PLAN_RTCP_SEG_RX_H
#define PLAN_RTCP_SEG_RX_H

#include "plan_rtcp_seg.h"
#include "plan_rx_rule.h"

/* a stream the table does not hold yet (stream.c:45-67) */
PLAN_FN struct rseg_rec rsrx_new(uint32_t ssrc)
{
	struct rseg_rec r;
	r.ssrc = ssrc;
	r.ix = r.blo = r.bhi = 0;
	return r;
}

/* rseg_known where only the table's SSRCs are at hand */
PLAN_FN uint32_t rsrx_known(const uint32_t *ssrcs, uint32_t nk, uint32_t ssrc)
{
	uint32_t q;
	for (q = 0; q < nk && q < RSEG_MAX; q++)
		if (ssrcs[q] == ssrc)
			return q;
	return RSEG_NONE;
}

/* where a stream's first arrival lies (arrival `rank`: that many behind it):
 * its session's segment starts at start, count[] are the arrivals of the
 * session's slots */
PLAN_FN uint32_t rsrx_first(uint32_t start, const uint32_t *count,
			    uint32_t slot)
{
	uint32_t q;
	for (q = 0; q < slot && q < RSEG_MAX; q++)
		start += count[q];
	return start;
}

/* the window before the batch */
PLAN_FN int64_t rsrx_lix0(struct rseg_rec st)
{
	return (int64_t)st.ix;
}

PLAN_FN uint64_t rsrx_bitmap0(struct rseg_rec st)
{
	return (uint64_t)st.bhi << 32 | st.blo;
}

/* the scan element of a stream's arrival: the first one carries its index,
 * the others their distance to the arrival before (pword) */
PLAN_FN int64_t rsrx_elem(int head, uint32_t word, uint32_t pword)
{
	const int64_t ix = (int64_t)(word & 0x7fffffffu);
	return head ? ix : ix - (int64_t)(pword & 0x7fffffffu);
}

/* every check of plan_rtcp_packet but the replay one, which the in-order
 * speculation there answers for a batch this planner is not given: the
 * packet as the first of a stream with an empty window */
PLAN_FN uint32_t rsrx_flags(struct sgpu_rplan_in c, struct rseg_rec st,
			    int parsed, uint32_t L, uint32_t word)
{
	st.ix = st.blo = st.bhi = 0;
	return rseg_packet(c, st, 0, parsed, L, 0, word, 0).flags &
	       ~(uint32_t)SPF_REPLAY;
}

/* verdict of arrival i of a stream (RX_OK / RX_DUP / RX_UNSETTLED): u[] its
 * arrivals' indices, mx[] their exclusive prefix maxima, K the look-back */
PLAN_FN int rsrx_verdict(const int64_t *u, const int64_t *mx, uint32_t i,
			 uint32_t K, struct rseg_rec st)
{
	return rx_replay(u, mx, i, K, rsrx_lix0(st), rsrx_bitmap0(st), 1);
}

/* desc word of a settled packet: an EALREADY packet's tag is still checked
 * over its own trailer bytes, and nothing of it is deciphered (E clear) */
PLAN_FN uint64_t rsrx_desc(int verdict, uint32_t word)
{
	return plan_rtcp_desc(word & 0x7fffffffu,
			      verdict == RX_DUP ? 0u : word >> 31);
}

/* an accepted packet below its window's top at its arrival */
PLAN_FN int rsrx_late(int64_t ui, struct rseg_rec st, int64_t mxi)
{
	return ui < rx_max(rsrx_lix0(st), mxi);
}

/* the maximum of a stream's indices from its last arrival's u and mx */
PLAN_FN uint32_t rsrx_smx(int64_t ulast, int64_t mxlast)
{
	return (uint32_t)rx_max(ulast, mxlast);
}

/* an accepted packet's bit in the window after the batch */
PLAN_FN uint64_t rsrx_bit(struct rseg_rec st, uint32_t smx, int64_t ui)
{
	return rseg_bit(rseg_top(st.ix, smx), (uint32_t)ui);
}

/* a touched stream's record after the batch: smx the maximum of its indices,
 * bits the OR of its accepted packets' rsrx_bit */
PLAN_FN struct rseg_rec rsrx_after(struct rseg_rec st, uint32_t smx,
				   uint64_t bits)
{
	const struct plan_win w =
		rseg_window_after(st, rseg_top(st.ix, smx), bits);
	st.ix = (uint32_t)w.lix;
	st.blo = (uint32_t)w.bitmap;
	st.bhi = (uint32_t)(w.bitmap >> 32);
	return st;
}

#endif
