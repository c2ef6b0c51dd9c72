/*
 * plan_rtcp_str.h -- how the one-session SRTCP planner (plan_streams_rtcp.hip)
 * composes the rules of plan_rtcp_seg.h and plan_rtcp_seg_rx.h over a session
 * that spans the grid: the packets are partitioned stably by stream slot, so a
 * stream's packets in batch order are one run of places [start, start + cnt).
 * What is stated here is only that composition -- which record a slot has
 * before the batch, which slot a place belongs to, where a packet lands and
 * which packet of its stream it then is; every check, index, verdict and
 * window is the other headers'.  Pure functions over the small arrays they
 * are handed.  Compiles as C (tests/c/rtcp_str_check.c runs them in the
 * kernels' decomposition against a sequential sender and receiver) and as HIP
 * device code.
 */
#ifndef PLAN_RTCP_STR_H
#define PLAN_RTCP_STR_H

#include "plan_rtcp_seg_rx.h"

/* slot q of the table after the batch as the rule sees it before the batch:
 * the session's record `known` (q < nk), or a stream the batch opens with the
 * SSRC the table launches found for it (stream.c:45-67) */
PLAN_FN struct rseg_rec rstr_rec(struct rseg_rec known, uint32_t q, uint32_t nk,
				 uint32_t ssrc)
{
	return q < nk && q < RSEG_MAX ? known : rsrx_new(ssrc);
}

/* the slot of an SSRC in the table after the batch (RSEG_NONE: a 9th) */
PLAN_FN uint32_t rstr_slot(const uint32_t *ssrcs, uint32_t nt, uint32_t ssrc)
{
	return rsrx_known(ssrcs, nt, ssrc);
}

/* the slots' runs of places, one behind the other, from their counts */
PLAN_FN void rstr_starts(const uint32_t *cnt, uint32_t *start)
{
	uint32_t q;
	for (q = 0; q < RSEG_MAX; q++)
		start[q] = rsrx_first(0, cnt, q);
}

/* where a packet lands: its slot's run starts at start, `before` packets of
 * the slot lie in the workgroups before its own and `ahead` in front of it in
 * its own workgroup */
PLAN_FN uint32_t rstr_place(uint32_t start, uint32_t before, uint32_t ahead)
{
	return start + before + ahead;
}

/* the slot whose run holds place p (RSEG_NONE: none) */
PLAN_FN uint32_t rstr_slot_at(const uint32_t *start, const uint32_t *cnt,
			      uint32_t p)
{
	uint32_t q, k = RSEG_NONE;
	for (q = 0; q < RSEG_MAX; q++)
		if (p >= start[q] && p - start[q] < cnt[q])
			k = q;
	return k;
}

/* the packet at a place is packet `rank` of its stream (rseg_packet's rank,
 * rsrx_verdict's position) */
PLAN_FN uint32_t rstr_rank(uint32_t place, uint32_t start)
{
	return place - start;
}

/* a place is its stream's first arrival: the scan's segment head */
PLAN_FN int rstr_head(uint32_t place, uint32_t start)
{
	return place == start;
}

/* sender: the packet's index, E and checks as packet `rank` of its stream */
PLAN_FN struct plan_rtcp rstr_tx(struct sgpu_rplan_in c, struct rseg_rec st,
				 uint32_t place, uint32_t start, int parsed,
				 uint32_t L, uint32_t wflags)
{
	return rseg_packet(c, st, rstr_rank(place, start), parsed, L, wflags, 0,
			   0);
}

/* sender: a touched stream's record after its cnt packets */
PLAN_FN struct rseg_rec rstr_tx_after(struct rseg_rec st, uint32_t cnt)
{
	st.ix = rseg_index_after(st.ix, cnt);
	return st;
}

/* every check of the packet but the receiver's replay one, its window's
 * (wflags) included; none of them depends on the packet's rank */
PLAN_FN uint32_t rstr_flags(struct sgpu_rplan_in c, uint32_t ssrc, int parsed,
			    uint32_t L, uint32_t wflags, uint32_t word)
{
	return wflags | rsrx_flags(c, rsrx_new(ssrc), parsed, L, word);
}

/* receiver: the largest index of the stream whose arrivals lie at
 * [start, start + cnt), cnt != 0 */
PLAN_FN uint32_t rstr_smx(const int64_t *u, const int64_t *mx, uint32_t start,
			  uint32_t cnt)
{
	return rsrx_smx(u[start + cnt - 1], mx[start + cnt - 1]);
}

#endif
