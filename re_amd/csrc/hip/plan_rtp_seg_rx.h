/*
 * plan_rtp_seg_rx.h -- the exact receive rule of plan_rx_rule.h composed per
 * (session, SSRC) for unprotect batches over many sessions with up to
 * RSEG_MAX SSRCs each whose packets arrive reordered, duplicated or with gaps
 * inside their streams (stream_get_seq, stream.c:29-109; srtp_decrypt,
 * srtp.c:313-432; srtp_get_index, misc.c:22-41; srtp_replay_check,
 * replay.c:32-62).  Pure functions over plan_rtcp_seg.h, plan_rtp_seg.h and
 * plan_rx_rule.h: no memory access, no atomics, none of their rules said
 * again.  Compiles as C (tests/c/rtp_seg_rx_check.c runs them in the kernel's
 * decomposition against a sequential receiver) and as HIP device code
 * (plan_buckets_rtp_streams_rx.hip).
 *
 * A packet finds its stream slot as in plan_rtp_seg.h (rseg_known over the
 * table's SSRCs, rseg_look_*, rseg_opens, rseg_slot, rseg_enosr): a new SSRC
 * opens a slot at its first arrival in batch order.  The look back's rank is
 * the packet's place among its stream's arrivals, so the streams of a session
 * lie one behind the other at tsrx_place and a stream's arrivals in batch
 * order are one segment of plan_rx_rule.h's (sum, max) scan.  The segment
 * starts from the stream's record: H0 = (roc, s_l), s_l being the first
 * arrival's seq where it is not set (a stream new in the batch, or one SRTCP
 * created: stream.c:87-109), lix0 and bitmap0 its window.  Every packet is
 * verified by rx_settle with positions local to its segment; RX_UNSETTLED
 * rejects the plan.  A touched stream's record after the batch is what
 * plan_buckets_rx.hip writes for a one-stream session (tsrx_after).
 */
#ifndef PLAN_RTP_SEG_RX_H
#define PLAN_RTP_SEG_RX_H

#include "plan_rtp_seg.h"
#include "plan_rx_rule.h"

/* a stream the table does not hold yet (stream.c:45-67) */
PLAN_FN struct tseg_rec tsrx_new(uint32_t ssrc)
{
	struct tseg_rec r;
	r.ssrc = ssrc;
	r.roc = r.sl = r.pad = 0;
	r.llo = r.lhi = r.blo = r.bhi = 0;
	return r;
}

/* tseg_known where only the table's SSRCs are at hand (the records stay in
 * global memory: plan_buckets_rtp_streams_rx.hip) */
PLAN_FN uint32_t tsrx_known(const uint32_t *ssrcs, uint32_t nk, uint32_t ssrc)
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
PLAN_FN uint32_t tsrx_first(uint32_t start, const uint32_t *count,
			    uint32_t slot)
{
	uint32_t q;
	for (q = 0; q < slot && q < RSEG_MAX; q++)
		start += count[q];
	return start;
}

/* a window the rule's signed arithmetic cannot hold is left to the host */
PLAN_FN int tsrx_held(struct tseg_rec st)
{
	return !(st.lhi >> 30);
}

/* the receiver's (roc, s_l) before the stream's first arrival (seq0) */
PLAN_FN int64_t tsrx_h0(struct tseg_rec st, uint32_t seq0)
{
	return (int64_t)((uint64_t)st.roc << 16 | tseg_sl0(st.sl, seq0));
}

/* the scan element of a stream's arrival: the first one carries its index
 * (the reference step from H0), the others their distance to the arrival
 * before (pseq); *bad: the first step is an ETIMEDOUT */
PLAN_FN int64_t tsrx_elem(int head, int64_t H0, uint32_t seq, uint32_t pseq,
			  int *bad)
{
	int64_t u0 = 0;
	int bump = 0;
	if (!head)
		return rx_sdiff16(seq, pseq);
	if (rx_step(H0, seq, &u0, &bump)) {
		*bad = 1;
		return 0;
	}
	return u0;
}

/* the maximum of a stream's indices from its last arrival's u and mx */
PLAN_FN int64_t tsrx_smx(int64_t ulast, int64_t mxlast)
{
	return rx_max(ulast, mxlast);
}

/* desc flags of a settled packet: an EALREADY packet's tag is still checked
 * (HMAC suites: not decrypted; GCM decrypts to authenticate) */
PLAN_FN uint32_t tsrx_fl(int verdict, int hmac)
{
	return verdict == RX_DUP && hmac ? SD_RUN : SD_RUN | SD_CIPHER;
}

/* an accepted packet below its window's top at its arrival */
PLAN_FN int tsrx_late(int64_t ui, int64_t lix0, int64_t mxi)
{
	return ui < rx_max(lix0, mxi);
}

/* an accepted packet's bit in the window after the batch */
PLAN_FN uint64_t tsrx_bit(struct tseg_rec st, int64_t smx, int64_t ui)
{
	return rx_bit(rx_max((int64_t)tseg_lix(st), smx), ui);
}

/* a touched stream's record after the batch: H0 as tsrx_h0, smx the maximum
 * of its indices, bits the OR of its accepted packets' tsrx_bit */
PLAN_FN struct tseg_rec tsrx_after(struct tseg_rec st, int64_t H0, int64_t smx,
				   uint64_t bits)
{
	const int64_t lix0 = (int64_t)tseg_lix(st);
	const int64_t Mn = rx_max(H0, smx), lix = rx_max(lix0, smx);
	const uint64_t bm = rx_bitmap_base(lix, lix0, tseg_bitmap(st)) | bits;
	st.roc = (uint32_t)((uint64_t)Mn >> 16);
	st.sl = (uint32_t)((uint64_t)Mn & 0xffffu) | TSEG_SL_SET;
	st.llo = (uint32_t)(uint64_t)lix;
	st.lhi = (uint32_t)((uint64_t)lix >> 32);
	st.blo = (uint32_t)bm;
	st.bhi = (uint32_t)(bm >> 32);
	return st;
}

#endif
