/*
 * rtcp_sess_rule.h -- the RTCP session rule, stated once: what rtcp_handler
 * does with a decoded SR / RR / BYE (src/rtp/sess.c:129-238), the transmit
 * statistics (rtcp_sess_tx_rtp, sess.c:593-611), the SR / RR descriptor of
 * mk_sr (sess.c:426-463) and the rtcp_stats row (sess.c:678-714).  Pure
 * functions of their arguments; compiles as C (re_amd/csrc/host/rtcp_sess.c,
 * tests/c/rtcp_sess_check.c) and as HIP device code (rtcp_sess.hip).  The
 * member lookup, the stored SR and the report block are rtp_rx_rule.h's.
 *
 * As there, state words are uint32_t and wrap modulo 2^32; a signed view is
 * taken only to sign-extend, to compare with 0 and to clamp.
 *
 * The member table is decomposed by slot, as the kernel walks it (8 lanes,
 * one per slot, each holding its struct rtp_rx_source and its three words
 * of struct rtcp_sess_ext): a removal is stated as what every slot does
 * (rsx_remove_slot), the transmit statistics as a reduction (rsx_tx_one,
 * rsx_tx_combine, rsx_tx_finish) whose combine is associative and
 * commutative.
 */
#ifndef RTCP_SESS_RULE_H
#define RTCP_SESS_RULE_H

#include "../../../include/re_rtcp_sess_batch.h"
#include "rtp_rx_rule.h"

/* ---- NTP time (src/rtp/ntp.c) ------------------------------------------- */

/* ntp_compact (ntp.c:78) */
RRX_FN uint32_t rsx_ntp_compact(uint32_t hi, uint32_t lo)
{
	return (hi & 0xffff) << 16 | lo >> 16;
}

/* ntp_compact2us (ntp.c:91-97) */
RRX_FN uint64_t rsx_compact2us(uint32_t ntpc)
{
	const uint32_t hi = ntpc >> 16;
	const uint32_t lo = (ntpc & 0xffff) << 16;

	return 1000000ULL * hi + ((1000000ULL * lo) >> 32);
}

#ifndef __HIPCC__
/* ntp_time_get / unix2ntp (ntp.c:35-39, 61-67) of now_us; host only: the
 * fraction goes through a double, in the reference's order */
RRX_FN void rsx_unix2ntp(uint64_t now_us, uint32_t *hi, uint32_t *lo)
{
	const uint64_t sec = now_us / 1000000u, usec = now_us % 1000000u;

	*hi = (uint32_t)(sec + 0x83aa7e80u);
	*lo = (uint32_t)((double)usec * (double)(1LL << 32) * 1.0e-6);
}
#endif

/* ---- the incoming packet ------------------------------------------------ */

/*
 * A packet's final stat when it takes no part in the walk, or 0.  skip:
 * res[i] != 0 (then nothing else of the packet was read: pass zeros);
 * bad_sess: sess[i] >= nsess.
 */
RRX_FN int rsx_packet_stat(int skip, int bad_sess, uint32_t nmsg,
			   uint32_t maxmsg, uint32_t nitem, uint32_t maxitem)
{
	if (skip)
		return RTP_RX_SKIPPED;
	if (bad_sess)
		return EINVAL;
	if (nmsg > maxmsg || nitem > maxitem)
		return RTCP_RX_TRUNCATED;
	return 0;
}

/* does rtcp_handler look the message's sender up? (sess.c:221-227) */
RRX_FN int rsx_is_report(uint32_t pt)
{
	return pt == 200 || pt == 201;
}

/* the three words a member owns in struct rtcp_sess_ext */
struct rsx_mbr {
	uint32_t cum_lost, jit, rtt;
};

/*
 * handle_rr_block (sess.c:129-142) with rtcp_calc_rtt (:111-125) on the
 * sender's member: lost24 is the block's 24-bit lost field (item v[2]),
 * a_compact the compact NTP word of the call's wall clock.
 */
RRX_FN void rsx_rr_block(struct rsx_mbr *m, uint32_t srate_tx,
			 uint32_t a_compact, uint32_t lost24, uint32_t jitter,
			 uint32_t lsr, uint32_t dlsr)
{
	/* struct rtcp_rr: signed int lost:24 */
	m->cum_lost = ((lost24 & 0xffffffu) ^ 0x800000u) - 0x800000u;
	if (srate_tx)
		m->jit = (uint32_t)(1000000u * jitter) / srate_tx;
	if (lsr && dlsr) {
		const uint64_t d = rsx_compact2us(a_compact) -
			rsx_compact2us(lsr) - 1000000ULL * dlsr / 65536;
		const int32_t rtt = (int32_t)(uint32_t)d;

		m->rtt = rtt > 0 ? (uint32_t)rtt : 0;
	}
}

/*
 * handle_incoming_bye's mem_deref(mbr) (sess.c:201-208) of the member at
 * slot j, by slot: what `slot` does when memberc members are in use.
 */
enum { RSX_KEEP = 0, RSX_TAKE_NEXT = 1, RSX_ZERO = 2 };

RRX_FN int rsx_remove_slot(uint32_t slot, uint32_t j, uint32_t memberc)
{
	if (slot < j || slot >= memberc)
		return RSX_KEEP;
	return slot + 1 < memberc ? RSX_TAKE_NEXT : RSX_ZERO;
}

/* ---- transmit statistics ------------------------------------------------ */

/*
 * The outgoing packet arena[pos, end): 0 and the timestamp and the bytes
 * after the fixed header and the CSRCs (rtp_send, rtp.c:560-567), or
 * EBADMSG / EINVAL / RTP_RX_SKIPPED.  Nothing outside arena[0 .. asz) is
 * read.
 */
RRX_FN int rsx_tx_packet(const uint8_t *arena, uint64_t asz, uint32_t pos,
			 uint32_t end, int skip, int bad_sess, uint32_t *ts,
			 uint32_t *payload)
{
	uint32_t len, hl;

	*ts = *payload = 0;
	if (skip)
		return RTP_RX_SKIPPED;
	if (bad_sess || end < pos || end > asz)
		return EINVAL;
	len = end - pos;
	if (len < 12)
		return EBADMSG;
	hl = 12 + 4 * (arena[pos] & 0x0fu);
	if (len < hl || (arena[pos] >> 6) != 2)
		return EBADMSG;
	*ts = rrx_be32(arena + pos + 4);
	*payload = len - hl;
	return 0;
}

/* a set of accepted packets of one session: how many, their payload bytes
 * and the lowest array index among them (none: ~0) */
struct rsx_tx {
	uint32_t cnt, sum, first;
};

#define RSX_TX_NONE 0xffffffffu

RRX_FN struct rsx_tx rsx_tx_zero(void)
{
	const struct rsx_tx t = {0, 0, RSX_TX_NONE};
	return t;
}

RRX_FN struct rsx_tx rsx_tx_one(uint32_t payload, uint32_t index)
{
	const struct rsx_tx t = {1, payload, index};
	return t;
}

RRX_FN struct rsx_tx rsx_tx_combine(struct rsx_tx a, struct rsx_tx b)
{
	const struct rsx_tx t = {a.cnt + b.cnt, a.sum + b.sum,
				 a.first < b.first ? a.first : b.first};
	return t;
}

/* rtcp_sess_tx_rtp for the whole set; 1: the caller now stores the
 * jfs_rt and the timestamp of packet t.first (rsx_tx_sync) */
RRX_FN int rsx_tx_finish(struct rtcp_sess_ext *x, struct rsx_tx t)
{
	x->psent += t.cnt;
	x->osent += t.sum;
	return t.cnt && !x->ts_synced;
}

RRX_FN void rsx_tx_sync(struct rtcp_sess_ext *x, uint64_t jfs_rt, uint32_t ts)
{
	x->jfs_rt_ref = jfs_rt;
	x->ts_ref = ts;
	x->ts_synced = 1;
}

/* ---- the report --------------------------------------------------------- */

/*
 * mk_sr (sess.c:426-463) once the report blocks stand: turns the RR
 * descriptor rrx wrote for the session into the SR when something was sent,
 * and clears ts_synced.
 */
RRX_FN void rsx_report_msg(struct rtcp_sess_ext *x, uint64_t now_us,
			   uint32_t ntp_hi, uint32_t ntp_lo,
			   struct rtcp_enc_msg *m)
{
	if (x->jfs_rt_ref) {
		const uint64_t dur = now_us - x->jfs_rt_ref;

		m->pt = 200;
		m->w[1] = ntp_hi;
		m->w[2] = ntp_lo;
		m->w[3] = (uint32_t)((uint64_t)x->ts_ref +
				     dur * x->srate_tx / 1000000u);
		m->w[4] = x->psent;
		m->w[5] = x->osent;
	}
	x->ts_synced = 0;
}

/* ---- rtcp_stats --------------------------------------------------------- */

/* the row of the member at slot k (sess.c:694-709) */
RRX_FN void rsx_stats_row(const struct rtp_rx_source *s,
			  const struct rtcp_sess_ext *x, uint32_t k,
			  uint32_t *out)
{
	out[0] = x->psent;
	out[1] = (uint32_t)x->cum_lost[k];
	out[2] = x->jit[k];
	out[3] = out[4] = out[5] = 0;
	out[6] = x->rtt[k];
	if (s->flags & RTP_RX_HAS_SOURCE) {
		/* rtp_source_calc_lost: the report block's clamped count */
		struct rtp_rx_source c = *s;
		struct rtcp_enc_rb rb;

		rrx_report_block(&c, 0, &rb);
		out[3] = s->received;
		out[4] = rb.lost;
		out[5] = x->srate_rx ? (uint32_t)(1000000u * (s->jitter >> 4)) /
				       x->srate_rx : 0;
	}
}

#endif
