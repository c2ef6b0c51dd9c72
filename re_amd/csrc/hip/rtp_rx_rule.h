/*
 * rtp_rx_rule.h -- the receiver-statistics rule, stated once: the RTP
 * header decode (rtp_hdr_decode + rtp_decode's version check,
 * src/rtp/rtp.c:88-137, 513-519), the member lookup (get_member,
 * src/rtp/sess.c:83-101), the per-packet update (rtcp_sess_rx_rtp,
 * sess.c:614-666, with rtp_source_update_seq / rtp_source_calc_jitter,
 * src/rtp/source.c:42-131), the incoming SR (handle_incoming_sr,
 * sess.c:168-185) and the report block (sender_apply_handler, sess.c:390-410,
 * source.c:135-177).  Pure functions of their arguments; compiles as C
 * (re_amd/csrc/host/rtp_stats.c, tests/c/rtp_rx_check.c) and as HIP device
 * code (rtp_stats.hip).
 *
 * Every state word is a uint32_t and every sum, difference and negation
 * wraps modulo 2^32, so no input is undefined behaviour; a signed view is
 * taken only to compare with 0, to clamp and to divide.  The reference
 * computes in `int` and agrees wherever that does not overflow.
 *
 * The member table is decomposed by slot, as the kernel walks it (8 lanes,
 * one per slot): rrx_slot_hit says whether a slot holds the packet's SSRC,
 * rrx_slot_new whether it is the slot a new SSRC takes; at most one slot
 * answers, and none for a 9th SSRC.
 */
#ifndef RTP_RX_RULE_H
#define RTP_RX_RULE_H

#include <errno.h>
#include <stdint.h>
#include "../../../include/re_rtp_stats_batch.h"

#ifdef __HIPCC__
#define RRX_FN __host__ __device__ static inline
#else
#define RRX_FN static inline
#endif

/*
 * The compact record the parallel pass leaves per packet (20 bytes):
 * seq_st = seq | RRX_REC_DROP when the packet takes no part in the walk
 * (its stat is already final).
 */
#define RRX_REC_DROP 0x10000u

struct rrx_rec {
	uint32_t seq_st;
	uint32_t ts;
	uint32_t arrival;
	uint32_t payload;
	uint32_t ssrc;
};

RRX_FN uint32_t rrx_be16(const uint8_t *p)
{
	return (uint32_t)p[0] << 8 | p[1];
}

RRX_FN uint32_t rrx_be32(const uint8_t *p)
{
	return rrx_be16(p) << 16 | rrx_be16(p + 2);
}

/*
 * rtp_hdr_decode + the version check over the len bytes at p; reads only
 * p[0 .. len).  0 and the record's seq / ts / ssrc / payload (the bytes
 * left after the header, padding included), or EBADMSG.
 */
RRX_FN int rrx_hdr_decode(const uint8_t *p, uint32_t len, struct rrx_rec *r)
{
	uint32_t left = len, cc, hl;

	if (left < 12)                          /* rtp.c:97 */
		return EBADMSG;
	cc = p[0] & 0x0f;
	left -= 12;
	if (left < cc * 4)                      /* rtp.c:116 */
		return EBADMSG;
	left -= cc * 4;
	hl = 12 + cc * 4;
	if (p[0] & 0x10) {
		uint32_t xl;
		if (left < 4)                   /* rtp.c:124 */
			return EBADMSG;
		xl = rrx_be16(p + hl + 2) * 4;
		left -= 4;
		if (left < xl)                  /* rtp.c:130 */
			return EBADMSG;
		left -= xl;
	}
	if ((p[0] >> 6) != 2)                   /* rtp.c:518 */
		return EBADMSG;
	r->seq_st = rrx_be16(p + 2);
	r->ts = rrx_be32(p + 4);
	r->ssrc = rrx_be32(p + 8);
	r->payload = left;
	return 0;
}

/*
 * The parallel pass for one packet: its final stat when it takes no part
 * in the walk (RTP_RX_SKIPPED, EINVAL, EBADMSG; the record is marked
 * RRX_REC_DROP), or 0 and the record.  skip: res[i] != 0; bad_sess:
 * sess[i] >= nsess.  Nothing outside arena[0 .. asz) is read.
 */
RRX_FN int rrx_record(const uint8_t *arena, uint64_t asz, uint32_t pos,
		      uint32_t end, int skip, int bad_sess, uint32_t arrival,
		      struct rrx_rec *r)
{
	int st;

	r->seq_st = RRX_REC_DROP;
	r->ts = r->payload = r->ssrc = 0;
	r->arrival = arrival;
	if (skip)
		return RTP_RX_SKIPPED;
	if (bad_sess || end < pos || end > asz)
		return EINVAL;
	st = rrx_hdr_decode(arena + pos, end - pos, r);
	if (st)
		r->seq_st = RRX_REC_DROP;
	return st;
}

/* get_member, by slot: the slot that holds ssrc ... */
RRX_FN int rrx_slot_hit(uint32_t memberc, uint32_t slot, uint32_t slot_ssrc,
			uint32_t ssrc)
{
	return slot < memberc && slot_ssrc == ssrc;
}

/* ... and, when no slot does, the one a new member takes (sess.c:91-98) */
RRX_FN int rrx_slot_new(uint32_t memberc, uint32_t slot, int any_hit)
{
	return !any_hit && slot == memberc && memberc < RTP_RX_MAX_MEMBERS;
}

/* rtp_member_add (member.c:27-39): a member without a source */
RRX_FN void rrx_member_init(struct rtp_rx_source *s, uint32_t ssrc)
{
	s->ssrc = ssrc;
	s->flags = 0;
	s->max_seq = s->cycles = s->base_seq = s->bad_seq = 0;
	s->received = s->expected_prior = s->received_prior = 0;
	s->transit = s->jitter = s->last_rtp_ts = 0;
	s->rx_bytes = s->sr_recv = 0;
	s->sr_ntp_hi = s->sr_ntp_lo = s->sr_rtp_ts = 0;
	s->sr_psent = s->sr_osent = s->reserved = 0;
}

/* rtp_source_init_seq (source.c:23-36) */
RRX_FN void rrx_init_seq(struct rtp_rx_source *s, uint32_t seq)
{
	s->base_seq = seq;
	s->max_seq = seq;
	s->bad_seq = 65536 + 1;
	s->cycles = 0;
	s->received = 0;
	s->received_prior = 0;
	s->expected_prior = 0;
}

/* rtp_source_update_seq (source.c:42-104) without probation */
RRX_FN int rrx_update_seq(struct rtp_rx_source *s, uint32_t seq)
{
	const uint32_t udelta = (seq - s->max_seq) & 0xffff;

	if (udelta < 3000) {                    /* MAX_DROPOUT */
		if (seq < s->max_seq)
			s->cycles += 65536;
		s->max_seq = seq;
	}
	else if (udelta <= 65536 - 100) {       /* MAX_MISORDER */
		if (seq == s->bad_seq) {
			rrx_init_seq(s, seq);
		}
		else {
			s->bad_seq = (seq + 1) & 0xffff;
			return 0;
		}
	}
	s->received++;
	return 1;
}

/* rtp_source_calc_jitter (source.c:114-131) */
RRX_FN void rrx_calc_jitter(struct rtp_rx_source *s, uint32_t ts,
			    uint32_t arrival)
{
	const uint32_t transit = arrival - ts;
	uint32_t d = transit - s->transit;

	if (!s->transit) {
		s->transit = transit;
		return;
	}
	s->transit = transit;
	if ((int32_t)d < 0)
		d = 0u - d;
	s->jitter += d - ((s->jitter + 8) >> 4);
}

/*
 * rtcp_sess_rx_rtp (sess.c:629-663) on the packet's member; what
 * rtp_source_update_seq returned.
 */
RRX_FN int rrx_source_rx(struct rtp_rx_source *s, uint32_t seq, uint32_t ts,
			 uint32_t arrival, int has_arrival, uint32_t payload)
{
	int ok;

	if (!(s->flags & RTP_RX_HAS_SOURCE)) {
		s->flags |= RTP_RX_HAS_SOURCE;
		rrx_init_seq(s, seq);
	}
	ok = rrx_update_seq(s, seq);
	if (has_arrival && ts != s->last_rtp_ts)
		rrx_calc_jitter(s, ts, arrival);
	s->last_rtp_ts = ts;
	s->rx_bytes += payload;
	return ok;
}

/* handle_incoming_sr (sess.c:175-185) on the SR's member */
RRX_FN void rrx_source_sr(struct rtp_rx_source *s, uint64_t recv_ms,
			  uint32_t ntp_sec, uint32_t ntp_frac,
			  uint32_t rtp_ts, uint32_t psent, uint32_t osent)
{
	if (!(s->flags & RTP_RX_HAS_SOURCE))
		return;
	s->sr_recv = recv_ms;
	s->sr_ntp_hi = ntp_sec;
	s->sr_ntp_lo = ntp_frac;
	s->sr_rtp_ts = rtp_ts;
	s->sr_psent = psent;
	s->sr_osent = osent;
}

/*
 * hash_apply over the 8-bucket member hash (member.c:35, hash.c:84, 136):
 * reports come by this key ascending; RRX_NOKEY: no report (no source, or
 * an unused slot).
 */
#define RRX_NOKEY 0xffu

RRX_FN uint32_t rrx_report_key(const struct rtp_rx_source *s, uint32_t slot,
			       uint32_t memberc)
{
	if (slot >= memberc || !(s->flags & RTP_RX_HAS_SOURCE))
		return RRX_NOKEY;
	return (s->ssrc & 7) * RTP_RX_MAX_MEMBERS + slot;
}

/* sender_apply_handler (sess.c:390-410); updates the priors */
RRX_FN void rrx_report_block(struct rtp_rx_source *s, uint64_t now_ms,
			     struct rtcp_enc_rb *rb)
{
	const uint32_t expected = s->cycles + s->max_seq - s->base_seq + 1;
	const uint32_t exp_int = expected - s->expected_prior;
	const uint32_t rcv_int = s->received - s->received_prior;
	const int32_t lost_int = (int32_t)(exp_int - rcv_int);
	int32_t lost = (int32_t)(expected - s->received);
	uint32_t fraction = 0;

	s->expected_prior = expected;
	s->received_prior = s->received;
	if (exp_int != 0 && lost_int > 0)       /* source.c:171-174 */
		fraction = (uint8_t)((int64_t)(int32_t)((uint32_t)lost_int << 8) /
				     (int64_t)(int32_t)exp_int);
	if (lost > 0x7fffff)
		lost = 0x7fffff;
	else if (lost < -0x7fffff)
		lost = -0x7fffff;
	rb->ssrc = s->ssrc;
	rb->fraction = fraction;
	rb->lost = (uint32_t)lost;
	rb->last_seq = s->cycles | s->max_seq;
	rb->jitter = s->jitter >> 4;
	/* calc_lsr / ntp_compact (sess.c:372, ntp.c:78) */
	rb->lsr = s->sr_ntp_hi ? (s->sr_ntp_hi & 0xffff) << 16 |
				 s->sr_ntp_lo >> 16 : 0;
	/* calc_dlsr (sess.c:378-387) */
	rb->dlsr = s->sr_recv ? (uint32_t)(65536 * (now_ms - s->sr_recv) / 1000)
			      : 0;
}

#endif
