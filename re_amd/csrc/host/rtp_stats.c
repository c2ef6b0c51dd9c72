/*
 * rtp_stats.c -- RTP receiver statistics (include/re_rtp_stats_batch.h):
 * argument checks of the device entries (kernels: hip/rtp_stats.hip) and
 * the host twins, a plain sequential walk with the rule of
 * hip/rtp_rx_rule.h.
 */
#include <errno.h>
#include <stdint.h>
#include <string.h>
#include "re_rtp_stats_batch.h"
#include "../srtpgpu.h"
#include "srtp_int.h"
#include "../hip/rtp_rx_rule.h"

/* get_member (sess.c:83-101), over the slots */
static struct rtp_rx_source *member_get(struct rtp_rx_sess *ss, uint32_t ssrc)
{
	int hit = 0;

	for (uint32_t k = 0; k < RTP_RX_MAX_MEMBERS; k++) {
		if (rrx_slot_hit(ss->memberc, k, ss->m[k].ssrc, ssrc))
			return &ss->m[k];
	}
	for (uint32_t k = 0; k < RTP_RX_MAX_MEMBERS; k++) {
		if (rrx_slot_new(ss->memberc, k, hit)) {
			rrx_member_init(&ss->m[k], ssrc);
			ss->memberc++;
			return &ss->m[k];
		}
	}
	return NULL;
}

int rtp_rx_stats_host(const uint8_t *arena, size_t arena_size,
		      const uint32_t *pos, const uint32_t *end,
		      const int32_t *res, const uint32_t *sess,
		      const uint32_t *arrival, size_t n,
		      struct rtp_rx_sess *sessv, size_t nsess, int32_t *stat)
{
	if (!n)
		return 0;
	if (!arena || !pos || !end || !sessv || !nsess || n > UINT32_MAX ||
	    nsess >= UINT32_MAX)
		return EINVAL;
	for (size_t i = 0; i < n; i++) {
		const uint32_t si = sess ? sess[i] : 0;
		struct rtp_rx_source *s;
		struct rrx_rec r;
		int st = rrx_record(arena, arena_size, pos[i], end[i],
				    res && res[i], si >= nsess,
				    arrival ? arrival[i] : 0, &r);
		if (!st) {
			s = member_get(&sessv[si], r.ssrc);
			if (!s)
				st = RTP_RX_NOMEMBER;
			else if (!rrx_source_rx(s, r.seq_st, r.ts, r.arrival,
						arrival != NULL, r.payload))
				st = RTP_RX_BADSEQ;
		}
		if (stat)
			stat[i] = st;
	}
	return 0;
}

int rtp_rx_sr_host(struct rtp_rx_sess *sessv, size_t nsess,
		   const uint32_t *sess, const uint32_t *ssrc,
		   const uint32_t *ntp_sec, const uint32_t *ntp_frac,
		   const uint32_t *rtp_ts, const uint32_t *psent,
		   const uint32_t *osent, uint64_t recv_ms, size_t n)
{
	if (!n)
		return 0;
	if (!sessv || !nsess || !ssrc || !ntp_sec || !ntp_frac || !rtp_ts ||
	    !psent || !osent || n > UINT32_MAX || nsess >= UINT32_MAX)
		return EINVAL;
	for (size_t i = 0; i < n; i++) {
		const uint32_t si = sess ? sess[i] : 0;
		struct rtp_rx_source *s;
		if (si >= nsess)
			continue;
		s = member_get(&sessv[si], ssrc[i]);
		if (s)
			rrx_source_sr(s, recv_ms, ntp_sec[i], ntp_frac[i],
				      rtp_ts[i], psent[i], osent[i]);
	}
	return 0;
}

int rtp_rx_report_host(struct rtp_rx_sess *sessv, size_t nsess,
		       uint64_t now_ms, struct rtcp_enc_rb *rbv, uint32_t *nrb,
		       const uint32_t *local_ssrc, struct rtcp_enc_msg *rr_msgv)
{
	if (!nsess)
		return 0;
	if (!sessv || !rbv || !nrb || (rr_msgv && !local_ssrc) ||
	    nsess > UINT32_MAX / RTP_RX_MAX_MEMBERS)
		return EINVAL;
	for (size_t i = 0; i < nsess; i++) {
		struct rtp_rx_sess *ss = &sessv[i];
		struct rtcp_enc_rb *rb = rbv + i * RTP_RX_MAX_MEMBERS;
		uint32_t c = 0;

		memset(rb, 0, RTP_RX_MAX_MEMBERS * sizeof(*rb));
		for (uint32_t key = 0; key < RRX_NOKEY; key++) {
			const uint32_t k = key % RTP_RX_MAX_MEMBERS;
			if (rrx_report_key(&ss->m[k], k, ss->memberc) == key)
				rrx_report_block(&ss->m[k], now_ms, &rb[c++]);
		}
		nrb[i] = c;
		if (rr_msgv) {
			struct rtcp_enc_msg *m = &rr_msgv[i];
			memset(m, 0, sizeof(*m));
			m->pt = 201;
			m->count = (uint8_t)c;
			m->w[0] = local_ssrc[i];
			m->first = (uint32_t)i * RTP_RX_MAX_MEMBERS;
			m->num = c;
		}
	}
	return 0;
}

/* ---- device entries ----------------------------------------------------- */

int rtp_rx_stats_batch_dev(const uint8_t *arena, size_t arena_size,
			   const uint32_t *pos, const uint32_t *end,
			   const int32_t *res, const uint32_t *sess,
			   const uint32_t *arrival, size_t n,
			   struct rtp_rx_sess *sessv, size_t nsess,
			   int32_t *stat, void *stream)
{
	if (!n)
		return 0;
	if (!arena || !pos || !end || !sessv || !nsess || n >= (1u << 31) ||
	    nsess >= (1u << 28))
		return EINVAL;
	if (!gpu_ready())
		return ENOSYS;
	return sgpu_rtp_rx_stats(arena, arena_size, pos, end, res, sess,
				 arrival, (uint32_t)n, sessv, (uint32_t)nsess,
				 stat, stream);
}

int rtp_rx_sr_batch_dev(struct rtp_rx_sess *sessv, size_t nsess,
			const uint32_t *sess, const uint32_t *ssrc,
			const uint32_t *ntp_sec, const uint32_t *ntp_frac,
			const uint32_t *rtp_ts, const uint32_t *psent,
			const uint32_t *osent, uint64_t recv_ms, size_t n,
			void *stream)
{
	if (!n)
		return 0;
	if (!sessv || !nsess || !ssrc || !ntp_sec || !ntp_frac || !rtp_ts ||
	    !psent || !osent || n >= (1u << 31) || nsess >= (1u << 28))
		return EINVAL;
	if (!gpu_ready())
		return ENOSYS;
	return sgpu_rtp_rx_sr(sessv, (uint32_t)nsess, sess, ssrc, ntp_sec,
			      ntp_frac, rtp_ts, psent, osent, recv_ms,
			      (uint32_t)n, stream);
}

int rtp_rx_report_batch_dev(struct rtp_rx_sess *sessv, size_t nsess,
			    uint64_t now_ms, struct rtcp_enc_rb *rbv,
			    uint32_t *nrb, const uint32_t *local_ssrc,
			    struct rtcp_enc_msg *rr_msgv, void *stream)
{
	if (!nsess)
		return 0;
	if (!sessv || !rbv || !nrb || (rr_msgv && !local_ssrc) ||
	    nsess >= (1u << 28))
		return EINVAL;
	if (!gpu_ready())
		return ENOSYS;
	return sgpu_rtp_rx_report(sessv, (uint32_t)nsess, now_ms, rbv, nrb,
				  local_ssrc, rr_msgv, stream);
}
