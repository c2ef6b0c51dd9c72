/*
 * rtcp_sess.c -- RTCP session state (include/re_rtcp_sess_batch.h):
 * argument checks of the device entries (kernels: hip/rtcp_sess.hip) and
 * the host twins, a plain sequential walk with the rule of
 * hip/rtcp_sess_rule.h.
 */
#include <errno.h>
#include <stdint.h>
#include <string.h>
#include "re_rtcp_sess_batch.h"
#include "../srtpgpu.h"
#include "srtp_int.h"
#include "../hip/rtcp_sess_rule.h"

/* get_member (sess.c:83-101), over the slots: the slot, or -1 */
static int member_get(struct rtp_rx_sess *ss, struct rtcp_sess_ext *x,
		      uint32_t ssrc)
{
	for (uint32_t k = 0; k < RTP_RX_MAX_MEMBERS; k++) {
		if (rrx_slot_hit(ss->memberc, k, ss->m[k].ssrc, ssrc))
			return (int)k;
	}
	for (uint32_t k = 0; k < RTP_RX_MAX_MEMBERS; k++) {
		if (rrx_slot_new(ss->memberc, k, 0)) {
			rrx_member_init(&ss->m[k], ssrc);
			x->cum_lost[k] = 0;
			x->jit[k] = x->rtt[k] = 0;
			ss->memberc++;
			return (int)k;
		}
	}
	return -1;
}

static void member_remove(struct rtp_rx_sess *ss, struct rtcp_sess_ext *x,
			  uint32_t ssrc)
{
	const uint32_t mc = ss->memberc;
	uint32_t j;

	for (j = 0; j < RTP_RX_MAX_MEMBERS; j++) {
		if (rrx_slot_hit(mc, j, ss->m[j].ssrc, ssrc))
			break;
	}
	if (j == RTP_RX_MAX_MEMBERS)
		return;
	/* ascending: a slot is overwritten after the one below took it */
	for (uint32_t k = 0; k < RTP_RX_MAX_MEMBERS; k++) {
		switch (rsx_remove_slot(k, j, mc)) {
		case RSX_TAKE_NEXT:
			ss->m[k] = ss->m[k + 1];
			x->cum_lost[k] = x->cum_lost[k + 1];
			x->jit[k] = x->jit[k + 1];
			x->rtt[k] = x->rtt[k + 1];
			break;
		case RSX_ZERO:
			memset(&ss->m[k], 0, sizeof(ss->m[k]));
			x->cum_lost[k] = 0;
			x->jit[k] = x->rtt[k] = 0;
			break;
		default:
			break;
		}
	}
	ss->memberc = mc - 1;
}

/* rtcp_handler for the messages of one decoded packet; 0 or
 * RTP_RX_NOMEMBER */
static int handle_packet(const struct rtcp_desc *d, uint32_t nm,
			 const struct rtcp_item *it, uint32_t ni,
			 struct rtp_rx_sess *ss, struct rtcp_sess_ext *x,
			 uint64_t recv_ms, uint32_t a_compact)
{
	uint32_t j = 0;
	int st = 0;

	for (uint32_t m = 0; m < nm; m++) {
		const uint32_t pt = d[m].pt;
		int k = -1;

		if (rsx_is_report(pt)) {
			k = member_get(ss, x, d[m].ssrc);
			if (k < 0)
				st = RTP_RX_NOMEMBER;
		}
		for (; j < ni && it[j].msg == (uint16_t)m; j++) {
			const struct rtcp_item *e = &it[j];

			if (k >= 0 && pt == 200 && e->kind == RTCP_ITEM_SR) {
				rrx_source_sr(&ss->m[k], recv_ms, e->v[0],
					      e->v[1], e->v[2], e->v[3],
					      e->v[4]);
			}
			else if (k >= 0 && e->kind == RTCP_ITEM_RB) {
				struct rsx_mbr mb = {(uint32_t)x->cum_lost[k],
						     x->jit[k], x->rtt[k]};
				rsx_rr_block(&mb, x->srate_tx, a_compact,
					     e->v[2], e->v[4], e->v[5],
					     e->v[6]);
				x->cum_lost[k] = (int32_t)mb.cum_lost;
				x->jit[k] = mb.jit;
				x->rtt[k] = mb.rtt;
			}
			else if (pt == 203 && e->kind == RTCP_ITEM_BYE_SRC) {
				member_remove(ss, x, e->v[0]);
			}
		}
	}
	return st;
}

static uint32_t a_compact_of(uint64_t now_us)
{
	uint32_t hi, lo;

	rsx_unix2ntp(now_us, &hi, &lo);
	return rsx_ntp_compact(hi, lo);
}

static int handle_args(const struct rtcp_desc *descv, uint32_t maxmsg,
		       const uint32_t *nmsg, const struct rtcp_item *itemv,
		       uint32_t maxitem, const uint32_t *nitem,
		       const struct rtp_rx_sess *sessv,
		       const struct rtcp_sess_ext *extv, size_t nsess)
{
	return descv && maxmsg && maxmsg <= 65536 && nmsg && itemv && maxitem &&
	       nitem && sessv && extv && nsess;
}

int rtcp_rx_handle_host(const struct rtcp_desc *descv, uint32_t maxmsg,
			const uint32_t *nmsg, const struct rtcp_item *itemv,
			uint32_t maxitem, const uint32_t *nitem,
			const int32_t *res, const uint32_t *sess, size_t n,
			struct rtp_rx_sess *sessv, struct rtcp_sess_ext *extv,
			size_t nsess, uint64_t recv_ms, uint64_t now_us,
			int32_t *stat)
{
	uint32_t a_compact;

	if (!n)
		return 0;
	if (!handle_args(descv, maxmsg, nmsg, itemv, maxitem, nitem, sessv,
			 extv, nsess) || n > UINT32_MAX || nsess >= UINT32_MAX)
		return EINVAL;
	a_compact = a_compact_of(now_us);
	for (size_t i = 0; i < n; i++) {
		const int skip = res && res[i];
		const uint32_t si = sess ? sess[i] : 0;
		int st = rsx_packet_stat(skip, si >= nsess, skip ? 0 : nmsg[i],
					 maxmsg, skip ? 0 : nitem[i], maxitem);
		if (!st)
			st = handle_packet(descv + i * maxmsg, nmsg[i],
					   itemv + i * maxitem, nitem[i],
					   &sessv[si], &extv[si], recv_ms,
					   a_compact);
		if (stat)
			stat[i] = st;
	}
	return 0;
}

int rtp_tx_stats_host(const uint8_t *arena, size_t arena_size,
		      const uint32_t *pos, const uint32_t *end,
		      const int32_t *res, const uint32_t *sess,
		      const uint64_t *jfs_rt, size_t n,
		      struct rtcp_sess_ext *extv, size_t nsess, int32_t *stat)
{
	if (!n)
		return 0;
	if (!arena || !pos || !end || !jfs_rt || !extv || !nsess ||
	    n > UINT32_MAX || nsess >= UINT32_MAX)
		return EINVAL;
	for (size_t i = 0; i < n; i++) {
		const uint32_t si = sess ? sess[i] : 0;
		uint32_t ts, payload;
		const int st = rsx_tx_packet(arena, arena_size, pos[i], end[i],
					     res && res[i], si >= nsess, &ts,
					     &payload);
		if (!st && rsx_tx_finish(&extv[si],
					 rsx_tx_one(payload, (uint32_t)i)))
			rsx_tx_sync(&extv[si], jfs_rt[i], ts);
		if (stat)
			stat[i] = st;
	}
	return 0;
}

int rtcp_tx_report_host(struct rtp_rx_sess *sessv, struct rtcp_sess_ext *extv,
			size_t nsess, uint64_t now_ms, uint64_t now_us,
			struct rtcp_enc_rb *rbv, uint32_t *nrb,
			const uint32_t *local_ssrc, struct rtcp_enc_msg *msgv)
{
	uint32_t hi, lo;
	int err;

	if (!nsess)
		return 0;
	if (!extv || !msgv)
		return EINVAL;
	err = rtp_rx_report_host(sessv, nsess, now_ms, rbv, nrb, local_ssrc,
				 msgv);
	if (err)
		return err;
	rsx_unix2ntp(now_us, &hi, &lo);
	for (size_t i = 0; i < nsess; i++)
		rsx_report_msg(&extv[i], now_us, hi, lo, &msgv[i]);
	return 0;
}

int rtcp_stats_host(const struct rtp_rx_sess *sessv,
		    const struct rtcp_sess_ext *extv, size_t nsess,
		    const uint32_t *sess, const uint32_t *ssrc, size_t n,
		    uint32_t *out, int32_t *err)
{
	if (!n)
		return 0;
	if (!sessv || !extv || !nsess || !ssrc || !out || !err ||
	    n > UINT32_MAX || nsess >= UINT32_MAX)
		return EINVAL;
	for (size_t i = 0; i < n; i++) {
		const uint32_t si = sess ? sess[i] : 0;
		uint32_t *row = out + 7 * i;

		memset(row, 0, 7 * sizeof(*row));
		err[i] = si >= nsess ? EINVAL : ENOENT;
		if (si >= nsess)
			continue;
		for (uint32_t k = 0; k < RTP_RX_MAX_MEMBERS; k++) {
			if (rrx_slot_hit(sessv[si].memberc, k,
					 sessv[si].m[k].ssrc, ssrc[i])) {
				rsx_stats_row(&sessv[si].m[k], &extv[si], k,
					      row);
				err[i] = 0;
				break;
			}
		}
	}
	return 0;
}

/* ---- device entries ----------------------------------------------------- */

int rtcp_rx_handle_batch_dev(const struct rtcp_desc *descv, uint32_t maxmsg,
			     const uint32_t *nmsg,
			     const struct rtcp_item *itemv, uint32_t maxitem,
			     const uint32_t *nitem, const int32_t *res,
			     const uint32_t *sess, size_t n,
			     struct rtp_rx_sess *sessv,
			     struct rtcp_sess_ext *extv, size_t nsess,
			     uint64_t recv_ms, uint64_t now_us, int32_t *stat,
			     void *stream)
{
	if (!n)
		return 0;
	if (!handle_args(descv, maxmsg, nmsg, itemv, maxitem, nitem, sessv,
			 extv, nsess) || n >= (1u << 31) || nsess >= (1u << 28))
		return EINVAL;
	if (!gpu_ready())
		return ENOSYS;
	return sgpu_rtcp_rx_handle(descv, maxmsg, nmsg, itemv, maxitem, nitem,
				   res, sess, (uint32_t)n, sessv, extv,
				   (uint32_t)nsess, recv_ms,
				   a_compact_of(now_us), stat, stream);
}

int rtp_tx_stats_batch_dev(const uint8_t *arena, size_t arena_size,
			   const uint32_t *pos, const uint32_t *end,
			   const int32_t *res, const uint32_t *sess,
			   const uint64_t *jfs_rt, size_t n,
			   struct rtcp_sess_ext *extv, size_t nsess,
			   int32_t *stat, void *stream)
{
	if (!n)
		return 0;
	if (!arena || !pos || !end || !jfs_rt || !extv || !nsess ||
	    n >= (1u << 31) || nsess >= (1u << 28))
		return EINVAL;
	if (!gpu_ready())
		return ENOSYS;
	return sgpu_rtp_tx_stats(arena, arena_size, pos, end, res, sess, jfs_rt,
				 (uint32_t)n, extv, (uint32_t)nsess, stat,
				 stream);
}

int rtcp_tx_report_batch_dev(struct rtp_rx_sess *sessv,
			     struct rtcp_sess_ext *extv, size_t nsess,
			     uint64_t now_ms, uint64_t now_us,
			     struct rtcp_enc_rb *rbv, uint32_t *nrb,
			     const uint32_t *local_ssrc,
			     struct rtcp_enc_msg *msgv, void *stream)
{
	uint32_t hi, lo;

	if (!nsess)
		return 0;
	if (!sessv || !extv || !rbv || !nrb || !local_ssrc || !msgv ||
	    nsess >= (1u << 28))
		return EINVAL;
	if (!gpu_ready())
		return ENOSYS;
	rsx_unix2ntp(now_us, &hi, &lo);
	return sgpu_rtcp_tx_report(sessv, extv, (uint32_t)nsess, now_ms, now_us,
				   hi, lo, rbv, nrb, local_ssrc, msgv, stream);
}

int rtcp_stats_batch_dev(const struct rtp_rx_sess *sessv,
			 const struct rtcp_sess_ext *extv, size_t nsess,
			 const uint32_t *sess, const uint32_t *ssrc, size_t n,
			 uint32_t *out, int32_t *err, void *stream)
{
	if (!n)
		return 0;
	if (!sessv || !extv || !nsess || !ssrc || !out || !err ||
	    n >= (1u << 28) || nsess >= (1u << 28))
		return EINVAL;
	if (!gpu_ready())
		return ENOSYS;
	return sgpu_rtcp_stats(sessv, extv, (uint32_t)nsess, sess, ssrc,
			       (uint32_t)n, out, err, stream);
}
