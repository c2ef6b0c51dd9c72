/**
 * @file re_rtcp_sess_batch.h  Batched RTCP session state on the GPU: the
 * rest of libre's src/rtp/sess.c (extension).
 *
 * re_rtp_stats_batch.h keeps the receiver statistics of a batch of RTP
 * packets; the entries here add what libre's rtcp_sess does with the peer's
 * reports and with the packets it sends itself:
 *
 *   rtcp_rx_handle_batch_dev   rtcp_handler (sess.c:213-238: SR, RR, BYE)
 *                              over rtcp_decode_full_batch_dev's output
 *   rtp_tx_stats_batch_dev     rtcp_sess_tx_rtp (sess.c:593-611)
 *   rtcp_tx_report_batch_dev   mk_sr (sess.c:426-463): SR or RR descriptors
 *                              for rtcp_encode_batch_dev
 *   rtcp_stats_batch_dev       rtcp_stats (sess.c:678-714)
 *
 * so that both directions stay on the device:
 *   receive  srtcp_decrypt_batch_dev -> rtcp_decode_full_batch_dev ->
 *            rtcp_rx_handle_batch_dev
 *   send     rtp_tx_stats_batch_dev -> srtp_encrypt_batch_dev, and
 *            rtcp_tx_report_batch_dev -> rtcp_encode_batch_dev ->
 *            srtcp_encrypt_batch_dev
 *
 * Not covered: the RTCP timer and sending (schedule, send_rtcp_report,
 * rtcp_send), the CNAME SDES message and rtcp_debug.
 */
#ifndef RE_RTCP_SESS_BATCH_H
#define RE_RTCP_SESS_BATCH_H

#include <stddef.h>
#include <stdint.h>
#include "re_rtcp_batch.h"
#include "re_rtp_stats_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/** per-packet status of rtcp_rx_handle_batch_dev beyond those of
 *  re_rtp_stats_batch.h */
enum {
	RTCP_RX_TRUNCATED = -4, /**< nmsg[i] > maxmsg or nitem[i] > maxitem:
				     nothing of the packet was applied        */
};

/**
 * What struct rtcp_sess and struct rtp_member hold beyond the receiver
 * statistics, per session, beside struct rtp_rx_sess: 128 bytes of plain
 * data the caller owns; all zero is a fresh session.  Slot k of cum_lost /
 * jit / rtt belongs to the member rtp_rx_sess.m[k].  Slots >= memberc are
 * zero in both structs: members are appended at slot memberc and a BYE
 * removes slot j by moving slots j+1.. down one place in both structs and
 * zeroing the vacated last one, which keeps the insertion order (and with
 * it the reference's hash order of the remaining members).
 */
struct rtcp_sess_ext {
	int32_t  cum_lost[8];   /**< mbr->cum_lost                            */
	uint32_t jit[8];        /**< mbr->jit [us]                            */
	uint32_t rtt[8];        /**< mbr->rtt [us]                            */
	uint32_t psent, osent;  /**< txstat                                   */
	uint64_t jfs_rt_ref;    /**< txstat.jfs_rt_ref; 0: nothing sent yet   */
	uint32_t ts_ref;        /**< txstat.ts_ref                            */
	uint32_t ts_synced;     /**< txstat.ts_synced, 0 or 1                 */
	uint32_t srate_tx;      /**< rtcp_set_srate; set by the caller        */
	uint32_t srate_rx;
};

/**
 * rtcp_recv_handler's inner call (rtp.c:164-167 -> rtcp_handler) for the n
 * packets rtcp_decode_full_batch_dev decoded, every pointer device memory:
 * descv / nmsg / itemv / nitem with maxmsg / maxitem are that call's
 * outputs.  Every decoded message of packet i goes, in message order, to
 * session sessv[sess[i]] / extv[sess[i]] (sess NULL: session 0); packets of
 * one session are taken in array order.  The decoder's err[i] is not an
 * input: the reference dispatches each message as it is decoded, so the
 * nmsg[i] messages before the failing call are all applied.
 *
 *   SR (200)  get_member(desc.ssrc) (a 9th SSRC: the message does nothing);
 *             a member with a source stores recv_ms (tmr_jiffies() at
 *             reception) and the SR item's five words; then every RB item
 *             of the message is a report block *from that member* (the
 *             block's own ssrc is ignored, as in the reference)
 *   RR (201)  get_member even when the count is 0, then the blocks
 *   BYE (203) each BYE_SRC item in order: the member, when there is one, is
 *             removed with its source and its ext slot; an unknown source,
 *             or one named twice, does nothing
 *   others    nothing
 *
 * A report block (handle_rr_block, sess.c:129-142) sets cum_lost to the
 * sign-extended 24-bit lost field (item v[2] holds the field's 24 bits);
 * with srate_tx != 0, jit = (uint32_t)(1000000 * jitter) / srate_tx, the
 * product modulo 2^32; with lsr and dlsr both non-zero, rtt =
 * max((int32_t)(a_us - ntp_compact2us(lsr) - 1000000 * dlsr / 65536), 0)
 * where a_us = ntp_compact2us(ntp_compact(unix2ntp(now_us))), now_us being
 * the wall clock in microseconds since the Unix epoch, one value for the
 * call.
 *
 * stat, when given, receives per packet 0, RTP_RX_SKIPPED (res given and
 * res[i] != 0: nothing read), EINVAL (sess[i] >= nsess), RTCP_RX_TRUNCATED,
 * or RTP_RX_NOMEMBER (some SR / RR of the packet found no slot; its other
 * messages were applied).
 *
 * Queued on stream with no host synchronisation; scratch memory is kept
 * between calls.  0 or EINVAL / ENOMEM / EIO / ENOSYS (no GPU).
 */
int rtcp_rx_handle_batch_dev(const struct rtcp_desc *descv, uint32_t maxmsg,
			     const uint32_t *nmsg,
			     const struct rtcp_item *itemv, uint32_t maxitem,
			     const uint32_t *nitem, const int32_t *res,
			     const uint32_t *sess, size_t n,
			     struct rtp_rx_sess *sessv,
			     struct rtcp_sess_ext *extv, size_t nsess,
			     uint64_t recv_ms, uint64_t now_us, int32_t *stat,
			     void *stream);

/**
 * rtcp_sess_tx_rtp as rtp_send calls it (rtp.c:560-567) for n outgoing RTP
 * packets, on the plaintext before srtp_encrypt_batch_dev: packet i is
 * arena[pos[i], end[i]) of session extv[sess[i]] (sess NULL: session 0) and
 * was sent at jfs_rt[i] (microseconds since the Unix epoch).  Per accepted
 * packet psent += 1 and osent += end - pos - 12 - 4 * cc: what follows the
 * header rtp_hdr_encode wrote.  A header extension therefore counts as
 * payload here, unlike on the receive side, where rtp_hdr_decode steps over
 * it.  If the session is not ts_synced, its first accepted packet in array
 * order sets jfs_rt_ref = jfs_rt[i], ts_ref = its timestamp, ts_synced = 1.
 *
 * stat, when given: 0, RTP_RX_SKIPPED (res[i] != 0), EBADMSG (under 12 +
 * 4 * cc bytes, version != 2) or EINVAL (window outside the arena, end <
 * pos, sess[i] >= nsess).
 */
int rtp_tx_stats_batch_dev(const uint8_t *arena, size_t arena_size,
			   const uint32_t *pos, const uint32_t *end,
			   const int32_t *res, const uint32_t *sess,
			   const uint64_t *jfs_rt, size_t n,
			   struct rtcp_sess_ext *extv, size_t nsess,
			   int32_t *stat, void *stream);

/**
 * mk_sr for every session at now_ms (tmr_jiffies()) / now_us (wall clock):
 * report blocks and nrb exactly as rtp_rx_report_batch_dev writes them
 * (expected_prior / received_prior updated), and one descriptor per
 * session for rtcp_encode_batch_dev.  A session with jfs_rt_ref != 0 gets
 * an SR: pt 200, w[] = local_ssrc[i], ntp.hi, ntp.lo (unix2ntp(now_us)),
 * rtp_ts = (uint32_t)(ts_ref + (now_us - jfs_rt_ref) * srate_tx / 1000000)
 * in 64-bit wrap-around, psent, osent; otherwise an RR: pt 201, w[0] =
 * local_ssrc[i].  Either way count = num = nrb[i] (the reference's senderc),
 * first = 8 * i, and ts_synced is cleared.
 */
int rtcp_tx_report_batch_dev(struct rtp_rx_sess *sessv,
			     struct rtcp_sess_ext *extv, size_t nsess,
			     uint64_t now_ms, uint64_t now_us,
			     struct rtcp_enc_rb *rbv, uint32_t *nrb,
			     const uint32_t *local_ssrc,
			     struct rtcp_enc_msg *msgv, void *stream);

/**
 * rtcp_stats for n queries (session sess[i], NULL: session 0; member
 * ssrc[i]): out[7 * i ..] = tx_sent, tx_lost (two's complement), tx_jit,
 * rx_sent, rx_lost, rx_jit, rtt; rx_* are 0 for a member without a source
 * and rx_jit = srate_rx ? (uint32_t)(1000000 * (jitter >> 4)) / srate_rx :
 * 0.  err[i]: 0, ENOENT (unknown member) or EINVAL (sess[i] >= nsess);
 * then the row is zero.
 */
int rtcp_stats_batch_dev(const struct rtp_rx_sess *sessv,
			 const struct rtcp_sess_ext *extv, size_t nsess,
			 const uint32_t *sess, const uint32_t *ssrc, size_t n,
			 uint32_t *out, int32_t *err, void *stream);

/**
 * The same four on host memory, sequentially on the calling thread, from
 * the same rule (re_amd/csrc/hip/rtcp_sess_rule.h); they need no GPU.
 */
int rtcp_rx_handle_host(const struct rtcp_desc *descv, uint32_t maxmsg,
			const uint32_t *nmsg, const struct rtcp_item *itemv,
			uint32_t maxitem, const uint32_t *nitem,
			const int32_t *res, const uint32_t *sess, size_t n,
			struct rtp_rx_sess *sessv, struct rtcp_sess_ext *extv,
			size_t nsess, uint64_t recv_ms, uint64_t now_us,
			int32_t *stat);
int rtp_tx_stats_host(const uint8_t *arena, size_t arena_size,
		      const uint32_t *pos, const uint32_t *end,
		      const int32_t *res, const uint32_t *sess,
		      const uint64_t *jfs_rt, size_t n,
		      struct rtcp_sess_ext *extv, size_t nsess, int32_t *stat);
int rtcp_tx_report_host(struct rtp_rx_sess *sessv, struct rtcp_sess_ext *extv,
			size_t nsess, uint64_t now_ms, uint64_t now_us,
			struct rtcp_enc_rb *rbv, uint32_t *nrb,
			const uint32_t *local_ssrc, struct rtcp_enc_msg *msgv);
int rtcp_stats_host(const struct rtp_rx_sess *sessv,
		    const struct rtcp_sess_ext *extv, size_t nsess,
		    const uint32_t *sess, const uint32_t *ssrc, size_t n,
		    uint32_t *out, int32_t *err);

#ifdef __cplusplus
}
#endif

#endif
