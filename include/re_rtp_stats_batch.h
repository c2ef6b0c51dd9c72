/**
 * @file re_rtp_stats_batch.h  Batched RTP receiver statistics on the GPU,
 * up to RTCP report blocks (extension).
 *
 * libre hands every received RTP packet from rtp_decode to rtcp_sess_rx_rtp
 * (src/rtp/rtp.c:203-209, src/rtp/sess.c:614-666), which finds or adds the
 * member of the packet's SSRC, runs the RFC 3550 A.1 sequence tracker and
 * the A.8 jitter estimator (src/rtp/source.c) and counts the payload bytes;
 * the sender-report path turns that state into report blocks
 * (sender_apply_handler, sess.c:390-410).  The entries here do the same for
 * a whole batch of packets resident in HBM -- typically the arena
 * srtp_decrypt_batch_dev just unprotected -- so that the chain
 * srtp_decrypt_batch_dev -> rtp_rx_stats_batch_dev ->
 * rtp_rx_report_batch_dev -> rtcp_encode_batch_dev ->
 * srtcp_encrypt_batch_dev never leaves the device.
 *
 * A batch leaves the state that the reference's calls would leave, taken
 * in array order.  All state arithmetic wraps modulo 2^32: where the
 * reference's `int` arithmetic is defined the results are the reference's,
 * elsewhere they are still defined.
 *
 * The report-block side of incoming reports (handle_rr_block,
 * sess.c:129-142: cum_lost, jit, rtt), the removal of members on BYE, the
 * transmit statistics (rtcp_sess_tx_rtp), sender reports and rtcp_stats
 * are in re_rtcp_sess_batch.h.
 */
#ifndef RE_RTP_STATS_BATCH_H
#define RE_RTP_STATS_BATCH_H

#include <stddef.h>
#include <stdint.h>
#include "re_rtcp_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
	RTP_RX_MAX_MEMBERS = 8,      /* MAX_MEMBERS, sess.c:35 */
	RTP_RX_HAS_SOURCE  = 1,      /* rtp_rx_source.flags: mbr->s exists */
};

/** per-packet status beyond 0 / EBADMSG / EINVAL (never an errno value) */
enum {
	RTP_RX_BADSEQ   = -1,  /**< rtp_source_update_seq returned 0 (a large
				    jump, not yet re-synchronised); jitter,
				    last_rtp_ts and rx_bytes were updated    */
	RTP_RX_NOMEMBER = -2,  /**< a 9th SSRC: nothing changed             */
	RTP_RX_SKIPPED  = -3,  /**< res[i] != 0: nothing read, nothing
				    changed                                  */
};

/**
 * One member of a session (struct rtp_member, src/rtp/rtcp.h:27, with its
 * struct rtp_source, include/re_rtp.h:374): 88 bytes, every field at its
 * natural alignment, no hidden padding.
 *
 *   offset  0  ssrc            member's SSRC (mbr->src)
 *           4  flags           RTP_RX_HAS_SOURCE once an RTP packet came
 *           8  max_seq         highest sequence number seen (16 bits)
 *          12  cycles          shifted count of sequence cycles
 *          16  base_seq
 *          20  bad_seq         last 'bad' seq + 1; 65537: none
 *          24  received
 *          28  expected_prior  at the last report
 *          32  received_prior  at the last report
 *          36  transit         relative transit time of the last packet;
 *                              0 also means "none yet" (source.c:120)
 *          40  jitter          scaled by 16
 *          44  last_rtp_ts
 *          48  rx_bytes        payload bytes (64 bits)
 *          56  sr_recv         recv_ms of the last SR (64 bits); 0: none
 *          64  sr_ntp_hi, 68 sr_ntp_lo, 72 sr_rtp_ts, 76 sr_psent,
 *          80  sr_osent        from the last SR
 *          84  reserved        0
 */
struct rtp_rx_source {
	uint32_t ssrc;
	uint32_t flags;
	uint32_t max_seq;
	uint32_t cycles;
	uint32_t base_seq;
	uint32_t bad_seq;
	uint32_t received;
	uint32_t expected_prior;
	uint32_t received_prior;
	uint32_t transit;
	uint32_t jitter;
	uint32_t last_rtp_ts;
	uint64_t rx_bytes;
	uint64_t sr_recv;
	uint32_t sr_ntp_hi;
	uint32_t sr_ntp_lo;
	uint32_t sr_rtp_ts;
	uint32_t sr_psent;
	uint32_t sr_osent;
	uint32_t reserved;
};

/**
 * One session's member table (struct rtcp_sess members / memberc): 712
 * bytes -- memberc at 0, 4 reserved bytes, then 8 sources of 88 bytes in
 * insertion order; m[0 .. memberc) are in use.  Plain data in memory the
 * caller owns; all zero is a fresh session.
 */
struct rtp_rx_sess {
	uint32_t memberc;
	uint32_t reserved;
	struct rtp_rx_source m[RTP_RX_MAX_MEMBERS];
};

/**
 * rtcp_sess_rx_rtp for n RTP packets, every pointer device memory: packet i
 * is arena[pos[i], end[i]) and belongs to session sessv[sess[i]] (sess
 * NULL: all to sessv[0]).  res, when given, holds srtp_decrypt_batch_dev's
 * per-packet results: a packet with res[i] != 0 is skipped.  arrival[i] is
 * the packet's hdr->ts_arrive in RTP timestamp units; NULL means no jitter
 * calculation (a session whose srate_rx is 0, sess.c:648).  Packets of one
 * session are applied in array order.  stat, when given, receives per
 * packet 0, RTP_RX_BADSEQ, RTP_RX_NOMEMBER, RTP_RX_SKIPPED, EBADMSG (what
 * rtp_decode rejects: under 12 bytes, CSRCs or the extension past the end,
 * version != 2) or EINVAL (window outside the arena, end < pos, sess[i] >=
 * nsess); the last four leave every state untouched and read nothing
 * outside the arena.  The payload size counted is end - pos - header bytes
 * (padding is not stripped, as in the reference).
 *
 * Queued on stream (hipStream_t, NULL: default) with no host
 * synchronisation (scratch memory is kept between calls; a call that has to
 * grow it allocates).  Returns 0 or EINVAL / ENOMEM / EIO / ENOSYS (no
 * GPU).
 */
int rtp_rx_stats_batch_dev(const uint8_t *arena, size_t arena_size,
			   const uint32_t *pos, const uint32_t *end,
			   const int32_t *res, const uint32_t *sess,
			   const uint32_t *arrival, size_t n,
			   struct rtp_rx_sess *sessv, size_t nsess,
			   int32_t *stat, void *stream);

/**
 * handle_incoming_sr (sess.c:168-185) for n sender reports in array order:
 * event i is for session sess[i] (NULL: sessv[0]) from ssrc[i].  The member
 * is looked up first, so an SR from an unknown SSRC takes a member slot
 * without a source (none when 8 are taken); only a member that has a source
 * stores recv_ms (tmr_jiffies() at reception, milliseconds) and the SR's
 * NTP time, RTP timestamp and packet / octet counts.  Events with sess[i]
 * >= nsess are ignored.
 */
int rtp_rx_sr_batch_dev(struct rtp_rx_sess *sessv, size_t nsess,
			const uint32_t *sess, const uint32_t *ssrc,
			const uint32_t *ntp_sec, const uint32_t *ntp_frac,
			const uint32_t *rtp_ts, const uint32_t *psent,
			const uint32_t *osent, uint64_t recv_ms, size_t n,
			void *stream);

/**
 * The report blocks of every session at now_ms (tmr_jiffies()), as
 * hash_apply(members, sender_apply_handler) writes them: session i's go to
 * rbv[8 * i ..] in the order of the reference's 8-bucket member hash (by
 * ssrc & 7, then by insertion), members without a source skipped, and
 * nrb[i] is their number; unused entries of rbv are zeroed.  lost is the
 * clamped signed count as a 32-bit two's-complement word (the encoder takes
 * its low 24 bits).  Like the reference's, a report updates expected_prior /
 * received_prior.  With rr_msgv, session i also gets the descriptor of one
 * RR message for rtcp_encode_batch_dev: pt 201, count = num = nrb[i],
 * w[0] = local_ssrc[i], first = 8 * i.
 */
int rtp_rx_report_batch_dev(struct rtp_rx_sess *sessv, size_t nsess,
			    uint64_t now_ms, struct rtcp_enc_rb *rbv,
			    uint32_t *nrb, const uint32_t *local_ssrc,
			    struct rtcp_enc_msg *rr_msgv, void *stream);

/**
 * The same three on host memory, sequentially on the calling thread, from
 * the same rule (re_amd/csrc/hip/rtp_rx_rule.h); they need no GPU.
 */
int rtp_rx_stats_host(const uint8_t *arena, size_t arena_size,
		      const uint32_t *pos, const uint32_t *end,
		      const int32_t *res, const uint32_t *sess,
		      const uint32_t *arrival, size_t n,
		      struct rtp_rx_sess *sessv, size_t nsess, int32_t *stat);
int rtp_rx_sr_host(struct rtp_rx_sess *sessv, size_t nsess,
		   const uint32_t *sess, const uint32_t *ssrc,
		   const uint32_t *ntp_sec, const uint32_t *ntp_frac,
		   const uint32_t *rtp_ts, const uint32_t *psent,
		   const uint32_t *osent, uint64_t recv_ms, size_t n);
int rtp_rx_report_host(struct rtp_rx_sess *sessv, size_t nsess,
		       uint64_t now_ms, struct rtcp_enc_rb *rbv, uint32_t *nrb,
		       const uint32_t *local_ssrc,
		       struct rtcp_enc_msg *rr_msgv);

#ifdef __cplusplus
}
#endif

#endif
