/*
 * gen_rtcp_sess_golden.c -- RTCP session goldens from the reference itself
 * (tests/golden/rtcp_sess_golden.json.gz).
 *
 * Built by scripts/make_rtcp_sess_golden.sh against the reference's
 * src/rtp/pkt.c, rr.c, sdes.c, fb.c, member.c, source.c, rtp.c, ntp.c and
 * src/hash/hash.c (and the mbuf / mem / list closure), into a temporary
 * directory; nothing of the reference is kept.  It calls the reference's
 * own rtcp_encode (to build the compound packets and the reports),
 * rtcp_decode, rtcp_rr_encode, rtcp_sdes_encode, rtp_hdr_encode /
 * rtp_hdr_decode, rtp_member_find / rtp_member_add, hash_apply, unix2ntp,
 * ntp_compact, ntp_compact2us and the rtp_source_* functions.
 *
 * What joins them in the reference lives in src/rtp/sess.c and is static
 * or bound to a socket, a timer, a lock and the wall clock.  Restated
 * below, with tmr_jiffies() / ntp_time_get() replaced by times the case
 * gives: get_member (:83-101), rtcp_calc_rtt (:111-125), handle_rr_block
 * (:129-142), handle_incoming_rr / _sr / _bye (:146-210), rtcp_handler's
 * switch (:219-235), calc_lsr / calc_dlsr (:372-387), sender_apply_handler
 * (:390-410), mk_sr (:426-463), rtcp_sess_tx_rtp (:601-608),
 * rtcp_sess_rx_rtp (:623-663), rtcp_stats (:688-709), ntp_time_get's split
 * of the microseconds (ntp.c:65-67), rtp_send's payload size (rtp.c:560-566)
 * and rtp_decode's version check (rtp.c:518).
 *
 * Every case runs the same stages, so that a test can run all cases as one
 * batch, one session per case, with one clock for all:
 *   rtp rx A, tx A, rtcp A (received at 1000 ms, wall clock T0), check,
 *   report (6000 ms, T0 + 5 s), check, rtcp B (7000 ms, T0 + 6 s), rtp rx B,
 *   tx B, check, report (11000 ms, T0 + 10 s), stats
 * T0 is chosen so that the compact NTP time wraps between rtcp A and
 * rtcp B.
 *
 * Output (JSON): cases[] of {name, srate_tx, srate_rx, local_ssrc, kinds[]
 * (what the reference's code went through in this case, noted by the glue
 * below), stages[]}; a stage is
 *   {"op":"rtp","pk":[[hex, arrival, stat], ...]}
 *   {"op":"tx","pk":[[hex, jfs_rt], ...]}
 *   {"op":"rtcp","recv_ms":T,"now_us":U,"pk":[{"pkt":hex,"msgs":[[off,
 *        size, pt, count, length, ssrc, aux], ...],"items":[[msg, kind, sub,
 *        v0 .. v6], ...],"stat":"ok" | "nomember"}, ...]}   descriptors and
 *        items as in rtcp_decode_golden.json.gz; ssrc / aux are given for
 *        SR, RR and BYE only (0 otherwise) and only SR, RB and BYE_SRC
 *        items are listed
 *   {"op":"check","memberc":N,"senderc":N,"m":[[ssrc, has_source, max_seq,
 *        cycles, base_seq, bad_seq, received, expected_prior,
 *        received_prior, transit, jitter, last_rtp_ts, rx_bytes, sr_recv,
 *        ntp_hi, ntp_lo, rtp_ts, psent, osent, cum_lost, jit, rtt], ...],
 *        "tx":[psent, osent, jfs_rt_ref, ts_ref, ts_synced]}   members in
 *        hash_apply order
 *   {"op":"report","now_ms":T,"now_us":U,"pt":200 | 201,"senderc":N,
 *        "w":[ssrc, ntp_hi, ntp_lo, rtp_ts, psent, osent],"rb":[[ssrc,
 *        fraction, lost, last_seq, jitter, lsr, dlsr], ...],"bytes":hex}
 *   {"op":"stats","q":[[ssrc, err, tx_sent, tx_lost, tx_jit, rx_sent,
 *        rx_lost, rx_jit, rtt], ...]}
 *
 * Where the reference computes in `int`: loss counts and transit
 * differences stay below 2^30, where that is defined.  Three quantities
 * leave the defined range on purpose, and there the golden holds gcc's
 * two's-complement result: the conversion of the 24-bit lost field to
 * `signed int lost:24` (rr.c:66, implementation-defined), `1000000 *
 * rr->jitter` (an int times a uint32_t: unsigned, wraps by definition) and
 * the cast `(int)(a_us - lsr_us - dlsr_us)` of a uint64_t
 * (implementation-defined).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include <re.h>
#include "rtcp.h"          /* struct rtp_member, ntp_*, rtcp_rr_encode */

enum { MAX_MEMBERS = 8, MAXEV = 64, MAXPKT = 256, MAXQ = 16 };

#define T0_US (0x6500817dULL * 1000000u + 654321u)

static const uint64_t RECV_MS[2] = {1000, 7000};
static const uint64_t RTCP_US[2] = {T0_US, T0_US + 6000000u};
static const uint64_t REP_MS[2] = {6000, 11000};
static const uint64_t REP_US[2] = {T0_US + 5000000u, T0_US + 10000000u};

/* ---- the case under construction --------------------------------------- */

struct pkt {
	uint8_t b[MAXPKT];
	size_t len;
	uint32_t arr;
	/* outgoing: rtp_send's ts, jfs_rt and mbuf_get_left() after the header */
	uint32_t ts;
	uint64_t jfs_rt;
	size_t left;
};

static struct {
	const char *name;
	uint32_t srate_tx, srate_rx, local_ssrc;
	struct pkt rtp[2][MAXEV], tx[2][MAXEV];
	size_t nrtp[2], ntx[2];
	struct mbuf *cp[2][MAXEV];
	size_t ncp[2];
	uint32_t q[MAXQ];
	size_t nq;
} C;

static int stage;               /* 0: A, 1: B */

static void begin(const char *name, uint32_t srate_tx, uint32_t srate_rx)
{
	memset(&C, 0, sizeof(C));
	C.name = name;
	C.srate_tx = srate_tx;
	C.srate_rx = srate_rx;
	C.local_ssrc = 0x4c000000u + (uint32_t)strlen(name);
	stage = 0;
}

/* a received packet with an 8-byte payload */
static void pk(uint32_t seq, uint32_t ts, uint32_t ssrc, uint32_t arr)
{
	struct pkt *p;
	size_t i;

	if (C.nrtp[stage] >= MAXEV)
		abort();
	p = &C.rtp[stage][C.nrtp[stage]++];
	memset(p->b, 0xa5, 20);
	p->b[0] = 0x80;
	p->b[1] = 96;
	p->b[2] = (uint8_t)(seq >> 8);
	p->b[3] = (uint8_t)seq;
	for (i = 0; i < 4; i++) {
		p->b[4 + i] = (uint8_t)(ts >> (24 - 8 * i));
		p->b[8 + i] = (uint8_t)(ssrc >> (24 - 8 * i));
	}
	p->len = 20;
	p->arr = arr;
}

/* an outgoing packet as rtp_send builds it: rtp_hdr_encode, then the
 * payload (with ext, its first bytes are the extension) */
static void tx(uint32_t cc, int ext, uint32_t ts, size_t payload,
	       uint64_t jfs_rt)
{
	struct rtp_header hdr;
	struct mbuf *mb = mbuf_alloc(MAXPKT);
	struct pkt *p;
	uint32_t i;

	if (C.ntx[stage] >= MAXEV || !mb)
		abort();
	p = &C.tx[stage][C.ntx[stage]++];
	memset(&hdr, 0, sizeof(hdr));
	hdr.ver = 2;
	hdr.ext = ext;
	hdr.cc = cc;
	hdr.pt = 96;
	hdr.seq = (uint16_t)(C.ntx[stage] + 100 * stage);
	hdr.ts = ts;
	hdr.ssrc = C.local_ssrc;
	for (i = 0; i < cc; i++)
		hdr.csrc[i] = 0xc0 + i;
	if (rtp_hdr_encode(mb, &hdr))
		abort();
	p->ts = ts;
	p->left = payload;
	for (i = 0; i < payload; i++)
		(void)mbuf_write_u8(mb, (uint8_t)(0x30 + i));
	if (mb->end > MAXPKT)
		abort();
	memcpy(p->b, mb->buf, mb->end);
	p->len = mb->end;
	p->jfs_rt = jfs_rt;
	mem_deref(mb);
}

/* ---- compound packets, by the reference's encoder ----------------------- */

struct blocks {
	const struct rtcp_rr *v;
	uint32_t n;
};

static int blocks_h(struct mbuf *mb, void *arg)
{
	const struct blocks *b = arg;
	uint32_t i;
	int err = 0;

	for (i = 0; i < b->n; i++)
		err |= rtcp_rr_encode(mb, &b->v[i]);
	return err;
}

static int sdes_h(struct mbuf *mb, void *arg)
{
	return rtcp_sdes_encode(mb, *(uint32_t *)arg, 1, RTCP_SDES_CNAME,
				"a@example");
}

static struct mbuf *cur;

static void compound(void)
{
	if (C.ncp[stage] >= MAXEV)
		abort();
	cur = C.cp[stage][C.ncp[stage]++] = mbuf_alloc(512);
	if (!cur)
		abort();
}

static void m_sr(uint32_t ssrc, uint32_t sec, uint32_t frac, uint32_t ts,
		 uint32_t ps, uint32_t os, const struct rtcp_rr *v, uint32_t n)
{
	struct blocks b = {v, n};

	if (rtcp_encode(cur, RTCP_SR, n, ssrc, sec, frac, ts, ps, os, blocks_h,
			&b))
		abort();
}

static void m_rr(uint32_t ssrc, const struct rtcp_rr *v, uint32_t n)
{
	struct blocks b = {v, n};

	if (rtcp_encode(cur, RTCP_RR, n, ssrc, blocks_h, &b))
		abort();
}

static void m_bye(const uint32_t *srcv, uint32_t n, const char *reason)
{
	if (rtcp_encode(cur, RTCP_BYE, n, srcv, reason))
		abort();
}

static void m_sdes(uint32_t src)
{
	if (rtcp_encode(cur, RTCP_SDES, 1, sdes_h, &src))
		abort();
}

static void m_app(uint32_t src)
{
	if (rtcp_encode(cur, RTCP_APP, 3, src, "test", (const uint8_t *)"12345678",
			(size_t)8))
		abort();
}

static void m_pli(uint32_t ssrc, uint32_t media)
{
	if (rtcp_encode(cur, RTCP_PSFB, RTCP_PSFB_PLI, ssrc, media, NULL, NULL))
		abort();
}

/* ---- what the glue went through (the case's "kinds") ------------------- */

enum kind {
	K_RR0_NEW, K_NINTH_SR, K_NINTH_RR, K_SR_NOSOURCE, K_SR_SOURCE,
	K_MULTI_BLOCK, K_LSR0, K_DLSR0, K_NEG_LOST, K_JIT_WRAP, K_SRATE_TX0,
	K_RTT_CLAMPED, K_RTT_POSITIVE, K_NTP_WRAP, K_BYE_SOURCE,
	K_BYE_NOSOURCE, K_BYE_UNKNOWN, K_BYE_TWICE, K_BYE_FIRST, K_BYE_MIDDLE,
	K_BYE_LAST, K_READD_SAME_BUCKET, K_BYE_THEN_RTP, K_OTHER_MSGS,
	K_REPORT_RR, K_REPORT_SR, K_TX_RESYNC, K_NOW_BEFORE_REF, K_COUNT
};

static const char *const kind_name[K_COUNT] = {
	"rr0_new", "ninth_sr", "ninth_rr", "sr_nosource", "sr_source",
	"multi_block", "lsr0", "dlsr0", "neg_lost", "jit_wrap", "srate_tx0",
	"rtt_clamped", "rtt_positive", "ntp_wrap", "bye_source",
	"bye_nosource", "bye_unknown", "bye_twice", "bye_first", "bye_middle",
	"bye_last", "readd_same_bucket", "bye_then_rtp", "other_msgs",
	"report_rr", "report_sr", "tx_resync", "now_before_ref"
};

static int kinds[K_COUNT];

/* ---- the glue of sess.c, restated -------------------------------------- */

struct sess {
	struct hash *members;
	uint32_t memberc, senderc;
	uint32_t srate_tx, srate_rx;
	uint32_t psent, osent;
	uint64_t jfs_rt_ref;
	uint32_t ts_ref;
	bool ts_synced;
	/* for the kinds only: the members in insertion order, and who left */
	uint32_t ord[MAX_MEMBERS], gone[64];
	uint32_t nord, ngone;
};

static uint64_t wall_us;        /* ntp_time_get's clock */

static void ntp_now(struct rtp_ntp_time *ntp, uint64_t jfs)
{
	struct timeval tv;

	tv.tv_sec = (time_t)(jfs / 1000000u);
	tv.tv_usec = (suseconds_t)(jfs % 1000000u);
	unix2ntp(ntp, &tv);
}

static bool was_gone(const struct sess *s, uint32_t src)
{
	uint32_t i;

	for (i = 0; i < s->ngone; i++) {
		if (s->gone[i] == src)
			return true;
	}
	return false;
}

static struct rtp_member *get_member(struct sess *s, uint32_t src, bool *isnew)
{
	struct rtp_member *mbr = rtp_member_find(s->members, src);
	uint32_t i;

	if (isnew)
		*isnew = false;
	if (mbr)
		return mbr;
	if (s->memberc >= MAX_MEMBERS)
		return NULL;
	mbr = rtp_member_add(s->members, src);
	if (!mbr)
		abort();
	++s->memberc;
	if (isnew)
		*isnew = true;
	for (i = 0; i < s->nord; i++) {
		if (s->ngone && (s->ord[i] & 7) == (src & 7))
			kinds[K_READD_SAME_BUCKET] |= was_gone(s, src);
	}
	s->ord[s->nord++] = src;
	return mbr;
}

static void handle_rr_block(struct sess *s, struct rtp_member *mbr,
			    const struct rtcp_rr *rr)
{
	mbr->cum_lost = rr->lost;
	kinds[K_NEG_LOST] |= rr->lost < 0;
	if (s->srate_tx) {
		mbr->jit = 1000000 * rr->jitter / s->srate_tx;
		kinds[K_JIT_WRAP] |= 1000000ULL * rr->jitter >= 1ULL << 32;
	}
	else {
		kinds[K_SRATE_TX0] = 1;
	}
	kinds[K_LSR0] |= !rr->lsr;
	kinds[K_DLSR0] |= !rr->dlsr;
	if (rr->lsr && rr->dlsr) {
		struct rtp_ntp_time ntp_time;
		uint64_t a_us, lsr_us, dlsr_us;

		ntp_now(&ntp_time, wall_us);
		a_us    = ntp_compact2us(ntp_compact(&ntp_time));
		lsr_us  = ntp_compact2us(rr->lsr);
		dlsr_us = 1000000ULL * rr->dlsr / 65536;
		mbr->rtt = MAX((int)(a_us - lsr_us - dlsr_us), 0);
		kinds[mbr->rtt ? K_RTT_POSITIVE : K_RTT_CLAMPED] = 1;
		kinds[K_NTP_WRAP] |= (ntp_compact(&ntp_time) >> 16) < 16 &&
				     (rr->lsr >> 16) > 0x8000;
	}
}

/* rtcp_handler; false: a member could not be added */
static bool handler(struct sess *s, const struct rtcp_msg *msg,
		    uint64_t recv_ms)
{
	struct rtp_member *mbr;
	uint32_t i, j;
	bool isnew;

	switch (msg->hdr.pt) {

	case RTCP_SR:
		mbr = get_member(s, msg->r.sr.ssrc, NULL);
		if (!mbr) {
			kinds[K_NINTH_SR] = 1;
			return false;
		}
		kinds[mbr->s ? K_SR_SOURCE : K_SR_NOSOURCE] = 1;
		if (mbr->s) {
			mbr->s->sr_recv = recv_ms;
			mbr->s->last_sr.hi = msg->r.sr.ntp_sec;
			mbr->s->last_sr.lo = msg->r.sr.ntp_frac;
			mbr->s->rtp_ts     = msg->r.sr.rtp_ts;
			mbr->s->psent      = msg->r.sr.psent;
			mbr->s->osent      = msg->r.sr.osent;
		}
		kinds[K_MULTI_BLOCK] |= msg->hdr.count > 1;
		for (i = 0; i < msg->hdr.count; i++)
			handle_rr_block(s, mbr, &msg->r.sr.rrv[i]);
		break;

	case RTCP_RR:
		mbr = get_member(s, msg->r.rr.ssrc, &isnew);
		if (!mbr) {
			kinds[K_NINTH_RR] = 1;
			return false;
		}
		kinds[K_RR0_NEW] |= isnew && !msg->hdr.count;
		kinds[K_MULTI_BLOCK] |= msg->hdr.count > 1;
		for (i = 0; i < msg->hdr.count; i++)
			handle_rr_block(s, mbr, &msg->r.rr.rrv[i]);
		break;

	case RTCP_BYE:
		for (i = 0; i < msg->hdr.count; i++) {
			const uint32_t src = msg->r.bye.srcv[i];

			mbr = rtp_member_find(s->members, src);
			if (!mbr) {
				kinds[K_BYE_UNKNOWN] = 1;
				for (j = 0; j < i; j++)
					kinds[K_BYE_TWICE] |=
						msg->r.bye.srcv[j] == src;
				continue;
			}
			kinds[mbr->s ? K_BYE_SOURCE : K_BYE_NOSOURCE] = 1;
			for (j = 0; s->ord[j] != src; j++)
				;
			if (s->nord >= 3)
				kinds[!j ? K_BYE_FIRST : j + 1 == s->nord ?
				      K_BYE_LAST : K_BYE_MIDDLE] = 1;
			memmove(&s->ord[j], &s->ord[j + 1],
				(s->nord - j - 1) * sizeof(s->ord[0]));
			s->nord--;
			if (s->ngone < 64)
				s->gone[s->ngone++] = src;
			if (mbr->s)
				--s->senderc;
			--s->memberc;
			mem_deref(mbr);
		}
		break;

	default:
		kinds[K_OTHER_MSGS] = 1;
		break;
	}
	return true;
}

/* udp_recv_handler -> rtp_decode -> rtcp_sess_rx_rtp */
static const char *rx_rtp(struct sess *s, const struct pkt *p)
{
	struct mbuf *mb = mbuf_alloc(MAXPKT);
	struct rtp_header hdr;
	struct rtp_member *mbr;
	size_t payload;
	int err, ok;

	if (!mb)
		abort();
	(void)mbuf_write_mem(mb, p->b, p->len);
	mb->pos = 0;
	memset(&hdr, 0, sizeof(hdr));
	err = rtp_hdr_decode(&hdr, mb);
	payload = mbuf_get_left(mb);
	mem_deref(mb);
	if (err || hdr.ver != 2)
		return "badmsg";
	mbr = get_member(s, hdr.ssrc, NULL);
	if (!mbr)
		return "nomember";
	if (!mbr->s) {
		mbr->s = mem_zalloc(sizeof(*mbr->s), NULL);
		if (!mbr->s)
			abort();
		rtp_source_init_seq(mbr->s, hdr.seq);
		++s->senderc;
		kinds[K_BYE_THEN_RTP] |= was_gone(s, hdr.ssrc);
	}
	ok = rtp_source_update_seq(mbr->s, hdr.seq);
	if (s->srate_rx && hdr.ts != mbr->s->last_rtp_ts)
		rtp_source_calc_jitter(mbr->s, hdr.ts, p->arr);
	mbr->s->last_rtp_ts = hdr.ts;
	mbr->s->rtp_rx_bytes += payload;
	return ok ? "ok" : "badseq";
}

/* rtp_send -> rtcp_sess_tx_rtp */
static void tx_rtp(struct sess *s, const struct pkt *p)
{
	s->osent += (uint32_t)p->left;
	s->psent += 1;
	if (!s->ts_synced) {
		kinds[K_TX_RESYNC] |= s->psent > 1;
		s->jfs_rt_ref = p->jfs_rt;
		s->ts_ref = p->ts;
		s->ts_synced = true;
	}
}

static int sep;
static uint64_t now_ms;

static bool check_h(struct le *le, void *arg)
{
	const struct rtp_member *mbr = le->data;
	const struct rtp_source *s = mbr->s;
	(void)arg;

	printf("%s[%u,%d", sep++ ? "," : "", mbr->src, s ? 1 : 0);
	if (s)
		printf(",%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%llu,%llu,%u,%u,%u,%u,%u",
		       s->max_seq, s->cycles, s->base_seq, s->bad_seq,
		       s->received, s->expected_prior, s->received_prior,
		       (uint32_t)s->transit, s->jitter, s->last_rtp_ts,
		       (unsigned long long)s->rtp_rx_bytes,
		       (unsigned long long)s->sr_recv, s->last_sr.hi,
		       s->last_sr.lo, s->rtp_ts, s->psent, s->osent);
	else
		printf(",0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0");
	printf(",%d,%u,%u]", mbr->cum_lost, mbr->jit, mbr->rtt);
	return false;
}

/* sender_apply_handler; prints the block it encodes */
static bool report_h(struct le *le, void *arg)
{
	struct rtp_member *mbr = le->data;
	struct rtp_source *s = mbr->s;
	struct mbuf *mb = arg;
	struct rtcp_rr rr;

	if (!s)
		return false;
	rr.ssrc     = mbr->src;
	rr.fraction = rtp_source_calc_fraction_lost(s);
	rr.lost     = rtp_source_calc_lost(s);
	rr.last_seq = s->cycles | s->max_seq;
	rr.jitter   = s->jitter >> 4;
	rr.lsr      = s->last_sr.hi ? ntp_compact(&s->last_sr) : 0;
	rr.dlsr     = s->sr_recv ?
		(uint32_t)((65536 * (now_ms - s->sr_recv)) / 1000) : 0;
	printf("%s[%u,%u,%d,%u,%u,%u,%u]", sep++ ? "," : "", rr.ssrc,
	       rr.fraction, rr.lost, rr.last_seq, rr.jitter, rr.lsr, rr.dlsr);
	return 0 != rtcp_rr_encode(mb, &rr);
}

static int encode_handler(struct mbuf *mb, void *arg)
{
	return hash_apply(arg, report_h, mb) ? ENOMEM : 0;
}

/* ---- run the case's stages --------------------------------------------- */

static void hex(const uint8_t *b, size_t n)
{
	size_t i;

	for (i = 0; i < n; i++)
		printf("%02x", b[i]);
}

static void st_rtp(struct sess *s, int k)
{
	size_t i;

	printf("{\"op\":\"rtp\",\"pk\":[");
	for (i = 0; i < C.nrtp[k]; i++) {
		const struct pkt *p = &C.rtp[k][i];
		printf("%s[\"", i ? "," : "");
		hex(p->b, p->len);
		printf("\",%u,\"%s\"]", p->arr, rx_rtp(s, p));
	}
	printf("]}");
}

static void st_tx(struct sess *s, int k)
{
	size_t i;

	printf(",{\"op\":\"tx\",\"pk\":[");
	for (i = 0; i < C.ntx[k]; i++) {
		const struct pkt *p = &C.tx[k][i];
		printf("%s[\"", i ? "," : "");
		hex(p->b, p->len);
		printf("\",%llu]", (unsigned long long)p->jfs_rt);
		tx_rtp(s, p);
	}
	printf("]}");
}

/* rtcp_recv_handler's loop (rtp.c:164-167) over one compound */
static void rtcp_packet(struct sess *s, struct mbuf *mb, uint64_t recv_ms)
{
	struct rtcp_msg *msgv[32], *msg;
	size_t start, nm = 0, i;
	bool all = true;
	uint32_t j;
	int ni = 0;

	printf("{\"pkt\":\"");
	hex(mb->buf, mb->end);
	printf("\",\"msgs\":[");
	mb->pos = 0;
	for (;;) {
		uint32_t ssrc = 0, aux = 0;

		start = mb->pos;
		if (rtcp_decode(&msg, mb))
			break;
		if (nm >= 32)
			abort();
		switch (msg->hdr.pt) {
		case RTCP_SR:
			ssrc = msg->r.sr.ssrc;
			aux = msg->r.sr.rtp_ts;
			break;
		case RTCP_RR:
			ssrc = msg->r.rr.ssrc;
			break;
		case RTCP_BYE:
			ssrc = msg->hdr.count ? msg->r.bye.srcv[0] : 0;
			break;
		default:
			break;
		}
		printf("%s[%zu,%zu,%u,%u,%u,%u,%u]", nm ? "," : "", start,
		       mb->pos - start, msg->hdr.pt, msg->hdr.count,
		       msg->hdr.length, ssrc, aux);
		/* dispatched as it is decoded, like the reference */
		all &= handler(s, msg, recv_ms);
		msgv[nm++] = msg;
	}
	printf("],\"items\":[");
	for (i = 0; i < nm; i++) {
		const struct rtcp_rr *rrv = NULL;

		msg = msgv[i];
		if (msg->hdr.pt == RTCP_SR) {
			printf("%s[%zu,1,0,%u,%u,%u,%u,%u,0,0]", ni++ ? "," : "",
			       i, msg->r.sr.ntp_sec, msg->r.sr.ntp_frac,
			       msg->r.sr.rtp_ts, msg->r.sr.psent,
			       msg->r.sr.osent);
			rrv = msg->r.sr.rrv;
		}
		else if (msg->hdr.pt == RTCP_RR) {
			rrv = msg->r.rr.rrv;
		}
		for (j = 0; rrv && j < msg->hdr.count; j++)
			printf("%s[%zu,2,0,%u,%u,%u,%u,%u,%u,%u]",
			       ni++ ? "," : "", i, rrv[j].ssrc, rrv[j].fraction,
			       (uint32_t)rrv[j].lost & 0xffffffu,
			       rrv[j].last_seq, rrv[j].jitter, rrv[j].lsr,
			       rrv[j].dlsr);
		for (j = 0; msg->hdr.pt == RTCP_BYE && j < msg->hdr.count; j++)
			printf("%s[%zu,5,0,%u,0,0,0,0,0,0]", ni++ ? "," : "", i,
			       msg->r.bye.srcv[j]);
		mem_deref(msg);
	}
	printf("],\"stat\":\"%s\"}", all ? "ok" : "nomember");
}

static void st_rtcp(struct sess *s, int k)
{
	size_t i;

	wall_us = RTCP_US[k];
	printf(",{\"op\":\"rtcp\",\"recv_ms\":%llu,\"now_us\":%llu,\"pk\":[",
	       (unsigned long long)RECV_MS[k], (unsigned long long)RTCP_US[k]);
	for (i = 0; i < C.ncp[k]; i++) {
		printf("%s", i ? "," : "");
		rtcp_packet(s, C.cp[k][i], RECV_MS[k]);
		mem_deref(C.cp[k][i]);
	}
	printf("]}");
}

static void st_check(struct sess *s)
{
	printf(",{\"op\":\"check\",\"memberc\":%u,\"senderc\":%u,\"m\":[",
	       s->memberc, s->senderc);
	sep = 0;
	(void)hash_apply(s->members, check_h, NULL);
	printf("],\"tx\":[%u,%u,%llu,%u,%d]}", s->psent, s->osent,
	       (unsigned long long)s->jfs_rt_ref, s->ts_ref, s->ts_synced);
}

/* mk_sr */
static void st_report(struct sess *s, int k)
{
	struct mbuf *mb = mbuf_alloc(512);
	const uint64_t jfs_rt = REP_US[k];
	struct rtp_ntp_time ntp = {0, 0};
	uint32_t rtp_ts = 0;
	const bool sr = s->jfs_rt_ref != 0;
	int err;

	if (!mb)
		abort();
	now_ms = REP_MS[k];
	s->ts_synced = false;
	printf(",{\"op\":\"report\",\"now_ms\":%llu,\"now_us\":%llu,"
	       "\"pt\":%d,\"senderc\":%u,\"rb\":[",
	       (unsigned long long)now_ms, (unsigned long long)jfs_rt,
	       sr ? 200 : 201, s->senderc);
	sep = 0;
	kinds[sr ? K_REPORT_SR : K_REPORT_RR] = 1;
	if (sr) {
		uint64_t dur;

		ntp_now(&ntp, jfs_rt);
		kinds[K_NOW_BEFORE_REF] |= jfs_rt < s->jfs_rt_ref;
		dur = jfs_rt - s->jfs_rt_ref;
		rtp_ts = (uint32_t)((uint64_t)s->ts_ref + dur *
				    s->srate_tx / 1000000u);
		err = rtcp_encode(mb, RTCP_SR, s->senderc, C.local_ssrc, ntp.hi,
				  ntp.lo, rtp_ts, s->psent, s->osent,
				  encode_handler, s->members);
	}
	else {
		err = rtcp_encode(mb, RTCP_RR, s->senderc, C.local_ssrc,
				  encode_handler, s->members);
	}
	if (err)
		abort();
	printf("],\"w\":[%u,%u,%u,%u,%u,%u],\"bytes\":\"", C.local_ssrc, ntp.hi,
	       ntp.lo, rtp_ts, sr ? s->psent : 0, sr ? s->osent : 0);
	hex(mb->buf, mb->end);
	printf("\"}");
	mem_deref(mb);
}

/* rtcp_stats */
static void st_stats(struct sess *s)
{
	size_t i;

	printf(",{\"op\":\"stats\",\"q\":[");
	for (i = 0; i < C.nq; i++) {
		const struct rtp_member *mbr =
			rtp_member_find(s->members, C.q[i]);
		struct rtcp_stats st;

		memset(&st, 0, sizeof(st));
		if (mbr) {
			st.tx.sent = s->psent;
			st.tx.lost = mbr->cum_lost;
			st.tx.jit  = mbr->jit;
			st.rtt = mbr->rtt;
			if (mbr->s) {
				st.rx.sent = mbr->s->received;
				st.rx.lost = rtp_source_calc_lost(mbr->s);
				st.rx.jit  = s->srate_rx ?
					1000000 * (mbr->s->jitter>>4) /
					s->srate_rx : 0;
			}
		}
		printf("%s[%u,%d,%u,%d,%u,%u,%d,%u,%u]", i ? "," : "", C.q[i],
		       mbr ? 0 : ENOENT, st.tx.sent, st.tx.lost, st.tx.jit,
		       st.rx.sent, st.rx.lost, st.rx.jit, st.rtt);
	}
	printf("]}");
}

static int casesep;
static int seen[K_COUNT];

static void end(void)
{
	struct sess s;
	int k, n = 0;

	memset(&s, 0, sizeof(s));
	memset(kinds, 0, sizeof(kinds));
	s.srate_tx = C.srate_tx;
	s.srate_rx = C.srate_rx;
	if (hash_alloc(&s.members, MAX_MEMBERS))
		abort();
	printf("%s\n{\"name\":\"%s\",\"srate_tx\":%u,\"srate_rx\":%u,"
	       "\"local_ssrc\":%u,\"stages\":[", casesep++ ? "," : "", C.name,
	       C.srate_tx, C.srate_rx, C.local_ssrc);
	st_rtp(&s, 0);
	st_tx(&s, 0);
	st_rtcp(&s, 0);
	st_check(&s);
	st_report(&s, 0);
	st_check(&s);
	st_rtcp(&s, 1);
	printf(",");
	st_rtp(&s, 1);
	st_tx(&s, 1);
	st_check(&s);
	st_report(&s, 1);
	st_stats(&s);
	printf("],\"kinds\":[");
	for (k = 0; k < K_COUNT; k++) {
		if (kinds[k]) {
			printf("%s\"%s\"", n++ ? "," : "", kind_name[k]);
			seen[k] = 1;
		}
	}
	printf("]}");
	hash_flush(s.members);
	mem_deref(s.members);
}

/* ---- the cases ---------------------------------------------------------- */

/* compact NTP times around the two rtcp stages' clocks (T0: hi 0xfffd,
 * T0 + 6 s: hi 0x0003 after the wrap; the fraction of 654321 us is 0xa781) */
#define NTPC(hi, lo) ((uint32_t)(hi) << 16 | (lo))

static void queries(const uint32_t *v, size_t n)
{
	memcpy(C.q, v, n * sizeof(*v));
	C.nq = n;
}

#define Q(...) queries((const uint32_t[]){__VA_ARGS__}, \
		       sizeof((const uint32_t[]){__VA_ARGS__}) / 4)

int main(void)
{
	uint32_t i;
	int k;

	printf("{\"source\":\"reference src/rtp/pkt.c, rr.c, sdes.c, fb.c, "
	       "member.c, source.c, rtp.c, ntp.c, src/hash/hash.c driven as "
	       "src/rtp/sess.c drives them\",\"cases\":[");

	/* an RR without blocks from an unknown SSRC takes a member; nothing
	 * is ever sent: both reports are RRs */
	begin("rr_count0_new_member", 8000, 8000);
	pk(10, 1000, 0x501, 5000);
	pk(11, 1160, 0x501, 5170);
	compound();
	m_rr(0x777, NULL, 0);
	m_sdes(0x777);
	stage = 1;
	compound();
	m_rr(0x777, (struct rtcp_rr[]){{C.local_ssrc, 3, 17, 4000, 80,
		     NTPC(0x0001, 0x8000), 65536}}, 1);
	pk(12, 1320, 0x501, 5300);
	Q(0x777, 0x501, 0x999);
	end();

	/* seven members by RTP, the 8th by SR, a 9th by SR and by RR in one
	 * compound whose RR of a known member still counts */
	begin("ninth_by_sr_and_rr", 48000, 48000);
	for (i = 0; i < 7; i++)
		pk(10 * i, 50 * i + 1, 0x40 + i, 60 * i + 3);
	tx(0, 0, 1000, 160, T0_US - 20000);
	compound();
	m_sr(0x47, 0x83aa7e80, 0x40000000, 777, 5, 800, NULL, 0);
	compound();
	m_sr(0x99, 1, 2, 3, 4, 5, (struct rtcp_rr[]){{1, 1, 1, 1, 1, 1, 1}}, 1);
	m_rr(0x9a, (struct rtcp_rr[]){{1, 1, 1, 1, 1, 1, 1}}, 1);
	m_rr(0x42, (struct rtcp_rr[]){{C.local_ssrc, 0, 9, 77, 480,
		     NTPC(0xfffc, 0x4000), 32768}}, 1);
	stage = 1;
	compound();
	m_rr(0x9a, NULL, 0);
	pk(1, 2, 0x9b, 3);
	Q(0x47, 0x42, 0x99, 0x9a, 0x40);
	end();

	/* SR before the first RTP packet (a member without a source: nothing
	 * stored) and after it */
	begin("sr_then_rtp_and_rtp_then_sr", 90000, 90000);
	pk(300, 2000, 0x71, 3000);
	pk(301, 2160, 0x71, 3170);
	tx(0, 0, 5000, 100, T0_US - 1000000);
	tx(0, 0, 5160, 100, T0_US - 980000);
	compound();
	m_sr(0x71, 0xe3aa7e86, 0x9abcdef0, 49111, 260, 41600, NULL, 0);
	m_sr(0x72, 0xe3aa7e80, 0x12345678, 1111, 10, 1600, NULL, 0);
	stage = 1;
	pk(9, 9, 0x72, 9);
	pk(302, 2320, 0x71, 3400);
	compound();
	m_sr(0x72, 0xe3aa7e8c, 0x22345678, 2111, 20, 3200, NULL, 0);
	Q(0x71, 0x72);
	end();

	/* several blocks per message: the last one wins for cum_lost / jit,
	 * the last one with lsr and dlsr for rtt; negative 24-bit lost; a
	 * jitter whose product with 1000000 wraps */
	begin("several_blocks_per_message", 8000, 8000);
	tx(2, 0, 70000, 33, T0_US - 5000000);
	compound();
	m_rr(0x81, (struct rtcp_rr[]){
		{C.local_ssrc, 1, 100, 5000, 40, NTPC(0xfffd, 0x2000), 6554},
		{0x12345, 2, -5, 5001, 5000, 0, 6554},
		{0x12346, 3, -0x7fffff, 5002, 0xfffffff0, NTPC(0xfffd, 0x2000),
		 0}}, 3);
	m_sr(0x82, 0xe3aa7e86, 1, 2, 3, 4, (struct rtcp_rr[]){
		{C.local_ssrc, 1, 0x7fffff, 5000, 4295, NTPC(0xfffb, 0), 65536},
		{C.local_ssrc, 9, -1, 5001, 4296, 0, 0}}, 2);
	stage = 1;
	compound();
	m_rr(0x81, (struct rtcp_rr[]){
		{C.local_ssrc, 1, -0x800000, 5000, 0x80000000,
		 NTPC(0x0002, 0x1000), 1}}, 1);
	Q(0x81, 0x82);
	end();

	/* srate_tx 0: jit is never set; srate_rx 0: no jitter is calculated
	 * (the packets carry timestamp 0, for which an entry given arrival
	 * times skips the calculation too) and rx_jit is 0 */
	begin("srate_zero", 0, 0);
	pk(100, 0, 0x91, 0);
	pk(101, 0, 0x91, 0);
	compound();
	m_rr(0x91, (struct rtcp_rr[]){{C.local_ssrc, 1, 33, 5000, 4000,
		     NTPC(0xfffd, 0x1000), 100}}, 1);
	stage = 1;
	tx(0, 0, 1, 1, T0_US + 7000000);
	Q(0x91);
	end();

	/* RTT: positive, clamped to 0 (lsr in the future), and across the
	 * compact-NTP wrap between the two rtcp stages */
	begin("rtt_positive_clamped_wrap", 8000, 8000);
	tx(0, 0, 160, 20, T0_US - 3000000);
	compound();
	m_rr(0xa1, (struct rtcp_rr[]){{C.local_ssrc, 0, 0, 10, 8,
		     NTPC(0xfffc, 0xa781), 32768}}, 1);   /* 1 s - 0.5 s */
	m_rr(0xa2, (struct rtcp_rr[]){{C.local_ssrc, 0, 0, 10, 8,
		     NTPC(0xfffd, 0xa782), 1}}, 1);       /* just ahead */
	m_rr(0xa3, (struct rtcp_rr[]){{C.local_ssrc, 0, 0, 10, 8,
		     NTPC(0xfffd, 0x0001), 65536 * 3}}, 1); /* dlsr too long */
	stage = 1;
	compound();
	m_rr(0xa1, (struct rtcp_rr[]){{C.local_ssrc, 0, 0, 10, 8,
		     NTPC(0xfffe, 0x0000), 65536}}, 1);   /* before the wrap */
	m_rr(0xa2, (struct rtcp_rr[]){{C.local_ssrc, 0, 0, 10, 8,
		     NTPC(0x0002, 0xa781), 6554}}, 1);    /* after it */
	m_rr(0xa4, (struct rtcp_rr[]){{C.local_ssrc, 0, 0, 10, 8,
		     NTPC(0xfb00, 0x0000), 1}}, 1);       /* long before it */
	Q(0xa1, 0xa2, 0xa3, 0xa4);
	end();

	/* BYE of members with and without a source, of an unknown source and
	 * of one named twice, at the first, a middle and the last slot; then
	 * RTP from a source that left */
	begin("bye_positions", 8000, 8000);
	for (i = 0; i < 3; i++)
		pk(100 + i, 1000 + 160 * i, 0xb0 + i, 3000 + 161 * i);
	compound();
	m_rr(0xb3, (struct rtcp_rr[]){{C.local_ssrc, 0, 3, 10, 80,
		     NTPC(0xfffd, 0x1000), 6554}}, 1);
	m_rr(0xb4, (struct rtcp_rr[]){{C.local_ssrc, 0, 4, 11, 160,
		     NTPC(0xfffd, 0x2000), 6554}}, 1);
	m_sr(0xb1, 0xe3aa7e86, 5, 6, 7, 8, (struct rtcp_rr[]){{C.local_ssrc, 0,
		     1, 12, 240, NTPC(0xfffd, 0x3000), 6554}}, 1);
	compound();
	m_bye((uint32_t[]){0xb2}, 1, NULL);               /* middle, source */
	stage = 1;
	compound();
	m_bye((uint32_t[]){0xb0, 0xb0, 0xdead}, 3, "bye");  /* first; twice */
	m_sdes(0xb1);
	m_bye((uint32_t[]){0xb4}, 1, NULL);               /* last, no source */
	compound();
	m_rr(0xb5, NULL, 0);
	m_bye(NULL, 0, NULL);
	m_bye((uint32_t[]){0xb3}, 1, "x");                /* middle, no source */
	pk(500, 9000, 0xb2, 20000);                       /* fresh source */
	pk(501, 9160, 0xb2, 20170);
	pk(103, 1480, 0xb1, 3490);
	Q(0xb0, 0xb1, 0xb2, 0xb3, 0xb4, 0xb5);
	end();

	/* a full table, one member leaves, and the one that takes its place
	 * lands in the hash bucket of older members, behind them */
	begin("readd_after_bye_same_bucket", 8000, 8000);
	for (i = 0; i < 8; i++)         /* buckets 3,3,3,0,0,5,7,3 */
		pk(100 + i, 1000 * i + 7,
		   (uint32_t[]){0x103, 0x20b, 0x3, 0x8, 0x10, 0x5, 0xf, 0x1b}[i],
		   2000 * i + 9);
	compound();
	m_bye((uint32_t[]){0x20b}, 1, NULL);
	m_rr(0x20b, (struct rtcp_rr[]){{C.local_ssrc, 0, 2, 10, 80,
		     NTPC(0xfffd, 0x1000), 6554}}, 1);    /* back, at the end */
	m_rr(0x33, NULL, 0);                              /* 9th */
	stage = 1;
	compound();
	m_bye((uint32_t[]){0x103, 0x1b}, 2, NULL);        /* first and a middle */
	m_sr(0x103, 0xe3aa7e86, 5, 6, 7, 8, NULL, 0);
	pk(101, 1167, 0x20b, 2200);
	pk(101, 167, 0x103, 300);
	pk(1, 1, 0x43, 1);
	pk(2, 2, 0x4b, 2);                                /* 9th */
	Q(0x103, 0x20b, 0x3, 0x1b, 0x43, 0x4b);
	end();

	/* SDES, APP and feedback messages between the reports: dispatched,
	 * ignored */
	begin("other_messages_between_reports", 16000, 16000);
	pk(7, 700, 0xc1, 900);
	tx(1, 1, 16000, 24, T0_US - 100000);
	compound();
	m_sdes(0xc1);
	m_sr(0xc1, 0xe3aa7e86, 0x80000000, 9, 10, 11, (struct rtcp_rr[]){{
		     C.local_ssrc, 0, 6, 10, 160, NTPC(0xfffd, 0x1000), 6554}},
	     1);
	m_app(0xc1);
	m_pli(0xc1, C.local_ssrc);
	m_rr(0xc2, (struct rtcp_rr[]){{C.local_ssrc, 0, 7, 10, 320,
		     NTPC(0xfffd, 0x2000), 6554}}, 1);
	m_sdes(0xc2);
	stage = 1;
	compound();
	m_pli(0xc3, C.local_ssrc);                        /* no member for it */
	m_app(0xc4);
	tx(0, 0, 96000, 50, T0_US + 6500000);
	Q(0xc1, 0xc2, 0xc3);
	end();

	/* the first report comes before anything was sent (RR), the second
	 * after (SR); a third stage of sending after the first SR re-syncs */
	begin("report_rr_then_sr", 8000, 8000);
	pk(7, 700, 0xd1, 900);
	pk(8, 860, 0xd1, 1100);
	stage = 1;
	tx(0, 0, 8000, 160, T0_US + 6100000);
	tx(0, 0, 8160, 160, T0_US + 6120000);
	tx(3, 1, 8320, 12, T0_US + 6140000);
	Q(0xd1);
	end();

	begin("report_sr_resync", 8000, 8000);
	tx(0, 0, 0xfffffff0, 160, T0_US - 2000000);
	tx(0, 0, 144, 160, T0_US - 1980000);
	stage = 1;
	tx(15, 0, 50000, 0, T0_US + 6200000);             /* the new reference */
	tx(0, 0, 50160, 160, T0_US + 6220000);
	Q(1);
	end();

	/* the reference time lies after the report's clock: the duration
	 * wraps in 64 bits */
	begin("now_before_reference", 90000, 90000);
	tx(0, 0, 123456, 10, T0_US + 5000001);
	tx(0, 0, 123457, 10, T0_US + 5000002);
	stage = 1;
	tx(0, 0, 999, 10, T0_US + 3600000000ULL);
	Q(2);
	end();

	printf("\n]}\n");
	for (k = 0; k < K_COUNT; k++) {
		if (!seen[k]) {
			fprintf(stderr, "no case went through %s\n",
				kind_name[k]);
			return 1;
		}
	}
	return 0;
}
