/*
 * rtcp_sess_check.c -- the RTCP session rule (re_amd/csrc/hip/
 * rtcp_sess_rule.h) on the CPU, in the decomposition of rtcp_sess.hip: the
 * packets that take part grouped by session (stable), per session eight
 * slot owners that find a message's member by a ballot over the slots, a
 * removal as a shuffle (every slot first fetches the state of the slot
 * above, then does its part), and the transmit statistics as a reduction
 * whose leaves are combined in random association orders.  Compared, on
 * random events over several rounds on the same states, against a plain
 * sequential walk written the reference's way -- a member list searched in
 * order and erased from, one packet after the other, 64-bit arithmetic cut
 * to 32 bits.  Stand-alone, run under -fsanitize=address,undefined by
 * tests/test_rtcp_sess_rule.py.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/re_rtcp_sess_batch.h"
#include "../../re_amd/csrc/hip/rtcp_sess_rule.h"

static int wrong;

#define CHECK(c, ...)                                                       \
	do {                                                                \
		if (!(c)) {                                                 \
			if (wrong++ < 20) {                                 \
				printf("FAIL %s:%d: ", __FILE__, __LINE__); \
				printf(__VA_ARGS__);                        \
				printf("\n");                               \
			}                                                   \
		}                                                           \
	} while (0)

static uint64_t rng_s = 0x9E3779B97F4A7C15ull;

static uint64_t rnd(void)
{
	rng_s ^= rng_s >> 12;
	rng_s ^= rng_s << 25;
	rng_s ^= rng_s >> 27;
	return rng_s * 0x2545F4914F6CDD1Dull;
}

static uint32_t rndn(uint32_t n) { return (uint32_t)(rnd() % n); }

enum { NSESS = 37, NPKT = 400, MAXMSG = 4, MAXITEM = 10, NTX = 900,
       NRTP = 150, ROUNDS = 40, POOL = 11 };

/* what happened, so that the test can see that everything did */
static long c_added_rr, c_ninth, c_rm_first, c_rm_middle, c_rm_last, c_readd,
	c_rtt_clamped, c_rtt_positive, c_jit_wrapped, c_truncated, c_skipped,
	c_einval, c_resync, c_sr, c_sr_stored, c_blocks, c_bye_unknown,
	c_reports_sr, c_reports_rr, c_tx_ok, c_tx_bad, c_stats;

/* ---- the plain sequential walk ----------------------------------------- */

struct pmem {
	uint32_t ssrc;
	int has;                /* mbr->s */
	uint32_t received;
	uint64_t sr_recv;
	uint32_t hi, lo, rtp_ts, psent, osent;
	int32_t cum_lost;
	uint32_t jit, rtt;
};

struct psess {
	uint32_t memberc;
	struct pmem m[8];
	uint32_t gone[256], ngone;      /* SSRCs that said BYE, for c_readd */
	uint32_t tx_psent, tx_osent, ts_ref;
	uint64_t jfs_rt_ref;
	int ts_synced;
	uint32_t srate_tx, srate_rx;
};

static struct pmem *p_find(struct psess *ss, uint32_t ssrc)
{
	for (uint32_t k = 0; k < ss->memberc; k++)
		if (ss->m[k].ssrc == ssrc)
			return &ss->m[k];
	return NULL;
}

static struct pmem *p_member(struct psess *ss, uint32_t ssrc, int *isnew)
{
	struct pmem *m = p_find(ss, ssrc);

	*isnew = 0;
	if (m)
		return m;
	if (ss->memberc >= 8)
		return NULL;
	for (uint32_t k = 0; k < ss->ngone; k++) {
		if (ss->gone[k] == ssrc) {
			c_readd++;
			break;
		}
	}
	*isnew = 1;
	memset(&ss->m[ss->memberc], 0, sizeof(ss->m[0]));
	ss->m[ss->memberc].ssrc = ssrc;
	return &ss->m[ss->memberc++];
}

static uint64_t p_compact2us(uint32_t c)
{
	return (uint64_t)(c >> 16) * 1000000u +
	       (((uint64_t)(c & 0xffff) * 1000000u) >> 16);
}

static void p_block(struct psess *ss, struct pmem *m, uint32_t a_compact,
		    const uint32_t *v)
{
	const uint32_t lost24 = v[2], jitter = v[4], lsr = v[5], dlsr = v[6];

	m->cum_lost = (lost24 & 0x800000) ? (int32_t)lost24 - 0x1000000
					  : (int32_t)lost24;
	if (ss->srate_tx) {
		const uint64_t prod = 1000000ULL * jitter;

		if (prod >> 32)
			c_jit_wrapped++;
		m->jit = (uint32_t)(prod & 0xffffffffu) / ss->srate_tx;
	}
	if (lsr && dlsr) {
		const int64_t d = (int64_t)p_compact2us(a_compact) -
			(int64_t)p_compact2us(lsr) -
			(int64_t)(1000000ULL * dlsr / 65536);
		const int32_t r = (int32_t)(uint32_t)(uint64_t)d;

		if (r > 0)
			c_rtt_positive++;
		else
			c_rtt_clamped++;
		m->rtt = r > 0 ? (uint32_t)r : 0;
	}
	c_blocks++;
}

/* one decoded packet; 0 or RTP_RX_NOMEMBER */
static int p_packet(struct psess *ss, const struct rtcp_desc *d, uint32_t nm,
		    const struct rtcp_item *it, uint32_t ni, uint64_t recv_ms,
		    uint32_t a_compact)
{
	int st = 0;

	for (uint32_t m = 0; m < nm; m++) {
		struct pmem *mb = NULL;
		int isnew;

		if (d[m].pt == 200 || d[m].pt == 201) {
			mb = p_member(ss, d[m].ssrc, &isnew);
			if (!mb) {
				st = RTP_RX_NOMEMBER;
				c_ninth++;
			}
			else if (isnew && d[m].pt == 201) {
				c_added_rr++;
			}
		}
		for (uint32_t j = 0; j < ni; j++) {
			if (it[j].msg != m)
				continue;
			if (mb && d[m].pt == 200 && it[j].kind == RTCP_ITEM_SR) {
				c_sr++;
				if (mb->has) {
					c_sr_stored++;
					mb->sr_recv = recv_ms;
					mb->hi = it[j].v[0];
					mb->lo = it[j].v[1];
					mb->rtp_ts = it[j].v[2];
					mb->psent = it[j].v[3];
					mb->osent = it[j].v[4];
				}
			}
			else if (mb && it[j].kind == RTCP_ITEM_RB) {
				p_block(ss, mb, a_compact, it[j].v);
			}
			else if (d[m].pt == 203 &&
				 it[j].kind == RTCP_ITEM_BYE_SRC) {
				struct pmem *x = p_find(ss, it[j].v[0]);
				uint32_t k;

				if (!x) {
					c_bye_unknown++;
					continue;
				}
				k = (uint32_t)(x - ss->m);
				if (ss->memberc >= 3) {
					if (k == 0)
						c_rm_first++;
					else if (k + 1 == ss->memberc)
						c_rm_last++;
					else
						c_rm_middle++;
				}
				if (ss->ngone < 256)
					ss->gone[ss->ngone++] = x->ssrc;
				memmove(x, x + 1,
					(ss->memberc - k - 1) * sizeof(*x));
				ss->memberc--;
			}
		}
	}
	return st;
}

/* ---- the decomposition -------------------------------------------------- */

struct lane {
	struct rtp_rx_source src;
	struct rsx_mbr mb;
};

static uint32_t ballot_hit(const struct lane *l, uint32_t memberc,
			   uint32_t ssrc)
{
	uint32_t b = 0;

	for (uint32_t k = 0; k < 8; k++)
		b |= (uint32_t)rrx_slot_hit(memberc, k, l[k].src.ssrc, ssrc) << k;
	return b;
}

static void lanes_load(struct lane *l, const struct rtp_rx_sess *ss,
		       const struct rtcp_sess_ext *x)
{
	for (uint32_t k = 0; k < 8; k++) {
		l[k].src = ss->m[k];
		l[k].mb.cum_lost = (uint32_t)x->cum_lost[k];
		l[k].mb.jit = x->jit[k];
		l[k].mb.rtt = x->rtt[k];
	}
}

static void lanes_store(const struct lane *l, struct rtp_rx_sess *ss,
			struct rtcp_sess_ext *x)
{
	for (uint32_t k = 0; k < 8; k++) {
		ss->m[k] = l[k].src;
		x->cum_lost[k] = (int32_t)l[k].mb.cum_lost;
		x->jit[k] = l[k].mb.jit;
		x->rtt[k] = l[k].mb.rtt;
	}
}

/* the member of ssrc as the eight lanes find or add it: its slot, or -1 */
static int lanes_member(struct lane *l, uint32_t *memberc, uint32_t ssrc)
{
	const uint32_t any = ballot_hit(l, *memberc, ssrc);
	int own = -1;

	for (uint32_t k = 0; k < 8; k++) {
		if (any >> k & 1)
			own = (int)k;
		if (rrx_slot_new(*memberc, k, any != 0)) {
			rrx_member_init(&l[k].src, ssrc);
			l[k].mb.cum_lost = l[k].mb.jit = l[k].mb.rtt = 0;
			own = (int)k;
		}
	}
	if (!any && own >= 0)
		(*memberc)++;
	return own;
}

static int d_packet(struct lane *l, uint32_t *memberc, uint32_t srate_tx,
		    const struct rtcp_desc *d, uint32_t nm,
		    const struct rtcp_item *it, uint32_t ni, uint64_t recv_ms,
		    uint32_t a_compact)
{
	uint32_t j = 0;
	int st = 0;

	for (uint32_t m = 0; m < nm; m++) {
		const uint32_t pt = d[m].pt;
		int own = -1;

		if (rsx_is_report(pt)) {
			own = lanes_member(l, memberc, d[m].ssrc);
			if (own < 0)
				st = RTP_RX_NOMEMBER;
		}
		for (; j < ni && it[j].msg == (uint16_t)m; j++) {
			const struct rtcp_item *e = &it[j];

			if (own >= 0 && pt == 200 && e->kind == RTCP_ITEM_SR) {
				rrx_source_sr(&l[own].src, recv_ms, e->v[0],
					      e->v[1], e->v[2], e->v[3],
					      e->v[4]);
			}
			else if (own >= 0 && e->kind == RTCP_ITEM_RB) {
				rsx_rr_block(&l[own].mb, srate_tx, a_compact,
					     e->v[2], e->v[4], e->v[5],
					     e->v[6]);
			}
			else if (pt == 203 && e->kind == RTCP_ITEM_BYE_SRC) {
				const uint32_t any = ballot_hit(l, *memberc,
								e->v[0]);
				struct lane up[8];
				uint32_t j0 = 0;

				if (!any)
					continue;
				while (!(any >> j0 & 1))
					j0++;
				/* the shuffle: every lane gets the lane above
				 * (the last one its own) */
				for (uint32_t k = 0; k < 8; k++)
					up[k] = l[k < 7 ? k + 1 : k];
				for (uint32_t k = 0; k < 8; k++) {
					const int act = rsx_remove_slot(
						k, j0, *memberc);
					if (act == RSX_TAKE_NEXT)
						l[k] = up[k];
					else if (act == RSX_ZERO)
						memset(&l[k], 0, sizeof(l[k]));
				}
				(*memberc)--;
			}
		}
	}
	return st;
}

/* ---- the states and their comparison ----------------------------------- */

static struct psess P[NSESS];
static struct rtp_rx_sess S[NSESS];
static struct rtcp_sess_ext X[NSESS];

static void compare(int round)
{
	static const struct rtp_rx_source zs;

	for (uint32_t s = 0; s < NSESS; s++) {
		const struct psess *p = &P[s];

		CHECK(S[s].memberc == p->memberc, "round %d sess %u memberc %u %u",
		      round, s, S[s].memberc, p->memberc);
		for (uint32_t k = 0; k < 8; k++) {
			const struct rtp_rx_source *g = &S[s].m[k];
			const struct pmem *m = &p->m[k];

			if (k >= p->memberc) {
				CHECK(!memcmp(g, &zs, sizeof(zs)) &&
				      !X[s].cum_lost[k] && !X[s].jit[k] &&
				      !X[s].rtt[k],
				      "round %d sess %u slot %u not zero", round,
				      s, k);
				continue;
			}
			CHECK(g->ssrc == m->ssrc &&
			      !(g->flags & RTP_RX_HAS_SOURCE) == !m->has &&
			      g->received == m->received &&
			      g->sr_recv == m->sr_recv && g->sr_ntp_hi == m->hi &&
			      g->sr_ntp_lo == m->lo && g->sr_rtp_ts == m->rtp_ts &&
			      g->sr_psent == m->psent && g->sr_osent == m->osent,
			      "round %d sess %u slot %u source", round, s, k);
			CHECK(X[s].cum_lost[k] == m->cum_lost &&
			      X[s].jit[k] == m->jit && X[s].rtt[k] == m->rtt,
			      "round %d sess %u slot %u ext %d/%d %u/%u %u/%u",
			      round, s, k, X[s].cum_lost[k], m->cum_lost,
			      X[s].jit[k], m->jit, X[s].rtt[k], m->rtt);
		}
		CHECK(X[s].psent == p->tx_psent && X[s].osent == p->tx_osent &&
		      X[s].jfs_rt_ref == p->jfs_rt_ref &&
		      X[s].ts_ref == p->ts_ref &&
		      X[s].ts_synced == (uint32_t)p->ts_synced,
		      "round %d sess %u txstat", round, s);
	}
}

/* ---- received RTP: gives members a source ------------------------------- */

static void round_rtp(void)
{
	for (uint32_t i = 0; i < NRTP; i++) {
		const uint32_t s = rndn(NSESS);
		const uint32_t ssrc = 0x100 * (s + 1) + rndn(POOL);
		struct lane l[8];
		uint32_t mc = S[s].memberc;
		struct pmem *m;
		int own, isnew;

		m = p_member(&P[s], ssrc, &isnew);
		if (m) {
			m->has = 1;
			m->received++;
		}
		lanes_load(l, &S[s], &X[s]);
		own = lanes_member(l, &mc, ssrc);
		if (own >= 0) {
			l[own].src.flags |= RTP_RX_HAS_SOURCE;
			l[own].src.received++;
		}
		lanes_store(l, &S[s], &X[s]);
		S[s].memberc = mc;
		CHECK((own >= 0) == (m != NULL), "rtp member");
	}
}

/* ---- incoming RTCP ------------------------------------------------------ */

static struct rtcp_desc descv[NPKT * MAXMSG];
static struct rtcp_item itemv[NPKT * MAXITEM];
static uint32_t nmsgv[NPKT], nitemv[NPKT], sessv[NPKT];
static int32_t resv[NPKT], stat_p[NPKT], stat_d[NPKT];

static void make_packet(uint32_t i, uint32_t a_compact)
{
	struct rtcp_desc *d = &descv[i * MAXMSG];
	struct rtcp_item *it = &itemv[i * MAXITEM];
	const uint32_t s = sessv[i] < NSESS ? sessv[i] : 0;
	uint32_t nm = 1 + rndn(3), ni = 0;

	if (rndn(25) == 0)
		nm = MAXMSG + 1 + rndn(3);      /* more than the array holds */
	for (uint32_t m = 0; m < nm; m++) {
		struct rtcp_desc dd;
		struct rtcp_item e[8];
		uint32_t ne = 0;
		const uint32_t w = rndn(100);

		memset(&dd, 0, sizeof(dd));
		memset(e, 0, sizeof(e));
		dd.ssrc = 0x100 * (s + 1) + rndn(POOL);
		if (w < 65) {
			const uint32_t nb = rndn(40) ? rndn(4) : 6;

			dd.pt = w < 30 ? 200 : 201;
			dd.count = (uint8_t)nb;
			if (dd.pt == 200) {
				e[ne].kind = RTCP_ITEM_SR;
				for (int k = 0; k < 5; k++)
					e[ne].v[k] = (uint32_t)rnd();
				ne++;
			}
			for (uint32_t b = 0; b < nb; b++, ne++) {
				e[ne].kind = RTCP_ITEM_RB;
				e[ne].v[0] = (uint32_t)rnd();
				e[ne].v[1] = rndn(256);
				e[ne].v[2] = rndn(1 << 24);
				e[ne].v[3] = (uint32_t)rnd();
				e[ne].v[4] = rndn(3) ? rndn(9000)
						     : (uint32_t)rnd();
				e[ne].v[5] = rndn(5) ? a_compact - 300000 +
						       rndn(400000) : 0;
				e[ne].v[6] = rndn(5) ? 1 + rndn(200000) : 0;
				if (rndn(50) == 0)
					e[ne].v[5] = (uint32_t)rnd();
			}
		}
		else if (w < 88) {
			const uint32_t nb = rndn(4);

			dd.pt = 203;
			dd.count = (uint8_t)nb;
			for (uint32_t b = 0; b < nb; b++, ne++) {
				e[ne].kind = RTCP_ITEM_BYE_SRC;
				e[ne].v[0] = b && rndn(3) == 0 ? e[ne - 1].v[0] :
					0x100 * (s + 1) + rndn(POOL);
			}
			dd.ssrc = nb ? e[0].v[0] : 0;
		}
		else {
			/* another message: its item would do harm if it were
			 * taken for a block or a source */
			dd.pt = (uint8_t)(rndn(2) ? 202 : 206);
			e[ne].kind = rndn(2) ? RTCP_ITEM_SDES_CHUNK :
					       RTCP_ITEM_FB;
			e[ne].v[0] = dd.ssrc;
			e[ne].v[2] = 5;
			ne++;
		}
		if (m < MAXMSG)
			d[m] = dd;
		for (uint32_t k = 0; k < ne; k++, ni++) {
			e[k].msg = (uint16_t)m;
			if (ni < MAXITEM)
				it[ni] = e[k];
		}
	}
	nmsgv[i] = nm;
	nitemv[i] = ni;
}

static int cmp_u32(const void *a, const void *b)
{
	const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
	return x < y ? -1 : x > y;
}

static void round_rtcp(int round)
{
	const uint64_t recv_ms = 1000 + 5000ull * (uint64_t)round;
	const uint64_t now_us = (rnd() >> 14) + (uint64_t)round * 5000000u;
	uint32_t hi, lo, a_compact;
	uint64_t order[NPKT];
	uint32_t live = 0;

	rsx_unix2ntp(now_us, &hi, &lo);
	a_compact = rsx_ntp_compact(hi, lo);
	for (uint32_t i = 0; i < NPKT; i++) {
		sessv[i] = rndn(30) ? rndn(NSESS) : NSESS + rndn(3);
		resv[i] = rndn(20) ? 0 : 217;
		make_packet(i, a_compact);
	}
	/* the plain walk: one packet after the other */
	for (uint32_t i = 0; i < NPKT; i++) {
		if (resv[i]) {
			stat_p[i] = RTP_RX_SKIPPED;
			c_skipped++;
		}
		else if (sessv[i] >= NSESS) {
			stat_p[i] = EINVAL;
			c_einval++;
		}
		else if (nmsgv[i] > MAXMSG || nitemv[i] > MAXITEM) {
			stat_p[i] = RTCP_RX_TRUNCATED;
			c_truncated++;
		}
		else {
			stat_p[i] = p_packet(&P[sessv[i]], &descv[i * MAXMSG],
					     nmsgv[i], &itemv[i * MAXITEM],
					     nitemv[i], recv_ms, a_compact);
		}
	}
	/* the decomposition: stat and key per packet, stable grouping (the
	 * sort of key << 32 | index), then each session's run */
	for (uint32_t i = 0; i < NPKT; i++) {
		const int skip = resv[i] != 0;

		stat_d[i] = rsx_packet_stat(skip, sessv[i] >= NSESS,
					    skip ? 0 : nmsgv[i], MAXMSG,
					    skip ? 0 : nitemv[i], MAXITEM);
		if (!stat_d[i])
			order[live++] = (uint64_t)sessv[i] << 32 | i;
	}
	for (uint32_t i = 0; i + 1 < live; i++)         /* a stable sort */
		for (uint32_t k = i + 1; k < live; k++)
			if (order[k] < order[i]) {
				const uint64_t t = order[i];
				order[i] = order[k];
				order[k] = t;
			}
	{
		uint32_t sorder[NSESS];

		for (uint32_t s = 0; s < NSESS; s++)
			sorder[s] = (uint32_t)rnd() << 8 | s;
		qsort(sorder, NSESS, sizeof(sorder[0]), cmp_u32);
		for (uint32_t q = 0; q < NSESS; q++) {  /* in any order */
			const uint32_t s = sorder[q] & 0xff;
			struct lane l[8];
			uint32_t mc = S[s].memberc;

			lanes_load(l, &S[s], &X[s]);
			for (uint32_t p = 0; p < live; p++) {
				const uint32_t i = (uint32_t)order[p];
				int st;

				if (order[p] >> 32 != s)
					continue;
				st = d_packet(l, &mc, X[s].srate_tx,
					      &descv[i * MAXMSG], nmsgv[i],
					      &itemv[i * MAXITEM], nitemv[i],
					      recv_ms, a_compact);
				if (st)
					stat_d[i] = st;
			}
			lanes_store(l, &S[s], &X[s]);
			S[s].memberc = mc;
		}
	}
	for (uint32_t i = 0; i < NPKT; i++)
		CHECK(stat_p[i] == stat_d[i], "round %d packet %u stat %d %d",
		      round, i, stat_p[i], stat_d[i]);
}

/* ---- outgoing RTP ------------------------------------------------------- */

static uint8_t arena[NTX * 96 + 64];
static uint32_t tpos[NTX], tend[NTX], tsess[NTX];
static uint64_t tjfs[NTX];
static int32_t tres[NTX];

/* leaves[0 .. n) combined in a random association (and, being
 * commutative, pairing) order */
static struct rsx_tx combine_random(struct rsx_tx *leaves, uint32_t n)
{
	if (!n)
		return rsx_tx_zero();
	while (n > 1) {
		const uint32_t a = rndn(n);
		uint32_t b = rndn(n - 1);

		if (b >= a)
			b++;
		leaves[a] = rsx_tx_combine(leaves[a], leaves[b]);
		leaves[b] = leaves[--n];
	}
	return leaves[0];
}

static void round_tx(int round)
{
	static struct rsx_tx leaves[NTX];
	static uint32_t tts[NTX];
	static int tst[NTX];
	uint32_t at = 7;
	const uint64_t asz = sizeof(arena);

	memset(arena, 0xee, sizeof(arena));
	for (uint32_t i = 0; i < NTX; i++) {
		const uint32_t cc = rndn(3) ? 0 : rndn(16);
		uint32_t len = 12 + 4 * cc + rndn(20);
		uint8_t *p = &arena[at];

		tsess[i] = rndn(40) ? rndn(NSESS) : NSESS + rndn(2);
		if (round % 3 == 0)             /* all in one session */
			tsess[i] = 5;
		tres[i] = rndn(25) ? 0 : 74;
		tjfs[i] = rnd() | 1;
		p[0] = (uint8_t)(0x80 | cc | (rndn(4) ? 0 : 0x10));
		for (int k = 1; k < 12; k++)
			p[k] = (uint8_t)rnd();
		if (rndn(20) == 0)
			p[0] ^= rndn(2) ? 0x40 : 0xc0;  /* another version */
		if (rndn(20) == 0)
			len = rndn(12 + 4 * cc);        /* cut */
		tpos[i] = at;
		tend[i] = at + len;
		at += len + rndn(3);
		if (rndn(60) == 0)
			tend[i] = rndn(2) ? tpos[i] - 1 : (uint32_t)asz + 1;
	}
	/* the plain walk */
	for (uint32_t i = 0; i < NTX; i++) {
		struct psess *p;
		const uint8_t *b = &arena[tpos[i]];
		int64_t len = (int64_t)tend[i] - tpos[i];
		int bad = 0;

		if (tres[i] || tsess[i] >= NSESS || len < 0 || tend[i] > asz)
			bad = 1;
		else if (len < 12 || len < 12 + 4 * (b[0] & 15) || b[0] >> 6 != 2)
			bad = 1;
		if (bad) {
			c_tx_bad++;
			continue;
		}
		c_tx_ok++;
		p = &P[tsess[i]];
		p->tx_osent += (uint32_t)(len - 12 - 4 * (b[0] & 15));
		p->tx_psent += 1;
		if (!p->ts_synced) {
			if (p->tx_psent > 1)
				c_resync++;
			p->jfs_rt_ref = tjfs[i];
			p->ts_ref = (uint32_t)b[4] << 24 | b[5] << 16 | b[6] << 8 |
				    b[7];
			p->ts_synced = 1;
		}
	}
	/* the reduction */
	for (uint32_t i = 0; i < NTX; i++) {
		uint32_t payload;

		tst[i] = rsx_tx_packet(arena, asz, tpos[i], tend[i],
				       tres[i] != 0, tsess[i] >= NSESS, &tts[i],
				       &payload);
		leaves[i] = rsx_tx_one(payload, i);
	}
	for (uint32_t s = 0; s < NSESS; s++) {
		static struct rsx_tx mine[NTX];
		uint32_t n = 0;
		struct rsx_tx t;

		for (uint32_t i = 0; i < NTX; i++)
			if (!tst[i] && tsess[i] == s)
				mine[n++] = leaves[i];
		t = combine_random(mine, n);
		if (!t.cnt)
			continue;
		if (rsx_tx_finish(&X[s], t))
			rsx_tx_sync(&X[s], tjfs[t.first], tts[t.first]);
	}
}

/* ---- reports and statistics -------------------------------------------- */

static void round_report(int round)
{
	const uint64_t now_us = (rnd() >> 14) + 77;
	uint32_t hi, lo;

	rsx_unix2ntp(now_us, &hi, &lo);
	for (uint32_t s = 0; s < NSESS; s++) {
		struct psess *p = &P[s];
		struct rtcp_enc_msg m;
		uint32_t want[6] = {0x4c00 + s, 0, 0, 0, 0, 0};
		uint8_t pt = 201;

		if (rndn(3))
			continue;
		if (p->jfs_rt_ref) {
			pt = 200;
			want[1] = hi;
			want[2] = lo;
			want[3] = (uint32_t)(p->ts_ref + (now_us - p->jfs_rt_ref) *
					     p->srate_tx / 1000000u);
			want[4] = p->tx_psent;
			want[5] = p->tx_osent;
			c_reports_sr++;
		}
		else {
			c_reports_rr++;
		}
		p->ts_synced = 0;
		memset(&m, 0, sizeof(m));
		m.pt = 201;
		m.w[0] = 0x4c00 + s;
		rsx_report_msg(&X[s], now_us, hi, lo, &m);
		CHECK(m.pt == pt && !memcmp(m.w, want, sizeof(want)),
		      "round %d sess %u report", round, s);
	}
	for (uint32_t s = 0; s < NSESS; s++) {
		const struct psess *p = &P[s];

		for (uint32_t k = 0; k < p->memberc; k++) {
			const struct pmem *m = &p->m[k];
			uint32_t row[7], want[7];

			rsx_stats_row(&S[s].m[k], &X[s], k, row);
			want[0] = p->tx_psent;
			want[1] = (uint32_t)m->cum_lost;
			want[2] = m->jit;
			want[3] = m->has ? m->received : 0;
			want[4] = row[4];       /* the report block's, checked
						   in rtp_rx_check.c */
			want[5] = m->has && p->srate_rx ? (uint32_t)(1000000ULL *
				(S[s].m[k].jitter >> 4)) / p->srate_rx : 0;
			want[6] = m->rtt;
			CHECK(!memcmp(row, want, sizeof(row)),
			      "round %d sess %u slot %u stats", round, s, k);
			c_stats++;
		}
	}
}

int main(void)
{
	for (uint32_t s = 0; s < NSESS; s++) {
		P[s].srate_tx = X[s].srate_tx = s % 5 ? 8000u * (1 + s % 7) : 0;
		P[s].srate_rx = X[s].srate_rx = s % 4 ? 8000 : 0;
	}
	for (int round = 0; round < ROUNDS; round++) {
		round_rtp();
		round_tx(round);
		round_rtcp(round);
		compare(round);
		round_report(round);
		compare(round);
	}
	printf("rtcp: %ld added by rr, %ld ninth refused, %ld removed first, "
	       "%ld removed middle, %ld removed last, %ld readded, "
	       "%ld rtt clamped, %ld rtt positive, %ld jit wrapped, "
	       "%ld truncated, %ld skipped, %ld einval, %ld sr, "
	       "%ld sr stored, %ld blocks, %ld bye unknown;\n",
	       c_added_rr, c_ninth, c_rm_first, c_rm_middle, c_rm_last, c_readd,
	       c_rtt_clamped, c_rtt_positive, c_jit_wrapped, c_truncated,
	       c_skipped, c_einval, c_sr, c_sr_stored, c_blocks, c_bye_unknown);
	printf("tx: %ld accepted, %ld rejected, %ld tx resyncs, "
	       "%ld sr reports, %ld rr reports, %ld stats rows;\n", c_tx_ok,
	       c_tx_bad, c_resync, c_reports_sr, c_reports_rr, c_stats);
	printf("rtcp_sess_check: %d wrong\n", wrong);
	return wrong != 0;
}
