/*
 * rtp_rx_check.c -- the receiver-statistics rule (re_amd/csrc/hip/
 * rtp_rx_rule.h) on the CPU, in the decomposition of rtp_stats.hip: a record
 * per packet, a stable grouping by session, and per session eight slot
 * owners that walk the run eight records at a time and find the member by
 * a ballot over the slots.  Compared, on random traffic with arbitrary
 * 32-bit timestamps and arrival times (full-range differences included),
 * against a plain sequential walk written the reference's way -- a member
 * list searched in order, 64-bit arithmetic cut to 32 bits -- and the same
 * for the SR events and the report blocks.  Stand-alone, run under
 * -fsanitize=address,undefined by tests/test_rtp_rx_rule.py.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/re_rtp_stats_batch.h"
#include "../../re_amd/csrc/hip/rtp_rx_rule.h"

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

/* ---- the plain sequential walk ----------------------------------------- */

struct psrc {
	int has;
	uint32_t max_seq, cycles, base_seq, bad_seq, received;
	uint32_t expected_prior, received_prior, transit, jitter, last_ts;
	uint64_t bytes, sr_recv;
	uint32_t hi, lo, rtp_ts, psent, osent;
};

struct pmem {
	uint32_t ssrc;
	struct psrc s;
};

struct psess {
	uint32_t memberc;
	struct pmem m[8];
};

static uint32_t cut(int64_t v) { return (uint32_t)(uint64_t)v; }
static int64_t sgn(uint32_t v) { return (int64_t)(int32_t)v; }

static struct pmem *p_member(struct psess *ss, uint32_t ssrc)
{
	for (uint32_t k = 0; k < ss->memberc; k++)
		if (ss->m[k].ssrc == ssrc)
			return &ss->m[k];
	if (ss->memberc >= 8)
		return NULL;
	memset(&ss->m[ss->memberc], 0, sizeof(ss->m[0]));
	ss->m[ss->memberc].ssrc = ssrc;
	return &ss->m[ss->memberc++];
}

static void p_init_seq(struct psrc *s, uint32_t seq)
{
	s->base_seq = s->max_seq = seq;
	s->bad_seq = 65537;
	s->cycles = s->received = s->received_prior = s->expected_prior = 0;
}

static int p_update_seq(struct psrc *s, uint32_t seq)
{
	const uint16_t udelta = (uint16_t)(seq - s->max_seq);

	if (udelta < 3000) {
		if (seq < s->max_seq)
			s->cycles = cut((int64_t)s->cycles + 65536);
		s->max_seq = seq;
	}
	else if (udelta <= 65536 - 100) {
		if (seq == s->bad_seq)
			p_init_seq(s, seq);
		else {
			s->bad_seq = (seq + 1) & 65535;
			return 0;
		}
	}
	s->received = cut((int64_t)s->received + 1);
	return 1;
}

/* 0 ok, else the stat */
static int p_header(const uint8_t *p, int64_t len, uint32_t *seq,
		    uint32_t *ts, uint32_t *ssrc, uint32_t *payload)
{
	int64_t at = 12;

	if (len < 12)
		return EBADMSG;
	at += 4 * (p[0] & 15);
	if (at > len)
		return EBADMSG;
	if (p[0] & 16) {
		if (at + 4 > len)
			return EBADMSG;
		at += 4 + 4 * (int64_t)(p[at + 2] * 256 + p[at + 3]);
		if (at > len)
			return EBADMSG;
	}
	if (p[0] / 64 != 2)
		return EBADMSG;
	*seq = p[2] * 256u + p[3];
	*ts = (uint32_t)p[4] << 24 | p[5] << 16 | p[6] << 8 | p[7];
	*ssrc = (uint32_t)p[8] << 24 | p[9] << 16 | p[10] << 8 | p[11];
	*payload = (uint32_t)(len - at);
	return 0;
}

static int p_packet(struct psess *sv, uint32_t nsess, const uint8_t *arena,
		    uint64_t asz, uint32_t pos, uint32_t end, int skip,
		    uint32_t si, int has_arr, uint32_t arrival)
{
	uint32_t seq, ts, ssrc, payload;
	struct pmem *m;
	int ok;

	if (skip)
		return RTP_RX_SKIPPED;
	if (si >= nsess || end < pos || end > asz)
		return EINVAL;
	if (p_header(arena + pos, (int64_t)end - pos, &seq, &ts, &ssrc,
		     &payload))
		return EBADMSG;
	m = p_member(&sv[si], ssrc);
	if (!m)
		return RTP_RX_NOMEMBER;
	if (!m->s.has) {
		m->s.has = 1;
		p_init_seq(&m->s, seq);
	}
	ok = p_update_seq(&m->s, seq);
	if (has_arr && ts != m->s.last_ts) {
		const uint32_t transit = cut((int64_t)arrival - ts);
		int64_t d = sgn(cut((int64_t)transit - m->s.transit));
		const int none = !m->s.transit;
		m->s.transit = transit;
		if (!none) {
			if (d < 0)
				d = -d;
			m->s.jitter = cut((int64_t)m->s.jitter + d -
					  ((cut((int64_t)m->s.jitter + 8)) >> 4));
		}
	}
	m->s.last_ts = ts;
	m->s.bytes += payload;
	return ok ? 0 : RTP_RX_BADSEQ;
}

static void p_sr(struct psess *ss, uint32_t ssrc, uint64_t recv,
		 const uint32_t v[5])
{
	struct pmem *m = p_member(ss, ssrc);

	if (!m || !m->s.has)
		return;
	m->s.sr_recv = recv;
	m->s.hi = v[0];
	m->s.lo = v[1];
	m->s.rtp_ts = v[2];
	m->s.psent = v[3];
	m->s.osent = v[4];
}

static uint32_t p_report(struct psess *ss, uint64_t now,
			 struct rtcp_enc_rb *rb)
{
	uint32_t c = 0;

	for (uint32_t b = 0; b < 8; b++) {
		for (uint32_t k = 0; k < ss->memberc; k++) {
			struct psrc *s = &ss->m[k].s;
			uint32_t expected;
			int64_t ei, li, lost;
			if ((ss->m[k].ssrc & 7) != b || !s->has)
				continue;
			expected = cut((int64_t)s->cycles + s->max_seq -
				       s->base_seq + 1);
			ei = sgn(cut((int64_t)expected - s->expected_prior));
			li = sgn(cut(ei - sgn(cut((int64_t)s->received -
						  s->received_prior))));
			lost = sgn(cut((int64_t)expected - s->received));
			s->expected_prior = expected;
			s->received_prior = s->received;
			rb[c].ssrc = ss->m[k].ssrc;
			rb[c].fraction = (ei == 0 || li <= 0) ? 0 :
				(uint8_t)(sgn(cut(li * 256)) / ei);
			rb[c].lost = cut(lost > 0x7fffff ? 0x7fffff :
					 lost < -0x7fffff ? -0x7fffff : lost);
			rb[c].last_seq = s->cycles | s->max_seq;
			rb[c].jitter = s->jitter / 16;
			rb[c].lsr = s->hi ? (s->hi & 65535) * 65536 +
					    s->lo / 65536 : 0;
			rb[c].dlsr = s->sr_recv ? (uint32_t)(65536 *
					(now - s->sr_recv) / 1000) : 0;
			c++;
		}
	}
	return c;
}

/* plain state against struct rtp_rx_sess */
static void compare(const struct psess *pv, const struct rtp_rx_sess *dv,
		    uint32_t nsess, const char *what)
{
	for (uint32_t i = 0; i < nsess; i++) {
		CHECK(pv[i].memberc == dv[i].memberc, "%s sess %u memberc %u %u",
		      what, i, pv[i].memberc, dv[i].memberc);
		for (uint32_t k = 0; k < pv[i].memberc && k < 8; k++) {
			const struct psrc *a = &pv[i].m[k].s;
			const struct rtp_rx_source *b = &dv[i].m[k];
			CHECK(pv[i].m[k].ssrc == b->ssrc &&
			      (uint32_t)a->has == b->flags &&
			      a->max_seq == b->max_seq &&
			      a->cycles == b->cycles &&
			      a->base_seq == b->base_seq &&
			      a->bad_seq == b->bad_seq &&
			      a->received == b->received &&
			      a->expected_prior == b->expected_prior &&
			      a->received_prior == b->received_prior &&
			      a->transit == b->transit &&
			      a->jitter == b->jitter &&
			      a->last_ts == b->last_rtp_ts &&
			      a->bytes == b->rx_bytes &&
			      a->sr_recv == b->sr_recv && a->hi == b->sr_ntp_hi &&
			      a->lo == b->sr_ntp_lo && a->rtp_ts == b->sr_rtp_ts &&
			      a->psent == b->sr_psent && a->osent == b->sr_osent &&
			      b->reserved == 0,
			      "%s sess %u member %u differs", what, i, k);
		}
	}
}

/* ---- the kernel's decomposition ----------------------------------------- */

/* stable grouping of n keys in [0, nsess]: order[], and run starts */
static void group(const uint32_t *key, uint32_t n, uint32_t nsess,
		  uint32_t *order, uint32_t *start)
{
	memset(start, 0, (nsess + 2) * sizeof(*start));
	for (uint32_t i = 0; i < n; i++)
		start[key[i] + 1]++;
	for (uint32_t k = 0; k <= nsess; k++)
		start[k + 1] += start[k];
	uint32_t *at = malloc((nsess + 1) * sizeof(*at));
	memcpy(at, start, (nsess + 1) * sizeof(*at));
	for (uint32_t i = 0; i < n; i++)
		order[at[key[i]]++] = i;
	free(at);
}

/* one step of the eight lanes: the member's slot, or 8 */
static uint32_t lanes_member(struct rtp_rx_source src[8], uint32_t *memberc,
			     uint32_t ssrc)
{
	uint32_t any = 0, anynew = 0, owner = 8;

	for (uint32_t slot = 0; slot < 8; slot++)
		if (rrx_slot_hit(*memberc, slot, src[slot].ssrc, ssrc)) {
			any |= 1u << slot;
			owner = slot;
		}
	CHECK(!(any & (any - 1)), "two slots hold ssrc %u", ssrc);
	for (uint32_t slot = 0; slot < 8; slot++)
		if (rrx_slot_new(*memberc, slot, any != 0)) {
			anynew |= 1u << slot;
			rrx_member_init(&src[slot], ssrc);
			owner = slot;
		}
	CHECK(!(anynew & (anynew - 1)), "two slots take ssrc %u", ssrc);
	if (anynew)
		(*memberc)++;
	return owner;
}

static void d_stats(const uint8_t *arena, uint64_t asz, const uint32_t *pos,
		    const uint32_t *end, const int32_t *res,
		    const uint32_t *sess, const uint32_t *arrival, uint32_t n,
		    struct rtp_rx_sess *sv, uint32_t nsess, int32_t *stat)
{
	struct rrx_rec *rec = malloc((n + 1) * sizeof(*rec));
	uint32_t *key = malloc((n + 1) * sizeof(*key));
	uint32_t *order = malloc((n + 1) * sizeof(*order));
	uint32_t *start = malloc((nsess + 2) * sizeof(*start));

	for (uint32_t i = 0; i < n; i++) {
		const uint32_t si = sess ? sess[i] : 0;
		const int st = rrx_record(arena, asz, pos[i], end[i],
					  res && res[i], si >= nsess,
					  arrival ? arrival[i] : 0, &rec[i]);
		key[i] = st ? nsess : si;
		if (st)
			stat[i] = st;
		CHECK(!st == !(rec[i].seq_st & RRX_REC_DROP), "drop mark");
	}
	group(key, n, nsess, order, start);
	for (uint32_t s = 0; s < nsess; s++) {
		const uint32_t lo = start[s], hi = start[s + 1];
		struct rtp_rx_source src[8];
		uint32_t memberc = sv[s].memberc;
		int dirty[8] = {0};

		if (lo == hi)
			continue;
		memcpy(src, sv[s].m, sizeof(src));
		for (uint32_t base = lo; base < hi; base += 8) {
			for (uint32_t k = 0; k < 8 && base + k < hi; k++) {
				const uint32_t i = order[base + k];
				const struct rrx_rec *r = &rec[i];
				const uint32_t o = lanes_member(src, &memberc,
								r->ssrc);
				if (o == 8) {
					stat[i] = RTP_RX_NOMEMBER;
					continue;
				}
				dirty[o] = 1;
				stat[i] = rrx_source_rx(&src[o], r->seq_st,
						r->ts, r->arrival,
						arrival != NULL, r->payload)
					? 0 : RTP_RX_BADSEQ;
			}
		}
		for (uint32_t k = 0; k < 8; k++)
			if (dirty[k])
				sv[s].m[k] = src[k];
		sv[s].memberc = memberc;
	}
	free(rec);
	free(key);
	free(order);
	free(start);
}

static void d_sr(struct rtp_rx_sess *sv, uint32_t nsess, const uint32_t *sess,
		 const uint32_t *ssrc, const uint32_t (*v)[5], uint64_t recv,
		 uint32_t n)
{
	uint32_t *key = malloc((n + 1) * sizeof(*key));
	uint32_t *order = malloc((n + 1) * sizeof(*order));
	uint32_t *start = malloc((nsess + 2) * sizeof(*start));

	for (uint32_t i = 0; i < n; i++)
		key[i] = sess[i] < nsess ? sess[i] : nsess;
	group(key, n, nsess, order, start);
	for (uint32_t s = 0; s < nsess; s++) {
		uint32_t memberc = sv[s].memberc;
		for (uint32_t p = start[s]; p < start[s + 1]; p++) {
			const uint32_t i = order[p];
			const uint32_t o = lanes_member(sv[s].m, &memberc,
							ssrc[i]);
			if (o < 8)
				rrx_source_sr(&sv[s].m[o], recv, v[i][0],
					      v[i][1], v[i][2], v[i][3],
					      v[i][4]);
		}
		sv[s].memberc = memberc;
	}
	free(key);
	free(order);
	free(start);
}

/* eight lanes rank their keys, as k_rrx_report does */
static uint32_t d_report(struct rtp_rx_sess *ss, uint64_t now,
			 struct rtcp_enc_rb *rb)
{
	uint32_t key[8], cnt = 0;

	memset(rb, 0x5a, 8 * sizeof(*rb));
	for (uint32_t k = 0; k < 8; k++) {
		key[k] = rrx_report_key(&ss->m[k], k, ss->memberc);
		cnt += key[k] != RRX_NOKEY;
	}
	for (uint32_t slot = 0; slot < 8; slot++) {
		uint32_t before = 0, spare = 0;
		for (uint32_t k = 0; k < 8; k++) {
			before += key[k] < key[slot];
			spare += key[k] == RRX_NOKEY && k < slot;
		}
		if (key[slot] != RRX_NOKEY)
			rrx_report_block(&ss->m[slot], now, &rb[before]);
		else
			memset(&rb[cnt + spare], 0, sizeof(*rb));
	}
	return cnt;
}

/* ---- traffic ------------------------------------------------------------ */

enum { NSESS = 24, NPKT = 1500, NSR = 40, ROUNDS = 120 };

static uint32_t seqv[NSESS][10], tsv[NSESS][10];

static uint32_t rnd32(void)
{
	/* small, full-range and boundary values alike */
	switch (rndn(6)) {
	case 0: return rndn(4000);
	case 1: return 0x80000000u + rndn(3) - 1;
	case 2: return 0xffffffffu - rndn(3);
	default: return (uint32_t)rnd();
	}
}

int main(void)
{
	static uint8_t arena[NPKT * 96 + 64];
	static uint32_t pos[NPKT], end[NPKT], sess[NPKT], arrival[NPKT];
	static int32_t res[NPKT], st_p[NPKT], st_d[NPKT];
	static struct psess pv[NSESS];
	static struct rtp_rx_sess dv[NSESS];
	unsigned cnt[7] = {0}, resync = 0, cyc = 0, reports = 0;
	uint64_t now = 5000, npk = 0;

	for (uint32_t round = 0; round < ROUNDS; round++) {
		uint32_t at = 8;
		const int has_arr = round % 5 != 4;
		const int has_sess = round % 7 != 6;
		const int has_res = round % 3 != 2;

		if (round % 6 == 0) {           /* fresh sessions */
			memset(pv, 0, sizeof(pv));
			memset(dv, 0, sizeof(dv));
			for (uint32_t s = 0; s < NSESS; s++)
				for (uint32_t k = 0; k < 10; k++) {
					seqv[s][k] = rndn(4) ? rndn(65536)
							     : 65530 + rndn(6);
					tsv[s][k] = rndn(4) ? rnd32() : 0;
				}
		}
		memset(arena, 0xee, sizeof(arena));
		for (uint32_t i = 0; i < NPKT; i++) {
			const uint32_t s = rndn(NSESS), k = rndn(1 + s % 10);
			const uint32_t w = rndn(100);
			uint32_t seq = seqv[s][k], len = 12 + rndn(30);
			uint8_t *p = arena + at;

			if (w < 5)
				seq = seqv[s][k] = (seq + 2995 + rndn(10)) & 65535;
			else if (w < 10)
				seq = (seq - rndn(104)) & 65535;
			else if (w < 16)
				seq = seqv[s][k] = (seq + 3000 + rndn(60000)) &
						   65535;
			else
				seqv[s][k] = (seq + 1) & 65535;
			if (w % 10 != 3)
				tsv[s][k] = w % 10 == 4 ? rnd32()
						: tsv[s][k] + rndn(4000);
			p[0] = 0x80;
			if (w >= 20 && w < 24)
				p[0] = (uint8_t)(rndn(4) << 6);
			if (w >= 24 && w < 32)
				p[0] |= (uint8_t)(rndn(32));    /* X, CC */
			p[1] = 96;
			p[2] = (uint8_t)(seq >> 8);
			p[3] = (uint8_t)seq;
			for (uint32_t b = 0; b < 4; b++) {
				p[4 + b] = (uint8_t)(tsv[s][k] >> (24 - 8 * b));
				p[8 + b] = (uint8_t)((0x100 * s + 9 * k) >>
						     (24 - 8 * b));
			}
			if (p[0] & 16) {                /* extension length */
				const uint32_t x = 12 + 4 * (p[0] & 15);
				p[x + 2] = 0;
				p[x + 3] = (uint8_t)rndn(4);
				len = rndn(3) ? x + 4 + 4 * p[x + 3] + rndn(3)
					      : x + 4 * p[x + 3] + rndn(8);
			}
			else if (p[0] & 15) {
				len = 12 + 4 * (p[0] & 15) - (rndn(4) ? 0 : 1);
			}
			if (w >= 32 && w < 35)
				len = rndn(12);
			pos[i] = at;
			end[i] = at + len;
			at += 96;
			sess[i] = s;
			arrival[i] = w % 7 == 5 ? tsv[s][k]
						: tsv[s][k] + rnd32();
			res[i] = (w >= 35 && w < 38) ? 74 : 0;
			if (w == 38)
				end[i] = pos[i] - 1 - rndn(3);
			if (w == 39)
				end[i] = sizeof(arena) + 1 + rndn(3);
			if (w == 40)
				sess[i] = NSESS + rndn(3);
		}
		for (uint32_t i = 0; i < NPKT; i++) {
			const uint32_t si = has_sess ? sess[i] : 0;
			const int had0 = si < NSESS && pv[si].m[0].s.has;
			const uint32_t base0 = had0 ? pv[si].m[0].s.base_seq : 0;
			st_p[i] = p_packet(pv, NSESS, arena, sizeof(arena),
					   pos[i], end[i], has_res && res[i],
					   si, has_arr, arrival[i]);
			if (had0 && pv[si].m[0].s.base_seq != base0)
				resync++;       /* only init_seq moves it */
			cnt[st_p[i] == 0 ? 0 : st_p[i] == RTP_RX_BADSEQ ? 1 :
			    st_p[i] == RTP_RX_NOMEMBER ? 2 :
			    st_p[i] == RTP_RX_SKIPPED ? 3 :
			    st_p[i] == EBADMSG ? 4 : st_p[i] == EINVAL ? 5 : 6]++;
			st_d[i] = 0x5a5a5a5a;
		}
		npk += NPKT;
		d_stats(arena, sizeof(arena), pos, end, has_res ? res : NULL,
			has_sess ? sess : NULL, has_arr ? arrival : NULL, NPKT,
			dv, NSESS, st_d);
		for (uint32_t i = 0; i < NPKT; i++)
			CHECK(st_p[i] == st_d[i], "round %u packet %u stat %d %d",
			      round, i, st_p[i], st_d[i]);
		compare(pv, dv, NSESS, "stats");

		if (round % 2) {                /* SR events */
			static uint32_t ss[NSR], sc[NSR], v[NSR][5];
			for (uint32_t i = 0; i < NSR; i++) {
				ss[i] = rndn(NSESS + 2);
				sc[i] = 0x100 * ss[i] + 9 * rndn(12);
				for (uint32_t k = 0; k < 5; k++)
					v[i][k] = rndn(3) ? rnd32() : 0;
				if (ss[i] < NSESS)
					p_sr(&pv[ss[i]], sc[i], now, v[i]);
			}
			d_sr(dv, NSESS, ss, sc, (const uint32_t (*)[5])v, now,
			     NSR);
			compare(pv, dv, NSESS, "sr");
			now += rndn(3000);
		}
		if (round % 3 == 1) {           /* a report */
			for (uint32_t s = 0; s < NSESS; s++) {
				struct rtcp_enc_rb ra[8], rb[8];
				const uint32_t ca = p_report(&pv[s], now, ra);
				const uint32_t cb = d_report(&dv[s], now, rb);
				CHECK(ca == cb, "report count %u %u", ca, cb);
				CHECK(!memcmp(ra, rb, ca * sizeof(ra[0])),
				      "round %u sess %u report blocks", round,
				      s);
				for (uint32_t k = cb; k < 8; k++)
					CHECK(!rb[k].ssrc && !rb[k].dlsr,
					      "spare block %u not zero", k);
				reports += ca;
			}
			compare(pv, dv, NSESS, "report");
			now += 5000;
		}
		for (uint32_t s = 0; s < NSESS; s++)
			for (uint32_t k = 0; k < pv[s].memberc; k++)
				cyc += pv[s].m[k].s.cycles != 0;
	}
	CHECK(!cnt[6], "unknown stat");
	printf("%u rounds, %llu packets: %u ok, %u badseq, %u nomember, "
	       "%u skipped, %u badmsg, %u einval; %u resyncs, %u cycled, "
	       "%u report blocks; %d wrong\n", ROUNDS,
	       (unsigned long long)npk, cnt[0], cnt[1], cnt[2], cnt[3], cnt[4],
	       cnt[5], resync, cyc, reports, wrong);
	return wrong ? 1 : 0;
}
