/*
 * gen_rtp_source_golden.c -- receiver-statistics goldens from the reference
 * itself (tests/golden/rtp_source_golden.json.gz).
 *
 * Built by scripts/make_rtp_source_golden.sh against the reference's
 * src/rtp/source.c, member.c, rtp.c, ntp.c and src/hash/hash.c (and the
 * mbuf / mem / list closure), into a temporary directory; nothing of the
 * reference is kept.  It calls the reference's own rtp_hdr_decode,
 * rtp_member_find / rtp_member_add, hash_apply, rtp_source_init_seq,
 * rtp_source_update_seq, rtp_source_calc_jitter, rtp_source_calc_lost,
 * rtp_source_calc_fraction_lost and ntp_compact.
 *
 * What joins them in the reference lives in src/rtp/sess.c and is static
 * or bound to a socket, a timer and the wall clock: get_member (:83-101),
 * handle_incoming_sr (:168-185), calc_lsr / calc_dlsr (:372-387),
 * sender_apply_handler (:390-410), rtcp_sess_rx_rtp (:614-666) and
 * rtp_decode's version check (rtp.c:518).  Those ~20 lines of glue are
 * restated below, with tmr_jiffies() replaced by a time the case gives.
 *
 * Every case runs the same stages, so that a test can run all cases as one
 * batch, one session per case:
 *   rtp A, sr A (received at 1000 ms), rtp B, check, report at 6000 ms,
 *   check, sr B (received at 7000 ms), rtp C, check, report at 11000 ms,
 *   check
 * Output (JSON): cases[] of {name, arrival (0: srate_rx == 0, no jitter),
 * stages[]}; a stage is
 *   {"op":"rtp","pk":[[hex, arrival, stat], ...]}   stat: ok | badseq (the
 *        sequence update returned 0) | nomember | badmsg
 *   {"op":"sr","recv_ms":T,"ev":[[ssrc, ntp_sec, ntp_frac, rtp_ts, psent,
 *        osent], ...]}
 *   {"op":"check","memberc":N,"m":[[ssrc, has_source, max_seq, cycles,
 *        base_seq, bad_seq, received, expected_prior, received_prior,
 *        transit, jitter, last_rtp_ts, rx_bytes, sr_recv, ntp_hi, ntp_lo,
 *        rtp_ts, psent, osent], ...]}   members in hash_apply order
 *   {"op":"report","now_ms":T,"rb":[[ssrc, fraction, lost, last_seq,
 *        jitter, lsr, dlsr], ...]}
 * Transit differences and loss counts stay below 2^30, where the
 * reference's int arithmetic is defined.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <re.h>
#include "rtcp.h"          /* struct rtp_member, ntp_compact (src/rtp) */

enum { MAX_MEMBERS = 8, MAXEV = 3072, MAXPKT = 96 };

/* ---- the case under construction --------------------------------------- */

struct pkt {
	uint8_t b[MAXPKT];
	size_t len;
	uint32_t arr;
};

struct srev {
	uint32_t ssrc, sec, frac, ts, ps, os;
};

static struct {
	const char *name;
	int arrival;
	struct pkt rtp[3][MAXEV];
	size_t nrtp[3];
	struct srev sr[2][MAXEV];
	size_t nsr[2];
} C;

static int stage;               /* rtp stage 0..2 / sr stage 0..1 to add to */

static void begin(const char *name, int arrival)
{
	memset(&C, 0, sizeof(C));
	C.name = name;
	C.arrival = arrival;
	stage = 0;
}

/* a raw packet: first byte, CSRC words and an extension of xlen words (-1:
 * none) as the header says, cut or padded with payload bytes to len */
static void raw(uint32_t b0, uint32_t seq, uint32_t ts, uint32_t ssrc,
		int xlen, size_t len, uint32_t arr)
{
	struct pkt *p;
	uint8_t b[MAXPKT];
	size_t n = 12, i;
	const uint32_t cc = b0 & 15;

	if (C.nrtp[stage] >= MAXEV || len > MAXPKT)
		abort();
	p = &C.rtp[stage][C.nrtp[stage]++];
	memset(b, 0xa5, sizeof(b));
	b[0] = (uint8_t)b0;
	b[1] = 96;
	b[2] = (uint8_t)(seq >> 8);
	b[3] = (uint8_t)seq;
	for (i = 0; i < 4; i++) {
		b[4 + i] = (uint8_t)(ts >> (24 - 8 * i));
		b[8 + i] = (uint8_t)(ssrc >> (24 - 8 * i));
	}
	n += 4 * cc;
	if (xlen >= 0 && n + 4 <= MAXPKT) {
		b[n] = 0xbe;
		b[n + 1] = 0xde;
		b[n + 2] = (uint8_t)(xlen >> 8);
		b[n + 3] = (uint8_t)xlen;
	}
	memcpy(p->b, b, len);
	p->len = len;
	p->arr = arr;
}

/* a plain packet with an 8-byte payload */
static void pk(uint32_t seq, uint32_t ts, uint32_t ssrc, uint32_t arr)
{
	raw(0x80, seq, ts, ssrc, -1, 20, arr);
}

static void sr(uint32_t ssrc, uint32_t sec, uint32_t frac, uint32_t ts,
	       uint32_t ps, uint32_t os)
{
	struct srev e = {ssrc, sec, frac, ts, ps, os};

	if (stage > 1 || C.nsr[stage] >= MAXEV)
		abort();
	C.sr[stage][C.nsr[stage]++] = e;
}

/* ---- the glue of sess.c, restated -------------------------------------- */

struct sess {
	struct hash *members;
	uint32_t memberc;
	int arrival;            /* srate_rx != 0 */
};

static struct rtp_member *get_member(struct sess *s, uint32_t src)
{
	struct rtp_member *mbr = rtp_member_find(s->members, src);

	if (mbr)
		return mbr;
	if (s->memberc >= MAX_MEMBERS)
		return NULL;
	mbr = rtp_member_add(s->members, src);
	if (!mbr)
		abort();
	++s->memberc;
	return mbr;
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
	if (p->len)
		(void)mbuf_write_mem(mb, p->b, p->len);
	mb->pos = 0;
	memset(&hdr, 0, sizeof(hdr));
	err = rtp_hdr_decode(&hdr, mb);
	payload = mbuf_get_left(mb);
	mem_deref(mb);
	if (err || hdr.ver != 2)
		return "badmsg";
	mbr = get_member(s, hdr.ssrc);
	if (!mbr)
		return "nomember";
	if (!mbr->s) {
		mbr->s = mem_zalloc(sizeof(*mbr->s), NULL);
		if (!mbr->s)
			abort();
		rtp_source_init_seq(mbr->s, hdr.seq);
	}
	ok = rtp_source_update_seq(mbr->s, hdr.seq);
	if (s->arrival && hdr.ts != mbr->s->last_rtp_ts)
		rtp_source_calc_jitter(mbr->s, hdr.ts, p->arr);
	mbr->s->last_rtp_ts = hdr.ts;
	mbr->s->rtp_rx_bytes += payload;
	return ok ? "ok" : "badseq";
}

static void rx_sr(struct sess *s, const struct srev *e, uint64_t recv_ms)
{
	struct rtp_member *mbr = get_member(s, e->ssrc);

	if (!mbr || !mbr->s)
		return;
	mbr->s->sr_recv = recv_ms;
	mbr->s->last_sr.hi = e->sec;
	mbr->s->last_sr.lo = e->frac;
	mbr->s->rtp_ts = e->ts;
	mbr->s->psent = e->ps;
	mbr->s->osent = e->os;
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
		printf(",%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%llu,%llu,%u,%u,%u,%u,%u]",
		       s->max_seq, s->cycles, s->base_seq, s->bad_seq,
		       s->received, s->expected_prior, s->received_prior,
		       (uint32_t)s->transit, s->jitter, s->last_rtp_ts,
		       (unsigned long long)s->rtp_rx_bytes,
		       (unsigned long long)s->sr_recv, s->last_sr.hi,
		       s->last_sr.lo, s->rtp_ts, s->psent, s->osent);
	else
		printf(",0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0]");
	return false;
}

static bool report_h(struct le *le, void *arg)
{
	struct rtp_member *mbr = le->data;
	struct rtp_source *s = mbr->s;
	uint32_t lsr, dlsr = 0;
	unsigned fraction;
	int lost;
	(void)arg;

	if (!s)
		return false;
	fraction = rtp_source_calc_fraction_lost(s);
	lost = rtp_source_calc_lost(s);
	lsr = s->last_sr.hi ? ntp_compact(&s->last_sr) : 0;
	if (s->sr_recv)
		dlsr = (uint32_t)((65536 * (now_ms - s->sr_recv)) / 1000);
	printf("%s[%u,%u,%d,%u,%u,%u,%u]", sep++ ? "," : "", mbr->src,
	       fraction, lost, s->cycles | s->max_seq, s->jitter >> 4, lsr,
	       dlsr);
	return false;
}

/* ---- run the case's stages --------------------------------------------- */

static int stsep;

static void st_rtp(struct sess *s, int k)
{
	size_t i, j;

	printf("%s{\"op\":\"rtp\",\"pk\":[", stsep++ ? "," : "");
	for (i = 0; i < C.nrtp[k]; i++) {
		const struct pkt *p = &C.rtp[k][i];
		printf("%s[\"", i ? "," : "");
		for (j = 0; j < p->len; j++)
			printf("%02x", p->b[j]);
		printf("\",%u,\"%s\"]", p->arr, rx_rtp(s, p));
	}
	printf("]}");
}

static void st_sr(struct sess *s, int k, uint64_t recv_ms)
{
	size_t i;

	printf(",{\"op\":\"sr\",\"recv_ms\":%llu,\"ev\":[",
	       (unsigned long long)recv_ms);
	for (i = 0; i < C.nsr[k]; i++) {
		const struct srev *e = &C.sr[k][i];
		printf("%s[%u,%u,%u,%u,%u,%u]", i ? "," : "", e->ssrc, e->sec,
		       e->frac, e->ts, e->ps, e->os);
		rx_sr(s, e, recv_ms);
	}
	printf("]}");
}

static void st_check(struct sess *s)
{
	printf(",{\"op\":\"check\",\"memberc\":%u,\"m\":[", s->memberc);
	sep = 0;
	(void)hash_apply(s->members, check_h, NULL);
	printf("]}");
}

static void st_report(struct sess *s, uint64_t t)
{
	printf(",{\"op\":\"report\",\"now_ms\":%llu,\"rb\":[",
	       (unsigned long long)t);
	sep = 0;
	now_ms = t;
	(void)hash_apply(s->members, report_h, NULL);
	printf("]}");
}

static int casesep;

static void end(void)
{
	struct sess s = {NULL, 0, C.arrival};

	if (hash_alloc(&s.members, MAX_MEMBERS))
		abort();
	printf("%s\n{\"name\":\"%s\",\"arrival\":%d,\"stages\":[",
	       casesep++ ? "," : "", C.name, C.arrival);
	stsep = 0;
	st_rtp(&s, 0);
	st_sr(&s, 0, 1000);
	st_rtp(&s, 1);
	st_check(&s);
	st_report(&s, 6000);
	st_check(&s);
	st_sr(&s, 1, 7000);
	st_rtp(&s, 2);
	st_check(&s);
	st_report(&s, 11000);
	st_check(&s);
	printf("]}");
	hash_flush(s.members);
	mem_deref(s.members);
}

/* ---- the cases ---------------------------------------------------------- */

/* a run of count packets from seq on, 160 timestamp units and 163 arrival
 * units apart */
static void run(uint32_t seq, uint32_t count, uint32_t ts, uint32_t ssrc,
		uint32_t arr)
{
	uint32_t i;

	for (i = 0; i < count; i++)
		pk((seq + i) & 0xffff, ts + 160 * i, ssrc, arr + 163 * i);
}

/* a backward step of `back` after a short run, then on */
static void backward(const char *name, uint32_t back)
{
	begin(name, 1);
	run(500, 3, 1000, 0x11, 5000);
	pk(502 - back, 90000, 0x11, 95000);
	stage = 1;
	pk(503, 1480, 0x11, 5499);
	stage = 2;
	pk(502 - back + 1, 90160, 0x11, 95170);
	pk(504, 1640, 0x11, 5660);
	end();
}

static void gap(const char *name, uint32_t g)
{
	begin(name, 1);
	run(100, 2, 3000, 0x22, 7000);
	pk(101 + g, 3000 + 160 * g, 0x22, 7000 + 161 * g);
	stage = 1;
	pk(102 + g, 3000 + 160 * (g + 1), 0x22, 7000 + 161 * (g + 1) + 40);
	stage = 2;
	pk(103 + g, 3000 + 160 * (g + 2), 0x22, 7000 + 161 * (g + 2));
	end();
}

int main(void)
{
	uint32_t i;

	printf("{\"source\":\"reference src/rtp/source.c, member.c, rtp.c "
	       "(rtp_hdr_decode), ntp.c, src/hash/hash.c driven as "
	       "src/rtp/sess.c drives them\",\"cases\":[");

	begin("first_packet_only", 1);
	pk(4711, 123456, 0xcafe0001, 999999);
	end();

	begin("first_ts_zero", 1);
	pk(10, 0, 0x31, 5000);           /* ts == last_rtp_ts (0): no jitter */
	pk(11, 160, 0x31, 5170);
	stage = 1;
	pk(12, 320, 0x31, 5300);
	stage = 2;
	pk(13, 480, 0x31, 5555);
	end();

	begin("arrival_equals_ts", 1);
	pk(20, 8000, 0x32, 8000);        /* transit 0: "none yet" again */
	pk(21, 8160, 0x32, 8200);
	pk(22, 8320, 0x32, 8320);        /* transit 0 stored */
	stage = 1;
	pk(23, 8480, 0x32, 8600);        /* taken as the first transit */
	pk(24, 8640, 0x32, 8700);
	stage = 2;
	pk(25, 8800, 0x32, 8950);
	end();

	begin("equal_ts", 1);
	pk(30, 4000, 0x33, 9000);
	pk(31, 4000, 0x33, 9100);        /* same frame: no jitter */
	pk(32, 4160, 0x33, 9300);
	stage = 1;
	pk(33, 4160, 0x33, 9400);
	pk(34, 4320, 0x33, 9420);
	stage = 2;
	pk(35, 4320, 0x33, 9500);
	pk(36, 1000, 0x33, 9600);        /* timestamp goes back */
	end();

	begin("wrap_65535_to_0", 1);
	run(65533, 3, 100000, 0x41, 200000);
	stage = 1;
	run(0, 3, 100480, 0x41, 200500);
	stage = 2;
	run(3, 2, 100960, 0x41, 201100);
	end();

	gap("gap_2999", 2999);
	gap("gap_3000", 3000);
	backward("backward_99", 99);
	backward("backward_100", 100);
	backward("backward_101", 101);

	begin("jump_then_next_resync", 1);
	run(1000, 4, 5000, 0x51, 6000);
	pk(30000, 700000, 0x51, 800000);         /* bad_seq = 30001 */
	pk(30001, 700160, 0x51, 800170);         /* resync */
	stage = 1;
	run(30002, 3, 700320, 0x51, 800333);
	stage = 2;
	pk(30006, 700960, 0x51, 801000);
	end();

	begin("jump_then_other", 1);
	run(1000, 4, 5000, 0x52, 6000);
	pk(30000, 700000, 0x52, 800000);         /* bad_seq = 30001 */
	pk(30002, 700160, 0x52, 800170);         /* not it: bad_seq = 30003 */
	pk(1004, 5640, 0x52, 6700);
	stage = 1;
	pk(30003, 700320, 0x52, 800400);         /* now it is */
	stage = 2;
	pk(30004, 700480, 0x52, 800500);
	end();

	begin("bad_seq_at_65535", 1);
	run(10000, 2, 5000, 0x53, 6000);
	pk(65535, 900000, 0x53, 950000);         /* bad_seq = 0 */
	pk(0, 900160, 0x53, 950200);             /* resync at 0 */
	stage = 1;
	pk(65534, 900320, 0x53, 950300);         /* bad_seq = 65535 */
	pk(65535, 900480, 0x53, 950500);         /* resync at 65535 */
	stage = 2;
	pk(0, 900640, 0x53, 950600);             /* and a wrap */
	end();

	begin("duplicates_negative_lost", 1);
	run(200, 3, 1000, 0x61, 2000);
	for (i = 0; i < 5; i++)
		pk(201, 1160, 0x61, 2500 + 7 * i);
	stage = 1;
	pk(203, 1480, 0x61, 2700);
	for (i = 0; i < 3; i++)
		pk(203, 1480, 0x61, 2800 + i);
	stage = 2;
	pk(207, 2120, 0x61, 3400);               /* a real loss afterwards */
	end();

	/* the only way to a large loss count is the wrap count: 128 wraps in
	 * steps of 2999, the largest step that is not a jump.  The first
	 * report comes just under the 24-bit clamp, the second over it. */
	begin("loss_clamp_by_wraps", 1);
	pk(0, 1000, 0x62, 2000);
	for (i = 1; i <= 2790; i++)
		pk((2999 * i) & 0xffff, 1000 + 160 * i, 0x62, 2000 + 161 * i);
	stage = 2;
	for (i = 2791; i <= 2810; i++)
		pk((2999 * i) & 0xffff, 1000 + 160 * i, 0x62, 2000 + 161 * i);
	end();

	begin("eight_ssrcs_shared_buckets", 1);
	for (i = 0; i < 8; i++)                  /* buckets 3,3,3,0,0,5,7,3 */
		pk(100 + i, 1000 * i + 7,
		   (uint32_t[]){0x103, 0x20b, 0x3, 0x8, 0x10, 0x5, 0xf, 0x1b}[i],
		   2000 * i + 9);
	stage = 1;
	for (i = 0; i < 8; i++)
		pk(101 + i + (i & 1), 1000 * i + 167,
		   (uint32_t[]){0x103, 0x20b, 0x3, 0x8, 0x10, 0x5, 0xf, 0x1b}[i],
		   2000 * i + 200);
	stage = 2;
	pk(104, 2333, 0x3, 4500);
	end();

	begin("nine_ssrcs", 1);
	for (i = 0; i < 9; i++)
		pk(100 + i, 1000 * i + 7, 0x100 * i + (i % 3), 2000 * i + 9);
	stage = 1;
	pk(109, 9999, 0x100 * 8 + 2, 10000);     /* the 9th again */
	pk(101, 167, 0, 300);
	stage = 2;
	pk(55, 5, 0xdead, 6);                    /* a 10th */
	pk(109, 8167, 0x100 * 7 + 1, 14300);
	end();

	begin("sr_unknown_as_8th_then_9th", 1);
	for (i = 0; i < 7; i++)
		pk(10 * i, 50 * i + 1, 0x40 + i, 60 * i + 3);
	stage = 0;
	sr(0x47, 0x83aa7e80, 0x40000000, 777, 5, 800);   /* takes slot 8 */
	stage = 1;
	pk(1, 2, 0x99, 3);                       /* the 9th: no member */
	pk(70, 351, 0x47, 500);                  /* the SR's member: source */
	stage = 1;
	sr(0x47, 0x83aa7e85, 0x80000000, 40777, 255, 40800);
	sr(0x99, 1, 2, 3, 4, 5);                 /* still no room */
	stage = 2;
	pk(71, 511, 0x47, 700);
	end();

	begin("sr_before_and_after_source", 1);
	sr(0x71, 0x83aa7e80, 0x12345678, 1111, 10, 1600);    /* no source yet */
	stage = 1;
	run(300, 3, 2000, 0x71, 3000);
	sr(0x71, 0xe3aa7e86, 0x9abcdef0, 49111, 260, 41600);
	sr(0x72, 0xe3aa7e86, 0x9abcdef0, 1, 2, 3);           /* member only */
	stage = 2;
	run(303, 2, 2480, 0x71, 3490);
	pk(9, 9, 0x72, 9);
	end();

	begin("sr_ntp_hi_zero", 1);
	run(300, 2, 2000, 0x73, 3000);
	stage = 0;
	sr(0x73, 0, 0xffff0000, 1111, 10, 1600);  /* lsr 0, dlsr counted */
	stage = 1;
	pk(302, 2320, 0x73, 3400);
	sr(0x73, 0x10000, 0xffff0000, 2222, 20, 3200);   /* hi & 0xffff == 0 */
	stage = 2;
	pk(303, 2480, 0x73, 3500);
	end();

	/* every header error at its boundary length; the good neighbours
	 * count, the bad ones change nothing */
	begin("header_errors", 1);
	raw(0x80, 1, 100, 0x81, -1, 0, 50);      /* empty */
	raw(0x80, 1, 100, 0x81, -1, 11, 50);     /* one short of a header */
	raw(0x80, 1, 100, 0x81, -1, 12, 50);     /* header only: payload 0 */
	raw(0x83, 2, 260, 0x81, -1, 23, 220);    /* 3 CSRCs, one byte short */
	raw(0x83, 2, 260, 0x81, -1, 24, 220);    /* exactly */
	raw(0x8f, 3, 420, 0x81, -1, 71, 390);    /* 15 CSRCs short */
	raw(0x8f, 3, 420, 0x81, -1, 72, 390);
	stage = 1;
	raw(0x90, 4, 580, 0x81, 0, 15, 560);     /* extension header short */
	raw(0x90, 4, 580, 0x81, 0, 16, 560);     /* empty extension */
	raw(0x90, 5, 740, 0x81, 2, 23, 730);     /* body one byte short */
	raw(0x90, 5, 740, 0x81, 2, 24, 730);
	raw(0x92, 6, 900, 0x81, 3, 35, 900);     /* CSRCs and extension */
	raw(0x92, 6, 900, 0x81, 3, 36, 900);
	raw(0x90, 7, 1060, 0x81, 0xffff, 96, 1070);      /* huge extension */
	stage = 2;
	raw(0x00, 7, 1060, 0x81, -1, 20, 1070);  /* version 0 */
	raw(0x40, 7, 1060, 0x81, -1, 20, 1070);  /* version 1 */
	raw(0xc0, 7, 1060, 0x81, -1, 20, 1070);  /* version 3 */
	raw(0xa0, 7, 1060, 0x81, -1, 20, 1070);  /* padding bit: not stripped */
	raw(0x50, 8, 1220, 0x81, 0, 15, 1230);   /* version 1 and short */
	end();

	begin("no_arrival_times", 0);            /* srate_rx == 0 */
	run(65534, 4, 1000, 0x91, 0);
	stage = 1;
	pk(9000, 5000, 0x91, 0);
	pk(9001, 5160, 0x91, 0);
	pk(9001, 5160, 0x92, 0);
	sr(0x91, 0x83aa7e80, 0x40000000, 777, 5, 800);
	stage = 2;
	run(9002, 2, 5320, 0x91, 0);
	end();

	printf("\n]}\n");
	return 0;
}
