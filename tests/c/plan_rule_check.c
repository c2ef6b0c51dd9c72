/*
 * plan_rule_check.c -- the planners' shared rules (re_amd/csrc/hip/
 * plan_rule.h, compiled as C) against a sequential receiver written after
 * the host engine's own (re_amd/csrc/host/srtp.c: plan_rtp_dec, get_index,
 * replay_check).  One stream's batch runs through the rules the way
 * k_plan_count + k_plan_desc compose them (a serial prefix stands for the
 * rollover scan); whenever the rules accept a batch, every index and the
 * stream's state after it must be the receiver's.
 *
 *   gcc -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -o plan_rule_check tests/c/plan_rule_check.c && ./plan_rule_check
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../re_amd/csrc/hip/plan_rule.h"

#define NMAX 256

static int g_bad;

#define CHECK(c, ...)                                                        \
	do {                                                                 \
		if (!(c)) {                                                  \
			if (g_bad++ < 20) {                                  \
				printf("FAIL %s:%d: ", __FILE__, __LINE__);  \
				printf(__VA_ARGS__);                         \
				printf("\n");                                \
			}                                                    \
		}                                                            \
	} while (0)

static uint32_t g_rng = 0x12345678u;

static uint32_t rnd(void)
{
	g_rng = g_rng * 1664525u + 1013904223u;
	return g_rng >> 8;
}

/* ---- the sequential receiver ---------------------------------------- */

struct rx {
	uint32_t roc;
	uint16_t s_l;
	uint64_t lix, bitmap;
};

enum { RX_OK = 0, RX_TIMEDOUT, RX_ALREADY };

/* replay.c:32-62 */
static int ref_replay_check(struct rx *r, uint64_t ix)
{
	uint64_t diff;
	if (ix > r->lix) {
		diff = ix - r->lix;
		r->bitmap = diff < 64 ? (r->bitmap << diff) | 1 : 1;
		r->lix = ix;
		return 1;
	}
	diff = r->lix - ix;
	if (diff >= 64 || (r->bitmap & (1ULL << diff)))
		return 0;
	r->bitmap |= 1ULL << diff;
	return 1;
}

/* misc.c:22-41, including the `int v` sign extension of roc +- 1 */
static uint64_t ref_get_index(uint32_t roc, uint16_t s_l, uint16_t seq)
{
	int32_t v;
	if (s_l < 32768)
		v = ((int)seq - (int)s_l > 32768) ? (int32_t)(roc - 1)
						  : (int32_t)roc;
	else
		v = ((int)s_l - 32768 > seq) ? (int32_t)(roc + 1) : (int32_t)roc;
	return seq + (uint64_t)(int64_t)v * 65536ull;
}

/* srtp_decrypt (srtp.c:310-321, 367, 426-427) for an authentic packet */
static int ref_packet(struct rx *r, uint16_t seq, uint64_t *ix)
{
	const int diff = (int)seq - (int)r->s_l;
	if (diff > 32768)
		return RX_TIMEDOUT;
	if (diff <= -32768) {
		r->roc++;
		r->s_l = 0;
	}
	*ix = ref_get_index(r->roc, r->s_l, seq);
	if (!ref_replay_check(r, *ix))
		return RX_ALREADY;
	if (seq > r->s_l)
		r->s_l = seq;
	return RX_OK;
}

/* ---- the batch through the shared rules ----------------------------- */

struct planned {
	uint32_t count_fail;    /* k_plan_count's bits */
	uint32_t desc_fail;     /* k_plan_desc's (SPF_REPLAY) */
	uint64_t ix[NMAX];
	struct rx after;
};

/* fresh: the stream has no s_l yet (stream.c:87-109: the first seq) */
static void plan_batch(const struct rx *st, int fresh, const uint16_t *seq,
		       uint32_t n, struct planned *p)
{
	uint32_t roc = st->roc, sb = 0, wrap = 0, i;
	memset(p, 0, sizeof(*p));
	for (i = 0; i < n; i++) {
		const uint32_t psb = sb;        /* what packet i-1 saw */
		sb = i == 0 ? (fresh ? seq[0] : st->s_l) : seq[i - 1];
		const struct plan_ord o = plan_order(seq[i], sb, i + 1 == n, 0);
		p->count_fail |= o.flags;
		wrap = o.wrap;
		roc += wrap;            /* the scan: ROC after its own rollover */
		const struct plan_idx x = plan_index(roc, (int)wrap, sb, seq[i],
						     0);
		const int ok = i == 0 ?
			plan_new_first(x.ix, st->lix, st->bitmap) :
			plan_new_later(x.ix, plan_prev_index(roc, (int)wrap, psb,
							     seq[i - 1]),
				       st->lix);
		if (!ok)
			p->desc_fail |= SPF_REPLAY;
		p->ix[i] = x.ix;
		/* the desc word round-trips, and its flags give the trailer ROC */
		CHECK(d_desc_ix(d_desc(x.ix, x.fl)) == (x.ix & 0xffffffffffffull),
		      "d_desc");
		CHECK((uint32_t)(x.ix >> 16) + ((x.fl & SD_ROC_P1) ? 1u : 0u) -
		      ((x.fl & SD_ROC_M1) ? 1u : 0u) == roc, "SD_ROC flags");
	}
	if (p->count_fail | p->desc_fail)
		return;         /* no plan: no state after it */
	p->after.roc = roc;
	p->after.s_l = (uint16_t)plan_s_l_after(seq[n - 1], sb, (int)wrap);
	/* the window: the stored one folded over the last <= 65 indices
	 * (k_mp_final; older bits have shifted out) */
	struct plan_win w = {st->lix, st->bitmap};
	i = 0;
	if (n > 65) {
		i = n - 65;
		w.lix = p->ix[i - 1];
		w.bitmap = 1;
	}
	for (; i < n; i++)
		w = plan_win_step(w, p->ix[i]);
	p->after.lix = w.lix;
	p->after.bitmap = w.bitmap;
}

/* an accepted plan is the receiver's run; returns whether it was accepted */
static int check_batch(const struct rx *st, int fresh, const uint16_t *seq,
		       uint32_t n, int must_accept, const char *what)
{
	static struct planned p;
	struct rx r = *st;
	uint32_t i;
	plan_batch(st, fresh, seq, n, &p);
	if (p.count_fail | p.desc_fail) {
		CHECK(!must_accept, "%s: n %u rejected %x %x", what, n,
		      p.count_fail, p.desc_fail);
		return 0;
	}
	if (fresh)
		r.s_l = seq[0];
	for (i = 0; i < n; i++) {
		uint64_t ix = 0;
		const int e = ref_packet(&r, seq[i], &ix);
		CHECK(e == RX_OK, "%s: n %u packet %u: receiver says %d", what, n,
		      i, e);
		CHECK(ix == p.ix[i], "%s: n %u packet %u: index %llx, not %llx",
		      what, n, i, (unsigned long long)p.ix[i],
		      (unsigned long long)ix);
		if (e != RX_OK || ix != p.ix[i])
			return 1;
	}
	CHECK(r.roc == p.after.roc && r.s_l == p.after.s_l,
	      "%s: n %u: state (%u, %u), not (%u, %u)", what, n, p.after.roc,
	      p.after.s_l, r.roc, r.s_l);
	CHECK(r.lix == p.after.lix && r.bitmap == p.after.bitmap,
	      "%s: n %u: window (%llx, %llx), not (%llx, %llx)", what, n,
	      (unsigned long long)p.after.lix,
	      (unsigned long long)p.after.bitmap, (unsigned long long)r.lix,
	      (unsigned long long)r.bitmap);
	return 1;
}

static uint32_t fails_of(const struct rx *st, int fresh, const uint16_t *seq,
			 uint32_t n, uint32_t *countp)
{
	static struct planned p;
	plan_batch(st, fresh, seq, n, &p);
	if (countp)
		*countp = p.count_fail;
	return p.count_fail | p.desc_fail;
}

/* ---- the checks ----------------------------------------------------- */

static void check_index(void)
{
	static const uint32_t rocs[] = {0, 1, 0xffffu, 0x10000u, 0x7ffffffeu,
					0x7fffffffu, 0x80000000u, 0xfffffffeu,
					0xffffffffu};
	static const uint16_t edge[] = {0, 1, 32767, 32768, 32769, 65535};
	uint32_t r, k;
	for (r = 0; r < sizeof(rocs) / sizeof(rocs[0]); r++) {
		for (k = 0; k < 36 + 4096; k++) {
			const uint16_t s_l = k < 36 ? edge[k / 6] : (uint16_t)rnd();
			const uint16_t seq = k < 36 ? edge[k % 6] : (uint16_t)rnd();
			const uint32_t roc = rocs[r];
			CHECK(plan_index(roc, 0, s_l, seq, 0).ix ==
			      ref_get_index(roc, s_l, seq),
			      "index roc %x s_l %u seq %u", roc, s_l, seq);
			/* after a rollover the receiver's s_l is 0 */
			CHECK(plan_index(roc, 1, s_l, seq, 0).ix ==
			      ref_get_index(roc, 0, seq),
			      "index after a rollover roc %x seq %u", roc, seq);
			CHECK(plan_index(roc, 0, s_l, seq, 1).ix ==
			      65536ull * roc + seq, "sender index");
		}
	}
}

/* a continuing stream: the window full of odd history, its top at s_l */
static struct rx continuing(uint32_t roc, uint16_t s_l)
{
	struct rx st;
	st.roc = roc;
	st.s_l = s_l;
	st.lix = 65536ull * roc + s_l;
	st.bitmap = 0xf0f0a5a5c3c30f01ull;
	return st;
}

static const uint32_t g_len[] = {1, 2, 64, 65, 66, 200};

/* strictly increasing, gaps below 32768, across `rolls` rollovers where
 * the length allows it */
static void increasing(uint16_t *seq, uint32_t n, uint16_t first,
		       uint32_t rolls)
{
	uint32_t gap = (rolls * 65536u + 1200u) / n + 1u, i;
	if (gap > 32767u)
		gap = 32767u;
	seq[0] = first;
	for (i = 1; i < n; i++)
		seq[i] = (uint16_t)(seq[i - 1] + (i % 3 ? gap : 1u));
}

static void check_accept(void)
{
	uint16_t seq[NMAX];
	uint32_t a, rolls, k;
	for (a = 0; a < 6; a++) {
		const uint32_t n = g_len[a];
		for (rolls = 0; rolls <= 2; rolls++) {
			/* (no rollover: from the low half of the seq space) */
			const uint16_t base = rolls ? 64990 : 2990;
			const struct rx fr = {0, 0, 0, 0};
			const struct rx co = continuing(5, base);
			uint32_t down = 0;
			increasing(seq, n, base + 10, rolls);
			for (k = 1; k < n; k++)
				down += seq[k] < seq[k - 1];
			CHECK(n < 64 || down == rolls, "n %u: %u rollovers, not %u",
			      n, down, rolls);
			(void)check_batch(&fr, 1, seq, n, 1, "fresh");
			(void)check_batch(&co, 0, seq, n, 1, "continuing");
			/* (a ROC of 2^31 or more makes the reference's index
			 * negative, misc.c:22-41: nothing must be accepted there,
			 * but what is must still be the receiver's) */
			const struct rx top = continuing(0xfffffffeu, base);
			(void)check_batch(&top, 0, seq, n, 0, "roc near 2^32");
			/* its siblings: nothing in the reference is special at
			 * 2^16; the batches of two rollovers cross 2^31 */
			const struct rx p16 = continuing(0xfffeu, base);
			(void)check_batch(&p16, 0, seq, n, 1, "roc near 2^16");
			const struct rx p31 = continuing(0x7ffffffeu, base);
			(void)check_batch(&p31, 0, seq, n, 0, "roc near 2^31");
			/* ... and with the window the reference itself leaves
			 * at such a ROC: its top sign-extended (misc.c:40) */
			struct rx sx = continuing(0x80000000u, base);
			sx.lix = ref_get_index(sx.roc, base, base);
			(void)check_batch(&sx, 0, seq, n, 0, "roc 2^31, its window");
			sx = continuing(0xfffffffeu, base);
			sx.lix = ref_get_index(sx.roc, base, base);
			(void)check_batch(&sx, 0, seq, n, 0, "roc near 2^32, its "
					  "window");
			/* packet 0 inside the stored window, on a clear bit: at or
			 * above s_l (a step back is SPF_ORDER unless it is the
			 * batch's last packet), the window's top 20 above it;
			 * every later packet above that top */
			struct rx in = continuing(5, base);
			in.lix += 20;
			increasing(seq, n, base + 10, rolls);
			seq[0] = base + 15;             /* bit 5: clear */
			for (k = 1; k < n && seq[k] <= base + 20 + k &&
				    seq[k] > base; k++)
				seq[k] = (uint16_t)(base + 20 + k);
			(void)check_batch(&in, 0, seq, n, 1, "first in window");
		}
	}
	/* the batch's only packet below s_l, in the window on a clear bit */
	const struct rx co = continuing(5, 64990);
	seq[0] = 64990 - 5;
	(void)check_batch(&co, 0, seq, 1, 1, "one packet below s_l");
}

static void check_reject(void)
{
	uint16_t seq[NMAX];
	uint32_t cf = 0;
	const struct rx fr = {0, 0, 0, 0};
	const struct rx co = continuing(5, 1000);

	/* a duplicate of an earlier packet of the batch */
	increasing(seq, 66, 2000, 0);
	seq[40] = seq[39];
	CHECK(fails_of(&co, 0, seq, 66, NULL) == SPF_REPLAY, "duplicate");
	CHECK(fails_of(&fr, 1, seq, 66, NULL) == SPF_REPLAY, "duplicate, fresh");

	/* packet 0 on a set bit of the window (its top: bit 0) */
	increasing(seq, 66, 1000, 0);
	CHECK(fails_of(&co, 0, seq, 66, NULL) == SPF_REPLAY, "first on a set bit");
	CHECK(fails_of(&co, 0, seq, 1, NULL) == SPF_REPLAY, "only one on a set bit");

	/* a packet i > 0 at or below the pre-batch lix: packet 0 in the window
	 * on a clear bit, packet 1 above it and still not above the window */
	struct rx in = continuing(5, 1000);
	in.lix += 20;
	increasing(seq, 66, 1100, 0);
	seq[0] = 1015;                  /* bit 5: clear */
	seq[1] = 1017;                  /* its bit (3) is clear too */
	CHECK(fails_of(&in, 0, seq, 66, NULL) == SPF_REPLAY, "second below lix");
	seq[1] = 1020;                  /* at lix */
	CHECK(fails_of(&in, 0, seq, 66, NULL) == SPF_REPLAY, "second at lix");

	/* a forward jump above 32768.  Its index is the ROC-1 estimate
	 * (misc.c:22-41), which at ROC 0 wraps above every index, so in the
	 * last position SPF_TIMEOUT stands alone; in the middle the packet
	 * behind it is then below it, and SPF_REPLAY joins */
	increasing(seq, 66, 100, 0);
	seq[65] = (uint16_t)(seq[64] + 32769u);
	CHECK(fails_of(&fr, 1, seq, 66, &cf) == SPF_TIMEOUT, "jump, last");
	increasing(seq, 66, 100, 0);
	seq[30] = (uint16_t)(seq[29] + 32769u);
	seq[31] = (uint16_t)(seq[30] + 1u);
	CHECK((fails_of(&fr, 1, seq, 32, &cf) & ~(uint32_t)SPF_REPLAY) ==
	      SPF_TIMEOUT && cf == SPF_TIMEOUT, "jump, middle");
	/* (32768 itself is no ETIMEDOUT: srtp.c:313) */
	increasing(seq, 3, 100, 0);
	seq[2] = (uint16_t)(seq[1] + 32768u);
	CHECK(!(fails_of(&fr, 1, seq, 3, NULL) & SPF_TIMEOUT), "jump of 32768");

	/* a backward step in the middle: the next packet's s_l speculation
	 * breaks (SPF_ORDER from the order rule alone; the packet is also
	 * below its predecessor's index, so k_plan_desc's SPF_REPLAY joins) */
	increasing(seq, 66, 2000, 0);
	seq[30] = (uint16_t)(seq[29] - 2u);
	CHECK((fails_of(&co, 0, seq, 66, &cf) & ~(uint32_t)SPF_REPLAY) ==
	      SPF_ORDER && cf == SPF_ORDER, "step back, middle");
	/* ... and against the stored s_l, by packet 0 on a clear bit of the
	 * window: SPF_ORDER alone while more packets follow, accepted as the
	 * batch's last (and only) packet */
	increasing(seq, 66, 2000, 0);
	seq[0] = 1000 - 5;
	CHECK(fails_of(&co, 0, seq, 66, NULL) == SPF_ORDER, "step back, first");
	(void)check_batch(&co, 0, seq, 1, 1, "step back, last");
	/* the order rule itself lets the last packet step back; behind
	 * another packet of the batch the replay speculation (every index
	 * above its predecessor's) still refuses it */
	CHECK(plan_order(1998, 2000, 0, 0).flags == SPF_ORDER &&
	      plan_order(1998, 2000, 1, 0).flags == 0, "plan_order last");
	increasing(seq, 66, 2000, 0);
	seq[65] = (uint16_t)(seq[64] - 2u);
	CHECK(fails_of(&co, 0, seq, 66, NULL) == SPF_REPLAY,
	      "step back behind a packet, last");
}

static void check_random(void)
{
	uint16_t seq[NMAX];
	uint32_t b, i, accepted = 0;
	for (b = 0; b < 2000; b++) {
		const uint32_t n = 1 + rnd() % 200;
		const int fresh = !(rnd() & 3);
		struct rx st = continuing(rnd() & 1 ? rnd() : 0xfffffff0u + rnd() % 32,
					  (uint16_t)rnd());
		const uint32_t big = rnd() % 4 == 0;
		st.bitmap = ((uint64_t)rnd() << 40 ^ (uint64_t)rnd() << 20 ^ rnd()) | 1;
		if (fresh)
			memset(&st, 0, sizeof(st));
		seq[0] = (uint16_t)(st.s_l + (fresh ? rnd() : rnd() % 40));
		for (i = 1; i < n; i++)
			seq[i] = (uint16_t)(seq[i - 1] + 1 +
					    (big ? rnd() % 3000 : rnd() % 3));
		/* every second batch: swaps and duplicates */
		if (b & 1) {
			for (i = rnd() % 3; i > 0 && n > 1; i--) {
				const uint32_t k = rnd() % (n - 1);
				const uint16_t t = seq[k];
				if (rnd() & 1) {
					seq[k] = seq[k + 1];
					seq[k + 1] = t;
				}
				else {
					seq[k + 1] = t;
				}
			}
		}
		accepted += (uint32_t)check_batch(&st, fresh, seq, n, 0, "random");
	}
	printf("random: %u of 2000 batches accepted\n", accepted);
}

/* ---- SRTCP (srtcp.c:143-287: the receiver is the replay window alone) - */

static uint32_t rtcp_batch(uint64_t lix, uint64_t bitmap, const uint32_t *ixv,
			   uint32_t n, struct plan_win *after)
{
	struct sgpu_rplan_in in;
	struct plan_win w = {lix, bitmap};
	uint32_t fail = 0, i;
	memset(&in, 0, sizeof(in));
	in.n = n;
	in.ssrc = 0x1234;
	in.tag = 10;
	in.hmac = 1;
	in.lix = lix;
	in.bitmap = bitmap;
	in.maxlen = 1u << 20;
	for (i = 0; i < n; i++) {
		const uint32_t E = i & 1;
		const uint32_t p = 64 * i, e = p + 60;
		const struct plan_rtcp r = plan_rtcp_packet(
			in, i, 1, 0x1234, 0x1234, e - p,
			plan_window_flags(p, e, 0, 0, 1u << 20, in.maxlen, 0, 0),
			ixv[i] | E << 31, i ? ixv[i - 1] | 0x80000000u : 0u);
		fail |= r.flags;
		CHECK(r.ix == ixv[i] && r.E == E, "rtcp index word");
		CHECK(plan_rtcp_desc(r.ix, r.E) ==
		      ((uint64_t)ixv[i] | (uint64_t)E << 31 | (uint64_t)SD_RUN << 48),
		      "rtcp desc");
	}
	*after = w;
	if (fail)
		return fail;    /* no plan: no state after it */
	i = 0;
	if (n > 65) {
		i = n - 65;
		w.lix = ixv[i - 1];
		w.bitmap = 1;
	}
	for (; i < n; i++)
		w = plan_win_step(w, ixv[i]);
	*after = w;
	return 0;
}

static void rtcp_accept(uint64_t lix, uint64_t bitmap, const uint32_t *ixv,
			uint32_t n, const char *what)
{
	struct plan_win w;
	struct rx r = {0, 0, lix, bitmap};
	uint32_t i;
	const uint32_t fail = rtcp_batch(lix, bitmap, ixv, n, &w);
	CHECK(fail == 0, "rtcp %s: n %u rejected %x", what, n, fail);
	for (i = 0; i < n; i++)
		CHECK(ref_replay_check(&r, ixv[i]), "rtcp %s: n %u packet %u",
		      what, n, i);
	CHECK(r.lix == w.lix && r.bitmap == w.bitmap, "rtcp %s: n %u window",
	      what, n);
}

static void check_rtcp(void)
{
	uint32_t ixv[NMAX], a, i;
	struct plan_win w;
	const uint64_t bm = 0xf0f0a5a5c3c30f01ull;
	for (a = 0; a < 6; a++) {
		const uint32_t n = g_len[a];
		for (i = 0; i < n; i++)
			ixv[i] = i ? ixv[i - 1] + 1 + i % 5 : 1;
		rtcp_accept(0, 0, ixv, n, "fresh");
		for (i = 0; i < n; i++)
			ixv[i] = i ? ixv[i - 1] + 1 + i % 70 : 70001;
		rtcp_accept(70000, bm, ixv, n, "continuing");
		ixv[0] = 70000 - 5;             /* in the window, bit clear */
		rtcp_accept(70000, bm, ixv, n, "first in window");
	}
	for (i = 0; i < 66; i++)
		ixv[i] = 70000 + i;
	CHECK(rtcp_batch(70000, bm, ixv, 66, &w) == SPF_REPLAY,
	      "rtcp first on a set bit");
	ixv[0] = 70000 - 64;
	CHECK(rtcp_batch(70000, bm, ixv, 66, &w) == SPF_REPLAY,
	      "rtcp first below the window");
	/* packet 0 below lix on a clear bit, packet 1 above it on a set bit of
	 * the window: the receiver says EALREADY to packet 1 */
	ixv[0] = 69941;                 /* bit 59: clear */
	ixv[1] = 69945;                 /* bit 55: set */
	for (i = 2; i < 66; i++)
		ixv[i] = 70000 + i;
	CHECK(rtcp_batch(70000, bm, ixv, 66, &w) == SPF_REPLAY,
	      "rtcp late first, second on a set bit");
	CHECK(rtcp_batch(70000, bm, ixv, 2, &w) == SPF_REPLAY,
	      "rtcp late first, second on a set bit, n 2");
}

#define RTCP_RANDOM 200000u

/* plan_rtcp_packet + plan_win_step against the sequential replay check, on
 * short batches around the stored window: whatever the rule accepts, the
 * receiver accepts packet by packet and leaves the same window.  The two
 * shares at the end keep the generator honest: the rule must accept a good
 * part of the batches, and the receiver must turn a packet down in a good
 * part of them (a rule that accepted those would be caught). */
static void check_rtcp_random(void)
{
	uint32_t ixv[6], b, i, k, accepted = 0, refused = 0;
	for (b = 0; b < RTCP_RANDOM; b++) {
		const uint32_t n = 1 + rnd() % 6;
		uint64_t lix = 0, bitmap = 0;
		struct plan_win w;
		struct rx r;
		uint32_t lo, down = 0;
		if (b % 3) {
			lix = b % 3 == 1 ? 40 + rnd() % 60 : 70000;
			bitmap = ((uint64_t)rnd() << 40 ^ (uint64_t)rnd() << 20 ^
				  rnd()) | 1;
			/* no history below index 0 */
			if (lix < 63)
				bitmap &= (2ull << lix) - 1;
		}
		lo = lix > 70 ? (uint32_t)lix - 70 : 0;
		for (i = 0; i < n; i++)
			ixv[i] = lo + rnd() % ((uint32_t)lix + 70 - lo + 1);
		if (rnd() & 3) {                /* three in four: ascending */
			for (i = 1; i < n; i++) {
				const uint32_t t = ixv[i];
				for (k = i; k > 0 && ixv[k - 1] > t; k--)
					ixv[k] = ixv[k - 1];
				ixv[k] = t;
			}
		}
		r.roc = 0;
		r.s_l = 0;
		r.lix = lix;
		r.bitmap = bitmap;
		for (i = 0; i < n; i++)
			down += !ref_replay_check(&r, ixv[i]);
		refused += down != 0;
		if (rtcp_batch(lix, bitmap, ixv, n, &w))
			continue;
		accepted++;
		CHECK(down == 0, "rtcp random: lix %llu bitmap %llx n %u (%u %u %u "
		      "%u %u %u): the receiver turns %u down",
		      (unsigned long long)lix, (unsigned long long)bitmap, n, ixv[0],
		      n > 1 ? ixv[1] : 0, n > 2 ? ixv[2] : 0, n > 3 ? ixv[3] : 0,
		      n > 4 ? ixv[4] : 0, n > 5 ? ixv[5] : 0, down);
		CHECK(down || (r.lix == w.lix && r.bitmap == w.bitmap),
		      "rtcp random: lix %llu n %u: window (%llx, %llx), not "
		      "(%llx, %llx)", (unsigned long long)lix, n,
		      (unsigned long long)w.lix, (unsigned long long)w.bitmap,
		      (unsigned long long)r.lix, (unsigned long long)r.bitmap);
	}
	printf("rtcp random: %u of %u batches accepted, the receiver turns a "
	       "packet down in %u\n", accepted, RTCP_RANDOM, refused);
	CHECK(accepted >= RTCP_RANDOM * 3 / 10, "rtcp random: %u accepted",
	      accepted);
	CHECK(refused >= RTCP_RANDOM * 3 / 10, "rtcp random: %u refused", refused);
}

int main(void)
{
	check_index();
	check_accept();
	check_reject();
	check_random();
	check_rtcp();
	check_rtcp_random();
	printf("%d wrong\n", g_bad);
	return g_bad ? 1 : 0;
}
