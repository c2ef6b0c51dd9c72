/*
 * rx_seg_check.c -- the receive rule for many streams in one scan
 * (re_amd/csrc/hip/plan_rx_rule.h: struct rx_seg, rx_seg_combine, compiled
 * as C) in the decomposition of k_bp_rx_plan (plan_buckets_rx.hip), against
 * each stream alone through the one-stream composition (as
 * srtp_rx_plan_host, batch_dev.c) and against a sequential receiver written
 * after the reference's srtp_decrypt.
 *
 * A batch interleaves 2-40 sessions at random, up to 4096 packets, each
 * session's arrivals network-shaped (loss, swaps, displacement, duplicates),
 * sequence numbers starting near 100, 32700 or 65000 (rollovers inside),
 * fresh and continuing states; some batches carry a session the rule must
 * leave unsettled.  A second series starts the continuing sessions one and
 * two rollovers below ROC 2^16, 2^31 and 2^32, beside fresh sessions at ROC
 * 0: the reference's index is sign-extended from 2^31 on (misc.c:22-41, the
 * sequential receiver here does the same), and a session that gets there
 * must be left unsettled.  Each batch runs twice:
 *
 *   (a) grouped by session and scanned as the kernel does: EPT consecutive
 *       sorted positions per "thread", the threads' aggregates scanned with
 *       the segmented combine inside "waves" of W lanes and across them --
 *       small EPT and W, so a segment head sits next to every thread and
 *       wave boundary;
 *   (b) every session alone: blocks of `block` packets, the aggregates'
 *       scan, u[] / Mx[], rx_settle -- and the sequential receiver.
 *
 * (a) must settle exactly the batches (b) settles, with identical verdicts,
 * u[] and final (roc, s_l, lix, bitmap) per session, and every settled
 * batch must equal the sequential receiver.
 *
 *   gcc -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -o rx_seg_check tests/c/rx_seg_check.c && ./rx_seg_check
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../re_amd/csrc/hip/plan_rx_rule.h"

#define NMAX 4096
#define SMAX 40
#define SEGMAX 1024

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

static uint32_t g_rng = 0x2545f491u;

static uint32_t rnd(void)
{
	g_rng = g_rng * 1664525u + 1013904223u;
	return g_rng >> 8;
}

/* true with probability pm / 1000 */
static int chance(uint32_t pm)
{
	return rnd() % 1000u < pm;
}

/* ---- the sequential receiver ---------------------------------------- */

struct rx {
	uint32_t roc;
	uint16_t s_l;
	int s_l_set;
	uint64_t lix, bitmap;
};

enum { SQ_OK = 0, SQ_TIMEDOUT, SQ_ALREADY };

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

/* srtp_decrypt (srtp.c:309-321, 367, 426-427) for an authentic packet; a
 * stream without s_l takes the packet's seq (stream.c:87-109) */
static int ref_packet(struct rx *r, uint16_t seq, uint64_t *ix)
{
	int diff;
	if (!r->s_l_set) {
		r->s_l = seq;
		r->s_l_set = 1;
	}
	diff = (int)seq - (int)r->s_l;
	if (diff > 32768)
		return SQ_TIMEDOUT;
	if (diff <= -32768) {
		r->roc++;
		r->s_l = 0;
	}
	*ix = ref_get_index(r->roc, r->s_l, seq);
	if (!ref_replay_check(r, *ix))
		return SQ_ALREADY;
	if (seq > r->s_l)
		r->s_l = seq;
	return SQ_OK;
}

/* ---- a batch --------------------------------------------------------- */

struct batch {
	uint32_t n, ns;
	uint16_t seq[NMAX];
	uint8_t sess[NMAX];
	struct rx st0[SMAX];
};

/* what a run leaves: settled or not; per packet (arrival order) index and
 * verdict; per session the state after the batch */
struct result {
	int settled;
	int64_t u[NMAX];
	uint8_t v[NMAX];
	struct rx st1[SMAX];
};

static int64_t h0_of(const struct rx *st, uint16_t seq0)
{
	return (int64_t)(((uint64_t)st->roc << 16) |
			 (st->s_l_set ? st->s_l : seq0));
}

static void state_after(struct rx *o, const struct rx *st, int64_t H0,
			int64_t smx, uint64_t bits)
{
	const int64_t lix0 = (int64_t)st->lix;
	const int64_t Mn = rx_max(H0, smx), lix = rx_max(lix0, smx);
	o->roc = (uint32_t)((uint64_t)Mn >> 16);
	o->s_l = (uint16_t)((uint64_t)Mn & 0xffffu);
	o->s_l_set = 1;
	o->lix = (uint64_t)lix;
	o->bitmap = rx_bitmap_base(lix, lix0, st->bitmap) | bits;
}

/* ---- (a): the kernel's decomposition --------------------------------- */

static void run_kernel_shape(const struct batch *B, uint32_t ept, uint32_t W,
			     uint32_t K, int tagged, struct result *R)
{
	static uint32_t srt[NMAX];
	static int64_t u[NMAX], mx[NMAX], dv[NMAX];
	static uint8_t hd[NMAX];
	static struct rx_seg ta[NMAX + 64], tb[NMAX + 64], ex[NMAX + 64];
	uint32_t cnt[SMAX] = {0}, start[SMAX], fill[SMAX];
	int64_t h0[SMAX], smx[SMAX];
	uint64_t bits[SMAX] = {0};
	const uint32_t m = B->n;
	uint32_t nt, i, k, l, t, d, bad = 0;

	R->settled = 0;
	/* grouped by session, arrival order inside (the stable rank) */
	for (i = 0; i < m; i++)
		cnt[B->sess[i]]++;
	for (l = 0, k = 0; l < B->ns; l++) {
		start[l] = fill[l] = k;
		k += cnt[l];
	}
	for (i = 0; i < m; i++)
		srt[fill[B->sess[i]]++] = i;
	for (l = 0; l < B->ns; l++) {
		if (cnt[l])
			h0[l] = h0_of(&B->st0[l], B->seq[srt[start[l]]]);
		smx[l] = RX_NEG;
	}
	/* the elements */
	for (k = 0; k < m; k++) {
		l = B->sess[srt[k]];
		hd[k] = k == start[l];
		if (hd[k]) {
			int64_t u0 = 0;
			int bump = 0;
			if (rx_step(h0[l], B->seq[srt[k]], &u0, &bump)) {
				bad = 1;
				u0 = 0;
			}
			dv[k] = u0;
		}
		else {
			dv[k] = rx_sdiff16(B->seq[srt[k]], B->seq[srt[k - 1]]);
		}
	}
	/* each thread's aggregate of its ept consecutive positions */
	nt = (m + ept - 1) / ept;
	nt = (nt + W - 1) / W * W;
	for (t = 0; t < nt; t++) {
		struct rx_seg a = rx_seg_identity();
		for (d = 0; d < ept && t * ept + d < m; d++)
			a = rx_seg_combine(a, rx_seg_elem(dv[t * ept + d],
							  hd[t * ept + d]));
		ta[t] = a;
	}
	/* inclusive scan inside each wave of W lanes (the shuffle steps) */
	for (d = 1; d < W; d <<= 1) {
		for (t = 0; t < nt; t++)
			tb[t] = t % W >= d ? rx_seg_combine(ta[t - d], ta[t])
					   : ta[t];
		memcpy(ta, tb, nt * sizeof(ta[0]));
	}
	/* across the waves: the aggregates before, then the lane below */
	{
		struct rx_seg pre = rx_seg_identity();
		for (t = 0; t < nt; t++) {
			ex[t] = rx_seg_combine(pre, t % W ? ta[t - 1]
							  : rx_seg_identity());
			if (t % W == W - 1)
				pre = rx_seg_combine(pre, ta[t]);
		}
	}
	for (t = 0; t < nt; t++) {
		struct rx_seg run = ex[t];
		for (d = 0; d < ept && t * ept + d < m; d++) {
			k = t * ept + d;
			l = B->sess[srt[k]];
			mx[k] = rx_seg_mx(run, hd[k]);
			run = rx_seg_combine(run, rx_seg_elem(dv[k], hd[k]));
			u[k] = run.a.s;
			if (k + 1 == start[l] + cnt[l])
				smx[l] = run.a.m;
		}
	}
	if (bad)
		return;
	/* settle with segment-local indices */
	for (k = 0; k < m; k++) {
		const uint32_t f0 = start[B->sess[srt[k]]];
		const struct rx *st;
		int r;
		l = B->sess[srt[k]];
		st = &B->st0[l];
		r = rx_settle(u + f0, mx + f0, k - f0, B->seq[srt[k]], K, h0[l],
			      (int64_t)st->lix, st->bitmap, tagged);
		if (r == RX_UNSETTLED)
			return;
		R->u[srt[k]] = u[k];
		R->v[srt[k]] = (uint8_t)r;
		if (r == RX_OK)
			bits[l] |= rx_bit(rx_max((int64_t)st->lix, smx[l]), u[k]);
	}
	for (l = 0; l < B->ns; l++) {
		R->st1[l] = B->st0[l];
		if (cnt[l])
			state_after(&R->st1[l], &B->st0[l], h0[l], smx[l],
				    bits[l]);
	}
	R->settled = 1;
}

/* ---- (b): every session alone ---------------------------------------- */

/* one stream as srtp_rx_plan_host composes the rule; 0: not settled */
static int one_stream(const struct rx *st, const uint16_t *seq, uint32_t n,
		      uint32_t block, uint32_t K, int tagged, int64_t *uo,
		      uint8_t *vo, struct rx *st1)
{
	static struct rx_agg agg[SEGMAX + 1];
	static int64_t u[SEGMAX], mx[SEGMAX];
	const uint32_t nb = (n + block - 1) / block;
	struct rx_agg total = rx_identity();
	const int64_t H0 = h0_of(st, seq[0]);
	int64_t u0 = 0;
	uint64_t bits = 0;
	uint32_t b, i;
	int bump = 0;

	if (rx_step(H0, seq[0], &u0, &bump))
		return 0;
#define RX_ELEM(i) rx_elem((i) ? rx_sdiff16(seq[i], seq[(i) - 1]) : u0)
	for (b = 0; b < nb; b++) {
		struct rx_agg a = rx_identity();
		for (i = b * block; i < (b + 1) * block && i < n; i++)
			a = rx_combine(a, RX_ELEM(i));
		agg[b] = a;
	}
	for (b = 0; b < nb; b++) {
		const struct rx_agg a = agg[b];
		agg[b] = total;
		total = rx_combine(total, a);
	}
	for (b = 0; b < nb; b++) {
		struct rx_agg run = agg[b];
		for (i = b * block; i < (b + 1) * block && i < n; i++) {
			mx[i] = run.m;
			run = rx_combine(run, RX_ELEM(i));
			u[i] = run.s;
		}
	}
#undef RX_ELEM
	for (i = 0; i < n; i++) {
		const int r = rx_settle(u, mx, i, seq[i], K, H0, (int64_t)st->lix,
					st->bitmap, tagged);
		if (r == RX_UNSETTLED)
			return 0;
		uo[i] = u[i];
		vo[i] = (uint8_t)r;
		if (r == RX_OK)
			bits |= rx_bit(rx_max((int64_t)st->lix, total.m), u[i]);
	}
	state_after(st1, st, H0, total.m, bits);
	return 1;
}

static void run_alone(const struct batch *B, uint32_t block, uint32_t K,
		      int tagged, struct result *R)
{
	static uint16_t sq[SEGMAX];
	static uint32_t at[SEGMAX];
	static int64_t u[SEGMAX];
	static uint8_t v[SEGMAX];
	uint32_t l, i, c;

	R->settled = 1;
	for (l = 0; l < B->ns; l++) {
		struct rx seqst = B->st0[l];
		R->st1[l] = B->st0[l];
		for (i = 0, c = 0; i < B->n; i++)
			if (B->sess[i] == l) {
				at[c] = i;
				sq[c++] = B->seq[i];
			}
		if (!c)
			continue;
		if (!one_stream(&B->st0[l], sq, c, block, K, tagged, u, v,
				&R->st1[l])) {
			R->settled = 0;
			continue;
		}
		/* a settled stream is the sequential receiver's */
		for (i = 0; i < c; i++) {
			uint64_t ix = 0;
			const int r = ref_packet(&seqst, sq[i], &ix);
			CHECK(r != SQ_TIMEDOUT, "session %u packet %u: settled, "
			      "the receiver says ETIMEDOUT", l, i);
			if (r == SQ_TIMEDOUT)
				break;
			CHECK((r == SQ_ALREADY) == (v[i] == RX_DUP) &&
			      ix == (uint64_t)u[i],
			      "session %u packet %u: verdict %d index %lld, the "
			      "receiver %d %llu", l, i, v[i], (long long)u[i], r,
			      (unsigned long long)ix);
			R->u[at[i]] = u[i];
			R->v[at[i]] = v[i];
		}
		CHECK(seqst.roc == R->st1[l].roc && seqst.s_l == R->st1[l].s_l &&
		      seqst.lix == R->st1[l].lix &&
		      seqst.bitmap == R->st1[l].bitmap,
		      "session %u: state (%u %u %llu %llx), the receiver (%u %u "
		      "%llu %llx)", l, R->st1[l].roc, R->st1[l].s_l,
		      (unsigned long long)R->st1[l].lix,
		      (unsigned long long)R->st1[l].bitmap, seqst.roc, seqst.s_l,
		      (unsigned long long)seqst.lix,
		      (unsigned long long)seqst.bitmap);
	}
}

/* ---- traffic ---------------------------------------------------------- */

/* arrival order of c sent packets (as network_shaped, tests/
 * test_gpu_rxplan.py, with higher rates: the sessions are short): loss,
 * adjacent swaps, displacement by up to 8, duplicates of one of the last
 * 32 arrivals (of the last K / 2 under a shorter look-back, so that most
 * batches still settle); at most cap arrivals.  Returns how many. */
static uint32_t network_shaped(uint32_t c, uint32_t *out, uint32_t cap,
			       uint32_t K)
{
	static uint32_t a[SEGMAX];
	uint32_t n = 0, i, k = 0;
	for (i = 0; i < c; i++)
		if (!chance(20))
			a[n++] = i;
	for (i = 0; i + 1 < n; i++)
		if (chance(40)) {
			const uint32_t x = a[i];
			a[i] = a[i + 1];
			a[i + 1] = x;
			i++;
		}
	for (i = n; i-- > 0;)
		if (chance(20)) {
			const uint32_t x = a[i];
			uint32_t to = i + 1 + rnd() % 8u, j;
			if (to >= n)
				to = n - 1;
			for (j = i; j < to; j++)
				a[j] = a[j + 1];
			a[to] = x;
		}
	for (i = 0; i < n && k < cap; i++) {
		out[k++] = a[i];
		if (chance(15) && k < cap) {
			const uint32_t far = K / 2 < 32 ? K / 2 : 32;
			const uint32_t back = 1 + rnd() % (k < far ? k : far);
			out[k] = out[k - back];
			k++;
		}
	}
	return k;
}

static const uint16_t S0[3] = {100, 32700, 65000};

/* the continuing sessions' ROC: g_roc0 + 0..g_rocn-1; g_cross: the victim
 * session continues at g_roc0 + 1 from 65000 and rolls over in the batch */
static uint32_t g_roc0, g_rocn = 3;
static int g_cross;

/*
 * A batch.  unsettled 1: one session gets a copy of its top packet more
 * than K of its own arrivals after it, the arrivals between (copies of the
 * packets just below) not moving the top; 2: one session starting at 65000
 * gets a packet from before its rollover after it.
 */
static void make_batch(struct batch *B, uint32_t K, int unsettled)
{
	static uint32_t ord[SMAX][SEGMAX];
	uint32_t cnt[SMAX], left[SMAX], first[SMAX];
	uint32_t l, total = 0, budget = NMAX, i;
	const uint32_t victim = rnd() % 2u;     /* among the first sessions */

	B->ns = 2 + rnd() % (SMAX - 1);
	for (l = 0; l < B->ns; l++) {
		struct rx *st = &B->st0[l];
		uint16_t s0 = S0[rnd() % 3u];
		uint32_t c = 1 + rnd() % (rnd() % 4u ? 160u : 1000u), k;
		uint32_t room = budget / (B->ns - l);
		if (room > SEGMAX)
			room = SEGMAX;
		memset(st, 0, sizeof(*st));
		if (l == victim && (unsettled || g_cross)) {
			if (unsettled == 2 || g_cross)
				s0 = 65000;
			c = 600 + rnd() % 100u;
			if (c + K + 16 > room)
				room = c + K + 16;      /* (the first sessions) */
		}
		if (c > room)
			c = room;
		if (rnd() % 2u || (l == victim && (unsettled == 2 || g_cross))) {
			/* continuing: `pre` packets up to s0 - 1 received */
			const uint32_t pre = 1 + rnd() % 100u;
			uint64_t ix;
			st->roc = g_roc0 + rnd() % g_rocn;
			if (l == victim && g_cross)
				st->roc = g_roc0 + 1;
			for (k = 0; k < pre; k++)
				ref_packet(st, (uint16_t)(s0 - pre + k), &ix);
		}
		first[l] = s0;
		k = network_shaped(c, ord[l], room, K);
		if (!k) {
			ord[l][0] = 0;
			k = 1;
		}
		if (l == victim && unsettled == 1 && k > 220 + K) {
			/* from arrival 200 on: the top so far, K + 3 copies of the
			 * ten sent before it, the top again */
			uint32_t top = 0, q;
			for (q = 0; q < 200; q++)
				if (ord[l][q] > top)
					top = ord[l][q];
			ord[l][200] = top;
			for (q = 0; q < K + 3; q++)
				ord[l][201 + q] = top > 10 ? top - 1 - q % 10 : 0;
			ord[l][201 + K + 3] = top;
			for (q = 202 + K + 3; q < k && q < SEGMAX; q++)
				ord[l][q] = top + 1 + (q - (202 + K + 3));
		}
		if (l == victim && unsettled == 2 && k > 560) {
			/* in order, the packet sent at 530 arriving at 545 (the
			 * rollover is the packet sent at 536) */
			uint32_t q;
			for (q = 0; q < k; q++)
				ord[l][q] = q < 530 ? q : q < 545 ? q + 1 :
					    q == 545 ? 530 : q;
		}
		cnt[l] = left[l] = k;
		total += k;
		budget -= k;
	}
	/* interleaved at random, every session in its own order */
	B->n = total;
	for (i = 0; i < total; i++) {
		uint32_t r = rnd() % (total - i);
		for (l = 0; l < B->ns; l++) {
			if (r < left[l])
				break;
			r -= left[l];
		}
		B->sess[i] = (uint8_t)l;
		B->seq[i] = (uint16_t)(first[l] + ord[l][cnt[l] - left[l]]);
		left[l]--;
	}
}

static int same_state(const struct rx *a, const struct rx *b)
{
	return a->roc == b->roc && a->s_l == b->s_l &&
	       a->s_l_set == b->s_l_set && a->lix == b->lix &&
	       a->bitmap == b->bitmap;
}

int main(void)
{
	static struct batch B;
	static struct result Ra, Rb;
	static const uint32_t EPT[4] = {1, 2, 3, 4}, WV[3] = {2, 4, 8};
	static const uint32_t KV[3] = {16, RX_LOOKBACK, 24};
	static const uint32_t BLK[3] = {3, 8, 256};
	uint32_t trial, nset = 0, nuns = 0, i, l, b;

	for (trial = 0; trial < 400; trial++) {
		const uint32_t K = KV[trial % 3u];
		const int unsettled = trial % 8u == 3 ? 1 : trial % 8u == 6 ? 2 : 0;
		const int tagged = (trial / 3u) % 2u;
		const uint32_t ept = EPT[rnd() % 4u], W = WV[rnd() % 3u];
		make_batch(&B, K, unsettled);
		run_kernel_shape(&B, ept, W, K, tagged, &Ra);
		run_alone(&B, BLK[rnd() % 3u], K, tagged, &Rb);
		CHECK(Ra.settled == Rb.settled, "trial %u (ept %u W %u K %u): "
		      "kernel shape settled %d, alone %d", trial, ept, W, K,
		      Ra.settled, Rb.settled);
		if (unsettled)
			CHECK(!Rb.settled, "trial %u: the unsettled shape %d "
			      "settled", trial, unsettled);
		if (Ra.settled)
			nset++;
		else
			nuns++;
		if (!Ra.settled || !Rb.settled)
			continue;
		for (i = 0; i < B.n; i++)
			CHECK(Ra.u[i] == Rb.u[i] && Ra.v[i] == Rb.v[i],
			      "trial %u packet %u (session %u): kernel shape "
			      "%lld/%d, alone %lld/%d", trial, i, B.sess[i],
			      (long long)Ra.u[i], Ra.v[i], (long long)Rb.u[i],
			      Rb.v[i]);
		for (l = 0; l < B.ns; l++)
			CHECK(same_state(&Ra.st1[l], &Rb.st1[l]),
			      "trial %u session %u: states differ", trial, l);
	}
	CHECK(nset >= 100 && nuns >= 50, "%u settled, %u unsettled batches: the "
	      "traffic does not cover both", nset, nuns);
	printf("%u batches settled, %u unsettled; ", nset, nuns);
	/* continuing sessions at B - 2 and B - 1 for B = 2^16, 2^31, 2^32; in
	 * every other batch the victim crosses B.  At 2^16 that is an
	 * ordinary rollover: the traffic settles as often as above (a
	 * quarter of the batches at least).  A session that crosses 2^31 or
	 * 2^32, and one whose window is sign-extended already (every
	 * continuing one below 2^32), must not settle */
	for (b = 0; b < 3; b++) {
		static const uint32_t BASE[3] = {0xfffeu, 0x7ffffffeu, 0xfffffffeu};
		uint32_t ns2 = 0;
		g_roc0 = BASE[b];
		g_rocn = 2;
		for (trial = 0; trial < 60; trial++) {
			const uint32_t K = KV[trial % 3u];
			const int tagged = (trial / 3u) % 2u;
			const uint32_t ept = EPT[rnd() % 4u], W = WV[rnd() % 3u];
			g_cross = trial % 2u;
			make_batch(&B, K, 0);
			run_kernel_shape(&B, ept, W, K, tagged, &Ra);
			run_alone(&B, BLK[rnd() % 3u], K, tagged, &Rb);
			CHECK(Ra.settled == Rb.settled, "roc %#x trial %u (ept %u W "
			      "%u K %u): kernel shape settled %d, alone %d", g_roc0,
			      trial, ept, W, K, Ra.settled, Rb.settled);
			if (b && g_cross)
				CHECK(!Rb.settled && !Ra.settled, "roc %#x trial %u: a "
				      "session crossed and settled", g_roc0, trial);
			if (!Ra.settled || !Rb.settled)
				continue;
			ns2++;
			for (i = 0; i < B.n; i++)
				CHECK(Ra.u[i] == Rb.u[i] && Ra.v[i] == Rb.v[i],
				      "roc %#x trial %u packet %u: kernel shape "
				      "%lld/%d, alone %lld/%d", g_roc0, trial, i,
				      (long long)Ra.u[i], Ra.v[i], (long long)Rb.u[i],
				      Rb.v[i]);
			for (l = 0; l < B.ns; l++)
				CHECK(same_state(&Ra.st1[l], &Rb.st1[l]), "roc %#x trial "
				      "%u session %u: states differ", g_roc0, trial, l);
		}
		CHECK(b || ns2 >= 15, "roc %#x: %u of 60 batches settled", g_roc0,
		      ns2);
		printf("roc %#x: %u of 60 settled; ", g_roc0, ns2);
	}
	printf("%d wrong\n", g_bad);
	return g_bad ? 1 : 0;
}
