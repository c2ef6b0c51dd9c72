/*
 * rtcp_str_check.c -- the one-session SRTCP planner's composition
 * (re_amd/csrc/hip/plan_rtcp_str.h over plan_rtcp_seg.h / plan_rtcp_seg_rx.h,
 * compiled as C) in the decomposition of plan_streams_rtcp.hip, against a
 * sequential restatement, written here, of stream_get (stream.c:29-84), of the
 * sender's index step (srtcp.c:54) and of the receiver's replay step on HMAC
 * suites (srtcp.c:208 + replay.c:32-62).
 *
 * A world is one session whose sender uses 1-9 SSRCs; the sender's table and
 * the two receivers' (one with a replay window: HMAC suites, one without:
 * GCM) are carried from batch to batch.  Tables start with known streams
 * (some of them streams RTP created: zero SRTCP state), with room for new
 * ones or none; streams start anywhere, some at 0x7ffffff0 (the 31-bit wrap),
 * some receivers' windows so that the first arrival lies at lix - 63, at
 * lix - 64 or on a set bit.  Per batch: protect, then the protected packets
 * arrive disturbed per stream -- swaps (adjacent and up to 8 apart),
 * duplicates, replays of the batch before -- and are unprotected with and
 * without a window.  Each of the three runs
 *
 *   (a) as the kernels do: the table after the batch, per packet its slot and
 *       checks, per "workgroup" of B packets and per slot a count taken wave
 *       by wave (W lanes), the counts' exclusive sums over the workgroups by S
 *       scan "threads", the stable partition (rstr_place), then protect: the
 *       rank numbers the packet; GCM: the packet's own word; HMAC: the
 *       three-phase segmented (sum, max) scan (workgroup aggregates by a
 *       doubling scan over B, their exclusive scan by S threads, u[] / mx[]),
 *       rsrx_verdict per place with look-back K, the records after -- small B,
 *       W, S and K so that runs, look-backs and seams cross every border;
 *   (b) packet by packet through the sequential sender / receiver.
 *
 * An accepted plan must equal (b) packet for packet (index, verdict, E in
 * desc) and record for record.  The accepted batches must be exactly those
 * with at most 8 streams that, with a window, the sequential per-stream
 * rx_replay settles with the same look-back.
 *
 *   rtcp_str_check           the random worlds
 *   rtcp_str_check FILE      a recorded traffic (lines "B", then "ssrc index"
 *                            per arrival; the table starts empty): per batch
 *                            the sequential receiver's errno counts and
 *                            whether (a) takes it at the kernels' own widths
 *
 *   gcc -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -o rtcp_str_check tests/c/rtcp_str_check.c && ./rtcp_str_check
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../re_amd/csrc/hip/plan_rtcp_str.h"

#define NMAX 1400
#define NRAND 600               /* a random world's batch, at most */
#define KMAX (RSEG_MAX + 1)     /* SSRCs the sender may use */
#define BMAX 256                /* "workgroup" width, at most */
#define SMAXT 1024              /* scan "threads", at most */
#define LASTN 4                 /* words of the batch before kept for replays */
#define IXMASK 0x7fffffffu
#define PKT_L 64u

enum { TX = 0, RXH = 1, RXG = 2 };

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

static uint32_t g_rng = 0x5eed1e55u;

static uint32_t rnd(void)
{
	g_rng = g_rng * 1664525u + 1013904223u;
	return g_rng >> 8;
}

static int chance(uint32_t pm)
{
	return rnd() % 1000u < pm;
}

struct tab {
	uint32_t n;
	struct rseg_rec st[RSEG_MAX];
};

struct pkt {
	uint32_t ssrc, word;    /* E || index (unprotect) */
};

struct batch {
	uint32_t n, encrypted;
	struct tab t0;
	struct pkt p[NMAX];
};

static struct sgpu_rplan_in plan_in(uint32_t n, int mode, uint32_t encrypted)
{
	struct sgpu_rplan_in c;
	memset(&c, 0, sizeof(c));
	c.n = n;
	c.prot = mode == TX;
	c.tag = mode == RXG ? 0 : 10;
	c.gcm = mode == RXG;
	c.hmac = mode != RXG;
	c.encrypted = encrypted;
	c.need = 4 + c.tag + (c.gcm ? 16u : 0u);
	c.maxlen = 1u << 20;
	return c;
}

/* ---- (b) the sequential sender and receiver ----------------------------- */

/* replay.c:32-62 */
static int ref_replay_check(uint64_t *lix, uint64_t *bitmap, uint64_t ix)
{
	uint64_t diff;
	if (ix > *lix) {
		diff = ix - *lix;
		*bitmap = diff < 64 ? (*bitmap << diff) | 1 : 1;
		*lix = ix;
		return 1;
	}
	diff = *lix - ix;
	if (diff >= 64 || (*bitmap & (1ULL << diff)))
		return 0;
	*bitmap |= 1ULL << diff;
	return 1;
}

/* stream.c:29-84 */
static int ref_stream_get(struct tab *t, uint32_t ssrc, struct rseg_rec **sp)
{
	uint32_t i;
	for (i = 0; i < t->n; i++)
		if (t->st[i].ssrc == ssrc) {
			*sp = &t->st[i];
			return 0;
		}
	if (t->n >= RSEG_MAX)
		return ENOSR;
	*sp = &t->st[t->n++];
	memset(*sp, 0, sizeof(**sp));
	(*sp)->ssrc = ssrc;
	return 0;
}

/* per packet errno (0, EALREADY, ENOSR) and the desc word its job runs with */
static void sequential(const struct batch *B, int mode, struct tab *t, int *err,
		       uint64_t *desc)
{
	uint32_t i;
	*t = B->t0;
	for (i = 0; i < B->n; i++) {
		const struct pkt *p = &B->p[i];
		struct rseg_rec *st;
		uint64_t lix, bm;
		desc[i] = 0;
		err[i] = ref_stream_get(t, p->ssrc, &st);
		if (err[i])
			continue;
		if (mode == TX) {
			/* srtcp.c:54 */
			st->ix = (st->ix + 1) & IXMASK;
			desc[i] = plan_rtcp_desc(st->ix, B->encrypted);
			continue;
		}
		if (mode == RXG) {
			desc[i] = plan_rtcp_desc(p->word & IXMASK, p->word >> 31);
			continue;
		}
		lix = st->ix;
		bm = (uint64_t)st->bhi << 32 | st->blo;
		if (!ref_replay_check(&lix, &bm, p->word & IXMASK)) {
			/* authenticated, never deciphered */
			err[i] = EALREADY;
			desc[i] = plan_rtcp_desc(p->word & IXMASK, 0);
			continue;
		}
		desc[i] = plan_rtcp_desc(p->word & IXMASK, p->word >> 31);
		st->ix = (uint32_t)lix;
		st->blo = (uint32_t)bm;
		st->bhi = (uint32_t)(bm >> 32);
	}
}

/* ---- (a) the kernels' decomposition -------------------------------------- */

struct geo {
	uint32_t B, W, S, K;    /* W divides B, both powers of two */
};

/* what sgpu_splan_table gives: the known streams, then the new SSRCs by first
 * appearance; a 9th: SPF_SSRC */
static uint32_t table_after(const struct batch *B, uint32_t *ssrcs, uint32_t *nt)
{
	uint32_t i, q, f = 0;
	*nt = B->t0.n;
	for (q = 0; q < RSEG_MAX; q++)
		ssrcs[q] = q < B->t0.n ? B->t0.st[q].ssrc : 0;
	for (i = 0; i < B->n; i++) {
		for (q = 0; q < *nt; q++)
			if (ssrcs[q] == B->p[i].ssrc)
				break;
		if (q < *nt)
			continue;
		if (*nt >= RSEG_MAX) {
			f |= SPF_SSRC;
			continue;
		}
		ssrcs[(*nt)++] = B->p[i].ssrc;
	}
	return f;
}

/* a workgroup's inclusive segmented scan by doubling, as the kernels': every
 * thread reads before any thread writes */
static void block_scan(struct rx_seg *e, uint32_t width)
{
	struct rx_seg v[BMAX > SMAXT ? BMAX : SMAXT];
	uint32_t d, t;
	for (d = 1; d < width; d <<= 1) {
		for (t = 0; t < width; t++)
			v[t] = t >= d ? e[t - d] : rx_seg_identity();
		for (t = 0; t < width; t++)
			e[t] = rx_seg_combine(v[t], e[t]);
	}
}

static struct rx_seg elem_at(const uint32_t *start, const uint32_t *cnt,
			     const uint32_t *sw, uint32_t p, uint32_t n)
{
	uint32_t q;
	int head;
	if (p >= n)
		return rx_seg_identity();
	q = rstr_slot_at(start, cnt, p);
	if (q == RSEG_NONE)
		return rx_seg_identity();
	head = rstr_head(p, start[q]);
	return rx_seg_elem(rsrx_elem(head, sw[p], head ? 0u : sw[p - 1]), head);
}

/* 0 accepted (desc[], vd[], *t: the plan), else the SPF_* bits */
static uint32_t planned(const struct batch *B, int mode, struct geo G,
			struct tab *t, uint64_t *desc, int *vd, uint32_t *nlate,
			uint32_t *ndup)
{
	const struct sgpu_rplan_in in = plan_in(B->n, mode, B->encrypted);
	const uint32_t n = B->n, nb = (n + G.B - 1) / G.B;
	static uint8_t slot[NMAX];
	static uint32_t bcnt[RSEG_MAX][NMAX], perm[NMAX], sw[NMAX];
	static int64_t u[NMAX], mx[NMAX];
	static struct rx_seg agg[NMAX];
	uint32_t ssrcs[RSEG_MAX], nt, start[RSEG_MAX], cnt[RSEG_MAX];
	uint64_t bits[RSEG_MAX];
	struct rseg_rec rec[RSEG_MAX];
	uint32_t fail, b, i, q, w, p;

	*t = B->t0;
	*nlate = *ndup = 0;
	fail = table_after(B, ssrcs, &nt);
	/* count: per packet slot and checks, per workgroup and slot the wave
	 * counts summed */
	for (b = 0; b < nb; b++)
		for (q = 0; q < RSEG_MAX; q++) {
			uint32_t s = 0;
			for (w = 0; w < G.B / G.W; w++) {
				uint32_t c = 0, l;
				for (l = 0; l < G.W; l++) {
					i = b * G.B + w * G.W + l;
					if (i >= n)
						continue;
					if (q == 0) {
						const uint32_t k = rstr_slot(
							ssrcs, nt, B->p[i].ssrc);
						slot[i] = (uint8_t)k;
						if (k == RSEG_NONE)
							fail |= SPF_SSRC;
						fail |= rstr_flags(in, B->p[i].ssrc,
								   1, PKT_L, 0,
								   B->p[i].word);
					}
					c += slot[i] == q;
				}
				s += c;
			}
			bcnt[q][b] = s;
		}
	/* starts: S threads, each over `per` consecutive workgroups */
	{
		const uint32_t per = (nb + G.S - 1) / G.S;
		uint32_t tot[RSEG_MAX];
		for (q = 0; q < RSEG_MAX; q++) {
			uint32_t part[SMAXT], th, run = 0;
			for (th = 0; th < G.S; th++) {
				const uint32_t a = th * per < nb ? th * per : nb;
				const uint32_t e = a + per < nb ? a + per : nb;
				part[th] = run;
				for (b = a; b < e; b++)
					run += bcnt[q][b];
			}
			for (th = G.S; th-- > 0;) {
				const uint32_t a = th * per < nb ? th * per : nb;
				const uint32_t e = a + per < nb ? a + per : nb;
				uint32_t r = part[th];
				for (b = a; b < e; b++) {
					const uint32_t v = bcnt[q][b];
					bcnt[q][b] = r;
					r += v;
				}
			}
			tot[q] = run;
		}
		rstr_starts(tot, start);
		memcpy(cnt, tot, sizeof(cnt));
	}
	if (fail)
		return fail;
	for (q = 0; q < RSEG_MAX; q++) {
		const struct rseg_rec none = {0, 0, 0, 0};
		rec[q] = rstr_rec(q < B->t0.n ? B->t0.st[q] : none, q, B->t0.n,
				  ssrcs[q]);
		bits[q] = 0;
	}
	/* place: the stable partition, lanes and waves in any order */
	for (i = n; i-- > 0;) {
		const uint32_t k = slot[i], b0 = i / G.B * G.B;
		const uint32_t w0 = (i - b0) / G.W * G.W + b0;
		uint32_t ahead = 0, j;
		for (j = w0; j < i; j++)        /* the lanes before in its wave */
			ahead += slot[j] == k;
		for (j = b0; j < w0; j++)       /* the waves before */
			ahead += slot[j] == k;
		p = rstr_place(start[k], bcnt[k][i / G.B], ahead);
		CHECK(p < n, "place %u of %u", p, n);
		if (p >= n)
			return SPF_BAD;
		if (mode == TX) {
			const struct plan_rtcp r =
				rstr_tx(in, rec[k], p, start[k], 1, PKT_L, 0);
			desc[i] = plan_rtcp_desc(r.ix, r.E);
			vd[i] = RX_OK;
		}
		else if (mode == RXG) {
			desc[i] = rsrx_desc(RX_OK, B->p[i].word);
			vd[i] = RX_OK;
		}
		else {
			perm[p] = i;
			sw[p] = B->p[i].word;
		}
	}
	if (mode == RXH) {
		static struct rx_seg sh[BMAX], part[SMAXT];
		const uint32_t per = (nb + G.S - 1) / G.S;
		uint32_t th;
		/* agg */
		for (b = nb; b-- > 0;) {
			for (i = 0; i < G.B; i++)
				sh[i] = elem_at(start, cnt, sw, b * G.B + i, n);
			block_scan(sh, G.B);
			agg[b] = sh[G.B - 1];
		}
		/* scan: exclusive, S threads */
		for (th = 0; th < G.S; th++) {
			const uint32_t a = th * per < nb ? th * per : nb;
			const uint32_t e = a + per < nb ? a + per : nb;
			part[th] = rx_seg_identity();
			for (b = a; b < e; b++)
				part[th] = rx_seg_combine(part[th], agg[b]);
		}
		{
			/* (S need not be a power of two here: doubling holds) */
			block_scan(part, G.S);
		}
		for (th = G.S; th-- > 0;) {
			const uint32_t a = th * per < nb ? th * per : nb;
			const uint32_t e = a + per < nb ? a + per : nb;
			struct rx_seg run = th ? part[th - 1] : rx_seg_identity();
			for (b = a; b < e; b++) {
				const struct rx_seg v = agg[b];
				agg[b] = run;
				run = rx_seg_combine(run, v);
			}
		}
		/* index */
		for (b = nb; b-- > 0;) {
			struct rx_seg el[BMAX];
			for (i = 0; i < G.B; i++)
				el[i] = sh[i] = elem_at(start, cnt, sw, b * G.B + i, n);
			block_scan(sh, G.B);
			for (i = 0; i < G.B; i++) {
				struct rx_seg ex;
				p = b * G.B + i;
				if (p >= n)
					continue;
				ex = rx_seg_combine(agg[b], i ? sh[i - 1]
							      : rx_seg_identity());
				mx[p] = rx_seg_mx(ex, (int)el[i].head);
				u[p] = rx_seg_combine(ex, el[i]).a.s;
			}
		}
		/* settle */
		for (p = n; p-- > 0;) {
			uint32_t f0;
			int r;
			q = rstr_slot_at(start, cnt, p);
			CHECK(q != RSEG_NONE, "place %u in no run", p);
			if (q == RSEG_NONE)
				return SPF_BAD;
			f0 = start[q];
			r = rsrx_verdict(u + f0, mx + f0, rstr_rank(p, f0), G.K,
					 rec[q]);
			if (r == RX_UNSETTLED) {
				fail |= SPF_REPLAY;
				continue;
			}
			i = perm[p];
			desc[i] = rsrx_desc(r, sw[p]);
			vd[i] = r;
			if (r == RX_DUP) {
				(*ndup)++;
				continue;
			}
			bits[q] |= rsrx_bit(rec[q], rstr_smx(u, mx, f0, cnt[q]), u[p]);
			if (rsrx_late(u[p], rec[q], mx[p]))
				(*nlate)++;
		}
		if (fail)
			return fail;
	}
	/* final: the table after */
	t->n = nt;
	for (q = 0; q < nt; q++) {
		struct rseg_rec a = rec[q];
		if (cnt[q]) {
			if (mode == TX)
				a = rstr_tx_after(a, cnt[q]);
			else if (mode == RXH)
				a = rsrx_after(a, rstr_smx(u, mx, start[q], cnt[q]),
					       bits[q]);
		}
		t->st[q] = a;
	}
	return 0;
}

/* ---- which batches the planner must take --------------------------------- */

static int must_accept(const struct batch *B, int mode, uint32_t K,
		       const int *err)
{
	static int64_t u[NMAX], mx[NMAX];
	static uint8_t seen[NMAX];
	uint32_t i, j, c;
	for (i = 0; i < B->n; i++)
		if (err[i] == ENOSR)
			return 0;
	if (mode != RXH)
		return 1;
	memset(seen, 0, sizeof(seen));
	for (i = 0; i < B->n; i++) {
		struct rseg_rec st = rsrx_new(B->p[i].ssrc);
		int64_t m = RX_NEG;
		if (seen[i])
			continue;
		for (j = 0; j < B->t0.n; j++)
			if (B->t0.st[j].ssrc == B->p[i].ssrc)
				st = B->t0.st[j];
		for (j = i, c = 0; j < B->n; j++)
			if (B->p[j].ssrc == B->p[i].ssrc) {
				seen[j] = 1;
				u[c] = (int64_t)(B->p[j].word & IXMASK);
				mx[c] = m;
				m = rx_max(m, u[c]);
				c++;
			}
		for (j = 0; j < c; j++)
			if (rx_replay(u, mx, j, K, (int64_t)st.ix,
				      (uint64_t)st.bhi << 32 | st.blo, 1) ==
			    RX_UNSETTLED)
				return 0;
	}
	return 1;
}

/* arrivals at or below an earlier arrival of their stream */
static uint32_t disturbed(const struct batch *B)
{
	uint32_t i, j, d = 0;
	for (i = 0; i < B->n; i++)
		for (j = 0; j < i; j++)
			if (B->p[j].ssrc == B->p[i].ssrc &&
			    (B->p[j].word & IXMASK) >= (B->p[i].word & IXMASK)) {
				d++;
				break;
			}
	return d;
}

/* ---- worlds --------------------------------------------------------------- */

struct world {
	uint32_t nss;
	struct tab t[3];        /* TX, RXH, RXG */
	uint32_t last[KMAX][LASTN], nlast[KMAX];
};

static uint32_t ssrc_of(uint32_t k)
{
	return 0x53000000u | k << 4 | 1u;
}

enum { TR_NINTH = 1, TR_DUP = 2, TR_SWAP = 4, TR_REPLAY = 8, TR_WRAP = 16,
       TR_E63 = 32, TR_E64 = 64, TR_SET = 128, TR_RTP = 256 };

static uint32_t make_world(struct world *W)
{
	uint32_t done = 0, k, nk;
	memset(W, 0, sizeof(*W));
	W->nss = 1 + rnd() % RSEG_MAX;
	if (chance(120)) {
		W->nss = KMAX;
		done |= TR_NINTH;
	}
	nk = rnd() % ((W->nss < RSEG_MAX ? W->nss : RSEG_MAX) + 1);
	if (chance(150))
		nk = W->nss < RSEG_MAX ? W->nss : RSEG_MAX;     /* no room */
	for (k = 0; k < nk; k++) {
		uint32_t ix = 1 + rnd() % 5000, lix, blo, bhi;
		if (chance(200)) {
			ix = 0x7ffffff0u - rnd() % 4 * 4;
			done |= TR_WRAP;
		}
		lix = ix;
		blo = rnd() << 8 | rnd() | 1u;
		bhi = rnd() << 8 | rnd();
		if (chance(150)) {
			/* a stream RTP created: zero SRTCP state */
			ix = lix = blo = bhi = 0;
			done |= TR_RTP;
		}
		else if (chance(120)) {
			lix = ix + 1 + 63;      /* the first arrival at lix - 63 */
			blo &= ~0u;
			bhi &= 0x7fffffffu;     /* bit 63 clear */
			done |= TR_E63;
		}
		else if (chance(120)) {
			lix = ix + 1 + 64;      /* ... at lix - 64 */
			done |= TR_E64;
		}
		else if (chance(120)) {
			lix = ix + 1 + 5;       /* ... on a set bit */
			blo |= 1u << 5;
			done |= TR_SET;
		}
		lix &= IXMASK;
		W->t[TX].st[k] = (struct rseg_rec){ssrc_of(k), ix, 0, 0};
		W->t[RXH].st[k] = (struct rseg_rec){ssrc_of(k), lix, blo, bhi};
		W->t[RXG].st[k] = (struct rseg_rec){ssrc_of(k), 0, 0, 0};
	}
	W->t[TX].n = W->t[RXH].n = W->t[RXG].n = nk;
	return done;
}

/* the arrivals of what the sender made: per stream swaps, duplicates and
 * replays of the batch before */
static uint32_t disturb(struct world *W, struct batch *B, uint32_t pm)
{
	static uint32_t arr[NMAX];
	uint32_t done = 0, k, i, j, c;
	for (k = 0; k < W->nss; k++) {
		const uint32_t x = ssrc_of(k);
		for (i = 0, c = 0; i < B->n; i++)
			if (B->p[i].ssrc == x)
				arr[c++] = i;
		for (j = 0; j < c; j++) {
			uint32_t d, w;
			if (!chance(pm / 8))
				continue;
			switch (rnd() % 3) {
			case 0:
				d = chance(600) ? 1 : 1 + rnd() % 8;
				if (j + d >= c)
					break;
				w = B->p[arr[j]].word;
				B->p[arr[j]].word = B->p[arr[j + d]].word;
				B->p[arr[j + d]].word = w;
				done |= TR_SWAP;
				break;
			case 1:
				d = chance(800) ? 1 + rnd() % 5 : 1 + rnd() % 30;
				if (j + d >= c)
					break;
				B->p[arr[j + d]].word = B->p[arr[j]].word;
				done |= TR_DUP;
				break;
			default:
				if (!W->nlast[k])
					break;
				B->p[arr[j]].word = W->last[k][rnd() % W->nlast[k]];
				done |= TR_REPLAY;
				break;
			}
		}
		if (c) {
			W->nlast[k] = c < LASTN ? c : LASTN;
			for (j = 0; j < W->nlast[k]; j++)
				W->last[k][j] = B->p[arr[c - 1 - j]].word;
		}
	}
	return done;
}

/* ---- a recorded traffic --------------------------------------------------- */

static int replay_file(const char *path)
{
	static struct batch B;
	static struct tab ts, tp;
	static int err[NMAX], vdp[NMAX];
	static uint64_t ds[NMAX], dp[NMAX];
	/* plan_streams_rtcp.hip SRT_BLOCK, a wave, SRT_SCAN, RX_LOOKBACK */
	const struct geo G = {.B = 256, .W = 64, .S = 1024, .K = RX_LOOKBACK};
	FILE *f = fopen(path, "r");
	char line[128];
	uint32_t nbatch = 0;
	int more = 1;
	if (!f) {
		perror(path);
		return 2;
	}
	memset(&B, 0, sizeof(B));
	B.encrypted = 1;
	while (more) {
		unsigned x, q;
		more = fgets(line, sizeof(line), f) != NULL;
		if (more && line[0] != 'B' && sscanf(line, "%x %u", &x, &q) == 2) {
			if (B.n >= NMAX) {
				printf("batch %u: out of range\n", nbatch);
				fclose(f);
				return 2;
			}
			B.p[B.n].ssrc = x;
			B.p[B.n].word = (q & IXMASK) | 0x80000000u;
			B.n++;
			continue;
		}
		if (B.n) {
			uint32_t i, ne[3] = {0, 0, 0}, fail, nl, nd;
			sequential(&B, RXH, &ts, err, ds);
			fail = planned(&B, RXH, G, &tp, dp, vdp, &nl, &nd);
			for (i = 0; i < B.n; i++)
				ne[err[i] == 0 ? 0 : err[i] == EALREADY ? 1 : 2]++;
			printf("batch %u: %u packets ok %u already %u other %u "
			       "disturbed %u streams %u plan %s must %d\n", nbatch,
			       B.n, ne[0], ne[1], ne[2], disturbed(&B), ts.n,
			       fail ? "rejected" : "accepted",
			       must_accept(&B, RXH, G.K, err));
			B.t0 = ts;
			B.n = 0;
			nbatch++;
		}
	}
	fclose(f);
	return 0;
}

/* one run of a batch both ways; returns 1 accepted, 0 rejected */
static int both(const struct batch *B, int mode, struct geo G, struct tab *ts,
		uint64_t *ds, uint32_t it, uint32_t *nmust, uint32_t *unsettled,
		uint32_t *ndups, uint32_t *nlates)
{
	static struct tab tp;
	static int err[NMAX], vdp[NMAX];
	static uint64_t dp[NMAX];
	uint32_t fail, i, k, nl = 0, nd = 0, nea = 0;
	int must;
	sequential(B, mode, ts, err, ds);
	memset(dp, 0, sizeof(dp));
	memset(vdp, 0, sizeof(vdp));
	fail = planned(B, mode, G, &tp, dp, vdp, &nl, &nd);
	must = must_accept(B, mode, G.K, err);
	*nmust += (uint32_t)must;
	CHECK(!(must && fail), "it %u mode %d: rejected (SPF %#x) a batch it must "
	      "accept", it, mode, fail);
	CHECK(must || fail, "it %u mode %d: accepted a batch it must not", it, mode);
	if (fail) {
		*unsettled += fail == SPF_REPLAY;
		return 0;
	}
	for (i = 0; i < B->n; i++) {
		CHECK(err[i] == 0 || err[i] == EALREADY, "it %u mode %d: accepted, "
		      "packet %u has errno %d", it, mode, i, err[i]);
		CHECK((vdp[i] == RX_DUP) == (err[i] == EALREADY),
		      "it %u mode %d: packet %u verdict %d, sequential errno %d", it,
		      mode, i, vdp[i], err[i]);
		CHECK(dp[i] == ds[i], "it %u mode %d: packet %u desc %#llx, "
		      "sequential %#llx", it, mode, i, (unsigned long long)dp[i],
		      (unsigned long long)ds[i]);
		nea += err[i] == EALREADY;
	}
	CHECK(nd == nea, "it %u mode %d: %u duplicates counted, sequential %u", it,
	      mode, nd, nea);
	*ndups += nd;
	*nlates += nl;
	CHECK(tp.n == ts->n, "it %u mode %d: %u streams, sequential %u", it, mode,
	      tp.n, ts->n);
	for (k = 0; k < ts->n && k < tp.n; k++) {
		const struct rseg_rec *a = &tp.st[k], *c = &ts->st[k];
		CHECK(!memcmp(a, c, sizeof(*a)), "it %u mode %d: stream %u {%#x ix "
		      "%#x bm %#x:%#x}, sequential {%#x ix %#x bm %#x:%#x}", it,
		      mode, k, a->ssrc, a->ix, a->bhi, a->blo, c->ssrc, c->ix,
		      c->bhi, c->blo);
	}
	return 1;
}

int main(int argc, char **argv)
{
	static struct world W;
	static struct batch B;
	static struct tab ts;
	static uint64_t ds[NMAX];
	const uint32_t all = TR_NINTH | TR_DUP | TR_SWAP | TR_REPLAY | TR_WRAP |
			     TR_E63 | TR_E64 | TR_SET | TR_RTP;
	uint32_t it, nacc = 0, nrej = 0, nmust = 0, seen = 0, unsettled = 0;
	uint32_t ndups = 0, nlates = 0, nwrapped = 0, nnew = 0, nacc_trouble = 0;
	uint32_t nseam = 0;

	if (argc > 1)
		return replay_file(argv[1]);
	for (it = 0; it < 4000; it++) {
		struct geo G;
		const uint32_t pm = it % 8 < 2 ? 0 : it % 8 < 6 ? 60 : 300;
		uint32_t i, tr, n0;
		int ok;

		if (it % 4 == 0)
			seen |= make_world(&W);
		G.W = 1u << (1 + rnd() % 3);                    /* 2 .. 8 */
		G.B = G.W << (rnd() % 3);                       /* W .. 4 W */
		G.S = 1 + rnd() % 7;
		G.K = chance(500) ? RX_LOOKBACK : 2 + rnd() % 12;
		/* the sender's batch */
		memset(&B, 0, sizeof(B));
		B.n = 1 + rnd() % NRAND;
		B.encrypted = rnd() & 1u;
		B.t0 = W.t[TX];
		for (i = 0; i < B.n; i++)
			B.p[i].ssrc = ssrc_of(rnd() % W.nss);
		n0 = W.t[TX].n;
		ok = both(&B, TX, G, &ts, ds, it, &nmust, &unsettled, &ndups,
			  &nlates);
		nacc += (uint32_t)ok;
		nrej += (uint32_t)!ok;
		for (i = 0; i < ts.n && i < n0; i++)
			nwrapped += ts.st[i].ix < W.t[TX].st[i].ix;
		W.t[TX] = ts;
		/* what it put on the wire (a refused packet: its index 0) */
		for (i = 0; i < B.n; i++)
			B.p[i].word = (uint32_t)ds[i];
		tr = disturb(&W, &B, pm);
		seen |= tr;
		/* the receivers */
		B.t0 = W.t[RXH];
		n0 = B.t0.n;
		ok = both(&B, RXH, G, &ts, ds, it, &nmust, &unsettled, &ndups,
			  &nlates);
		nacc += (uint32_t)ok;
		nrej += (uint32_t)!ok;
		if (ok) {
			nacc_trouble += tr != 0;
			nnew += ts.n - n0;
			nseam += B.n > 3 * G.B;
		}
		W.t[RXH] = ts;
		B.t0 = W.t[RXG];
		ok = both(&B, RXG, G, &ts, ds, it, &nmust, &unsettled, &ndups,
			  &nlates);
		nacc += (uint32_t)ok;
		nrej += (uint32_t)!ok;
		W.t[RXG] = ts;
	}
	/* the run met what it is about */
	CHECK(nacc > 3000 && nrej > 300, "accepted %u rejected %u", nacc, nrej);
	CHECK(unsettled > 30, "rejected for a copy beyond the look-back only %u",
	      unsettled);
	CHECK(nacc_trouble > 300, "accepted disturbed batches %u", nacc_trouble);
	CHECK(ndups > 300 && nlates > 300, "duplicates %u late %u", ndups, nlates);
	CHECK(nwrapped > 10, "senders past the 31-bit wrap %u", nwrapped);
	CHECK(nnew > 100, "streams opened in accepted batches %u", nnew);
	CHECK(nseam > 300, "accepted batches over more than three workgroups %u",
	      nseam);
	CHECK((seen & all) == all, "seen %#x", seen);
	printf("%u batches: %u accepted (%u must), %u rejected (%u unsettled), "
	       "%d wrong\n", 3 * it, nacc, nmust, nrej, unsettled, g_bad);
	return g_bad ? 1 : 0;
}
