/*
 * streams_rx_check.c -- the exact receive rule composed per SSRC of ONE
 * session (re_amd/csrc/hip/plan_rx_rule.h and plan_rtp_seg_rx.h, compiled as
 * C) in the decomposition of plan_streams_rx.hip, against a sequential
 * restatement of stream_get_seq (stream.c:29-109) and of srtp_decrypt's index
 * and replay steps (srtp.c:310-321, 367, 421, 426-427; misc.c:22-41;
 * replay.c:32-62) written here.
 *
 * A world is one session whose sender uses 1-9 SSRCs, every stream starting
 * just below 65536, received in a few batches one after the other: the table
 * a batch starts from is the one the sequential receiver left.  A batch
 * interleaves the streams; per stream it carries swaps (adjacent and up to 8
 * apart), gaps, duplicates, replays of the batch before and now and then a
 * jump past 32768; the table starts with known streams, streams SRTCP created
 * (s_l not set) and room for new ones -- or not (a 9th SSRC).  Each batch runs
 *
 *   (a) as the kernels do: the stream table (known streams, then new SSRCs
 *       by first appearance), per "workgroup" of `B` packets and slot the
 *       count (`W` lanes per wave: ballots, then the waves' counts), the
 *       exclusive sums over the workgroups by a scan workgroup of `T` threads
 *       with consecutive workgroups per thread, place = start[slot] +
 *       before[workgroup][slot] + rank, then over the stream-major places the
 *       three-phase segmented (sum, max) scan (workgroup aggregates, their
 *       exclusive scan by the scan workgroup, u[] / mx[] per place),
 *       rx_settle per place with segment-local positions and look-back `K`,
 *       the records after -- small B / W / T and K = 2..13 as well as 128, so
 *       that segments and look-backs cross every boundary;
 *   (b) packet by packet through the sequential receiver.
 *
 * An accepted plan must equal (b) packet for packet (index, verdict, desc
 * flags) and record for record.  The accepted batches must be exactly those
 * with at most 8 streams in which rx_settle over each stream's arrivals, with
 * u[] and mx[] from the serial recurrence and the same K, settles every
 * packet (a first step that is an ETIMEDOUT settles nothing).
 *
 * The worlds run once with the known streams at ROC 0..2 and then with them
 * at B - 2 .. B for B = 2^16, 2^31 and 2^32, beside the streams a batch opens
 * at ROC 0.  The sequential receiver widens `int v` as misc.c:40 does, so the
 * window's top is sign-extended from ROC 2^31 on; a batch in which a stream
 * crosses 2^31 or 2^32 must be declined, every accepted one is exact.
 *
 *   streams_rx_check            the random worlds
 *   streams_rx_check FILE       a recorded traffic (lines "B", then "ssrc seq"
 *                               per arrival; the table starts empty): per
 *                               batch the sequential receiver's errno counts,
 *                               how many packets arrived out of their stream's
 *                               order, and whether (a) accepts it at the
 *                               kernels' own widths
 *
 *   gcc -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -o streams_rx_check tests/c/streams_rx_check.c && ./streams_rx_check
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../re_amd/csrc/hip/plan_rx_rule.h"
#include "../../re_amd/csrc/hip/plan_rtp_seg_rx.h"

#define NMAX 1400
#define KMAX (RSEG_MAX + 1)     /* SSRCs the session's sender may use */
#define BMAX 64                 /* "workgroup" width, at most */
#define TMAX 16                 /* scan workgroup's "threads", at most */
#define NBMAX NMAX              /* workgroups, at most (B = 1 is not used) */
#define LASTN 4                 /* seqs of the batch before kept for replays */

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

static uint32_t g_rng = 0x3b1c55a7u;

static uint32_t rnd(void)
{
	g_rng = g_rng * 1664525u + 1013904223u;
	return g_rng >> 8;
}

static int chance(uint32_t pm)
{
	return rnd() % 1000u < pm;
}

/* ---- the batch ------------------------------------------------------- */

struct tab {
	uint32_t n;
	struct tseg_rec st[RSEG_MAX];
};

struct pkt {
	uint32_t ssrc, seq;
};

struct batch {
	int hmac;
	uint32_t n;
	struct tab t0;
	struct pkt p[NMAX];
};

/* ---- (b) the sequential receiver --------------------------------------- */

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

/* misc.c:22-41: the ROC the receiver estimates */
static uint32_t ref_v(uint32_t roc, uint32_t s_l, uint32_t seq)
{
	if (s_l < 32768)
		return (int)seq - (int)s_l > 32768 ? roc - 1 : roc;
	return (int)s_l - 32768 > (int)seq ? roc + 1 : roc;
}

/* stream.c:29-109 */
static int ref_stream_get_seq(struct tab *t, uint32_t ssrc, uint32_t seq,
			      struct tseg_rec **sp)
{
	struct tseg_rec *st = NULL;
	uint32_t i;
	for (i = 0; i < t->n; i++)
		if (t->st[i].ssrc == ssrc)
			st = &t->st[i];
	if (!st) {
		if (t->n >= RSEG_MAX)
			return ENOSR;
		st = &t->st[t->n++];
		memset(st, 0, sizeof(*st));
		st->ssrc = ssrc;
	}
	if (!(st->sl & TSEG_SL_SET))
		st->sl = seq | TSEG_SL_SET;
	*sp = st;
	return 0;
}

/* per packet: errno (0, EALREADY, ETIMEDOUT, ENOSR), index, desc flags */
static void sequential(const struct batch *B, struct tab *t, int *err,
		       uint64_t *ix, uint32_t *fl)
{
	uint32_t i;
	*t = B->t0;
	for (i = 0; i < B->n; i++) {
		const struct pkt *p = &B->p[i];
		struct tseg_rec *st;
		uint64_t lix, bm, ixf;
		uint32_t s_l, v;
		int diff;
		ix[i] = 0;
		fl[i] = 0;
		err[i] = ref_stream_get_seq(t, p->ssrc, p->seq, &st);
		if (err[i])
			continue;
		s_l = st->sl & 0xffffu;
		diff = (int)p->seq - (int)s_l;
		if (diff > 32768) {                     /* srtp.c:313-316 */
			err[i] = ETIMEDOUT;
			continue;
		}
		if (diff <= -32768) {                   /* srtp.c:318-321 */
			st->roc++;
			s_l = 0;
		}
		lix = tseg_lix(*st);
		bm = tseg_bitmap(*st);
		v = ref_v(st->roc, s_l, p->seq);
		/* misc.c:40: `int v` widened -- the window holds the
		 * sign-extended index, the IV its low 48 bits */
		ixf = p->seq + (uint64_t)(int64_t)(int32_t)v * 65536ull;
		ix[i] = ixf & 0xffffffffffffull;
		fl[i] = SD_RUN | SD_CIPHER;
		if (!ref_replay_check(&lix, &bm, ixf)) {
			/* (the rollover above stays, s_l does not; the tag was
			 * checked before: HMAC suites do not decrypt it) */
			st->sl = s_l | TSEG_SL_SET;
			err[i] = EALREADY;
			if (B->hmac)
				fl[i] = SD_RUN;
			continue;
		}
		st->llo = (uint32_t)lix;
		st->lhi = (uint32_t)(lix >> 32);
		st->blo = (uint32_t)bm;
		st->bhi = (uint32_t)(bm >> 32);
		if (p->seq > s_l)                       /* srtp.c:426-427 */
			s_l = p->seq;
		st->sl = s_l | TSEG_SL_SET;
	}
}

/* ---- (a) the kernels' decomposition ------------------------------------- */

struct geo {
	uint32_t B, W, T, K;    /* workgroup, wave, scan workgroup, look-back */
};

/* inclusive segmented scan of one element per thread over a workgroup of m
 * threads: every thread reads before any thread writes (srx_block_scan) */
static void block_scan(struct rx_seg *x, uint32_t m)
{
	struct rx_seg y[BMAX];
	uint32_t t, d;
	for (d = 1; d < m; d <<= 1) {
		for (t = 0; t < m; t++)
			y[t] = t >= d ? x[t - d] : rx_seg_identity();
		for (t = 0; t < m; t++)
			x[t] = rx_seg_combine(y[t], x[t]);
	}
}

struct plan {
	struct tab t;
	uint32_t nlate, ndup;
	uint64_t ix[NMAX];
	uint32_t fl[NMAX];
	int vd[NMAX];
};

/* the slot whose segment holds place p (srx_slot_at) */
static uint32_t slot_at(const uint32_t *start, const uint32_t *cnt, uint32_t p)
{
	uint32_t q, k = RSEG_MAX;
	for (q = 0; q < RSEG_MAX; q++)
		if (p >= start[q] && p - start[q] < cnt[q])
			k = q;
	return k;
}

/* 0 accepted (P: the plan), else the SPF_* bits */
static uint32_t planned(const struct batch *Bt, struct geo G, struct plan *P)
{
	const uint32_t n = Bt->n, nb = (n + G.B - 1) / G.B;
	const uint32_t per = (nb + G.T - 1) / G.T;
	static uint8_t slot[NMAX];
	static uint32_t bcnt[RSEG_MAX][NBMAX], perm[NMAX], sseq[NMAX];
	static struct rx_seg agg[NBMAX], el[NMAX];
	static int64_t u[NMAX], mx[NMAX];
	uint32_t tabs[RSEG_MAX], nt, nk = Bt->t0.n;
	uint32_t start[RSEG_MAX], cnt[RSEG_MAX];
	uint64_t bits[RSEG_MAX];
	struct tseg_rec rec[RSEG_MAX];
	uint32_t fail = 0, b, i, q, t, p, w;

	P->t = Bt->t0;
	P->nlate = P->ndup = 0;
	/* the stream table: known streams, then new SSRCs by first appearance */
	nt = nk;
	for (q = 0; q < nk; q++)
		tabs[q] = Bt->t0.st[q].ssrc;
	for (i = 0; i < n; i++) {
		if (tsrx_known(tabs, nt, Bt->p[i].ssrc) != RSEG_NONE)
			continue;
		if (nt >= RSEG_MAX)
			return SPF_SSRC;        /* a 9th stream */
		tabs[nt++] = Bt->p[i].ssrc;
	}
	for (q = 0; q < RSEG_MAX; q++)
		rec[q] = q < nk ? Bt->t0.st[q] : tsrx_new(q < nt ? tabs[q] : 0u);
	memset(bits, 0, sizeof(bits));
	/* k_srx_count: slot per packet, counts per workgroup and slot through
	 * the waves' counts */
	for (b = 0; b < nb; b++) {
		for (q = 0; q < RSEG_MAX; q++)
			bcnt[q][b] = 0;
		for (w = 0; w * G.W < G.B; w++) {
			uint32_t wc[RSEG_MAX] = {0};
			for (t = w * G.W; t < (w + 1) * G.W && t < G.B; t++) {
				i = b * G.B + t;
				if (i >= n)
					continue;
				slot[i] = (uint8_t)tsrx_known(tabs, nt, Bt->p[i].ssrc);
				wc[slot[i]]++;
			}
			for (q = 0; q < RSEG_MAX; q++)
				bcnt[q][b] += wc[q];
		}
	}
	/* k_srx_starts: per slot, consecutive workgroups per scan thread */
	for (q = 0; q < RSEG_MAX; q++) {
		uint32_t part[TMAX], run = 0;
		for (t = 0; t < G.T; t++) {
			part[t] = 0;
			for (b = t * per; b < (t + 1) * per && b < nb; b++)
				part[t] += bcnt[q][b];
		}
		for (t = 0; t < G.T; t++) {
			const uint32_t v = part[t];
			part[t] = run;
			run += v;
		}
		cnt[q] = run;
		for (t = G.T; t-- > 0;) {
			uint32_t r = part[t];
			for (b = t * per; b < (t + 1) * per && b < nb; b++) {
				const uint32_t v = bcnt[q][b];
				bcnt[q][b] = r;
				r += v;
			}
		}
	}
	for (q = 0, p = 0; q < RSEG_MAX; q++) {
		start[q] = p;
		p += cnt[q];
	}
	/* k_srx_place: workgroups in any order, rank = the lanes below in the
	 * wave plus the waves below */
	for (b = nb; b-- > 0;) {
		uint32_t wcs[BMAX][RSEG_MAX];
		memset(wcs, 0, sizeof(wcs));
		for (t = 0; t < G.B; t++)
			if (b * G.B + t < n)
				wcs[t / G.W][slot[b * G.B + t]]++;
		for (t = G.B; t-- > 0;) {
			uint32_t rank = 0, l;
			i = b * G.B + t;
			if (i >= n)
				continue;
			q = slot[i];
			for (l = t - t % G.W; l < t; l++)
				rank += slot[b * G.B + l] == q;
			for (w = 0; w < t / G.W; w++)
				rank += wcs[w][q];
			p = start[q] + bcnt[q][b] + rank;
			perm[p] = i;
			sseq[p] = Bt->p[i].seq;
		}
	}
	/* the scan elements (srx_elem) */
	for (p = 0; p < n; p++) {
		const uint32_t k = slot_at(start, cnt, p);
		const int head = p == start[k];
		int64_t H0 = 0;
		int bad = 0;
		if (head) {
			if (!tsrx_held(rec[k]))
				fail |= SPF_ORDER;
			H0 = tsrx_h0(rec[k], sseq[p]);
		}
		el[p] = rx_seg_elem(tsrx_elem(head, H0, sseq[p],
					      head ? 0u : sseq[p - 1], &bad), head);
		if (bad)
			fail |= SPF_TIMEOUT;
	}
	if (fail)
		return fail;
	/* k_srx_agg */
	for (b = 0; b < nb; b++) {
		struct rx_seg x[BMAX];
		for (t = 0; t < G.B; t++)
			x[t] = b * G.B + t < n ? el[b * G.B + t] : rx_seg_identity();
		block_scan(x, G.B);
		agg[b] = x[G.B - 1];
	}
	/* k_srx_scan */
	{
		struct rx_seg part[BMAX];
		for (t = 0; t < G.T; t++) {
			part[t] = rx_seg_identity();
			for (b = t * per; b < (t + 1) * per && b < nb; b++)
				part[t] = rx_seg_combine(part[t], agg[b]);
		}
		block_scan(part, G.T);
		for (t = G.T; t-- > 0;) {
			struct rx_seg run = t ? part[t - 1] : rx_seg_identity();
			for (b = t * per; b < (t + 1) * per && b < nb; b++) {
				const struct rx_seg v = agg[b];
				agg[b] = run;
				run = rx_seg_combine(run, v);
			}
		}
	}
	/* k_srx_index */
	for (b = nb; b-- > 0;) {
		struct rx_seg x[BMAX];
		for (t = 0; t < G.B; t++)
			x[t] = b * G.B + t < n ? el[b * G.B + t] : rx_seg_identity();
		block_scan(x, G.B);
		for (t = 0; t < G.B; t++) {
			struct rx_seg ex;
			p = b * G.B + t;
			if (p >= n)
				continue;
			ex = rx_seg_combine(agg[b], t ? x[t - 1] : rx_seg_identity());
			mx[p] = rx_seg_mx(ex, (int)el[p].head);
			u[p] = rx_seg_combine(ex, el[p]).a.s;
		}
	}
	/* k_srx_settle */
	for (p = n; p-- > 0;) {
		const uint32_t k = slot_at(start, cnt, p);
		const uint32_t f0 = start[k], c = cnt[k];
		const struct tseg_rec st = rec[k];
		const int64_t H0 = tsrx_h0(st, sseq[f0]);
		const int64_t lix0 = (int64_t)tseg_lix(st);
		const int r = rx_settle(u + f0, mx + f0, p - f0, sseq[p], G.K, H0,
					lix0, tseg_bitmap(st), 1);
		if (r == RX_UNSETTLED) {
			fail |= SPF_ORDER;
			continue;
		}
		i = perm[p];
		P->ix[i] = d_desc_ix(d_desc((uint64_t)u[p], 0));
		P->fl[i] = tsrx_fl(r, Bt->hmac);
		P->vd[i] = r;
		if (r == RX_DUP) {
			P->ndup++;
			continue;
		}
		bits[k] |= tsrx_bit(st, tsrx_smx(u[f0 + c - 1], mx[f0 + c - 1]),
				    u[p]);
		if (tsrx_late(u[p], lix0, mx[p]))
			P->nlate++;
	}
	if (fail)
		return fail;
	/* k_srx_final, and the host's apply */
	P->t.n = nt;
	for (q = 0; q < nt; q++) {
		struct tseg_rec st = rec[q];
		if (cnt[q]) {
			const uint32_t f0 = start[q], c = cnt[q];
			st = tsrx_after(st, tsrx_h0(st, sseq[f0]),
					tsrx_smx(u[f0 + c - 1], mx[f0 + c - 1]),
					bits[q]);
		}
		P->t.st[q] = st;
	}
	return 0;
}

/* ---- the property: which batches a planner must accept ------------------ */

/* at most 8 streams (err: the sequential receiver's) and every stream's
 * arrivals, u[] and mx[] from the serial recurrence, settle under rx_settle;
 * *ooo: arrivals below an earlier one of their stream or equal to one */
static int must_accept(const struct batch *B, uint32_t K, const int *err,
		       uint32_t *ooo)
{
	static uint32_t seq[NMAX];
	static int64_t u[NMAX], mx[NMAX];
	static uint8_t seen[NMAX];
	uint32_t i, j, c;
	int ok = 1;
	memset(seen, 0, sizeof(seen));
	*ooo = 0;
	for (i = 0; i < B->n; i++)
		if (err[i] == ENOSR)
			return 0;
	for (i = 0; i < B->n; i++) {
		const struct pkt *p = &B->p[i];
		struct tseg_rec st = tsrx_new(p->ssrc);
		int64_t H0, lix0, m = RX_NEG;
		int bump = 0;
		if (seen[i])
			continue;
		for (j = 0; j < B->t0.n; j++)
			if (B->t0.st[j].ssrc == p->ssrc)
				st = B->t0.st[j];
		for (j = i, c = 0; j < B->n; j++)
			if (B->p[j].ssrc == p->ssrc) {
				seen[j] = 1;
				seq[c++] = B->p[j].seq;
			}
		H0 = tsrx_h0(st, seq[0]);
		lix0 = (int64_t)tseg_lix(st);
		if (!tsrx_held(st) || rx_step(H0, seq[0], &u[0], &bump)) {
			ok = 0;
			continue;
		}
		for (j = 0; j < c; j++) {
			if (j)
				u[j] = u[j - 1] + rx_sdiff16(seq[j], seq[j - 1]);
			mx[j] = m;
			if (u[j] <= rx_max(m, lix0))
				(*ooo)++;
			m = rx_max(m, u[j]);
		}
		for (j = 0; j < c; j++)
			if (rx_settle(u, mx, j, seq[j], K, H0, lix0,
				      tseg_bitmap(st), 1) == RX_UNSETTLED)
				ok = 0;
	}
	return ok;
}

/* ---- worlds ------------------------------------------------------------- */

struct world {
	uint32_t nss;                   /* SSRCs the session's sender uses */
	uint64_t nxt[KMAX];             /* its next extended seq */
	uint32_t last[KMAX][LASTN], nlast[KMAX];
	struct tab t;
};

static uint32_t ssrc_of(uint32_t k)
{
	return 0x57000000u | k;
}

/* what the generator did on purpose */
enum { TR_NINTH = 1, TR_DUP = 2, TR_SWAP = 4, TR_JUMP = 8, TR_REPLAY = 16,
       TR_UNSET = 32, TR_GAP = 64, TR_FAR = 128 };

/* the known streams' ROC: g_roc0 + 0..2 */
static uint32_t g_roc0;

static uint32_t make_world(struct world *W, uint32_t trouble_pm)
{
	struct tab *t = &W->t;
	uint32_t done = 0, k;
	memset(W, 0, sizeof(*W));
	W->nss = 1 + rnd() % RSEG_MAX;
	if (chance(trouble_pm / 3)) {
		W->nss = KMAX;
		done |= TR_NINTH;
	}
	t->n = rnd() % ((W->nss < RSEG_MAX ? W->nss : RSEG_MAX) + 1);
	for (k = 0; k < KMAX; k++)
		W->nxt[k] = 65300 + rnd() % 236;
	for (k = 0; k < t->n; k++) {
		struct tseg_rec *r = &t->st[k];
		uint64_t lix;
		r->ssrc = ssrc_of(k);
		if (chance(200)) {
			/* SRTCP created it: zeros, s_l not set */
			done |= TR_UNSET;
			continue;
		}
		r->roc = g_roc0 + rnd() % 3;
		W->nxt[k] += 65536ull * r->roc;
		/* the window's top as the reference leaves it (misc.c:40) */
		lix = ((W->nxt[k] - 1) & 0xffffu) +
		      (uint64_t)(int64_t)(int32_t)r->roc * 65536ull;
		r->sl = (uint32_t)(lix & 0xffffu) | TSEG_SL_SET;
		r->llo = (uint32_t)lix;
		r->lhi = (uint32_t)(lix >> 32);
		r->blo = rnd() << 8 | rnd() | 1u;
		r->bhi = rnd() << 8 | rnd();
	}
	return done;
}

static uint32_t make_batch(struct world *W, struct batch *B, uint32_t nmax,
			   uint32_t trouble_pm)
{
	static uint32_t arr[NMAX];
	uint32_t done = 0, k, i, j, c;

	memset(B, 0, sizeof(*B));
	B->hmac = (int)(rnd() & 1u);
	B->n = 1 + rnd() % nmax;
	B->t0 = W->t;
	for (i = 0; i < B->n; i++) {
		struct pkt *p = &B->p[i];
		/* now and then one long stream among short ones */
		k = chance(500) ? 0 : rnd() % W->nss;
		p->ssrc = ssrc_of(k);
		if (chance(trouble_pm / 100)) {
			W->nxt[k] += 40000;
			done |= TR_JUMP;
		}
		p->seq = (uint32_t)(W->nxt[k] & 0xffffu);
		W->nxt[k]++;
		if (chance(trouble_pm / 4)) {
			W->nxt[k] += 1 + rnd() % 3;     /* loss */
			done |= TR_GAP;
		}
	}
	/* per stream: its arrivals' places, then the trouble */
	for (k = 0; k < W->nss; k++) {
		const uint32_t x = ssrc_of(k);
		for (i = 0, c = 0; i < B->n; i++)
			if (B->p[i].ssrc == x)
				arr[c++] = i;
		for (j = 0; j < c; j++) {
			uint32_t d, w;
			if (!chance(trouble_pm / 8))
				continue;
			switch (rnd() % 4) {
			case 0:
				d = chance(600) ? 1 : 1 + rnd() % 8;
				if (j + d >= c)
					break;
				w = B->p[arr[j]].seq;
				B->p[arr[j]].seq = B->p[arr[j + d]].seq;
				B->p[arr[j + d]].seq = w;
				done |= TR_SWAP;
				break;
			case 1:
				d = 1 + rnd() % 14;
				if (j + d >= c)
					break;
				B->p[arr[j + d]].seq = B->p[arr[j]].seq;
				done |= TR_DUP;
				break;
			case 2:
				if (!W->nlast[k])
					break;
				B->p[arr[j]].seq = W->last[k][rnd() % W->nlast[k]];
				done |= TR_REPLAY;
				break;
			default:
				/* far below the window's top */
				if (chance(700))
					break;
				B->p[arr[j]].seq = (B->p[arr[j]].seq - 70 -
						    rnd() % 200) & 0xffffu;
				done |= TR_FAR;
				break;
			}
		}
		if (c) {
			W->nlast[k] = c < LASTN ? c : LASTN;
			for (j = 0; j < W->nlast[k]; j++)
				W->last[k][j] = B->p[arr[c - 1 - j]].seq;
		}
	}
	return done;
}

/* ---- a recorded traffic -------------------------------------------------- */

static struct batch g_B;
static struct plan g_P;
static struct tab g_ts;
static int g_err[NMAX];
static uint64_t g_ixs[NMAX];
static uint32_t g_fls[NMAX];

static int replay_file(const char *path)
{
	/* the kernels' workgroup is wider than BMAX; the scan is associative,
	 * so the widest this program has stands in for it */
	const struct geo G = {.B = BMAX, .W = BMAX, .T = TMAX, .K = RX_LOOKBACK};
	FILE *f = fopen(path, "r");
	char line[128];
	uint32_t nbatch = 0;
	int more = 1;
	if (!f) {
		perror(path);
		return 2;
	}
	memset(&g_B, 0, sizeof(g_B));
	g_B.hmac = 1;
	while (more) {
		unsigned x, q;
		more = fgets(line, sizeof(line), f) != NULL;
		if (more && line[0] != 'B' && sscanf(line, "%x %u", &x, &q) == 2) {
			if (g_B.n >= NMAX) {
				printf("batch %u: out of range\n", nbatch);
				fclose(f);
				return 2;
			}
			g_B.p[g_B.n].ssrc = x;
			g_B.p[g_B.n].seq = q & 0xffffu;
			g_B.n++;
			continue;
		}
		if (g_B.n) {
			uint32_t i, ne[4] = {0, 0, 0, 0}, fail, ooo;
			int must;
			sequential(&g_B, &g_ts, g_err, g_ixs, g_fls);
			fail = planned(&g_B, G, &g_P);
			must = must_accept(&g_B, G.K, g_err, &ooo);
			for (i = 0; i < g_B.n; i++)
				ne[g_err[i] == 0 ? 0 : g_err[i] == EALREADY ? 1 :
				   g_err[i] == ETIMEDOUT ? 2 : 3]++;
			printf("batch %u: %u packets ok %u already %u timedout %u "
			       "other %u disturbed %u streams %u plan %s must %d\n",
			       nbatch, g_B.n, ne[0], ne[1], ne[2], ne[3], ooo,
			       g_ts.n, fail ? "rejected" : "accepted", must);
			g_B.t0 = g_ts;
			g_B.n = 0;
			nbatch++;
		}
	}
	fclose(f);
	return 0;
}

/* what a run of random batches met */
struct tally {
	uint32_t naccept, nreject, nmust, seen, nroll, ndups, nlates, nlong;
	uint32_t nacc_trouble, nnew, nshortk, ncross;
};

/* nit batches from worlds whose known streams start at g_roc0 + 0..2 */
static void random_batches(struct world *W, uint32_t nit, struct tally *Y)
{
	uint32_t it;
	memset(Y, 0, sizeof(*Y));
	for (it = 0; it < nit; it++) {
		struct geo G;
		const uint32_t pm = it % 8 < 2 ? 0 : it % 8 < 6 ? 60 : 300;
		uint32_t tr, fail, i, k, nea = 0, ooo, cross = 0;
		int must;

		if (it % 4 == 0)
			Y->seen |= make_world(W, pm);
		G.W = 1u << (1 + rnd() % 3);            /* 2 .. 8 */
		G.B = G.W << (rnd() % 4);               /* .. 64, a power of two */
		G.T = 1u << (rnd() % 5);                /* 1 .. 16 */
		G.K = chance(500) ? RX_LOOKBACK : 2 + rnd() % 12;
		tr = make_batch(W, &g_B, chance(800) ? 400 : 40, pm);
		sequential(&g_B, &g_ts, g_err, g_ixs, g_fls);
		memset(&g_P, 0, sizeof(g_P));
		fail = planned(&g_B, G, &g_P);
		must = must_accept(&g_B, G.K, g_err, &ooo);
		Y->nmust += (uint32_t)must;
		Y->seen |= tr;
		CHECK(!(must && fail), "roc %#x it %u: rejected (SPF %#x) a batch it "
		      "must accept", g_roc0, it, fail);
		CHECK(must || fail, "roc %#x it %u: accepted a batch the sequential "
		      "rx_settle does not settle", g_roc0, it);
		/* a stream the receiver took across ROC 2^31 or 2^32: its index
		 * is sign-extended from there on, the planner must decline */
		for (k = 0; k < g_B.t0.n; k++) {
			const uint32_t r0 = g_B.t0.st[k].roc, r1 = g_ts.st[k].roc;
			cross |= (!(r0 >> 31) && (r1 >> 31)) || r1 < r0;
		}
		Y->ncross += cross;
		CHECK(!cross || fail, "roc %#x it %u: accepted a batch that crosses "
		      "2^31 or 2^32", g_roc0, it);
		/* the next batch starts from what the receiver holds */
		W->t = g_ts;
		if (fail) {
			Y->nreject++;
			continue;
		}
		Y->naccept++;
		Y->nacc_trouble += (tr & (TR_DUP | TR_SWAP | TR_REPLAY)) != 0;
		Y->nshortk += G.K < 14 && ooo;
		for (i = 0; i < g_B.n; i++) {
			CHECK(g_err[i] == 0 || g_err[i] == EALREADY, "it %u: "
			      "accepted, packet %u has errno %d", it, i, g_err[i]);
			CHECK((g_P.vd[i] == RX_DUP) == (g_err[i] == EALREADY),
			      "it %u: packet %u verdict %d, sequential errno %d",
			      it, i, g_P.vd[i], g_err[i]);
			CHECK(g_P.ix[i] == g_ixs[i] && g_P.fl[i] == g_fls[i],
			      "it %u: packet %u index %#llx flags %#x, sequential "
			      "%#llx %#x", it, i, (unsigned long long)g_P.ix[i],
			      g_P.fl[i], (unsigned long long)g_ixs[i], g_fls[i]);
			nea += g_err[i] == EALREADY;
		}
		CHECK(g_P.ndup == nea, "it %u: %u duplicates counted, sequential "
		      "%u", it, g_P.ndup, nea);
		Y->ndups += g_P.ndup;
		Y->nlates += g_P.nlate;
		CHECK(g_P.t.n == g_ts.n, "it %u: %u streams, sequential %u", it,
		      g_P.t.n, g_ts.n);
		Y->nnew += g_ts.n - g_B.t0.n;
		for (k = 0; k < g_ts.n && k < g_P.t.n; k++) {
			const struct tseg_rec *a = &g_P.t.st[k];
			const struct tseg_rec *c = &g_ts.st[k];
			uint32_t per = 0;
			CHECK(!memcmp(a, c, sizeof(*a)),
			      "it %u: stream %u {%#x roc %u sl %#x lix %#x:%#x bm "
			      "%#x:%#x}, sequential {%#x roc %u sl %#x lix %#x:%#x "
			      "bm %#x:%#x}", it, k, a->ssrc, a->roc, a->sl, a->lhi,
			      a->llo, a->bhi, a->blo, c->ssrc, c->roc, c->sl,
			      c->lhi, c->llo, c->bhi, c->blo);
			if (k < g_B.t0.n && c->roc != g_B.t0.st[k].roc)
				Y->nroll++;
			for (i = 0; i < g_B.n; i++)
				per += g_B.p[i].ssrc == c->ssrc;
			Y->nlong += per > 2 * G.B;
		}
	}
}

int main(int argc, char **argv)
{
	static struct world W;
	static const uint32_t BASE[3] = {0xfffeu, 0x7ffffffeu, 0xfffffffeu};
	const uint32_t all = TR_NINTH | TR_DUP | TR_SWAP | TR_JUMP | TR_REPLAY |
			     TR_UNSET | TR_GAP | TR_FAR;
	struct tally Y, Z;
	uint32_t b;

	if (argc > 1)
		return replay_file(argv[1]);
	random_batches(&W, 6000, &Y);
	/* the run met what it is about */
	CHECK(Y.naccept > 1500 && Y.nreject > 300, "accepted %u rejected %u",
	      Y.naccept, Y.nreject);
	CHECK(Y.nacc_trouble > 300, "accepted batches with swaps, duplicates or "
	      "replays %u", Y.nacc_trouble);
	CHECK(Y.nshortk > 100, "accepted disturbed batches under a short look-back "
	      "%u", Y.nshortk);
	CHECK(Y.ndups > 300 && Y.nlates > 300, "duplicates %u late %u", Y.ndups,
	      Y.nlates);
	CHECK(Y.nroll > 300, "rollovers inside accepted batches %u", Y.nroll);
	CHECK(Y.nnew > 300, "streams opened in accepted batches %u", Y.nnew);
	CHECK(Y.nlong > 300, "streams longer than two workgroups %u", Y.nlong);
	CHECK((Y.seen & all) == all, "seen %#x", Y.seen);
	CHECK(Y.ncross == 0, "%u batches crossed 2^31 from ROC 0..3", Y.ncross);
	/* the same traffic with the known streams at B - 2 .. B for B = 2^16,
	 * 2^31 and 2^32, beside the streams the batches open at ROC 0.  2^16 is
	 * an ordinary rollover: the shares of the run above hold (a quarter
	 * of the batches accepted, a twentieth with a rollover inside).  At
	 * the others some batches cross (and are declined, checked above) and
	 * some stay below or open new streams only (accepted, exactly) */
	for (b = 0; b < 3; b++) {
		g_roc0 = BASE[b];
		random_batches(&W, 1500, &Z);
		if (!b)
			CHECK(Z.naccept > 375 && Z.nroll > 75 && !Z.ncross,
			      "roc %#x: accepted %u rollovers %u crossed %u", g_roc0,
			      Z.naccept, Z.nroll, Z.ncross);
		else
			CHECK(Z.naccept && Z.ncross, "roc %#x: accepted %u crossed "
			      "%u", g_roc0, Z.naccept, Z.ncross);
		printf("roc %#x: 1500 batches, %u taken, %u declined, %u crossed\n",
		       g_roc0, Z.naccept, Z.nreject, Z.ncross);
	}
	printf("%u batches: %u accepted (%u must), %u rejected, %d wrong\n", 6000u,
	       Y.naccept, Y.nmust, Y.nreject, g_bad);
	return g_bad ? 1 : 0;
}
