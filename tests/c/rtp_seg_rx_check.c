/*
 * rtp_seg_rx_check.c -- the exact receive rule composed per (session, SSRC)
 * (re_amd/csrc/hip/plan_rtp_seg_rx.h, compiled as C) in the decomposition of
 * k_bsr_plan (plan_buckets_rtp_streams_rx.hip), against a sequential
 * restatement of stream_get_seq (stream.c:29-109) and of srtp_decrypt's
 * index and replay steps (srtp.c:310-321, 367, 421, 426-427; misc.c:22-41;
 * replay.c:32-62) written here.
 *
 * A world is 2-40 sessions whose senders use 1-9 SSRCs each, every stream
 * starting just below 65536, received in a few batches one after the other:
 * the tables a batch starts from are the ones the sequential receiver left.
 * A batch interleaves the streams; per stream it carries swaps (adjacent and
 * up to 8 apart), gaps, duplicates, replays of the batch before and now and
 * then a jump past 32768; tables start with known streams, streams SRTCP
 * created (s_l not set) and room for new ones -- or not (a 9th SSRC).  Each
 * batch runs
 *
 *   (a) as the kernel does: sessions cut into buckets of 2^bshift ids, a
 *       bucket's entries in an arbitrary order (the scatter's atomics),
 *       grouped by session, ranked by packet index, the look back for slot
 *       and rank, the streams of a session one behind the other, then the
 *       segmented (sum, max) scan with `ept` consecutive positions per
 *       "thread", `W` threads per "wave" (shuffles) and the waves' aggregates,
 *       rx_settle per packet, the tables after -- small bshift / segmax / T /
 *       W / ept so that segments cross every boundary;
 *   (b) packet by packet through the sequential receiver.
 *
 * An accepted plan must equal (b) packet for packet (index, verdict, desc
 * flags) and record for record.  The accepted batches must be exactly those
 * in which no slot overflows, the buckets hold the batch, and rx_settle over
 * each stream's arrivals, with u[] and mx[] from the serial recurrence,
 * settles every packet (a first step that is an ETIMEDOUT settles nothing).
 *
 * The worlds run once with the known streams at ROC 0..2 and then with about
 * a third of them at B - 2 .. B for B = 2^16, 2^31 and 2^32 between the
 * others.  The sequential receiver widens `int v` as misc.c:40 does, so the
 * window's top is sign-extended from ROC 2^31 on; a batch in which a stream
 * crosses 2^31 or 2^32 must be declined, every accepted one is exact.
 *
 *   rtp_seg_rx_check            the random worlds
 *   rtp_seg_rx_check FILE       a recorded traffic (lines "B", then "session
 *                               ssrc seq" per arrival; tables start empty):
 *                               per batch the sequential receiver's errno
 *                               counts and whether (a) accepts it at the
 *                               kernel's own widths
 *
 *   gcc -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -o rtp_seg_rx_check tests/c/rtp_seg_rx_check.c && ./rtp_seg_rx_check
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../re_amd/csrc/hip/plan_rtp_seg_rx.h"

#define NMAX 600
#define SMAX 40
#define KMAX (RSEG_MAX + 1)     /* SSRCs a session's sender may use */
#define TMAX 64                 /* "threads" */
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

static uint32_t g_rng = 0x2c9277b5u;

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
	uint32_t sess, ssrc, seq;
};

struct batch {
	int hmac;
	uint32_t nsess, n;
	struct tab t0[SMAX];
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
	memcpy(t, B->t0, sizeof(B->t0));
	for (i = 0; i < B->n; i++) {
		const struct pkt *p = &B->p[i];
		struct tseg_rec *st;
		uint64_t lix, bm, ixf;
		uint32_t s_l, v;
		int diff;
		ix[i] = 0;
		fl[i] = 0;
		err[i] = ref_stream_get_seq(&t[p->sess], p->ssrc, p->seq, &st);
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

/* ---- (a) the kernel's decomposition ----------------------------------- */

struct geo {
	uint32_t bshift, segmax, T, W, ept;     /* cap = T * ept */
};

/* the workgroup's exclusive segmented scan of one aggregate per thread:
 * inside a wave by shuffles (every lane reads before any lane writes),
 * across the waves through their aggregates */
static void excl_scan(const struct rx_seg *agg, struct geo G,
		      struct rx_seg *run)
{
	struct rx_seg x[TMAX], y[TMAX], wagg[TMAX];
	uint32_t t, d, q;
	memcpy(x, agg, G.T * sizeof(*x));
	for (d = 1; d < G.W; d <<= 1) {
		for (t = 0; t < G.T; t++)
			y[t] = t % G.W >= d ? x[t - d] : x[t];
		for (t = 0; t < G.T; t++)
			if (t % G.W >= d)
				x[t] = rx_seg_combine(y[t], x[t]);
	}
	for (t = 0; t < G.T; t++)
		if (t % G.W == G.W - 1)
			wagg[t / G.W] = x[t];
	for (t = 0; t < G.T; t++) {
		const struct rx_seg below = t % G.W ? x[t - 1] : rx_seg_identity();
		struct rx_seg pre = rx_seg_identity();
		for (q = 0; q < t / G.W; q++)
			pre = rx_seg_combine(pre, wagg[q]);
		run[t] = rx_seg_combine(pre, below);
	}
}

/* 0 accepted (ix[], fl[], vd[], t[]: the plan), else the SPF_* bits */
static uint32_t planned(const struct batch *B, struct geo G, struct tab *t,
			uint64_t *ix, uint32_t *fl, int *vd, uint32_t *nlate,
			uint32_t *ndup)
{
	const uint32_t nsb = 1u << G.bshift, cap = G.T * G.ept;
	const uint32_t nb = (B->nsess + nsb - 1) >> G.bshift;
	uint32_t fail = 0, b, i;

	memcpy(t, B->t0, sizeof(B->t0));
	*nlate = *ndup = 0;
	for (b = 0; b < nb; b++) {
		const uint32_t s0 = b << G.bshift;
		const uint32_t ns = B->nsess - s0 < nsb ? B->nsess - s0 : nsb;
		static uint32_t ent[NMAX], gidx[NMAX], idx[NMAX], ru[NMAX];
		static uint32_t kn[NMAX], sl[NMAX], rank[NMAX], firstk[NMAX];
		static uint8_t opens[NMAX];
		static uint32_t pi[NMAX], pq[NMAX], ps[NMAX];
		static int64_t u[NMAX], mx[NMAX], dv[NMAX];
		static uint8_t hd[NMAX];
		uint32_t cnt[SMAX], start[SMAX], nk[SMAX], nst[SMAX];
		uint32_t tmask[SMAX], acc[SMAX][RSEG_MAX], tss[SMAX][RSEG_MAX];
		uint32_t first[SMAX][RSEG_MAX];
		uint64_t bits[SMAX][RSEG_MAX];
		struct rx_seg agg[TMAX], run[TMAX];
		uint32_t m = 0, f = 0, k, l, x, tid, j, p;

		for (i = 0; i < B->n; i++)
			if (B->p[i].sess >> G.bshift == b)
				ent[m++] = i;
		for (k = m; k > 1; k--) {
			const uint32_t q = rnd() % k, w = ent[q];
			ent[q] = ent[k - 1];
			ent[k - 1] = w;
		}
		if (m > cap) {
			fail |= SPF_SEG;
			continue;
		}
		memset(acc, 0, sizeof(acc));
		memset(bits, 0, sizeof(bits));
		memset(tss, 0, sizeof(tss));
		for (l = 0; l < ns; l++) {
			nk[l] = nst[l] = B->t0[s0 + l].n;
			cnt[l] = tmask[l] = 0;
			for (x = 0; x < nk[l]; x++)
				tss[l][x] = B->t0[s0 + l].st[x].ssrc;
		}
#define REC(l, x) ((x) < nk[l] ? B->t0[s0 + (l)].st[x] : tsrx_new(tss[l][x]))
		for (k = 0; k < m; k++)
			ru[k] = cnt[B->p[ent[k]].sess - s0]++;
		for (l = 0, k = 0; l < ns; l++) {
			start[l] = k;
			k += cnt[l];
			if (cnt[l] > G.segmax)
				f |= SPF_SEG;
		}
		if (f) {
			fail |= f;
			continue;
		}
		for (k = 0; k < m; k++)
			gidx[start[B->p[ent[k]].sess - s0] + ru[k]] = ent[k];
		for (k = 0; k < m; k++) {
			uint32_t r = 0, q;
			l = B->p[ent[k]].sess - s0;
			for (q = start[l]; q < start[l] + cnt[l]; q++)
				r += gidx[q] < ent[k];
			idx[start[l] + r] = ent[k];
		}
#define EACH_POSITION                                                        \
	for (tid = G.T; tid-- > 0;)                                          \
		for (k = tid; k < m; k += G.T)
		/* pass 1: the known slot, the look back */
		EACH_POSITION {
			const struct pkt *q = &B->p[idx[k]];
			struct rseg_look lk = rseg_look_init(k);
			uint32_t w;
			l = q->sess - s0;
			kn[k] = tsrx_known(tss[l], nk[l], q->ssrc);
			for (w = start[l]; w < k; w++)
				lk = rseg_look_step(lk, w,
						    B->p[idx[w]].ssrc == q->ssrc);
			opens[k] = (uint8_t)rseg_opens(kn[k], lk);
			rank[k] = lk.rank;
			firstk[k] = lk.first;
		}
		/* pass 2: the slot, new SSRCs, the streams' arrivals */
		EACH_POSITION {
			const struct pkt *q = &B->p[idx[k]];
			uint32_t nnew = 0, slot, w;
			l = q->sess - s0;
			sl[k] = RSEG_NONE;
			if (kn[k] == RSEG_NONE)
				for (w = start[l]; w < firstk[k]; w++)
					nnew += opens[w];
			slot = rseg_slot(kn[k], nk[l], nnew);
			if (rseg_enosr(slot)) {
				f |= SPF_SSRC;
				continue;
			}
			sl[k] = slot;
			if (opens[k]) {
				tss[l][slot] = q->ssrc;
				if (nst[l] < slot + 1)
					nst[l] = slot + 1;
			}
			tmask[l] |= 1u << slot;
			if (acc[l][slot] < rank[k] + 1)
				acc[l][slot] = rank[k] + 1;
		}
		if (f) {
			fail |= f;
			continue;
		}
		/* a session's streams one behind the other */
		for (l = 0; l < ns; l++)
			for (x = 0; x < RSEG_MAX; x++)
				first[l][x] = tsrx_first(start[l], acc[l], x);
		EACH_POSITION {
			l = B->p[idx[k]].sess - s0;
			p = first[l][sl[k]] + rank[k];
			pi[p] = idx[k];
			pq[p] = B->p[idx[k]].seq;
			ps[p] = l << 3 | sl[k];
		}
		/* the scan: ept consecutive positions per thread */
		for (tid = 0; tid < G.T; tid++) {
			agg[tid] = rx_seg_identity();
			for (j = 0; j < G.ept; j++) {
				int64_t H0 = 0;
				int bad = 0;
				p = tid * G.ept + j;
				if (p >= m)
					continue;
				l = ps[p] >> 3;
				x = ps[p] & 7u;
				hd[p] = p == first[l][x];
				if (hd[p]) {
					const struct tseg_rec st = REC(l, x);
					if (!tsrx_held(st))
						f |= SPF_ORDER;
					H0 = tsrx_h0(st, pq[p]);
				}
				dv[p] = tsrx_elem(hd[p], H0, pq[p],
						  hd[p] ? 0u : pq[p - 1], &bad);
				if (bad)
					f |= SPF_TIMEOUT;
				agg[tid] = rx_seg_combine(agg[tid],
							  rx_seg_elem(dv[p], hd[p]));
			}
		}
		excl_scan(agg, G, run);
		for (tid = G.T; tid-- > 0;)
			for (j = 0; j < G.ept; j++) {
				p = tid * G.ept + j;
				if (p >= m)
					continue;
				mx[p] = rx_seg_mx(run[tid], hd[p]);
				run[tid] = rx_seg_combine(run[tid],
							  rx_seg_elem(dv[p], hd[p]));
				u[p] = run[tid].a.s;
			}
		if (f) {
			fail |= f;
			continue;
		}
		/* per packet: rx_settle with positions local to its stream */
		for (tid = G.T; tid-- > 0;)
			for (p = tid; p < m; p += G.T) {
				struct tseg_rec st;
				uint32_t f0;
				int64_t H0, lix0, smx;
				int r;
				l = ps[p] >> 3;
				x = ps[p] & 7u;
				f0 = first[l][x];
				st = REC(l, x);
				H0 = tsrx_h0(st, pq[f0]);
				lix0 = (int64_t)tseg_lix(st);
				r = rx_settle(u + f0, mx + f0, p - f0, pq[p],
					      RX_LOOKBACK, H0, lix0, tseg_bitmap(st),
					      1);
				if (r == RX_UNSETTLED) {
					f |= SPF_ORDER;
					continue;
				}
				ix[pi[p]] = d_desc_ix(d_desc((uint64_t)u[p], 0));
				fl[pi[p]] = tsrx_fl(r, B->hmac);
				vd[pi[p]] = r;
				if (r == RX_DUP) {
					(*ndup)++;
					continue;
				}
				smx = tsrx_smx(u[f0 + acc[l][x] - 1],
					       mx[f0 + acc[l][x] - 1]);
				bits[l][x] |= tsrx_bit(st, smx, u[p]);
				if (tsrx_late(u[p], lix0, mx[p]))
					(*nlate)++;
			}
		if (f) {
			fail |= f;
			continue;
		}
		/* the touched sessions' tables after the batch */
		for (l = 0; l < ns; l++) {
			if (!tmask[l])
				continue;
			t[s0 + l].n = nst[l];
			for (x = 0; x < nst[l]; x++) {
				struct tseg_rec st = REC(l, x);
				if (tmask[l] >> x & 1u) {
					const uint32_t f0 = first[l][x];
					st = tsrx_after(st, tsrx_h0(st, pq[f0]),
						tsrx_smx(u[f0 + acc[l][x] - 1],
							 mx[f0 + acc[l][x] - 1]),
						bits[l][x]);
				}
				t[s0 + l].st[x] = st;
			}
		}
#undef EACH_POSITION
#undef REC
	}
	return fail;
}

/* ---- the property: which batches a planner must accept ------------------ */

/* every stream's arrivals, u[] and mx[] from the serial recurrence, settle
 * under rx_settle; no slot overflows (err: the sequential receiver's); the
 * buckets hold the batch */
static int must_accept(const struct batch *B, struct geo G, const int *err)
{
	const uint32_t nb = (B->nsess + (1u << G.bshift) - 1) >> G.bshift;
	static uint32_t inb[SMAX], ins[SMAX], seq[NMAX];
	static int64_t u[NMAX], mx[NMAX];
	static uint8_t seen[NMAX];
	uint32_t i, j, c;
	memset(inb, 0, sizeof(inb));
	memset(ins, 0, sizeof(ins));
	memset(seen, 0, sizeof(seen));
	for (i = 0; i < B->n; i++) {
		if (err[i] == ENOSR)
			return 0;
		inb[B->p[i].sess >> G.bshift]++;
		ins[B->p[i].sess]++;
	}
	for (i = 0; i < nb; i++)
		if (inb[i] > G.T * G.ept)
			return 0;
	for (i = 0; i < B->nsess; i++)
		if (ins[i] > G.segmax)
			return 0;
	for (i = 0; i < B->n; i++) {
		const struct pkt *p = &B->p[i];
		const struct tab *t = &B->t0[p->sess];
		struct tseg_rec st = tsrx_new(p->ssrc);
		int64_t H0, lix0, m = RX_NEG;
		int bump = 0;
		if (seen[i])
			continue;
		for (j = 0; j < t->n; j++)
			if (t->st[j].ssrc == p->ssrc)
				st = t->st[j];
		for (j = i, c = 0; j < B->n; j++)
			if (B->p[j].sess == p->sess && B->p[j].ssrc == p->ssrc) {
				seen[j] = 1;
				seq[c++] = B->p[j].seq;
			}
		H0 = tsrx_h0(st, seq[0]);
		lix0 = (int64_t)tseg_lix(st);
		if (!tsrx_held(st) || rx_step(H0, seq[0], &u[0], &bump))
			return 0;
		for (j = 0; j < c; j++) {
			if (j)
				u[j] = u[j - 1] + rx_sdiff16(seq[j], seq[j - 1]);
			mx[j] = m;
			m = rx_max(m, u[j]);
		}
		for (j = 0; j < c; j++)
			if (rx_settle(u, mx, j, seq[j], RX_LOOKBACK, H0, lix0,
				      tseg_bitmap(st), 1) == RX_UNSETTLED)
				return 0;
	}
	return 1;
}

/* ---- worlds ------------------------------------------------------------- */

struct world {
	uint32_t nsess;
	uint32_t nss[SMAX];             /* SSRCs the session's sender uses */
	uint64_t nxt[SMAX][KMAX];       /* its next extended seq */
	uint32_t last[SMAX][KMAX][LASTN], nlast[SMAX][KMAX];
	struct tab t[SMAX];
};

static uint32_t ssrc_of(uint32_t s, uint32_t k)
{
	return 0x54000000u | s << 8 | k;
}

/* what the generator did on purpose */
enum { TR_NINTH = 1, TR_DUP = 2, TR_SWAP = 4, TR_JUMP = 8, TR_REPLAY = 16,
       TR_UNSET = 32, TR_GAP = 64, TR_FAR = 128 };

/* not 0: about a third of the known streams are at ROC g_roc0 + 0..2, the
 * others beside them at 0..2 as ever */
static uint32_t g_roc0;

static uint32_t make_world(struct world *W, uint32_t trouble_pm)
{
	uint32_t done = 0, s, k;
	memset(W, 0, sizeof(*W));
	W->nsess = chance(300) ? 2 + rnd() % 3 : 2 + rnd() % (SMAX - 1);
	for (s = 0; s < W->nsess; s++) {
		struct tab *t = &W->t[s];
		W->nss[s] = 1 + rnd() % RSEG_MAX;
		if (chance(trouble_pm / 6)) {
			W->nss[s] = KMAX;
			done |= TR_NINTH;
		}
		t->n = rnd() % ((W->nss[s] < RSEG_MAX ? W->nss[s] : RSEG_MAX) + 1);
		for (k = 0; k < KMAX; k++)
			W->nxt[s][k] = 65300 + rnd() % 236;
		for (k = 0; k < t->n; k++) {
			struct tseg_rec *r = &t->st[k];
			uint64_t lix;
			r->ssrc = ssrc_of(s, k);
			if (chance(200)) {
				/* SRTCP created it: zeros, s_l not set */
				done |= TR_UNSET;
				continue;
			}
			r->roc = rnd() % 3;
			if (g_roc0 && chance(300))
				r->roc += g_roc0;
			W->nxt[s][k] += 65536ull * r->roc;
			/* the window's top as the reference leaves it
			 * (misc.c:40) */
			lix = ((W->nxt[s][k] - 1) & 0xffffu) +
			      (uint64_t)(int64_t)(int32_t)r->roc * 65536ull;
			r->sl = (uint32_t)(lix & 0xffffu) | TSEG_SL_SET;
			r->llo = (uint32_t)lix;
			r->lhi = (uint32_t)(lix >> 32);
			r->blo = rnd() << 8 | rnd() | 1u;
			r->bhi = rnd() << 8 | rnd();
		}
	}
	return done;
}

static uint32_t make_batch(struct world *W, struct batch *B, uint32_t trouble_pm)
{
	static uint32_t arr[NMAX];
	uint32_t done = 0, s, k, i, j, c;

	memset(B, 0, sizeof(*B));
	B->hmac = (int)(rnd() & 1u);
	B->nsess = W->nsess;
	B->n = 1 + rnd() % NMAX;
	memcpy(B->t0, W->t, sizeof(B->t0));
	for (i = 0; i < B->n; i++) {
		struct pkt *p = &B->p[i];
		s = rnd() % W->nsess;
		k = rnd() % W->nss[s];
		p->sess = s;
		p->ssrc = ssrc_of(s, k);
		if (chance(trouble_pm / 100)) {
			W->nxt[s][k] += 40000;
			done |= TR_JUMP;
		}
		p->seq = (uint32_t)(W->nxt[s][k] & 0xffffu);
		W->nxt[s][k]++;
		if (chance(trouble_pm / 4)) {
			W->nxt[s][k] += 1 + rnd() % 3;  /* loss */
			done |= TR_GAP;
		}
	}
	/* per stream: its arrivals' places, then the trouble */
	for (s = 0; s < W->nsess; s++)
		for (k = 0; k < W->nss[s]; k++) {
			const uint32_t x = ssrc_of(s, k);
			for (i = 0, c = 0; i < B->n; i++)
				if (B->p[i].sess == s && B->p[i].ssrc == x)
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
					d = 1 + rnd() % 5;
					if (j + d >= c)
						break;
					B->p[arr[j + d]].seq = B->p[arr[j]].seq;
					done |= TR_DUP;
					break;
				case 2:
					if (!W->nlast[s][k])
						break;
					B->p[arr[j]].seq =
						W->last[s][k][rnd() % W->nlast[s][k]];
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
				W->nlast[s][k] = c < LASTN ? c : LASTN;
				for (j = 0; j < W->nlast[s][k]; j++)
					W->last[s][k][j] = B->p[arr[c - 1 - j]].seq;
			}
		}
	return done;
}

/* ---- a recorded traffic -------------------------------------------------- */

static int replay_file(const char *path)
{
	static struct batch B;
	static struct tab ts[SMAX], tp[SMAX];
	static int err[NMAX], vdp[NMAX];
	static uint64_t ixs[NMAX], ixp[NMAX];
	static uint32_t fls[NMAX], flp[NMAX];
	const struct geo G = {.bshift = 4, .segmax = NMAX, .T = 64, .W = 64,
			      .ept = (NMAX + 63) / 64};
	FILE *f = fopen(path, "r");
	char line[128];
	uint32_t nbatch = 0;
	int more = 1;
	if (!f) {
		perror(path);
		return 2;
	}
	memset(&B, 0, sizeof(B));
	B.hmac = 1;
	while (more) {
		unsigned s, x, q;
		more = fgets(line, sizeof(line), f) != NULL;
		if (more && sscanf(line, "%u %x %u", &s, &x, &q) == 3 &&
		    line[0] != 'B') {
			if (s >= SMAX || B.n >= NMAX) {
				printf("batch %u: out of range\n", nbatch);
				fclose(f);
				return 2;
			}
			if (B.nsess < s + 1)
				B.nsess = s + 1;
			B.p[B.n].sess = s;
			B.p[B.n].ssrc = x;
			B.p[B.n].seq = q & 0xffffu;
			B.n++;
			continue;
		}
		if (B.n) {
			uint32_t i, ne[4] = {0, 0, 0, 0}, fail, nl, nd;
			if (B.nsess < 2)
				B.nsess = 2;
			sequential(&B, ts, err, ixs, fls);
			fail = planned(&B, G, tp, ixp, flp, vdp, &nl, &nd);
			for (i = 0; i < B.n; i++)
				ne[err[i] == 0 ? 0 : err[i] == EALREADY ? 1 :
				   err[i] == ETIMEDOUT ? 2 : 3]++;
			printf("batch %u: %u packets ok %u already %u timedout %u "
			       "other %u plan %s must %d\n", nbatch, B.n, ne[0],
			       ne[1], ne[2], ne[3], fail ? "rejected" : "accepted",
			       must_accept(&B, G, err));
			memcpy(B.t0, ts, sizeof(B.t0));
			B.n = 0;
			nbatch++;
		}
	}
	fclose(f);
	return 0;
}

/* what a run of random worlds met */
struct tally {
	uint32_t naccept, nreject, nmust, seen, nroll, ndups, nlates, nlong;
	uint32_t nacc_trouble, nnew, ncross;
};

static void random_worlds(struct world *W, uint32_t nit, struct tally *Y)
{
	static struct batch B;
	static struct tab ts[SMAX], tp[SMAX];
	static int err[NMAX], vdp[NMAX];
	static uint64_t ixs[NMAX], ixp[NMAX];
	static uint32_t fls[NMAX], flp[NMAX];
	uint32_t it;
	memset(Y, 0, sizeof(*Y));
	for (it = 0; it < nit; it++) {
		struct geo G;
		const uint32_t pm = it % 8 < 2 ? 0 : it % 8 < 6 ? 60 : 300;
		uint32_t tr, fail, i, s, k, nl = 0, nd = 0, nea = 0, cross = 0;
		int must;

		if (it % 4 == 0)
			Y->seen |= make_world(W, pm);
		G.bshift = rnd() % 4;
		G.segmax = chance(850) ? NMAX : 8 + rnd() % 64;
		G.W = 1u << (1 + rnd() % 4);            /* 2 .. 16 */
		G.T = G.W * (1 + rnd() % (TMAX / G.W));
		G.ept = 1 + rnd() % 4;
		if (chance(850))                        /* cap >= the batch */
			G.ept = (NMAX + G.T - 1) / G.T;
		tr = make_batch(W, &B, pm);
		sequential(&B, ts, err, ixs, fls);
		memset(ixp, 0, sizeof(ixp));
		memset(flp, 0, sizeof(flp));
		memset(vdp, 0, sizeof(vdp));
		fail = planned(&B, G, tp, ixp, flp, vdp, &nl, &nd);
		must = must_accept(&B, G, err);
		Y->nmust += (uint32_t)must;
		Y->seen |= tr;
		CHECK(!(must && fail), "it %u: rejected (SPF %#x) a batch it must "
		      "accept", it, fail);
		CHECK(must || fail, "it %u: accepted a batch the sequential "
		      "rx_settle does not settle", it);
		/* a stream the receiver took across ROC 2^31 or 2^32: its index
		 * is sign-extended from there on, the planner must decline */
		for (s = 0; s < B.nsess; s++)
			for (k = 0; k < B.t0[s].n; k++) {
				const uint32_t r0 = B.t0[s].st[k].roc;
				const uint32_t r1 = ts[s].st[k].roc;
				cross |= (!(r0 >> 31) && (r1 >> 31)) || r1 < r0;
			}
		Y->ncross += cross;
		CHECK(!cross || fail, "roc %#x it %u: accepted a batch that crosses "
		      "2^31 or 2^32", g_roc0, it);
		/* the next batch starts from what the receiver holds */
		memcpy(W->t, ts, sizeof(W->t));
		if (fail) {
			Y->nreject++;
			continue;
		}
		Y->naccept++;
		Y->nacc_trouble += (tr & (TR_DUP | TR_SWAP | TR_REPLAY)) != 0;
		for (i = 0; i < B.n; i++) {
			CHECK(err[i] == 0 || err[i] == EALREADY, "it %u: accepted, "
			      "packet %u has errno %d", it, i, err[i]);
			CHECK((vdp[i] == RX_DUP) == (err[i] == EALREADY),
			      "it %u: packet %u verdict %d, sequential errno %d",
			      it, i, vdp[i], err[i]);
			CHECK(ixp[i] == ixs[i] && flp[i] == fls[i],
			      "it %u: packet %u index %#llx flags %#x, sequential "
			      "%#llx %#x", it, i, (unsigned long long)ixp[i],
			      flp[i], (unsigned long long)ixs[i], fls[i]);
			nea += err[i] == EALREADY;
		}
		CHECK(nd == nea, "it %u: %u duplicates counted, sequential %u", it,
		      nd, nea);
		Y->ndups += nd;
		Y->nlates += nl;
		for (s = 0; s < B.nsess; s++) {
			uint32_t per[KMAX] = {0};
			CHECK(tp[s].n == ts[s].n, "it %u: session %u has %u "
			      "streams, sequential %u", it, s, tp[s].n, ts[s].n);
			Y->nnew += ts[s].n - B.t0[s].n;
			for (k = 0; k < ts[s].n && k < tp[s].n; k++) {
				const struct tseg_rec *a = &tp[s].st[k];
				const struct tseg_rec *c = &ts[s].st[k];
				CHECK(!memcmp(a, c, sizeof(*a)),
				      "it %u: session %u stream %u {%#x roc %u sl "
				      "%#x lix %#x:%#x bm %#x:%#x}, sequential {%#x "
				      "roc %u sl %#x lix %#x:%#x bm %#x:%#x}", it,
				      s, k, a->ssrc, a->roc, a->sl, a->lhi, a->llo,
				      a->bhi, a->blo, c->ssrc, c->roc, c->sl,
				      c->lhi, c->llo, c->bhi, c->blo);
				if (k < B.t0[s].n && c->roc != B.t0[s].st[k].roc)
					Y->nroll++;
			}
			for (i = 0; i < B.n; i++)
				if (B.p[i].sess == s)
					per[B.p[i].ssrc & 0xffu]++;
			for (k = 0; k < KMAX; k++)
				Y->nlong += per[k] > 4 * G.W;
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
	random_worlds(&W, 6000, &Y);
	/* the run met what it is about */
	CHECK(Y.naccept > 1500 && Y.nreject > 300, "accepted %u rejected %u",
	      Y.naccept, Y.nreject);
	CHECK(Y.nacc_trouble > 300, "accepted batches with swaps, duplicates or "
	      "replays %u", Y.nacc_trouble);
	CHECK(Y.ndups > 300 && Y.nlates > 300, "duplicates %u late %u", Y.ndups,
	      Y.nlates);
	CHECK(Y.nroll > 300, "rollovers inside accepted batches %u", Y.nroll);
	CHECK(Y.nnew > 300, "streams opened in accepted batches %u", Y.nnew);
	CHECK(Y.nlong > 300, "streams across several waves %u", Y.nlong);
	CHECK((Y.seen & all) == all, "seen %#x", Y.seen);
	CHECK(Y.ncross == 0, "%u batches crossed 2^31 from ROC 0..3", Y.ncross);
	/* the same worlds with about a third of the known streams at B - 2 .. B
	 * for B = 2^16, 2^31 and 2^32, between streams at ROC 0..2 and the
	 * ones the batches open: the segmented scan carries indices of 2^47
	 * and small ones side by side.  2^16 is an ordinary rollover: the
	 * shares of the run above hold (a quarter of the batches accepted, a
	 * twentieth of that many rollovers).  At the others some batches cross
	 * (declined, checked above), the others are accepted exactly */
	for (b = 0; b < 3; b++) {
		g_roc0 = BASE[b];
		random_worlds(&W, 1500, &Z);
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
