/*
 * rtcp_seg_fold_check.c -- settling forged packets of many-session SRTCP
 * unprotect batches (re_amd/csrc/hip/plan_rtcp_seg_fold.h, compiled as C) in
 * the decomposition of k_bprf_settle (plan_buckets_rtcp_fold.hip), against a
 * sequential restatement of srtcp_decrypt on HMAC suites written here:
 * stream_get (stream.c:29-84), the tag first (srtcp.c:200-201), then
 * srtp_replay_check (srtcp.c:208-209; replay.c:32-62).
 *
 * A world is 2-40 sessions whose senders use 1-9 SSRCs each, some streams
 * starting just below 0x7fffffff, received in a few batches one after the
 * other: the tables a batch starts from are the ones the sequential receiver
 * left.  A batch interleaves the streams; per stream it carries swaps, gaps,
 * duplicates, replays of the batch before and indices more than 64 below the
 * top, as tests/c/rtcp_seg_rx_check.c makes them, and about 5 % forged
 * arrivals: random ones, one with an index far above its stream's top
 * followed by genuine packets, a forged copy ahead of and behind its genuine
 * packet, one on an unset bit of the stored window (the genuine packet of that
 * index later in the batch), streams forged throughout and SSRCs that only a
 * forged arrival opens.  Each batch runs
 *
 *   (a) as the kernel does: sessions cut into buckets of 2^bshift ids, a
 *       bucket's entries in an arbitrary order, grouped by session, ranked by
 *       packet index, the look back for slot and rank, the streams of a
 *       session one behind the other, the segmented (sum, max) scan over
 *       rsfold_elem with `ept` consecutive positions per "thread", `W` threads
 *       per "wave" and the waves' aggregates, rsfold_result per packet with
 *       look-back K, the tables after -- once with every arrival taken for
 *       authentic (the plan that ran first) and once masked (the settle);
 *   (b) packet by packet through the sequential receiver.
 *
 * A settled batch must equal (b) packet for packet (result, desc word of the
 * authentic ones) and record for record.  The settled batches must be exactly
 * those in which no slot overflows, the buckets hold the batch, and rx_replay
 * over each stream's arrivals with the forged ones masked, u[] and mx[] from
 * the serial recurrence, settles every authentic packet.  Where the unmasked
 * plan of the same batch is accepted too, the results of the authentic packets
 * differ from its verdicts only EALREADY -> accepted and only behind a forged
 * arrival of the same stream, and rsfold_flip names exactly those of them that
 * carry E.
 *
 *   rtcp_seg_fold_check         the random worlds
 *   rtcp_seg_fold_check FILE    a recorded traffic (lines "B", then "session
 *                               ssrc index forged" per arrival; tables start
 *                               empty): per batch the sequential receiver's
 *                               errno counts and whether (a) settles it at the
 *                               kernel's own widths
 *
 *   gcc -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -o rtcp_seg_fold_check tests/c/rtcp_seg_fold_check.c && \
 *       ./rtcp_seg_fold_check
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../re_amd/csrc/hip/plan_rtcp_seg_fold.h"

#define NMAX 600
#define SMAX 40
#define KMAX (RSEG_MAX + 1)     /* SSRCs a session's sender may use */
#define TMAX 64                 /* "threads" */
#define LASTN 4                 /* indices of the batch before kept for replays */
#define IXMASK 0x7fffffffu
#define ERR_AUTH 1000           /* EAUTH has no errno everywhere */

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

static uint32_t g_rng = 0x0f01d5edu;

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
	struct rseg_rec st[RSEG_MAX];
};

struct pkt {
	uint32_t sess, ssrc, word;      /* E || index */
	uint32_t forged;                /* its tag does not verify */
};

struct batch {
	uint32_t nsess, n;
	struct tab t0[SMAX];
	struct pkt p[NMAX];
};

/* what every packet of these batches shares: an HMAC suite, 80-bit tag, and
 * lengths that pass the length checks */
#define PKT_L 64u

static struct sgpu_rplan_in plan_in(uint32_t n)
{
	struct sgpu_rplan_in c;
	memset(&c, 0, sizeof(c));
	c.n = n;
	c.tag = 10;
	c.hmac = 1;
	c.encrypted = 1;
	c.maxlen = 1u << 20;
	return c;
}

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

/* per packet: errno (0, EALREADY, ERR_AUTH, ENOSR) and the desc word an
 * authentic packet's job runs with (an EALREADY packet is authenticated,
 * never deciphered) */
static void sequential(const struct batch *B, struct tab *t, int *err,
		       uint64_t *desc)
{
	uint32_t i;
	memcpy(t, B->t0, sizeof(B->t0));
	for (i = 0; i < B->n; i++) {
		const struct pkt *p = &B->p[i];
		struct rseg_rec *st;
		uint64_t lix, bm;
		desc[i] = 0;
		err[i] = ref_stream_get(&t[p->sess], p->ssrc, &st);
		if (err[i])
			continue;
		if (p->forged) {
			err[i] = ERR_AUTH;      /* srtcp.c:200-201 */
			continue;
		}
		lix = st->ix;
		bm = (uint64_t)st->bhi << 32 | st->blo;
		if (!ref_replay_check(&lix, &bm, p->word & IXMASK)) {
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

/* ---- (a) the kernel's decomposition ----------------------------------- */

struct geo {
	uint32_t bshift, segmax, T, W, ept, K;  /* cap = T * ept */
};

#define PS_FORGED 0x4000u

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

/*
 * masked = 0: the plan that ran first, every arrival taken for authentic
 * (plan_rtcp_seg_rx.h's rule: rsfold_* with forged = 0 are rsrx_*).
 * masked = 1: the settle; desc0[] is the first plan's, rb[] the byte per
 * packet (rsfold_byte).
 * 0 settled (desc[], res[], t[]), else the SPF_* bits.
 */
static uint32_t planned(const struct batch *B, struct geo G, int masked,
			const uint64_t *desc0, struct tab *t, uint64_t *desc,
			int *res, uint8_t *rb)
{
	const struct sgpu_rplan_in in = plan_in(B->n);
	const uint32_t nsb = 1u << G.bshift, cap = G.T * G.ept;
	const uint32_t nb = (B->nsess + nsb - 1) >> G.bshift;
	uint32_t fail = 0, b, i;

	memcpy(t, B->t0, sizeof(B->t0));
	for (b = 0; b < nb; b++) {
		const uint32_t s0 = b << G.bshift;
		const uint32_t ns = B->nsess - s0 < nsb ? B->nsess - s0 : nsb;
		static uint32_t ent[NMAX], gidx[NMAX], idx[NMAX], ru[NMAX];
		static uint32_t kn[NMAX], sl[NMAX], rank[NMAX], firstk[NMAX];
		static uint8_t opens[NMAX];
		static uint32_t pi[NMAX], pw[NMAX], ps[NMAX];
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
#define REC(l, x) ((x) < nk[l] ? B->t0[s0 + (l)].st[x] : rsrx_new(tss[l][x]))
#define SMX(l, x) rsfold_smx(REC(l, x), u[first[l][x] + acc[l][x] - 1],      \
			     mx[first[l][x] + acc[l][x] - 1])
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
		/* pass 1: the known slot, the look back (forged arrivals take
		 * and open slots like the others) */
		EACH_POSITION {
			const struct pkt *q = &B->p[idx[k]];
			struct rseg_look lk = rseg_look_init(k);
			uint32_t w;
			l = q->sess - s0;
			kn[k] = rsrx_known(tss[l], nk[l], q->ssrc);
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
				first[l][x] = rsrx_first(start[l], acc[l], x);
		EACH_POSITION {
			l = B->p[idx[k]].sess - s0;
			p = first[l][sl[k]] + rank[k];
			pi[p] = idx[k];
			pw[p] = B->p[idx[k]].word;
			ps[p] = l << 3 | sl[k] |
				(masked && B->p[idx[k]].forged ? PS_FORGED : 0u);
		}
		/* the scan: ept consecutive positions per thread */
		for (tid = 0; tid < G.T; tid++) {
			agg[tid] = rx_seg_identity();
			for (j = 0; j < G.ept; j++) {
				p = tid * G.ept + j;
				if (p >= m)
					continue;
				l = ps[p] >> 3 & 0xffu;
				x = ps[p] & 7u;
				hd[p] = p == first[l][x];
				dv[p] = rsfold_elem(hd[p], pw[p],
						    (ps[p] & PS_FORGED) != 0,
						    hd[p] ? 0u : pw[p - 1],
						    !hd[p] && (ps[p - 1] & PS_FORGED));
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
		/* per packet: the checks, the result with positions local to its
		 * stream */
		for (tid = G.T; tid-- > 0;)
			for (p = tid; p < m; p += G.T) {
				struct rseg_rec st;
				uint32_t f0, pf;
				int r, flip;
				l = ps[p] >> 3 & 0xffu;
				x = ps[p] & 7u;
				f0 = first[l][x];
				st = REC(l, x);
				pf = rsrx_flags(in, st, 1, PKT_L, pw[p]);
				if (pf) {
					f |= pf;
					continue;
				}
				r = rsfold_result(u + f0, mx + f0, p - f0, G.K, st,
						  (ps[p] & PS_FORGED) != 0);
				if (r < 0) {
					f |= SPF_REPLAY;
					continue;
				}
				res[pi[p]] = r;
				if (r == RSF_AUTH) {
					rb[pi[p]] = rsfold_byte(r, 0);
					continue;
				}
				desc[pi[p]] = rsfold_desc(r, pw[p]);
				flip = 0;
				if (masked)
					flip = rsfold_flip(desc0[pi[p]], desc[pi[p]],
							   in.encrypted);
				rb[pi[p]] = rsfold_byte(r, flip);
				if (r == RSF_DUP)
					continue;
				bits[l][x] |= rsrx_bit(st, SMX(l, x), u[p]);
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
				struct rseg_rec st = REC(l, x);
				if (tmask[l] >> x & 1u)
					st = rsrx_after(st, SMX(l, x), bits[l][x]);
				t[s0 + l].st[x] = st;
			}
		}
#undef EACH_POSITION
#undef REC
#undef SMX
	}
	return fail;
}

/* ---- the property: which batches a settle must take --------------------- */

/* every stream's arrivals, the forged ones masked (masked = 0: none is), u[]
 * and mx[] from the serial recurrence, settle under rx_replay; no slot
 * overflows (err: the sequential receiver's); the buckets hold the batch */
static int must_accept(const struct batch *B, struct geo G, const int *err,
		       int masked)
{
	const uint32_t nb = (B->nsess + (1u << G.bshift) - 1) >> G.bshift;
	static uint32_t inb[SMAX], ins[SMAX];
	static int64_t u[NMAX], mx[NMAX];
	static uint8_t seen[NMAX], fg[NMAX];
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
		struct rseg_rec st = rsrx_new(p->ssrc);
		int64_t m = RX_NEG;
		if (seen[i])
			continue;
		for (j = 0; j < t->n; j++)
			if (t->st[j].ssrc == p->ssrc)
				st = t->st[j];
		for (j = i, c = 0; j < B->n; j++)
			if (B->p[j].sess == p->sess && B->p[j].ssrc == p->ssrc) {
				seen[j] = 1;
				fg[c] = masked && B->p[j].forged;
				u[c] = fg[c] ? -1 : (int64_t)(B->p[j].word & IXMASK);
				mx[c] = m;
				m = rx_max(m, u[c]);
				c++;
			}
		for (j = 0; j < c; j++)
			if (!fg[j] &&
			    rx_replay(u, mx, j, G.K, (int64_t)st.ix,
				      (uint64_t)st.bhi << 32 | st.blo, 1) ==
			    RX_UNSETTLED)
				return 0;
	}
	return 1;
}

/* ---- worlds ------------------------------------------------------------- */

struct world {
	uint32_t nsess;
	uint32_t nss[SMAX];             /* SSRCs the session's sender uses */
	uint64_t nxt[SMAX][KMAX];       /* its next index, before the 31-bit cut */
	uint32_t last[SMAX][KMAX][LASTN], nlast[SMAX][KMAX];
	struct tab t[SMAX];
};

static uint32_t ssrc_of(uint32_t s, uint32_t k)
{
	return 0x52000000u | s << 8 | k;
}

/* what the generator did on purpose */
enum { TR_NINTH = 1, TR_DUP = 2, TR_SWAP = 4, TR_REPLAY = 8, TR_GAP = 16,
       TR_FAR = 32, TR_WRAP = 64, TR_FORGED = 128, TR_FHIGH = 256,
       TR_FAHEAD = 512, TR_FBEHIND = 1024, TR_FBIT = 2048, TR_FALL = 4096 };

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
		for (k = 0; k < KMAX; k++) {
			W->nxt[s][k] = 1 + rnd() % 5000;
			if (chance(150)) {
				/* just below the 31-bit wrap */
				W->nxt[s][k] = 0x7fffffffull - rnd() % 40;
				done |= TR_WRAP;
			}
		}
		for (k = 0; k < t->n; k++) {
			struct rseg_rec *r = &t->st[k];
			r->ssrc = ssrc_of(s, k);
			r->ix = (uint32_t)((W->nxt[s][k] - 1) & IXMASK);
			r->blo = rnd() << 8 | rnd() | 1u;
			r->bhi = rnd() << 8 | rnd();
		}
	}
	return done;
}

static const struct rseg_rec *stored(const struct batch *B, uint32_t s,
				     uint32_t ssrc)
{
	uint32_t j;
	for (j = 0; j < B->t0[s].n; j++)
		if (B->t0[s].st[j].ssrc == ssrc)
			return &B->t0[s].st[j];
	return NULL;
}

/* forged_pm: the share of arrivals forged at random, in 1/1000 */
static uint32_t make_batch(struct world *W, struct batch *B, uint32_t trouble_pm,
			   uint32_t forged_pm)
{
	static uint32_t arr[NMAX];
	uint32_t done = 0, s, k, i, j, c;

	memset(B, 0, sizeof(*B));
	B->nsess = W->nsess;
	B->n = 1 + rnd() % NMAX;
	memcpy(B->t0, W->t, sizeof(B->t0));
	for (i = 0; i < B->n; i++) {
		struct pkt *p = &B->p[i];
		s = rnd() % W->nsess;
		k = rnd() % W->nss[s];
		p->sess = s;
		p->ssrc = ssrc_of(s, k);
		p->word = (uint32_t)(W->nxt[s][k] & IXMASK) | (rnd() & 1u) << 31;
		W->nxt[s][k]++;
		if (chance(trouble_pm / 4)) {
			W->nxt[s][k] += 1 + rnd() % 3;  /* a gap */
			done |= TR_GAP;
		}
	}
	/* per stream: its arrivals' places, then the trouble */
	for (s = 0; s < W->nsess; s++)
		for (k = 0; k < W->nss[s]; k++) {
			const uint32_t x = ssrc_of(s, k);
			const struct rseg_rec *rec = stored(B, s, x);
			uint32_t d, w;
			for (i = 0, c = 0; i < B->n; i++)
				if (B->p[i].sess == s && B->p[i].ssrc == x)
					arr[c++] = i;
			for (j = 0; j < c; j++) {
				if (!chance(trouble_pm / 8))
					continue;
				switch (rnd() % 4) {
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
				case 2:
					if (!W->nlast[s][k])
						break;
					B->p[arr[j]].word =
						W->last[s][k][rnd() % W->nlast[s][k]];
					done |= TR_REPLAY;
					break;
				default:
					/* far below the window's top */
					if (chance(700))
						break;
					B->p[arr[j]].word =
						((B->p[arr[j]].word & IXMASK) - 64 -
						 rnd() % 200) & IXMASK;
					done |= TR_FAR;
					break;
				}
			}
			if (!forged_pm)
				goto keep;
			/* the forged arrivals: at random ... */
			for (j = 0; j < c; j++)
				if (chance(forged_pm)) {
					B->p[arr[j]].forged = 1;
					done |= TR_FORGED;
				}
			/* ... one far above the top, genuine ones behind it */
			if (c >= 3 && chance(40)) {
				j = rnd() % (c - 2);
				w = (B->p[arr[j]].word & IXMASK) + 100 + rnd() % 5000;
				if (w <= IXMASK) {
					B->p[arr[j]].word = w | 0x80000000u;
					B->p[arr[j]].forged = 1;
					B->p[arr[j + 1]].forged = 0;
					done |= TR_FHIGH;
				}
			}
			/* ... a forged copy ahead of / behind its genuine packet */
			if (c >= 2 && chance(40)) {
				j = rnd() % (c - 1);
				d = j + 1 + rnd() % (c - 1 - j);
				if (chance(500)) {
					B->p[arr[j]].word = B->p[arr[d]].word;
					B->p[arr[j]].forged = 1;
					B->p[arr[d]].forged = 0;
					done |= TR_FAHEAD;
				}
				else {
					B->p[arr[d]].word = B->p[arr[j]].word;
					B->p[arr[d]].forged = 1;
					B->p[arr[j]].forged = 0;
					done |= TR_FBEHIND;
				}
			}
			/* ... one on an unset bit of the stored window, the
			 * genuine packet of that index behind it */
			if (rec && c >= 2 && chance(60)) {
				const uint64_t bm = (uint64_t)rec->bhi << 32 | rec->blo;
				for (d = 1; d < 64 && d <= rec->ix; d++)
					if (!(bm >> d & 1u))
						break;
				if (d < 64 && d <= rec->ix) {
					j = rnd() % (c - 1);
					B->p[arr[j]].word = (rec->ix - d) | 0x80000000u;
					B->p[arr[j]].forged = 1;
					B->p[arr[j + 1]].word = B->p[arr[j]].word;
					B->p[arr[j + 1]].forged = 0;
					done |= TR_FBIT;
				}
			}
			/* ... a stream forged throughout (an SSRC the table does
			 * not hold is opened by a forged arrival alone) */
			if (c && chance(30)) {
				for (j = 0; j < c; j++)
					B->p[arr[j]].forged = 1;
				done |= TR_FALL;
			}
keep:
			/* what the receiver may have taken of it: replays */
			for (j = c, W->nlast[s][k] = 0; j-- > 0 &&
			     W->nlast[s][k] < LASTN;)
				if (!B->p[arr[j]].forged)
					W->last[s][k][W->nlast[s][k]++] =
						B->p[arr[j]].word;
		}
	return done;
}

/* ---- a recorded traffic -------------------------------------------------- */

static int replay_file(const char *path)
{
	static struct batch B;
	static struct tab ts[SMAX], tp[SMAX];
	static int err[NMAX], rp[NMAX];
	static uint64_t ds[NMAX], dp[NMAX], d0[NMAX];
	static uint8_t rb[NMAX];
	const struct geo G = {.bshift = 4, .segmax = NMAX, .T = 64, .W = 64,
			      .ept = (NMAX + 63) / 64, .K = RX_LOOKBACK};
	FILE *f = fopen(path, "r");
	char line[128];
	uint32_t nbatch = 0;
	int more = 1;
	if (!f) {
		perror(path);
		return 2;
	}
	memset(&B, 0, sizeof(B));
	while (more) {
		unsigned s, x, q, fg;
		more = fgets(line, sizeof(line), f) != NULL;
		if (more && line[0] != 'B' &&
		    sscanf(line, "%u %x %u %u", &s, &x, &q, &fg) == 4) {
			if (s >= SMAX || B.n >= NMAX) {
				printf("batch %u: out of range\n", nbatch);
				fclose(f);
				return 2;
			}
			if (B.nsess < s + 1)
				B.nsess = s + 1;
			B.p[B.n].sess = s;
			B.p[B.n].ssrc = x;
			B.p[B.n].word = (q & IXMASK) | 0x80000000u;
			B.p[B.n].forged = fg != 0;
			B.n++;
			continue;
		}
		if (B.n) {
			uint32_t i, ne[4] = {0, 0, 0, 0}, fail;
			if (B.nsess < 2)
				B.nsess = 2;
			sequential(&B, ts, err, ds);
			memset(d0, 0, sizeof(d0));
			fail = planned(&B, G, 1, d0, tp, dp, rp, rb);
			for (i = 0; i < B.n; i++)
				ne[err[i] == 0 ? 0 : err[i] == EALREADY ? 1 :
				   err[i] == ERR_AUTH ? 2 : 3]++;
			printf("batch %u: %u packets ok %u already %u forged %u "
			       "other %u settle %s must %d\n", nbatch, B.n, ne[0],
			       ne[1], ne[2], ne[3], fail ? "declined" : "settled",
			       must_accept(&B, G, err, 1));
			memcpy(B.t0, ts, sizeof(B.t0));
			B.n = 0;
			nbatch++;
		}
	}
	fclose(f);
	return 0;
}

int main(int argc, char **argv)
{
	static struct world W;
	static struct batch B;
	static struct tab ts[SMAX], tp[SMAX], tq[SMAX];
	static int err[NMAX], r0[NMAX], r1[NMAX];
	static uint64_t ds[NMAX], d0[NMAX], d1[NMAX];
	static uint8_t b0[NMAX], b1[NMAX];
	const uint32_t all = TR_NINTH | TR_DUP | TR_SWAP | TR_REPLAY | TR_GAP |
			     TR_FAR | TR_WRAP | TR_FORGED | TR_FHIGH | TR_FAHEAD |
			     TR_FBEHIND | TR_FBIT | TR_FALL;
	uint32_t it, nsettled = 0, ndeclined = 0, nmust = 0, seen = 0, sseen = 0;
	uint32_t nunsettled = 0, nforged = 0, npackets = 0, nflips = 0, nboth = 0;
	uint32_t nkept = 0, nopened = 0, nsetbit = 0, ninorder = 0, nlost = 0;
	uint32_t wtr = 0;               /* what the world was made with */

	if (argc > 1)
		return replay_file(argv[1]);
	for (it = 0; it < 6000; it++) {
		struct geo G;
		const uint32_t pm = it % 8 < 2 ? 0 : it % 8 < 6 ? 60 : 300;
		uint32_t tr, fail0, fail, i, j, s, k, nf = 0;
		int must;

		if (it % 4 == 0)
			seen |= wtr = make_world(&W, pm);
		G.bshift = rnd() % 4;
		G.segmax = chance(850) ? NMAX : 8 + rnd() % 64;
		G.W = 1u << (1 + rnd() % 4);            /* 2 .. 16 */
		G.T = G.W * (1 + rnd() % (TMAX / G.W));
		G.ept = 1 + rnd() % 4;
		if (chance(850))                        /* cap >= the batch */
			G.ept = (NMAX + G.T - 1) / G.T;
		G.K = chance(500) ? RX_LOOKBACK : 2 + rnd() % 12;
		tr = make_batch(&W, &B, pm, it % 16 == 15 ? 0 : 50);
		sequential(&B, ts, err, ds);
		memset(d0, 0, sizeof(d0));
		memset(d1, 0, sizeof(d1));
		memset(r0, 0, sizeof(r0));
		memset(r1, 0, sizeof(r1));
		memset(b0, 0, sizeof(b0));
		memset(b1, 0, sizeof(b1));
		/* the plan that ran first, then the settle */
		fail0 = planned(&B, G, 0, NULL, tq, d0, r0, b0);
		fail = planned(&B, G, 1, d0, tp, d1, r1, b1);
		must = must_accept(&B, G, err, 1);
		nmust += (uint32_t)must;
		seen |= tr;
		CHECK(!(must && fail), "it %u: declined (SPF %#x) a batch it must "
		      "settle", it, fail);
		CHECK(must || fail, "it %u: settled a batch the sequential masked "
		      "rx_replay does not settle", it);
		/* the next batch starts from what the receiver holds */
		memcpy(W.t, ts, sizeof(W.t));
		if (fail) {
			ndeclined++;
			nunsettled += fail == SPF_REPLAY;
			nlost += !fail0 && fail == SPF_REPLAY;
			continue;
		}
		nsettled++;
		sseen |= tr | (wtr & TR_WRAP);
		for (i = 0; i < B.n; i++) {
			const int e = r1[i] == RSF_OK ? 0 :
				      r1[i] == RSF_DUP ? EALREADY : ERR_AUTH;
			CHECK(err[i] == e, "it %u: packet %u result %d, sequential "
			      "errno %d", it, i, r1[i], err[i]);
			CHECK(rsfold_byte_result(b1[i]) == r1[i], "it %u: packet %u "
			      "byte %#x, result %d", it, i, b1[i], r1[i]);
			if (B.p[i].forged) {
				CHECK(!(b1[i] & SV_CIPHERED), "it %u: forged packet "
				      "%u named for the decipher launch", it, i);
				nf++;
				continue;
			}
			CHECK(d1[i] == ds[i], "it %u: packet %u desc %#llx, "
			      "sequential %#llx", it, i, (unsigned long long)d1[i],
			      (unsigned long long)ds[i]);
		}
		nforged += nf;
		npackets += B.n;
		for (s = 0; s < B.nsess; s++) {
			CHECK(tp[s].n == ts[s].n, "it %u: session %u has %u "
			      "streams, sequential %u", it, s, tp[s].n, ts[s].n);
			for (k = 0; k < ts[s].n && k < tp[s].n; k++) {
				const struct rseg_rec *a = &tp[s].st[k];
				const struct rseg_rec *c = &ts[s].st[k];
				uint32_t na = 0, nfg = 0;
				CHECK(!memcmp(a, c, sizeof(*a)),
				      "it %u: session %u stream %u {%#x lix %#x bm "
				      "%#x:%#x}, sequential {%#x lix %#x bm %#x:%#x}",
				      it, s, k, a->ssrc, a->ix, a->bhi, a->blo,
				      c->ssrc, c->ix, c->bhi, c->blo);
				for (i = 0; i < B.n; i++)
					if (B.p[i].sess == s && B.p[i].ssrc == c->ssrc) {
						na++;
						nfg += B.p[i].forged;
					}
				if (!na || na != nfg)
					continue;
				/* forged throughout: the record stays, a new one
				 * is the SSRC and an empty window */
				if (k < B.t0[s].n) {
					CHECK(!memcmp(c, &B.t0[s].st[k], sizeof(*c)),
					      "it %u: session %u stream %u forged "
					      "throughout moved", it, s, k);
					nkept++;
				}
				else {
					CHECK(!c->ix && !c->blo && !c->bhi,
					      "it %u: session %u stream %u opened "
					      "by forged packets holds a window", it,
					      s, k);
					nopened++;
				}
			}
		}
		/* a forged arrival on an unset bit of the stored window, the
		 * genuine packet of that index accepted behind it */
		for (i = 0; i < B.n; i++) {
			const struct rseg_rec *rec =
				stored(&B, B.p[i].sess, B.p[i].ssrc);
			const uint32_t ix = B.p[i].word & IXMASK;
			if (!B.p[i].forged || !rec || ix > rec->ix ||
			    rec->ix - ix >= 64 ||
			    (((uint64_t)rec->bhi << 32 | rec->blo) >>
			     (rec->ix - ix) & 1u))
				continue;
			for (j = i + 1; j < B.n; j++)
				if (B.p[j].sess == B.p[i].sess &&
				    B.p[j].ssrc == B.p[i].ssrc &&
				    !B.p[j].forged && (B.p[j].word & IXMASK) == ix) {
					nsetbit += err[j] == 0;
					break;
				}
		}
		/* relative to the plan that ran: only EALREADY -> accepted, only
		 * behind a forged arrival of the same stream */
		if (fail0)
			continue;
		nboth++;
		for (i = 0, j = 0; i < B.n; i++)
			j += r0[i] == RSF_DUP;
		ninorder += !j && nf;
		for (i = 0; i < B.n; i++) {
			int behind = 0;
			const int flip = (b1[i] & SV_CIPHERED) != 0;
			if (B.p[i].forged)
				continue;
			CHECK(flip == (r0[i] == RSF_DUP && r1[i] == RSF_OK &&
				       B.p[i].word >> 31),
			      "it %u: packet %u flip %d, verdicts %d -> %d, E %u",
			      it, i, flip, r0[i], r1[i], B.p[i].word >> 31);
			if (r0[i] == r1[i])
				continue;
			CHECK(r0[i] == RSF_DUP && r1[i] == RSF_OK, "it %u: packet "
			      "%u moved %d -> %d", it, i, r0[i], r1[i]);
			for (j = 0; j < i; j++)
				behind |= B.p[j].forged &&
					  B.p[j].sess == B.p[i].sess &&
					  B.p[j].ssrc == B.p[i].ssrc;
			CHECK(behind, "it %u: packet %u moved with no forged "
			      "arrival of its stream before it", it, i);
			nflips += (uint32_t)flip;
		}
	}
	/* the run met what it is about */
	CHECK(nsettled > 1500 && ndeclined > 300, "settled %u declined %u",
	      nsettled, ndeclined);
	CHECK(nunsettled > 30, "declined for a copy beyond the look-back only %u",
	      nunsettled);
	CHECK(nlost > 0, "no settle met a copy beyond the look-back behind an "
	      "accepted plan");
	CHECK(nforged * 100 > npackets * 3 && nforged * 100 < npackets * 9,
	      "forged %u of %u packets in settled batches", nforged, npackets);
	CHECK(nboth > 1000 && nflips > 100, "settled behind an accepted plan %u, "
	      "packets to decipher %u", nboth, nflips);
	CHECK(ninorder > 100, "settled behind a plan without EALREADY %u",
	      ninorder);
	CHECK(nkept > 30 && nopened > 30, "streams forged throughout: known %u, "
	      "opened %u", nkept, nopened);
	CHECK(nsetbit > 30, "genuine packets accepted behind a forged one on an "
	      "unset bit %u", nsetbit);
	CHECK((seen & all) == all, "seen %#x", seen);
	CHECK((sseen & all & ~(uint32_t)TR_NINTH) == (all & ~(uint32_t)TR_NINTH),
	      "seen in settled batches %#x", sseen);
	printf("%u batches: %u settled (%u must), %u declined (%u unsettled), "
	       "%u forged packets, %u deciphered behind them, %d wrong\n", it,
	       nsettled, nmust, ndeclined, nunsettled, nforged, nflips, g_bad);
	return g_bad ? 1 : 0;
}
