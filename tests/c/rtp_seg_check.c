/*
 * rtp_seg_check.c -- the in-order RTP rule composed per (session, SSRC)
 * (re_amd/csrc/hip/plan_rtp_seg.h, compiled as C) in the decomposition of
 * k_bps_plan (plan_buckets_rtp_streams.hip), against a sequential
 * restatement of stream_get_seq (stream.c:29-109), the sender's and the
 * receiver's ROC / s_l / index (srtp.c:203-215, 279-280, 310-321, 426-427;
 * misc.c:22-41) and the replay check (replay.c:32-62) written here.
 *
 * A batch interleaves 2-40 sessions with 1-9 SSRCs each: known streams, some
 * with s_l not set (SRTCP created them), new streams, 9th SSRCs; every
 * stream starts just below a multiple of 65536, so rollovers fall inside
 * batches; some batches carry a swap, a duplicate, a jump past 32768 or a
 * first packet below its window's top.  It runs
 *
 *   (a) as the kernel does: sessions cut into buckets of 2^bshift ids with
 *       `cap` entries each, a bucket's entries in an arbitrary order (the
 *       scatter's atomics), grouped by session, ranked by packet index, then
 *       the passes of k_bps_plan with `T` "threads" striding over the sorted
 *       positions (visited from the last thread down, so a pass that read
 *       what the same pass writes would show), small bshift / cap / segmax /
 *       T so that every boundary is met;
 *   (b) packet by packet through the sequential restatement.
 *
 * An accepted plan must equal (b) packet for packet (index, desc flags) and
 * state for state; and (a) must accept whenever (b) returns 0 everywhere,
 * every stream is in order (each packet but the stream's last leaves s_l at
 * its own seq), the receiver's indices increase and lie above the stored
 * lix apart from a stream's first packet, and the buckets hold the batch --
 * so rejecting everything does not pass.
 *
 *   gcc -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -o rtp_seg_check tests/c/rtp_seg_check.c && ./rtp_seg_check
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../re_amd/csrc/hip/plan_rtp_seg.h"

#define NMAX 600
#define SMAX 40
#define KMAX (RSEG_MAX + 1)     /* SSRCs a session's sender may use */

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

static uint32_t g_rng = 0x7f4a7c15u;

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
	int prot;
	uint32_t nsess, n;
	struct tab t0[SMAX];
	struct pkt p[NMAX];
};

/* ---- (b) the sequential restatement ---------------------------------- */

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

/* per packet: errno, index, desc flags, and whether it left s_l at its seq */
static void sequential(const struct batch *B, struct tab *t, int *err,
		       uint64_t *ix, uint32_t *fl, uint8_t *left)
{
	uint32_t i;
	memcpy(t, B->t0, sizeof(B->t0));
	for (i = 0; i < B->n; i++) {
		const struct pkt *p = &B->p[i];
		struct tseg_rec *st;
		uint32_t s_l, v;
		int diff;
		ix[i] = 0;
		fl[i] = 0;
		left[i] = 0;
		err[i] = ref_stream_get_seq(&t[p->sess], p->ssrc, p->seq, &st);
		if (err[i])
			continue;
		s_l = st->sl & 0xffffu;
		diff = (int)p->seq - (int)s_l;
		if (!B->prot && diff > 32768) {         /* srtp.c:313-316 */
			err[i] = ETIMEDOUT;
			continue;
		}
		if (diff <= -32768) {                   /* srtp.c:208-213 */
			st->roc++;
			s_l = 0;
		}
		fl[i] = SD_RUN | SD_CIPHER;
		if (B->prot) {
			ix[i] = 65536ull * st->roc + p->seq;
		}
		else {
			uint64_t lix = tseg_lix(*st), bm = tseg_bitmap(*st);
			v = ref_v(st->roc, s_l, p->seq);
			ix[i] = p->seq + (uint64_t)(int64_t)(int32_t)v * 65536ull;
			if (v != st->roc)
				fl[i] |= v + 1 == st->roc ? SD_ROC_P1 : SD_ROC_M1;
			if (!ref_replay_check(&lix, &bm, ix[i])) {
				/* (the rollover above stays, s_l does not) */
				st->sl = s_l | TSEG_SL_SET;
				err[i] = EALREADY;
				continue;
			}
			st->llo = (uint32_t)lix;
			st->lhi = (uint32_t)(lix >> 32);
			st->blo = (uint32_t)bm;
			st->bhi = (uint32_t)(bm >> 32);
		}
		if (p->seq > s_l)                       /* srtp.c:279-280 */
			s_l = p->seq;
		st->sl = s_l | TSEG_SL_SET;
		left[i] = s_l == p->seq;
	}
}

/* ---- (a) the kernel's decomposition ----------------------------------- */

struct geo {
	uint32_t bshift, cap, segmax, T;
};

/* 0 accepted (ix[], fl[], t[]: the plan), else the SPF_* bits */
static uint32_t planned(const struct batch *B, struct geo G, struct tab *t,
			uint64_t *ix, uint32_t *fl)
{
	const uint32_t nsb = 1u << G.bshift;
	const uint32_t nb = (B->nsess + nsb - 1) >> G.bshift;
	uint32_t fail = 0, b, i;

	memcpy(t, B->t0, sizeof(B->t0));
	for (b = 0; b < nb; b++) {
		const uint32_t s0 = b << G.bshift;
		const uint32_t ns = B->nsess - s0 < nsb ? B->nsess - s0 : nsb;
		/* the bucket's entries in an arbitrary order */
		static uint32_t ent[NMAX], gidx[NMAX], idx[NMAX], ru[NMAX];
		static uint32_t kn[NMAX], sl[NMAX];
		static struct tseg_look lk[NMAX];
		static struct tseg_pkt pk[NMAX];
		static uint8_t opens[NMAX];
		uint32_t cnt[SMAX], start[SMAX], nk[SMAX], nst[SMAX];
		uint32_t tmask[SMAX], acc[SMAX][RSEG_MAX];
		uint64_t bits[SMAX][RSEG_MAX], top[SMAX][RSEG_MAX];
		struct tseg_rec rec[SMAX][RSEG_MAX];
		uint32_t m = 0, f = 0, k, l, tid;

		for (i = 0; i < B->n; i++)
			if (B->p[i].sess >> G.bshift == b)
				ent[m++] = i;
		for (k = m; k > 1; k--) {
			const uint32_t q = rnd() % k, x = ent[q];
			ent[q] = ent[k - 1];
			ent[k - 1] = x;
		}
		if (m > G.cap) {
			fail |= SPF_SEG;
			continue;
		}
		memset(rec, 0, sizeof(rec));
		memset(acc, 0, sizeof(acc));
		memset(bits, 0, sizeof(bits));
		memset(top, 0, sizeof(top));
		for (l = 0; l < ns; l++) {
			nk[l] = nst[l] = B->t0[s0 + l].n;
			cnt[l] = tmask[l] = 0;
			memcpy(rec[l], B->t0[s0 + l].st, nk[l] * sizeof(rec[0][0]));
		}
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
			const struct pkt *p = &B->p[idx[k]];
			uint32_t q, slw;
			l = p->sess - s0;
			kn[k] = tseg_known(rec[l], nk[l], p->ssrc);
			slw = kn[k] != RSEG_NONE ? rec[l][kn[k]].sl : 0u;
			lk[k] = tseg_look_init(k);
			for (q = start[l]; q < k; q++)
				lk[k] = tseg_look_step(lk[k], q,
					B->p[idx[q]].ssrc == p->ssrc,
					B->p[idx[q]].seq, slw);
			opens[k] = (uint8_t)rseg_opens(kn[k], lk[k].a);
		}
		/* pass 2: the slot, new records, the streams' packet counts */
		EACH_POSITION {
			const struct pkt *p = &B->p[idx[k]];
			uint32_t nnew = 0, slot, q;
			l = p->sess - s0;
			sl[k] = RSEG_NONE;
			if (kn[k] == RSEG_NONE)
				for (q = start[l]; q < lk[k].a.first; q++)
					nnew += opens[q];
			slot = rseg_slot(kn[k], nk[l], nnew);
			if (rseg_enosr(slot)) {
				f |= SPF_SSRC;
				continue;
			}
			sl[k] = slot;
			if (opens[k]) {
				memset(&rec[l][slot], 0, sizeof(rec[l][slot]));
				rec[l][slot].ssrc = p->ssrc;
				if (nst[l] < slot + 1)
					nst[l] = slot + 1;
			}
			tmask[l] |= 1u << slot;
			if (acc[l][slot] < lk[k].a.rank + 1)
				acc[l][slot] = lk[k].a.rank + 1;
		}
		/* pass 3: the rule; a stream's last packet: the window's top */
		EACH_POSITION {
			const struct pkt *p = &B->p[idx[k]];
			if (sl[k] == RSEG_NONE)
				continue;
			l = p->sess - s0;
			pk[k] = tseg_packet(B->prot, rec[l][sl[k]], lk[k], p->seq);
			f |= pk[k].flags;
			ix[idx[k]] = pk[k].ix;
			fl[idx[k]] = pk[k].fl;
			if (lk[k].a.rank + 1 == acc[l][sl[k]])
				top[l][sl[k]] = tseg_top(tseg_lix(rec[l][sl[k]]),
							 pk[k].ix);
		}
		/* pass 4: the window bits */
		if (!B->prot)
			EACH_POSITION {
				if (sl[k] == RSEG_NONE)
					continue;
				l = B->p[idx[k]].sess - s0;
				bits[l][sl[k]] |= tseg_bit(top[l][sl[k]], pk[k].ix);
			}
		if (f) {
			fail |= f;
			continue;
		}
		/* the touched sessions' tables after the batch: a touched stream
		 * from its last packet, the others as they were */
		for (l = 0; l < ns; l++) {
			uint32_t x;
			if (!tmask[l])
				continue;
			t[s0 + l].n = nst[l];
			for (x = 0; x < nst[l]; x++)
				if (!(tmask[l] >> x & 1u))
					t[s0 + l].st[x] = rec[l][x];
		}
		EACH_POSITION {
			if (sl[k] == RSEG_NONE)
				continue;
			l = B->p[idx[k]].sess - s0;
			if (lk[k].a.rank + 1 == acc[l][sl[k]])
				t[s0 + l].st[sl[k]] = tseg_after(B->prot,
					rec[l][sl[k]], pk[k], bits[l][sl[k]]);
		}
#undef EACH_POSITION
	}
	return fail;
}

/* ---- batches ---------------------------------------------------------- */

static uint32_t ssrc_of(uint32_t s, uint32_t k)
{
	return 0x52000000u | s << 8 | k;
}

/* what the generator did on purpose */
enum { TR_NINTH = 1, TR_DUP = 2, TR_SWAP = 4, TR_JUMP = 8, TR_BELOW = 16,
       TR_UNSET = 32 };

static uint32_t make_batch(struct batch *B, int prot, uint32_t trouble_pm)
{
	/* the sender's next extended seq per (session, SSRC) */
	static uint64_t nxt[SMAX][KMAX];
	uint32_t done = 0, s, k, i;

	memset(B, 0, sizeof(*B));
	B->prot = prot;
	B->nsess = 2 + rnd() % (SMAX - 1);
	B->n = 1 + rnd() % NMAX;
	for (s = 0; s < B->nsess; s++) {
		struct tab *t = &B->t0[s];
		t->n = rnd() % (RSEG_MAX + 1);
		for (k = 0; k < KMAX; k++)
			nxt[s][k] = 65400 + rnd() % 136;
		for (k = 0; k < t->n; k++) {
			struct tseg_rec *r = &t->st[k];
			r->ssrc = ssrc_of(s, k);
			if (chance(200)) {
				/* SRTCP created it: zeros, s_l not set */
				done |= TR_UNSET;
				continue;
			}
			r->roc = rnd() % 3;
			nxt[s][k] += 65536ull * r->roc;
			r->sl = (uint32_t)((nxt[s][k] - 1) & 0xffffu) | TSEG_SL_SET;
			if (!prot) {
				const uint64_t lix = nxt[s][k] - 1;
				r->llo = (uint32_t)lix;
				r->lhi = (uint32_t)(lix >> 32);
				r->blo = rnd() << 8 | rnd() | 1u;
				r->bhi = rnd() << 8 | rnd();
			}
		}
	}
	for (i = 0; i < B->n; i++) {
		struct pkt *p = &B->p[i];
		uint32_t nss = RSEG_MAX;
		s = rnd() % B->nsess;
		/* mostly streams the table can hold; sometimes one more */
		if (chance(trouble_pm / 4)) {
			nss = KMAX;
			done |= TR_NINTH;       /* (maybe: the check asks (b)) */
		}
		k = chance(600) ? rnd() % (B->t0[s].n + 1) : rnd() % nss;
		if (k >= nss)
			k = nss - 1;
		p->sess = s;
		p->ssrc = ssrc_of(s, k);
		if (chance(trouble_pm / 40)) {
			nxt[s][k] += 40000;
			done |= TR_JUMP;
		}
		p->seq = (uint32_t)(nxt[s][k] & 0xffffu);
		nxt[s][k] += 1 + (chance(200) ? rnd() % 70 : 0);
	}
	for (i = 0; i + 1 < B->n; i++) {
		uint32_t j;
		if (!chance(trouble_pm / 8))
			continue;
		for (j = i + 1; j < B->n; j++)
			if (B->p[j].sess == B->p[i].sess &&
			    B->p[j].ssrc == B->p[i].ssrc)
				break;
		if (j == B->n)
			continue;
		if (chance(500)) {
			B->p[j].seq = B->p[i].seq;
			done |= TR_DUP;
		}
		else {
			const uint32_t w = B->p[i].seq;
			B->p[i].seq = B->p[j].seq;
			B->p[j].seq = w;
			done |= TR_SWAP;
		}
	}
	if (prot)
		return done;
	/* a stream whose first packet lies below its window's top, mostly on
	 * an unset bit */
	for (s = 0; s < B->nsess; s++)
		for (k = 0; k < B->t0[s].n; k++) {
			struct tseg_rec *r = &B->t0[s].st[k];
			uint32_t d;
			if (!chance(15) || !(r->sl & TSEG_SL_SET))
				continue;
			for (i = 0; i < B->n; i++)
				if (B->p[i].sess == s && B->p[i].ssrc == r->ssrc)
					break;
			if (i == B->n)
				continue;
			d = rnd() % 64;
			B->p[i].seq = ((r->sl & 0xffffu) - d) & 0xffffu;
			if (chance(700)) {
				const uint64_t bm = tseg_bitmap(*r) & ~(1ull << d);
				r->blo = (uint32_t)bm;
				r->bhi = (uint32_t)(bm >> 32);
			}
			done |= TR_BELOW;
		}
	return done;
}

/* the condition under which a plan must be accepted: (b) returns 0
 * everywhere (no ENOSR, ETIMEDOUT or EALREADY), every packet but its
 * stream's last left s_l at its own seq, the receiver's indices increase
 * within a stream and, from the second on, lie above the stored lix, and the
 * buckets hold the batch */
static int must_accept(const struct batch *B, struct geo G, const int *err,
		       const uint64_t *ix, const uint8_t *left)
{
	const uint32_t nb = (B->nsess + (1u << G.bshift) - 1) >> G.bshift;
	static uint32_t inb[SMAX], ins[SMAX];
	uint32_t i, j;
	memset(inb, 0, sizeof(inb));
	memset(ins, 0, sizeof(ins));
	for (i = 0; i < B->n; i++) {
		if (err[i])
			return 0;
		inb[B->p[i].sess >> G.bshift]++;
		ins[B->p[i].sess]++;
	}
	for (i = 0; i < nb; i++)
		if (inb[i] > G.cap)
			return 0;
	for (i = 0; i < B->nsess; i++)
		if (ins[i] > G.segmax)
			return 0;
	for (i = 0; i < B->n; i++) {
		const struct pkt *p = &B->p[i];
		const struct tab *t = &B->t0[p->sess];
		uint64_t lix = 0;
		uint32_t k;
		for (k = 0; k < t->n; k++)
			if (t->st[k].ssrc == p->ssrc)
				lix = tseg_lix(t->st[k]);
		for (j = i; j-- > 0;)
			if (B->p[j].sess == p->sess && B->p[j].ssrc == p->ssrc) {
				if (!left[j])
					return 0;
				if (!B->prot && (ix[j] >= ix[i] || ix[i] <= lix))
					return 0;
				break;
			}
	}
	return 1;
}

int main(void)
{
	static struct batch B;
	static struct tab ts[SMAX], tp[SMAX];
	static int err[NMAX];
	static uint64_t ixs[NMAX], ixp[NMAX];
	static uint32_t fls[NMAX], flp[NMAX];
	static uint8_t left[NMAX];
	const uint32_t all = TR_NINTH | TR_DUP | TR_SWAP | TR_JUMP | TR_BELOW |
			     TR_UNSET;
	uint32_t it, naccept = 0, nreject = 0, nmust = 0, seen = 0, nroll = 0;
	uint32_t nacc_mode[2] = {0, 0};

	for (it = 0; it < 6000; it++) {
		const int prot = (int)(it % 2);
		const struct geo G = {
			.bshift = rnd() % 4,
			.cap = chance(850) ? NMAX : 16 + rnd() % 200,
			.segmax = chance(850) ? NMAX : 8 + rnd() % 64,
			.T = 1 + rnd() % 70};
		const uint32_t tr = make_batch(&B, prot, it % 4 < 2 ? 300 : 0);
		uint32_t fail, i, s, k;
		int must;

		sequential(&B, ts, err, ixs, fls, left);
		memset(ixp, 0, sizeof(ixp));
		memset(flp, 0, sizeof(flp));
		fail = planned(&B, G, tp, ixp, flp);
		must = must_accept(&B, G, err, ixs, left);
		nmust += (uint32_t)must;
		seen |= tr;
		CHECK(!(must && fail), "it %u prot %d: rejected (SPF %#x) a batch "
		      "it must accept", it, prot, fail);
		if (fail) {
			nreject++;
			continue;
		}
		naccept++;
		nacc_mode[prot]++;
		for (i = 0; i < B.n; i++) {
			CHECK(!err[i], "it %u prot %d: accepted, packet %u has "
			      "errno %d", it, prot, i, err[i]);
			CHECK(ixp[i] == ixs[i] && flp[i] == fls[i],
			      "it %u prot %d: packet %u index %#llx flags %#x, "
			      "sequential %#llx %#x", it, prot, i,
			      (unsigned long long)ixp[i], flp[i],
			      (unsigned long long)ixs[i], fls[i]);
		}
		for (s = 0; s < B.nsess; s++) {
			CHECK(tp[s].n == ts[s].n, "it %u prot %d: session %u has "
			      "%u streams, sequential %u", it, prot, s, tp[s].n,
			      ts[s].n);
			for (k = 0; k < ts[s].n && k < tp[s].n; k++) {
				const struct tseg_rec *a = &tp[s].st[k];
				const struct tseg_rec *c = &ts[s].st[k];
				CHECK(!memcmp(a, c, sizeof(*a)),
				      "it %u prot %d: session %u stream %u {%#x "
				      "roc %u sl %#x lix %#x:%#x bm %#x:%#x}, "
				      "sequential {%#x roc %u sl %#x lix %#x:%#x "
				      "bm %#x:%#x}", it, prot, s, k, a->ssrc,
				      a->roc, a->sl, a->lhi, a->llo, a->bhi, a->blo,
				      c->ssrc, c->roc, c->sl, c->lhi, c->llo,
				      c->bhi, c->blo);
				if (k < B.t0[s].n && c->roc != B.t0[s].st[k].roc)
					nroll++;
			}
		}
	}
	/* the run met what it is about */
	CHECK(nacc_mode[0] > 300 && nacc_mode[1] > 300, "accepted %u / %u",
	      nacc_mode[0], nacc_mode[1]);
	CHECK(nreject > 300, "rejected %u", nreject);
	CHECK(nmust > 900, "must-accept batches %u", nmust);
	CHECK(nroll > 1000, "rollovers inside accepted batches %u", nroll);
	CHECK((seen & all) == all, "seen %#x", seen);
	printf("%u batches: %u accepted (%u must), %u rejected, %d wrong\n", it,
	       naccept, nmust, nreject, g_bad);
	return g_bad ? 1 : 0;
}
