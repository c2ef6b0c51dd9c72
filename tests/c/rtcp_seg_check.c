/*
 * rtcp_seg_check.c -- the SRTCP rule composed per session
 * (re_amd/csrc/hip/plan_rtcp_seg.h, compiled as C) in the decomposition of
 * k_bpr_plan (plan_buckets_rtcp.hip), against a sequential restatement of
 * stream_get (stream.c:29-84), the sender's index (srtcp.c:54) and the
 * receiver's replay check (srtcp.c:208-209, replay.c:32-62) written here.
 *
 * A batch interleaves 2-40 sessions with 0-8 known streams each: known and
 * new SSRCs, 9th SSRCs, indices that wrap at 0x7fffffff, replayed and
 * swapped indices, streams that start below their window's top on a set or
 * an unset bit.  It runs
 *
 *   (a) as the kernel does: sessions cut into buckets of 2^bshift ids with
 *       `cap` entries each, a bucket's entries in an arbitrary order (the
 *       scatter's atomics), grouped by session, ranked by packet index, then
 *       the passes of k_bpr_plan with `T` "threads" striding over the sorted
 *       positions (visited from the last thread down, so a pass that read
 *       what the same pass writes would show), small bshift / cap / segmax /
 *       T so that every boundary is met;
 *   (b) packet by packet through the sequential restatement.
 *
 * An accepted plan must equal (b) packet for packet and state for state;
 * and (a) must accept whenever (b) returns 0 everywhere, every stream's
 * indices increase and lie above its stored lix (apart from a first packet
 * on an unset bit), no session passes 8 streams and the buckets hold the
 * batch -- so rejecting everything does not pass.
 *
 *   gcc -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -o rtcp_seg_check tests/c/rtcp_seg_check.c && ./rtcp_seg_check
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../re_amd/csrc/hip/plan_rtcp_seg.h"

#define NMAX 600
#define SMAX 40
#define TAG 10u

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

static uint32_t g_rng = 0x9e3779b9u;

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
	uint32_t sess, ssrc, word;
};

struct batch {
	int prot, hmac;
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
	memset(&t->st[t->n], 0, sizeof(t->st[0]));
	t->st[t->n].ssrc = ssrc;
	*sp = &t->st[t->n++];
	return 0;
}

static void sequential(const struct batch *B, struct tab *t, int *err,
		       uint32_t *ix)
{
	uint32_t i;
	memcpy(t, B->t0, sizeof(B->t0));
	for (i = 0; i < B->n; i++) {
		const struct pkt *p = &B->p[i];
		struct rseg_rec *st;
		err[i] = ref_stream_get(&t[p->sess], p->ssrc, &st);
		ix[i] = 0;
		if (err[i])
			continue;
		if (B->prot) {
			st->ix = (st->ix + 1) & 0x7fffffffu;    /* srtcp.c:54 */
			ix[i] = st->ix;
			continue;
		}
		ix[i] = p->word & 0x7fffffffu;
		if (B->hmac) {
			uint64_t lix = st->ix;
			uint64_t bm = (uint64_t)st->bhi << 32 | st->blo;
			if (!ref_replay_check(&lix, &bm, ix[i])) {
				err[i] = EALREADY;
				continue;
			}
			st->ix = (uint32_t)lix;
			st->blo = (uint32_t)bm;
			st->bhi = (uint32_t)(bm >> 32);
		}
	}
}

/* ---- (a) the kernel's decomposition ----------------------------------- */

struct geo {
	uint32_t bshift, cap, segmax, T;
};

/* 0 accepted (ix[], t[]: the plan), else the SPF_* bits */
static uint32_t planned(const struct batch *B, struct geo G, struct tab *t,
			uint32_t *ix)
{
	const uint32_t nsb = 1u << G.bshift;
	const uint32_t nb = (B->nsess + nsb - 1) >> G.bshift;
	struct sgpu_rplan_in in;
	uint32_t fail = 0, b, i;

	memset(&in, 0, sizeof(in));
	in.n = B->n;
	in.prot = (uint32_t)B->prot;
	in.tag = B->hmac ? TAG : 0;
	in.gcm = !B->hmac;
	in.hmac = (uint32_t)B->hmac;
	in.encrypted = 1;
	memcpy(t, B->t0, sizeof(B->t0));
	for (b = 0; b < nb; b++) {
		const uint32_t s0 = b << G.bshift;
		const uint32_t ns = B->nsess - s0 < nsb ? B->nsess - s0 : nsb;
		/* the bucket's entries in an arbitrary order */
		static uint32_t ent[NMAX], gidx[NMAX], idx[NMAX], ru[NMAX];
		static uint32_t kn[NMAX], sl[NMAX];
		static struct rseg_look lk[NMAX];
		static uint8_t opens[NMAX];
		uint32_t cnt[SMAX], start[SMAX], nk[SMAX], nst[SMAX];
		uint32_t tmask[SMAX], acc[SMAX][RSEG_MAX];
		uint64_t bits[SMAX][RSEG_MAX];
		struct rseg_rec rec[SMAX][RSEG_MAX];
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
			uint32_t q;
			l = p->sess - s0;
			kn[k] = rseg_known(rec[l], nk[l], p->ssrc);
			lk[k] = rseg_look_init(k);
			for (q = start[l]; q < k; q++)
				lk[k] = rseg_look_step(lk[k], q,
					B->p[idx[q]].ssrc == p->ssrc);
			opens[k] = (uint8_t)rseg_opens(kn[k], lk[k]);
		}
		/* pass 2: the slot, new records, counts / largest indices */
		EACH_POSITION {
			const struct pkt *p = &B->p[idx[k]];
			uint32_t nnew = 0, slot, q, v;
			l = p->sess - s0;
			sl[k] = RSEG_NONE;
			if (kn[k] == RSEG_NONE)
				for (q = start[l]; q < lk[k].first; q++)
					nnew += opens[q];
			slot = rseg_slot(kn[k], nk[l], nnew);
			if (rseg_enosr(slot)) {
				f |= SPF_SSRC;
				continue;
			}
			sl[k] = slot;
			if (opens[k]) {
				const struct rseg_rec r = {p->ssrc, 0, 0, 0};
				rec[l][slot] = r;
				if (nst[l] < slot + 1)
					nst[l] = slot + 1;
			}
			tmask[l] |= 1u << slot;
			v = B->prot ? lk[k].rank + 1 : p->word & 0x7fffffffu;
			if (acc[l][slot] < v)
				acc[l][slot] = v;
		}
		/* pass 3: the rule, the window bit */
		EACH_POSITION {
			const struct pkt *p = &B->p[idx[k]];
			struct plan_rtcp r;
			if (sl[k] == RSEG_NONE)
				continue;
			l = p->sess - s0;
			r = rseg_packet(in, rec[l][sl[k]], lk[k].rank, 1, 200, 0,
					p->word, lk[k].rank ?
					B->p[idx[lk[k].prev]].word : 0);
			f |= r.flags;
			ix[idx[k]] = r.ix;
			if (!B->prot && B->hmac)
				bits[l][sl[k]] |= rseg_bit(
					rseg_top(rec[l][sl[k]].ix, acc[l][sl[k]]),
					r.ix);
		}
#undef EACH_POSITION
		if (f) {
			fail |= f;
			continue;
		}
		/* the touched sessions' tables after the batch */
		for (l = 0; l < ns; l++) {
			uint32_t x;
			if (!tmask[l])
				continue;
			t[s0 + l].n = nst[l];
			for (x = 0; x < nst[l]; x++) {
				struct rseg_rec o = rec[l][x];
				if (!(tmask[l] >> x & 1u)) {
					t[s0 + l].st[x] = o;
					continue;
				}
				if (B->prot) {
					o.ix = rseg_index_after(o.ix, acc[l][x]);
				}
				else if (B->hmac) {
					const struct plan_win w = rseg_window_after(
						o, rseg_top(o.ix, acc[l][x]),
						bits[l][x]);
					o.ix = (uint32_t)w.lix;
					o.blo = (uint32_t)w.bitmap;
					o.bhi = (uint32_t)(w.bitmap >> 32);
				}
				t[s0 + l].st[x] = o;
			}
		}
	}
	return fail;
}

/* ---- batches ---------------------------------------------------------- */

static uint32_t ssrc_of(uint32_t s, uint32_t k)
{
	return 0x51000000u | s << 8 | k;
}

/* what the generator did on purpose */
enum { TR_NINTH = 1, TR_REPLAY = 2, TR_SWAP = 4, TR_BELOW_SET = 8 };

static uint32_t make_batch(struct batch *B, int mode, uint32_t trouble_pm)
{
	/* the sender's next index per (session, stream) */
	static uint32_t nxt[SMAX][RSEG_MAX + 4];
	uint32_t done = 0, s, k, i;

	memset(B, 0, sizeof(*B));
	B->prot = mode == 0;
	B->hmac = mode != 2;
	B->nsess = 2 + rnd() % (SMAX - 1);
	B->n = 1 + rnd() % NMAX;
	for (s = 0; s < B->nsess; s++) {
		struct tab *t = &B->t0[s];
		t->n = rnd() % (RSEG_MAX + 1);
		for (k = 0; k < RSEG_MAX + 4; k++)
			nxt[s][k] = 1;
		for (k = 0; k < t->n; k++) {
			struct rseg_rec *r = &t->st[k];
			const uint32_t at = chance(B->prot ? 150 : 4) ?
					    0x7fffffffu - rnd() % 40
					  : chance(300) ? rnd() % 100
							: rnd() & 0x3fffffffu;
			r->ssrc = ssrc_of(s, k);
			if (B->prot) {
				r->ix = at;
			}
			else if (B->hmac) {
				r->ix = at;
				r->blo = rnd() << 8 | rnd() | 1u;
				r->bhi = rnd() << 8 | rnd();
				nxt[s][k] = at + 1;
			}
		}
	}
	for (i = 0; i < B->n; i++) {
		struct pkt *p = &B->p[i];
		uint32_t nss;
		s = rnd() % B->nsess;
		/* mostly streams the table can hold; sometimes one more */
		nss = RSEG_MAX;
		if (chance(trouble_pm / 4)) {
			nss = RSEG_MAX + 4;
			done |= TR_NINTH;       /* (maybe: the check asks (b)) */
		}
		k = chance(600) ? rnd() % (B->t0[s].n + 1) : rnd() % nss;
		if (k >= nss)
			k = nss - 1;
		p->sess = s;
		p->ssrc = ssrc_of(s, k);
		if (B->prot)
			continue;
		if (nxt[s][k] > 0x7fffffffu)
			nxt[s][k] = 0x7fffffffu;        /* (a replay then) */
		p->word = 0x80000000u | nxt[s][k];
		nxt[s][k] += 1 + (chance(200) ? rnd() % 70 : 0);
	}
	if (B->prot || !B->hmac)
		return done;
	/* the receiver's troubles */
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
			B->p[j].word = B->p[i].word;
			done |= TR_REPLAY;
		}
		else {
			const uint32_t w = B->p[i].word;
			B->p[i].word = B->p[j].word;
			B->p[j].word = w;
			done |= TR_SWAP;
		}
	}
	/* a stream that starts below its window's top */
	for (s = 0; s < B->nsess; s++)
		for (k = 0; k < B->t0[s].n; k++) {
			struct rseg_rec *r = &B->t0[s].st[k];
			uint32_t d;
			if (!chance(12) || r->ix < 64)
				continue;
			for (i = 0; i < B->n; i++)
				if (B->p[i].sess == s && B->p[i].ssrc == r->ssrc)
					break;
			if (i == B->n)
				continue;
			d = rnd() % 64;
			B->p[i].word = 0x80000000u | (r->ix - d);
			if (chance(700)) {
				const uint64_t bm = ((uint64_t)r->bhi << 32 |
						     r->blo) & ~(1ull << d);
				r->blo = (uint32_t)bm;
				r->bhi = (uint32_t)(bm >> 32);
			}
			else if (((uint64_t)r->bhi << 32 | r->blo) >> d & 1u) {
				done |= TR_BELOW_SET;
			}
		}
	return done;
}

/* the condition under which a plan must be accepted: (b) returns 0
 * everywhere, every stream's indices increase and lie above its stored lix
 * apart from a first packet (on an unset bit: (b) accepted it), no session
 * passes 8 streams (no ENOSR), the buckets hold the batch */
static int must_accept(const struct batch *B, struct geo G, const int *err)
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
	if (B->prot || !B->hmac)
		return 1;
	for (i = 0; i < B->n; i++) {
		const struct pkt *p = &B->p[i];
		const struct tab *t = &B->t0[p->sess];
		const uint32_t ix = p->word & 0x7fffffffu;
		uint32_t lix = 0, k;
		int first = 1;
		for (k = 0; k < t->n; k++)
			if (t->st[k].ssrc == p->ssrc)
				lix = t->st[k].ix;
		for (j = i; j-- > 0;)
			if (B->p[j].sess == p->sess && B->p[j].ssrc == p->ssrc) {
				first = 0;
				if ((B->p[j].word & 0x7fffffffu) >= ix)
					return 0;
				break;
			}
		if (!first && ix <= lix)
			return 0;
	}
	return 1;
}

int main(void)
{
	static struct batch B;
	static struct tab ts[SMAX], tp[SMAX];
	static int err[NMAX];
	static uint32_t ixs[NMAX], ixp[NMAX];
	uint32_t it, naccept = 0, nreject = 0, nmust = 0, seen = 0;
	uint32_t nacc_mode[3] = {0, 0, 0};

	for (it = 0; it < 6000; it++) {
		const int mode = (int)(it % 3);         /* protect, HMAC, GCM */
		const struct geo G = {
			.bshift = rnd() % 4,
			.cap = chance(850) ? NMAX : 16 + rnd() % 200,
			.segmax = chance(850) ? NMAX : 8 + rnd() % 64,
			.T = 1 + rnd() % 70};
		const uint32_t tr = make_batch(&B, mode, it % 2 ? 400 : 0);
		uint32_t fail, i, s, k;
		int must;

		sequential(&B, ts, err, ixs);
		memset(ixp, 0, sizeof(ixp));
		fail = planned(&B, G, tp, ixp);
		must = must_accept(&B, G, err);
		nmust += (uint32_t)must;
		seen |= tr;
		CHECK(!(must && fail), "it %u mode %d: rejected (SPF %#x) a batch "
		      "it must accept", it, mode, fail);
		if (fail) {
			nreject++;
			continue;
		}
		naccept++;
		nacc_mode[mode]++;
		for (i = 0; i < B.n; i++) {
			CHECK(!err[i], "it %u mode %d: accepted, packet %u has "
			      "errno %d", it, mode, i, err[i]);
			CHECK(ixp[i] == ixs[i], "it %u mode %d: packet %u index "
			      "%#x, sequential %#x", it, mode, i, ixp[i], ixs[i]);
		}
		for (s = 0; s < B.nsess; s++) {
			CHECK(tp[s].n == ts[s].n, "it %u mode %d: session %u has "
			      "%u streams, sequential %u", it, mode, s, tp[s].n,
			      ts[s].n);
			for (k = 0; k < ts[s].n && k < tp[s].n; k++)
				CHECK(!memcmp(&tp[s].st[k], &ts[s].st[k],
					      sizeof(ts[s].st[k])),
				      "it %u mode %d: session %u stream %u "
				      "{%#x %#x %#x %#x}, sequential {%#x %#x "
				      "%#x %#x}", it, mode, s, k,
				      tp[s].st[k].ssrc, tp[s].st[k].ix,
				      tp[s].st[k].blo, tp[s].st[k].bhi,
				      ts[s].st[k].ssrc, ts[s].st[k].ix,
				      ts[s].st[k].blo, ts[s].st[k].bhi);
		}
	}
	/* the run met what it is about */
	CHECK(nacc_mode[0] > 300 && nacc_mode[1] > 300 && nacc_mode[2] > 300,
	      "accepted %u / %u / %u", nacc_mode[0], nacc_mode[1], nacc_mode[2]);
	CHECK(nreject > 300, "rejected %u", nreject);
	CHECK(nmust > 900, "must-accept batches %u", nmust);
	CHECK((seen & (TR_NINTH | TR_REPLAY | TR_SWAP | TR_BELOW_SET)) ==
	      (TR_NINTH | TR_REPLAY | TR_SWAP | TR_BELOW_SET), "seen %#x", seen);
	printf("%u batches: %u accepted (%u must), %u rejected, %d wrong\n", it,
	       naccept, nmust, nreject, g_bad);
	return g_bad ? 1 : 0;
}
