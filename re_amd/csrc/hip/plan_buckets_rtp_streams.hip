/*
 * plan_buckets_rtp_streams.hip -- RTP protect / unprotect batches over many
 * sessions with up to 8 SSRCs each, every stream in order, planned on the
 * device behind the bucket planner (srtpgpu.h struct sgpu_bplan_rtps; the
 * rule per (session, SSRC): plan_rtp_seg.h).
 *
 * plan_buckets.hip takes sessions of one stream: its k_bp_plan rejects a
 * session whose packets carry two SSRCs, and its gather a session whose
 * table holds two.  The reference keeps one RTP state per (session, SSRC)
 * (stream_get_seq, stream.c:29-109; srtp_encrypt / srtp_decrypt,
 * srtp.c:183-432), in a table stream_get appends to in the order SSRCs first
 * appear, so a bundled session is a few independent in-order streams behind
 * one key.  Sessions are cut into buckets as plan_buckets.hip does, and:
 *
 *   k_bp_scatter  (plan_buckets.hip, launched again unchanged) per packet:
 *                 parse, window and header checks, the end copy, its entry
 *                 -- index, seq, session in bucket, SSRC -- into its bucket
 *   k_bps_plan    per bucket, in LDS: the sessions' stream tables, the
 *                 entries grouped by session and ranked by packet index,
 *                 then per packet the look back over its session's segment:
 *                 as k_bpr_plan its rank in its stream and first appearance
 *                 (new SSRCs take the slots behind the known ones in
 *                 first-appearance order; a 9th: SPF_SSRC), and in the same
 *                 walk its predecessor's seq, the s_l that one saw and the
 *                 stream's rollovers so far -- the one-stream rule needs no
 *                 more, so there is no second grouping by stream and no scan;
 *                 the rule, desc, the stream's last packet its window's top,
 *                 every packet its window bit, and per touched session the
 *                 table after the batch
 *   (the general crypto kernels in array order with per-packet keys, guarded
 *   by skip[] / fail)
 *   k_bps_finish  end / err per packet only if the plan held and every tag
 *                 verified; the bucket and bin counters back to zero; the
 *                 plan out to its pinned mirror
 *
 * No workgroup waits for another.  Any failed check rejects the whole plan:
 * nothing of the caller's is modified and the host plans.  k_bps_plan's front
 * (entries, table words, grouping and rank), pass 2's slot and the finish tail
 * are plan_bucket_common.h's; pass 1's step carries the seq and is its own.
 */
#include "plan_bucket_common.h"

static_assert(RSEG_MAX == 8, "sinfo holds 8 touched bits");

/* ---- per bucket, the plan --------------------------------------------- */

/*
 * The bucket in LDS (157 KiB of the CU's 160).  The entries are written
 * once in (session, packet index) order, so a look back reads consecutive
 * words, every lane of a session the same ones; a thread keeps what it
 * learnt about its own (at most BK_EPT) positions in registers between the
 * passes.  The windows' tops take the place of the grouping's scratch, which
 * is dead once the entries are ranked.
 */
struct BpsLds {
	union {
		uint32_t gidx[SGPU_BP_CAPMAX];  /* packet index, grouped by
						   session */
		uint64_t top[SGPU_BP_NSB][RSEG_MAX];    /* unprotect: lix after */
	} u;
	uint32_t idx[SGPU_BP_CAPMAX];   /* sorted position k: packet index, */
	uint32_t ssrc[SGPU_BP_CAPMAX];  /* SSRC, */
	uint16_t sq[SGPU_BP_CAPMAX];    /* seq, */
	uint8_t sl[SGPU_BP_CAPMAX];     /* session in bucket */
	uint8_t opens[SGPU_BP_CAPMAX];  /* it opens a new stream */
	struct tseg_rec rec[SGPU_BP_NSB][RSEG_MAX];
	uint32_t acc[SGPU_BP_NSB][RSEG_MAX];    /* the stream's packets */
	uint32_t wlo[SGPU_BP_NSB][RSEG_MAX];    /* the packets' window bits */
	uint32_t whi[SGPU_BP_NSB][RSEG_MAX];
	uint32_t cnt[SGPU_BP_NSB], start[SGPU_BP_NSB];
	uint32_t nk[SGPU_BP_NSB];       /* streams before the batch */
	uint32_t nst[SGPU_BP_NSB];      /* ... and after */
	uint32_t tmask[SGPU_BP_NSB];    /* streams with packets */
	uint32_t bf;
};

static_assert(SGPU_BP_NSB * RSEG_MAX * sizeof(uint64_t) ==
	      SGPU_BP_CAPMAX * sizeof(uint32_t),
	      "the tops fit the grouping's scratch");

__global__ void __launch_bounds__(BPB)
k_bps_plan(const struct sgpu_bplan_rtps R)
{
	__shared__ BpsLds S;
	const struct sgpu_bplan &P = R.b;
	const int prot = (int)P.prot;
	const uint32_t tid = threadIdx.x, b = blockIdx.x;
	const uint32_t s0 = b << P.bshift;
	const uint32_t ns = min(1u << P.bshift, P.nsess - s0);
	/* the bucket's entries: index | length bin << 26, seq | session in
	 * bucket << 16, SSRC, (place in the bin: not used) */
	uint4 ev4[BK_EPT];
	uint32_t m;
	uint32_t f = bk_entries(P.afail, P.n, P.nb, P.bcount, P.tmp, P.cap, &m,
				ev4);
#pragma unroll
	for (int j = 0; j < BK_EPT; j++)
		ev4[j].x &= BP_IMASK;
	if (tid == 0)
		S.bf = 0;
	f |= bk_tables(R.toff, s0, ns, NULL, S.nk, S.nst, S.cnt, S.tmask,
		       &S.acc[0][0], &S.wlo[0][0], &S.whi[0][0]);
	__syncthreads();
	/* the sessions' tables, one record per thread */
	for (uint32_t q = tid; q < ns * RSEG_MAX; q += BPB) {
		const uint32_t l = q / RSEG_MAX, x = q % RSEG_MAX;
		struct tseg_rec r = {0, 0, 0, 0, 0, 0, 0, 0};
		if (x < S.nk[l])
			r = bk_ld(R.recs + R.toff[s0 + l] + x);
		S.rec[l][x] = r;
	}
	/* by (session, packet index): the order the reference sees them in */
	uint32_t pos[BK_EPT];
	const bool dead = bk_sort(ev4, 16, m, ns, f, S.cnt, S.start, S.u.gidx,
				  &S.bf, pos);
	f = 0;
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		if (dead || tid + j * BPB >= m)
			continue;
		S.idx[pos[j]] = ev4[j].x;
		S.sq[pos[j]] = (uint16_t)ev4[j].y;
		S.sl[pos[j]] = (uint8_t)bk_key(ev4[j], 16);
		S.ssrc[pos[j]] = ev4[j].z;
	}
	__syncthreads();
	/* pass 1, per sorted position: the known slot, the look back */
	uint32_t kn[BK_EPT];
	struct tseg_look lk[BK_EPT];
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		kn[j] = RSEG_NONE;
		lk[j] = tseg_look_init(k);
		if (dead || k >= m)
			continue;
		const uint32_t l = S.sl[k], x = S.ssrc[k];
		kn[j] = tseg_known(S.rec[l], S.nk[l], x);
		const uint32_t slw = kn[j] != RSEG_NONE ? S.rec[l][kn[j]].sl : 0u;
		for (uint32_t t = S.start[l]; t < k; t++) {
			const int same = S.ssrc[t] == x;
			lk[j] = tseg_look_step(lk[j], t, same,
					       same ? (uint32_t)S.sq[t] : 0u, slw);
		}
		S.opens[k] = (uint8_t)rseg_opens(kn[j], lk[j].a);
	}
	__syncthreads();
	/* pass 2: the slot; a new stream's record; the stream's packet count */
	uint32_t sl[BK_EPT];
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		sl[j] = RSEG_NONE;
		if (dead || k >= m)
			continue;
		const uint32_t l = S.sl[k];
		const uint32_t slot = bk_slot(kn[j], lk[j].a.first, S.start[l],
					      S.nk[l], S.opens);
		if (rseg_enosr(slot)) {
			f |= SPF_SSRC;  /* a 9th stream: ENOSR on the host */
			continue;
		}
		sl[j] = slot;
		if (S.opens[k]) {
			const struct tseg_rec r = {S.ssrc[k], 0, 0, 0, 0, 0, 0, 0};
			S.rec[l][slot] = r;
		}
		bk_touch(l, slot, S.opens[k], lk[j].a.rank + 1u, S.nst, S.tmask,
			 &S.acc[l][slot]);
	}
	__syncthreads();
	/* pass 3: the rule, desc; the stream's last packet: its window's top
	 * (u.gidx is dead: every thread passed the barriers behind the rank) */
	struct tseg_pkt pk[BK_EPT];
	uint32_t lastm = 0;
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		if (dead || k >= m || sl[j] == RSEG_NONE)
			continue;
		const uint32_t l = S.sl[k];
		const struct tseg_rec st = S.rec[l][sl[j]];
		pk[j] = tseg_packet(prot, st, lk[j], S.sq[k]);
		f |= pk[j].flags;
		P.desc[S.idx[k]] = d_desc(pk[j].ix, pk[j].fl);
		if (lk[j].a.rank + 1u == S.acc[l][sl[j]]) {
			lastm |= 1u << j;
			S.u.top[l][sl[j]] = tseg_top(tseg_lix(st), pk[j].ix);
		}
	}
	if (f)
		atomicOr(&S.bf, f);
	__syncthreads();
	/* pass 4 (unprotect): one window bit per packet within 64 of the top */
	if (!prot) {
#pragma unroll
		for (int j = 0; j < BK_EPT; j++) {
			const uint32_t k = tid + j * BPB;
			if (dead || k >= m || sl[j] == RSEG_NONE)
				continue;
			const uint32_t l = S.sl[k];
			const uint64_t bit = tseg_bit(S.u.top[l][sl[j]], pk[j].ix);
			if ((uint32_t)bit)
				atomicOr(&S.wlo[l][sl[j]], (uint32_t)bit);
			if ((uint32_t)(bit >> 32))
				atomicOr(&S.whi[l][sl[j]], (uint32_t)(bit >> 32));
		}
	}
	__syncthreads();
	const bool held = S.bf == 0;
	/* every touched session's table after the batch: a touched stream from
	 * its last packet, the others as they were */
	if (held) {
#pragma unroll
		for (int j = 0; j < BK_EPT; j++) {
			if (!(lastm >> j & 1u))
				continue;
			const uint32_t k = tid + j * BPB, l = S.sl[k];
			const uint64_t bits = (uint64_t)S.whi[l][sl[j]] << 32 |
					      S.wlo[l][sl[j]];
			bk_st(R.sout + (size_t)(s0 + l) * RSEG_MAX + sl[j],
			       tseg_after(prot, S.rec[l][sl[j]], pk[j], bits));
		}
		for (uint32_t q = tid; q < ns * RSEG_MAX; q += BPB) {
			const uint32_t l = q / RSEG_MAX, x = q % RSEG_MAX;
			if (!S.tmask[l] || x >= S.nst[l] || (S.tmask[l] >> x & 1u))
				continue;
			bk_st(R.sout + (size_t)(s0 + l) * RSEG_MAX + x,
			       S.rec[l][x]);
		}
	}
	if (tid < ns)
		R.sinfo[s0 + tid] = held && S.tmask[tid] ?
				    S.nst[tid] | S.tmask[tid] << 8 : 0u;
	if (!held) {
		/* a rejected plan closes the crypto launches' class guards (the
		 * scatter opened packet 0's class) */
		if (tid == 0)
			atomicOr(&P.out->fail, S.bf);
		if (tid < 4)
			P.out->skip[tid] = 1;
	}
}

/* ---- results, counters, the plan out ---------------------------------- */

__global__ void __launch_bounds__(BPB)
k_bps_finish(const struct sgpu_bplan_rtps R)
{
	const struct sgpu_bplan &P = R.b;
	const uint32_t tid = threadIdx.x;
	const uint32_t fail = P.out->fail;
	const uint32_t nf = *(volatile const uint32_t *)P.nfail;
	if (blockIdx.x >= P.nb) {
		/* per packet (coalesced): the caller's results */
		if (fail || nf)
			return;
		const uint32_t i0 = (blockIdx.x - P.nb) * (BPB * SGPU_BP_PPT);
#pragma unroll
		for (int j = 0; j < SGPU_BP_PPT; j++) {
			const uint32_t i = i0 + j * BPB + tid;
			if (i >= P.n)
				break;
			P.endw[i] = P.es[i] + (uint32_t)P.delta;
			P.err[i] = 0;
		}
		return;
	}
	/* the scatter's counters back to zero for the next call */
	if (tid == 0)
		P.bcount[blockIdx.x] = 0;
	if (blockIdx.x != 0)
		return;
	if (tid < BP_OBINS)
		P.obins[tid] = 0;
	/* the call's outcome: the miss count next to the plan out, all of it
	 * to the pinned mirror with vector stores (out->fail is final: the
	 * plan kernel completed before the crypto launches) */
	if (tid == 0)
		P.out->nfail = nf;
	bk_post(P.out, P.outh, P.outbytes,
		offsetof(struct sgpu_plan_out, nfail) / 4u, nf);
}

/* ---- host side ------------------------------------------------------ */

static int bps_check(const struct sgpu_bplan_rtps *r)
{
	const struct sgpu_bplan *b = &r->b;
	if (bk_geom_bad(b->n, b->nsess, b->nb, b->bshift, b->cap) ||
	    !b->endw || !b->err || !b->es || !b->desc || !b->tmp ||
	    !b->bcount || !b->obins || !b->afail || !b->out || !b->nfail ||
	    !r->toff || !r->recs || !r->sout || !r->sinfo ||
	    b->outbytes % 4u || b->outbytes > sizeof(struct sgpu_plan_out))
		return EINVAL;
	return 0;
}

extern "C" int sgpu_bplan_rtps_plan(const struct sgpu_bplan_rtps *r,
				    void *stream)
{
	if (bps_check(r))
		return EINVAL;
	hipLaunchKernelGGL(k_bps_plan, dim3(r->b.nb), dim3(BPB), 0,
			   (hipStream_t)stream, *r);
	return bk_err("k_bps_plan");
}

extern "C" int sgpu_bplan_rtps_finish(const struct sgpu_bplan_rtps *r,
				      void *stream)
{
	if (bps_check(r))
		return EINVAL;
	hipLaunchKernelGGL(k_bps_finish, dim3(r->b.nb + bk_grid(r->b.n)),
			   dim3(BPB), 0, (hipStream_t)stream, *r);
	return bk_err("k_bps_finish");
}
