/*
 * plan_buckets_rtcp.hip -- SRTCP protect / unprotect batches over many
 * sessions with up to 8 SSRCs each, planned on the device in three launches
 * around the crypto (srtpgpu.h struct sgpu_bplan_rtcp; the rule per session
 * and why the final window needs no order: plan_rtcp_seg.h).
 *
 * The reference keeps one SRTCP state per (session, SSRC): the sender's
 * rtcp_index (srtcp_encrypt, srtcp.c:31-140), the receiver's replay window
 * (srtcp_decrypt, srtcp.c:143-287; replay.c:32-62), in a table stream_get
 * (stream.c:29-84) appends to in the order SSRCs first appear.  Sessions are
 * independent, so they are cut into buckets of 2^bshift consecutive ids as
 * plan_buckets.hip does, and every step of a session happens inside the one
 * workgroup that owns its bucket:
 *
 *   k_bpr_scatter  per packet: the RTCP parse (the SSRC into hdr word 0,
 *                  which rtcp_job reads), the window checks, the end copy,
 *                  unprotect: the E || index word in front of the tag, read
 *                  byte by byte (it lies at any alignment); its slot in its
 *                  bucket (LDS count per workgroup, one global atomic per
 *                  (workgroup, bucket) for the base)
 *   k_bpr_plan     per bucket, in LDS: the sessions' stream tables, the
 *                  entries grouped by session and ranked by packet index,
 *                  then per packet the look back over its session's segment
 *                  (rank in its stream, predecessor, first appearance), its
 *                  slot (new SSRCs behind the known ones in first-appearance
 *                  order; a 9th: SPF_SSRC), the rule, desc, and per touched
 *                  session the table after the batch
 *   (the compact crypto kernels with per-packet keys, guarded by out->fail)
 *   k_bpr_finish   end / err per packet only if the plan held and every tag
 *                  verified; the bucket counters back to zero; the plan out
 *                  to its pinned mirror
 *
 * No workgroup waits for another.  Any failed check rejects the whole plan:
 * nothing of the caller's is modified and the host plans.  k_bpr_plan's front
 * (entries, table words, grouping and rank), pass 2's slot and the finish tail
 * are plan_bucket_common.h's; pass 1 keeps the records in LDS and is its own.
 */
#include "plan_bucket_common.h"

static_assert(RSEG_MAX == 8, "sinfo holds 8 touched bits");

__device__ __forceinline__ uint32_t bpr_be32(const uint8_t *q)
{
	return (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 |
	       (uint32_t)q[2] << 8 | q[3];
}

/* ---- 1: parse, checks, bucket scatter --------------------------------- */

__global__ void __launch_bounds__(BPB)
k_bpr_scatter(const uint8_t *__restrict__ arena, uint64_t asz,
	      const struct sgpu_bplan_rtcp P)
{
	__shared__ uint32_t hist[SGPU_BP_NBMAX], base[SGPU_BP_NBMAX];
	__shared__ uint32_t bf;
	const uint32_t tid = threadIdx.x, nb = P.nb;
	const struct sgpu_rplan_in &in = P.in;
	for (uint32_t k = tid; k < nb; k += BPB)
		hist[k] = 0;
	if (tid == 0) {
		bf = 0;
		if (blockIdx.x == 0) {
			/* the call's outs: nothing else writes them before the
			 * plan kernel (the crypto launch's miss counter too);
			 * SRTCP's cipher region starts at byte 8: class 2 */
			*P.nfail = 0;
			P.out->fail = 0;
			P.out->wraps = 0;
			P.out->ssrc0 = 0;
			P.out->hl0 = 8;
			P.out->s_l_last = 0;
			P.out->nfail = 0;
			for (uint32_t q = 0; q < 4; q++)
				P.out->skip[q] = q != 2u;
		}
	}
	uint32_t bk[SGPU_BP_PPT], rk[SGPU_BP_PPT];
	uint32_t wy[SGPU_BP_PPT], wz[SGPU_BP_PPT], ww[SGPU_BP_PPT];
	uint32_t pv[SGPU_BP_PPT], ev[SGPU_BP_PPT], cv[SGPU_BP_PPT];
	uint32_t sv[SGPU_BP_PPT];
	uint32_t f = 0;
	const uint32_t i0 = blockIdx.x * (BPB * SGPU_BP_PPT) + tid;
#pragma unroll
	for (int j = 0; j < SGPU_BP_PPT; j++) {
		const uint32_t i = i0 + j * BPB;
		pv[j] = ev[j] = cv[j] = sv[j] = 0;
		if (i < in.n) {
			pv[j] = P.pos[i];
			ev[j] = P.end[i];
			cv[j] = P.capv ? P.capv[i] : 0u;
			sv[j] = P.sess[i];
		}
	}
	__syncthreads();
#pragma unroll
	for (int j = 0; j < SGPU_BP_PPT; j++) {
		const uint32_t i = i0 + j * BPB;
		bk[j] = 0xffffffffu;
		rk[j] = wy[j] = wz[j] = ww[j] = 0;
		if (i >= in.n)
			continue;
		const uint32_t p = pv[j], e = ev[j], c = cv[j];
		uint32_t s = sv[j];
		P.es[i] = e;
		/* a window outside the arena is never read */
		const uint32_t left = (e > p && e <= asz) ? e - p : 0u;
		const int parsed = left >= 8u;
		struct sgpu_hdr h;
		h.ssrc = 0;
		h.seq = 0;
		h.err_pos = 0;
		h.hdr_len = PLAN_NOHDR;
		if (parsed) {
			/* get_rtcp_ssrc (srtcp.c:19-28) */
			h.ssrc = (p & 3u) ? bpr_be32(arena + p + 4)
					  : __builtin_bswap32(*(const uint32_t *)
							      (arena + p + 4));
			h.hdr_len = 8;
		}
		P.hdr[i] = h;
		f |= plan_window_flags(p, e, P.capv != NULL, c, asz, in.maxlen,
				       in.need, (int)in.prot);
		if (s >= P.nsess) {
			f |= SPF_BAD;
			s = P.nsess - 1u;
		}
		/* unprotect: E || index in front of the tag -- with the 80-bit
		 * tag 2 bytes off a word boundary, and lengths are no multiples
		 * of 4: byte loads, only where the packet has room for it (the
		 * rule flags the others from their length) */
		if (!in.prot &&
		    left >= 8u + 4u + in.tag + (in.gcm ? 16u : 0u))
			ww[j] = bpr_be32(arena + e - 4u - in.tag);
		const uint32_t L = e >= p ? e - p : 0u;
		bk[j] = s >> P.bshift;
		rk[j] = atomicAdd(&hist[bk[j]], 1u);
		wy[j] = (s - (bk[j] << P.bshift)) | (parsed ? 0x100u : 0u) |
			(L < 0xffffu ? L : 0xffffu) << 16;
		wz[j] = h.ssrc;
	}
	__syncthreads();
	for (uint32_t k = tid; k < nb; k += BPB)
		base[k] = hist[k] ? atomicAdd(&P.bcount[k], hist[k]) : 0u;
	__syncthreads();
#pragma unroll
	for (int j = 0; j < SGPU_BP_PPT; j++) {
		if (bk[j] == 0xffffffffu)
			continue;
		const uint32_t slot = base[bk[j]] + rk[j];
		if (slot < P.cap)
			P.tmp[(size_t)bk[j] * P.cap + slot] =
				make_uint4(i0 + j * BPB, wy[j], wz[j], ww[j]);
		else
			f |= SPF_SEG;   /* the bucket overflows */
	}
	if (f)
		atomicOr(&bf, f);
	__syncthreads();
	if (tid == 0)
		P.afail[blockIdx.x] = bf;
}

/* ---- 2: per bucket, the plan ------------------------------------------ */

/*
 * The bucket in LDS.  The entries are written once in (session, packet
 * index) order, so a look back reads consecutive words; a thread keeps what
 * it learnt about its own (at most BK_EPT) positions in registers between
 * the passes.
 */
struct BprLds {
	uint32_t gidx[SGPU_BP_CAPMAX];  /* packet index, grouped by session */
	uint32_t idx[SGPU_BP_CAPMAX];   /* sorted position k: packet index, */
	uint32_t ssrc[SGPU_BP_CAPMAX];  /* SSRC, */
	uint32_t word[SGPU_BP_CAPMAX];  /* E || index, */
	uint32_t meta[SGPU_BP_CAPMAX];  /* session | parsed << 8 | L << 16 */
	uint8_t opens[SGPU_BP_CAPMAX];  /* it opens a new stream */
	struct rseg_rec rec[SGPU_BP_NSB][RSEG_MAX];
	uint32_t acc[SGPU_BP_NSB][RSEG_MAX];    /* protect: the stream's packets;
						   unprotect: its largest index */
	uint32_t wlo[SGPU_BP_NSB][RSEG_MAX];    /* the packets' window bits */
	uint32_t whi[SGPU_BP_NSB][RSEG_MAX];
	uint32_t cnt[SGPU_BP_NSB], start[SGPU_BP_NSB];
	uint32_t nk[SGPU_BP_NSB];       /* streams before the batch */
	uint32_t nst[SGPU_BP_NSB];      /* ... and after */
	uint32_t tmask[SGPU_BP_NSB];    /* streams with packets */
	uint32_t bf;
};

__global__ void __launch_bounds__(BPB)
k_bpr_plan(const struct sgpu_bplan_rtcp P)
{
	__shared__ BprLds S;
	const struct sgpu_rplan_in &in = P.in;
	const uint32_t tid = threadIdx.x, b = blockIdx.x;
	const uint32_t s0 = b << P.bshift;
	const uint32_t ns = min(1u << P.bshift, P.nsess - s0);
	uint4 ev4[BK_EPT];
	uint32_t m;
	uint32_t f = bk_entries(P.afail, in.n, P.nb, P.bcount, P.tmp, P.cap, &m,
				ev4);
	if (tid == 0)
		S.bf = 0;
	f |= bk_tables(P.toff, s0, ns, NULL, S.nk, S.nst, S.cnt, S.tmask,
		       &S.acc[0][0], &S.wlo[0][0], &S.whi[0][0]);
	__syncthreads();
	/* the sessions' tables, one record per thread */
	for (uint32_t q = tid; q < ns * RSEG_MAX; q += BPB) {
		const uint32_t l = q / RSEG_MAX, x = q % RSEG_MAX;
		struct rseg_rec r = {0, 0, 0, 0};
		if (x < S.nk[l])
			r = bk_ld(P.recs + P.toff[s0 + l] + x);
		S.rec[l][x] = r;
	}
	/* by (session, packet index): the order the reference sees them in */
	uint32_t pos[BK_EPT];
	const bool dead = bk_sort(ev4, 0, m, ns, f, S.cnt, S.start, S.gidx, &S.bf,
				  pos);
	f = 0;
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		if (dead || tid + j * BPB >= m)
			continue;
		S.idx[pos[j]] = ev4[j].x;
		S.meta[pos[j]] = ev4[j].y;
		S.ssrc[pos[j]] = ev4[j].z;
		S.word[pos[j]] = ev4[j].w;
	}
	__syncthreads();
	/* pass 1, per sorted position: the known slot, the look back */
	uint32_t kn[BK_EPT];
	struct rseg_look lk[BK_EPT];
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		kn[j] = RSEG_NONE;
		lk[j] = rseg_look_init(k);
		if (dead || k >= m)
			continue;
		const uint32_t l = S.meta[k] & 0xffu, x = S.ssrc[k];
		kn[j] = rseg_known(S.rec[l], S.nk[l], x);
		for (uint32_t t = S.start[l]; t < k; t++)
			lk[j] = rseg_look_step(lk[j], t, S.ssrc[t] == x);
		S.opens[k] = (uint8_t)rseg_opens(kn[j], lk[j]);
	}
	__syncthreads();
	/* pass 2: the slot; a new stream's record; the stream's packet count
	 * (protect) or largest index (unprotect) */
	uint32_t sl[BK_EPT];
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		sl[j] = RSEG_NONE;
		if (dead || k >= m)
			continue;
		const uint32_t l = S.meta[k] & 0xffu;
		const uint32_t slot = bk_slot(kn[j], lk[j].first, S.start[l],
					      S.nk[l], S.opens);
		if (rseg_enosr(slot)) {
			f |= SPF_SSRC;  /* a 9th stream: ENOSR on the host */
			continue;
		}
		sl[j] = slot;
		if (S.opens[k]) {
			const struct rseg_rec r = {S.ssrc[k], 0, 0, 0};
			S.rec[l][slot] = r;
		}
		bk_touch(l, slot, S.opens[k],
			 in.prot ? lk[j].rank + 1u : S.word[k] & 0x7fffffffu,
			 S.nst, S.tmask, &S.acc[l][slot]);
	}
	__syncthreads();
	/* pass 3: the rule, desc, the window bit */
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		if (dead || k >= m || sl[j] == RSEG_NONE)
			continue;
		const uint32_t mt = S.meta[k], l = mt & 0xffu;
		const struct rseg_rec st = S.rec[l][sl[j]];
		const uint32_t pword = lk[j].rank ? S.word[lk[j].prev] : 0u;
		const struct plan_rtcp r =
			rseg_packet(in, st, lk[j].rank, (int)(mt >> 8 & 1u),
				    mt >> 16, 0, S.word[k], pword);
		f |= r.flags;
		P.desc[S.idx[k]] = plan_rtcp_desc(r.ix, r.E);
		if (!in.prot && in.hmac) {
			const uint64_t bit =
				rseg_bit(rseg_top(st.ix, S.acc[l][sl[j]]), r.ix);
			if ((uint32_t)bit)
				atomicOr(&S.wlo[l][sl[j]], (uint32_t)bit);
			if ((uint32_t)(bit >> 32))
				atomicOr(&S.whi[l][sl[j]], (uint32_t)(bit >> 32));
		}
	}
	if (f)
		atomicOr(&S.bf, f);
	__syncthreads();
	const bool held = S.bf == 0;
	/* every touched session's table after the batch */
	for (uint32_t q = tid; q < ns * RSEG_MAX; q += BPB) {
		const uint32_t l = q / RSEG_MAX, x = q % RSEG_MAX;
		if (!held || !S.tmask[l] || x >= S.nst[l])
			continue;
		struct rseg_rec o = S.rec[l][x];
		if (S.tmask[l] >> x & 1u) {
			if (in.prot) {
				o.ix = rseg_index_after(o.ix, S.acc[l][x]);
			}
			else if (in.hmac) {
				const struct plan_win w = rseg_window_after(
					o, rseg_top(o.ix, S.acc[l][x]),
					(uint64_t)S.whi[l][x] << 32 | S.wlo[l][x]);
				o.ix = (uint32_t)w.lix;
				o.blo = (uint32_t)w.bitmap;
				o.bhi = (uint32_t)(w.bitmap >> 32);
			}
		}
		*(uint4 *)(P.sout + (size_t)(s0 + l) * RSEG_MAX + x) =
			make_uint4(o.ssrc, o.ix, o.blo, o.bhi);
	}
	if (tid < ns)
		P.sinfo[s0 + tid] = held && S.tmask[tid] ?
				    S.nst[tid] | S.tmask[tid] << 8 : 0u;
	if (tid == 0 && !held)
		atomicOr(&P.out->fail, S.bf);
}

/* ---- 3: results, counters, the plan out ------------------------------- */

__global__ void __launch_bounds__(BPB)
k_bpr_finish(const struct sgpu_bplan_rtcp P)
{
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
			if (i >= P.in.n)
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
	/* the call's outcome: the miss count next to the plan out, all of it
	 * to the pinned mirror with vector stores (out->fail is final: the
	 * plan kernel completed before the crypto launches) */
	if (tid == 0)
		P.out->nfail = nf;
	bk_post(P.out, P.outh, P.outbytes,
		offsetof(struct sgpu_plan_out, nfail) / 4u, nf);
}

/* ---- host side ------------------------------------------------------ */

static int bpr_check(const struct sgpu_bplan_rtcp *r)
{
	if (bk_geom_bad(r->in.n, r->nsess, r->nb, r->bshift, r->cap) ||
	    !r->pos || !r->end || !r->sess || !r->endw || !r->err || !r->es ||
	    !r->hdr || !r->desc || !r->tmp || !r->bcount || !r->afail ||
	    !r->toff || !r->recs || !r->sout || !r->sinfo || !r->out ||
	    !r->nfail || r->outbytes % 4u ||
	    r->outbytes > sizeof(struct sgpu_plan_out))
		return EINVAL;
	return 0;
}

extern "C" int sgpu_bplan_rtcp_scatter(const uint8_t *arena,
				       uint64_t arena_size,
				       const struct sgpu_bplan_rtcp *r,
				       void *stream)
{
	if (bpr_check(r))
		return EINVAL;
	hipLaunchKernelGGL(k_bpr_scatter, dim3(bk_grid(r->in.n)), dim3(BPB), 0,
			   (hipStream_t)stream, arena, arena_size, *r);
	return bk_err("k_bpr_scatter");
}

extern "C" int sgpu_bplan_rtcp_plan(const struct sgpu_bplan_rtcp *r,
				    void *stream)
{
	if (bpr_check(r))
		return EINVAL;
	hipLaunchKernelGGL(k_bpr_plan, dim3(r->nb), dim3(BPB), 0,
			   (hipStream_t)stream, *r);
	return bk_err("k_bpr_plan");
}

extern "C" int sgpu_bplan_rtcp_finish(const struct sgpu_bplan_rtcp *r,
				      void *stream)
{
	if (bpr_check(r))
		return EINVAL;
	hipLaunchKernelGGL(k_bpr_finish, dim3(r->nb + bk_grid(r->in.n)),
			   dim3(BPB), 0, (hipStream_t)stream, *r);
	return bk_err("k_bpr_finish");
}
