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
 * nothing of the caller's is modified and the host plans.
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdio.h>
#include "../srtpgpu.h"
#include "plan_rtp_seg.h"

#define BPB SGPU_BP_BLOCK
#define BP_IMASK 0x3ffffffu     /* entry: packet index | length bin << 26 */
#define BP_OBINS 64
#define BPS_EPT (SGPU_BP_CAPMAX / BPB)  /* entries per thread, at most */

static_assert(sizeof(struct tseg_rec) == 32 &&
	      sizeof(struct sgpu_rtp_rec) == 32 &&
	      offsetof(struct sgpu_rtp_rec, llo) ==
	      offsetof(struct tseg_rec, llo),
	      "a stream record moves as two 16-byte words");
static_assert(RSEG_MAX == 8, "sinfo holds 8 touched bits");

__device__ __forceinline__ struct tseg_rec bps_ld(const struct sgpu_rtp_rec *p)
{
	const uint4 a = ((const uint4 *)p)[0], b = ((const uint4 *)p)[1];
	struct tseg_rec r;
	r.ssrc = a.x; r.roc = a.y; r.sl = a.z; r.pad = 0;
	r.llo = b.x; r.lhi = b.y; r.blo = b.z; r.bhi = b.w;
	return r;
}

__device__ __forceinline__ void bps_st(struct sgpu_rtp_rec *p,
				       const struct tseg_rec &r)
{
	((uint4 *)p)[0] = make_uint4(r.ssrc, r.roc, r.sl, 0u);
	((uint4 *)p)[1] = make_uint4(r.llo, r.lhi, r.blo, r.bhi);
}

/* ---- per bucket, the plan --------------------------------------------- */

/*
 * The bucket in LDS (157 KiB of the CU's 160).  The entries are written
 * once in (session, packet index) order, so a look back reads consecutive
 * words, every lane of a session the same ones; a thread keeps what it
 * learnt about its own (at most BPS_EPT) positions in registers between the
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
	uint32_t m = P.bcount[b];
	uint32_t f = 0;
	{
		/* the scatter workgroups' fail words, spread over the buckets
		 * (no workgroup waits for another) */
		const uint32_t na = (P.n + BPB * SGPU_BP_PPT - 1) /
				    (BPB * SGPU_BP_PPT);
		for (uint32_t k = b + tid * P.nb; k < na; k += BPB * P.nb)
			f |= P.afail[k];
	}
	if (m > P.cap) {
		f |= SPF_SEG;           /* (the scatter flagged it too) */
		m = 0;
	}
	/* the bucket's entries: index | length bin << 26, seq | session in
	 * bucket << 16, SSRC, (place in the bin: not used) */
	uint4 ev4[BPS_EPT];
#pragma unroll
	for (int j = 0; j < BPS_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		ev4[j] = k < m ? P.tmp[(size_t)b * P.cap + k]
			       : make_uint4(0, 0, 0, 0);
		ev4[j].x &= BP_IMASK;
	}
	if (tid == 0)
		S.bf = 0;
	if (tid < ns) {
		const uint32_t s = s0 + tid;
		const uint32_t t0 = R.toff[s], t1 = R.toff[s + 1];
		uint32_t nk = t1 - t0;
		if (t1 < t0 || nk > RSEG_MAX) {
			f |= SPF_BAD;   /* (the host builds toff: never) */
			nk = 0;
		}
		S.nk[tid] = nk;
		S.nst[tid] = nk;
		S.cnt[tid] = 0;
		S.tmask[tid] = 0;
	}
	for (uint32_t q = tid; q < SGPU_BP_NSB * RSEG_MAX; q += BPB) {
		(&S.acc[0][0])[q] = 0;
		(&S.wlo[0][0])[q] = 0;
		(&S.whi[0][0])[q] = 0;
	}
	__syncthreads();
	/* the sessions' tables, one record per thread */
	for (uint32_t q = tid; q < ns * RSEG_MAX; q += BPB) {
		const uint32_t l = q / RSEG_MAX, x = q % RSEG_MAX;
		struct tseg_rec r = {0, 0, 0, 0, 0, 0, 0, 0};
		if (x < S.nk[l])
			r = bps_ld(R.recs + R.toff[s0 + l] + x);
		S.rec[l][x] = r;
	}
	/* rank in session (unstable) */
	uint32_t ru[BPS_EPT];
#pragma unroll
	for (int j = 0; j < BPS_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		ru[j] = 0;
		if (k < m)
			ru[j] = atomicAdd(&S.cnt[ev4[j].y >> 16 & 0xffu], 1u);
	}
	__syncthreads();
	/* segment starts (sessions, <= 256: wave 0) */
	if (tid < 64) {
		uint32_t c4[4], v = 0;
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const uint32_t l = 4 * tid + q;
			c4[q] = l < ns ? S.cnt[l] : 0u;
			v += c4[q];
		}
		uint32_t x = v;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t y = (uint32_t)__shfl_up((int)x, d);
			if (tid >= (uint32_t)d)
				x += y;
		}
		uint32_t run = x - v;
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const uint32_t l = 4 * tid + q;
			if (l < SGPU_BP_NSB)
				S.start[l] = run;
			run += c4[q];
		}
	}
	if (tid < ns && S.cnt[tid] > SGPU_BP_SEGMAX)
		f |= SPF_SEG;
	if (f)
		atomicOr(&S.bf, f);
	f = 0;
	__syncthreads();
	const bool dead = S.bf != 0;    /* the plan fails: nothing more */
	if (!dead) {
		/* grouped by session */
#pragma unroll
		for (int j = 0; j < BPS_EPT; j++) {
			const uint32_t k = tid + j * BPB;
			if (k < m)
				S.u.gidx[S.start[ev4[j].y >> 16 & 0xffu] + ru[j]] =
					ev4[j].x;
		}
	}
	__syncthreads();
	if (!dead) {
		/* inside a session by packet index: the order the reference
		 * sees them in */
#pragma unroll
		for (int j = 0; j < BPS_EPT; j++) {
			const uint32_t k = tid + j * BPB;
			if (k >= m)
				continue;
			const uint32_t l = ev4[j].y >> 16 & 0xffu;
			const uint32_t f0 = S.start[l], c = S.cnt[l];
			uint32_t r = 0;
			for (uint32_t t = f0; t < f0 + c; t++)
				r += S.u.gidx[t] < ev4[j].x ? 1u : 0u;
			S.idx[f0 + r] = ev4[j].x;
			S.sq[f0 + r] = (uint16_t)ev4[j].y;
			S.sl[f0 + r] = (uint8_t)l;
			S.ssrc[f0 + r] = ev4[j].z;
		}
	}
	__syncthreads();
	/* pass 1, per sorted position: the known slot, the look back */
	uint32_t kn[BPS_EPT];
	struct tseg_look lk[BPS_EPT];
#pragma unroll
	for (int j = 0; j < BPS_EPT; j++) {
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
	uint32_t sl[BPS_EPT];
#pragma unroll
	for (int j = 0; j < BPS_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		sl[j] = RSEG_NONE;
		if (dead || k >= m)
			continue;
		const uint32_t l = S.sl[k];
		uint32_t nnew = 0;
		if (kn[j] == RSEG_NONE)
			for (uint32_t t = S.start[l]; t < lk[j].a.first; t++)
				nnew += S.opens[t];
		const uint32_t slot = rseg_slot(kn[j], S.nk[l], nnew);
		if (rseg_enosr(slot)) {
			f |= SPF_SSRC;  /* a 9th stream: ENOSR on the host */
			continue;
		}
		sl[j] = slot;
		if (S.opens[k]) {
			const struct tseg_rec r = {S.ssrc[k], 0, 0, 0, 0, 0, 0, 0};
			S.rec[l][slot] = r;
			atomicMax(&S.nst[l], slot + 1u);
		}
		atomicOr(&S.tmask[l], 1u << slot);
		atomicMax(&S.acc[l][slot], lk[j].a.rank + 1u);
	}
	__syncthreads();
	/* pass 3: the rule, desc; the stream's last packet: its window's top
	 * (u.gidx is dead: every thread passed the barriers behind the rank) */
	struct tseg_pkt pk[BPS_EPT];
	uint32_t lastm = 0;
#pragma unroll
	for (int j = 0; j < BPS_EPT; j++) {
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
		for (int j = 0; j < BPS_EPT; j++) {
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
		for (int j = 0; j < BPS_EPT; j++) {
			if (!(lastm >> j & 1u))
				continue;
			const uint32_t k = tid + j * BPB, l = S.sl[k];
			const uint64_t bits = (uint64_t)S.whi[l][sl[j]] << 32 |
					      S.wlo[l][sl[j]];
			bps_st(R.sout + (size_t)(s0 + l) * RSEG_MAX + sl[j],
			       tseg_after(prot, S.rec[l][sl[j]], pk[j], bits));
		}
		for (uint32_t q = tid; q < ns * RSEG_MAX; q += BPB) {
			const uint32_t l = q / RSEG_MAX, x = q % RSEG_MAX;
			if (!S.tmask[l] || x >= S.nst[l] || (S.tmask[l] >> x & 1u))
				continue;
			bps_st(R.sout + (size_t)(s0 + l) * RSEG_MAX + x,
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
	if (P.outh) {
		const uint32_t *src = (const uint32_t *)P.out;
		const uint32_t wn = offsetof(struct sgpu_plan_out, nfail) / 4u;
		for (uint32_t w = tid; w < P.outbytes / 4u; w += BPB)
			P.outh[w] = w == wn ? nf : src[w];
	}
}

/* ---- host side ------------------------------------------------------ */

static int bps_check(const struct sgpu_bplan_rtps *r)
{
	const struct sgpu_bplan *b = &r->b;
	if (!b->n || b->n > SGPU_BP_NMAX || b->nsess < 2 || !b->nb ||
	    b->nb > SGPU_BP_NBMAX || b->bshift > 8 || !b->cap ||
	    b->cap > SGPU_BP_CAPMAX || b->cap % BPB ||
	    ((uint64_t)b->nb << b->bshift) < b->nsess ||
	    ((uint64_t)(b->nb - 1) << b->bshift) >= b->nsess ||
	    !b->endw || !b->err || !b->es || !b->desc || !b->tmp ||
	    !b->bcount || !b->obins || !b->afail || !b->out || !b->nfail ||
	    !r->toff || !r->recs || !r->sout || !r->sinfo ||
	    b->outbytes % 4u || b->outbytes > sizeof(struct sgpu_plan_out))
		return EINVAL;
	return 0;
}

static int bps_err(const char *what)
{
	const hipError_t e = hipGetLastError();
	if (e == hipSuccess)
		return 0;
	fprintf(stderr, "re_srtp: %s launch: %s\n", what, hipGetErrorString(e));
	return EIO;
}

extern "C" int sgpu_bplan_rtps_plan(const struct sgpu_bplan_rtps *r,
				    void *stream)
{
	if (bps_check(r))
		return EINVAL;
	hipLaunchKernelGGL(k_bps_plan, dim3(r->b.nb), dim3(BPB), 0,
			   (hipStream_t)stream, *r);
	return bps_err("k_bps_plan");
}

extern "C" int sgpu_bplan_rtps_finish(const struct sgpu_bplan_rtps *r,
				      void *stream)
{
	if (bps_check(r))
		return EINVAL;
	const uint32_t g = (r->b.n + BPB * SGPU_BP_PPT - 1) /
			   (BPB * SGPU_BP_PPT);
	hipLaunchKernelGGL(k_bps_finish, dim3(r->b.nb + g), dim3(BPB), 0,
			   (hipStream_t)stream, *r);
	return bps_err("k_bps_finish");
}
