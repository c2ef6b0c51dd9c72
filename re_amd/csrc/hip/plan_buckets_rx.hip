/*
 * plan_buckets_rx.hip -- exact device plan of a many-session RTP unprotect
 * batch (one stream per session) whose packets arrive reordered, duplicated
 * or with gaps inside their sessions (srtpgpu.h struct sgpu_bplan_rx; the
 * rule and why it is exact: plan_rx_rule.h).
 *
 * The bucket planner (plan_buckets.hip k_bp_plan) speculates strict arrival
 * order per session and rejects such a batch with SPF_ORDER / SPF_REPLAY;
 * this one runs behind that rejection.  k_bp_scatter runs again unchanged
 * (k_bp_finish zeroed the bucket counters of the rejected plan; nothing of
 * its scratch is read), then
 *
 *   k_bp_rx_plan    per bucket, in LDS, as k_bp_plan: the sessions' resident
 *                   states (+ uploads), the entries grouped by session and
 *                   ranked by packet index inside each session; then the
 *                   receive rule per session segment: one segmented
 *                   (sum, max) scan over the sorted positions gives u[]
 *                   (speculated index) and Mx[] (maximum of the segment's
 *                   indices before it), rx_settle verifies every packet with
 *                   segment-local indices, desc / verdict byte per packet,
 *                   each touched session's state after the batch, the
 *                   bucket's late / duplicate counts.  An unsettled packet
 *                   or a failed check ORs the plan's fail word and closes
 *                   the crypto launches' class guards.
 *   (the general descriptor-driven crypto kernels, array order, guarded by
 *   skip[] / fail, counting their tag misses)
 *   k_bp_rx_finish  only if the plan held and every tag verified: pos / end
 *                   / err per packet (0 or EALREADY), the touched states into
 *                   the resident table; always: the scatter's counters back
 *                   to zero, the call's outcome to the pinned mirror.
 *
 * No workgroup waits for another.  The front (entries, segment starts, the
 * order inside a session), the workgroup's segmented scan and the finish tail
 * are plan_bucket_common.h's.
 */
#include "plan_bucket_common.h"

/* sgpu_desc() (srtpgpu.h) on the device */
__device__ __forceinline__ uint64_t brx_desc(int64_t ix, uint32_t flags)
{
	return ((uint64_t)ix & 0xffffffffffffull) | ((uint64_t)flags << 48);
}

/*
 * The bucket in LDS.  u[] / mx[] are read by rx_settle with one sorted
 * position per lane, so a wave's look-back step reads 64 consecutive
 * 8-byte words (ds_read_b64: each 32-lane half covers one 256-byte bank
 * row, conflict-free); they are written once, EPT consecutive positions
 * per thread.
 */
struct BrxLds {
	int64_t u[SGPU_BP_CAPMAX];      /* speculated index of sorted position k */
	int64_t mx[SGPU_BP_CAPMAX];     /* max of its segment's indices before k */
	uint32_t ent[SGPU_BP_CAPMAX];   /* entry word, arrival order in bucket */
	uint16_t sq[SGPU_BP_CAPMAX];    /* seq */
	uint16_t srt[SGPU_BP_CAPMAX];   /* rank in session, then: entries by
					   (session, packet index) */
	uint16_t un[SGPU_BP_CAPMAX];    /* entries by session (unstable) */
	uint8_t sl[SGPU_BP_CAPMAX];     /* session in bucket */
	struct sgpu_sstate st[SGPU_BP_NSB];
	int64_t h0[SGPU_BP_NSB];        /* (roc, s_l) the segment starts from */
	int64_t smx[SGPU_BP_NSB];       /* maximum of the segment's indices */
	uint32_t cnt[SGPU_BP_NSB], start[SGPU_BP_NSB];
	uint32_t smin[SGPU_BP_NSB], smax[SGPU_BP_NSB];
	uint32_t wlo[SGPU_BP_NSB], whi[SGPU_BP_NSB];    /* accepted packets' bits */
	struct rx_seg wagg[BPB / 64];
	uint32_t bf, nlate, ndup;
};

/* sorted position k's scan element: a segment's first packet carries its
 * index (the reference step from the session's state), the others their
 * distance to the packet before; *bad: that step is an ETIMEDOUT */
__device__ __forceinline__ int64_t brx_elem(const BrxLds &S, uint32_t k,
					    bool *head, bool *bad)
{
	const uint32_t e = S.srt[k], l = S.sl[e];
	const uint32_t seq = S.sq[e];
	*head = k == S.start[l];
	if (*head) {
		int64_t u0 = 0;
		int bump = 0;
		if (rx_step(S.h0[l], seq, &u0, &bump)) {
			*bad = true;
			u0 = 0;
		}
		return u0;
	}
	return rx_sdiff16(seq, S.sq[S.srt[k - 1]]);
}

__global__ void __launch_bounds__(BPB)
k_bp_rx_plan(const struct sgpu_bplan_rx R)
{
	__shared__ BrxLds S;
	const struct sgpu_bplan &P = R.b;
	const uint32_t tid = threadIdx.x, b = blockIdx.x;
	const uint32_t s0 = b << P.bshift;
	const uint32_t ns = min(1u << P.bshift, P.nsess - s0);
	const uint32_t EPT = P.cap / BPB;
	/* the bucket's entries (EPT per thread, all in flight): index, seq and
	 * session, SSRC */
	uint4 ev4[BK_EPT];
	uint32_t m;
	uint32_t f = bk_entries(P.afail, P.n, P.nb, P.bcount, P.tmp, P.cap, &m,
				ev4);
	if (tid == 0) {
		S.bf = 0;
		S.nlate = S.ndup = 0;
	}
	if (tid < ns) {
		/* the session's resident state: the host's upload first where
		 * the device copy is stale */
		const uint32_t s = s0 + tid, slot = P.cm[s] >> 1;
		struct sgpu_sstate x;
		if (P.upneed && P.upneed[s]) {
			x = bk_ld(P.up + s);
			bk_st(P.sst + slot, x);
		}
		else {
			x = bk_ld(P.sst + slot);
		}
		S.st[tid] = x;
		S.cnt[tid] = 0;
		S.smin[tid] = 0xffffffffu;
		S.smax[tid] = 0;
		S.wlo[tid] = S.whi[tid] = 0;
	}
	__syncthreads();
	/* the entries: seq, session, rank in session */
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		if (k >= m)
			continue;
		const uint32_t l = ev4[j].y >> 16;
		S.ent[k] = ev4[j].x;
		S.sq[k] = (uint16_t)ev4[j].y;
		S.sl[k] = (uint8_t)l;
		S.srt[k] = (uint16_t)atomicAdd(&S.cnt[l], 1u);
		atomicMin(&S.smin[l], ev4[j].z);
		atomicMax(&S.smax[l], ev4[j].z);
	}
	__syncthreads();
	bk_starts(S.cnt, S.start, ns);
	/* one SSRC per session: the stored one, or the segment's; a window
	 * the rule's signed arithmetic cannot hold is left to the host */
	if (tid < ns && S.cnt[tid]) {
		const struct sgpu_sstate &x = S.st[tid];
		if (S.smin[tid] != S.smax[tid] ||
		    ((x.flags & SST_EXISTS) && S.smin[tid] != x.ssrc))
			f |= SPF_SSRC;
		if (S.cnt[tid] > SGPU_BP_SEGMAX)
			f |= SPF_SEG;
		if (x.lix >> 62)
			f |= SPF_ORDER;
	}
	if (f)
		atomicOr(&S.bf, f);
	f = 0;
	__syncthreads();
	const bool dead = S.bf != 0;    /* the plan fails: nothing more */
	/* by (session, packet index): the order the reference receives them in */
	bk_sort16(m, dead, S.ent, S.sl, S.cnt, S.start, S.un, S.srt);
	__syncthreads();
	if (tid < ns && !dead && S.cnt[tid]) {
		/* the receiver's state before the batch as one number; a fresh
		 * stream takes its first packet's seq as s_l (stream_get_seq) */
		const struct sgpu_sstate &x = S.st[tid];
		const uint32_t s_l = (x.flags & SST_SL_SET) ?
				     (x.s_l & 0xffffu) : S.sq[S.srt[S.start[tid]]];
		S.h0[tid] = (int64_t)(((uint64_t)x.roc << 16) | s_l);
		S.smx[tid] = RX_NEG;
	}
	__syncthreads();
	/* the segmented (sum, max) scan over the sorted positions: EPT
	 * consecutive positions per thread, the threads' aggregates scanned
	 * across the workgroup */
	int64_t dv[BK_EPT];
	uint32_t hbits = 0;
	struct rx_seg agg = rx_seg_identity();
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid * EPT + j;
		dv[j] = 0;
		if (dead || (uint32_t)j >= EPT || k >= m)
			continue;
		bool head = false, bad = false;
		dv[j] = brx_elem(S, k, &head, &bad);
		if (bad)
			f |= SPF_TIMEOUT;
		hbits |= (head ? 1u : 0u) << j;
		agg = rx_seg_combine(agg, rx_seg_elem(dv[j], head));
	}
	{
		struct rx_seg run = bk_excl_scan(agg, S.wagg);
#pragma unroll
		for (int j = 0; j < BK_EPT; j++) {
			const uint32_t k = tid * EPT + j;
			if (dead || (uint32_t)j >= EPT || k >= m)
				continue;
			const int head = (hbits >> j) & 1u;
			const uint32_t l = S.sl[S.srt[k]];
			S.mx[k] = rx_seg_mx(run, head);
			run = rx_seg_combine(run, rx_seg_elem(dv[j], head));
			S.u[k] = run.a.s;
			if (k + 1 == S.start[l] + S.cnt[l])
				S.smx[l] = run.a.m;
		}
	}
	if (f)
		atomicOr(&S.bf, f);
	f = 0;
	__syncthreads();
	uint32_t nlate = 0, ndup = 0;
	if (!S.bf) {
		/* per packet: the verification and the replay verdict with
		 * segment-local indices (the look-back counts arrivals of its
		 * own stream), desc as scan_dec (batch_host.c) writes it */
		for (uint32_t k = tid; k < m; k += BPB) {
			const uint32_t e = S.srt[k], l = S.sl[e];
			const uint32_t f0 = S.start[l];
			const uint32_t i = S.ent[e] & BP_IMASK;
			const struct sgpu_sstate &x = S.st[l];
			const int64_t lix0 = (int64_t)x.lix;
			const int r = rx_settle(S.u + f0, S.mx + f0, k - f0, S.sq[e],
						R.lookback, S.h0[l], lix0, x.bitmap,
						1);
			if (r == RX_UNSETTLED) {
				f |= SPF_ORDER;
				continue;
			}
			const int64_t ui = S.u[k];
			/* an EALREADY packet's MAC is still checked (HMAC suites:
			 * not decrypted; GCM decrypts to authenticate) */
			P.desc[i] = brx_desc(ui, r == RX_DUP && R.hmac ?
						 SD_RUN : SD_RUN | SD_CIPHER);
			R.rs[i] = (uint8_t)r;
			if (r == RX_DUP) {
				ndup++;
				continue;
			}
			const uint64_t bit = rx_bit(rx_max(lix0, S.smx[l]), ui);
			if ((uint32_t)bit)
				atomicOr(&S.wlo[l], (uint32_t)bit);
			if ((uint32_t)(bit >> 32))
				atomicOr(&S.whi[l], (uint32_t)(bit >> 32));
			if (ui < rx_max(lix0, S.mx[k]))
				nlate++;
		}
	}
	if (f)
		atomicOr(&S.bf, f);
	if (nlate)
		atomicAdd(&S.nlate, nlate);
	if (ndup)
		atomicAdd(&S.ndup, ndup);
	__syncthreads();
	const bool held = S.bf == 0;
	/* every session's state after the batch */
	if (tid < ns) {
		const uint32_t s = s0 + tid, c = S.cnt[tid];
		struct sgpu_sstate o = S.st[tid];
		o.flags &= ~(uint32_t)SST_TOUCHED;
		if (c && held) {
			const struct sgpu_sstate &x = S.st[tid];
			const int64_t lix0 = (int64_t)x.lix;
			const int64_t Mn = rx_max(S.h0[tid], S.smx[tid]);
			const int64_t lix = rx_max(lix0, S.smx[tid]);
			o.ssrc = (x.flags & SST_EXISTS) ? x.ssrc : S.smin[tid];
			o.roc = (uint32_t)((uint64_t)Mn >> 16);
			o.s_l = (uint32_t)((uint64_t)Mn & 0xffffu);
			o.flags = SST_EXISTS | SST_SL_SET | SST_TOUCHED;
			o.lix = (uint64_t)lix;
			o.bitmap = rx_bitmap_base(lix, lix0, x.bitmap) |
				   (uint64_t)S.whi[tid] << 32 | S.wlo[tid];
		}
		bk_st(P.sout + s, o);
	}
	if (tid == 0) {
		R.cnt[2 * b] = S.nlate;
		R.cnt[2 * b + 1] = S.ndup;
		if (!held)
			atomicOr(&P.out->fail, S.bf);
	}
	/* a rejected plan closes the crypto launches' class guards (the
	 * scatter opened packet 0's class) */
	if (!held && tid < 4)
		P.out->skip[tid] = 1;
}

__global__ void __launch_bounds__(BPB)
k_bp_rx_finish(const struct sgpu_bplan_rx R)
{
	__shared__ uint32_t tot[2];
	const struct sgpu_bplan &P = R.b;
	const uint32_t tid = threadIdx.x;
	const uint32_t fail = P.out->fail;
	const uint32_t nf = *(volatile const uint32_t *)P.nfail;
	const bool ok = !fail && !nf;
	if (blockIdx.x >= P.nb) {
		/* per packet (coalesced): the caller's results, as k_rx_commit */
		if (!ok)
			return;
		const uint32_t i0 = (blockIdx.x - P.nb) * (BPB * SGPU_BP_PPT);
#pragma unroll
		for (int j = 0; j < SGPU_BP_PPT; j++) {
			const uint32_t i = i0 + j * BPB + tid;
			if (i >= P.n)
				break;
			P.endw[i] = P.es[i] + (uint32_t)P.delta;
			if (R.rs[i] == RX_DUP) {
				/* srtp.c:355-368 / 413-422: pos at the payload */
				P.posw[i] += P.hdr[i].hdr_len;
				P.err[i] = EALREADY;
			}
			else {
				P.err[i] = 0;
			}
		}
		return;
	}
	const uint32_t b = blockIdx.x;
	const uint32_t s0 = b << P.bshift;
	const uint32_t ns = min(1u << P.bshift, P.nsess - s0);
	/* the scatter's counters back to zero for the next call */
	if (tid == 0)
		P.bcount[b] = 0;
	if (b == 0 && tid < BP_OBINS)
		P.obins[tid] = 0;
	if (ok && tid < ns) {
		/* the touched states replace the resident ones */
		const uint32_t s = s0 + tid;
		struct sgpu_sstate o = bk_ld(P.sout + s);
		if (o.flags & SST_TOUCHED) {
			o.flags &= ~(uint32_t)SST_TOUCHED;
			bk_st(P.sst + (P.cm[s] >> 1), o);
		}
	}
	if (b != 0)
		return;
	/* the call's outcome: the buckets' counts, the miss count next to the
	 * plan out, all of it to the pinned mirror with vector stores */
	bk_counts(R.cnt, P.nb, tot);
	if (tid == 0) {
		R.ro->nlate = tot[0];
		R.ro->ndup = tot[1];
		P.out->nfail = nf;
	}
	__syncthreads();
	bk_post(P.out, P.outh, P.outbytes, BK_NOWORD, 0);
}

/* ---- host side ------------------------------------------------------ */

static int brx_check(const struct sgpu_bplan_rx *r)
{
	const struct sgpu_bplan *b = &r->b;
	if (bk_geom_bad(b->n, b->nsess, b->nb, b->bshift, b->cap) ||
	    b->prot || !r->rs || !r->cnt || !r->ro)
		return EINVAL;
	return 0;
}

extern "C" int sgpu_bplan_rx_plan(const struct sgpu_bplan_rx *r, void *stream)
{
	if (brx_check(r))
		return EINVAL;
	hipLaunchKernelGGL(k_bp_rx_plan, dim3(r->b.nb), dim3(BPB), 0,
			   (hipStream_t)stream, *r);
	return bk_err("k_bp_rx_plan");
}

extern "C" int sgpu_bplan_rx_finish(const struct sgpu_bplan_rx *r,
				    void *stream)
{
	if (brx_check(r))
		return EINVAL;
	hipLaunchKernelGGL(k_bp_rx_finish, dim3(r->b.nb + bk_grid(r->b.n)),
			   dim3(BPB), 0, (hipStream_t)stream, *r);
	return bk_err("k_bp_rx_finish");
}
