/*
 * plan_buckets_rtp_streams_rx.hip -- exact device plan of an RTP unprotect
 * batch over many sessions with up to 8 SSRCs each whose packets arrive
 * reordered, duplicated or with gaps inside their streams (srtpgpu.h struct
 * sgpu_bplan_rtps_rx; the rule per (session, SSRC): plan_rtp_seg_rx.h).
 *
 * plan_buckets_rtp_streams.hip speculates every stream in order and rejects
 * such a batch with SPF_ORDER / SPF_REPLAY; this planner runs behind that
 * rejection, on the stream tables that plan uploaded.  k_bp_scatter runs again
 * unchanged (k_bps_finish zeroed the bucket counters), then
 *
 *   k_bsr_plan    per bucket, in LDS: k_bps_plan's front half -- the entries
 *                 grouped by session and ranked by packet index, per packet
 *                 the look back over its session's segment for its slot and
 *                 its rank among its stream's arrivals, new SSRCs behind the
 *                 known ones in first-appearance order (a 9th: SPF_SSRC).
 *                 A session's streams then lie one behind the other (a
 *                 stream's first arrival at the sum of the slots' counts
 *                 before it, an arrival `rank` behind that), and
 *                 k_bp_rx_plan's back half runs per stream segment: one
 *                 segmented (sum, max) scan over the regrouped positions
 *                 gives u[] and mx[], rx_settle verifies every packet with
 *                 segment-local positions, desc / verdict byte per packet,
 *                 the window bits, the bucket's late / duplicate counts, each
 *                 touched session's table after the batch.  An unsettled
 *                 packet or a failed check ORs the plan's fail word and closes
 *                 the crypto launches' class guards.
 *   (the general crypto kernels in array order with per-packet keys, guarded
 *   by skip[] / fail, counting their tag misses)
 *   k_bsr_finish  only if the plan held and every tag verified: pos / end /
 *                 err per packet (0 or EALREADY); always: the scatter's
 *                 counters back to zero, the call's outcome to the pinned
 *                 mirror.
 *
 * LDS: u[] / mx[] (64 KiB as int64, read by rx_settle as they are) do not fit
 * beside k_bps_plan's 157 KiB, 64 KiB of them the stream records.  The records
 * stay in global memory here (the upload is L2-resident; a lane reads the one
 * record it needs where it needs it) and only the tables' SSRCs, 8 KiB, are
 * held for the slot search; the arrays in (session, packet index) order are
 * dead once every thread holds its packets' slot and rank in registers, and
 * u[] / mx[] take their place: 138 KiB.
 *
 * No workgroup waits for another.  The front, both passes' look back and slot,
 * the workgroup's segmented scan and the finish tail are
 * plan_bucket_common.h's, with the barriers each of them contains.
 */
#include "plan_bucket_common.h"

static_assert(RSEG_MAX == 8, "sinfo holds 8 touched bits, ps 3 slot bits");

/* ---- per bucket, the plan --------------------------------------------- */

/* sorted position k (session, packet index): live until every thread holds
 * its packets' slot and rank */
struct BsrSorted {
	uint32_t gidx[SGPU_BP_CAPMAX];  /* packet index, grouped by session */
	uint32_t idx[SGPU_BP_CAPMAX];   /* packet index, */
	uint32_t ssrc[SGPU_BP_CAPMAX];  /* SSRC, */
	uint16_t sq[SGPU_BP_CAPMAX];    /* seq, */
	uint8_t sl[SGPU_BP_CAPMAX];     /* session in bucket */
	uint8_t opens[SGPU_BP_CAPMAX];  /* it opens a new stream */
};

/* regrouped position p (session, slot, arrival): the scan's */
struct BsrScan {
	int64_t u[SGPU_BP_CAPMAX];      /* speculated index */
	int64_t mx[SGPU_BP_CAPMAX];     /* max of its stream's indices before p */
};

static_assert(sizeof(struct BsrScan) == sizeof(struct BsrSorted),
	      "u / mx take the sorted arrays' place");

struct BsrLds {
	union {
		struct BsrSorted a;
		struct BsrScan b;
	} v;
	uint32_t pi[SGPU_BP_CAPMAX];    /* regrouped position p: packet index, */
	uint16_t pq[SGPU_BP_CAPMAX];    /* seq, */
	uint16_t ps[SGPU_BP_CAPMAX];    /* session in bucket << 3 | slot */
	uint32_t tss[SGPU_BP_NSB][RSEG_MAX];    /* the tables' SSRCs */
	uint32_t acc[SGPU_BP_NSB][RSEG_MAX];    /* the stream's arrivals */
	uint32_t wlo[SGPU_BP_NSB][RSEG_MAX];    /* accepted packets' bits */
	uint32_t whi[SGPU_BP_NSB][RSEG_MAX];
	uint16_t first[SGPU_BP_NSB][RSEG_MAX];  /* the stream's first position */
	uint32_t cnt[SGPU_BP_NSB], start[SGPU_BP_NSB];
	uint32_t t0[SGPU_BP_NSB];       /* the session's records in recs[] */
	uint32_t nk[SGPU_BP_NSB];       /* streams before the batch */
	uint32_t nst[SGPU_BP_NSB];      /* ... and after */
	uint32_t tmask[SGPU_BP_NSB];    /* streams with packets */
	struct rx_seg wagg[BPB / 64];
	uint32_t bf, nlate, ndup;
};

/* stream x of session l before the batch: the uploaded record, or a stream
 * the batch opened */
__device__ __forceinline__ struct tseg_rec
bsr_rec(const struct sgpu_bplan_rtps &T, const BsrLds &S, uint32_t l,
	uint32_t x)
{
	if (x < S.nk[l])
		return bk_ld(T.recs + S.t0[l] + x);
	return tsrx_new(S.tss[l][x]);
}

/* the maximum of the indices of the stream whose arrivals lie at
 * [f0, f0 + c) */
__device__ __forceinline__ int64_t bsr_smx(const BsrLds &S, uint32_t f0,
					   uint32_t c)
{
	return tsrx_smx(S.v.b.u[f0 + c - 1], S.v.b.mx[f0 + c - 1]);
}

__global__ void __launch_bounds__(BPB)
k_bsr_plan(const struct sgpu_bplan_rtps_rx R)
{
	__shared__ BsrLds S;
	const struct sgpu_bplan_rtps &T = R.s;
	const struct sgpu_bplan &P = T.b;
	const uint32_t tid = threadIdx.x, b = blockIdx.x;
	const uint32_t s0 = b << P.bshift;
	const uint32_t ns = min(1u << P.bshift, P.nsess - s0);
	const uint32_t EPT = P.cap / BPB;
	/* the bucket's entries: index | length bin << 26, seq | session in
	 * bucket << 16, SSRC, (place in the bin: not used) */
	uint4 ev4[BK_EPT];
	uint32_t m;
	uint32_t f = bk_entries(P.afail, P.n, P.nb, P.bcount, P.tmp, P.cap, &m,
				ev4);
#pragma unroll
	for (int j = 0; j < BK_EPT; j++)
		ev4[j].x &= BP_IMASK;
	if (tid == 0) {
		S.bf = 0;
		S.nlate = S.ndup = 0;
	}
	f |= bk_tables(T.toff, s0, ns, S.t0, S.nk, S.nst, S.cnt, S.tmask,
		       &S.acc[0][0], &S.wlo[0][0], &S.whi[0][0]);
	__syncthreads();
	/* the tables' SSRCs, one per thread */
	for (uint32_t q = tid; q < ns * RSEG_MAX; q += BPB) {
		const uint32_t l = q / RSEG_MAX, x = q % RSEG_MAX;
		S.tss[l][x] = x < S.nk[l] ? T.recs[S.t0[l] + x].ssrc : 0u;
	}
	/* by (session, packet index): the order the reference receives them in */
	uint32_t pos[BK_EPT];
	bool dead = bk_sort(ev4, 16, m, ns, f, S.cnt, S.start, S.v.a.gidx, &S.bf,
			    pos);
	f = 0;
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		if (dead || tid + j * BPB >= m)
			continue;
		S.v.a.idx[pos[j]] = ev4[j].x;
		S.v.a.sq[pos[j]] = (uint16_t)ev4[j].y;
		S.v.a.sl[pos[j]] = (uint8_t)bk_key(ev4[j], 16);
		S.v.a.ssrc[pos[j]] = ev4[j].z;
	}
	__syncthreads();
	/* pass 1, per sorted position: the known slot, the look back */
	uint32_t kn[BK_EPT], rank[BK_EPT], firstk[BK_EPT];
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		kn[j] = RSEG_NONE;
		rank[j] = 0;
		firstk[j] = k;
		if (dead || k >= m)
			continue;
		const uint32_t l = S.v.a.sl[k];
		kn[j] = bk_look(k, S.start[l], S.v.a.ssrc, S.tss[l], S.nk[l],
				S.v.a.opens, &rank[j], &firstk[j]);
	}
	__syncthreads();
	/* pass 2: the slot; a new stream's SSRC; the stream's arrivals; what
	 * the packet is, into registers */
	uint32_t sl[BK_EPT], pidx[BK_EPT], pseq[BK_EPT], psess[BK_EPT];
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		sl[j] = RSEG_NONE;
		pidx[j] = pseq[j] = psess[j] = 0;
		if (dead || k >= m)
			continue;
		const uint32_t l = S.v.a.sl[k];
		const uint32_t slot = bk_slot(kn[j], firstk[j], S.start[l], S.nk[l],
					      S.v.a.opens);
		if (rseg_enosr(slot)) {
			f |= SPF_SSRC;  /* a 9th stream: ENOSR on the host */
			continue;
		}
		sl[j] = slot;
		pidx[j] = S.v.a.idx[k];
		pseq[j] = S.v.a.sq[k];
		psess[j] = l;
		if (S.v.a.opens[k])
			S.tss[l][slot] = S.v.a.ssrc[k];
		bk_touch(l, slot, S.v.a.opens[k], rank[j] + 1u, S.nst, S.tmask,
			 &S.acc[l][slot]);
	}
	if (f)
		atomicOr(&S.bf, f);
	f = 0;
	__syncthreads();
	dead = S.bf != 0;
	/* a session's streams one behind the other */
	if (!dead)
		for (uint32_t q = tid; q < ns * RSEG_MAX; q += BPB) {
			const uint32_t l = q / RSEG_MAX, x = q % RSEG_MAX;
			S.first[l][x] = (uint16_t)tsrx_first(S.start[l], S.acc[l], x);
		}
	__syncthreads();
	if (!dead) {
#pragma unroll
		for (int j = 0; j < BK_EPT; j++) {
			const uint32_t k = tid + j * BPB;
			if (k >= m || sl[j] == RSEG_NONE)
				continue;
			const uint32_t p = S.first[psess[j]][sl[j]] + rank[j];
			S.pi[p] = pidx[j];
			S.pq[p] = (uint16_t)pseq[j];
			S.ps[p] = (uint16_t)(psess[j] << 3 | sl[j]);
		}
	}
	__syncthreads();
	/* the segmented (sum, max) scan over the regrouped positions: EPT
	 * consecutive positions per thread, the threads' aggregates scanned
	 * across the workgroup (the sorted arrays are dead: every thread passed
	 * the barriers behind pass 2) */
	int64_t dv[BK_EPT];
	uint32_t hbits = 0;
	struct rx_seg agg = rx_seg_identity();
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t p = tid * EPT + j;
		dv[j] = 0;
		if (dead || (uint32_t)j >= EPT || p >= m)
			continue;
		const uint32_t l = S.ps[p] >> 3, x = S.ps[p] & 7u;
		const int head = p == S.first[l][x];
		int64_t H0 = 0;
		int bad = 0;
		if (head) {
			const struct tseg_rec st = bsr_rec(T, S, l, x);
			if (!tsrx_held(st))
				f |= SPF_ORDER;
			H0 = tsrx_h0(st, S.pq[p]);
		}
		dv[j] = tsrx_elem(head, H0, S.pq[p], head ? 0u : S.pq[p - 1], &bad);
		if (bad)
			f |= SPF_TIMEOUT;
		hbits |= (head ? 1u : 0u) << j;
		agg = rx_seg_combine(agg, rx_seg_elem(dv[j], head));
	}
	{
		struct rx_seg run = bk_excl_scan(agg, S.wagg);
#pragma unroll
		for (int j = 0; j < BK_EPT; j++) {
			const uint32_t p = tid * EPT + j;
			if (dead || (uint32_t)j >= EPT || p >= m)
				continue;
			const int head = (hbits >> j) & 1u;
			S.v.b.mx[p] = rx_seg_mx(run, head);
			run = rx_seg_combine(run, rx_seg_elem(dv[j], head));
			S.v.b.u[p] = run.a.s;
		}
	}
	if (f)
		atomicOr(&S.bf, f);
	f = 0;
	__syncthreads();
	uint32_t nlate = 0, ndup = 0;
	if (!S.bf) {
		/* per packet: the verification and the replay verdict with
		 * positions local to its stream's segment */
		for (uint32_t p = tid; p < m; p += BPB) {
			const uint32_t l = S.ps[p] >> 3, x = S.ps[p] & 7u;
			const uint32_t f0 = S.first[l][x], i = S.pi[p];
			const struct tseg_rec st = bsr_rec(T, S, l, x);
			const int64_t H0 = tsrx_h0(st, S.pq[f0]);
			const int64_t lix0 = (int64_t)tseg_lix(st);
			const int r = rx_settle(S.v.b.u + f0, S.v.b.mx + f0, p - f0,
						S.pq[p], R.lookback, H0, lix0,
						tseg_bitmap(st), 1);
			if (r == RX_UNSETTLED) {
				f |= SPF_ORDER;
				continue;
			}
			const int64_t ui = S.v.b.u[p];
			P.desc[i] = d_desc((uint64_t)ui, tsrx_fl(r, (int)R.hmac));
			R.rs[i] = (uint8_t)r;
			if (r == RX_DUP) {
				ndup++;
				continue;
			}
			const uint64_t bit = tsrx_bit(st, bsr_smx(S, f0, S.acc[l][x]),
						      ui);
			if ((uint32_t)bit)
				atomicOr(&S.wlo[l][x], (uint32_t)bit);
			if ((uint32_t)(bit >> 32))
				atomicOr(&S.whi[l][x], (uint32_t)(bit >> 32));
			if (tsrx_late(ui, lix0, S.v.b.mx[p]))
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
	/* every touched session's table after the batch: a touched stream from
	 * its segment, the others as they were */
	if (held) {
		for (uint32_t q = tid; q < ns * RSEG_MAX; q += BPB) {
			const uint32_t l = q / RSEG_MAX, x = q % RSEG_MAX;
			if (!S.tmask[l] || x >= S.nst[l])
				continue;
			struct tseg_rec st = bsr_rec(T, S, l, x);
			if (S.tmask[l] >> x & 1u) {
				const uint32_t f0 = S.first[l][x];
				st = tsrx_after(st, tsrx_h0(st, S.pq[f0]),
						bsr_smx(S, f0, S.acc[l][x]),
						(uint64_t)S.whi[l][x] << 32 |
						S.wlo[l][x]);
			}
			bk_st(T.sout + (size_t)(s0 + l) * RSEG_MAX + x, st);
		}
	}
	if (tid < ns)
		T.sinfo[s0 + tid] = held && S.tmask[tid] ?
				    S.nst[tid] | S.tmask[tid] << 8 : 0u;
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

/* ---- results, counters, the plan out ---------------------------------- */

__global__ void __launch_bounds__(BPB)
k_bsr_finish(const struct sgpu_bplan_rtps_rx R)
{
	__shared__ uint32_t tot[2];
	const struct sgpu_bplan &P = R.s.b;
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
	/* the scatter's counters back to zero for the next call */
	if (tid == 0)
		P.bcount[blockIdx.x] = 0;
	if (blockIdx.x != 0)
		return;
	if (tid < BP_OBINS)
		P.obins[tid] = 0;
	/* the call's outcome: the buckets' counts, the miss count next to the
	 * plan out, all of it to the pinned mirror with vector stores
	 * (out->fail is final: the plan kernel completed before the crypto
	 * launches) */
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

static int bsr_check(const struct sgpu_bplan_rtps_rx *r)
{
	const struct sgpu_bplan *b = &r->s.b;
	if (bk_geom_bad(b->n, b->nsess, b->nb, b->bshift, b->cap) ||
	    b->prot || !b->posw || !b->endw || !b->err || !b->es || !b->hdr ||
	    !b->desc || !b->tmp || !b->bcount || !b->obins || !b->afail ||
	    !b->out || !b->nfail || !r->s.toff || !r->s.recs || !r->s.sout ||
	    !r->s.sinfo || !r->rs || !r->cnt || !r->ro ||
	    b->outbytes % 4u)
		return EINVAL;
	return 0;
}

extern "C" int sgpu_bplan_rtps_rx_plan(const struct sgpu_bplan_rtps_rx *r,
				       void *stream)
{
	if (bsr_check(r))
		return EINVAL;
	hipLaunchKernelGGL(k_bsr_plan, dim3(r->s.b.nb), dim3(BPB), 0,
			   (hipStream_t)stream, *r);
	return bk_err("k_bsr_plan");
}

extern "C" int sgpu_bplan_rtps_rx_finish(const struct sgpu_bplan_rtps_rx *r,
					 void *stream)
{
	if (bsr_check(r))
		return EINVAL;
	hipLaunchKernelGGL(k_bsr_finish, dim3(r->s.b.nb + bk_grid(r->s.b.n)),
			   dim3(BPB), 0, (hipStream_t)stream, *r);
	return bk_err("k_bsr_finish");
}
