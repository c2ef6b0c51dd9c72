/*
 * plan_buckets_rtcp_rx.hip -- exact device plan of an SRTCP unprotect batch
 * (HMAC suites) over many sessions with up to 8 SSRCs each whose packets
 * arrive reordered, duplicated or replayed inside their streams (srtpgpu.h
 * struct sgpu_bplan_rtcp_rx; the rule per (session, SSRC):
 * plan_rtcp_seg_rx.h).
 *
 * plan_buckets_rtcp.hip speculates every stream's indices new and increasing
 * and rejects such a batch with SPF_REPLAY; this planner runs behind that
 * rejection, on the stream tables that plan uploaded.  k_bpr_scatter runs
 * again unchanged (k_bpr_finish zeroed the bucket counters), then
 *
 *   k_bprx_plan    per bucket, in LDS: k_bpr_plan's front half -- the entries
 *                  grouped by session and ranked by packet index, per packet
 *                  the look back over its session's segment for its slot and
 *                  its rank among its stream's arrivals, new SSRCs behind the
 *                  known ones in first-appearance order (a 9th: SPF_SSRC).
 *                  A session's streams then lie one behind the other (a
 *                  stream's first arrival at the sum of the slots' counts
 *                  before it, an arrival `rank` behind that), and one
 *                  segmented (sum, max) scan over the regrouped positions
 *                  gives every arrival's index u[] and the maximum mx[] of
 *                  its stream's indices before it.  Per packet: the checks of
 *                  plan_rtcp_packet other than the replay one, rx_replay with
 *                  segment-local positions, desc (an EALREADY packet's with
 *                  E clear: its tag is verified, nothing is deciphered), a
 *                  verdict byte, the window bits, the bucket's late /
 *                  duplicate counts; per touched session its table after the
 *                  batch.  An unsettled packet or a failed check ORs the
 *                  plan's fail word, which guards the crypto launches.
 *   (the compact crypto kernels with per-packet keys, guarded by out->fail)
 *   k_bprx_finish  only if the plan held and every tag verified: end / err
 *                  per packet (0, or EALREADY with the tag taken off as the
 *                  reference leaves it); always: the scatter's counters back
 *                  to zero, the call's outcome to the pinned mirror.
 *
 * LDS: u[] / mx[] (64 KiB as int64, read by rx_replay as they are) take the
 * place of the arrays in (session, packet index) order, which are dead once
 * every thread holds its packets' slot and rank in registers; the array the
 * entries are first grouped in becomes the regrouped packet index.  The
 * stream records stay in global memory (the upload is L2-resident; a lane
 * reads the one record it needs) and only the tables' SSRCs are held for the
 * slot search: 158 KiB.
 *
 * No workgroup waits for another.  The front, both passes' look back and slot,
 * the workgroup's segmented scan and the finish tail are
 * plan_bucket_common.h's, with the barriers each of them contains.
 */
#include "plan_bucket_common.h"

static_assert(RSEG_MAX == 8, "sinfo holds 8 touched bits, ps 3 slot bits");
static_assert(SGPU_BP_NSB <= 256, "ps holds 8 session bits");

/* ---- per bucket, the plan --------------------------------------------- */

/* sorted position k (session, packet index): live until every thread holds
 * its packets' slot and rank */
struct BprxSorted {
	uint32_t idx[SGPU_BP_CAPMAX];   /* packet index, */
	uint32_t ssrc[SGPU_BP_CAPMAX];  /* SSRC, */
	uint32_t word[SGPU_BP_CAPMAX];  /* E || index, */
	uint32_t meta[SGPU_BP_CAPMAX];  /* session | parsed << 8 | L << 16 */
};

/* regrouped position p (session, slot, arrival): the scan's */
struct BprxScan {
	int64_t u[SGPU_BP_CAPMAX];      /* the arrival's index */
	int64_t mx[SGPU_BP_CAPMAX];     /* max of its stream's indices before p */
};

static_assert(sizeof(struct BprxScan) == sizeof(struct BprxSorted),
	      "u / mx take the sorted arrays' place");

#define PS_PARSED 0x8000u

struct BprxLds {
	union {
		struct BprxSorted a;
		struct BprxScan b;
	} v;
	uint32_t pi[SGPU_BP_CAPMAX];    /* first: packet index, grouped by
					   session; then regrouped position p:
					   packet index, */
	uint32_t pw[SGPU_BP_CAPMAX];    /* E || index, */
	uint32_t ps[SGPU_BP_CAPMAX];    /* session << 3 | slot | PS_PARSED |
					   L << 16 */
	uint8_t opens[SGPU_BP_CAPMAX];  /* sorted position k opens a new stream */
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

static_assert(sizeof(struct BprxLds) <= 160 * 1024, "one workgroup's LDS");

/* stream x of session l before the batch: the uploaded record, or a stream
 * the batch opened */
__device__ __forceinline__ struct rseg_rec
bprx_rec(const struct sgpu_bplan_rtcp &P, const BprxLds &S, uint32_t l,
	 uint32_t x)
{
	if (x < S.nk[l])
		return bk_ld(P.recs + S.t0[l] + x);
	return rsrx_new(S.tss[l][x]);
}

/* the maximum of the indices of the stream whose arrivals lie at
 * [f0, f0 + c) */
__device__ __forceinline__ uint32_t bprx_smx(const BprxLds &S, uint32_t f0,
					     uint32_t c)
{
	return rsrx_smx(S.v.b.u[f0 + c - 1], S.v.b.mx[f0 + c - 1]);
}

__global__ void __launch_bounds__(BPB)
k_bprx_plan(const struct sgpu_bplan_rtcp_rx R)
{
	__shared__ BprxLds S;
	const struct sgpu_bplan_rtcp &P = R.r;
	const struct sgpu_rplan_in &in = P.in;
	const uint32_t tid = threadIdx.x, b = blockIdx.x;
	const uint32_t s0 = b << P.bshift;
	const uint32_t ns = min(1u << P.bshift, P.nsess - s0);
	const uint32_t EPT = P.cap / BPB;
	/* the bucket's entries: packet index, session in bucket | parsed << 8 |
	 * L << 16, SSRC, E || index */
	uint4 ev4[BK_EPT];
	uint32_t m;
	uint32_t f = bk_entries(P.afail, in.n, P.nb, P.bcount, P.tmp, P.cap, &m,
				ev4);
	if (tid == 0) {
		S.bf = 0;
		S.nlate = S.ndup = 0;
	}
	f |= bk_tables(P.toff, s0, ns, S.t0, S.nk, S.nst, S.cnt, S.tmask,
		       &S.acc[0][0], &S.wlo[0][0], &S.whi[0][0]);
	__syncthreads();
	/* the tables' SSRCs, one per thread */
	for (uint32_t q = tid; q < ns * RSEG_MAX; q += BPB) {
		const uint32_t l = q / RSEG_MAX, x = q % RSEG_MAX;
		S.tss[l][x] = x < S.nk[l] ? P.recs[S.t0[l] + x].ssrc : 0u;
	}
	/* by (session, packet index): the order the reference receives them in */
	uint32_t pos[BK_EPT];
	bool dead = bk_sort(ev4, 0, m, ns, f, S.cnt, S.start, S.pi, &S.bf, pos);
	f = 0;
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		if (dead || tid + j * BPB >= m)
			continue;
		S.v.a.idx[pos[j]] = ev4[j].x;
		S.v.a.meta[pos[j]] = ev4[j].y;
		S.v.a.ssrc[pos[j]] = ev4[j].z;
		S.v.a.word[pos[j]] = ev4[j].w;
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
		const uint32_t l = S.v.a.meta[k] & 0xffu;
		kn[j] = bk_look(k, S.start[l], S.v.a.ssrc, S.tss[l], S.nk[l],
				S.opens, &rank[j], &firstk[j]);
	}
	__syncthreads();
	/* pass 2: the slot; a new stream's SSRC; the stream's arrivals; what
	 * the packet is, into registers */
	uint32_t sl[BK_EPT], pidx[BK_EPT], pword[BK_EPT], pmeta[BK_EPT];
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		sl[j] = RSEG_NONE;
		pidx[j] = pword[j] = pmeta[j] = 0;
		if (dead || k >= m)
			continue;
		const uint32_t mt = S.v.a.meta[k], l = mt & 0xffu;
		const uint32_t slot = bk_slot(kn[j], firstk[j], S.start[l], S.nk[l],
					      S.opens);
		if (rseg_enosr(slot)) {
			f |= SPF_SSRC;  /* a 9th stream: ENOSR on the host */
			continue;
		}
		sl[j] = slot;
		pidx[j] = S.v.a.idx[k];
		pword[j] = S.v.a.word[k];
		pmeta[j] = mt;
		if (S.opens[k])
			S.tss[l][slot] = S.v.a.ssrc[k];
		bk_touch(l, slot, S.opens[k], rank[j] + 1u, S.nst, S.tmask,
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
			S.first[l][x] = (uint16_t)rsrx_first(S.start[l], S.acc[l], x);
		}
	__syncthreads();
	if (!dead) {
#pragma unroll
		for (int j = 0; j < BK_EPT; j++) {
			const uint32_t k = tid + j * BPB;
			if (k >= m || sl[j] == RSEG_NONE)
				continue;
			const uint32_t l = pmeta[j] & 0xffu;
			const uint32_t p = S.first[l][sl[j]] + rank[j];
			S.pi[p] = pidx[j];
			S.pw[p] = pword[j];
			S.ps[p] = l << 3 | sl[j] |
				  ((pmeta[j] >> 8 & 1u) ? PS_PARSED : 0u) |
				  (pmeta[j] & 0xffff0000u);
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
		const uint32_t l = S.ps[p] >> 3 & 0xffu, x = S.ps[p] & 7u;
		const int head = p == S.first[l][x];
		dv[j] = rsrx_elem(head, S.pw[p], head ? 0u : S.pw[p - 1]);
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
	__syncthreads();
	uint32_t nlate = 0, ndup = 0;
	if (!dead) {
		/* per packet: the checks, the replay verdict with positions
		 * local to its stream's segment */
		for (uint32_t p = tid; p < m; p += BPB) {
			const uint32_t e = S.ps[p], l = e >> 3 & 0xffu, x = e & 7u;
			const uint32_t f0 = S.first[l][x], i = S.pi[p];
			const struct rseg_rec st = bprx_rec(P, S, l, x);
			const uint32_t pf = rsrx_flags(in, st, (e & PS_PARSED) != 0,
						       e >> 16, S.pw[p]);
			if (pf) {
				f |= pf;
				continue;
			}
			const int r = rsrx_verdict(S.v.b.u + f0, S.v.b.mx + f0,
						   p - f0, R.lookback, st);
			if (r == RX_UNSETTLED) {
				f |= SPF_REPLAY;
				continue;
			}
			const int64_t ui = S.v.b.u[p];
			P.desc[i] = rsrx_desc(r, S.pw[p]);
			R.rs[i] = (uint8_t)r;
			if (r == RX_DUP) {
				ndup++;
				continue;
			}
			const uint64_t bit =
				rsrx_bit(st, bprx_smx(S, f0, S.acc[l][x]), ui);
			if ((uint32_t)bit)
				atomicOr(&S.wlo[l][x], (uint32_t)bit);
			if ((uint32_t)(bit >> 32))
				atomicOr(&S.whi[l][x], (uint32_t)(bit >> 32));
			if (rsrx_late(ui, st, S.v.b.mx[p]))
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
			struct rseg_rec o = bprx_rec(P, S, l, x);
			if (S.tmask[l] >> x & 1u)
				o = rsrx_after(o, bprx_smx(S, S.first[l][x],
							   S.acc[l][x]),
					       (uint64_t)S.whi[l][x] << 32 |
					       S.wlo[l][x]);
			*(uint4 *)(P.sout + (size_t)(s0 + l) * RSEG_MAX + x) =
				make_uint4(o.ssrc, o.ix, o.blo, o.bhi);
		}
	}
	if (tid < ns)
		P.sinfo[s0 + tid] = held && S.tmask[tid] ?
				    S.nst[tid] | S.tmask[tid] << 8 : 0u;
	if (tid == 0) {
		R.cnt[2 * b] = held ? S.nlate : 0u;
		R.cnt[2 * b + 1] = held ? S.ndup : 0u;
		/* a rejected plan closes the crypto launch's guard */
		if (!held)
			atomicOr(&P.out->fail, S.bf);
	}
}

/* ---- results, counters, the plan out ---------------------------------- */

__global__ void __launch_bounds__(BPB)
k_bprx_finish(const struct sgpu_bplan_rtcp_rx R)
{
	__shared__ uint32_t tot[2];
	const struct sgpu_bplan_rtcp &P = R.r;
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
			if (R.rs[i] == RX_DUP) {
				/* srtcp.c:187-209: the tag is off, E || index
				 * stays, pos where it was */
				P.endw[i] = P.es[i] - P.in.tag;
				P.err[i] = EALREADY;
			}
			else {
				P.endw[i] = P.es[i] + (uint32_t)P.delta;
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
	/* the call's outcome: the buckets' counts, the miss count next to the
	 * plan out, all of it to the pinned mirror with vector stores
	 * (out->fail is final: the plan kernel completed before the crypto
	 * launch) */
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

static int bprx_check(const struct sgpu_bplan_rtcp_rx *x)
{
	const struct sgpu_bplan_rtcp *r = &x->r;
	const uintptr_t o = (uintptr_t)r->out, q = (uintptr_t)x->ro;
	if (bk_geom_bad(r->in.n, r->nsess, r->nb, r->bshift, r->cap) ||
	    r->in.prot || r->in.gcm || !r->in.hmac ||
	    !r->pos || !r->end || !r->sess || !r->endw || !r->err || !r->es ||
	    !r->hdr || !r->desc || !r->tmp || !r->bcount || !r->afail ||
	    !r->toff || !r->recs || !r->sout || !r->sinfo || !r->out ||
	    !r->nfail || !x->rs || !x->cnt || !x->ro || r->outbytes % 4u ||
	    q < o || q + sizeof(struct sgpu_bprx_out) > o + r->outbytes)
		return EINVAL;
	return 0;
}

extern "C" int sgpu_bplan_rtcp_rx_plan(const struct sgpu_bplan_rtcp_rx *r,
				       void *stream)
{
	if (bprx_check(r))
		return EINVAL;
	hipLaunchKernelGGL(k_bprx_plan, dim3(r->r.nb), dim3(BPB), 0,
			   (hipStream_t)stream, *r);
	return bk_err("k_bprx_plan");
}

extern "C" int sgpu_bplan_rtcp_rx_finish(const struct sgpu_bplan_rtcp_rx *r,
					 void *stream)
{
	if (bprx_check(r))
		return EINVAL;
	hipLaunchKernelGGL(k_bprx_finish, dim3(r->r.nb + bk_grid(r->r.in.n)),
			   dim3(BPB), 0, (hipStream_t)stream, *r);
	return bk_err("k_bprx_finish");
}
