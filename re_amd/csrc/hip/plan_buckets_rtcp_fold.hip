/*
 * plan_buckets_rtcp_fold.hip -- forged packets of an SRTCP unprotect batch
 * over many sessions settled on the device (srtpgpu.h struct
 * sgpu_bplan_rtcp_fold; the rule per (session, SSRC): plan_rtcp_seg_fold.h).
 *
 * It runs behind a plan of plan_buckets_rtcp.hip or plan_buckets_rtcp_rx.hip
 * that was accepted and whose crypto launch counted tag misses: the verdict
 * bytes of that launch are final (the index travels in the packet, the HMAC
 * covers it with the session's key), a forged packet lies there as it arrived
 * and an EALREADY one with its tag verified and nothing deciphered.  On the
 * stream tables that plan uploaded, HMAC suites: k_bpr_scatter runs again
 * unchanged (the plan's finish zeroed the bucket counters; it zeroes
 * out->fail, which is the settle's own fail word from here on), then
 *
 *   k_bprf_settle  per bucket, in LDS, the decomposition of k_bprx_plan: the
 *                  entries grouped by session and ranked by packet index, slot
 *                  and rank from the look back (a forged arrival takes or
 *                  opens its slot like any other; a 9th: SPF_SSRC), the
 *                  session's streams one behind the other, one segmented
 *                  (sum, max) scan in which a forged arrival carries the
 *                  index -1.  Per packet: EAUTH, or rx_replay over the
 *                  authentic arrivals; the byte rs[] (the result, and
 *                  SV_CIPHERED for a packet the plan left undeciphered as
 *                  EALREADY and the settle accepts), the window bits of the
 *                  accepted ones, late / duplicate counts; per touched session
 *                  its table after the batch.  An unsettled packet ORs
 *                  out->fail, which guards what follows.
 *   (the compact crypto kernels' keystream launch -- sgpu_compact undo -- with
 *   rs[] for its verdict bytes: AES-CM over [8, end - 4 - tag) of exactly the
 *   packets named there, each with its session's round keys and salt, byte-
 *   exact at the region's end, guarded by out->fail)
 *   k_bprf_finish  only if the settle held: end / err per packet (0; EALREADY
 *                  and EAUTH with the tag taken off as the reference leaves
 *                  them, srtcp.c:192-209), the desc word of a deciphered
 *                  packet; always: the scatter's counters back to zero, the
 *                  outcome to the pinned mirror.
 *
 * GCM suites keep no SRTCP replay window (srtcp.c:180): no packet hangs on a
 * forged one and the plan's tables hold.  k_bprf_gcm writes the results alone:
 * a forged packet's pos behind its 8 header bytes, its end at the E || index
 * word, its payload as the cipher left it (srtcp.c:212-279; the compact GCM
 * kernel deciphers whatever the tag says, as the reference does).
 *
 * LDS: that of k_bprx_plan; the forged flag travels in a free bit of the
 * words that hold the session and the slot, so nothing is added.  No
 * workgroup waits for another.
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdio.h>
#include "../srtpgpu.h"
#include "plan_rtcp_seg_fold.h"

#ifndef EAUTH
#define EAUTH 217               /* include/re_types.h:215-217 */
#endif

#define BPB SGPU_BP_BLOCK
#define BPRF_EPT (SGPU_BP_CAPMAX / BPB) /* entries per thread, at most */

static_assert(sizeof(struct rseg_rec) == 16 &&
	      sizeof(struct sgpu_rtcp_rec) == 16 &&
	      offsetof(struct sgpu_rtcp_rec, blo) ==
	      offsetof(struct rseg_rec, blo),
	      "a stream record moves as one 16-byte word");
static_assert(RSEG_MAX == 8, "sinfo holds 8 touched bits, ps 3 slot bits");
static_assert(SGPU_BP_NSB <= 256, "ps holds 8 session bits");

__device__ __forceinline__ struct rseg_rec bprf_ld(const struct sgpu_rtcp_rec *p)
{
	const uint4 a = *(const uint4 *)p;
	struct rseg_rec r;
	r.ssrc = a.x; r.ix = a.y; r.blo = a.z; r.bhi = a.w;
	return r;
}

__device__ __forceinline__ struct rx_seg bprf_shfl_up(struct rx_seg v, int d)
{
	struct rx_seg r;
	r.a.s = __shfl_up((long long)v.a.s, d);
	r.a.m = __shfl_up((long long)v.a.m, d);
	r.head = (uint32_t)__shfl_up((int)v.head, d);
	return r;
}

/* exclusive segmented scan of one element per thread over the workgroup
 * (every thread calls it): in the wave by shuffles, across the 16 waves
 * through their aggregates (as plan_buckets_rtcp_rx.hip bprx_excl_scan) */
__device__ __forceinline__ struct rx_seg bprf_excl_scan(struct rx_seg v,
							struct rx_seg *wagg)
{
	const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
	struct rx_seg x = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const struct rx_seg y = bprf_shfl_up(x, d);
		if (lane >= (uint32_t)d)
			x = rx_seg_combine(y, x);
	}
	if (lane == 63)
		wagg[wv] = x;
	struct rx_seg below = bprf_shfl_up(x, 1);
	if (lane == 0)
		below = rx_seg_identity();
	__syncthreads();
	struct rx_seg pre = rx_seg_identity();
	for (uint32_t q = 0; q < wv; q++)
		pre = rx_seg_combine(pre, wagg[q]);
	__syncthreads();
	return rx_seg_combine(pre, below);
}

/* ---- per bucket, the settle -------------------------------------------- */

/* sorted position k (session, packet index): live until every thread holds
 * its packets' slot and rank */
struct BprfSorted {
	uint32_t idx[SGPU_BP_CAPMAX];   /* packet index, */
	uint32_t ssrc[SGPU_BP_CAPMAX];  /* SSRC, */
	uint32_t word[SGPU_BP_CAPMAX];  /* E || index, */
	uint32_t meta[SGPU_BP_CAPMAX];  /* session | parsed << 8 | forged << 9 |
					   L << 16 */
};

/* regrouped position p (session, slot, arrival): the scan's */
struct BprfScan {
	int64_t u[SGPU_BP_CAPMAX];      /* the arrival's index (forged: -1) */
	int64_t mx[SGPU_BP_CAPMAX];     /* max of its stream's indices before p */
};

static_assert(sizeof(struct BprfScan) == sizeof(struct BprfSorted),
	      "u / mx take the sorted arrays' place");

#define META_FORGED 0x200u
#define PS_PARSED 0x8000u
#define PS_FORGED 0x4000u

struct BprfLds {
	union {
		struct BprfSorted a;
		struct BprfScan b;
	} v;
	uint32_t pi[SGPU_BP_CAPMAX];    /* first: packet index, grouped by
					   session; then regrouped position p:
					   packet index, */
	uint32_t pw[SGPU_BP_CAPMAX];    /* E || index, */
	uint32_t ps[SGPU_BP_CAPMAX];    /* session << 3 | slot | PS_FORGED |
					   PS_PARSED | L << 16 */
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

static_assert(sizeof(struct BprfLds) <= 160 * 1024, "one workgroup's LDS");

/* stream x of session l before the batch: the uploaded record, or a stream
 * the batch opened */
__device__ __forceinline__ struct rseg_rec
bprf_rec(const struct sgpu_bplan_rtcp &P, const BprfLds &S, uint32_t l,
	 uint32_t x)
{
	if (x < S.nk[l])
		return bprf_ld(P.recs + S.t0[l] + x);
	return rsrx_new(S.tss[l][x]);
}

/* the maximum of the authentic indices of stream st, whose arrivals lie at
 * [f0, f0 + c) */
__device__ __forceinline__ uint32_t bprf_smx(const BprfLds &S,
					     struct rseg_rec st, uint32_t f0,
					     uint32_t c)
{
	return rsfold_smx(st, S.v.b.u[f0 + c - 1], S.v.b.mx[f0 + c - 1]);
}

__global__ void __launch_bounds__(BPB)
k_bprf_settle(const struct sgpu_bplan_rtcp_fold F)
{
	__shared__ BprfLds S;
	const struct sgpu_bplan_rtcp_rx &R = F.x;
	const struct sgpu_bplan_rtcp &P = R.r;
	const struct sgpu_rplan_in &in = P.in;
	const uint32_t tid = threadIdx.x, b = blockIdx.x;
	const uint32_t s0 = b << P.bshift;
	const uint32_t ns = min(1u << P.bshift, P.nsess - s0);
	const uint32_t EPT = P.cap / BPB;
	uint32_t m = P.bcount[b];
	uint32_t f = 0;
	{
		/* the scatter workgroups' fail words, spread over the buckets
		 * (no workgroup waits for another) */
		const uint32_t na = (in.n + BPB * SGPU_BP_PPT - 1) /
				    (BPB * SGPU_BP_PPT);
		for (uint32_t k = b + tid * P.nb; k < na; k += BPB * P.nb)
			f |= P.afail[k];
	}
	if (m > P.cap) {
		f |= SPF_SEG;           /* (the scatter flagged it too) */
		m = 0;
	}
	/* the bucket's entries: packet index, session in bucket | parsed << 8 |
	 * L << 16, SSRC, E || index; the crypto launch's verdict joins them */
	uint4 ev4[BPRF_EPT];
#pragma unroll
	for (int j = 0; j < BPRF_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		ev4[j] = k < m ? P.tmp[(size_t)b * P.cap + k]
			       : make_uint4(0, 0, 0, 0);
		if (k < m && ev4[j].x < in.n && !(F.vd[ev4[j].x] & SV_TAG_OK))
			ev4[j].y |= META_FORGED;
	}
	if (tid == 0) {
		S.bf = 0;
		S.nlate = S.ndup = 0;
	}
	if (tid < ns) {
		const uint32_t s = s0 + tid;
		const uint32_t t0 = P.toff[s], t1 = P.toff[s + 1];
		uint32_t nk = t1 - t0;
		if (t1 < t0 || nk > RSEG_MAX) {
			f |= SPF_BAD;   /* (the host builds toff: never) */
			nk = 0;
		}
		S.t0[tid] = t0;
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
	/* the tables' SSRCs, one per thread */
	for (uint32_t q = tid; q < ns * RSEG_MAX; q += BPB) {
		const uint32_t l = q / RSEG_MAX, x = q % RSEG_MAX;
		S.tss[l][x] = x < S.nk[l] ? P.recs[S.t0[l] + x].ssrc : 0u;
	}
	/* rank in session (unstable) */
	uint32_t ru[BPRF_EPT];
#pragma unroll
	for (int j = 0; j < BPRF_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		ru[j] = 0;
		if (k < m)
			ru[j] = atomicAdd(&S.cnt[ev4[j].y & 0xffu], 1u);
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
	bool dead = S.bf != 0;          /* the settle declines: nothing more */
	if (!dead) {
		/* grouped by session */
#pragma unroll
		for (int j = 0; j < BPRF_EPT; j++) {
			const uint32_t k = tid + j * BPB;
			if (k < m)
				S.pi[S.start[ev4[j].y & 0xffu] + ru[j]] = ev4[j].x;
		}
	}
	__syncthreads();
	if (!dead) {
		/* inside a session by packet index: the order the reference
		 * receives them in */
#pragma unroll
		for (int j = 0; j < BPRF_EPT; j++) {
			const uint32_t k = tid + j * BPB;
			if (k >= m)
				continue;
			const uint32_t l = ev4[j].y & 0xffu;
			const uint32_t f0 = S.start[l], c = S.cnt[l];
			uint32_t r = 0;
			for (uint32_t t = f0; t < f0 + c; t++)
				r += S.pi[t] < ev4[j].x ? 1u : 0u;
			S.v.a.idx[f0 + r] = ev4[j].x;
			S.v.a.meta[f0 + r] = ev4[j].y;
			S.v.a.ssrc[f0 + r] = ev4[j].z;
			S.v.a.word[f0 + r] = ev4[j].w;
		}
	}
	__syncthreads();
	/* pass 1, per sorted position: the known slot, the look back */
	uint32_t kn[BPRF_EPT], rank[BPRF_EPT], firstk[BPRF_EPT];
#pragma unroll
	for (int j = 0; j < BPRF_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		kn[j] = RSEG_NONE;
		rank[j] = 0;
		firstk[j] = k;
		if (dead || k >= m)
			continue;
		const uint32_t l = S.v.a.meta[k] & 0xffu, x = S.v.a.ssrc[k];
		struct rseg_look lk = rseg_look_init(k);
		kn[j] = rsrx_known(S.tss[l], S.nk[l], x);
		for (uint32_t t = S.start[l]; t < k; t++)
			lk = rseg_look_step(lk, t, S.v.a.ssrc[t] == x);
		S.opens[k] = (uint8_t)rseg_opens(kn[j], lk);
		rank[j] = lk.rank;
		firstk[j] = lk.first;
	}
	__syncthreads();
	/* pass 2: the slot; a new stream's SSRC; the stream's arrivals; what
	 * the packet is, into registers */
	uint32_t sl[BPRF_EPT], pidx[BPRF_EPT], pword[BPRF_EPT], pmeta[BPRF_EPT];
#pragma unroll
	for (int j = 0; j < BPRF_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		sl[j] = RSEG_NONE;
		pidx[j] = pword[j] = pmeta[j] = 0;
		if (dead || k >= m)
			continue;
		const uint32_t mt = S.v.a.meta[k], l = mt & 0xffu;
		uint32_t nnew = 0;
		if (kn[j] == RSEG_NONE)
			for (uint32_t t = S.start[l]; t < firstk[j]; t++)
				nnew += S.opens[t];
		const uint32_t slot = rseg_slot(kn[j], S.nk[l], nnew);
		if (rseg_enosr(slot)) {
			f |= SPF_SSRC;  /* a 9th stream: ENOSR on the host */
			continue;
		}
		sl[j] = slot;
		pidx[j] = S.v.a.idx[k];
		pword[j] = S.v.a.word[k];
		pmeta[j] = mt;
		if (S.opens[k]) {
			S.tss[l][slot] = S.v.a.ssrc[k];
			atomicMax(&S.nst[l], slot + 1u);
		}
		atomicOr(&S.tmask[l], 1u << slot);
		atomicMax(&S.acc[l][slot], rank[j] + 1u);
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
		for (int j = 0; j < BPRF_EPT; j++) {
			const uint32_t k = tid + j * BPB;
			if (k >= m || sl[j] == RSEG_NONE)
				continue;
			const uint32_t l = pmeta[j] & 0xffu;
			const uint32_t p = S.first[l][sl[j]] + rank[j];
			S.pi[p] = pidx[j];
			S.pw[p] = pword[j];
			S.ps[p] = l << 3 | sl[j] |
				  ((pmeta[j] >> 8 & 1u) ? PS_PARSED : 0u) |
				  ((pmeta[j] & META_FORGED) ? PS_FORGED : 0u) |
				  (pmeta[j] & 0xffff0000u);
		}
	}
	__syncthreads();
	/* the segmented (sum, max) scan over the regrouped positions: EPT
	 * consecutive positions per thread, the threads' aggregates scanned
	 * across the workgroup (the sorted arrays are dead: every thread passed
	 * the barriers behind pass 2) */
	int64_t dv[BPRF_EPT];
	uint32_t hbits = 0;
	struct rx_seg agg = rx_seg_identity();
#pragma unroll
	for (int j = 0; j < BPRF_EPT; j++) {
		const uint32_t p = tid * EPT + j;
		dv[j] = 0;
		if (dead || (uint32_t)j >= EPT || p >= m)
			continue;
		const uint32_t e = S.ps[p], l = e >> 3 & 0xffu, x = e & 7u;
		const int head = p == S.first[l][x];
		dv[j] = rsfold_elem(head, S.pw[p], (e & PS_FORGED) != 0,
				    head ? 0u : S.pw[p - 1],
				    !head && (S.ps[p - 1] & PS_FORGED));
		hbits |= (head ? 1u : 0u) << j;
		agg = rx_seg_combine(agg, rx_seg_elem(dv[j], head));
	}
	{
		struct rx_seg run = bprf_excl_scan(agg, S.wagg);
#pragma unroll
		for (int j = 0; j < BPRF_EPT; j++) {
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
		/* per packet: the checks, the result with positions local to its
		 * stream's segment */
		for (uint32_t p = tid; p < m; p += BPB) {
			const uint32_t e = S.ps[p], l = e >> 3 & 0xffu, x = e & 7u;
			const uint32_t f0 = S.first[l][x], i = S.pi[p];
			const struct rseg_rec st = bprf_rec(P, S, l, x);
			const uint32_t pf = rsrx_flags(in, st, (e & PS_PARSED) != 0,
						       e >> 16, S.pw[p]);
			if (pf) {
				f |= pf;
				continue;
			}
			const int r = rsfold_result(S.v.b.u + f0, S.v.b.mx + f0,
						    p - f0, R.lookback, st,
						    (e & PS_FORGED) != 0);
			if (r < 0) {
				f |= SPF_REPLAY;
				continue;
			}
			if (r == RSF_AUTH) {
				R.rs[i] = rsfold_byte(r, 0);
				continue;
			}
			R.rs[i] = rsfold_byte(r, rsfold_flip(P.desc[i],
							     rsfold_desc(r, S.pw[p]),
							     in.encrypted));
			if (r == RSF_DUP) {
				ndup++;
				continue;
			}
			const int64_t ui = S.v.b.u[p];
			const uint64_t bit =
				rsrx_bit(st, bprf_smx(S, st, f0, S.acc[l][x]), ui);
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
			struct rseg_rec o = bprf_rec(P, S, l, x);
			if (S.tmask[l] >> x & 1u)
				o = rsrx_after(o, bprf_smx(S, o, S.first[l][x],
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
		/* a declined settle closes the guard of what follows */
		if (!held)
			atomicOr(&P.out->fail, S.bf);
	}
}

/* ---- results, counters, the outcome ------------------------------------ */

__global__ void __launch_bounds__(BPB)
k_bprf_finish(const struct sgpu_bplan_rtcp_fold F)
{
	__shared__ uint32_t tot[2];
	const struct sgpu_bplan_rtcp_rx &R = F.x;
	const struct sgpu_bplan_rtcp &P = R.r;
	const uint32_t tid = threadIdx.x;
	const uint32_t fail = P.out->fail;
	if (blockIdx.x >= P.nb) {
		/* per packet (coalesced): the caller's results */
		if (fail)
			return;
		const uint32_t i0 = (blockIdx.x - P.nb) * (BPB * SGPU_BP_PPT);
#pragma unroll
		for (int j = 0; j < SGPU_BP_PPT; j++) {
			const uint32_t i = i0 + j * BPB + tid;
			if (i >= P.in.n)
				break;
			const uint8_t rb = R.rs[i];
			const int r = rsfold_byte_result(rb);
			if (r == RSF_OK) {
				P.endw[i] = P.es[i] + (uint32_t)P.delta;
				P.err[i] = 0;
				/* deciphered behind the plan: its desc word as
				 * the rule gives it */
				if (rb & SV_CIPHERED)
					P.desc[i] |= 1ull << 31;
			}
			else {
				/* srtcp.c:187-209: the tag is off, E || index
				 * stays, pos where it was */
				P.endw[i] = P.es[i] - P.in.tag;
				P.err[i] = r == RSF_DUP ? EALREADY : EAUTH;
			}
		}
		return;
	}
	/* the scatter's counters back to zero for the next call */
	if (tid == 0)
		P.bcount[blockIdx.x] = 0;
	if (blockIdx.x != 0)
		return;
	/* the call's outcome: the buckets' counts next to the plan out, all of
	 * it to the pinned mirror with vector stores (out->fail is final: the
	 * settle completed before the keystream launch) */
	if (tid < 2)
		tot[tid] = 0;
	__syncthreads();
	{
		uint32_t a = 0, d = 0;
		for (uint32_t q = tid; q < P.nb; q += BPB) {
			a += R.cnt[2 * q];
			d += R.cnt[2 * q + 1];
		}
		if (a)
			atomicAdd(&tot[0], a);
		if (d)
			atomicAdd(&tot[1], d);
	}
	__syncthreads();
	if (tid == 0) {
		R.ro->nlate = tot[0];
		R.ro->ndup = tot[1];
	}
	__syncthreads();
	if (P.outh) {
		const uint32_t *src = (const uint32_t *)P.out;
		for (uint32_t w = tid; w < P.outbytes / 4u; w += BPB)
			P.outh[w] = src[w];
	}
}

/* GCM: the results alone */
__global__ void __launch_bounds__(BPB)
k_bprf_gcm(const struct sgpu_bplan_rtcp_fold F)
{
	const struct sgpu_bplan_rtcp &P = F.x.r;
	const uint32_t i = blockIdx.x * BPB + threadIdx.x;
	if (i >= P.in.n)
		return;
	if (F.vd[i] & SV_TAG_OK) {
		P.endw[i] = P.es[i] + (uint32_t)P.delta;
		P.err[i] = 0;
	}
	else {
		/* srtcp.c:212, 244, 276-279: the end at E || index, pos behind
		 * the header */
		F.posw[i] = P.pos[i] + 8u;
		P.endw[i] = P.es[i] - 4u;
		P.err[i] = EAUTH;
	}
}

/* ---- host side ------------------------------------------------------ */

static int bprf_check(const struct sgpu_bplan_rtcp_fold *f)
{
	const struct sgpu_bplan_rtcp_rx *x = &f->x;
	const struct sgpu_bplan_rtcp *r = &x->r;
	const uintptr_t o = (uintptr_t)r->out, q = (uintptr_t)x->ro;
	if (!r->in.n || r->in.n > SGPU_BP_NMAX || r->nsess < 2 || !r->nb ||
	    r->nb > SGPU_BP_NBMAX || r->bshift > 8 || !r->cap ||
	    r->cap > SGPU_BP_CAPMAX || r->cap % BPB ||
	    ((uint64_t)r->nb << r->bshift) < r->nsess ||
	    ((uint64_t)(r->nb - 1) << r->bshift) >= r->nsess ||
	    r->in.prot || r->in.gcm || !r->in.hmac ||
	    !r->pos || !r->end || !r->sess || !r->endw || !r->err || !r->es ||
	    !r->hdr || !r->desc || !r->tmp || !r->bcount || !r->afail ||
	    !r->toff || !r->recs || !r->sout || !r->sinfo || !r->out ||
	    !x->rs || !x->cnt || !x->ro || !f->vd || r->outbytes % 4u ||
	    q < o || q + sizeof(struct sgpu_bprx_out) > o + r->outbytes)
		return EINVAL;
	return 0;
}

static int bprf_err(const char *what)
{
	const hipError_t e = hipGetLastError();
	if (e == hipSuccess)
		return 0;
	fprintf(stderr, "re_srtp: %s launch: %s\n", what, hipGetErrorString(e));
	return EIO;
}

extern "C" int sgpu_bplan_rtcp_fold_settle(const struct sgpu_bplan_rtcp_fold *f,
					   void *stream)
{
	if (bprf_check(f))
		return EINVAL;
	hipLaunchKernelGGL(k_bprf_settle, dim3(f->x.r.nb), dim3(BPB), 0,
			   (hipStream_t)stream, *f);
	return bprf_err("k_bprf_settle");
}

extern "C" int sgpu_bplan_rtcp_fold_finish(const struct sgpu_bplan_rtcp_fold *f,
					   void *stream)
{
	if (bprf_check(f))
		return EINVAL;
	const uint32_t g = (f->x.r.in.n + BPB * SGPU_BP_PPT - 1) /
			   (BPB * SGPU_BP_PPT);
	hipLaunchKernelGGL(k_bprf_finish, dim3(f->x.r.nb + g), dim3(BPB), 0,
			   (hipStream_t)stream, *f);
	return bprf_err("k_bprf_finish");
}

extern "C" int sgpu_bplan_rtcp_fold_gcm(const struct sgpu_bplan_rtcp_fold *f,
					void *stream)
{
	const struct sgpu_bplan_rtcp *r = &f->x.r;
	if (!r->in.n || r->in.n > SGPU_BP_NMAX || r->in.prot || !r->in.gcm ||
	    !r->pos || !r->es || !r->endw || !r->err || !f->posw || !f->vd)
		return EINVAL;
	hipLaunchKernelGGL(k_bprf_gcm, dim3((r->in.n + BPB - 1) / BPB), dim3(BPB),
			   0, (hipStream_t)stream, *f);
	return bprf_err("k_bprf_gcm");
}
