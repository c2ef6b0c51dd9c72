/*
 * plan_streams_rtcp.hip -- exact device plan of a single-session SRTCP batch,
 * protect or unprotect, whose packets belong to up to SRTP_MAX_STREAMS (8)
 * SSRCs and arrive in any order: interleaved, reordered, duplicated or
 * replayed inside their streams (srtpgpu.h sgpu_splan_rtcp; the rules:
 * plan_rtcp_seg.h, plan_rtcp_seg_rx.h, composed by plan_rtcp_str.h).
 *
 * k_plan_rtcp / k_rp_plan take one stream in order and reject such a batch
 * with SPF_SSRC / SPF_REPLAY; this planner runs behind that rejection, or at
 * once for a session that already holds several streams.  The bucket planners
 * hold a whole session in one workgroup's LDS; here one session spans the
 * grid, so the streams are laid out one behind the other as
 * plan_streams_rx.hip lays out its RTP streams.  The SRTCP index travels in
 * the packet, so nothing is speculated and one planner serves in-order and
 * disturbed arrivals alike:
 *
 *   (sgpu_splan_table: k_sp_ssrc, k_sp_merge of plan_streams.hip -- the
 *                 session's stream table after the batch, which RTP and RTCP
 *                 share; a 9th SSRC: SPF_SSRC)
 *   k_srt_count   per packet its slot in that table and every check but the
 *                 replay one (fewer than 8 bytes, no room for the trailer,
 *                 size, window, cap); per workgroup and slot the number of
 *                 packets
 *   k_srt_starts  one workgroup: per slot the exclusive sum of those counts
 *                 over the workgroups, the slots' totals and run starts
 *   k_srt_place   per packet place = start[slot] + before[workgroup][slot] +
 *                 its rank among the workgroup's packets of the slot -- a
 *                 stable partition.  Protect: place - start[slot] is the
 *                 packet's rank in its stream, which numbers it: desc.
 *                 Unprotect, GCM: no replay window, desc from the packet's own
 *                 E || index.  Unprotect, HMAC suites: perm[place] = packet,
 *                 word[place] = its E || index
 *   (HMAC unprotect only)
 *   k_srt_agg     per place the scan element (rsrx_elem: a run's head carries
 *                 its index, the others their distance to the arrival
 *                 before); per workgroup the segmented (sum, max) aggregate
 *   k_srt_scan    one workgroup: exclusive segmented scan of the aggregates
 *   k_srt_index   per place u[] (its index) and mx[] (the maximum of its
 *                 stream's indices before it)
 *   k_srt_settle  per place rsrx_verdict with positions local to its run (the
 *                 look-back reads u[] across workgroups, never before the
 *                 run's head), desc (an EALREADY packet's with E clear) and
 *                 verdict byte of perm[place], the accepted packet's bit of
 *                 its stream's window after the batch (atomicOr), late /
 *                 duplicate counts
 *   (all)
 *   k_srt_final   per touched slot the record after the batch
 *
 * and, behind the crypto launch, k_srt_commit: the caller's end / err, only
 * if the plan held (fail == 0) and every tag verified (nfail == 0) -- a
 * rejected plan modifies nothing.  No workgroup waits for another: every
 * launch ends with its own grid.
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdio.h>
#include <string.h>
#include "../srtpgpu.h"
#include "plan_rtcp_str.h"
#include "plan_streams_tab.h"

#define SRT_BLOCK 256
#define SRT_WAVES (SRT_BLOCK / 64)
#define SRT_SCAN 1024

static_assert(sizeof(struct rseg_rec) == sizeof(struct sgpu_rtcp_rec) &&
	      offsetof(struct sgpu_rtcp_rec, blo) == offsetof(struct rseg_rec, blo),
	      "a record is stored as the rule gives it");
static_assert(SP_K == RSEG_MAX, "one slot rule");
static_assert(SRT_BLOCK >= 2 * SP_K, "srt_stage");

/* the runs and the streams' records before the batch, staged in LDS */
struct srt_lds {
	uint32_t start[SP_K], cnt[SP_K];
	struct rseg_rec rec[SP_K];
	uint32_t fail;
};

__device__ __forceinline__ struct rseg_rec srt_known(const struct sgpu_rtcp_rec &x)
{
	struct rseg_rec r;
	r.ssrc = x.ssrc; r.ix = x.ix; r.blo = x.blo; r.bhi = x.bhi;
	return r;
}

/* (every thread of the workgroup; blockDim.x >= 2 * SP_K) */
__device__ __forceinline__ void srt_stage(const struct sgpu_srplan_in &in,
					  const struct sgpu_srplan_out *out,
					  struct srt_lds &L)
{
	const uint32_t t = threadIdx.x;
	if (t < SP_K) {
		L.start[t] = out->start[t];
		L.cnt[t] = out->cnt[t];
	}
#pragma unroll
	for (uint32_t q = 0; q < SP_K; q++)
		if (t == SP_K + q)
			L.rec[q] = rstr_rec(srt_known(in.st[q]), q, in.nst,
					    out->tab.ssrc[q]);
	if (t == 0)
		L.fail = out->tab.base.fail;
	__syncthreads();
}

/* the E || index word of packet i (k_parse's eix word for the tag length) */
__device__ __forceinline__ uint32_t srt_word(const struct sgpu_rplan_in &c,
					     const uint32_t *eix, uint32_t i)
{
	return eix[3 * (size_t)i + (c.tag == 0 ? 0 : c.tag == 4 ? 1 : 2)];
}

/* place p's scan element */
__device__ __forceinline__ struct rx_seg
srt_elem(const struct srt_lds &L, const uint32_t *sw, uint32_t p, uint32_t n)
{
	if (p >= n)
		return rx_seg_identity();
	const uint32_t q = rstr_slot_at(L.start, L.cnt, p);
	if (q == RSEG_NONE)
		return rx_seg_identity();
	const int head = rstr_head(p, L.start[q]);
	return rx_seg_elem(rsrx_elem(head, sw[p], head ? 0u : sw[p - 1]), head);
}

/* inclusive segmented scan of one element per thread over the workgroup
 * (blockDim.x threads, a power of two, sh[] of as many); sh[] then holds
 * every thread's inclusive value */
__device__ __forceinline__ struct rx_seg
srt_block_scan(struct rx_seg e, struct rx_seg *sh)
{
	const uint32_t t = threadIdx.x;
	sh[t] = e;
	__syncthreads();
	for (uint32_t d = 1; d < blockDim.x; d <<= 1) {
		struct rx_seg v = rx_seg_identity();
		if (t >= d)
			v = sh[t - d];
		__syncthreads();
		e = rx_seg_combine(v, e);
		sh[t] = e;
		__syncthreads();
	}
	return e;
}

__global__ void __launch_bounds__(SRT_BLOCK)
k_srt_count(const struct sgpu_srplan_in in, const struct sgpu_hdr *hdr,
	    const uint32_t *eix, const uint32_t *pos, const uint32_t *end,
	    const uint32_t *cap, uint64_t asz, uint8_t *slot, uint32_t *bcnt,
	    struct sgpu_srplan_out *out)
{
	__shared__ uint32_t tab[SP_K], nt;
	__shared__ uint32_t wc[SRT_WAVES][SP_K];
	const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
	const uint32_t i = blockIdx.x * SRT_BLOCK + t;
	if (t < SP_K)
		tab[t] = out->tab.ssrc[t];
	if (t == 0)
		nt = min(out->tab.nst, (uint32_t)SP_K);
	__syncthreads();
	uint32_t k = SP_K, f = 0;
	if (i < in.c.n) {
		const struct sgpu_hdr h = hdr[i];
		const uint32_t p = pos[i], e = end[i];
		const int parsed = h.hdr_len != PLAN_NOHDR;
		if (parsed) {
			/* the packet's SSRC chooses its stream */
			const uint32_t s = rstr_slot(tab, nt, h.ssrc);
			if (s == RSEG_NONE)
				f |= SPF_SSRC;
			else
				k = s;
		}
		f |= rstr_flags(in.c, h.ssrc, parsed, e - p,
				plan_window_flags(p, e, cap != NULL,
						  cap ? cap[i] : 0u, asz,
						  in.c.maxlen, in.c.need,
						  (int)in.c.prot),
				in.c.prot ? 0u : srt_word(in.c, eix, i));
		slot[i] = (uint8_t)k;
		if (f)
			atomicOr(&out->tab.base.fail, f);
	}
#pragma unroll
	for (uint32_t q = 0; q < SP_K; q++) {
		const uint64_t b = __ballot(k == q);
		if (lane == 0)
			wc[wv][q] = (uint32_t)__popcll(b);
	}
	__syncthreads();
	if (t < SP_K) {
		uint32_t s = 0;
		for (uint32_t w = 0; w < SRT_WAVES; w++)
			s += wc[w][t];
		bcnt[(size_t)t * gridDim.x + blockIdx.x] = s;
	}
}

/* per slot the exclusive sums of the workgroups' counts, in place (one
 * workgroup); the slots' totals and their runs' starts */
__global__ void __launch_bounds__(SRT_SCAN)
k_srt_starts(uint32_t *bcnt, uint32_t nb, struct sgpu_srplan_out *out)
{
	__shared__ uint32_t part[SP_K][SRT_SCAN];
	__shared__ uint32_t wt[SRT_SCAN / 64][SP_K];
	__shared__ uint32_t tot[SP_K];
	const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
	const uint32_t per = (nb + SRT_SCAN - 1) / SRT_SCAN;
	const uint32_t a = min(t * per, nb), e = min(a + per, nb);
#pragma unroll 1
	for (uint32_t q = 0; q < SP_K; q++) {
		uint32_t s = 0;
		for (uint32_t b = a; b < e; b++)
			s += bcnt[(size_t)q * nb + b];
		uint32_t v = s;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t y = (uint32_t)__shfl_up((int)v, d);
			if ((int)lane >= d)
				v += y;
		}
		if (lane == 63)
			wt[wv][q] = v;
		part[q][t] = v - s;
	}
	__syncthreads();
#pragma unroll 1
	for (uint32_t q = 0; q < SP_K; q++) {
		uint32_t pre = 0, all = 0;
		for (uint32_t w = 0; w < SRT_SCAN / 64; w++) {
			const uint32_t v = wt[w][q];
			if (w < wv)
				pre += v;
			all += v;
		}
		uint32_t run = part[q][t] + pre;
		for (uint32_t b = a; b < e; b++) {
			const uint32_t v = bcnt[(size_t)q * nb + b];
			bcnt[(size_t)q * nb + b] = run;
			run += v;
		}
		if (t == 0)
			tot[q] = all;
	}
	__syncthreads();
	if (t == 0) {
		uint32_t st[SP_K];
		rstr_starts(tot, st);
		for (uint32_t q = 0; q < SP_K; q++) {
			out->start[q] = st[q];
			out->cnt[q] = tot[q];
		}
	}
}

__global__ void __launch_bounds__(SRT_BLOCK)
k_srt_place(const struct sgpu_srplan_in in, const struct sgpu_hdr *hdr,
	    const uint32_t *eix, const uint32_t *pos, const uint32_t *end,
	    const uint8_t *slot, const uint32_t *before,
	    const struct sgpu_srplan_out *out, uint64_t *desc, uint32_t *perm,
	    uint32_t *sw)
{
	__shared__ struct srt_lds L;
	__shared__ uint32_t wc[SRT_WAVES][SP_K];
	const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
	const uint32_t n = in.c.n;
	const uint32_t i = blockIdx.x * SRT_BLOCK + t;
	const uint32_t k = i < n ? slot[i] : SP_K;
	uint64_t mine = 0;
#pragma unroll
	for (uint32_t q = 0; q < SP_K; q++) {
		const uint64_t b = __ballot(k == q);
		if (k == q)
			mine = b;
		if (lane == 0)
			wc[wv][q] = (uint32_t)__popcll(b);
	}
	srt_stage(in, out, L);
	/* a check of k_srt_count failed: the counts do not cover the batch */
	if (L.fail || k >= SP_K)
		return;
	uint32_t ahead = (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
	for (uint32_t w = 0; w < wv; w++)
		ahead += wc[w][k];
	const uint32_t place =
		rstr_place(L.start[k],
			   before[(size_t)k * gridDim.x + blockIdx.x], ahead);
	if (place >= n)
		return;
	if (in.c.prot) {
		const struct plan_rtcp r =
			rstr_tx(in.c, L.rec[k], place, L.start[k], 1,
				end[i] - pos[i], 0);
		desc[i] = plan_rtcp_desc(r.ix, r.E);
	}
	else if (!in.c.hmac) {
		desc[i] = rsrx_desc(RX_OK, srt_word(in.c, eix, i));
	}
	else {
		perm[place] = i;
		sw[place] = srt_word(in.c, eix, i);
	}
}

__global__ void __launch_bounds__(SRT_BLOCK)
k_srt_agg(const struct sgpu_srplan_in in, const uint32_t *sw,
	  struct rx_seg *agg, const struct sgpu_srplan_out *out)
{
	__shared__ struct srt_lds L;
	__shared__ struct rx_seg sh[SRT_BLOCK];
	srt_stage(in, out, L);
	/* (the places mean nothing: k_srt_place did not run) */
	if (L.fail)
		return;
	const uint32_t p = blockIdx.x * SRT_BLOCK + threadIdx.x;
	const struct rx_seg a =
		srt_block_scan(srt_elem(L, sw, p, in.c.n), sh);
	if (threadIdx.x == SRT_BLOCK - 1)
		agg[blockIdx.x] = a;
}

/* exclusive segmented scan of the nb workgroup aggregates (one workgroup) */
__global__ void __launch_bounds__(SRT_SCAN)
k_srt_scan(struct rx_seg *agg, uint32_t nb, const struct sgpu_srplan_out *out)
{
	__shared__ struct rx_seg part[SRT_SCAN];
	__shared__ uint32_t fail;
	if (threadIdx.x == 0)
		fail = out->tab.base.fail;
	__syncthreads();
	if (fail)
		return;
	const uint32_t per = (nb + SRT_SCAN - 1) / SRT_SCAN;
	const uint32_t a = min(threadIdx.x * per, nb), e = min(a + per, nb);
	struct rx_seg sum = rx_seg_identity();
	for (uint32_t k = a; k < e; k++)
		sum = rx_seg_combine(sum, agg[k]);
	srt_block_scan(sum, part);
	struct rx_seg run = threadIdx.x ? part[threadIdx.x - 1]
					: rx_seg_identity();
	for (uint32_t k = a; k < e; k++) {
		const struct rx_seg v = agg[k];
		agg[k] = run;
		run = rx_seg_combine(run, v);
	}
}

__global__ void __launch_bounds__(SRT_BLOCK)
k_srt_index(const struct sgpu_srplan_in in, const uint32_t *sw,
	    const struct rx_seg *pre, const struct sgpu_srplan_out *out,
	    int64_t *u, int64_t *mx)
{
	__shared__ struct srt_lds L;
	__shared__ struct rx_seg sh[SRT_BLOCK];
	srt_stage(in, out, L);
	if (L.fail)
		return;
	const uint32_t p = blockIdx.x * SRT_BLOCK + threadIdx.x;
	const struct rx_seg e = srt_elem(L, sw, p, in.c.n);
	srt_block_scan(e, sh);
	if (p >= in.c.n)
		return;
	const struct rx_seg ex = rx_seg_combine(
		pre[blockIdx.x],
		threadIdx.x ? sh[threadIdx.x - 1] : rx_seg_identity());
	mx[p] = rx_seg_mx(ex, (int)e.head);
	u[p] = rx_seg_combine(ex, e).a.s;
}

__global__ void __launch_bounds__(SRT_BLOCK)
k_srt_settle(const struct sgpu_srplan_in in, const uint32_t *sw,
	     const uint32_t *perm, const int64_t *u, const int64_t *mx,
	     uint64_t *desc, uint8_t *rs, struct sgpu_srplan_out *out)
{
	__shared__ struct srt_lds L;
	srt_stage(in, out, L);
	/* a check before failed: the indices mean nothing */
	if (L.fail)
		return;
	const uint32_t p = blockIdx.x * SRT_BLOCK + threadIdx.x;
	const uint32_t q = p < in.c.n ? rstr_slot_at(L.start, L.cnt, p)
				      : RSEG_NONE;
	bool late = false, dup = false;
	if (q != RSEG_NONE) {
		const uint32_t f0 = L.start[q], c = L.cnt[q];
		const struct rseg_rec st = L.rec[q];
		const int r = rsrx_verdict(u + f0, mx + f0, rstr_rank(p, f0),
					   in.lookback, st);
		if (r == RX_UNSETTLED) {
			atomicOr(&out->tab.base.fail, (uint32_t)SPF_REPLAY);
		}
		else {
			const int64_t ui = u[p];
			const uint32_t i = perm[p];
			desc[i] = rsrx_desc(r, sw[p]);
			rs[i] = (uint8_t)r;
			dup = r == RX_DUP;
			if (!dup) {
				const uint64_t bit =
					rsrx_bit(st, rstr_smx(u, mx, f0, c), ui);
				if (bit)
					atomicOr((unsigned long long *)&out->bits[q],
						 (unsigned long long)bit);
				late = rsrx_late(ui, st, mx[p]);
			}
		}
	}
	const uint32_t nl = (uint32_t)__popcll(__ballot(late));
	const uint32_t nd = (uint32_t)__popcll(__ballot(dup));
	if ((threadIdx.x & 63u) == 0) {
		if (nl)
			atomicAdd(&out->nlate, nl);
		if (nd)
			atomicAdd(&out->ndup, nd);
	}
}

/* the touched streams' records after the batch, once every packet is
 * settled */
__global__ void __launch_bounds__(64)
k_srt_final(const struct sgpu_srplan_in in, const int64_t *u,
	    const int64_t *mx, struct sgpu_srplan_out *out)
{
	__shared__ struct srt_lds L;
	srt_stage(in, out, L);
	const uint32_t t = threadIdx.x;
	if (t < SP_K && !L.fail && L.cnt[t]) {
		struct rseg_rec a = L.rec[t];
		if (in.c.prot)
			a = rstr_tx_after(a, L.cnt[t]);
		else if (in.c.hmac)
			a = rsrx_after(a, rstr_smx(u, mx, L.start[t], L.cnt[t]),
				       out->bits[t]);
		struct sgpu_rtcp_rec r;
		r.ssrc = a.ssrc; r.ix = a.ix; r.blo = a.blo; r.bhi = a.bhi;
		out->after[t] = r;
	}
}

/* rs: NULL where no packet can be an EALREADY (protect, GCM) */
__global__ void __launch_bounds__(SRT_BLOCK)
k_srt_commit(const struct sgpu_srplan_out *out, const uint8_t *rs,
	     const uint32_t *es, uint32_t *end, int32_t *err, uint32_t n,
	     uint32_t tag, int32_t delta)
{
	const uint32_t i = blockIdx.x * SRT_BLOCK + threadIdx.x;
	if (i >= n || out->tab.base.fail || out->tab.base.nfail)
		return;
	if (rs && rs[i] == RX_DUP) {
		/* srtcp.c:187-209: the tag is off, E || index stays, pos where
		 * it was */
		end[i] = es[i] - tag;
		err[i] = EALREADY;
	}
	else {
		end[i] = es[i] + (uint32_t)delta;
		err[i] = 0;
	}
}

/* ---- host side ------------------------------------------------------ */

/* the table launches' scratch | slot[] | per workgroup and slot counts |
 * perm[] | word[] | workgroup aggregates | u[] | mx[] | verdict bytes */
struct srt_scratch {
	uint8_t *tab, *slot, *rs;
	uint32_t *bcnt, *perm, *sw;
	struct rx_seg *agg;
	int64_t *u, *mx;
	size_t bytes;
};

static struct srt_scratch srt_layout(void *scratch, uint32_t n)
{
	const size_t nb = ((size_t)n + SRT_BLOCK - 1) / SRT_BLOCK;
	struct srt_scratch s;
	uint8_t *p = (uint8_t *)scratch;
	s.tab = p;
	p += sp_al(sgpu_splan_table_scratch(n));
	s.slot = p;
	p += sp_al(n);
	s.bcnt = (uint32_t *)p;
	p += sp_al(nb * SP_K * 4);
	s.perm = (uint32_t *)p;
	p += sp_al((size_t)n * 4);
	s.sw = (uint32_t *)p;
	p += sp_al((size_t)n * 4);
	s.agg = (struct rx_seg *)p;
	p += sp_al(nb * sizeof(struct rx_seg));
	s.u = (int64_t *)p;
	p += sp_al((size_t)n * 8);
	s.mx = (int64_t *)p;
	p += sp_al((size_t)n * 8);
	s.rs = p;
	p += sp_al(n);
	s.bytes = (size_t)(p - (uint8_t *)scratch);
	return s;
}

static int srt_rx_hmac(const struct sgpu_srplan_in *in)
{
	return !in->c.prot && in->c.hmac;
}

extern "C" unsigned sgpu_splan_rtcp_block(void)
{
	return SRT_BLOCK;
}

extern "C" size_t sgpu_splan_rtcp_scratch(uint32_t n)
{
	return srt_layout(NULL, n).bytes;
}

extern "C" int sgpu_splan_rtcp(const struct sgpu_srplan_in *in,
			       const struct sgpu_hdr *hdr, const uint32_t *eix,
			       const uint32_t *pos, const uint32_t *end,
			       const uint32_t *cap, uint64_t arena_size,
			       uint64_t *desc, void *scratch,
			       size_t scratch_bytes, struct sgpu_srplan_out *out,
			       void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	const uint32_t n = in->c.n;
	const uint32_t nb = (n + SRT_BLOCK - 1) / SRT_BLOCK;
	struct sgpu_splan_in ti;
	if (!n || in->nst > SP_K || (!in->c.prot && !eix) ||
	    (in->c.hmac && in->c.gcm) ||
	    scratch_bytes < sgpu_splan_rtcp_scratch(n))
		return EINVAL;
	const struct srt_scratch s = srt_layout(scratch, n);
	if (!in->zeroed &&
	    hipMemsetAsync(out, 0, sizeof(*out), st) != hipSuccess)
		return EIO;
	/* the table launches read n, nst and the known SSRCs */
	memset(&ti, 0, sizeof(ti));
	ti.n = n;
	ti.nst = in->nst;
	for (uint32_t q = 0; q < in->nst; q++)
		ti.st[q].ssrc = in->st[q].ssrc;
	if (sgpu_splan_table(&ti, hdr, s.tab, &out->tab, stream))
		return EIO;
	hipLaunchKernelGGL(k_srt_count, dim3(nb), dim3(SRT_BLOCK), 0, st, *in,
			   hdr, eix, pos, end, cap, arena_size, s.slot, s.bcnt,
			   out);
	hipLaunchKernelGGL(k_srt_starts, dim3(1), dim3(SRT_SCAN), 0, st, s.bcnt,
			   nb, out);
	hipLaunchKernelGGL(k_srt_place, dim3(nb), dim3(SRT_BLOCK), 0, st, *in,
			   hdr, eix, pos, end, (const uint8_t *)s.slot,
			   (const uint32_t *)s.bcnt,
			   (const struct sgpu_srplan_out *)out, desc, s.perm, s.sw);
	if (srt_rx_hmac(in)) {
		hipLaunchKernelGGL(k_srt_agg, dim3(nb), dim3(SRT_BLOCK), 0, st,
				   *in, (const uint32_t *)s.sw, s.agg,
				   (const struct sgpu_srplan_out *)out);
		hipLaunchKernelGGL(k_srt_scan, dim3(1), dim3(SRT_SCAN), 0, st,
				   s.agg, nb, (const struct sgpu_srplan_out *)out);
		hipLaunchKernelGGL(k_srt_index, dim3(nb), dim3(SRT_BLOCK), 0, st,
				   *in, (const uint32_t *)s.sw,
				   (const struct rx_seg *)s.agg,
				   (const struct sgpu_srplan_out *)out, s.u, s.mx);
		hipLaunchKernelGGL(k_srt_settle, dim3(nb), dim3(SRT_BLOCK), 0, st,
				   *in, (const uint32_t *)s.sw,
				   (const uint32_t *)s.perm, (const int64_t *)s.u,
				   (const int64_t *)s.mx, desc, s.rs, out);
	}
	hipLaunchKernelGGL(k_srt_final, dim3(1), dim3(64), 0, st, *in,
			   (const int64_t *)s.u, (const int64_t *)s.mx, out);
	return hipGetLastError() == hipSuccess ? 0 : EIO;
}

extern "C" int sgpu_splan_rtcp_commit(const struct sgpu_srplan_in *in,
				      const struct sgpu_srplan_out *out,
				      const void *scratch, const uint32_t *es,
				      uint32_t *end, int32_t *err, int32_t delta,
				      void *stream)
{
	const uint32_t n = in->c.n;
	const uint32_t nb = (n + SRT_BLOCK - 1) / SRT_BLOCK;
	if (!n)
		return 0;
	const struct srt_scratch s = srt_layout((void *)scratch, n);
	hipLaunchKernelGGL(k_srt_commit, dim3(nb), dim3(SRT_BLOCK), 0,
			   (hipStream_t)stream, out,
			   srt_rx_hmac(in) ? (const uint8_t *)s.rs : NULL, es, end,
			   err, n, in->c.tag, delta);
	return hipGetLastError() == hipSuccess ? 0 : EIO;
}
