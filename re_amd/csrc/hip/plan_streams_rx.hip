/*
 * plan_streams_rx.hip -- exact device plan of a single-session RTP unprotect
 * batch whose packets belong to up to SRTP_MAX_STREAMS (8) streams, any of
 * which arrives reordered, duplicated, with gaps or replayed (srtpgpu.h
 * sgpu_splan_rx; the rule: plan_rx_rule.h, composed per stream by
 * plan_rtp_seg_rx.h).
 *
 * plan_streams.hip speculates every stream in order and rejects such a batch
 * with SPF_ORDER / SPF_REPLAY; this planner runs behind that rejection.  The
 * bucket planners hold a whole session in one workgroup's LDS; here one
 * session spans the grid, so the streams are first laid out one behind the
 * other and then scanned as plan_rx.hip scans its one stream:
 *
 *   (sgpu_splan_table: k_sp_ssrc, k_sp_merge of plan_streams.hip -- the
 *                 session's stream table after the batch; a 9th SSRC:
 *                 SPF_SSRC)
 *   k_srx_count   per packet its slot in that table and the checks of
 *                 k_sp_count (parse, one header class, tag room, size, window
 *                 validity); per workgroup and slot the number of packets
 *   k_srx_starts  one workgroup: per slot the exclusive sum of those counts
 *                 over the workgroups, the slots' totals and segment starts
 *   k_srx_place   per packet place = start[slot] + before[workgroup][slot] +
 *                 its rank among the workgroup's packets of the slot -- a
 *                 stable partition: perm[place] = packet, sseq[place] = seq,
 *                 a stream's arrivals in batch order are one segment
 *   k_srx_agg     per place the scan element (tsrx_elem: a segment's head
 *                 carries its index from the stream's record, the others
 *                 their distance to the arrival before); per workgroup the
 *                 segmented (sum, max) aggregate
 *   k_srx_scan    one workgroup: exclusive segmented scan of the aggregates
 *   k_srx_index   per place u[] (speculated index) and mx[] (maximum of the
 *                 stream's indices before it)
 *   k_srx_settle  per place rx_settle with positions local to its segment
 *                 (the look-back reads u[] across workgroups, never before
 *                 the segment's head), desc and verdict byte of perm[place],
 *                 the accepted packet's bit of its stream's final window
 *                 (atomicOr), late / duplicate counts
 *   k_srx_final   per touched slot the record after the batch; the crypto
 *                 launches' class guards skip[]
 *
 * and, behind the crypto launches, k_srx_commit: the caller's pos / end / err,
 * only if the plan held (fail == 0) and every tag verified (nfail == 0) -- a
 * rejected plan modifies nothing.  No workgroup waits for another: every
 * launch ends with its own grid.
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdio.h>
#include "../srtpgpu.h"
#include "plan_rtp_seg_rx.h"
#include "plan_streams_tab.h"

#define SRX_BLOCK 256
#define SRX_WAVES (SRX_BLOCK / 64)
#define SRX_SCAN 1024

static_assert(sizeof(struct tseg_rec) == sizeof(struct sgpu_rtp_rec) &&
	      offsetof(struct sgpu_rtp_rec, llo) == offsetof(struct tseg_rec, llo),
	      "a record after the batch is stored as tsrx_after gives it");
static_assert(SP_K == RSEG_MAX, "one slot rule");

/* the segments and the streams' records before the batch, staged in LDS */
struct srx_lds {
	uint32_t start[SP_K], cnt[SP_K];
	struct tseg_rec rec[SP_K];
	uint32_t fail;
};

/* stream q of the table before the batch as the rule sees it: the session's
 * record, or a stream the batch opens (stream.c:45-67) */
__device__ __forceinline__ struct tseg_rec
srx_rec(const struct sgpu_sstate &x)
{
	struct tseg_rec r;
	r.ssrc = x.ssrc;
	r.roc = x.roc;
	r.sl = (x.s_l & 0xffffu) | ((x.flags & SST_SL_SET) ? TSEG_SL_SET : 0u);
	r.pad = 0;
	r.llo = (uint32_t)x.lix;
	r.lhi = (uint32_t)(x.lix >> 32);
	r.blo = (uint32_t)x.bitmap;
	r.bhi = (uint32_t)(x.bitmap >> 32);
	return r;
}

/* (every thread of the workgroup; blockDim.x >= 2 * SP_K) */
__device__ __forceinline__ void srx_stage(const struct sgpu_srxplan_in &in,
					  const struct sgpu_srxplan_out *out,
					  struct srx_lds &L)
{
	const uint32_t t = threadIdx.x;
	if (t < SP_K) {
		L.start[t] = out->start[t];
		L.cnt[t] = out->cnt[t];
	}
#pragma unroll
	for (uint32_t q = 0; q < SP_K; q++)
		if (t == SP_K + q)
			L.rec[q] = q < in.s.nst ? srx_rec(in.s.st[q])
						: tsrx_new(out->tab.ssrc[q]);
	if (t == 0)
		L.fail = out->tab.base.fail;
	__syncthreads();
}

/* the slot whose segment holds place p (SP_K: none) */
__device__ __forceinline__ uint32_t srx_slot_at(const struct srx_lds &L,
						uint32_t p)
{
	uint32_t k = SP_K;
#pragma unroll
	for (uint32_t q = 0; q < SP_K; q++)
		if (p >= L.start[q] && p - L.start[q] < L.cnt[q])
			k = q;
	return k;
}

/* place p's scan element; *f: a record the rule cannot hold, or a head whose
 * step is an ETIMEDOUT */
__device__ __forceinline__ struct rx_seg
srx_elem(const struct srx_lds &L, const uint16_t *sseq, uint32_t p, uint32_t n,
	 uint32_t *f)
{
	if (p >= n)
		return rx_seg_identity();
	const uint32_t q = srx_slot_at(L, p);
	if (q == SP_K)
		return rx_seg_identity();
	const int head = p == L.start[q];
	const uint32_t seq = sseq[p];
	int64_t H0 = 0;
	int bad = 0;
	if (head) {
		const struct tseg_rec st = L.rec[q];
		if (!tsrx_held(st))
			*f |= SPF_ORDER;
		H0 = tsrx_h0(st, seq);
	}
	const int64_t d = tsrx_elem(head, H0, seq, head ? 0u : sseq[p - 1], &bad);
	if (bad)
		*f |= SPF_TIMEOUT;
	return rx_seg_elem(d, head);
}

/* inclusive segmented scan of one element per thread over the workgroup
 * (blockDim.x threads, a power of two, sh[] of as many); sh[] then holds
 * every thread's inclusive value (as plan_rx.hip rx_block_scan) */
__device__ __forceinline__ struct rx_seg
srx_block_scan(struct rx_seg e, struct rx_seg *sh)
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

__global__ void __launch_bounds__(SRX_BLOCK)
k_srx_count(const struct sgpu_srxplan_in in, const struct sgpu_hdr *hdr,
	    const uint32_t *pos, const uint32_t *end, const uint32_t *cap,
	    uint64_t asz, uint8_t *slot, uint32_t *bcnt,
	    struct sgpu_srxplan_out *out)
{
	__shared__ uint32_t tab[SP_K], nt;
	__shared__ uint32_t wc[SRX_WAVES][SP_K];
	const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
	const uint32_t i = blockIdx.x * SRX_BLOCK + t;
	if (t < SP_K)
		tab[t] = out->tab.ssrc[t];
	if (t == 0)
		nt = min(out->tab.nst, (uint32_t)SP_K);
	__syncthreads();
	uint32_t k = SP_K, f = 0;
	if (i < in.s.n) {
		const struct sgpu_hdr h = hdr[i];
		const uint32_t p = pos[i], e = end[i];
		if (h.hdr_len == PLAN_NOHDR) {
			f |= SPF_PARSE;
		}
		else {
			/* the packet's SSRC chooses its stream */
			k = sp_slot(tab, nt, h.ssrc);
			if (k == SP_K)
				f |= SPF_SSRC;
			else
				f |= plan_header_flags(h.hdr_len, hdr[0].hdr_len, 0, 0,
						       PLAN_SSRC_NONE, e - p,
						       in.s.tag, 1, 0);
		}
		f |= plan_window_flags(p, e, cap != NULL, cap ? cap[i] : 0u, asz,
				       in.s.maxlen, 0, 0);
		if (i == 0)
			out->tab.base.hl0 = h.hdr_len;
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
		for (uint32_t w = 0; w < SRX_WAVES; w++)
			s += wc[w][t];
		bcnt[(size_t)t * gridDim.x + blockIdx.x] = s;
	}
}

/* per slot the exclusive sums of the workgroups' counts, in place (one
 * workgroup); the slots' totals and their segments' starts */
__global__ void __launch_bounds__(SRX_SCAN)
k_srx_starts(uint32_t *bcnt, uint32_t nb, struct sgpu_srxplan_out *out)
{
	__shared__ uint32_t part[SP_K][SRX_SCAN];
	__shared__ uint32_t wt[SRX_SCAN / 64][SP_K];
	__shared__ uint32_t tot[SP_K];
	const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
	const uint32_t per = (nb + SRX_SCAN - 1) / SRX_SCAN;
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
		for (uint32_t w = 0; w < SRX_SCAN / 64; w++) {
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
		uint32_t s = 0;
		for (uint32_t q = 0; q < SP_K; q++) {
			out->start[q] = s;
			out->cnt[q] = tot[q];
			s += tot[q];
		}
	}
}

__global__ void __launch_bounds__(SRX_BLOCK)
k_srx_place(uint32_t n, const struct sgpu_hdr *hdr, const uint8_t *slot,
	    const uint32_t *before, const struct sgpu_srxplan_out *out,
	    uint32_t *perm, uint16_t *sseq)
{
	__shared__ uint32_t start[SP_K], fail;
	__shared__ uint32_t wc[SRX_WAVES][SP_K];
	const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
	const uint32_t i = blockIdx.x * SRX_BLOCK + t;
	if (t < SP_K)
		start[t] = out->start[t];
	if (t == 0)
		fail = out->tab.base.fail;
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
	__syncthreads();
	/* a check of k_srx_count failed: the counts do not cover the batch */
	if (fail || k >= SP_K)
		return;
	uint32_t rank = (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
	for (uint32_t w = 0; w < wv; w++)
		rank += wc[w][k];
	const uint32_t place = start[k] +
			       before[(size_t)k * gridDim.x + blockIdx.x] + rank;
	if (place < n) {
		perm[place] = i;
		sseq[place] = hdr[i].seq;
	}
}

__global__ void __launch_bounds__(SRX_BLOCK)
k_srx_agg(const struct sgpu_srxplan_in in, const uint16_t *sseq,
	  struct rx_seg *agg, struct sgpu_srxplan_out *out)
{
	__shared__ struct srx_lds L;
	__shared__ struct rx_seg sh[SRX_BLOCK];
	srx_stage(in, out, L);
	/* (the places mean nothing: k_srx_place did not run) */
	if (L.fail)
		return;
	const uint32_t p = blockIdx.x * SRX_BLOCK + threadIdx.x;
	uint32_t f = 0;
	const struct rx_seg a =
		srx_block_scan(srx_elem(L, sseq, p, in.s.n, &f), sh);
	if (f)
		atomicOr(&out->tab.base.fail, f);
	if (threadIdx.x == SRX_BLOCK - 1)
		agg[blockIdx.x] = a;
}

/* exclusive segmented scan of the nb workgroup aggregates (one workgroup),
 * as k_rx_scan */
__global__ void __launch_bounds__(SRX_SCAN)
k_srx_scan(struct rx_seg *agg, uint32_t nb, const struct sgpu_srxplan_out *out)
{
	__shared__ struct rx_seg part[SRX_SCAN];
	__shared__ uint32_t fail;
	if (threadIdx.x == 0)
		fail = out->tab.base.fail;
	__syncthreads();
	if (fail)
		return;
	const uint32_t per = (nb + SRX_SCAN - 1) / SRX_SCAN;
	const uint32_t a = min(threadIdx.x * per, nb), e = min(a + per, nb);
	struct rx_seg sum = rx_seg_identity();
	for (uint32_t k = a; k < e; k++)
		sum = rx_seg_combine(sum, agg[k]);
	srx_block_scan(sum, part);
	struct rx_seg run = threadIdx.x ? part[threadIdx.x - 1]
					: rx_seg_identity();
	for (uint32_t k = a; k < e; k++) {
		const struct rx_seg v = agg[k];
		agg[k] = run;
		run = rx_seg_combine(run, v);
	}
}

__global__ void __launch_bounds__(SRX_BLOCK)
k_srx_index(const struct sgpu_srxplan_in in, const uint16_t *sseq,
	    const struct rx_seg *pre, const struct sgpu_srxplan_out *out,
	    int64_t *u, int64_t *mx)
{
	__shared__ struct srx_lds L;
	__shared__ struct rx_seg sh[SRX_BLOCK];
	srx_stage(in, out, L);
	if (L.fail)
		return;
	const uint32_t p = blockIdx.x * SRX_BLOCK + threadIdx.x;
	uint32_t f = 0;
	const struct rx_seg e = srx_elem(L, sseq, p, in.s.n, &f);
	srx_block_scan(e, sh);
	if (p >= in.s.n)
		return;
	const struct rx_seg ex = rx_seg_combine(
		pre[blockIdx.x],
		threadIdx.x ? sh[threadIdx.x - 1] : rx_seg_identity());
	mx[p] = rx_seg_mx(ex, (int)e.head);
	u[p] = rx_seg_combine(ex, e).a.s;
}

__global__ void __launch_bounds__(SRX_BLOCK)
k_srx_settle(const struct sgpu_srxplan_in in, const uint16_t *sseq,
	     const uint32_t *perm, const int64_t *u, const int64_t *mx,
	     uint64_t *desc, uint8_t *rs, struct sgpu_srxplan_out *out)
{
	__shared__ struct srx_lds L;
	srx_stage(in, out, L);
	/* a check before failed: the indices mean nothing */
	if (L.fail)
		return;
	const uint32_t p = blockIdx.x * SRX_BLOCK + threadIdx.x;
	const uint32_t q = p < in.s.n ? srx_slot_at(L, p) : SP_K;
	bool late = false, dup = false;
	if (q < SP_K) {
		const uint32_t f0 = L.start[q], c = L.cnt[q];
		const struct tseg_rec st = L.rec[q];
		const int64_t H0 = tsrx_h0(st, sseq[f0]);
		const int64_t lix0 = (int64_t)tseg_lix(st);
		const int r = rx_settle(u + f0, mx + f0, p - f0, sseq[p],
					in.lookback, H0, lix0, tseg_bitmap(st), 1);
		if (r == RX_UNSETTLED) {
			atomicOr(&out->tab.base.fail, (uint32_t)SPF_ORDER);
		}
		else {
			const int64_t ui = u[p];
			const uint32_t i = perm[p];
			desc[i] = d_desc((uint64_t)ui, tsrx_fl(r, (int)in.hmac));
			rs[i] = (uint8_t)r;
			dup = r == RX_DUP;
			if (!dup) {
				const int64_t smx = tsrx_smx(u[f0 + c - 1],
							     mx[f0 + c - 1]);
				const uint64_t bit = tsrx_bit(st, smx, ui);
				if (bit)
					atomicOr((unsigned long long *)&out->bits[q],
						 (unsigned long long)bit);
				late = tsrx_late(ui, lix0, mx[p]);
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

/* the touched streams' records after the batch; per-class launch guards,
 * once every packet is settled (k_rx_final) */
__global__ void __launch_bounds__(64)
k_srx_final(const struct sgpu_srxplan_in in, const uint16_t *sseq,
	    const int64_t *u, const int64_t *mx, struct sgpu_srxplan_out *out)
{
	__shared__ struct srx_lds L;
	srx_stage(in, out, L);
	const uint32_t t = threadIdx.x;
	if (t < SP_K && !L.fail && L.cnt[t]) {
		const uint32_t f0 = L.start[t], c = L.cnt[t];
		const struct tseg_rec st = L.rec[t];
		const struct tseg_rec a =
			tsrx_after(st, tsrx_h0(st, sseq[f0]),
				   tsrx_smx(u[f0 + c - 1], mx[f0 + c - 1]),
				   out->bits[t]);
		struct sgpu_rtp_rec r;
		r.ssrc = a.ssrc; r.roc = a.roc; r.sl = a.sl; r.pad = 0;
		r.llo = a.llo; r.lhi = a.lhi; r.blo = a.blo; r.bhi = a.bhi;
		out->after[t] = r;
	}
	if (t < 4)
		out->tab.base.skip[t] =
			L.fail || (((out->tab.base.hl0 >> 2) & 3u) != t);
}

__global__ void __launch_bounds__(SRX_BLOCK)
k_srx_commit(const struct sgpu_srxplan_out *out, const struct sgpu_hdr *hdr,
	     const uint8_t *rs, const uint32_t *es, uint32_t *pos,
	     uint32_t *end, int32_t *err, uint32_t n, uint32_t tag)
{
	const uint32_t i = blockIdx.x * SRX_BLOCK + threadIdx.x;
	if (i >= n || out->tab.base.fail || out->tab.base.nfail)
		return;
	end[i] = es[i] - tag;
	if (rs[i] == RX_DUP) {
		/* srtp.c:355-368 / 413-422: pos at the payload */
		pos[i] += hdr[i].hdr_len;
		err[i] = EALREADY;
	}
	else {
		err[i] = 0;
	}
}

/* ---- host side ------------------------------------------------------ */

/* the table launches' scratch | slot[] | per workgroup and slot counts |
 * perm[] | sseq[] | workgroup aggregates | u[] | mx[] | verdict bytes */
struct srx_scratch {
	uint8_t *tab, *slot, *rs;
	uint32_t *bcnt, *perm;
	uint16_t *sseq;
	struct rx_seg *agg;
	int64_t *u, *mx;
	size_t bytes;
};

static struct srx_scratch srx_layout(void *scratch, uint32_t n)
{
	const size_t nb = ((size_t)n + SRX_BLOCK - 1) / SRX_BLOCK;
	struct srx_scratch s;
	uint8_t *p = (uint8_t *)scratch;
	s.tab = p;
	p += sp_al(sgpu_splan_table_scratch(n));
	s.slot = p;
	p += sp_al(n);
	s.bcnt = (uint32_t *)p;
	p += sp_al(nb * SP_K * 4);
	s.perm = (uint32_t *)p;
	p += sp_al((size_t)n * 4);
	s.sseq = (uint16_t *)p;
	p += sp_al((size_t)n * 2);
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

extern "C" unsigned sgpu_splan_rx_block(void)
{
	return SRX_BLOCK;
}

extern "C" size_t sgpu_splan_rx_scratch(uint32_t n)
{
	return srx_layout(NULL, n).bytes;
}

extern "C" int sgpu_splan_rx(const struct sgpu_srxplan_in *in,
			     const struct sgpu_hdr *hdr, const uint32_t *pos,
			     const uint32_t *end, const uint32_t *cap,
			     uint64_t arena_size, uint64_t *desc, void *scratch,
			     size_t scratch_bytes, struct sgpu_srxplan_out *out,
			     void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	const uint32_t n = in->s.n;
	const uint32_t nb = (n + SRX_BLOCK - 1) / SRX_BLOCK;
	if (!n || in->s.nst > SP_K || in->s.prot ||
	    scratch_bytes < sgpu_splan_rx_scratch(n))
		return EINVAL;
	const struct srx_scratch s = srx_layout(scratch, n);
	if (!in->s.zeroed &&
	    hipMemsetAsync(out, 0, sizeof(*out), st) != hipSuccess)
		return EIO;
	if (sgpu_splan_table(&in->s, hdr, s.tab, &out->tab, stream))
		return EIO;
	hipLaunchKernelGGL(k_srx_count, dim3(nb), dim3(SRX_BLOCK), 0, st, *in,
			   hdr, pos, end, cap, arena_size, s.slot, s.bcnt, out);
	hipLaunchKernelGGL(k_srx_starts, dim3(1), dim3(SRX_SCAN), 0, st, s.bcnt,
			   nb, out);
	hipLaunchKernelGGL(k_srx_place, dim3(nb), dim3(SRX_BLOCK), 0, st, n, hdr,
			   (const uint8_t *)s.slot, (const uint32_t *)s.bcnt,
			   (const struct sgpu_srxplan_out *)out, s.perm, s.sseq);
	hipLaunchKernelGGL(k_srx_agg, dim3(nb), dim3(SRX_BLOCK), 0, st, *in,
			   (const uint16_t *)s.sseq, s.agg, out);
	hipLaunchKernelGGL(k_srx_scan, dim3(1), dim3(SRX_SCAN), 0, st, s.agg, nb,
			   (const struct sgpu_srxplan_out *)out);
	hipLaunchKernelGGL(k_srx_index, dim3(nb), dim3(SRX_BLOCK), 0, st, *in,
			   (const uint16_t *)s.sseq, (const struct rx_seg *)s.agg,
			   (const struct sgpu_srxplan_out *)out, s.u, s.mx);
	hipLaunchKernelGGL(k_srx_settle, dim3(nb), dim3(SRX_BLOCK), 0, st, *in,
			   (const uint16_t *)s.sseq, (const uint32_t *)s.perm,
			   (const int64_t *)s.u, (const int64_t *)s.mx, desc, s.rs,
			   out);
	hipLaunchKernelGGL(k_srx_final, dim3(1), dim3(64), 0, st, *in,
			   (const uint16_t *)s.sseq, (const int64_t *)s.u,
			   (const int64_t *)s.mx, out);
	return hipGetLastError() == hipSuccess ? 0 : EIO;
}

extern "C" int sgpu_splan_rx_commit(const struct sgpu_srxplan_out *out,
				    const struct sgpu_hdr *hdr,
				    const void *scratch, const uint32_t *es,
				    uint32_t *pos, uint32_t *end, int32_t *err,
				    uint32_t n, uint32_t tag, void *stream)
{
	const uint32_t nb = (n + SRX_BLOCK - 1) / SRX_BLOCK;
	if (!n)
		return 0;
	const struct srx_scratch s = srx_layout((void *)scratch, n);
	hipLaunchKernelGGL(k_srx_commit, dim3(nb), dim3(SRX_BLOCK), 0,
			   (hipStream_t)stream, out, hdr, (const uint8_t *)s.rs, es,
			   pos, end, err, n, tag);
	return hipGetLastError() == hipSuccess ? 0 : EIO;
}
