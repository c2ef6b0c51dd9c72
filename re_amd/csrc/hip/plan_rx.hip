/*
 * plan_rx.hip -- exact device plan of a single-stream RTP unprotect batch
 * whose packets arrive reordered, duplicated or with gaps (srtpgpu.h
 * sgpu_plan_rx; the rule and why it is exact: plan_rx_rule.h).
 *
 * The in-order planners (k_plan_*, k_ctr_fused.h, k_lp_plan) reject such a
 * batch with SPF_ORDER / SPF_REPLAY; this one runs behind that rejection.
 * Five launches, no workgroup waits for another:
 *
 *   k_rx_agg     per packet the window checks of k_plan_count (parse, one
 *                SSRC, one header class, size, window validity, tag room)
 *                and its scan element; per workgroup the (sum, max)
 *                aggregate of its RX_BLOCK elements
 *   k_rx_scan    one workgroup: exclusive scan of the aggregates; the final
 *                state (roc, s_l, lix, the moved pre-batch bitmap)
 *   k_rx_index   per packet u[i] (speculated index) and Mx[i] (maximum of
 *                the indices before it) into the workspace
 *   k_rx_settle  per packet the verification and the replay verdict
 *                (rx_settle: reads u[i - K .. i), across workgroups), desc
 *                as scan_dec (batch_host.c) writes it, its verdict byte,
 *                its bit of the final replay window (atomicOr)
 *   k_rx_final   the crypto launches' class guards skip[]
 *
 * and, behind the crypto launches, k_rx_commit: the caller's pos / end /
 * err, only if the plan held (fail == 0) and every tag verified
 * (nfail == 0) -- a rejected plan modifies nothing.
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdio.h>
#include "../srtpgpu.h"
#include "plan_rx_rule.h"

#define RX_BLOCK 256

/* sgpu_desc() (srtpgpu.h) on the device */
__device__ __forceinline__ uint64_t rx_desc(int64_t ix, uint32_t flags)
{
	return ((uint64_t)ix & 0xffffffffffffull) | ((uint64_t)flags << 48);
}

/* the receiver's state before the batch as one number (stream_get_seq:
 * a fresh stream takes packet 0's sequence number as s_l) */
__device__ __forceinline__ int64_t rx_h0(const struct sgpu_rxplan_in &in,
					 const struct sgpu_hdr *hdr)
{
	const uint32_t s_l = in.fresh ? hdr[0].seq : (in.s_l & 0xffffu);
	return (int64_t)(((uint64_t)in.roc << 16) | s_l);
}

/* packet i's scan element; *bad: packet 0 does not pass the reference step */
__device__ __forceinline__ struct rx_agg
rx_elem_of(const struct sgpu_rxplan_in &in, const struct sgpu_hdr *hdr,
	   uint32_t i, bool *bad)
{
	if (i >= in.n)
		return rx_identity();
	if (i == 0) {
		int64_t u0 = 0;
		int bump = 0;
		if (rx_step(rx_h0(in, hdr), hdr[0].seq, &u0, &bump)) {
			*bad = true;
			u0 = 0;
		}
		return rx_elem(u0);
	}
	return rx_elem(rx_sdiff16(hdr[i].seq, hdr[i - 1].seq));
}

/* inclusive scan of one element per thread over the workgroup (blockDim.x
 * threads, a power of two, sh[] of as many); sh[] then holds every
 * thread's inclusive value */
__device__ __forceinline__ struct rx_agg
rx_block_scan(struct rx_agg e, struct rx_agg *sh)
{
	const uint32_t t = threadIdx.x;
	sh[t] = e;
	__syncthreads();
	for (uint32_t d = 1; d < blockDim.x; d <<= 1) {
		struct rx_agg v = rx_identity();
		if (t >= d)
			v = sh[t - d];
		__syncthreads();
		e = rx_combine(v, e);
		sh[t] = e;
		__syncthreads();
	}
	return e;
}

__global__ void __launch_bounds__(RX_BLOCK)
k_rx_agg(const struct sgpu_rxplan_in in, const struct sgpu_hdr *hdr,
	 const uint32_t *pos, const uint32_t *end, const uint32_t *cap,
	 uint64_t asz, struct rx_agg *agg, struct sgpu_rxplan_out *out)
{
	__shared__ struct rx_agg sh[RX_BLOCK];
	const uint32_t i = blockIdx.x * RX_BLOCK + threadIdx.x;
	bool bad = false;
	uint32_t f = 0;
	if (i < in.n) {
		const struct sgpu_hdr h = hdr[i];
		const uint32_t hl0 = hdr[0].hdr_len;
		const uint32_t ssrc0 = in.ssrc_any ? hdr[0].ssrc : in.ssrc;
		const uint32_t p = pos[i], e = end[i];
		if (h.hdr_len == 0xffffffffu || hl0 == 0xffffffffu)
			f |= SPF_PARSE;
		else if (((h.hdr_len ^ hl0) >> 2) & 3u)
			f |= SPF_CLASS;
		if (h.ssrc != ssrc0)
			f |= SPF_SSRC;
		if ((p & 3u) || p > e || e > asz ||
		    (cap && (e > cap[i] || cap[i] > asz)))
			f |= SPF_BAD;
		else if (h.hdr_len != 0xffffffffu &&
			 (e - p < h.hdr_len || e - p - h.hdr_len < in.tag))
			f |= SPF_PARSE;
		if (e - p >= in.maxlen)
			f |= SPF_SIZE;
		if (i == 0) {
			out->ssrc0 = h.ssrc;
			out->hl0 = h.hdr_len;
		}
	}
	const struct rx_agg a = rx_block_scan(rx_elem_of(in, hdr, i, &bad), sh);
	if (bad)
		f |= SPF_TIMEOUT;
	if (f)
		atomicOr(&out->fail, f);
	if (threadIdx.x == RX_BLOCK - 1)
		agg[blockIdx.x] = a;
}

/* exclusive scan of the nb workgroup aggregates (one workgroup), as
 * k_plan_scan; the state after the batch from the total */
__global__ void __launch_bounds__(1024)
k_rx_scan(const struct sgpu_rxplan_in in, const struct sgpu_hdr *hdr,
	  struct rx_agg *agg, uint32_t nb, struct sgpu_rxplan_out *out)
{
	__shared__ struct rx_agg part[1024];
	const uint32_t per = (nb + 1023u) / 1024u;
	const uint32_t a = threadIdx.x * per;
	struct rx_agg sum = rx_identity();
	for (uint32_t k = a; k < a + per && k < nb; k++)
		sum = rx_combine(sum, agg[k]);
	const struct rx_agg incl = rx_block_scan(sum, part);
	__syncthreads();
	struct rx_agg run = threadIdx.x ? part[threadIdx.x - 1] : rx_identity();
	for (uint32_t k = a; k < a + per && k < nb; k++) {
		const struct rx_agg v = agg[k];
		agg[k] = run;
		run = rx_combine(run, v);
	}
	if (threadIdx.x == 1023) {
		const int64_t H0 = rx_h0(in, hdr), lix0 = (int64_t)in.lix;
		const int64_t Mn = rx_max(H0, incl.m);
		const int64_t lix = rx_max(lix0, incl.m);
		out->roc = (uint32_t)((uint64_t)Mn >> 16);
		out->s_l = (uint32_t)((uint64_t)Mn & 0xffffu);
		out->lix = (uint64_t)lix;
		out->bitmap = rx_bitmap_base(lix, lix0, in.bitmap);
	}
}

__global__ void __launch_bounds__(RX_BLOCK)
k_rx_index(const struct sgpu_rxplan_in in, const struct sgpu_hdr *hdr,
	   const struct rx_agg *pre, int64_t *u, int64_t *mx)
{
	__shared__ struct rx_agg sh[RX_BLOCK];
	const uint32_t i = blockIdx.x * RX_BLOCK + threadIdx.x;
	bool bad = false;
	const struct rx_agg p = pre[blockIdx.x];
	const struct rx_agg a = rx_block_scan(rx_elem_of(in, hdr, i, &bad), sh);
	if (i >= in.n)
		return;
	const struct rx_agg ex = threadIdx.x ? sh[threadIdx.x - 1] : rx_identity();
	u[i] = p.s + a.s;
	mx[i] = rx_combine(p, ex).m;
}

__global__ void __launch_bounds__(RX_BLOCK)
k_rx_settle(const struct sgpu_rxplan_in in, const struct sgpu_hdr *hdr,
	    const int64_t *u, const int64_t *mx, uint64_t *desc, uint8_t *rs,
	    struct sgpu_rxplan_out *out)
{
	const uint32_t i = blockIdx.x * RX_BLOCK + threadIdx.x;
	/* a check of k_rx_agg failed: the indices mean nothing */
	if (i >= in.n || out->fail)
		return;
	const int64_t lix0 = (int64_t)in.lix;
	const int r = rx_settle(u, mx, i, hdr[i].seq, in.lookback,
				rx_h0(in, hdr), lix0, in.bitmap, 1);
	if (r == RX_UNSETTLED) {
		atomicOr(&out->fail, (uint32_t)SPF_ORDER);
		return;
	}
	const int64_t ui = u[i];
	/* scan_dec (batch_host.c): an EALREADY packet's MAC is still checked
	 * (HMAC suites: not decrypted; GCM decrypts to authenticate) */
	desc[i] = rx_desc(ui, r == RX_DUP && in.hmac ? SD_RUN
						     : SD_RUN | SD_CIPHER);
	rs[i] = (uint8_t)r;
	if (r == RX_DUP) {
		atomicAdd(&out->ndup, 1u);
		return;
	}
	const uint64_t bit = rx_bit((int64_t)out->lix, ui);
	if (bit)
		atomicOr((unsigned long long *)&out->bitmap,
			 (unsigned long long)bit);
	if (ui < rx_max(lix0, mx[i]))
		atomicAdd(&out->nlate, 1u);
}

/* per-class launch guards, once every packet is settled (k_plan_final) */
__global__ void k_rx_final(struct sgpu_rxplan_out *out)
{
	if (threadIdx.x < 4)
		out->skip[threadIdx.x] =
			out->fail || (((out->hl0 >> 2) & 3u) != threadIdx.x);
}

__global__ void __launch_bounds__(RX_BLOCK)
k_rx_commit(const struct sgpu_rxplan_out *out, const struct sgpu_hdr *hdr,
	    const uint8_t *rs, const uint32_t *es, uint32_t *pos,
	    uint32_t *end, int32_t *err, uint32_t n, uint32_t tag)
{
	const uint32_t i = blockIdx.x * RX_BLOCK + threadIdx.x;
	if (i >= n || out->fail || out->nfail)
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

static size_t rx_align(size_t v)
{
	return (v + 63u) & ~(size_t)63;
}

extern "C" size_t sgpu_plan_rx_scratch(uint32_t n)
{
	const size_t nb = ((size_t)n + RX_BLOCK - 1) / RX_BLOCK;
	return 2 * rx_align((size_t)n * 8) + rx_align((nb + 1) * 16) +
	       rx_align(n);
}

extern "C" int sgpu_plan_rx(const struct sgpu_rxplan_in *in,
			    const struct sgpu_hdr *hdr, const uint32_t *pos,
			    const uint32_t *end, const uint32_t *cap,
			    uint64_t arena_size, uint64_t *desc, void *scratch,
			    size_t scratch_bytes, struct sgpu_rxplan_out *out,
			    void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	const uint32_t n = in->n;
	const uint32_t nb = (n + RX_BLOCK - 1) / RX_BLOCK;
	uint8_t *w = (uint8_t *)scratch;
	if (!n || scratch_bytes < sgpu_plan_rx_scratch(n))
		return EINVAL;
	int64_t *u = (int64_t *)w;
	int64_t *mx = (int64_t *)(w + rx_align((size_t)n * 8));
	struct rx_agg *agg = (struct rx_agg *)(w + 2 * rx_align((size_t)n * 8));
	uint8_t *rs = (uint8_t *)agg + rx_align(((size_t)nb + 1) * 16);
	if (!in->zeroed &&
	    hipMemsetAsync(out, 0, sizeof(*out), st) != hipSuccess)
		return EIO;
	hipLaunchKernelGGL(k_rx_agg, dim3(nb), dim3(RX_BLOCK), 0, st, *in, hdr,
			   pos, end, cap, arena_size, agg, out);
	hipLaunchKernelGGL(k_rx_scan, dim3(1), dim3(1024), 0, st, *in, hdr, agg,
			   nb, out);
	hipLaunchKernelGGL(k_rx_index, dim3(nb), dim3(RX_BLOCK), 0, st, *in, hdr,
			   (const struct rx_agg *)agg, u, mx);
	hipLaunchKernelGGL(k_rx_settle, dim3(nb), dim3(RX_BLOCK), 0, st, *in,
			   hdr, (const int64_t *)u, (const int64_t *)mx, desc, rs,
			   out);
	hipLaunchKernelGGL(k_rx_final, dim3(1), dim3(64), 0, st, out);
	return hipGetLastError() == hipSuccess ? 0 : EIO;
}

extern "C" int sgpu_plan_rx_commit(const struct sgpu_rxplan_out *out,
				   const struct sgpu_hdr *hdr,
				   const void *scratch, const uint32_t *es,
				   uint32_t *pos, uint32_t *end, int32_t *err,
				   uint32_t n, uint32_t tag, void *stream)
{
	const uint32_t nb = (n + RX_BLOCK - 1) / RX_BLOCK;
	const uint8_t *w = (const uint8_t *)scratch;
	const uint8_t *rs = w + 2 * rx_align((size_t)n * 8) +
			    rx_align(((size_t)nb + 1) * 16);
	if (!n)
		return 0;
	hipLaunchKernelGGL(k_rx_commit, dim3(nb), dim3(RX_BLOCK), 0,
			   (hipStream_t)stream, out, hdr, rs, es, pos, end, err,
			   n, tag);
	return hipGetLastError() == hipSuccess ? 0 : EIO;
}
