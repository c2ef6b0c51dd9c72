/*
 * plan_bucket_common.h -- the per-bucket mechanics every many-session device
 * planner (plan_buckets*.hip) runs around its rule, stated once: a bucket's
 * entries in, the sessions' segments, the order inside a session, a packet's
 * slot in its session's stream table, the workgroup's segmented scan, the
 * finish kernels' tail, the record movers, the host's geometry check.
 *
 * A helper takes the LDS arrays it works on as arguments and knows nothing of
 * its caller.  One workgroup of BPB threads owns a bucket; every helper says
 * who calls it, which barriers it contains and expects, and which arrays are
 * dead behind it -- the planners' LDS unions rest on exactly that.
 */
#ifndef PLAN_BUCKET_COMMON_H
#define PLAN_BUCKET_COMMON_H

#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdio.h>
#include "../srtpgpu.h"
#include "plan_rtcp_seg_rx.h"
#include "plan_rtp_seg_rx.h"

#define BPB SGPU_BP_BLOCK
#define BP_IMASK 0x3ffffffu     /* entry: packet index | length bin << 26 */
#define BP_OBINS 64
#define BK_EPT (SGPU_BP_CAPMAX / BPB)   /* entries per thread, at most */
#define BK_NOWORD 0xffffffffu

/* the scatter kernels' grid: BPB threads, SGPU_BP_PPT packets each */
__host__ __device__ static inline uint32_t bk_grid(uint32_t n)
{
	return (n + BPB * SGPU_BP_PPT - 1) / (BPB * SGPU_BP_PPT);
}

/* ---- the record movers ------------------------------------------------ */

static_assert(sizeof(struct sgpu_sstate) == 32 &&
	      offsetof(struct sgpu_sstate, flags) == 12,
	      "a session state moves as two 16-byte words");
static_assert(sizeof(struct rseg_rec) == 16 &&
	      sizeof(struct sgpu_rtcp_rec) == 16 &&
	      offsetof(struct sgpu_rtcp_rec, blo) ==
	      offsetof(struct rseg_rec, blo),
	      "an SRTCP stream record moves as one 16-byte word");
static_assert(sizeof(struct tseg_rec) == 32 &&
	      sizeof(struct sgpu_rtp_rec) == 32 &&
	      offsetof(struct sgpu_rtp_rec, llo) ==
	      offsetof(struct tseg_rec, llo),
	      "an RTP stream record moves as two 16-byte words");

__device__ __forceinline__ struct sgpu_sstate bk_ld(const struct sgpu_sstate *p)
{
	const uint4 a = ((const uint4 *)p)[0], b = ((const uint4 *)p)[1];
	struct sgpu_sstate s;
	s.ssrc = a.x; s.roc = a.y; s.s_l = a.z; s.flags = a.w;
	s.lix = (uint64_t)b.y << 32 | b.x;
	s.bitmap = (uint64_t)b.w << 32 | b.z;
	return s;
}

__device__ __forceinline__ void bk_st(struct sgpu_sstate *p,
				      const struct sgpu_sstate &s)
{
	((uint4 *)p)[0] = make_uint4(s.ssrc, s.roc, s.s_l, s.flags);
	((uint4 *)p)[1] = make_uint4((uint32_t)s.lix, (uint32_t)(s.lix >> 32),
				     (uint32_t)s.bitmap,
				     (uint32_t)(s.bitmap >> 32));
}

__device__ __forceinline__ struct rseg_rec bk_ld(const struct sgpu_rtcp_rec *p)
{
	const uint4 a = *(const uint4 *)p;
	struct rseg_rec r;
	r.ssrc = a.x; r.ix = a.y; r.blo = a.z; r.bhi = a.w;
	return r;
}

__device__ __forceinline__ struct tseg_rec bk_ld(const struct sgpu_rtp_rec *p)
{
	const uint4 a = ((const uint4 *)p)[0], b = ((const uint4 *)p)[1];
	struct tseg_rec r;
	r.ssrc = a.x; r.roc = a.y; r.sl = a.z; r.pad = 0;
	r.llo = b.x; r.lhi = b.y; r.blo = b.z; r.bhi = b.w;
	return r;
}

__device__ __forceinline__ void bk_st(struct sgpu_rtp_rec *p,
				      const struct tseg_rec &r)
{
	((uint4 *)p)[0] = make_uint4(r.ssrc, r.roc, r.sl, 0u);
	((uint4 *)p)[1] = make_uint4(r.llo, r.lhi, r.blo, r.bhi);
}

/* ---- the plan kernels' front ------------------------------------------ */

/*
 * The bucket's entries into registers, entry tid + j * BPB in ev4[j] (zero
 * beyond *m), and the fail bits the bucket starts with.  Every thread of the
 * bucket's workgroup calls it first; no barrier, no LDS.  *m: the bucket's
 * count, 0 for a bucket over cap, so that nothing below indexes past the
 * region.
 */
__device__ __forceinline__ uint32_t
bk_entries(const uint32_t *afail, uint32_t n, uint32_t nb,
	   const uint32_t *bcount, const uint4 *tmp, uint32_t cap, uint32_t *m,
	   uint4 (&ev4)[BK_EPT])
{
	const uint32_t tid = threadIdx.x, b = blockIdx.x;
	uint32_t f = 0;
	*m = bcount[b];
	/* the scatter workgroups' fail words, spread over the buckets
	 * (no workgroup waits for another) */
	for (uint32_t k = b + tid * nb; k < bk_grid(n); k += BPB * nb)
		f |= afail[k];
	if (*m > cap) {
		f |= SPF_SEG;           /* (the scatter flagged it too) */
		*m = 0;
	}
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		ev4[j] = k < *m ? tmp[(size_t)b * cap + k]
				: make_uint4(0, 0, 0, 0);
	}
	return f;
}

/*
 * The stream tables' per-session words from toff[] (thread l: session s0 + l
 * of the bucket's ns; t0, where the session's records lie, only if the caller
 * keeps it), cnt[] zeroed for bk_sort, and the per-stream accumulators zeroed
 * (SGPU_BP_NSB * RSEG_MAX words each).  Returns SPF_BAD for a table toff[]
 * cannot describe.  Every thread calls it; it contains no barrier and the
 * caller places one before anything reads these arrays.
 */
__device__ __forceinline__ uint32_t
bk_tables(const uint32_t *toff, uint32_t s0, uint32_t ns, uint32_t *t0,
	  uint32_t *nk, uint32_t *nst, uint32_t *cnt, uint32_t *tmask,
	  uint32_t *acc, uint32_t *wlo, uint32_t *whi)
{
	const uint32_t tid = threadIdx.x;
	uint32_t f = 0;
	if (tid < ns) {
		const uint32_t a = toff[s0 + tid], e = toff[s0 + tid + 1];
		uint32_t k = e - a;
		if (e < a || k > RSEG_MAX) {
			f = SPF_BAD;    /* (the host builds toff: never) */
			k = 0;
		}
		if (t0)
			t0[tid] = a;
		nk[tid] = k;
		nst[tid] = k;
		cnt[tid] = 0;
		tmask[tid] = 0;
	}
	for (uint32_t q = tid; q < SGPU_BP_NSB * RSEG_MAX; q += BPB) {
		acc[q] = 0;
		wlo[q] = 0;
		whi[q] = 0;
	}
	return f;
}

/*
 * start[l] = the sum of cnt[0 .. l) over the bucket's ns sessions (beyond
 * ns: the bucket's count).  Every thread may call it, wave 0 works; no
 * barrier inside.  A barrier lies between the last update of cnt[] and the
 * call, and another between the call and the first reader of start[].
 */
__device__ __forceinline__ void bk_starts(const uint32_t *cnt, uint32_t *start,
					  uint32_t ns)
{
	const uint32_t tid = threadIdx.x;
	/* segment starts (sessions, <= 256: wave 0) */
	if (tid < 64) {
		uint32_t c4[4], v = 0;
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const uint32_t l = 4 * tid + q;
			c4[q] = l < ns ? cnt[l] : 0u;
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
				start[l] = run;
			run += c4[q];
		}
	}
}

/* the session-in-bucket byte of an entry's second word, ksh bits up */
__device__ __forceinline__ uint32_t bk_key(uint4 e, uint32_t ksh)
{
	return e.y >> ksh & 0xffu;
}

/*
 * The entries grouped by session and ranked by packet index (ev4[j].x)
 * inside each session, the order the reference sees them in: pos[j] is the
 * sorted position of ev4[j] (for k = tid + j * BPB < m of a plan that lives),
 * and the caller stores whatever it keeps per position there.  f: the
 * thread's fail bits so far; they and SPF_SEG for a session over
 * SGPU_BP_SEGMAX go into *bf.  Returns whether the plan is dead (*bf set).
 *
 * Every thread calls it, behind a barrier behind cnt[] = 0 and *bf = 0.  It
 * contains three barriers; start[] and cnt[] are final behind the second.
 * It ends without one: grp[] (the packet indices grouped by session, m
 * words) is still being read, and is dead behind the caller's next barrier,
 * which also publishes the caller's stores.
 */
__device__ __forceinline__ bool
bk_sort(const uint4 (&ev4)[BK_EPT], uint32_t ksh, uint32_t m, uint32_t ns,
	uint32_t f, uint32_t *cnt, uint32_t *start, uint32_t *grp, uint32_t *bf,
	uint32_t (&pos)[BK_EPT])
{
	const uint32_t tid = threadIdx.x;
	/* rank in session (unstable) */
	uint32_t ru[BK_EPT];
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		ru[j] = 0;
		if (k < m)
			ru[j] = atomicAdd(&cnt[bk_key(ev4[j], ksh)], 1u);
	}
	__syncthreads();
	bk_starts(cnt, start, ns);
	if (tid < ns && cnt[tid] > SGPU_BP_SEGMAX)
		f |= SPF_SEG;
	if (f)
		atomicOr(bf, f);
	__syncthreads();
	const bool dead = *bf != 0;     /* the plan fails: nothing more */
	if (!dead) {
		/* grouped by session */
#pragma unroll
		for (int j = 0; j < BK_EPT; j++) {
			const uint32_t k = tid + j * BPB;
			if (k < m)
				grp[start[bk_key(ev4[j], ksh)] + ru[j]] = ev4[j].x;
		}
	}
	__syncthreads();
	/* inside a session by packet index */
#pragma unroll
	for (int j = 0; j < BK_EPT; j++) {
		const uint32_t k = tid + j * BPB;
		pos[j] = 0;
		if (dead || k >= m)
			continue;
		const uint32_t l = bk_key(ev4[j], ksh);
		const uint32_t f0 = start[l], c = cnt[l];
		uint32_t r = 0;
		for (uint32_t t = f0; t < f0 + c; t++)
			r += grp[t] < ev4[j].x ? 1u : 0u;
		pos[j] = f0 + r;
	}
	return dead;
}

/*
 * The same order through 16-bit indirection, for the planners that keep the
 * entries where they arrived (ent[k]: packet index | bin << 26, sl[k]: the
 * session) and sort indices to them: srt[k] comes in as entry k's unstable
 * rank in its session and leaves as the entry at sorted position k.  Every
 * thread calls it with the same dead, behind the barrier that makes start[]
 * visible.  One barrier inside, none at the end: the caller's next barrier
 * publishes srt[], and un[] is dead behind it.
 */
__device__ __forceinline__ void
bk_sort16(uint32_t m, bool dead, const uint32_t *ent, const uint8_t *sl,
	  const uint32_t *cnt, const uint32_t *start, uint16_t *un,
	  uint16_t *srt)
{
	const uint32_t tid = threadIdx.x;
	if (!dead) {
		/* grouped by session */
#pragma unroll
		for (int j = 0; j < BK_EPT; j++) {
			const uint32_t k = tid + j * BPB;
			if (k >= m)
				continue;
			un[start[sl[k]] + srt[k]] = (uint16_t)k;
		}
	}
	__syncthreads();
	if (!dead) {
		/* inside a session by packet index: the stable order the
		 * reference processes them in */
		for (uint32_t q = tid; q < m; q += BPB) {
			const uint32_t e = un[q], l = sl[e];
			const uint32_t f0 = start[l], c = cnt[l];
			const uint32_t ie = ent[e] & BP_IMASK;
			uint32_t r = 0;
			for (uint32_t t = f0; t < f0 + c; t++)
				r += (ent[un[t]] & BP_IMASK) < ie ? 1u : 0u;
			srt[f0 + r] = (uint16_t)e;
		}
	}
}

/* ---- a packet's stream ------------------------------------------------ */

/*
 * Pass 1 of the receive planners, which hold only the tables' SSRCs: sorted
 * position k of session l (its segment starts at f0) looks back over
 * ssrc[f0 .. k) for its rank among its stream's arrivals and its stream's
 * first position, and finds its known slot in the nk SSRCs of tss.  Writes
 * opens[k].  Per position, no barrier; ssrc[] is published by a barrier
 * before, opens[] by one behind.  Returns the known slot or RSEG_NONE.
 */
__device__ __forceinline__ uint32_t
bk_look(uint32_t k, uint32_t f0, const uint32_t *ssrc, const uint32_t *tss,
	uint32_t nk, uint8_t *opens, uint32_t *rank, uint32_t *first)
{
	const uint32_t x = ssrc[k];
	struct rseg_look lk = rseg_look_init(k);
	const uint32_t kn = rsrx_known(tss, nk, x);
	for (uint32_t t = f0; t < k; t++)
		lk = rseg_look_step(lk, t, ssrc[t] == x);
	opens[k] = (uint8_t)rseg_opens(kn, lk);
	*rank = lk.rank;
	*first = lk.first;
	return kn;
}

/*
 * Pass 2's slot of a packet whose known slot is kn and whose stream first
 * appears at sorted position first, in a session of nk known streams whose
 * segment starts at f0: new SSRCs lie behind the known ones in
 * first-appearance order (rseg_enosr(slot): a 9th stream, the caller's
 * SPF_SSRC).  Per position, no barrier; a barrier lies between pass 1's
 * opens[] and the call.
 */
__device__ __forceinline__ uint32_t
bk_slot(uint32_t kn, uint32_t first, uint32_t f0, uint32_t nk,
	const uint8_t *opens)
{
	uint32_t nnew = 0;
	if (kn == RSEG_NONE)
		for (uint32_t t = f0; t < first; t++)
			nnew += opens[t];
	return rseg_slot(kn, nk, nnew);
}

/*
 * ... and the marks it leaves on session l: the table's length after the
 * batch if the packet opens the stream, the stream touched, its accumulator
 * (*acc) raised to v.  Atomics only: the values are final behind the caller's
 * next barrier.
 */
__device__ __forceinline__ void
bk_touch(uint32_t l, uint32_t slot, int opens, uint32_t v, uint32_t *nst,
	 uint32_t *tmask, uint32_t *acc)
{
	if (opens)
		atomicMax(&nst[l], slot + 1u);
	atomicOr(&tmask[l], 1u << slot);
	atomicMax(acc, v);
}

/* ---- the workgroup's segmented (sum, max) scan ------------------------ */

__device__ __forceinline__ struct rx_seg bk_shfl_up(struct rx_seg v, int d)
{
	struct rx_seg r;
	r.a.s = __shfl_up((long long)v.a.s, d);
	r.a.m = __shfl_up((long long)v.a.m, d);
	r.head = (uint32_t)__shfl_up((int)v.head, d);
	return r;
}

/*
 * Exclusive segmented scan of one element per thread over the workgroup: in
 * the wave by shuffles, across the 16 waves through their aggregates in
 * wagg[BPB / 64].  Every thread calls it, in uniform control flow.  Two
 * barriers inside: whatever the callers wrote before is visible behind it,
 * whatever they read before may be overwritten (the planners' u[] / mx[]
 * take the sorted arrays' place here); wagg[] is free again on return.
 */
__device__ __forceinline__ struct rx_seg bk_excl_scan(struct rx_seg v,
						      struct rx_seg *wagg)
{
	const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
	struct rx_seg x = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const struct rx_seg y = bk_shfl_up(x, d);
		if (lane >= (uint32_t)d)
			x = rx_seg_combine(y, x);
	}
	if (lane == 63)
		wagg[wv] = x;
	struct rx_seg below = bk_shfl_up(x, 1);
	if (lane == 0)
		below = rx_seg_identity();
	__syncthreads();
	struct rx_seg pre = rx_seg_identity();
	for (uint32_t q = 0; q < wv; q++)
		pre = rx_seg_combine(pre, wagg[q]);
	__syncthreads();
	return rx_seg_combine(pre, below);
}

/* ---- the finish kernels' tail (workgroup 0) ---------------------------- */

/*
 * The buckets' late / duplicate counts (cnt[2 * b], cnt[2 * b + 1]) summed
 * into tot[0], tot[1] in LDS.  Every thread of the workgroup calls it; two
 * barriers inside, the second behind the last add: thread 0 may read tot[]
 * at once.
 */
__device__ __forceinline__ void bk_counts(const uint32_t *cnt, uint32_t nb,
					  uint32_t *tot)
{
	const uint32_t tid = threadIdx.x;
	uint32_t a = 0, d = 0;
	if (tid < 2)
		tot[tid] = 0;
	__syncthreads();
	for (uint32_t q = tid; q < nb; q += BPB) {
		a += cnt[2 * q];
		d += cnt[2 * q + 1];
	}
	if (a)
		atomicAdd(&tot[0], a);
	if (d)
		atomicAdd(&tot[1], d);
	__syncthreads();
}

/*
 * The call's outcome (the plan out and what lies behind it, bytes in all) to
 * the caller's pinned mirror with vector stores, once it is final: no blit
 * copy behind the launch.  Every thread calls it; no barrier inside, so the
 * caller has one between its last store to out and the call -- or names that
 * store: word wn is taken from v, not from memory (BK_NOWORD: none).
 */
__device__ __forceinline__ void bk_post(const void *out, uint32_t *outh,
					uint32_t bytes, uint32_t wn, uint32_t v)
{
	if (!outh)
		return;
	const uint32_t *src = (const uint32_t *)out;
	for (uint32_t w = threadIdx.x; w < bytes / 4u; w += BPB)
		outh[w] = w == wn ? v : src[w];
}

/* ---- host side ------------------------------------------------------ */

/* the bucket geometry every launch checks: n packets of nsess sessions in nb
 * buckets of 2^bshift sessions and cap entries each, the last one part full */
static int bk_geom_bad(uint32_t n, uint32_t nsess, uint32_t nb,
		       uint32_t bshift, uint32_t cap)
{
	return !n || n > SGPU_BP_NMAX || nsess < 2 || !nb ||
	       nb > SGPU_BP_NBMAX || bshift > 8 || !cap ||
	       cap > SGPU_BP_CAPMAX || cap % BPB ||
	       ((uint64_t)nb << bshift) < nsess ||
	       ((uint64_t)(nb - 1) << bshift) >= nsess;
}

static int bk_err(const char *what)
{
	const hipError_t e = hipGetLastError();
	if (e == hipSuccess)
		return 0;
	fprintf(stderr, "re_srtp: %s launch: %s\n", what, hipGetErrorString(e));
	return EIO;
}

#endif
