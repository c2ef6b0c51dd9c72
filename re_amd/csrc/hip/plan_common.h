/*
 * plan_common.h -- the device-only helpers shared by the RTP planners
 * (srtp_kernels.hip, k_ctr_fused.h, plan_multi.hip, plan_streams.hip,
 * plan_buckets.hip): the RTP header parse and the decoupled look-back of
 * the one-launch single-stream planners.  The per-packet rules themselves
 * are plan_rule.h's.
 */
#pragma once
#include "kern_common.h"
#include "plan_rule.h"

/* one RTP header (rtp_hdr_decode, rtp.c:88-137) from a window of `left`
 * bytes at b (p: its arena offset, for the aligned fast load) */
__device__ __forceinline__ struct sgpu_hdr parse_rtp_hdr(const uint8_t *b,
							 uint32_t p,
							 uint32_t left)
{
	struct sgpu_hdr h;
	h.ssrc = 0; h.seq = 0; h.err_pos = 0; h.hdr_len = 0xffffffffu;
	if (left < 12)
		return h;
	uint32_t b0;
	if (!(p & 3u)) {
		const uint32_t w0 = *(const uint32_t *)b;
		const uint32_t w2 = *(const uint32_t *)(b + 8);
		b0 = w0 & 0xffu;
		h.seq = (uint16_t)((w0 >> 8 & 0xff00u) | (w0 >> 24));
		h.ssrc = __builtin_bswap32(w2);
	}
	else {
		b0 = b[0];
		h.seq = (uint16_t)(b[2] << 8 | b[3]);
		h.ssrc = (uint32_t)b[8] << 24 | (uint32_t)b[9] << 16 |
			 (uint32_t)b[10] << 8 | b[11];
	}
	const uint32_t cc = b0 & 0x0fu, x = (b0 >> 4) & 1u;
	uint32_t hl = 12;
	if (left - hl < 4 * cc) {
		h.err_pos = (uint16_t)hl;
		return h;
	}
	hl += 4 * cc;
	if (x) {
		if (left - hl < 4) {
			h.err_pos = (uint16_t)hl;
			return h;
		}
		const uint32_t xl = (uint32_t)b[hl + 2] << 8 | b[hl + 3];
		hl += 4;
		if (left - hl < 4 * xl) {
			h.err_pos = (uint16_t)hl;
			return h;
		}
		hl += 4 * xl;
	}
	h.hdr_len = hl;
	return h;
}

/* ---- decoupled look-back over per-workgroup words (fz_plan, k_lp_plan) -- */

/* SPF_* bits a look-back word carries (bits 32..45) */
#define FZ_FMASK 0x3fffu
static_assert((SPF_SLOW | SPF_SEG | SPF_PRED | 0x1ffu) <= FZ_FMASK, "fz_word");

/* epoch || state (1: the workgroup's own aggregate, 2: its inclusive
 * prefix) || fail bits || rollovers */
__device__ __forceinline__ uint64_t fz_word(uint32_t epoch, uint32_t st,
					    uint32_t fail, uint32_t wraps)
{
	return (uint64_t)epoch << 48 | (uint64_t)st << 46 |
	       (uint64_t)(fail & FZ_FMASK) << 32 | wraps;
}

__device__ __forceinline__ void fz_store(unsigned long long *w, uint64_t v)
{
	__hip_atomic_store(w, (unsigned long long)v, __ATOMIC_RELAXED,
			   __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t fz_load(unsigned long long *w)
{
	return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		v += (uint32_t)__shfl_xor((int)v, o);
	return v;
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		v |= (uint32_t)__shfl_xor((int)v, o);
	return v;
}

struct fz_prefix {
	uint32_t excl;          /* rollovers in the workgroups before t */
	uint32_t fail;          /* fail bits of workgroup t and those before */
};

/*
 * One whole wave of workgroup t (ticket order: every workgroup below t is
 * running or done), which counted tot rollovers and raised lf: publish the
 * aggregate, look back over the workgroups before it, 64 at a time, to the
 * nearest one that published its inclusive prefix, publish the own one,
 * and raise in *out_fail the bits that reject the plan from here (the own
 * ones; SPF_BAD | SPF_SLOW of the workgroups before).
 */
__device__ __forceinline__ struct fz_prefix
fz_lookback(unsigned long long *agg, uint32_t epoch, uint32_t t, uint32_t lane,
	    uint32_t lf, uint32_t tot, uint32_t *out_fail)
{
	uint32_t excl = 0, xf = 0;
	if (t != 0) {
		if (lane == 0)
			fz_store(&agg[t], fz_word(epoch, 1, lf, tot));
		int32_t j = (int32_t)t - 1;
		for (;;) {
			const int32_t k = j - (int32_t)lane;
			uint64_t w = 0;
			uint32_t st = 2;
			if (k >= 0) {
				/* every workgroup below t publishes before it
				 * waits; the bound (2^18 polls of s_sleep 1, ~64
				 * clocks each: ~7 ms at 2.4 GHz) only turns a
				 * stalled predecessor or a broken ticket count
				 * into a rejected plan (SPF_SLOW: the host
				 * re-plans, resets the counters and counts it
				 * apart from a bad window, "lbtimeouts") instead
				 * of a wave that never ends */
				for (uint32_t spin = 0;; spin++) {
					w = fz_load(&agg[k]);
					st = (uint32_t)(w >> 46) & 3u;
					if ((uint32_t)(w >> 48) == epoch && st != 0)
						break;
					if (spin > (1u << 18)) {
						w = fz_word(0, 2, SPF_SLOW, 0);
						st = 2;
						break;
					}
					__builtin_amdgcn_s_sleep(1);
				}
			}
			const uint64_t inc = __ballot(st == 2);
			const uint32_t first = inc ?
				(uint32_t)__ffsll((long long)inc) - 1u : 64u;
			const bool take = lane <= first;
			excl += wave_sum(take ? (uint32_t)w : 0u);
			xf |= wave_or(take ? (uint32_t)(w >> 32) & FZ_FMASK : 0u);
			if (inc)
				break;
			j -= 64;
		}
	}
	struct fz_prefix r;
	r.excl = excl;
	r.fail = lf | xf;
	if (lane == 0) {
		fz_store(&agg[t], fz_word(epoch, 2, r.fail, excl + tot));
		if (lf | (xf & (SPF_BAD | SPF_SLOW)))
			atomicOr(out_fail, lf | (xf & (SPF_BAD | SPF_SLOW)));
	}
	return r;
}
