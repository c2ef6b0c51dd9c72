/*
 * rtp_stats_common.h -- what the per-session kernels of rtp_stats.hip and
 * rtcp_sess.hip share: eight lanes per session (the group ballot, a
 * session's run in the grouped order) and, on the host side, the radix
 * sort's sizes and the one scratch that is kept between calls.
 */
#ifndef RTP_STATS_COMMON_H
#define RTP_STATS_COMMON_H

#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <mutex>
#include "re_rtp_stats_batch.h"
#include "rtp_rx_rule.h"

namespace {

constexpr uint32_t RRX_BLOCK = 256;
constexpr uint32_t RRX_LANES = RTP_RX_MAX_MEMBERS;      /* per session */

static_assert(sizeof(struct rtp_rx_source) == 88 &&
	      sizeof(struct rtp_rx_sess) == 8 + 8 * 88 &&
	      sizeof(struct rrx_rec) == 20 && RRX_LANES == 8 &&
	      RRX_BLOCK % 64 == 0, "layouts of re_rtp_stats_batch.h");

/* the 8 ballot bits of this lane's group */
__device__ __forceinline__ uint32_t group_ballot(int pred)
{
	const uint32_t lane = threadIdx.x & 63;
	return (uint32_t)(__ballot(pred) >> (lane & ~7u)) & 0xffu;
}

/* first index in keys[0 .. n) (ascending) with keys[i] >= v */
__device__ __forceinline__ uint32_t lower_bound(const uint32_t *keys,
						uint32_t n, uint32_t v)
{
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (keys[mid] < v)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

/* a session's run [lo, hi) of the grouped order; no keys: one run, s = 0 */
__device__ __forceinline__ void run_of(const uint32_t *keys, uint32_t n,
				       uint32_t s, uint32_t &lo, uint32_t &hi)
{
	if (keys) {
		lo = lower_bound(keys, n, s);
		hi = lower_bound(keys, n, s + 1);
	}
	else {
		lo = 0;
		hi = s ? 0 : n;
	}
}

/* ---- host side ---------------------------------------------------------- */

inline size_t al(size_t x)
{
	return (x + 255) & ~(size_t)255;
}

inline uint32_t key_bits(uint32_t nsess)
{
	uint32_t b = 1;
	while (b < 32 && (nsess >> b))
		b++;
	return b;
}

inline size_t sort_bytes(uint32_t n, uint32_t bits)
{
	size_t tb = 0;
	(void)rocprim::radix_sort_pairs((void *)NULL, tb,
					(const uint32_t *)NULL,
					(uint32_t *)NULL,
					(const uint32_t *)NULL,
					(uint32_t *)NULL, n, 0, bits);
	return tb ? tb : 1;
}

inline uint32_t blocks(uint64_t threads)
{
	return (uint32_t)((threads + RRX_BLOCK - 1) / RRX_BLOCK);
}

} /* namespace */

/*
 * The scratch both files' calls use, one per device, kept between calls
 * and only growing (defined once, in rtp_stats.hip).  With rrx_mu held:
 * rrx_scratch_get gives >= bytes, ordered on the device behind the last
 * use; rrx_scratch_put records that use's end.
 */
struct rrx_scratch {
	void *p;
	size_t size;
	hipEvent_t ev;          /* after the last use */
	bool used;
};

extern std::mutex rrx_mu;
int rrx_scratch_get(size_t bytes, hipStream_t st, struct rrx_scratch **sp);
int rrx_scratch_put(struct rrx_scratch *sc, hipStream_t st);

#endif
