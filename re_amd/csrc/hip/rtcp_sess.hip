/*
 * rtcp_sess.hip -- RTCP session state for batches in HBM: rtcp_handler over
 * decoded compounds, the transmit statistics, the SR / RR descriptors and
 * rtcp_stats (include/re_rtcp_sess_batch.h; the rule: rtcp_sess_rule.h).
 *
 * The handler works like rtp_stats.hip's walk.  k_rsx_keys gives every
 * packet its final stat when it takes no part (skipped, bad session,
 * truncated) and its grouping key; rocPRIM's stable radix sort of (key,
 * index) pairs puts a session's packets together in array order (without a
 * session array there is one run and no sort).  k_rsx_walk then takes eight
 * lanes per session, lane k holding member slot k -- its struct
 * rtp_rx_source and its cum_lost / jit / rtt -- in registers.  All eight
 * read the same descriptors and items; the sender's member is found by the
 * 8-bit group ballot, the one lane that owns it applies the SR and the
 * report blocks, and a BYE moves the state of the slots above the removed
 * one down the group with shuffles.  The workload is many sessions with one
 * to a few compounds each, so the parallelism is across sessions; a group's
 * work depends on its session alone, and no workgroup waits for another.
 *
 * The transmit statistics are a reduction, not a walk: per session the
 * number of accepted packets, their payload bytes and the lowest index
 * among them.  k_rsx_tx takes one lane per packet (several packets per lane
 * without a session array, summed in registers first); the lanes of a wave
 * that share a session combine with wave reductions, and one lane per
 * distinct session adds the wave's part to the session's accumulator with
 * three atomics.  Sums and minima of integers do not depend on the order,
 * so neither does the result.  k_rsx_tx_finish applies each accumulator to
 * its session (rsx_tx_finish) and re-reads the first packet's timestamp.
 *
 * The report is rtp_stats.hip's report kernel followed by k_rsx_report_msg,
 * which turns the RR descriptor into the SR where something was sent.
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>
#include <string.h>
#include "re_rtcp_sess_batch.h"
#include "../srtpgpu.h"
#include "rtcp_sess_rule.h"
#include "rtp_stats_common.h"

static_assert(sizeof(struct rtcp_sess_ext) == 128 &&
	      sizeof(struct rtcp_item) == 32 && sizeof(struct rtcp_desc) == 20 &&
	      sizeof(struct rtp_rx_source) == 18 * 4 + 2 * 8,
	      "layouts of re_rtcp_sess_batch.h");

namespace {

/* the struct rtp_rx_source of the next lane of the group (the last lane:
 * its own) */
__device__ __forceinline__ struct rtp_rx_source
src_from_above(const struct rtp_rx_source &s)
{
	struct rtp_rx_source u;
#define RSX_DOWN(f) u.f = __shfl_down(s.f, 1, RRX_LANES)
	RSX_DOWN(ssrc);
	RSX_DOWN(flags);
	RSX_DOWN(max_seq);
	RSX_DOWN(cycles);
	RSX_DOWN(base_seq);
	RSX_DOWN(bad_seq);
	RSX_DOWN(received);
	RSX_DOWN(expected_prior);
	RSX_DOWN(received_prior);
	RSX_DOWN(transit);
	RSX_DOWN(jitter);
	RSX_DOWN(last_rtp_ts);
	RSX_DOWN(rx_bytes);
	RSX_DOWN(sr_recv);
	RSX_DOWN(sr_ntp_hi);
	RSX_DOWN(sr_ntp_lo);
	RSX_DOWN(sr_rtp_ts);
	RSX_DOWN(sr_psent);
	RSX_DOWN(sr_osent);
	RSX_DOWN(reserved);
#undef RSX_DOWN
	return u;
}

/* the sum / minimum of v over the wave's active lanes */
__device__ __forceinline__ uint32_t wave_add(uint32_t v)
{
#pragma unroll
	for (int o = 32; o; o >>= 1)
		v += __shfl_xor(v, o);
	return v;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
	for (int o = 32; o; o >>= 1) {
		const uint32_t w = __shfl_xor(v, o);
		v = w < v ? w : v;
	}
	return v;
}

} /* namespace */

/* one lane per packet: final stat of those that take no part, key, index */
__global__ void k_rsx_keys(const uint32_t *__restrict__ nmsg, uint32_t maxmsg,
			   const uint32_t *__restrict__ nitem, uint32_t maxitem,
			   const int32_t *__restrict__ res,
			   const uint32_t *__restrict__ sess, uint32_t n,
			   uint32_t nsess, uint32_t *__restrict__ key,
			   uint32_t *__restrict__ idx,
			   int32_t *__restrict__ stat)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const int skip = res && res[i] != 0;
	const uint32_t si = sess ? sess[i] : 0;
	const int st = rsx_packet_stat(skip, si >= nsess, skip ? 0 : nmsg[i],
				       maxmsg, skip ? 0 : nitem[i], maxitem);
	if (key) {
		key[i] = st ? nsess : si;
		idx[i] = i;
	}
	if (stat)
		stat[i] = st;
}

/* eight lanes per session walk its run of decoded packets in order */
__global__ void __launch_bounds__(RRX_BLOCK)
k_rsx_walk(const struct rtcp_desc *__restrict__ descv, uint32_t maxmsg,
	   const uint32_t *__restrict__ nmsg,
	   const struct rtcp_item *__restrict__ itemv, uint32_t maxitem,
	   const uint32_t *__restrict__ nitem, const int32_t *__restrict__ res,
	   const uint32_t *__restrict__ order,
	   const uint32_t *__restrict__ keys, uint32_t n,
	   struct rtp_rx_sess *__restrict__ sessv,
	   struct rtcp_sess_ext *__restrict__ extv, uint32_t nsess,
	   uint64_t recv_ms, uint32_t a_compact, int32_t *__restrict__ stat)
{
	const uint32_t gid = blockIdx.x * RRX_BLOCK + threadIdx.x;
	const uint32_t s = gid / RRX_LANES, slot = gid % RRX_LANES;
	if (s >= nsess)
		return;
	uint32_t lo, hi;
	run_of(keys, n, s, lo, hi);
	if (lo == hi)
		return;

	struct rtp_rx_sess *ss = &sessv[s];
	struct rtcp_sess_ext *xs = &extv[s];
	struct rtp_rx_source src = ss->m[slot];
	struct rsx_mbr mb = {(uint32_t)xs->cum_lost[slot], xs->jit[slot],
			     xs->rtt[slot]};
	const uint32_t srate_tx = xs->srate_tx;
	const uint32_t memberc0 = ss->memberc;
	uint32_t memberc = memberc0;
	bool dirty = false;

	for (uint32_t p = lo; p < hi; p++) {
		const uint32_t i = order ? order[p] : p;
		/* without keys the run holds the packets that take no part */
		if (!keys) {
			const int skip = res && res[i] != 0;
			if (rsx_packet_stat(skip, 0, skip ? 0 : nmsg[i], maxmsg,
					    skip ? 0 : nitem[i], maxitem))
				continue;
		}
		const struct rtcp_desc *d = descv + (size_t)i * maxmsg;
		const struct rtcp_item *it = itemv + (size_t)i * maxitem;
		const uint32_t nm = nmsg[i], ni = nitem[i];
		bool nomember = false;
		uint32_t j = 0;

		for (uint32_t m = 0; m < nm; m++) {
			const uint32_t pt = d[m].pt;
			bool own = false;

			if (rsx_is_report(pt)) {
				const uint32_t ssrc = d[m].ssrc;
				const int hit = rrx_slot_hit(memberc, slot,
							     src.ssrc, ssrc);
				const uint32_t any = group_ballot(hit);
				const int nw = rrx_slot_new(memberc, slot,
							    any != 0);
				const uint32_t anynew = group_ballot(nw);
				if (nw) {
					rrx_member_init(&src, ssrc);
					mb.cum_lost = mb.jit = mb.rtt = 0;
					dirty = true;
				}
				if (anynew)
					memberc++;
				own = hit || nw;
				if (!any && !anynew)
					nomember = true;
			}
			for (; j < ni && it[j].msg == (uint16_t)m; j++) {
				const struct rtcp_item e = it[j];

				if (own && pt == 200 &&
				    e.kind == RTCP_ITEM_SR) {
					rrx_source_sr(&src, recv_ms, e.v[0],
						      e.v[1], e.v[2], e.v[3],
						      e.v[4]);
					dirty = true;
				}
				else if (own && e.kind == RTCP_ITEM_RB) {
					rsx_rr_block(&mb, srate_tx, a_compact,
						     e.v[2], e.v[4], e.v[5],
						     e.v[6]);
					dirty = true;
				}
				else if (pt == 203 &&
					 e.kind == RTCP_ITEM_BYE_SRC) {
					const uint32_t any = group_ballot(
						rrx_slot_hit(memberc, slot,
							     src.ssrc, e.v[0]));
					if (!any)
						continue;
					/* the state of the slot above, to
					 * every lane; then each slot's part */
					const struct rtp_rx_source us =
						src_from_above(src);
					const struct rsx_mbr up = {
						__shfl_down(mb.cum_lost, 1,
							    RRX_LANES),
						__shfl_down(mb.jit, 1, RRX_LANES),
						__shfl_down(mb.rtt, 1, RRX_LANES)};
					const int act = rsx_remove_slot(
						slot, __ffs(any) - 1, memberc);
					if (act == RSX_TAKE_NEXT) {
						src = us;
						mb = up;
						dirty = true;
					}
					else if (act == RSX_ZERO) {
						src = rtp_rx_source{};
						mb.cum_lost = mb.jit = mb.rtt = 0;
						dirty = true;
					}
					memberc--;
				}
			}
		}
		if (nomember && slot == 0 && stat)
			stat[i] = RTP_RX_NOMEMBER;
	}
	if (dirty) {
		ss->m[slot] = src;
		xs->cum_lost[slot] = (int32_t)mb.cum_lost;
		xs->jit[slot] = mb.jit;
		xs->rtt[slot] = mb.rtt;
	}
	if (slot == 0 && memberc != memberc0)
		ss->memberc = memberc;
}

/*
 * The transmit reduction: lane t takes packets t, t + stride, ... (`per` of
 * them; 1 with a session array), the wave's lanes of one session combine,
 * and one lane per distinct session adds to acc[0 .. nsess) (cnt),
 * acc[nsess ..) (sum) and acc[2 * nsess ..) (lowest index).
 */
__global__ void k_rsx_tx(const uint8_t *__restrict__ arena, uint64_t asz,
			 const uint32_t *__restrict__ pos,
			 const uint32_t *__restrict__ end,
			 const int32_t *__restrict__ res,
			 const uint32_t *__restrict__ sess, uint32_t n,
			 uint32_t nsess, uint32_t per,
			 uint32_t *__restrict__ acc, int32_t *__restrict__ stat)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t stride = gridDim.x * blockDim.x;
	struct rsx_tx a = rsx_tx_zero();
	uint32_t key = 0;

	for (uint32_t r = 0; r < per; r++) {
		const uint64_t i64 = (uint64_t)t + (uint64_t)r * stride;
		if (i64 >= n)
			break;
		const uint32_t i = (uint32_t)i64;
		const uint32_t si = sess ? sess[i] : 0;
		uint32_t ts, payload;
		const int st = rsx_tx_packet(arena, asz, pos[i], end[i],
					     res && res[i] != 0, si >= nsess,
					     &ts, &payload);
		if (stat)
			stat[i] = st;
		if (!st) {
			key = si;       /* per > 1: always session 0 */
			a = rsx_tx_combine(a, rsx_tx_one(payload, i));
		}
	}
	/* the lanes that hold something, one session at a time */
	uint64_t todo = __ballot(a.cnt != 0);
	while (todo) {
		const uint32_t k = __shfl(key, __ffsll((long long)todo) - 1);
		const bool mine = a.cnt != 0 && key == k;
		const uint64_t grp = __ballot(mine);
		struct rsx_tx g = mine ? a : rsx_tx_zero();

		if (grp & (grp - 1)) {  /* more than one lane */
			g.cnt = wave_add(g.cnt);
			g.sum = wave_add(g.sum);
			g.first = wave_min(g.first);
		}
		if (mine && (threadIdx.x & 63) == (uint32_t)__ffsll((long long)grp) - 1) {
			atomicAdd(&acc[k], g.cnt);
			atomicAdd(&acc[nsess + k], g.sum);
			atomicMin(&acc[2 * (size_t)nsess + k], g.first);
		}
		todo &= ~grp;
	}
}

/* one lane per session: its accumulator into its state */
__global__ void k_rsx_tx_finish(const uint8_t *__restrict__ arena,
				const uint32_t *__restrict__ pos,
				const uint64_t *__restrict__ jfs_rt,
				const uint32_t *__restrict__ acc,
				struct rtcp_sess_ext *__restrict__ extv,
				uint32_t nsess)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= nsess)
		return;
	const struct rsx_tx t = {acc[s], acc[nsess + s],
				 acc[2 * (size_t)nsess + s]};
	if (!t.cnt)
		return;
	struct rtcp_sess_ext *x = &extv[s];
	if (rsx_tx_finish(x, t))
		/* accepted: its window lies in the arena and holds a header */
		rsx_tx_sync(x, jfs_rt[t.first],
			    rrx_be32(arena + pos[t.first] + 4));
}

/* one lane per session: mk_sr's descriptor from the RR the report wrote */
__global__ void k_rsx_report_msg(struct rtcp_sess_ext *__restrict__ extv,
				 uint32_t nsess, uint64_t now_us,
				 uint32_t ntp_hi, uint32_t ntp_lo,
				 struct rtcp_enc_msg *__restrict__ msgv)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= nsess)
		return;
	struct rtcp_enc_msg m = msgv[s];
	rsx_report_msg(&extv[s], now_us, ntp_hi, ntp_lo, &m);
	msgv[s] = m;
}

/* eight lanes per query: the member by ballot, its lane writes the row */
__global__ void k_rsx_stats(const struct rtp_rx_sess *__restrict__ sessv,
			    const struct rtcp_sess_ext *__restrict__ extv,
			    uint32_t nsess, const uint32_t *__restrict__ sess,
			    const uint32_t *__restrict__ ssrc, uint32_t n,
			    uint32_t *__restrict__ out,
			    int32_t *__restrict__ err)
{
	const uint32_t gid = blockIdx.x * RRX_BLOCK + threadIdx.x;
	const uint32_t q = gid / RRX_LANES, slot = gid % RRX_LANES;
	if (q >= n)
		return;
	const uint32_t si = sess ? sess[q] : 0;
	uint32_t *row = out + (size_t)q * 7;
	if (si >= nsess) {
		if (slot < 7)
			row[slot] = 0;
		if (slot == 0)
			err[q] = EINVAL;
		return;
	}
	const struct rtp_rx_sess *ss = &sessv[si];
	const int hit = rrx_slot_hit(ss->memberc, slot, ss->m[slot].ssrc,
				     ssrc[q]);
	const uint32_t any = group_ballot(hit);
	if (hit) {
		const struct rtp_rx_source src = ss->m[slot];
		rsx_stats_row(&src, &extv[si], slot, row);
		err[q] = 0;
	}
	else if (!any) {
		if (slot < 7)
			row[slot] = 0;
		if (slot == 0)
			err[q] = ENOENT;
	}
}

/* ---- host side ---------------------------------------------------------- */

extern "C" int sgpu_rtcp_rx_handle(const struct rtcp_desc *descv,
				   uint32_t maxmsg, const uint32_t *nmsg,
				   const struct rtcp_item *itemv,
				   uint32_t maxitem, const uint32_t *nitem,
				   const int32_t *res, const uint32_t *sess,
				   uint32_t n, struct rtp_rx_sess *sessv,
				   struct rtcp_sess_ext *extv, uint32_t nsess,
				   uint64_t recv_ms, uint32_t a_compact,
				   int32_t *stat, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	const uint32_t bits = key_bits(nsess);
	uint32_t *kin = NULL, *kout = NULL, *vin = NULL, *vout = NULL;
	struct rrx_scratch *sc = NULL;
	int err = 0;
	std::unique_lock<std::mutex> g(rrx_mu, std::defer_lock);

	if (sess) {
		/* the grouping's four arrays, then the sort's storage */
		const size_t an = al((size_t)n * 4);
		size_t tb = sort_bytes(n, bits);
		g.lock();
		err = rrx_scratch_get(4 * an + al(tb), st, &sc);
		if (err)
			return err;
		uint8_t *b = (uint8_t *)sc->p;
		kin = (uint32_t *)b;
		kout = (uint32_t *)(b + an);
		vin = (uint32_t *)(b + 2 * an);
		vout = (uint32_t *)(b + 3 * an);
		hipLaunchKernelGGL(k_rsx_keys, dim3(blocks(n)), dim3(RRX_BLOCK),
				   0, st, nmsg, maxmsg, nitem, maxitem, res,
				   sess, n, nsess, kin, vin, stat);
		if (rocprim::radix_sort_pairs(b + 4 * an, tb, kin, kout, vin,
					      vout, n, 0, bits, st) !=
		    hipSuccess)
			err = EIO;
	}
	else if (stat) {
		hipLaunchKernelGGL(k_rsx_keys, dim3(blocks(n)), dim3(RRX_BLOCK),
				   0, st, nmsg, maxmsg, nitem, maxitem, res,
				   sess, n, nsess, kin, vin, stat);
	}
	if (!err)
		hipLaunchKernelGGL(k_rsx_walk,
				   dim3(blocks((uint64_t)(sess ? nsess : 1u) *
					       RRX_LANES)),
				   dim3(RRX_BLOCK), 0, st, descv, maxmsg, nmsg,
				   itemv, maxitem, nitem, res, vout, kout, n,
				   sessv, extv, sess ? nsess : 1u, recv_ms,
				   a_compact, stat);
	if (hipGetLastError() != hipSuccess)
		err = EIO;
	if (sc && rrx_scratch_put(sc, st) && !err)
		err = EIO;
	return err;
}

extern "C" int sgpu_rtp_tx_stats(const uint8_t *arena, uint64_t arena_size,
				 const uint32_t *pos, const uint32_t *end,
				 const int32_t *res, const uint32_t *sess,
				 const uint64_t *jfs_rt, uint32_t n,
				 struct rtcp_sess_ext *extv, uint32_t nsess,
				 int32_t *stat, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	/* without a session array: at most 1024 waves, each lane summing its
	 * packets in registers */
	const uint32_t ns = sess ? nsess : 1u;
	const uint32_t nb = sess ? blocks(n)
				 : (blocks(n) < 256u ? blocks(n) : 256u);
	const uint32_t per = sess ? 1u
		: (uint32_t)(((uint64_t)n + (uint64_t)nb * RRX_BLOCK - 1) /
			     ((uint64_t)nb * RRX_BLOCK));
	const size_t an = (size_t)ns * 4;
	std::lock_guard<std::mutex> g(rrx_mu);
	struct rrx_scratch *sc;
	int err = rrx_scratch_get(al(3 * an), st, &sc);
	if (err)
		return err;
	uint32_t *acc = (uint32_t *)sc->p;
	if (hipMemsetAsync(acc, 0, 2 * an, st) != hipSuccess ||
	    hipMemsetAsync(acc + 2 * (size_t)ns, 0xff, an, st) != hipSuccess)
		err = EIO;
	if (!err) {
		hipLaunchKernelGGL(k_rsx_tx, dim3(nb), dim3(RRX_BLOCK), 0, st,
				   arena, arena_size, pos, end, res, sess, n,
				   ns, per, acc, stat);
		hipLaunchKernelGGL(k_rsx_tx_finish, dim3(blocks(ns)),
				   dim3(RRX_BLOCK), 0, st, arena, pos, jfs_rt,
				   acc, extv, ns);
	}
	if (hipGetLastError() != hipSuccess)
		err = EIO;
	if (rrx_scratch_put(sc, st) && !err)
		err = EIO;
	return err;
}

extern "C" int sgpu_rtcp_tx_report(struct rtp_rx_sess *sessv,
				   struct rtcp_sess_ext *extv, uint32_t nsess,
				   uint64_t now_ms, uint64_t now_us,
				   uint32_t ntp_hi, uint32_t ntp_lo,
				   struct rtcp_enc_rb *rbv, uint32_t *nrb,
				   const uint32_t *local_ssrc,
				   struct rtcp_enc_msg *msgv, void *stream)
{
	const int err = sgpu_rtp_rx_report(sessv, nsess, now_ms, rbv, nrb,
					   local_ssrc, msgv, stream);
	if (err)
		return err;
	hipLaunchKernelGGL(k_rsx_report_msg, dim3(blocks(nsess)),
			   dim3(RRX_BLOCK), 0, (hipStream_t)stream, extv, nsess,
			   now_us, ntp_hi, ntp_lo, msgv);
	return hipGetLastError() == hipSuccess ? 0 : EIO;
}

extern "C" int sgpu_rtcp_stats(const struct rtp_rx_sess *sessv,
			       const struct rtcp_sess_ext *extv, uint32_t nsess,
			       const uint32_t *sess, const uint32_t *ssrc,
			       uint32_t n, uint32_t *out, int32_t *err,
			       void *stream)
{
	hipLaunchKernelGGL(k_rsx_stats, dim3(blocks((uint64_t)n * RRX_LANES)),
			   dim3(RRX_BLOCK), 0, (hipStream_t)stream, sessv, extv,
			   nsess, sess, ssrc, n, out, err);
	return hipGetLastError() == hipSuccess ? 0 : EIO;
}
