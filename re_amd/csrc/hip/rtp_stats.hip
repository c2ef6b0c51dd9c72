/*
 * rtp_stats.hip -- RTP receiver statistics for a batch of packets in HBM,
 * up to RTCP report blocks (include/re_rtp_stats_batch.h; the rule:
 * rtp_rx_rule.h).
 *
 * rtp_rx_stats_batch_dev runs in two parts.  The parallel part
 * (k_rrx_record) takes one lane per packet: it checks the window, decodes
 * the header and leaves a 20-byte record, its grouping key (the session; a
 * packet that takes no part gets the key nsess and its final stat at once)
 * and its index.  The A.1 sequence tracker is a state machine and the A.8
 * jitter estimator a non-linear integer recurrence, so the second part
 * (k_rrx_walk) walks each session's packets serially in array order, all
 * sessions in parallel.  The order comes from rocPRIM's radix sort of
 * (key, index) pairs, which is stable; a session finds its run in the
 * sorted keys by binary search.  Without a session array there is one run
 * and no sort.
 *
 * Eight lanes walk a session, lane k holding member slot k in registers:
 * they read the run eight records at a time (one each, the next eight
 * prefetched), pass each record round with a shuffle, find the packet's
 * member by ballot (rrx_slot_hit; the lane at memberc takes a new SSRC,
 * rrx_slot_new), and the one lane that owns the member applies the packet.
 * A group's work depends on its session alone: the result is independent
 * of the grid, and no workgroup waits for another.  The SR and report
 * kernels use the same eight lanes per session.
 *
 * The scratch (records, keys, indices, sort storage) is kept between
 * calls and only grows; an event recorded after its last use orders a call
 * on another stream behind it, on the device.
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>
#include <string.h>
#include "re_rtp_stats_batch.h"
#include "../srtpgpu.h"
#include "rtp_rx_rule.h"
#include "rtp_stats_common.h"

/* one lane per packet: window, header, record, key, index, final stats */
__global__ void k_rrx_record(const uint8_t *__restrict__ arena, uint64_t asz,
			     const uint32_t *__restrict__ pos,
			     const uint32_t *__restrict__ end,
			     const int32_t *__restrict__ res,
			     const uint32_t *__restrict__ sess,
			     const uint32_t *__restrict__ arrival, uint32_t n,
			     uint32_t nsess, struct rrx_rec *__restrict__ rec,
			     uint32_t *__restrict__ key,
			     uint32_t *__restrict__ idx,
			     int32_t *__restrict__ stat)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const uint32_t si = sess ? sess[i] : 0;
	struct rrx_rec r;
	const int st = rrx_record(arena, asz, pos[i], end[i],
				  res && res[i] != 0, si >= nsess,
				  arrival ? arrival[i] : 0, &r);
	rec[i] = r;
	if (key) {
		key[i] = st ? nsess : si;
		idx[i] = i;
	}
	if (st && stat)
		stat[i] = st;
}

/* the grouping key and index of n events (SR) */
__global__ void k_rrx_keys(const uint32_t *__restrict__ sess, uint32_t n,
			   uint32_t nsess, uint32_t *__restrict__ key,
			   uint32_t *__restrict__ idx)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	key[i] = sess[i] < nsess ? sess[i] : nsess;
	idx[i] = i;
}

/* eight lanes per session walk its run of records in order */
__global__ void k_rrx_walk(const struct rrx_rec *__restrict__ rec,
			   const uint32_t *__restrict__ order,
			   const uint32_t *__restrict__ keys, uint32_t n,
			   struct rtp_rx_sess *__restrict__ sessv,
			   uint32_t nsess, int has_arrival,
			   int32_t *__restrict__ stat)
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
	struct rtp_rx_source src = ss->m[slot];
	const uint32_t memberc0 = ss->memberc;
	uint32_t memberc = memberc0;
	bool dirty = false;

	const struct rrx_rec none = {RRX_REC_DROP, 0, 0, 0, 0};
	/* this lane's record of the next eight */
	uint32_t p = lo + slot;
	uint32_t ni = p < hi ? (order ? order[p] : p) : 0;
	struct rrx_rec nr = p < hi ? rec[ni] : none;

	for (uint32_t base = lo; base < hi; base += RRX_LANES) {
		const struct rrx_rec r = nr;
		const uint32_t ri = ni;
		p = base + RRX_LANES + slot;
		ni = p < hi ? (order ? order[p] : p) : 0;
		nr = p < hi ? rec[ni] : none;
#pragma unroll
		for (uint32_t k = 0; k < RRX_LANES; k++) {
			const uint32_t seq_st = __shfl(r.seq_st, k, RRX_LANES);
			const uint32_t ssrc = __shfl(r.ssrc, k, RRX_LANES);
			const uint32_t ts = __shfl(r.ts, k, RRX_LANES);
			const uint32_t arr = __shfl(r.arrival, k, RRX_LANES);
			const uint32_t pay = __shfl(r.payload, k, RRX_LANES);
			const uint32_t i = __shfl(ri, k, RRX_LANES);
			const bool live = !(seq_st & RRX_REC_DROP);
			const int hit = live &&
				rrx_slot_hit(memberc, slot, src.ssrc, ssrc);
			const uint32_t any = group_ballot(hit);
			const int nw = live &&
				rrx_slot_new(memberc, slot, any != 0);
			const uint32_t anynew = group_ballot(nw);
			if (nw)
				rrx_member_init(&src, ssrc);
			if (anynew)
				memberc++;
			if (hit || nw) {
				const int ok = rrx_source_rx(&src, seq_st, ts,
							     arr, has_arrival,
							     pay);
				dirty = true;
				if (stat)
					stat[i] = ok ? 0 : RTP_RX_BADSEQ;
			}
			else if (live && !any && !anynew && slot == 0 && stat) {
				stat[i] = RTP_RX_NOMEMBER;
			}
		}
	}
	if (dirty)
		ss->m[slot] = src;
	if (slot == 0 && memberc != memberc0)
		ss->memberc = memberc;
}

/* eight lanes per session apply its run of sender reports in order */
__global__ void k_rrx_sr(struct rtp_rx_sess *__restrict__ sessv,
			 uint32_t nsess, const uint32_t *__restrict__ order,
			 const uint32_t *__restrict__ keys,
			 const uint32_t *__restrict__ ssrc,
			 const uint32_t *__restrict__ ntp_sec,
			 const uint32_t *__restrict__ ntp_frac,
			 const uint32_t *__restrict__ rtp_ts,
			 const uint32_t *__restrict__ psent,
			 const uint32_t *__restrict__ osent, uint64_t recv_ms,
			 uint32_t n)
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
	struct rtp_rx_source src = ss->m[slot];
	const uint32_t memberc0 = ss->memberc;
	uint32_t memberc = memberc0;
	bool dirty = false;

	for (uint32_t p = lo; p < hi; p++) {
		const uint32_t i = order ? order[p] : p;
		const uint32_t e = ssrc[i];
		const int hit = rrx_slot_hit(memberc, slot, src.ssrc, e);
		const uint32_t any = group_ballot(hit);
		const int nw = rrx_slot_new(memberc, slot, any != 0);
		const uint32_t anynew = group_ballot(nw);
		if (nw)
			rrx_member_init(&src, e);
		if (anynew)
			memberc++;
		if (hit || nw) {
			rrx_source_sr(&src, recv_ms, ntp_sec[i], ntp_frac[i],
				      rtp_ts[i], psent[i], osent[i]);
			dirty = true;
		}
	}
	if (dirty)
		ss->m[slot] = src;
	if (slot == 0 && memberc != memberc0)
		ss->memberc = memberc;
}

/* eight lanes per session: each member's report block, in hash order */
__global__ void k_rrx_report(struct rtp_rx_sess *__restrict__ sessv,
			     uint32_t nsess, uint64_t now_ms,
			     struct rtcp_enc_rb *__restrict__ rbv,
			     uint32_t *__restrict__ nrb,
			     const uint32_t *__restrict__ local_ssrc,
			     struct rtcp_enc_msg *__restrict__ rr_msgv)
{
	const uint32_t gid = blockIdx.x * RRX_BLOCK + threadIdx.x;
	const uint32_t s = gid / RRX_LANES, slot = gid % RRX_LANES;
	if (s >= nsess)
		return;
	struct rtp_rx_sess *ss = &sessv[s];
	struct rtp_rx_source src = ss->m[slot];
	const uint32_t key = rrx_report_key(&src, slot, ss->memberc);
	/* rank among the reports; a lane without one zeroes a spare entry */
	uint32_t before = 0, cnt = 0, spare = 0;
#pragma unroll
	for (uint32_t k = 0; k < RRX_LANES; k++) {
		const uint32_t kk = __shfl(key, k, RRX_LANES);
		before += kk < key;
		cnt += kk != RRX_NOKEY;
		spare += kk == RRX_NOKEY && k < slot;
	}
	struct rtcp_enc_rb rb = {0, 0, 0, 0, 0, 0, 0};
	struct rtcp_enc_rb *out = rbv + (size_t)s * RRX_LANES;
	if (key != RRX_NOKEY) {
		rrx_report_block(&src, now_ms, &rb);
		ss->m[slot].expected_prior = src.expected_prior;
		ss->m[slot].received_prior = src.received_prior;
		out[before] = rb;
	}
	else {
		out[cnt + spare] = rb;
	}
	if (slot == 0) {
		nrb[s] = cnt;
		if (rr_msgv) {
			struct rtcp_enc_msg m = {};
			m.pt = 201;
			m.count = (uint8_t)cnt;
			m.w[0] = local_ssrc[s];
			m.first = s * RRX_LANES;
			m.num = cnt;
			rr_msgv[s] = m;
		}
	}
}

/* ---- host side ---------------------------------------------------------- */

std::mutex rrx_mu;
static struct rrx_scratch g_scr[16];

/* with rrx_mu held: >= bytes of scratch, ordered behind its last use */
int rrx_scratch_get(size_t bytes, hipStream_t st, struct rrx_scratch **sp)
{
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16)
		return EIO;
	struct rrx_scratch *sc = &g_scr[dev];
	if (!sc->ev &&
	    hipEventCreateWithFlags(&sc->ev, hipEventDisableTiming) != hipSuccess)
		return EIO;
	if (sc->size < bytes) {
		/* hipFree waits for the work that still uses the old one */
		if (sc->p)
			(void)hipFree(sc->p);
		sc->p = NULL;
		sc->size = 0;
		sc->used = false;
		if (hipMalloc(&sc->p, bytes) != hipSuccess) {
			sc->p = NULL;
			(void)hipGetLastError();
			return ENOMEM;
		}
		sc->size = bytes;
	}
	if (sc->used && hipStreamWaitEvent(st, sc->ev, 0) != hipSuccess)
		return EIO;
	*sp = sc;
	return 0;
}

int rrx_scratch_put(struct rrx_scratch *sc, hipStream_t st)
{
	sc->used = true;
	return hipEventRecord(sc->ev, st) == hipSuccess ? 0 : EIO;
}

namespace {

/* the scratch of a call over n items: records (stats only), then the
 * grouping's four arrays and the sort's storage */
struct layout {
	size_t o_rec, o_kin, o_kout, o_vin, o_vout, o_tmp, tmp, total;
};

struct layout lay(uint32_t n, bool recs, bool group, uint32_t bits)
{
	struct layout l = {};
	size_t o = 0;
	l.o_rec = o;
	o += recs ? al((size_t)n * sizeof(struct rrx_rec)) : 0;
	if (group) {
		l.o_kin = o;
		o += al((size_t)n * 4);
		l.o_kout = o;
		o += al((size_t)n * 4);
		l.o_vin = o;
		o += al((size_t)n * 4);
		l.o_vout = o;
		o += al((size_t)n * 4);
		l.o_tmp = o;
		l.tmp = sort_bytes(n, bits);
		o += al(l.tmp);
	}
	l.total = o ? o : 256;
	return l;
}

} /* namespace */

extern "C" int sgpu_rtp_rx_stats(const uint8_t *arena, uint64_t arena_size,
				 const uint32_t *pos, const uint32_t *end,
				 const int32_t *res, const uint32_t *sess,
				 const uint32_t *arrival, uint32_t n,
				 struct rtp_rx_sess *sessv, uint32_t nsess,
				 int32_t *stat, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	const uint32_t bits = key_bits(nsess);
	const struct layout l = lay(n, true, sess != NULL, bits);
	std::lock_guard<std::mutex> g(rrx_mu);
	struct rrx_scratch *sc;
	int err = rrx_scratch_get(l.total, st, &sc);
	if (err)
		return err;
	uint8_t *b = (uint8_t *)sc->p;
	struct rrx_rec *rec = (struct rrx_rec *)(b + l.o_rec);
	uint32_t *kin = NULL, *kout = NULL, *vin = NULL, *vout = NULL;
	if (sess) {
		kin = (uint32_t *)(b + l.o_kin);
		kout = (uint32_t *)(b + l.o_kout);
		vin = (uint32_t *)(b + l.o_vin);
		vout = (uint32_t *)(b + l.o_vout);
	}
	hipLaunchKernelGGL(k_rrx_record, dim3(blocks(n)), dim3(RRX_BLOCK), 0,
			   st, arena, arena_size, pos, end, res, sess, arrival,
			   n, nsess, rec, kin, vin, stat);
	if (sess) {
		size_t tb = l.tmp;
		if (rocprim::radix_sort_pairs(b + l.o_tmp, tb, kin, kout, vin,
					      vout, n, 0, bits, st) !=
		    hipSuccess)
			err = EIO;
	}
	if (!err)
		hipLaunchKernelGGL(k_rrx_walk,
				   dim3(blocks((uint64_t)(sess ? nsess : 1u) *
					       RRX_LANES)),
				   dim3(RRX_BLOCK), 0, st, rec, vout, kout, n,
				   sessv, sess ? nsess : 1u, arrival != NULL,
				   stat);
	if (hipGetLastError() != hipSuccess)
		err = EIO;
	if (rrx_scratch_put(sc, st) && !err)
		err = EIO;
	return err;
}

extern "C" int sgpu_rtp_rx_sr(struct rtp_rx_sess *sessv, uint32_t nsess,
			      const uint32_t *sess, const uint32_t *ssrc,
			      const uint32_t *ntp_sec, const uint32_t *ntp_frac,
			      const uint32_t *rtp_ts, const uint32_t *psent,
			      const uint32_t *osent, uint64_t recv_ms,
			      uint32_t n, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	const uint32_t bits = key_bits(nsess);
	uint32_t *kout = NULL, *vout = NULL;
	struct rrx_scratch *sc = NULL;
	int err = 0;
	std::unique_lock<std::mutex> g(rrx_mu, std::defer_lock);
	if (sess) {
		const struct layout l = lay(n, false, true, bits);
		g.lock();
		err = rrx_scratch_get(l.total, st, &sc);
		if (err)
			return err;
		uint8_t *b = (uint8_t *)sc->p;
		uint32_t *kin = (uint32_t *)(b + l.o_kin);
		uint32_t *vin = (uint32_t *)(b + l.o_vin);
		size_t tb = l.tmp;
		kout = (uint32_t *)(b + l.o_kout);
		vout = (uint32_t *)(b + l.o_vout);
		hipLaunchKernelGGL(k_rrx_keys, dim3(blocks(n)), dim3(RRX_BLOCK),
				   0, st, sess, n, nsess, kin, vin);
		if (rocprim::radix_sort_pairs(b + l.o_tmp, tb, kin, kout, vin,
					      vout, n, 0, bits, st) !=
		    hipSuccess)
			err = EIO;
	}
	if (!err)
		hipLaunchKernelGGL(k_rrx_sr,
				   dim3(blocks((uint64_t)(sess ? nsess : 1u) *
					       RRX_LANES)),
				   dim3(RRX_BLOCK), 0, st, sessv,
				   sess ? nsess : 1u, vout, kout, ssrc, ntp_sec,
				   ntp_frac, rtp_ts, psent, osent, recv_ms, n);
	if (hipGetLastError() != hipSuccess)
		err = EIO;
	if (sc && rrx_scratch_put(sc, st) && !err)
		err = EIO;
	return err;
}

extern "C" int sgpu_rtp_rx_report(struct rtp_rx_sess *sessv, uint32_t nsess,
				  uint64_t now_ms, struct rtcp_enc_rb *rbv,
				  uint32_t *nrb, const uint32_t *local_ssrc,
				  struct rtcp_enc_msg *rr_msgv, void *stream)
{
	hipLaunchKernelGGL(k_rrx_report,
			   dim3(blocks((uint64_t)nsess * RRX_LANES)),
			   dim3(RRX_BLOCK), 0, (hipStream_t)stream, sessv, nsess,
			   now_ms, rbv, nrb, local_ssrc, rr_msgv);
	return hipGetLastError() == hipSuccess ? 0 : EIO;
}
