/*
 * plan_rx_rule.h -- the exact receive-side index and replay rule for ONE
 * RTP stream whose packets arrive reordered, duplicated or with gaps
 * (srtp_decrypt: src/srtp/srtp.c:313-323, 367, 421, 426-427; srtp_get_index
 * misc.c:22-41; srtp_replay_check replay.c:32-62), in the form a parallel
 * planner needs: speculate, then verify every packet with the reference's
 * own step.  Compiles as C (the host twin srtp_rx_plan_host, batch_dev.c)
 * and as HIP device code (plan_rx.hip); both run the same functions.
 *
 * State: the receiver's (roc, s_l) as one number H = roc * 65536 + s_l.
 *
 *   speculate  u[0] = step(H0, seq[0]);  u[i] = u[i-1] + sdiff16(seq[i],
 *              seq[i-1]) -- a 64-bit prefix sum -- and Mx[i] = max(u[0..i)),
 *              an exclusive prefix maximum.  Both scan under the one
 *              associative operator rx_combine on (sum, max) pairs.
 *   verify     the receiver's state before packet i is M = max(H0, Mx[i])
 *              if every packet before it was settled (an accepted packet
 *              leaves max(M, u), an EALREADY one below M leaves M); the
 *              reference step from M must give exactly u[i] (rx_step).
 *   replay     its window's top is L = max(lix0, Mx[i]); below it a packet
 *              is a duplicate if the pre-batch bitmap or one of the K
 *              arrivals before it holds its index, and new if nothing
 *              older than those K can (rx_replay).
 *
 * By induction over i a batch whose every packet verifies is exactly what
 * the reference receiver computes; anything else is unsettled and the
 * whole batch is planned sequentially instead.
 */
#ifndef PLAN_RX_RULE_H
#define PLAN_RX_RULE_H

#include <stdint.h>

#ifdef __HIPCC__
#define RX_FN __host__ __device__ static inline
#else
#define RX_FN static inline
#endif

#define RX_NEG (-((int64_t)1 << 62))    /* "no packet yet" for a maximum */
#define RX_LOOKBACK 128u                /* arrivals searched for a copy */

/* per-packet verdicts */
enum {
	RX_OK = 0,              /* accepted */
	RX_DUP = 1,             /* EALREADY */
	RX_UNSETTLED = 2,       /* the rule cannot tell: plan sequentially */
};

/* (sum of the differences, maximum of their inclusive prefix sums) */
struct rx_agg {
	int64_t s, m;
};

RX_FN int64_t rx_max(int64_t a, int64_t b)
{
	return a > b ? a : b;
}

RX_FN struct rx_agg rx_identity(void)
{
	struct rx_agg r;
	r.s = 0;
	r.m = RX_NEG;
	return r;
}

/* one packet's element: its difference d (packet 0: u[0] itself) */
RX_FN struct rx_agg rx_elem(int64_t d)
{
	struct rx_agg r;
	r.s = d;
	r.m = d;
	return r;
}

/* a then b: associative, not commutative; rx_identity() on either side */
RX_FN struct rx_agg rx_combine(struct rx_agg a, struct rx_agg b)
{
	struct rx_agg r;
	r.s = a.s + b.s;
	r.m = b.m <= RX_NEG / 2 ? a.m : rx_max(a.m, a.s + b.m);
	return r;
}

/*
 * Many streams in one scan (plan_buckets_rx.hip: the packets of a bucket
 * sorted by session): an element carries a segment-head flag beside its
 * pair.  A head on the right operand restarts the sum and the maximum, so
 * the inclusive scan of position k holds its own stream's pair only and
 * u[] / Mx[] restart at each stream's first packet (a head's element: its
 * u[0] itself, as packet 0's above).
 */
struct rx_seg {
	struct rx_agg a;
	uint32_t head;          /* a stream's first packet lies in the range */
};

RX_FN struct rx_seg rx_seg_identity(void)
{
	struct rx_seg r;
	r.a = rx_identity();
	r.head = 0;
	return r;
}

RX_FN struct rx_seg rx_seg_elem(int64_t d, int head)
{
	struct rx_seg r;
	r.a = rx_elem(d);
	r.head = head ? 1u : 0u;
	return r;
}

/* a then b: associative; rx_seg_identity() on either side */
RX_FN struct rx_seg rx_seg_combine(struct rx_seg a, struct rx_seg b)
{
	struct rx_seg r;
	if (b.head)
		return b;
	r.a = rx_combine(a.a, b.a);
	r.head = a.head;
	return r;
}

/* the exclusive prefix maximum of a position from the scan's exclusive
 * value before it: nothing for a stream's first packet */
RX_FN int64_t rx_seg_mx(struct rx_seg excl, int head)
{
	return head ? RX_NEG : excl.a.m;
}

/* seq - prev as the nearest signed distance, in (-32768, 32768] */
RX_FN int64_t rx_sdiff16(uint32_t seq, uint32_t prev)
{
	const int32_t d = (int32_t)((seq - prev) & 0xffffu);
	return d > 32768 ? d - 65536 : d;
}

/* srtp_get_index (misc.c:22-41), including the int wrap of roc +- 1 */
RX_FN int32_t rx_v(uint32_t roc, uint32_t s_l, uint32_t seq)
{
	if (s_l < 32768)
		return ((int)seq - (int)s_l > 32768) ? (int32_t)(roc - 1)
						     : (int32_t)roc;
	return ((int)s_l - 32768 > (int)seq) ? (int32_t)(roc + 1)
					     : (int32_t)roc;
}

/*
 * The reference receiver's step (srtp.c:313-323) from state M with a
 * packet of sequence number seq: 0 with *u = its 48-bit index and *bump =
 * it rolled the ROC over (roc + 1, s_l = 0: srtp.c:318-321), or -1 for
 * ETIMEDOUT.  (After the ETIMEDOUT test and the rollover srtp_get_index
 * always answers the stream's own ROC -- its roc - 1 branch needs
 * seq - s_l > 32768, its roc + 1 branch seq - s_l < -32768 -- so a
 * different answer is treated as ETIMEDOUT is: not settled here.)
 *
 * srtp_get_index holds that ROC in an int and widens it to the 64-bit index
 * (misc.c:24, 40): from ROC 2^31 on the index the replay window stores is
 * sign-extended, 0xffff8000_0000_0000 and above.  A step that leaves the ROC
 * there -- a stream taken over at such a ROC, the rollover that crosses
 * 2^31, the one behind 2^32 - 1 (the uint32_t ROC is 0 again, the window's
 * top stays near 2^64) -- is not settled either: H, u[] and the window live
 * in the signed 48-bit domain below it, and the batch is planned
 * sequentially with the reference's own arithmetic.
 */
RX_FN int rx_step(int64_t M, uint32_t seq, int64_t *u, int *bump)
{
	uint32_t roc = (uint32_t)((uint64_t)M >> 16);
	uint32_t s_l = (uint32_t)((uint64_t)M & 0xffffu);
	const int diff = (int)seq - (int)s_l;
	if (M < 0 || diff > 32768)
		return -1;
	*bump = diff <= -32768;
	if (*bump) {
		roc++;
		s_l = 0;
	}
	if (roc >> 31 || (*bump && !roc))
		return -1;
	if ((uint32_t)rx_v(roc, s_l, seq) != roc)
		return -1;
	*u = (int64_t)(((uint64_t)roc << 16) | (seq & 0xffffu));
	return 0;
}

/*
 * Replay verdict of packet i (replay.c:32-62) from the speculated indices
 * u[], their exclusive prefix maxima mx[] and the window before the batch
 * (lix0, bitmap0); K: how many arrivals before i are searched for a copy.
 * Reads u[max(i - K, 0) .. i] and mx[i], mx[i - K].
 *
 * tagged: every packet's tag is verified behind the plan, EALREADY ones
 * included (the device: a miss sends the batch to the host).  A packet 64
 * or more below the top is EALREADY whatever it is -- if its tag verifies
 * at u[i] (srtp.c:358-359 and 408-411 come before the replay check).  Such
 * a verdict with no copy of the packet in sight rests on that tag alone (a
 * forward jump of more than 32768 looks exactly like it, and the reference
 * answers EAUTH there), so without tags (the host twin) it is unsettled.
 */
RX_FN int rx_replay(const int64_t *u, const int64_t *mx, uint32_t i,
		    uint32_t K, int64_t lix0, uint64_t bitmap0, int tagged)
{
	const int64_t ui = u[i], L = rx_max(lix0, mx[i]);
	const uint32_t lo = i > K ? i - K : 0u;
	const int far = ui <= L && L - ui >= 64;
	uint32_t j;
	if (ui > L)
		return RX_OK;
	if (far && tagged)
		return RX_DUP;
	if (ui <= lix0 && lix0 - ui < 64 && ((bitmap0 >> (lix0 - ui)) & 1u))
		return RX_DUP;
	for (j = lo; j < i; j++)
		if (u[j] == ui)
			return RX_DUP;
	if (far)
		return RX_UNSETTLED;
	/* no copy among the K before it; none can be older if every older
	 * index (and the window before the batch) lies below it */
	if (i <= K || rx_max(lix0, mx[i - K]) < ui)
		return RX_OK;
	return RX_UNSETTLED;
}

/*
 * Packet i settled: RX_OK / RX_DUP are the reference's 0 / EALREADY and
 * u[i] the index it authenticates at.  An EALREADY packet must leave the
 * state as the speculation assumes: one that rolled the ROC over (the
 * reference keeps roc + 1, s_l = 0) or lies above M is unsettled.  So is
 * every packet of a stream whose window before the batch holds a
 * sign-extended index (lix0 of 2^62 or more as an unsigned number: the
 * reference's own from ROC 2^31 on, and still there behind 2^32 when the
 * ROC is small again): the maxima here are signed.
 */
RX_FN int rx_settle(const int64_t *u, const int64_t *mx, uint32_t i,
		    uint32_t seq, uint32_t K, int64_t H0, int64_t lix0,
		    uint64_t bitmap0, int tagged)
{
	const int64_t M = rx_max(H0, mx[i]);
	int64_t v = 0;
	int bump = 0, r;
	if ((uint64_t)lix0 >> 62 || rx_step(M, seq, &v, &bump) || v != u[i])
		return RX_UNSETTLED;
	r = rx_replay(u, mx, i, K, lix0, bitmap0, tagged);
	if (r == RX_DUP && (bump || u[i] > M))
		return RX_UNSETTLED;
	return r;
}

/* the replay bitmap after the batch, before the accepted packets' bits
 * (rx_bit) are ORed in: the old window moved up to the new top */
RX_FN uint64_t rx_bitmap_base(int64_t lix, int64_t lix0, uint64_t bitmap0)
{
	return lix - lix0 < 64 ? bitmap0 << (lix - lix0) : 0u;
}

/* an accepted packet's bit in the final window (0: it has left it) */
RX_FN uint64_t rx_bit(int64_t lix, int64_t ui)
{
	return lix - ui < 64 ? (uint64_t)1 << (lix - ui) : 0u;
}

#endif
